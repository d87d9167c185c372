// detect_shared.h — device code shared by the offline detector (detect.hip), the streaming step (stream.hip) and the decoder
// sweep (tune.hip): the stitch of one (output frame, class) cell, the exclusive scan of per-(segment, class) event counts, the
// median by selection and the edge walk of the event decoder.  The files call the SAME functions, so a streamed track row is
// bit for bit the row sed_detect_stitch writes, and the events a sweep scores are the events sed_detect_events_batch writes.
#pragma once
#include "common.h"

// 64-bit words of one bit track of n_out frames: the extra word holds the fall edge of a run that reaches the end
static inline long detect_words(long n_out) { return n_out / 64 + 1; }

// last r with off[r] <= x (off[0] = 0 <= x, off ascending)
__device__ __forceinline__ int find_seg(const int* __restrict__ off, int R, long x) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// median of the M frames around j of class k, edges 'nearest'; a selection (exact, ties included)
template <int M>
__device__ __forceinline__ float median_nearest(const float* __restrict__ probs, int j, int k, int K, int n_out) {
    if (M == 1) return probs[(size_t)j * K + k];
    float v[M];
#pragma unroll
    for (int d = 0; d < M; ++d) {
        int t = j + d - M / 2;
        t = t < 0 ? 0 : (t >= n_out ? n_out - 1 : t);
        v[d] = probs[(size_t)t * K + k];
    }
    float med = v[0];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        int less = 0, leq = 0;
#pragma unroll
        for (int d = 0; d < M; ++d) { less += v[d] < v[i]; leq += v[d] <= v[i]; }
        if (less <= M / 2 && M / 2 < leq) med = v[i];                 // v[i] is the (M/2)-th smallest
    }
    return med;
}

// The edge walk of the event decoder, run by ONE wave over the two bit tracks of one (recording, class): ob = p' > lo,
// hb = p' > hi, n_words 64-bit words each.  64-word chunks: edges from on ^ (on << 1), the number of high bits before every
// edge from a wave scan of popcounts, so a run [a, b) is kept iff H(b) - H(a) > 0; lane 0 then walks the chunk's edge list with
// the carried state (open run, pending event) to merge across gaps of <= min_gap frames and drop events shorter than min_len.
// emit(onset, offset) is called by lane 0 for every finished event, in increasing onset.  epos / eh: DETECT_EDGE_CAP ints of
// LDS each; the workgroup is the one wave (the barriers are the wave's own).
#define DETECT_EDGE_CAP 4096                                      // 64 words x 64 bits: every edge of a chunk
template <class Emit>
__device__ __forceinline__ void detect_walk_body(const unsigned long long* __restrict__ ob, const unsigned long long* __restrict__ hb,
                                                 long n_words, int min_gap, int min_len, int* epos, int* eh, Emit& emit) {
    const int lane = threadIdx.x;
    unsigned carry_top = 0;                      // bit 63 of the previous chunk's last word
    long hbase = 0;                              // high bits before this chunk
    // lane 0's walk state
    bool open = false, have = false;
    int r_on = 0, p_on = 0, p_off = 0;
    long r_h = 0;
    for (long w0 = 0; w0 < n_words; w0 += 64) {
        const long w = w0 + lane;
        const unsigned long long on = w < n_words ? ob[w] : 0ull, hi = w < n_words ? hb[w] : 0ull;
        unsigned prev = __shfl((unsigned)(on >> 63), (lane + 63) & 63, 64);
        if (lane == 0) prev = carry_top;
        const unsigned long long sh = (on << 1) | prev;
        const unsigned long long edges = on ^ sh;                // rises (on & ~sh) and falls (~on & sh) alternate globally
        int hc = __popcll(hi), ne = __popcll(edges);
        int hpre = hc, epre = ne;                                // inclusive wave scans
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(hpre, o, 64), b = __shfl_up(epre, o, 64);
            if (lane >= o) { hpre += a; epre += b; }
        }
        const int n_edges = __shfl(epre, 63, 64), n_high = __shfl(hpre, 63, 64);
        hpre -= hc;
        epre -= ne;
        for (unsigned long long m = edges; m; m &= m - 1) {
            const int b = __ffsll((long long)m) - 1;
            epos[epre] = (int)(w * 64 + b);
            eh[epre] = (int)(hbase + hpre + __popcll(hi & ((1ull << b) - 1ull)));
            ++epre;
        }
        __syncthreads();
        if (lane == 0) {
            for (int e = 0; e < n_edges; ++e) {
                if (!open) { open = true; r_on = epos[e]; r_h = eh[e]; continue; }
                open = false;
                const int r_off = epos[e];
                if (eh[e] - r_h <= 0) continue;                  // no frame of the run above hi
                if (have && r_on - p_off <= min_gap) { p_off = r_off; continue; }
                if (have && p_off - p_on >= min_len) emit(p_on, p_off);
                have = true; p_on = r_on; p_off = r_off;
            }
        }
        __syncthreads();
        carry_top = (unsigned)__shfl((unsigned)(on >> 63), 63, 64);
        hbase += n_high;
    }
    if (lane == 0 && have && p_off - p_on >= min_len) emit(p_on, p_off);
}

// where the logits of window w, output row `row` (of win_out), class 0 live: the offline paths keep every window back to back
struct LinearLogits {
    const float* base; int win_out, K;
    __device__ __forceinline__ const float* at(int w, int row) const { return base + ((size_t)w * win_out + row) * K; }
};

// One (output frame j, class k): the covering windows are a contiguous range of w (start(w) = min(w hop_out, last_start) is
// strictly increasing); they are visited in increasing w, so the sum has one fixed order (bitwise deterministic, no atomics).
template <class Logits>
__device__ __forceinline__ float stitch_one(const Logits& logits, int n_win, int win_out, int hop_out, int last_start, int n_out,
                                            int combine, int trim, int j, int k) {
    // last window whose start is <= j
    int whi = j >= last_start ? n_win - 1 : j / hop_out;
    if (whi > n_win - 1) whi = n_win - 1;
    int wlo = whi;
    while (wlo > 0) {                                                // first window that still reaches j
        const long s = (long)(wlo - 1) * hop_out < last_start ? (long)(wlo - 1) * hop_out : last_start;
        if (s + win_out <= j) break;
        --wlo;
    }
    float acc = combine ? -INFINITY : 0.f;
    int cnt = 0;
    for (int w = wlo; w <= whi; ++w) {
        const long s = (long)w * hop_out < last_start ? (long)w * hop_out : last_start;
        const long lo = s + (s > 0 ? trim : 0);
        const long hi = s + win_out - (s + win_out < n_out ? trim : 0);
        if (j < lo || j >= hi) continue;
        const float x = logits.at(w, (int)(j - s))[k];
        const float p = 1.0f / (1.0f + expf(-x));
        if (combine) acc = fmaxf(acc, p);
        else acc += p;
        ++cnt;
    }
    return combine ? acc : acc / (float)cnt;                          // cnt >= 1: the host checked coverage
}

// exclusive scan of the n = R*K counts by one workgroup (wave scans + the 16 wave totals, 1 024 counts per step) ->
// offsets [R*K]; event_off [R+1] = the offset of each segment's first class, and the total
static __global__ __launch_bounds__(1024) void detect_scan_k(const int* __restrict__ counts, int n, int K, int* __restrict__ offsets,
                                                             int* __restrict__ event_off) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const int c = i < n ? counts[i] : 0;
        int x = c;                                                    // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int pre = 0, step = 0;
        for (int w = 0; w < 16; ++w) {
            pre += w < wv ? wsum[w] : 0;
            step += wsum[w];
        }
        const int excl = carry + pre + x - c;
        if (i < n) {
            offsets[i] = excl;
            if (i % K == 0) event_off[i / K] = excl;
        }
        carry += step;
        __syncthreads();                                              // wsum is rewritten by the next step
    }
    if (tid == 0) event_off[n / K] = carry;
}
