// detect.hip — whole-recording event detection (sed_crnn_amd/detect.py): the per-window outputs of the eval
// forward stitched into one probability track, and that track turned into (class, onset, offset, peak) events.
//
// Frame arithmetic (output frames, tf input frames each): window w covers [start(w), start(w) + win_out) with
// start(w) = min(w * hop_out, last_start_out) — the regular grid 0, hop, 2 hop, ... plus, where the last regular window stops
// short of the end, one extra window aligned to the end (last_start_out + win_out == n_out).  The host planner builds that grid.
#include "common.h"

// ───────────────────────── stitch: sigmoid, then mean / max over the covering windows ─────────────────────────
// One thread per (output frame, class): the covering windows are a contiguous range of w (start(w) is strictly increasing);
// they are visited in increasing w, so the sum has one fixed order (bitwise deterministic, no atomics).
__global__ __launch_bounds__(256) void detect_stitch_k(const float* __restrict__ logits, int n_win, int win_out, int K,
                                                       int hop_out, int last_start, int n_out, int combine, int trim,
                                                       float* __restrict__ probs) {
    const long total = (long)n_out * K;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i / K), k = (int)(i - (long)j * K);
        // last window whose start is <= j
        int whi = j >= last_start ? n_win - 1 : j / hop_out;
        if (whi > n_win - 1) whi = n_win - 1;
        int wlo = whi;
        while (wlo > 0) {                                            // first window that still reaches j
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
            const float x = logits[((size_t)w * win_out + (j - s)) * K + k];
            const float p = 1.0f / (1.0f + expf(-x));
            if (combine) acc = fmaxf(acc, p);
            else acc += p;
            ++cnt;
        }
        probs[i] = combine ? acc : acc / (float)cnt;                  // cnt >= 1: the host checked coverage
    }
}

extern "C" int sed_detect_stitch(const float* logits, long n_win, int win_out, int K, int hop_out, long last_start_out,
                                 long n_out, int combine, int trim, float* probs, void* stream) {
    SED_REQUIRE(logits && probs, "detect_stitch: null pointer");
    SED_REQUIRE(n_win >= 1 && win_out >= 1 && K >= 1 && hop_out >= 1 && last_start_out >= 0 && n_out >= 1 &&
                    n_out <= 0x7fffffffL && n_win <= 0x7fffffffL && (long)n_out * K <= 0x7fffffffL,
                "detect_stitch: bad sizes (n_win=%ld, win_out=%d, K=%d, hop_out=%d, n_out=%ld)", n_win, win_out, K, hop_out, n_out);
    SED_REQUIRE(combine == 0 || combine == 1, "detect_stitch: combine must be 0 (mean) or 1 (max), got %d", combine);
    SED_REQUIRE(last_start_out + win_out == n_out, "detect_stitch: the last window must end at the recording's end");
    // start(w) = min(w hop, last): the last window starts at `last`, every earlier one strictly before it
    SED_REQUIRE((n_win - 1) * (long)hop_out >= last_start_out && (n_win < 2 || (n_win - 2) * (long)hop_out < last_start_out),
                "detect_stitch: last_start_out=%ld is not the last start of a %ld-window grid with hop %d", last_start_out, n_win, hop_out);
    SED_REQUIRE(trim >= 0 && (n_win == 1 || hop_out + 2L * trim <= win_out),
                "detect_stitch: trim=%d leaves output frames uncovered (hop_out=%d, win_out=%d)", trim, hop_out, win_out);
    const long total = n_out * K;
    long nb = (total + 255) / 256;
    detect_stitch_k<<<(unsigned)(nb < 8192 ? nb : 8192), 256, 0, as_stream(stream)>>>(
        logits, (int)n_win, win_out, K, hop_out, (int)last_start_out, (int)n_out, combine, trim, probs);
    SED_LAUNCH_CHECK("detect_stitch");
    return 0;
}

// ───────────────────────── events ─────────────────────────
// Phase 1 (all frames in parallel): median filter (a selection: exact), then two bit tracks per class packed by __ballot —
// on = p' > lo and high = p' > hi — as 64-bit words [K][n_words], n_words = n_out/64 + 1 (the extra word holds the fall edge
// of a run that reaches the end).  Phase 2 (one wave per class walking 64-word chunks): edges from the words, the number of
// high bits before every edge from a wave scan of popcounts, so a run [a, b) is kept iff H(b) - H(a) > 0; lane 0 then walks the
// chunk's edge list with the carried state (open run, pending event) to merge and drop.  Run once to count, a one-thread scan
// turns the counts into per-class offsets, run again to write.  Phase 3: peak / first arg-max of the unfiltered track.
static inline long detect_words(long n_out) { return n_out / 64 + 1; }

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

template <int M>
__global__ __launch_bounds__(256) void detect_bits_k(const float* __restrict__ probs, int n_out, int K, long n_words, float lo,
                                                     float hi, unsigned long long* __restrict__ on_bits,
                                                     unsigned long long* __restrict__ hi_bits) {
    const int k = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    bool on = false, high = false;
    if (j < n_out) {
        const float p = median_nearest<M>(probs, (int)j, k, K, n_out);
        on = p > lo;
        high = p > hi;
    }
    const unsigned long long bo = __ballot(on), bh = __ballot(high);      // wave64: bit l = frame (j - lane + l)
    const long w = j >> 6;
    if ((threadIdx.x & 63) == 0 && w < n_words) {
        on_bits[(size_t)k * n_words + w] = bo;
        hi_bits[(size_t)k * n_words + w] = bh;
    }
}

#define DETECT_EDGE_CAP 4096                                      // 64 words x 64 bits: every edge of a chunk
__global__ __launch_bounds__(64) void detect_walk_k(const unsigned long long* __restrict__ on_bits,
                                                    const unsigned long long* __restrict__ hi_bits, long n_words, int min_gap,
                                                    int min_len, int write, int max_events, int* __restrict__ counts,
                                                    const int* __restrict__ offsets, int* __restrict__ cls,
                                                    int* __restrict__ onset, int* __restrict__ offset) {
    __shared__ int epos[DETECT_EDGE_CAP], eh[DETECT_EDGE_CAP];
    const int k = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* ob = on_bits + (size_t)k * n_words;
    const unsigned long long* hb = hi_bits + (size_t)k * n_words;
    const long base = write ? offsets[k] : 0;
    unsigned carry_top = 0;                      // bit 63 of the previous chunk's last word
    long hbase = 0;                              // high bits before this chunk
    // lane 0's walk state
    bool open = false, have = false;
    int r_on = 0, p_on = 0, p_off = 0;
    long r_h = 0;
    int cnt = 0;
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
                if (have && p_off - p_on >= min_len) {
                    if (write && base + cnt < max_events) {
                        cls[base + cnt] = k; onset[base + cnt] = p_on; offset[base + cnt] = p_off;
                    }
                    ++cnt;
                }
                have = true; p_on = r_on; p_off = r_off;
            }
        }
        __syncthreads();
        carry_top = (unsigned)__shfl((unsigned)(on >> 63), 63, 64);
        hbase += n_high;
    }
    if (lane == 0) {
        if (have && p_off - p_on >= min_len) {
            if (write && base + cnt < max_events) { cls[base + cnt] = k; onset[base + cnt] = p_on; offset[base + cnt] = p_off; }
            ++cnt;
        }
        if (!write) counts[k] = cnt;
    }
}

__global__ void detect_offsets_k(const int* __restrict__ counts, int K, int* __restrict__ offsets, int* __restrict__ total) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int t = 0;
    for (int k = 0; k < K; ++k) { offsets[k] = t; t += counts[k]; }
    *total = t;
}

// one workgroup per event (grid-stride over the events): max of the unfiltered track over [onset, offset), first arg-max
__global__ __launch_bounds__(256) void detect_peaks_k(const float* __restrict__ probs, int K, const int* __restrict__ total,
                                                      int max_events, const int* __restrict__ cls, const int* __restrict__ onset,
                                                      const int* __restrict__ offset, float* __restrict__ peak,
                                                      int* __restrict__ peak_frame) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int n = *total < max_events ? *total : max_events;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const int k = cls[e], a = onset[e], b = offset[e];
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = a + (int)threadIdx.x; j < b; j += 256) {
            const float v = probs[(size_t)j * K + k];
            if (v > bv) { bv = v; bi = j; }                       // ascending j: the first maximum of this thread's frames
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < 4; ++q)
                if (sv[q] > bv || (sv[q] == bv && si[q] < bi)) { bv = sv[q]; bi = si[q]; }
            peak[e] = bv;
            peak_frame[e] = bi;
        }
        __syncthreads();
    }
}

extern "C" size_t sed_detect_workspace_bytes(long n_out, int K, int max_events) {
    if (n_out < 1 || n_out > 0x7fffffffL || K < 1 || K > 32 || max_events < 0 || n_out * K > 0x7fffffffL) return 0;
    return (size_t)2 * K * detect_words(n_out) * sizeof(unsigned long long) + (size_t)2 * K * sizeof(int);
}

template <int M>
static void launch_bits(const float* probs, int n_out, int K, long n_words, float lo, float hi, unsigned long long* ob,
                        unsigned long long* hb, hipStream_t s) {
    detect_bits_k<M><<<dim3((unsigned)cdiv(n_words * 64, 256), (unsigned)K), 256, 0, s>>>(probs, n_out, K, n_words, lo, hi, ob, hb);
}

extern "C" int sed_detect_events(const float* probs, long n_out, int K, int median, float lo, float hi, int min_gap, int min_len,
                                 int max_events, void* workspace, size_t workspace_bytes, int* cls, int* onset, int* offset,
                                 float* peak, int* peak_frame, int* count, void* stream) {
    SED_REQUIRE(probs && workspace && count, "detect_events: null pointer");
    const size_t need = sed_detect_workspace_bytes(n_out, K, max_events);
    SED_REQUIRE(need > 0, "detect_events: bad sizes (n_out=%ld, K=%d in 1..32, max_events=%d >= 0)", n_out, K, max_events);
    SED_REQUIRE(workspace_bytes >= need, "detect_events: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(median >= 1 && median <= 31 && (median & 1), "detect_events: median width must be odd, 1..31 (got %d)", median);
    SED_REQUIRE(hi >= lo, "detect_events: need hi >= lo (got lo=%g, hi=%g)", (double)lo, (double)hi);
    SED_REQUIRE(min_gap >= 0 && min_len >= 1, "detect_events: min_gap >= 0 and min_len >= 1 (got %d, %d)", min_gap, min_len);
    SED_REQUIRE(max_events == 0 || (cls && onset && offset && peak && peak_frame), "detect_events: null output pointer");
    hipStream_t s = as_stream(stream);
    const long nw = detect_words(n_out);
    unsigned long long* ob = (unsigned long long*)workspace;
    unsigned long long* hb = ob + (size_t)K * nw;
    int* counts = (int*)(hb + (size_t)K * nw);
    int* offs = counts + K;
    switch (median) {
#define DETECT_MED(m) case m: launch_bits<m>(probs, (int)n_out, K, nw, lo, hi, ob, hb, s); break;
        DETECT_MED(1) DETECT_MED(3) DETECT_MED(5) DETECT_MED(7) DETECT_MED(9) DETECT_MED(11) DETECT_MED(13) DETECT_MED(15)
        DETECT_MED(17) DETECT_MED(19) DETECT_MED(21) DETECT_MED(23) DETECT_MED(25) DETECT_MED(27) DETECT_MED(29) DETECT_MED(31)
#undef DETECT_MED
    }
    SED_LAUNCH_CHECK("detect_bits");
    detect_walk_k<<<K, 64, 0, s>>>(ob, hb, nw, min_gap, min_len, 0, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk(count)");
    detect_offsets_k<<<1, 64, 0, s>>>(counts, K, offs, count);
    SED_LAUNCH_CHECK("detect_offsets");
    if (max_events == 0) return 0;
    detect_walk_k<<<K, 64, 0, s>>>(ob, hb, nw, min_gap, min_len, 1, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk(write)");
    detect_peaks_k<<<max_events < 1024 ? max_events : 1024, 256, 0, s>>>(probs, K, count, max_events, cls, onset, offset, peak, peak_frame);
    SED_LAUNCH_CHECK("detect_peaks");
    return 0;
}
