// detect_shared.h — device code shared by the offline detector (detect.hip) and the streaming step (stream.hip): the stitch of
// one (output frame, class) cell and the exclusive scan of per-(segment, class) event counts.  Both files call the SAME
// functions, so a streamed track row is bit for bit the row sed_detect_stitch writes.
#pragma once
#include "common.h"

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
