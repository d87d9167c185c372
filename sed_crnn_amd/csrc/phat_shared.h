// phat_shared.h — the PHAT-whitened cross spectrum and its lag synthesis, once, for the kernels that promise each other's bits:
// gcc_phat_k (gcc.hip), tdoa_accum_k / tdoa_finish_k (tdoa.hip, 5o/5p) and doa_steer_k (doa.hip, 5q).  Per-event TDOA
// sums gcc.hip's Pk over frames, DOA at Q = 1 is TDOA bit for bit: the callers differ only in what they do with what these
// functions return.  Device code, force-inlined.
#pragma once
#include "common.h"
#include "fft2048.h"

#define PHAT_SPEC 1026                            // float2 per spectrum / Pk / accumulator row (1025 bins + 1 pad)

namespace {

// pair p of C channels -> (i, j), i < j, lexicographic
__device__ __forceinline__ void phat_pair(int p, int C, int& i, int& j) {
    i = 0;
    while (p >= C - 1 - i) { p -= C - 1 - i; ++i; }
    j = i + 1 + p;
}

// Bin k of Pk = G / |G|, G = a conj b, for the spectra a = X_i[k], b = X_j[k]: 0 where |G|^2 < 1e-30.  Pk[0] is halved (the lag
// sum counts every bin twice) and the DC and Nyquist bins are real.
__device__ __forceinline__ float2 phat_bin(float2 a, float2 b, int k) {
    const float gr = a.x * b.x + a.y * b.y, gi = a.y * b.x - a.x * b.y;
    const float m2 = gr * gr + gi * gi;
    // (m2 beyond the float range — samples of ~1e6 and more — is inf, and G / sqrt(inf) = 0 by the definition for a
    // finite G; G * rsqrt(inf) with an infinite G would be NaN instead, so those bins are written as 0 explicitly)
    const float inv = (m2 >= 1e-30f && m2 <= 3.0e38f) ? rsqrtf(m2) : 0.f;
    float pr = gr * inv, pi = gi * inv;
    if (k == 0) { pr *= 0.5f; pi = 0.f; }
    if (k == LM_N) pi = 0.f;
    return make_float2(pr, pi);
}

// (cos, sin)(2 pi m / N), 0 <= m < N = 4 NQ, unfolded by index from the quarter wave q[k] = (cos, +-sin)(2 pi k / N), k = 0..NQ
// (float64 values rounded once: exact table values, no recurrences).  NEG_SIN: the quarter wave stores -sin, as the log-mel
// blob's pairing twiddles pw do (N = 2048).
template <bool NEG_SIN>
__device__ __forceinline__ float2 phat_angle(const float2* q, int m, int NQ, int NH, int N) {
    const int mm = m <= NH ? m : N - m;                      // cos(2 pi - a) = cos a, sin(2 pi - a) = -sin a
    const int k = mm <= NQ ? mm : NH - mm;                   // cos(pi - a) = -cos a, sin(pi - a) = sin a
    const float2 w = q[k];
    return make_float2(mm <= NQ ? w.x : -w.x, (m <= NH) != NEG_SIN ? w.y : -w.y);
}
// the whole wave of N = 2048 from pw into `lag` [2048]
__device__ __forceinline__ void phat_lag_table(float2* lag, const float2* pw, int tid, int threads) {
    for (int m = tid; m < LM_NFFT; m += threads) lag[m] = phat_angle<true>(pw, m, LM_N / 2, LM_N, LM_NFFT);
}

// The lag sum of one item (a row S of whitened bins, lag tau of N a turn), by the 8 neighbouring lanes j8 = 0..7 that own it:
// lane j8 sums the bins k = j8, j8 + 8, ... in ascending order against table(k tau mod N) = (cos, sin)(2 pi k tau / N) in two fma
// chains, A over Re S cos and B over Im S sin, and the eight partial sums are joined by the xor-1, 2, 4 shuffle tree.  Every
// lane of the group returns the whole sums (A, B): +tau is A - B, -tau is A + B.  (Returned by value, for the reason given at
// first_max_wave.)
template <typename Table>
__device__ __forceinline__ float2 phat_lag_sum(const float2* S, int j8, int tau, int N, Table table) {
    float A = 0.f, B = 0.f;
    int m = (j8 * tau) & (N - 1);
    const int step = (8 * tau) & (N - 1);
#pragma unroll 8
    for (int i = 0; i < LM_N / 8; ++i) {                     // bins k = j8 + 8 i, ascending
        const float2 q = S[j8 + 8 * i], t = table(m);
        A = fmaf(q.x, t.x, A);
        B = fmaf(q.y, t.y, B);
        m = (m + step) & (N - 1);
    }
    A += __shfl_xor(A, 1, 64); B += __shfl_xor(B, 1, 64);
    A += __shfl_xor(A, 2, 64); B += __shfl_xor(B, 2, 64);
    A += __shfl_xor(A, 4, 64); B += __shfl_xor(B, 4, 64);
    return make_float2(A, B);
}

// S [1025] (LDS) = pair p's chunk partials of one event (`wev`: chunk c / pair p at row c P + p), in ascending chunk order
__device__ __forceinline__ void phat_sum_chunks(float2* S, const float2* __restrict__ wev, int p, int P, int nch, int tid, int threads) {
    for (int k = tid; k < 1025; k += threads) {
        float2 s = wev[(long)p * PHAT_SPEC + k];
        for (int c = 1; c < nch; ++c) {
            const float2 v = wev[((long)c * P + p) * PHAT_SPEC + k];
            s.x += v.x; s.y += v.y;
        }
        S[k] = s;
    }
}

// The first maximum of a scan — best at index `at`, ties go to the lower index — and the minimum `low`, over the 64 lanes of a
// wave; every lane returns the result.  (By value: a local whose address a call takes stays in memory until the call is
// inlined, and hipcc then shapes the code around it differently.)
struct FirstMax { float best, low; int at; };
__device__ __forceinline__ FirstMax first_max_wave(FirstMax m) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ob = __shfl_xor(m.best, o, 64), ol = __shfl_xor(m.low, o, 64);
        const int oa = __shfl_xor(m.at, o, 64);
        if (ob > m.best || (ob == m.best && oa < m.at)) { m.best = ob; m.at = oa; }
        m.low = fminf(m.low, ol);
    }
    return m;
}

}  // namespace
