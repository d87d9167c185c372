// mvdr.hip — the audio of every located event through an adaptive (MVDR) beam: sed_event_mvdr, and on the PCM rings
// of live feeds sed_event_mvdr_ring.
//
// The events, their samples [s0, s1) and the packed output (audio_len, audio_start) are sed_event_beam_spans' (beam_shared.h).  The
// transform grid is the event's own: N = 2048, B = 1024, len = s1 - s0, J = ceil(len / B); frame j = 0..J holds
// x_c[s0 + (j - 1) B + m], m < 2048, with EVERY sample outside [s0, s1) read as 0, under the window w[m] = sqrt(hann[m]) of the
// table blob (w[m]^2 + w[m + B]^2 = 1).  With X_{c,j} the half spectrum of frame j of channel c, per bin k = 0..1024:
//   R[k]  = sum_{j=0..J} X_j[k] X_j[k]^H                      fp32, ascending j (chunk partials added in ascending chunk order)
//   d_c   = exp(+2 pi i k tau[dir][c] / 2048),  lambda = loading trace(R) / C
//   v = (R + lambda I)^-1 d,  w = v / (d^H v)                 float64, Cholesky;  trace(R) not > 0: w = d / C;  stored as fp32
//   Y_j[k] = sum_c conj(w_c[k]) X_{c,j}[k]                    ascending c; the imaginary parts of Y[0] and Y[1024] are dropped
// v_j = the inverse real FFT of Y_j, and output sample i = j B + m < len is w[m + B] v_j[m + B] + w[m] v_{j+1}[m].
// An event's audio is a function of its own samples, tau[dir] and loading alone: no atomics, and nothing depends on the launch
// shape, the slice or the workspace.
//
// Shape (gfx950), three plain launches per slice of the event table, workspace rows of 1026 float2 per event:
//   mvdr_cov_k      one workgroup of 8 waves per (event, chunk of MV_CHUNK frames): per frame the FFT of the C channels into LDS
//                   (a half wave per channel: tdoa_accum_k's transform), then the C(C+1)/2 entries X_i conj X_j, j <= i, of every
//                   bin added into LDS accumulators, an entry by one lane, frame after frame; the chunk's partial sums go to the
//                   workspace.  Where the accumulators do not fit beside the spectra (C >= 5) the entries go in batches and the
//                   chunk's frames are transformed again for every batch, as tdoa_accum_k does with its pairs.
//   mvdr_weights_k  one thread per (event, bin): the chunk partials added in ascending order, the matrix, d and the solve in
//                   float64, every thread's own column of three LDS arrays (an 8 x 8 complex double matrix does not fit registers).
//   mvdr_apply_k    one workgroup per (event, run of MV_RUN output blocks) walks the run's frames: transforms the C channels again
//                   (the spectra are not stored: 8 KB per channel and frame) while one more wave inverts the Y of the frame before
//                   (ifft2048_unpair / ifft2048_passes) to the windowed frame in LDS; then every thread adds that frame's first
//                   half to the tail it kept of the frame before it — each block is written once, as consecutive floats — and
//                   combines the new spectra with w from the workspace into the next Y.  Two barriers per frame.
// A frame inside [s0, s1) on an 8-byte boundary takes tdoa_accum_k's direct loads; frames 0 and J, which reach outside the event,
// and unaligned events go through fft_load_guarded: the same samples.
//
// Live feeds: sed_event_mvdr_ring is the same three launches with mvdr_ring_cov_k and mvdr_ring_apply_k, the same
// bodies with the frame loaded from the feed's PCM rings (sed_stream_ring_write; TdArgs.cap) — directly where the frame does not
// wrap, through the guarded loads with the index taken modulo cap where it does — so the registers hold the samples the linear
// call loads and everything after the loads is one code: the same bits.  The weight kernel reads no PCM and has no ring form.
//
// The covariance from before the onset: sed_event_mvdr_noise / sed_event_mvdr_noise_ring with Kn = noise_blocks >= 1
// and G = noise_guard.  An extracted event with s0 >= (G + Kn + 1) B gets its weights from Rn[k] = sum_q X_q X_q^H over the Kn
// frames q of 2048 samples that start at s0 - (G + Kn + 1 - q) B of its RECORDING (fp32, ascending q, chunks of MV_CHUNK added
// in ascending order), by the formula above with Rn for R; every other event is the above, bit for bit.  mvdr_noise_k /
// mvdr_ring_noise_k are the covariance body over those frames (mv_load_abs / mv_load_abs_ring: direct loads, or guarded ones
// with every index checked against the recording); a slice is then four launches — own covariance, noise covariance, weights,
// apply — and each covariance launch returns at once for the other's events.  noise_frames_out says which events used it.
#include <math.h>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "beam_shared.h"

#define MV_WAVES 8
#define MV_THREADS (MV_WAVES * 64)
#define MV_TAB_WORDS LM_OFF_ENT                   // of the table blob: header, window, inter-pass and pairing twiddles
#define MV_FFT_SCR (2 * LM_SCR)                   // floats of exchange scratch per transforming wave
#define MV_LDS_MAX ((size_t)160 * 1024)
#define MV_B (LM_NFFT / 2)                        // the hop of the event's own grid: an output block
#define MV_CHUNK 32                               // frames per workgroup of the covariance launch
#define MV_RUN 16                                 // output blocks per workgroup of the apply launch (MV_RUN + 1 frames)
#define MV_WT 64                                  // bins per workgroup of the weight launch
#define MV_MAX_TRI (TD_MAX_CH * (TD_MAX_CH + 1) / 2)

namespace {

struct MvArgs {
    const int *ev_dir, *ev_loc;                  // [E] the direction row (-1: not extracted) and the frames it was located on
    int D;
    const int* audio_len;                        // [E]
    const long* audio_start;                     // [E]
    long total;
    int cpe;                                     // chunk slots per event in the workspace
    int rows;                                    // rows per event: cpe x C(C+1)/2 partials, then the C rows of w
    int batch;                                   // entries of the triangle that mvdr_cov_k holds at a time
    int kn, guard;                               // Kn noise frames that end guard blocks before the onset (kn = 0: none)
    int* noise_frames;                           // [E] kn where the event's weights come from the noise covariance, else 0 (kn > 0)
};

// whether the weights of an extracted event at s0 come from the covariance of the kn frames before its onset: the samples
// [s0 - (guard + kn + 1) B, s0 - guard B) must exist: s0 >= (guard + kn + 1) B.  All or nothing, and a function of the event
// and the settings alone.  Compared in whole blocks and in 32 bits (0 <= s0 < 2^42: mv_run refuses longer recordings with
// kn > 0): the scalar unit has no 64-bit ordering compare, and a vector one would be new to mvdr_cov_k's prologue.
__device__ __forceinline__ bool mv_uses_noise(const MvArgs& ma, long s0) {
    return ma.kn > 0 && (unsigned)(s0 >> 10) >= (unsigned)(ma.guard + ma.kn + 1);
}

// event e: its recording, first sample and length.  len = 0: not extracted, or a span table that was not made from this event
// table (nothing is read or written for it, as in beam_sum_k)
__device__ __forceinline__ void mv_event(const TdArgs& ta, const MvArgs& ma, long e, int& rec, long& s0, int& len) {
    bm_event_span(ta, ma.ev_dir, ma.ev_loc, ma.D, e, rec, s0, len);
    if (len == 0) return;
    const long start = ma.audio_start[e];
    if (ma.audio_len[e] != len || start < 0 || start > ma.total - len) len = 0;
}

// entry t of the lower triangle, row by row -> (i, j), j <= i
__device__ __forceinline__ void mv_tri(int t, int& i, int& j) {
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    j = t - i * (i + 1) / 2;
}

// frame j of an event into the registers the passes read: ev = the channel's sample s0; sample (j - 1) B + off of the event, 0 outside [0, len)
__device__ __forceinline__ void mv_load_frame(f2 (&z)[32], const float* __restrict__ ev, int len, int j, float* scr, const FftLane& fl) {
    const long first = (long)(j - 1) * MV_B;
    const bool fast = first >= 0 && first + LM_NFFT <= len && (reinterpret_cast<uintptr_t>(ev) & 7) == 0;
    if (__all(fast)) {
        const f2* src = reinterpret_cast<const f2*>(ev + first) + fl.r();
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
    } else {
        fft_load_guarded(z, scr, fl, [&](int off) -> float {
            const long i = first + off;
            return i >= 0 && i < len ? ev[i] : 0.f;
        });
    }
}

// ... of a live feed: lane = the channel's ring of cap samples, sample i of the feed at lane[i % cap] while kept <= i < n (the
// event ends at or before n: bm_event_span).  A frame inside the event and inside what the ring holds that does not wrap and
// starts on an 8-byte boundary takes the same 32 loads; every other frame — 0 and J, one that straddles the wrap point, an odd
// s0 — the guarded ones, with the index taken modulo cap: the registers hold the same samples either way.
__device__ __forceinline__ void mv_load_frame_ring(f2 (&z)[32], const float* __restrict__ lane, long cap, long kept, long s0, int len,
                                                   int j, float* scr, const FftLane& fl) {
    const long first = (long)(j - 1) * MV_B;
    long pos = (s0 + first) % cap;                               // the frame's first sample in the ring (s0 + first >= -B)
    if (pos < 0) pos += cap;
    const bool fast = first >= 0 && first + LM_NFFT <= len && s0 + first >= kept && pos + LM_NFFT <= cap &&
                      (reinterpret_cast<uintptr_t>(lane + pos) & 7) == 0;
    if (__all(fast)) {
        const f2* src = reinterpret_cast<const f2*>(lane + pos) + fl.r();
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
    } else {
        fft_load_guarded(z, scr, fl, [&](int off) -> float {
            const long i = first + off, p = pos + off;           // (cap >= 2048: p < 2 cap)
            return i >= 0 && i < len && s0 + i >= kept ? lane[p >= cap ? p - cap : p] : 0.f;
        });
    }
}

// 2048 samples of a recording of n samples from sample `first` on — a noise frame, which lies before the event:
// chan = the channel's sample 0.  A frame inside [0, n) on an 8-byte boundary takes the direct loads; every other one the
// guarded loads, each index checked against [0, n): whatever the event table says, nothing outside the channel is read.
__device__ __forceinline__ void mv_load_abs(f2 (&z)[32], const float* __restrict__ chan, long n, long first, float* scr, const FftLane& fl) {
    const bool fast = first >= 0 && first + LM_NFFT <= n && (reinterpret_cast<uintptr_t>(chan + first) & 7) == 0;
    if (__all(fast)) {
        const f2* src = reinterpret_cast<const f2*>(chan + first) + fl.r();
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
    } else {
        fft_load_guarded(z, scr, fl, [&](int off) -> float {
            const long i = first + off;
            return i >= 0 && i < n ? chan[i] : 0.f;
        });
    }
}

// ... of a live feed that has received n samples: mv_load_frame_ring's scheme — one remainder per frame; direct loads where the
// frame does not wrap, is aligned and is at or after kept = max(0, n - cap); otherwise guarded loads with the index taken
// modulo cap, and a sample outside [kept, n) reads as 0
__device__ __forceinline__ void mv_load_abs_ring(f2 (&z)[32], const float* __restrict__ lane, long cap, long n, long first, float* scr,
                                                 const FftLane& fl) {
    const long kept = n > cap ? n - cap : 0;
    long pos = first % cap;
    if (pos < 0) pos += cap;
    const bool fast = first >= kept && first + LM_NFFT <= n && pos + LM_NFFT <= cap && (reinterpret_cast<uintptr_t>(lane + pos) & 7) == 0;
    if (__all(fast)) {
        const f2* src = reinterpret_cast<const f2*>(lane + pos) + fl.r();
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
    } else {
        fft_load_guarded(z, scr, fl, [&](int off) -> float {
            const long i = first + off, p = pos + off;           // (cap >= 2048: p < 2 cap)
            return i >= kept && i < n ? lane[p >= cap ? p - cap : p] : 0.f;
        });
    }
}

// noise frame q of channel ch of the event at s0 of recording rec: the 2048 samples from s0 - (guard + kn + 1 - q) B
// on, read from the recording
template <bool RING>
__device__ __forceinline__ void mv_load_noise(f2 (&z)[32], const float* __restrict__ pcm, const TdArgs& ta, const MvArgs& ma, int rec, int ch,
                                              long s0, int q, float* scr, const FftLane& fl) {
    const long n = ta.n_samples[rec], first = s0 - (long)(ma.guard + ma.kn + 1 - q) * MV_B;
    if (RING) mv_load_abs_ring(z, pcm + ((long)rec * ta.C + ch) * ta.cap, ta.cap, n, first, scr, fl);
    else mv_load_abs(z, pcm + ta.sample_off[(long)rec * ta.C + ch], n, first, scr, fl);
}

// frame j of channel ch of the event at s0 of recording rec: RING = false from the planar PCM, RING = true from the feed's rings
template <bool RING>
__device__ __forceinline__ void mv_load(f2 (&z)[32], const float* __restrict__ pcm, const TdArgs& ta, int rec, int ch, long s0, int len,
                                        int j, float* scr, const FftLane& fl) {
    if (RING) {
        const long n = ta.n_samples[rec];
        mv_load_frame_ring(z, pcm + ((long)rec * ta.C + ch) * ta.cap, ta.cap, n > ta.cap ? n - ta.cap : 0, s0, len, j, scr, fl);
    } else {
        mv_load_frame(z, pcm + ta.sample_off[(long)rec * ta.C + ch] + s0, len, j, scr, fl);
    }
}

// The bodies of the covariance and the apply kernels, once for the planar PCM (mvdr_cov_k, mvdr_apply_k) and once for the rings
// of live feeds (mvdr_ring_cov_k, mvdr_ring_apply_k): two kernels each, not one with a run-time branch, so that the linear
// kernels compile to what they were before the rings existed; only mv_load differs.  NOISE = true (mvdr_noise_k,
// mvdr_ring_noise_k) is the same body over the kn frames before the onset of the events whose weights come from
// them; with kn > 0 the two launches share the events between them and each leaves the other's alone.
template <bool RING, bool NOISE>
__device__ __forceinline__ void mv_cov_body(const float* __restrict__ pcm, const uint32_t* __restrict__ tables, float2* __restrict__ ws,
                                            TdArgs ta, MvArgs ma) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long e = ta.e0 + blockIdx.y;
    int rec, len;
    long s0;
    mv_event(ta, ma, e, rec, s0, len);
    const bool noise = len != 0 && mv_uses_noise(ma, s0);
    if (NOISE && blockIdx.x == 0 && tid == 0) ma.noise_frames[e] = noise ? ma.kn : 0;
    if (len == 0 || noise != NOISE) return;                      // (block-uniform: before any barrier)
    const int nfr = NOISE ? ma.kn : (len + MV_B - 1) / MV_B + 1; // the frames before the onset, or frames 0 .. J
    const int fc0 = blockIdx.x * MV_CHUNK;
    if (fc0 >= nfr) return;
    const int fc1 = fc0 + MV_CHUNK < nfr ? fc0 + MV_CHUNK : nfr;
    fft_stage_tables(lds, tables, MV_TAB_WORDS, tid, MV_THREADS);
    const f2* s_win = reinterpret_cast<const f2*>(lds + LM_OFF_WIN);
    const f2* s_tw = reinterpret_cast<const f2*>(lds + LM_OFF_TW);
    const f2* s_pw = reinterpret_cast<const f2*>(lds + LM_OFF_PW);
    const int C = ta.C, T = C * (C + 1) / 2;
    const int nfw = (C + 1) >> 1;                                // waves that transform
    float2* s_spec = reinterpret_cast<float2*>(lds + MV_TAB_WORDS);                              // [C][PHAT_SPEC]
    float* s_scr = lds + MV_TAB_WORDS + C * PHAT_SPEC * 2;                                       // [nfw][MV_FFT_SCR]
    float2* s_acc = reinterpret_cast<float2*>(s_scr + nfw * MV_FFT_SCR);                         // [batch][PHAT_SPEC]
    const int wave = tid >> 6;
    float* wscr = s_scr + (wave < nfw ? wave : 0) * MV_FFT_SCR;  // (only used by waves < nfw)
    const FftLane fl = fft_lane(tid & 63, wscr - lds);
    const int half = fl.half();
    float* scr = wscr + half * LM_SCR;
    float2* wrow = ws + ((long)blockIdx.y * ma.rows + (long)blockIdx.x * T) * PHAT_SPEC;

    for (int t0 = 0; t0 < T; t0 += ma.batch) {
        const int nb = T - t0 < ma.batch ? T - t0 : ma.batch;
        for (int idx = tid; idx < nb * PHAT_SPEC; idx += MV_THREADS) s_acc[idx] = make_float2(0.f, 0.f);
        __syncthreads();                                         // the tables are in LDS (first batch); the spectra are free
        for (int j = fc0; j < fc1; ++j) {
            if (wave < nfw) {
                // the frame of channel 2 wave + half (an odd C: the last half wave repeats channel C-1 and stores the same values)
                const int ch = (2 * wave + half < C) ? 2 * wave + half : C - 1;
                f2 z[32];
                if (NOISE) mv_load_noise<RING>(z, pcm, ta, ma, rec, ch, s0, j, scr, fl);
                else mv_load<RING>(z, pcm, ta, rec, ch, s0, len, j, scr, fl);
                fft2048_passes(z, fl, s_win, s_tw);
                fft2048_spectrum(z, fl, s_pw, s_spec + ch * PHAT_SPEC);
            }
            __syncthreads();
            // bin k of every entry is read and written by this lane alone, frame after frame; the entry is uniform
            for (int tb = 0; tb < nb; ++tb) {
                int i, jj;
                mv_tri(t0 + tb, i, jj);
                const float2 *sa = s_spec + i * PHAT_SPEC, *sb = s_spec + jj * PHAT_SPEC;
                float2* acc = s_acc + tb * PHAT_SPEC;
                for (int k = tid; k <= LM_N; k += MV_THREADS) {
                    const float2 a = sa[k], b = sb[k];
                    float2 s = acc[k];
                    if (i == jj) s.x += a.x * a.x + a.y * a.y;   // (a diagonal entry is real)
                    else { s.x += a.x * b.x + a.y * b.y; s.y += a.y * b.x - a.x * b.y; }
                    acc[k] = s;
                }
            }
            __syncthreads();                                     // the spectra may be overwritten
        }
        for (int idx = tid; idx < nb * 1025; idx += MV_THREADS) {
            const int tb = idx / 1025, k = idx - tb * 1025;
            wrow[(long)(t0 + tb) * PHAT_SPEC + k] = s_acc[tb * PHAT_SPEC + k];
        }
        __syncthreads();                                         // the accumulators are zeroed for the next batch
    }
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_cov_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                         float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<false, false>(pcm, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_ring_cov_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                              float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<true, false>(ring, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_noise_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                           float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<false, true>(pcm, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_ring_noise_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                                float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<true, true>(ring, tables, ws, ta, ma);
}

// Every thread works in its own column of the three arrays: no thread reads what another writes, and there is no barrier.
__global__ __launch_bounds__(MV_WT) void mvdr_weights_k(float2* __restrict__ ws, const double* __restrict__ tau, double loading,
                                                        TdArgs ta, MvArgs ma) {
    __shared__ double2 s_A[MV_MAX_TRI][MV_WT];                   // the lower triangle of R + lambda I, then of its Cholesky factor
    __shared__ double2 s_d[TD_MAX_CH][MV_WT];
    __shared__ double2 s_v[TD_MAX_CH][MV_WT];
    const int tid = threadIdx.x, k = blockIdx.x * MV_WT + tid;
    if (k > LM_N) return;
    const long e = ta.e0 + blockIdx.y;
    int rec, len;
    long s0;
    mv_event(ta, ma, e, rec, s0, len);
    if (len == 0) return;
    const int C = ta.C, T = C * (C + 1) / 2;
    const int nfr = mv_uses_noise(ma, s0) ? ma.kn : (len + MV_B - 1) / MV_B + 1, nch = (nfr + MV_CHUNK - 1) / MV_CHUNK;
    float2* wev = ws + (long)blockIdx.y * ma.rows * PHAT_SPEC;
    float2* wout = wev + (long)ma.cpe * T * PHAT_SPEC;           // [C][PHAT_SPEC]
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float2 s = wev[(long)t * PHAT_SPEC + k];
#pragma unroll 1
        for (int c = 1; c < nch; ++c) {                          // fp32, ascending chunks
            const float2 p = wev[((long)c * T + t) * PHAT_SPEC + k];
            s.x += p.x; s.y += p.y;
        }
        s_A[t][tid] = make_double2((double)s.x, (double)s.y);
    }
    double trace = 0.0;
#pragma unroll 1
    for (int i = 0; i < C; ++i) trace += s_A[i * (i + 1) / 2 + i][tid].x;
    const double* trow = tau + (long)ma.ev_dir[e] * C;           // (0 <= dir < D: the event has samples)
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        double sn, cs;
        sincospi((double)k * trow[c] * (1.0 / MV_B), &sn, &cs);  // 2 pi k tau / 2048
        s_d[c][tid] = make_double2(cs, sn);
    }
    if (!(trace > 0.0)) {                                        // digital silence (or NaN samples): the plain average
#pragma unroll 1
        for (int c = 0; c < C; ++c) wout[(long)c * PHAT_SPEC + k] = make_float2((float)(s_d[c][tid].x / C), (float)(s_d[c][tid].y / C));
        return;
    }
    const double lambda = loading * trace / C;
#pragma unroll 1
    for (int i = 0; i < C; ++i) {
        double2 a = s_A[i * (i + 1) / 2 + i][tid];
        s_A[i * (i + 1) / 2 + i][tid] = make_double2(a.x + lambda, 0.0);
    }
    // ── Cholesky, in place: L[i][j], j <= i, at i (i + 1) / 2 + j; the diagonal holds 1 / L[j][j] in .y ──
#pragma unroll 1
    for (int j = 0; j < C; ++j) {
        const int rj = j * (j + 1) / 2;
        double s = s_A[rj + j][tid].x;
#pragma unroll 1
        for (int p = 0; p < j; ++p) { const double2 l = s_A[rj + p][tid]; s -= l.x * l.x + l.y * l.y; }
        const double ljj = sqrt(s), inv = 1.0 / ljj;
        s_A[rj + j][tid] = make_double2(ljj, inv);
#pragma unroll 1
        for (int i = j + 1; i < C; ++i) {
            const int ri = i * (i + 1) / 2;
            double2 a = s_A[ri + j][tid];
#pragma unroll 1
            for (int p = 0; p < j; ++p) {                        // a -= L[i][p] conj L[j][p]
                const double2 li = s_A[ri + p][tid], lj = s_A[rj + p][tid];
                a.x -= li.x * lj.x + li.y * lj.y;
                a.y -= li.y * lj.x - li.x * lj.y;
            }
            s_A[ri + j][tid] = make_double2(a.x * inv, a.y * inv);
        }
    }
    // ── L y = d, then L^H v = y ──
#pragma unroll 1
    for (int i = 0; i < C; ++i) {
        const int ri = i * (i + 1) / 2;
        double2 y = s_d[i][tid];
#pragma unroll 1
        for (int p = 0; p < i; ++p) {
            const double2 l = s_A[ri + p][tid], v = s_v[p][tid];
            y.x -= l.x * v.x - l.y * v.y;
            y.y -= l.x * v.y + l.y * v.x;
        }
        const double inv = s_A[ri + i][tid].y;
        s_v[i][tid] = make_double2(y.x * inv, y.y * inv);
    }
#pragma unroll 1
    for (int i = C - 1; i >= 0; --i) {
        double2 y = s_v[i][tid];
#pragma unroll 1
        for (int p = i + 1; p < C; ++p) {                        // y -= conj L[p][i] v[p]
            const double2 l = s_A[p * (p + 1) / 2 + i][tid], v = s_v[p][tid];
            y.x -= l.x * v.x + l.y * v.y;
            y.y -= l.x * v.y - l.y * v.x;
        }
        const double inv = s_A[i * (i + 1) / 2 + i][tid].y;
        s_v[i][tid] = make_double2(y.x * inv, y.y * inv);
    }
    double den = 0.0;                                            // d^H v = d^H (R + lambda I)^-1 d: real and positive
#pragma unroll 1
    for (int c = 0; c < C; ++c) den += s_d[c][tid].x * s_v[c][tid].x + s_d[c][tid].y * s_v[c][tid].y;
    const double scale = 1.0 / den;
#pragma unroll 1
    for (int c = 0; c < C; ++c) wout[(long)c * PHAT_SPEC + k] = make_float2((float)(s_v[c][tid].x * scale), (float)(s_v[c][tid].y * scale));
}

template <bool RING>
__device__ __forceinline__ void mv_apply_body(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                              const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta, MvArgs ma) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long e = ta.e0 + blockIdx.y;
    int rec, len;
    long s0;
    mv_event(ta, ma, e, rec, s0, len);
    if (len == 0) return;                                        // (block-uniform: before any barrier)
    const int J = (len + MV_B - 1) / MV_B;
    const int b0 = blockIdx.x * MV_RUN;                          // the run's blocks [b0, b1) need the frames b0 .. b1
    if (b0 >= J) return;
    const int b1 = b0 + MV_RUN < J ? b0 + MV_RUN : J;
    fft_stage_tables(lds, tables, MV_TAB_WORDS, tid, MV_THREADS);
    const f2* s_win = reinterpret_cast<const f2*>(lds + LM_OFF_WIN);
    const f2* s_tw = reinterpret_cast<const f2*>(lds + LM_OFF_TW);
    const f2* s_pw = reinterpret_cast<const f2*>(lds + LM_OFF_PW);
    const int C = ta.C, T = C * (C + 1) / 2;
    const int nfw = (C + 1) >> 1;
    float2* s_spec = reinterpret_cast<float2*>(lds + MV_TAB_WORDS);                              // [C][PHAT_SPEC]
    float* s_scr = lds + MV_TAB_WORDS + C * PHAT_SPEC * 2;                                       // [nfw + 1][MV_FFT_SCR]
    float2* s_y = reinterpret_cast<float2*>(s_scr + (nfw + 1) * MV_FFT_SCR);                     // [PHAT_SPEC] Y_j
    float* s_frame = reinterpret_cast<float*>(s_y + PHAT_SPEC);                                  // [2048] the windowed v_j
    float* s_tail = s_frame + LM_NFFT;                                                           // [1024] w[m + B] v_{j-1}[m + B]
    const int wave = tid >> 6;                                   // waves 0 .. nfw - 1 transform, wave nfw (<= 4) inverts
    float* wscr = s_scr + (wave <= nfw ? wave : 0) * MV_FFT_SCR;
    const FftLane fl = fft_lane(tid & 63, wscr - lds);
    const int half = fl.half(), r = fl.r();
    float* scr = wscr + half * LM_SCR;
    const float2* wts = ws + ((long)blockIdx.y * ma.rows + (long)ma.cpe * T) * PHAT_SPEC;        // [C][PHAT_SPEC] w
    float* dst = audio + ma.audio_start[e];
    __syncthreads();                                             // the tables are in LDS

    // Step j: the transforming waves turn frame j into spectra while wave nfw turns Y_{j-1} into the windowed frame j - 1; after
    // the barrier every thread adds that frame's first half to the tail it kept (block j - 2 of the event), keeps its second
    // half, and combines the new spectra into Y_j.  One more step drains the last frame.
    for (int j = b0; j <= b1 + 1; ++j) {
        if (wave < nfw && j <= b1) {
            const int ch = (2 * wave + half < C) ? 2 * wave + half : C - 1;
            f2 z[32];
            mv_load<RING>(z, pcm, ta, rec, ch, s0, len, j, scr, fl);
            fft2048_passes(z, fl, s_win, s_tw);
            fft2048_spectrum(z, fl, s_pw, s_spec + ch * PHAT_SPEC);
        } else if (wave == nfw && j > b0) {                      // (both halves transform the same Y_{j-1}; one stores)
            f2 z[32];
            ifft2048_unpair(z, fl, s_pw, s_y);
            ifft2048_passes(z, fl, s_win, s_tw);
            if (half == 0) {
#pragma unroll
                for (int k2 = 0; k2 < 32; ++k2) reinterpret_cast<f2*>(s_frame)[r + 32 * k2] = z[brev5(k2)];
            }
        }
        __syncthreads();
        if (j > b0) {
            for (int m = tid; m < MV_B; m += MV_THREADS) {       // entry m of the tail belongs to this thread
                const long i = (long)(j - 2) * MV_B + m;         // frame j - 1 starts at block j - 2
                if (j - 1 > b0 && i < len) dst[i] = s_tail[m] + s_frame[m];
                s_tail[m] = s_frame[m + MV_B];
            }
        }
        if (j <= b1) {
            for (int k = tid; k <= LM_N; k += MV_THREADS) {
                float2 y = make_float2(0.f, 0.f);
                for (int c = 0; c < C; ++c) {                    // conj(w) x, ascending c
                    const float2 w = wts[(long)c * PHAT_SPEC + k], x = s_spec[c * PHAT_SPEC + k];
                    y.x += w.x * x.x + w.y * x.y;
                    y.y += w.x * x.y - w.y * x.x;
                }
                if (k == 0 || k == LM_N) y.y = 0.f;
                s_y[k] = y;
            }
        }
        __syncthreads();                                         // Y_j is whole; the spectra and the frame may be overwritten
    }
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_apply_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                           const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta, MvArgs ma) {
    mv_apply_body<false>(pcm, tables, ws, audio, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_ring_apply_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                                const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta,
                                                                MvArgs ma) {
    mv_apply_body<true>(ring, tables, ws, audio, ta, ma);
}

// rows of 1026 float2 per event: the chunk partials of every entry of the triangle, then w
long mv_chunks(int max_frames, int hop) {
    const long J = ((long)max_frames * hop + MV_B - 1) / MV_B;   // no event has more output blocks
    return (J + 1 + MV_CHUNK - 1) / MV_CHUNK;
}
long mv_noise_chunks(int kn) { return (kn + MV_CHUNK - 1) / MV_CHUNK; }
// chunk slots per event: the own frames' or the noise frames', whichever are more (an event uses one kind)
long mv_slots(int max_frames, int hop, int kn) {
    const long own = mv_chunks(max_frames, hop), nz = mv_noise_chunks(kn);
    return own > nz ? own : nz;
}
size_t mv_event_bytes(int C, long cpe) { return ((size_t)cpe * (C * (C + 1) / 2) + C) * TD_ROW_BYTES; }
size_t mv_cov_lds(int C, int batch) {
    return ((size_t)MV_TAB_WORDS + (size_t)C * PHAT_SPEC * 2 + (size_t)((C + 1) / 2) * MV_FFT_SCR + (size_t)batch * PHAT_SPEC * 2) * sizeof(float);
}
size_t mv_apply_lds(int C) {
    return ((size_t)MV_TAB_WORDS + (size_t)C * PHAT_SPEC * 2 + (size_t)((C + 1) / 2 + 1) * MV_FFT_SCR + PHAT_SPEC * 2 + LM_NFFT + MV_B) * sizeof(float);
}

bool mv_sizes_ok(int R, int channels, int max_frames, int hop) {
    return R >= 1 && channels >= 2 && channels <= TD_MAX_CH && max_frames >= 1 && hop >= 1 && (long)max_frames * hop <= 0x7fffffffL;
}

#define MV_MAX_NOISE 256                          // localize.MVDR: noise_blocks
#define MV_MAX_GUARD 64                           //                noise_guard

// the steering delays [D][C], the diagonal loading and the table blob
struct MvTables { const double* tau; double loading; const void* tables; size_t tables_bytes; };
// kn noise frames that end guard blocks before the onset, and which events used them; entry: one of the noise entries,
// which must be given frames_out
struct MvNoise { int kn, guard; int* frames_out; bool entry; };

// what all entries do once the events and the recordings are checked.  kn = 0 (sed_event_mvdr, sed_event_mvdr_ring, or a noise
// entry asked for no noise frames): three launches per slice, and the noise entries' frames_out is zeroed
template <bool RING>
int mv_run(const char* who, const RecSource& src, const EvTable& ev, const MvTables& mt, const MvNoise& nz, const BeamOut& out,
           void* workspace, size_t workspace_bytes, void* stream) {
    const int kn = nz.kn;
    const long E = ev.E;
    const size_t tab = src.tab;
    SED_REQUIRE(kn >= 0 && kn <= MV_MAX_NOISE, "%s: noise_blocks must be in [0, %d], got %d", who, MV_MAX_NOISE, kn);
    SED_REQUIRE(nz.guard >= 0 && nz.guard <= MV_MAX_GUARD, "%s: noise_guard must be in [0, %d], got %d", who, MV_MAX_GUARD, nz.guard);
    SED_REQUIRE(!nz.entry || E == 0 || nz.frames_out, "%s: null pointer (noise_frames_out)", who);
    SED_REQUIRE(mt.loading >= 1e-6 && mt.loading <= 1e6, "%s: loading must be in [1e-6, 1e6], got %g", who, mt.loading);
    SED_REQUIRE(out.total >= 0, "%s: a total of %ld samples", who, out.total);
    SED_REQUIRE(E == 0 || (mt.tau && out.audio_len && out.audio_start), "%s: null pointer (tau, audio_len or audio_start)", who);
    SED_REQUIRE(out.audio || out.total == 0, "%s: null output buffer for %ld samples", who, out.total);
    SED_REQUIRE(mt.tables && mt.tables_bytes % 16 == 0 && mt.tables_bytes / 4 >= (size_t)MV_TAB_WORDS, "%s: table blob of %zu bytes is malformed",
                who, mt.tables_bytes);
    SED_REQUIRE(((uintptr_t)src.x & 3) == 0, "%s: the samples must be 4-byte aligned", who);
    SED_REQUIRE(kn == 0 || src.longest < (1L << 42), "%s: a recording of %ld samples; with noise_blocks > 0 fewer than 2^42 are taken", who,
                src.longest);
    if (E == 0 || out.total == 0) return 0;                      // nothing to launch (frames_out is not written: no event is extracted)
    const int C = src.C, T = C * (C + 1) / 2;
    const long cpe = mv_slots(ev.max_frames, ev.hop, kn);
    const size_t per_event = mv_event_bytes(C, cpe);
    SED_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device buffer", who);
    SED_REQUIRE(workspace_bytes >= tab + per_event, "%s: workspace of %zu bytes, at least %zu needed (one event)", who, workspace_bytes,
                tab + per_event);
    long slice = (long)((workspace_bytes - tab) / per_event);
    if (slice > E) slice = E;
    if (slice > 65535) slice = 65535;                            // gridDim.y
    int batch = T;
    while (batch > 1 && mv_cov_lds(C, batch) > MV_LDS_MAX) --batch;
    const size_t lds_cov = mv_cov_lds(C, batch), lds_apply = mv_apply_lds(C);
    SED_REQUIRE(lds_cov <= MV_LDS_MAX && lds_apply <= MV_LDS_MAX, "%s: %d spectra and the tables (%zu B, %zu B) exceed the 160 KiB LDS", who,
                C, lds_cov, lds_apply);
    long most = (long)ev.max_frames * ev.hop;                    // no event has more samples than this, or than its recording
    if (most > src.longest) most = src.longest;
    const long blocks = (most + MV_B - 1) / MV_B;
    if (blocks < 1) return 0;
    const unsigned chunks = (unsigned)((blocks + 1 + MV_CHUNK - 1) / MV_CHUNK), runs = (unsigned)((blocks + MV_RUN - 1) / MV_RUN);

    hipStream_t s = as_stream(stream);
    SED_TRY(beam_upload(who, src, workspace, workspace_bytes, s));
    const auto cov_k = RING ? mvdr_ring_cov_k : mvdr_cov_k;
    const auto apply_k = RING ? mvdr_ring_apply_k : mvdr_apply_k;
    hipError_t err = hipFuncSetAttribute((const void*)cov_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    if (err == hipSuccess) err = hipFuncSetAttribute((const void*)apply_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    const auto noise_k = RING ? mvdr_ring_noise_k : mvdr_noise_k;
    if (err == hipSuccess && kn > 0) err = hipFuncSetAttribute((const void*)noise_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    if (kn == 0 && nz.frames_out) {
        err = hipMemsetAsync(nz.frames_out, 0, (size_t)E * sizeof(int), s);
        if (err != hipSuccess) { sed_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(err)); return (int)err; }
    }
    TdArgs ta = td_args(src, ev, workspace);
    const MvArgs ma{ev.dir, ev.loc, ev.D, out.audio_len, out.audio_start, out.total, (int)cpe, (int)(cpe * T + C), batch, kn, nz.guard,
                    nz.frames_out};
    const uint32_t* tables = (const uint32_t*)mt.tables;
    float2* part = (float2*)((char*)workspace + tab);
    for (long e0 = 0; e0 < E; e0 += slice) {
        ta.e0 = e0;
        ta.n_ev = (int)(E - e0 < slice ? E - e0 : slice);
        cov_k<<<dim3(chunks, (unsigned)ta.n_ev), MV_THREADS, lds_cov, s>>>(src.x, tables, part, ta, ma);
        SED_LAUNCH_CHECK("mvdr (covariance)");
        if (kn > 0) {                                            // the host does not know which events use it: both launches run
            noise_k<<<dim3((unsigned)mv_noise_chunks(kn), (unsigned)ta.n_ev), MV_THREADS, lds_cov, s>>>(src.x, tables, part, ta, ma);
            SED_LAUNCH_CHECK("mvdr (noise covariance)");
        }
        mvdr_weights_k<<<dim3((LM_N + MV_WT) / MV_WT, (unsigned)ta.n_ev), MV_WT, 0, s>>>(part, mt.tau, mt.loading, ta, ma);
        SED_LAUNCH_CHECK("mvdr (weights)");
        apply_k<<<dim3(runs, (unsigned)ta.n_ev), MV_THREADS, lds_apply, s>>>(src.x, tables, part, out.audio, ta, ma);
        SED_LAUNCH_CHECK("mvdr (apply)");
    }
    return 0;
}

// an entry: the events and the recordings checked, then the launches
template <bool RING>
int mv_entry(const char* who, RecSource src, const EvTable& ev, const MvTables& mt, const MvNoise& nz, const BeamOut& out, void* workspace,
             size_t workspace_bytes, void* stream) {
    SED_TRY(beam_source<RING>(who, src, ev));
    return mv_run<RING>(who, src, ev, mt, nz, out, workspace, workspace_bytes, stream);
}

}  // namespace

extern "C" size_t sed_event_mvdr_workspace_bytes(int R, int channels, int max_frames, int hop) {
    if (!mv_sizes_ok(R, channels, max_frames, hop)) return 0;
    return rec_table_bytes(R, channels) + mv_event_bytes(channels, mv_chunks(max_frames, hop));
}

extern "C" size_t sed_event_mvdr_ring_workspace_bytes(int R, int channels, int max_frames, int hop) {
    if (!mv_sizes_ok(R, channels, max_frames, hop)) return 0;
    return rec_ring_table_bytes(R) + mv_event_bytes(channels, mv_chunks(max_frames, hop));
}

extern "C" int sed_event_mvdr(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                              const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                              const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                              double loading, const void* tables, size_t tables_bytes, const int* audio_len, const long* audio_start,
                              float* audio, long audio_total, void* workspace, size_t workspace_bytes, void* stream) {
    return mv_entry<false>("mvdr", {pcm, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           {tau, loading, tables, tables_bytes}, {0, 0, nullptr, false}, {audio_len, audio_start, audio, audio_total},
                           workspace, workspace_bytes, stream);
}

extern "C" int sed_event_mvdr_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels, const int* ev_rec,
                                   const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                                   const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                                   double loading, const void* tables, size_t tables_bytes, const int* audio_len,
                                   const long* audio_start, float* audio, long audio_total, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    return mv_entry<true>("mvdr_ring", {ring, true, cap, ring_len, R, channels, n_host},
                          {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                          {tau, loading, tables, tables_bytes}, {0, 0, nullptr, false}, {audio_len, audio_start, audio, audio_total},
                          workspace, workspace_bytes, stream);
}

// ── DESIGN 5u: the weights from the covariance of the noise_blocks frames that end noise_guard blocks before the onset ──
extern "C" size_t sed_event_mvdr_noise_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || noise_blocks < 0 || noise_blocks > MV_MAX_NOISE) return 0;
    return rec_table_bytes(R, channels) + mv_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks));
}

extern "C" size_t sed_event_mvdr_noise_ring_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || noise_blocks < 0 || noise_blocks > MV_MAX_NOISE) return 0;
    return rec_ring_table_bytes(R) + mv_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks));
}

extern "C" int sed_event_mvdr_noise(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                                    const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                                    const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                                    double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                                    const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return mv_entry<false>("mvdr_noise", {pcm, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                           {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream);
}

extern "C" int sed_event_mvdr_noise_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                         const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                                         const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                                         const double* tau, int D, double loading, int noise_blocks, int noise_guard, const void* tables,
                                         size_t tables_bytes, const int* audio_len, const long* audio_start, float* audio,
                                         long audio_total, int* noise_frames_out, void* workspace, size_t workspace_bytes, void* stream) {
    return mv_entry<true>("mvdr_noise_ring", {ring, true, cap, ring_len, R, channels, n_host},
                          {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                          {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                          {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream);
}
