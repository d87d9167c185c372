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
//
// The noise frames where the event's class is silent: sed_event_quiet_frames / sed_event_mvdr_quiet.  The whole
// event table is rasterised once into mask[r][t], a uint32 of class bits per recording and output frame of H = tf hop samples
// (act_mask_build, activity.hip: shared with the contrast SRP-PHAT); mvdr_select_k, a wave per event, gives the S
// candidates q — the 2048 samples from s0 - (G + 2 + q) B, tested on [s0 - (2 G + 2 + q) B, s0 - q B) against the mask — to the
// shared walk (act_select_walk, activity_shared.h): the first Kn eligible ones in summation order (descending q) to noise_sel,
// n_e >= noise_min of them to noise_frames (else 0 and a row of -1: the event keeps its own frames).  A slice is then
// mvdr_quiet_own_k (the own covariance of the events with noise_frames = 0), mvdr_quiet_k (the covariance body over the selected
// frames, mv_load_abs at s0 - (G + 2 + noise_sel[e][j]) B), mvdr_quiet_weights_k (the weight body with the chunk count taken from
// noise_frames) and mvdr_apply_k as it is.  An event whose Kn nearest candidates are eligible reads the frames of
// sed_event_mvdr_noise in its order through the same code: the same bits.  All of it is integer and a function of the table and
// the settings alone.
//
// The beam steered along the event's direction track: sed_event_mvdr_track / sed_event_mvdr_track_ring /
// sed_event_mvdr_quiet_track.  The samples, the covariance launches above and the transform grid are untouched; with T = trk_len[e]
// clamped to [0, Tm] and W = block_chunks, frame j is combined with the weights of track block b_j = min((j B / hop) / (32 W), T - 1),
// steered at trk_dir[e][b_j] where T > 0 and that is a row of tau, else at dir.  mvdr_trk_weights_k / mvdr_trk_quiet_weights_k are the
// weight body with ONE Cholesky factor per (event, bin) and the steering vector, the two solves and the normalisation per block
// b < max(T, 1) — block b's C rows of w behind block b - 1's, an event's rows cpe C(C+1)/2 + C Tm; mvdr_trk_apply_k /
// mvdr_trk_ring_apply_k are the apply body with the weight pointer taken per frame.  The overlap-add is the cross-fade between
// consecutive blocks' beams.  A track whose every used row equals dir gives the untracked kernels' bits.
#include <math.h>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "beam_shared.h"
#include "activity_shared.h"

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

// the frames mvdr_select_k listed for event e (0: it keeps its own), never more than the kn its row of noise_sel holds
__device__ __forceinline__ int mv_quiet_frames(const MvArgs& ma, long e) {
    const int n = ma.noise_frames[e];
    return n < 0 ? 0 : n > ma.kn ? ma.kn : n;
}

// candidate q of channel ch of the event at s0 of recording rec: the 2048 samples from s0 - (guard + 2 + q) B on,
// read from the recording; q = kn - 1 - j is mv_load_noise's frame j
__device__ __forceinline__ void mv_load_quiet(f2 (&z)[32], const float* __restrict__ pcm, const TdArgs& ta, const MvArgs& ma, int rec, int ch,
                                              long s0, int q, float* scr, const FftLane& fl) {
    const long n = ta.n_samples[rec], first = s0 - (long)(ma.guard + 2 + q) * MV_B;
    mv_load_abs(z, pcm + ta.sample_off[(long)rec * ta.C + ch], n, first, scr, fl);
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
// them; with kn > 0 the two launches share the events between them and each leaves the other's alone.  MV_QUIET (mvdr_quiet_k;
// DESIGN 5w) is the same body over the noise_frames[e] frames that mvdr_select_k listed in qsel [E][kn], and MV_QUIET_OWN
// (mvdr_quiet_own_k) the own frames of the events it listed none for: the pair shares the events by noise_frames, which the
// selection has written before the first slice.
#define MV_OWN 0
#define MV_NOISE 1
#define MV_QUIET 2
#define MV_QUIET_OWN 3
template <bool RING, int MODE>
__device__ __forceinline__ void mv_cov_body(const float* __restrict__ pcm, const uint32_t* __restrict__ tables, float2* __restrict__ ws,
                                            TdArgs ta, MvArgs ma, const int* __restrict__ qsel = nullptr) {
    constexpr bool NOISE = MODE == MV_NOISE, PRE = MODE == MV_NOISE || MODE == MV_QUIET;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const long e = ta.e0 + blockIdx.y;
    int rec, len;
    long s0;
    mv_event(ta, ma, e, rec, s0, len);
    const int listed = MODE >= MV_QUIET ? mv_quiet_frames(ma, e) : 0;
    const bool noise = len != 0 && (MODE >= MV_QUIET ? listed > 0 : mv_uses_noise(ma, s0));
    if (NOISE && blockIdx.x == 0 && tid == 0) ma.noise_frames[e] = noise ? ma.kn : 0;
    if (len == 0 || noise != PRE) return;                        // (block-uniform: before any barrier)
    const int nfr = NOISE ? ma.kn : MODE == MV_QUIET ? listed : (len + MV_B - 1) / MV_B + 1;     // the frames before the onset, or frames 0 .. J
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
                else if (MODE == MV_QUIET) mv_load_quiet(z, pcm, ta, ma, rec, ch, s0, qsel[e * ma.kn + j], scr, fl);
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
    mv_cov_body<false, MV_OWN>(pcm, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_ring_cov_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                              float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<true, MV_OWN>(ring, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_noise_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                           float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<false, MV_NOISE>(pcm, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_ring_noise_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                                float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<true, MV_NOISE>(ring, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_quiet_own_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                               float2* __restrict__ ws, TdArgs ta, MvArgs ma) {
    mv_cov_body<false, MV_QUIET_OWN>(pcm, tables, ws, ta, ma);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_quiet_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                           float2* __restrict__ ws, TdArgs ta, MvArgs ma, const int* __restrict__ qsel) {
    mv_cov_body<false, MV_QUIET>(pcm, tables, ws, ta, ma, qsel);
}

// Every thread works in its own column of the three arrays: no thread reads what another writes, and there is no barrier.
// One text for two kernels (a macro, not a shared function: mvdr_weights_k must compile to what it was before its sibling
// existed, and with its body in an inlined function it does not).  FRAMES: the frames behind an extracted event's weights —
// mvdr_weights_k: its own 0 .. J, or the kn before its onset; mvdr_quiet_weights_k: those that
// mvdr_select_k listed for it.  The text is in five parts — the chunk sums and the trace, the steering vector, the silent bin, the
// loading and the Cholesky factor, the two solves and the store — which the tracked kernels put together with the
// steering vector, the silent bin and the solves inside a loop over the event's track blocks: one factor per (event, bin), a
// pair of solves per block.
#define MV_WB_SUM(FRAMES)                                                                                                                    \
    __shared__ double2 s_A[MV_MAX_TRI][MV_WT];                   /* the lower triangle of R + lambda I, then of its Cholesky factor */       \
    __shared__ double2 s_d[TD_MAX_CH][MV_WT];                                                                                                \
    __shared__ double2 s_v[TD_MAX_CH][MV_WT];                                                                                                \
    const int tid = threadIdx.x, k = blockIdx.x * MV_WT + tid;                                                                               \
    if (k > LM_N) return;                                                                                                                    \
    const long e = ta.e0 + blockIdx.y;                                                                                                       \
    int rec, len;                                                                                                                            \
    long s0;                                                                                                                                 \
    mv_event(ta, ma, e, rec, s0, len);                                                                                                       \
    if (len == 0) return;                                                                                                                    \
    const int C = ta.C, T = C * (C + 1) / 2;                                                                                                 \
    const int nfr = FRAMES, nch = (nfr + MV_CHUNK - 1) / MV_CHUNK;                                                                           \
    float2* wev = ws + (long)blockIdx.y * ma.rows * PHAT_SPEC;                                                                               \
    float2* wout = wev + (long)ma.cpe * T * PHAT_SPEC;           /* [C][PHAT_SPEC] */                                                        \
    _Pragma("unroll 1")                                                                                                                      \
    for (int t = 0; t < T; ++t) {                                                                                                            \
        float2 s = wev[(long)t * PHAT_SPEC + k];                                                                                             \
    _Pragma("unroll 1")                                                                                                                      \
        for (int c = 1; c < nch; ++c) {                          /* fp32, ascending chunks */                                                \
            const float2 p = wev[((long)c * T + t) * PHAT_SPEC + k];                                                                         \
            s.x += p.x; s.y += p.y;                                                                                                          \
        }                                                                                                                                    \
        s_A[t][tid] = make_double2((double)s.x, (double)s.y);                                                                                \
    }                                                                                                                                        \
    double trace = 0.0;                                                                                                                      \
    _Pragma("unroll 1")                                                                                                                      \
    for (int i = 0; i < C; ++i) trace += s_A[i * (i + 1) / 2 + i][tid].x;
#define MV_WB_STEER(DIR)                                                                                                                     \
    const double* trow = tau + (long)DIR * C;                    /* (0 <= dir < D: the event has samples) */                                 \
    _Pragma("unroll 1")                                                                                                                      \
    for (int c = 0; c < C; ++c) {                                                                                                            \
        double sn, cs;                                                                                                                       \
        sincospi((double)k * trow[c] * (1.0 / MV_B), &sn, &cs);  /* 2 pi k tau / 2048 */                                                     \
        s_d[c][tid] = make_double2(cs, sn);                                                                                                  \
    }
#define MV_WB_SILENT(EXIT)                                                                                                                   \
    if (!(trace > 0.0)) {                                        /* digital silence (or NaN samples): the plain average */                   \
    _Pragma("unroll 1")                                                                                                                      \
        for (int c = 0; c < C; ++c) wout[(long)c * PHAT_SPEC + k] = make_float2((float)(s_d[c][tid].x / C), (float)(s_d[c][tid].y / C));     \
        EXIT;                                                                                                                                \
    }
#define MV_WB_CHOL                                                                                                                           \
    const double lambda = loading * trace / C;                                                                                               \
    _Pragma("unroll 1")                                                                                                                      \
    for (int i = 0; i < C; ++i) {                                                                                                            \
        double2 a = s_A[i * (i + 1) / 2 + i][tid];                                                                                           \
        s_A[i * (i + 1) / 2 + i][tid] = make_double2(a.x + lambda, 0.0);                                                                     \
    }                                                                                                                                        \
    /* ── Cholesky, in place: L[i][j], j <= i, at i (i + 1) / 2 + j; the diagonal holds 1 / L[j][j] in .y ── */                              \
    _Pragma("unroll 1")                                                                                                                      \
    for (int j = 0; j < C; ++j) {                                                                                                            \
        const int rj = j * (j + 1) / 2;                                                                                                      \
        double s = s_A[rj + j][tid].x;                                                                                                       \
    _Pragma("unroll 1")                                                                                                                      \
        for (int p = 0; p < j; ++p) { const double2 l = s_A[rj + p][tid]; s -= l.x * l.x + l.y * l.y; }                                      \
        const double ljj = sqrt(s), inv = 1.0 / ljj;                                                                                         \
        s_A[rj + j][tid] = make_double2(ljj, inv);                                                                                           \
    _Pragma("unroll 1")                                                                                                                      \
        for (int i = j + 1; i < C; ++i) {                                                                                                    \
            const int ri = i * (i + 1) / 2;                                                                                                  \
            double2 a = s_A[ri + j][tid];                                                                                                    \
    _Pragma("unroll 1")                                                                                                                      \
            for (int p = 0; p < j; ++p) {                        /* a -= L[i][p] conj L[j][p] */                                             \
                const double2 li = s_A[ri + p][tid], lj = s_A[rj + p][tid];                                                                  \
                a.x -= li.x * lj.x + li.y * lj.y;                                                                                            \
                a.y -= li.y * lj.x - li.x * lj.y;                                                                                            \
            }                                                                                                                                \
            s_A[ri + j][tid] = make_double2(a.x * inv, a.y * inv);                                                                           \
        }                                                                                                                                    \
    }
#define MV_WB_SOLVE                                                                                                                          \
    /* ── L y = d, then L^H v = y ── */                                                                                                      \
    _Pragma("unroll 1")                                                                                                                      \
    for (int i = 0; i < C; ++i) {                                                                                                            \
        const int ri = i * (i + 1) / 2;                                                                                                      \
        double2 y = s_d[i][tid];                                                                                                             \
    _Pragma("unroll 1")                                                                                                                      \
        for (int p = 0; p < i; ++p) {                                                                                                        \
            const double2 l = s_A[ri + p][tid], v = s_v[p][tid];                                                                             \
            y.x -= l.x * v.x - l.y * v.y;                                                                                                    \
            y.y -= l.x * v.y + l.y * v.x;                                                                                                    \
        }                                                                                                                                    \
        const double inv = s_A[ri + i][tid].y;                                                                                               \
        s_v[i][tid] = make_double2(y.x * inv, y.y * inv);                                                                                    \
    }                                                                                                                                        \
    _Pragma("unroll 1")                                                                                                                      \
    for (int i = C - 1; i >= 0; --i) {                                                                                                       \
        double2 y = s_v[i][tid];                                                                                                             \
    _Pragma("unroll 1")                                                                                                                      \
        for (int p = i + 1; p < C; ++p) {                        /* y -= conj L[p][i] v[p] */                                                \
            const double2 l = s_A[p * (p + 1) / 2 + i][tid], v = s_v[p][tid];                                                                \
            y.x -= l.x * v.x + l.y * v.y;                                                                                                    \
            y.y -= l.x * v.y - l.y * v.x;                                                                                                    \
        }                                                                                                                                    \
        const double inv = s_A[i * (i + 1) / 2 + i][tid].y;                                                                                  \
        s_v[i][tid] = make_double2(y.x * inv, y.y * inv);                                                                                    \
    }                                                                                                                                        \
    double den = 0.0;                                            /* d^H v = d^H (R + lambda I)^-1 d: real and positive */                    \
    _Pragma("unroll 1")                                                                                                                      \
    for (int c = 0; c < C; ++c) den += s_d[c][tid].x * s_v[c][tid].x + s_d[c][tid].y * s_v[c][tid].y;                                        \
    const double scale = 1.0 / den;                                                                                                          \
    _Pragma("unroll 1")                                                                                                                      \
    for (int c = 0; c < C; ++c) wout[(long)c * PHAT_SPEC + k] = make_float2((float)(s_v[c][tid].x * scale), (float)(s_v[c][tid].y * scale));

#define MV_WEIGHTS_BODY(FRAMES) MV_WB_SUM(FRAMES) MV_WB_STEER(ma.ev_dir[e]) MV_WB_SILENT(return) MV_WB_CHOL MV_WB_SOLVE

__global__ __launch_bounds__(MV_WT) void mvdr_weights_k(float2* __restrict__ ws, const double* __restrict__ tau, double loading,
                                                        TdArgs ta, MvArgs ma) {
    MV_WEIGHTS_BODY(mv_uses_noise(ma, s0) ? ma.kn : (len + MV_B - 1) / MV_B + 1)
}

__global__ __launch_bounds__(MV_WT) void mvdr_quiet_weights_k(float2* __restrict__ ws, const double* __restrict__ tau, double loading,
                                                              TdArgs ta, MvArgs ma) {
    MV_WEIGHTS_BODY(mv_quiet_frames(ma, e) > 0 ? mv_quiet_frames(ma, e) : (len + MV_B - 1) / MV_B + 1)
}

// ───────────────────────── DESIGN 5y: the beam steered along the event's direction track ─────────────────────────
// The track of sed_event_doa_track: trk_len [E] blocks of 32 W located frames an event, their directions in trk_dir [E][Tm].  An
// event's workspace rows are then cpe x C(C+1)/2 partials and C rows of w for each of Tm blocks, block b's behind block b - 1's.
struct MvTrack {
    const int *len, *dir;                        // [E], [E][Tm]
    int W, Tm;                                   // block_chunks; the columns of dir
};

// the blocks of event e that the rule reads: trk_len clamped to [0, Tm]
__device__ __forceinline__ int mv_trk_blocks(const MvTrack& tk, long e) {
    const int T = tk.len[e];
    return T < 0 ? 0 : T > tk.Tm ? tk.Tm : T;
}

// THE RULE, device side (localize.mvdr_frame_blocks; tests/mvdr_track_ref.py): the centre of frame j is sample j B of the event,
// which lies in located frame j B / hop, and that in track block (j B / hop) / (32 W); frame J and the short tail that joins the
// last block take block T - 1.  T = 0: block 0, whose weights are steered at dir
__device__ __forceinline__ int mv_trk_frame_block(const MvTrack& tk, int hop, int T, int j) {
    const unsigned b = ((unsigned)j * MV_B / (unsigned)hop) / (unsigned)(TD_CHUNK * tk.W);     // (j B < len + B < 2^32: mv_sizes_ok)
    return T < 1 ? 0 : b < (unsigned)(T - 1) ? (int)b : T - 1;
}

// the direction block b < max(T, 1) is steered at: its row of the track where that names a direction, else the event's dir — a
// silent block (-1), an event without a track (T = 0) and a row outside [0, D) never index tau
__device__ __forceinline__ int mv_trk_dir(const MvArgs& ma, const MvTrack& tk, long e, int T, int b) {
    int d = ma.ev_dir[e];
    if (T > 0) {
        const int t = tk.dir[e * tk.Tm + b];
        if (t >= 0 && t < ma.D) d = t;
    }
    return d;
}

// mvdr_trk_weights_k / mvdr_trk_quiet_weights_k: the parts of the weight body with ONE factor per (event, bin) and the steering
// vector, the two solves and the normalisation once per block — the float64 expressions of mvdr_weights_k in their order, so that a
// block steered at dir holds mvdr_weights_k's bits.  A silent bin (trace not > 0) gets d_b / C in every block.
#define MV_TRK_WEIGHTS_BODY(FRAMES)                                                                                                          \
    MV_WB_SUM(FRAMES)                                                                                                                        \
    const int nblk = mv_trk_blocks(tk, e);                                                                                                   \
    if (trace > 0.0) { MV_WB_CHOL }                                                                                                          \
    _Pragma("unroll 1")                                                                                                                      \
    for (int b = 0; b < (nblk > 1 ? nblk : 1); ++b, wout += (long)C * PHAT_SPEC) {                                                           \
        MV_WB_STEER(mv_trk_dir(ma, tk, e, nblk, b))                                                                                          \
        MV_WB_SILENT(continue)                                                                                                               \
        MV_WB_SOLVE                                                                                                                          \
    }

__global__ __launch_bounds__(MV_WT) void mvdr_trk_weights_k(float2* __restrict__ ws, const double* __restrict__ tau, double loading,
                                                            TdArgs ta, MvArgs ma, MvTrack tk) {
    MV_TRK_WEIGHTS_BODY(mv_uses_noise(ma, s0) ? ma.kn : (len + MV_B - 1) / MV_B + 1)
}

__global__ __launch_bounds__(MV_WT) void mvdr_trk_quiet_weights_k(float2* __restrict__ ws, const double* __restrict__ tau, double loading,
                                                                  TdArgs ta, MvArgs ma, MvTrack tk) {
    MV_TRK_WEIGHTS_BODY(mv_quiet_frames(ma, e) > 0 ? mv_quiet_frames(ma, e) : (len + MV_B - 1) / MV_B + 1)
}

// TRK (mvdr_trk_apply_k, mvdr_trk_ring_apply_k): frame j is combined with the weights of its track block, the rows at
// wts + b_j C PHAT_SPEC; nothing else differs, and the sqrt-Hann overlap-add cross-fades from one block's beam to the next
template <bool RING, bool TRK = false>
__device__ __forceinline__ void mv_apply_body(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                              const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta, MvArgs ma,
                                              MvTrack tk = MvTrack{}) {
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
    const int nblk = TRK ? mv_trk_blocks(tk, e) : 0;             // the event's track blocks
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
            const float2* wj = wts;
            if (TRK) wj += (long)mv_trk_frame_block(tk, ta.hop, nblk, j) * C * PHAT_SPEC;
            for (int k = tid; k <= LM_N; k += MV_THREADS) {
                float2 y = make_float2(0.f, 0.f);
                for (int c = 0; c < C; ++c) {                    // conj(w) x, ascending c
                    const float2 w = wj[(long)c * PHAT_SPEC + k], x = s_spec[c * PHAT_SPEC + k];
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

__global__ __launch_bounds__(MV_THREADS) void mvdr_trk_apply_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                               const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta, MvArgs ma,
                                                               MvTrack tk) {
    mv_apply_body<false, true>(pcm, tables, ws, audio, ta, ma, tk);
}

__global__ __launch_bounds__(MV_THREADS) void mvdr_trk_ring_apply_k(const float* __restrict__ ring, const uint32_t* __restrict__ tables,
                                                                    const float2* __restrict__ ws, float* __restrict__ audio, TdArgs ta,
                                                                    MvArgs ma, MvTrack tk) {
    mv_apply_body<true, true>(ring, tables, ws, audio, ta, ma, tk);
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
// ... with the weights of Tm track blocks behind the partials
size_t mv_trk_event_bytes(int C, long cpe, int Tm) { return ((size_t)cpe * (C * (C + 1) / 2) + (size_t)C * Tm) * TD_ROW_BYTES; }
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
#define MV_MAX_TRK_W 64                           // localize.DirectionTrack: block_chunks (doatrack.hip: TRK_MAX_W)
#define MV_MAX_TRK_BLOCKS 256                     //                          the blocks of an event (doatrack.hip: TRK_MAX_BLOCKS)
bool mv_trk_sizes_ok(int Tm) { return Tm >= 1 && Tm <= MV_MAX_TRK_BLOCKS; }

// ───────────────────────── DESIGN 5w: the noise frames where the event's class is silent ─────────────────────────
#define MV_MAX_SEARCH 1024                        // localize.MVDR: noise_search
#define MV_MAX_CLASSES 32                         // the bits of a mask word

static_assert(MV_MAX_NOISE <= ACT_MAX_SEL, "act_select_walk keeps at most ACT_MAX_SEL entries");

struct MqArgs {
    ActMask act;                                 // the event classes, the rows of the whole table and the activity mask
    int search, min_frames, any;                 // S candidates, at least M of them, and whether every class excludes (else the event's own)
    int* sel;                                    // [E][kn] the candidates of every event in summation order, -1 behind them
};

// candidate q: the 2048 samples from s0 - (G + 2 + q) B, which exist when that is >= 0, tested on [s0 - (2 G + 2 + q) B, s0 - q B)
__global__ __launch_bounds__(64) void mvdr_select_k(TdArgs ta, MvArgs ma, MqArgs qa) {
    for (long e = blockIdx.x; e < qa.act.E; e += gridDim.x) {
        int rec, len;
        long s0;
        bm_event_span(ta, ma.ev_dir, ma.ev_loc, ma.D, e, rec, s0, len);
        const int cls = qa.act.ev_cls[e];
        const bool takes = len != 0 && cls >= 0 && cls < qa.act.n_classes;           // (block-uniform)
        const ActWindow w{s0, MV_B, (long)(2 * ma.guard + 2) * MV_B, 0, (long)(ma.guard + 2) * MV_B};
        act_select_walk(ta, qa.act, takes, rec, qa.any ? 0xffffffffu : takes ? 1u << cls : 0u, w, ma.kn, qa.search, qa.min_frames,
                        qa.sel + e * ma.kn, ma.noise_frames + e);
    }
}

bool mq_sizes_ok(int R, long frames, int kn) { return act_mask_ok(R, frames) && kn >= 1 && kn <= MV_MAX_NOISE; }

// the settings of a quiet call and its outputs beside frames_out (MvNoise)
struct MvQuiet { const int* cls; int n_classes, search, min_frames, any; int* sel_out; };

int mq_check(const char* who, const EvTable& ev, int kn, int guard, const int* frames_out, const MvQuiet& qz) {
    SED_REQUIRE(kn >= 1 && kn <= MV_MAX_NOISE, "%s: noise_blocks must be in [1, %d], got %d", who, MV_MAX_NOISE, kn);
    SED_REQUIRE(guard >= 0 && guard <= MV_MAX_GUARD, "%s: noise_guard must be in [0, %d], got %d", who, MV_MAX_GUARD, guard);
    SED_REQUIRE(qz.search >= kn && qz.search <= MV_MAX_SEARCH, "%s: noise_search must be in [noise_blocks = %d, %d], got %d", who, kn,
                MV_MAX_SEARCH, qz.search);
    SED_REQUIRE(qz.min_frames >= 1 && qz.min_frames <= kn, "%s: noise_min must be in [1, noise_blocks = %d], got %d", who, kn, qz.min_frames);
    SED_REQUIRE(qz.n_classes >= 1 && qz.n_classes <= MV_MAX_CLASSES, "%s: n_classes must be in [1, %d], got %d", who, MV_MAX_CLASSES,
                qz.n_classes);
    SED_REQUIRE(qz.any == 0 || qz.any == 1, "%s: exclude_any must be 0 or 1, got %d", who, qz.any);
    SED_REQUIRE(ev.E == 0 || (qz.cls && frames_out && qz.sel_out), "%s: null pointer (ev_cls, noise_frames_out or noise_sel_out)", who);
    return 0;
}

// the activity of the whole table into the mask behind the recording table (which is uploaded), then every event's frames:
// frames_out [E] and sel_out [E][kn] are written for all E rows.  The workspace holds src.tab + act_mask_bytes (checked by the caller).
int mq_select(const char* who, const RecSource& src, const EvTable& ev, int kn, int guard, int* frames_out, const MvQuiet& qz,
              void* workspace, hipStream_t s) {
    MvArgs ma{};
    ma.ev_dir = ev.dir; ma.ev_loc = ev.loc; ma.D = ev.D; ma.kn = kn; ma.guard = guard; ma.noise_frames = frames_out;
    MqArgs qa{{}, qz.search, qz.min_frames, qz.any, qz.sel_out};
    SED_TRY(act_mask_build(who, "mvdr (activity)", src, ev, qz.cls, qz.n_classes, workspace, s, &qa.act));
    const long cap = 1L << 20;
    mvdr_select_k<<<(unsigned)(ev.E < cap ? ev.E : cap), 64, 0, s>>>(td_args(src, ev, workspace), ma, qa);
    SED_LAUNCH_CHECK("mvdr (selection)");
    return 0;
}

// the steering delays [D][C], the diagonal loading and the table blob
struct MvTables { const double* tau; double loading; const void* tables; size_t tables_bytes; };
// kn noise frames that end guard blocks before the onset, and which events used them; entry: one of the noise entries,
// which must be given frames_out
struct MvNoise { int kn, guard; int* frames_out; bool entry; };
// the track of a track entry — W = block_chunks, Tm = track_slots, trk_len [E], trk_dir [E][Tm]
struct MvTrackIn { int W, Tm; const int *len, *dir; };

// what all entries do once the events and the recordings are checked.  kn = 0 (sed_event_mvdr, sed_event_mvdr_ring, or a noise
// entry asked for no noise frames): three launches per slice, and the noise entries' frames_out is zeroed
// qz (sed_event_mvdr_quiet; linear only): the mask lies between the table and the partials, the selection runs once over
// the whole table, and a slice is own covariance, quiet covariance, weights, apply with the quiet kernels
// trk (the track entries): the covariance launches as they are, then the tracked weight and apply kernels on rows of
// Tm weight sets an event; without it exactly the launches above
template <bool RING>
int mv_run(const char* who, const RecSource& src, const EvTable& ev, const MvTables& mt, const MvNoise& nz, const BeamOut& out,
           void* workspace, size_t workspace_bytes, void* stream, const MvQuiet* qz = nullptr, const MvTrackIn* trk = nullptr) {
    const int kn = nz.kn;
    const long E = ev.E;
    if (qz) SED_TRY(mq_check(who, ev, kn, nz.guard, nz.frames_out, *qz));
    const size_t tab = src.tab + (qz ? act_mask_bytes(src.R, act_mask_frames(src, ev)) : 0);
    SED_REQUIRE(kn >= 0 && kn <= MV_MAX_NOISE, "%s: noise_blocks must be in [0, %d], got %d", who, MV_MAX_NOISE, kn);
    SED_REQUIRE(nz.guard >= 0 && nz.guard <= MV_MAX_GUARD, "%s: noise_guard must be in [0, %d], got %d", who, MV_MAX_GUARD, nz.guard);
    SED_REQUIRE(!nz.entry || E == 0 || nz.frames_out, "%s: null pointer (noise_frames_out)", who);
    if (trk) {
        SED_REQUIRE(trk->W >= 1 && trk->W <= MV_MAX_TRK_W, "%s: block_chunks must be in [1, %d], got %d", who, MV_MAX_TRK_W, trk->W);
        SED_REQUIRE(mv_trk_sizes_ok(trk->Tm), "%s: track_slots must be in [1, %d], got %d", who, MV_MAX_TRK_BLOCKS, trk->Tm);
        SED_REQUIRE(E == 0 || (trk->len && trk->dir), "%s: null pointer (trk_len or trk_dir)", who);
    }
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
    const size_t per_event = trk ? mv_trk_event_bytes(C, cpe, trk->Tm) : mv_event_bytes(C, cpe);
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
    if (qz) SED_TRY(mq_select(who, src, ev, kn, nz.guard, nz.frames_out, *qz, workspace, s));
    const auto cov_k = RING ? mvdr_ring_cov_k : qz ? mvdr_quiet_own_k : mvdr_cov_k;
    const auto apply_k = RING ? mvdr_ring_apply_k : mvdr_apply_k;
    const auto trk_apply_k = RING ? mvdr_trk_ring_apply_k : mvdr_trk_apply_k;
    hipError_t err = hipFuncSetAttribute((const void*)cov_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    if (err == hipSuccess) err = hipFuncSetAttribute(trk ? (const void*)trk_apply_k : (const void*)apply_k,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    const auto noise_k = RING ? mvdr_ring_noise_k : mvdr_noise_k;
    if (err == hipSuccess && kn > 0) err = hipFuncSetAttribute((const void*)noise_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    if (err == hipSuccess && qz) err = hipFuncSetAttribute((const void*)mvdr_quiet_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MV_LDS_MAX);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    if (kn == 0 && nz.frames_out) {
        err = hipMemsetAsync(nz.frames_out, 0, (size_t)E * sizeof(int), s);
        if (err != hipSuccess) { sed_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(err)); return (int)err; }
    }
    TdArgs ta = td_args(src, ev, workspace);
    const MvArgs ma{ev.dir, ev.loc, ev.D, out.audio_len, out.audio_start, out.total, (int)cpe, (int)(cpe * T + C * (trk ? trk->Tm : 1)), batch,
                    kn, nz.guard, nz.frames_out};
    const MvTrack tk = trk ? MvTrack{trk->len, trk->dir, trk->W, trk->Tm} : MvTrack{};
    const uint32_t* tables = (const uint32_t*)mt.tables;
    float2* part = (float2*)((char*)workspace + tab);
    for (long e0 = 0; e0 < E; e0 += slice) {
        ta.e0 = e0;
        ta.n_ev = (int)(E - e0 < slice ? E - e0 : slice);
        cov_k<<<dim3(chunks, (unsigned)ta.n_ev), MV_THREADS, lds_cov, s>>>(src.x, tables, part, ta, ma);
        SED_LAUNCH_CHECK("mvdr (covariance)");
        if (qz) {
            mvdr_quiet_k<<<dim3((unsigned)mv_noise_chunks(kn), (unsigned)ta.n_ev), MV_THREADS, lds_cov, s>>>(src.x, tables, part, ta, ma, qz->sel_out);
            SED_LAUNCH_CHECK("mvdr (quiet covariance)");
        } else if (kn > 0) {                                     // the host does not know which events use it: both launches run
            noise_k<<<dim3((unsigned)mv_noise_chunks(kn), (unsigned)ta.n_ev), MV_THREADS, lds_cov, s>>>(src.x, tables, part, ta, ma);
            SED_LAUNCH_CHECK("mvdr (noise covariance)");
        }
        if (trk) {
            (qz ? mvdr_trk_quiet_weights_k : mvdr_trk_weights_k)<<<dim3((LM_N + MV_WT) / MV_WT, (unsigned)ta.n_ev), MV_WT, 0, s>>>(
                part, mt.tau, mt.loading, ta, ma, tk);
            SED_LAUNCH_CHECK("mvdr (tracked weights)");
            trk_apply_k<<<dim3(runs, (unsigned)ta.n_ev), MV_THREADS, lds_apply, s>>>(src.x, tables, part, out.audio, ta, ma, tk);
            SED_LAUNCH_CHECK("mvdr (tracked apply)");
            continue;
        }
        (qz ? mvdr_quiet_weights_k : mvdr_weights_k)<<<dim3((LM_N + MV_WT) / MV_WT, (unsigned)ta.n_ev), MV_WT, 0, s>>>(part, mt.tau, mt.loading, ta, ma);
        SED_LAUNCH_CHECK("mvdr (weights)");
        apply_k<<<dim3(runs, (unsigned)ta.n_ev), MV_THREADS, lds_apply, s>>>(src.x, tables, part, out.audio, ta, ma);
        SED_LAUNCH_CHECK("mvdr (apply)");
    }
    return 0;
}

// an entry: the events and the recordings checked, then the launches
template <bool RING>
int mv_entry(const char* who, RecSource src, const EvTable& ev, const MvTables& mt, const MvNoise& nz, const BeamOut& out, void* workspace,
             size_t workspace_bytes, void* stream, const MvQuiet* qz = nullptr, const MvTrackIn* trk = nullptr) {
    SED_TRY(beam_source<RING>(who, src, ev));
    return mv_run<RING>(who, src, ev, mt, nz, out, workspace, workspace_bytes, stream, qz, trk);
}

// sed_event_quiet_frames: the activity and the selection alone; no sample is read
int mq_frames_entry(const char* who, RecSource src, const EvTable& ev, int kn, int guard, int* frames_out, const MvQuiet& qz, void* workspace,
                    size_t workspace_bytes, void* stream) {
    SED_TRY((beam_source<false, false>(who, src, ev)));
    SED_TRY(mq_check(who, ev, kn, guard, frames_out, qz));
    if (ev.E == 0) return 0;
    const size_t need = src.tab + act_mask_bytes(src.R, act_mask_frames(src, ev));
    SED_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device buffer", who);
    SED_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    SED_TRY(rec_upload(who, src, workspace, s));
    return mq_select(who, src, ev, kn, guard, frames_out, qz, workspace, s);
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

// ── DESIGN 5w: the noise covariance from the frames where the event's class — or, with exclude_any, every class — is silent ──
extern "C" size_t sed_event_quiet_frames_workspace_bytes(int R, int channels, long mask_frames, int noise_blocks) {
    if (R < 1 || channels < 2 || channels > TD_MAX_CH || !mq_sizes_ok(R, mask_frames, noise_blocks)) return 0;
    return rec_table_bytes(R, channels) + act_mask_bytes(R, mask_frames);
}

extern "C" size_t sed_event_mvdr_quiet_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, long mask_frames) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || !mq_sizes_ok(R, mask_frames, noise_blocks)) return 0;
    return rec_table_bytes(R, channels) + act_mask_bytes(R, mask_frames) + mv_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks));
}

extern "C" int sed_event_quiet_frames(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_cls,
                                      const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                                      const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, int D, int n_classes,
                                      int noise_blocks, int noise_guard, int noise_search, int noise_min, int exclude_any,
                                      int* noise_frames_out, int* noise_sel_out, void* workspace, size_t workspace_bytes, void* stream) {
    return mq_frames_entry("quiet_frames", {nullptr, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           noise_blocks, noise_guard, noise_frames_out, {ev_cls, n_classes, noise_search, noise_min, exclude_any, noise_sel_out},
                           workspace, workspace_bytes, stream);
}

extern "C" int sed_event_mvdr_quiet(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                                    const int* ev_cls, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                                    const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                                    const double* tau, int D, double loading, int noise_blocks, int noise_guard, int n_classes,
                                    int noise_search, int noise_min, int exclude_any, const void* tables, size_t tables_bytes,
                                    const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                                    int* noise_sel_out, void* workspace, size_t workspace_bytes, void* stream) {
    const MvQuiet qz{ev_cls, n_classes, noise_search, noise_min, exclude_any, noise_sel_out};
    return mv_entry<false>("mvdr_quiet", {pcm, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                           {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream, &qz);
}

// ── DESIGN 5y: the beam steered along the event's direction track; noise_blocks = 0 is the own-frames form ──
extern "C" size_t sed_event_mvdr_track_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, int track_slots) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || noise_blocks < 0 || noise_blocks > MV_MAX_NOISE || !mv_trk_sizes_ok(track_slots)) return 0;
    return rec_table_bytes(R, channels) + mv_trk_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks), track_slots);
}

extern "C" size_t sed_event_mvdr_track_ring_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, int track_slots) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || noise_blocks < 0 || noise_blocks > MV_MAX_NOISE || !mv_trk_sizes_ok(track_slots)) return 0;
    return rec_ring_table_bytes(R) + mv_trk_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks), track_slots);
}

extern "C" size_t sed_event_mvdr_quiet_track_workspace_bytes(int R, int channels, int max_frames, int hop, int noise_blocks, long mask_frames,
                                                             int track_slots) {
    if (!mv_sizes_ok(R, channels, max_frames, hop) || !mq_sizes_ok(R, mask_frames, noise_blocks) || !mv_trk_sizes_ok(track_slots)) return 0;
    return rec_table_bytes(R, channels) + act_mask_bytes(R, mask_frames) +
           mv_trk_event_bytes(channels, mv_slots(max_frames, hop, noise_blocks), track_slots);
}

extern "C" int sed_event_mvdr_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                                    const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                                    const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const double* tau, int D,
                                    double loading, int noise_blocks, int noise_guard, const void* tables, size_t tables_bytes,
                                    const int* audio_len, const long* audio_start, float* audio, long audio_total, int* noise_frames_out,
                                    int block_chunks, int track_slots, const int* trk_len, const int* trk_dir, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const MvTrackIn trk{block_chunks, track_slots, trk_len, trk_dir};
    return mv_entry<false>("mvdr_track", {pcm, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                           {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream, nullptr, &trk);
}

extern "C" int sed_event_mvdr_track_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                         const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                                         const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                                         const double* tau, int D, double loading, int noise_blocks, int noise_guard, const void* tables,
                                         size_t tables_bytes, const int* audio_len, const long* audio_start, float* audio,
                                         long audio_total, int* noise_frames_out, int block_chunks, int track_slots, const int* trk_len,
                                         const int* trk_dir, void* workspace, size_t workspace_bytes, void* stream) {
    const MvTrackIn trk{block_chunks, track_slots, trk_len, trk_dir};
    return mv_entry<true>("mvdr_track_ring", {ring, true, cap, ring_len, R, channels, n_host},
                          {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                          {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                          {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream, nullptr, &trk);
}

extern "C" int sed_event_mvdr_quiet_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                                          const int* ev_cls, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                                          const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                                          const double* tau, int D, double loading, int noise_blocks, int noise_guard, int n_classes,
                                          int noise_search, int noise_min, int exclude_any, const void* tables, size_t tables_bytes,
                                          const int* audio_len, const long* audio_start, float* audio, long audio_total,
                                          int* noise_frames_out, int* noise_sel_out, int block_chunks, int track_slots, const int* trk_len,
                                          const int* trk_dir, void* workspace, size_t workspace_bytes, void* stream) {
    const MvQuiet qz{ev_cls, n_classes, noise_search, noise_min, exclude_any, noise_sel_out};
    const MvTrackIn trk{block_chunks, track_slots, trk_len, trk_dir};
    return mv_entry<false>("mvdr_quiet_track", {pcm, false, 0, pcm_len, R, channels, clips_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                           {tau, loading, tables, tables_bytes}, {noise_blocks, noise_guard, noise_frames_out, true},
                           {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream, &qz, &trk);
}
