// tdoa_accum.h — the body of an accumulate launch, once, for the kernels that promise each other's bits: tdoa_accum_k (tdoa.hip,
// DESIGN 5o/5p), which sums the whitened cross spectra of a chunk of an event's located frames, and contrast_accum_k
// (contrast.hip), which sums those of a chunk of the event's background frames.  The two differ in which feature frame
// a step of the chunk is and in the workspace row the partial goes to: everything between the loads and the stores is one text,
// so that a frame gives the same Pk wherever it is summed.  With it the sizes that belong to that text: the workgroup, its LDS
// and the chunk slots of an event.
#pragma once
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"

#define TD_WAVES 8
#define TD_THREADS (TD_WAVES * 64)
#define TD_TAB_WORDS LM_OFF_ENT                   // of the log-mel blob: header, window, inter-pass and pairing twiddles
#define TD_FFT_SCR (2 * LM_SCR)                   // floats of exchange scratch per transforming wave
#define TD_LDS_MAX ((size_t)160 * 1024)

namespace {

// One workgroup of TD_THREADS, one chunk: the n_fr <= TD_CHUNK frames frame_of(0 .. n_fr - 1) of recording `rec`, every pair's
// sum in ascending step order into the P rows at `wrow`.  frame_of is called for steps < n_fr only.
// RING: the channels are rings (TdArgs.cap); a frame that does not wrap takes the same 8-byte loads, one that does goes through
// the guarded loads, and either way the registers hold the same samples: everything after the loads is one code.
template <bool RING, typename FrameOf>
__device__ __forceinline__ void td_accum_chunk(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                               float2* __restrict__ wrow, int pad_mode, const TdArgs& ta, int rec, int n_fr,
                                               FrameOf frame_of) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    fft_stage_tables(lds, tables, TD_TAB_WORDS, tid, TD_THREADS);
    const f2* s_win = reinterpret_cast<const f2*>(lds + LM_OFF_WIN);
    const f2* s_tw = reinterpret_cast<const f2*>(lds + LM_OFF_TW);
    const f2* s_pw = reinterpret_cast<const f2*>(lds + LM_OFF_PW);
    const int C = ta.C, P = ta.P;
    const int nfw = (C + 1) >> 1;                                // waves that transform
    const bool pipe = ta.pipelined != 0;
    float2* s_spec = reinterpret_cast<float2*>(lds + TD_TAB_WORDS);                              // [1 or 2][C][PHAT_SPEC]
    float* s_scr = lds + TD_TAB_WORDS + (pipe ? 2 : 1) * C * PHAT_SPEC * 2;                      // [nfw][TD_FFT_SCR]
    float2* s_acc = reinterpret_cast<float2*>(s_scr + nfw * TD_FFT_SCR);                         // [batch][PHAT_SPEC]

    const int wave = tid >> 6;
    float* wscr = s_scr + (wave < nfw ? wave : 0) * TD_FFT_SCR;  // (only used by waves < nfw)
    const FftLane fl = fft_lane(tid & 63, wscr - lds);
    const int half = fl.half(), r = fl.r();
    float* scr = wscr + half * LM_SCR;
    const long ns = ta.n_samples[rec];
    // Pipelined (the spectra fit twice, C <= 4): in step s the transforming waves fill buffer s & 1 with frame s while the other
    // waves whiten frame s - 1 from the other buffer; one barrier per step.  Otherwise every wave whitens, between two barriers.
    // Either way an accumulator entry belongs to one lane and receives the frames in ascending order: the same sums.
    const int wt0 = pipe ? nfw * 64 : 0, wstride = TD_THREADS - wt0;

    for (int p0 = 0; p0 < P; p0 += ta.pairs_per_batch) {
        const int nb = (P - p0 < ta.pairs_per_batch) ? P - p0 : ta.pairs_per_batch;
        for (int idx = tid; idx < nb * PHAT_SPEC; idx += TD_THREADS) s_acc[idx] = make_float2(0.f, 0.f);
        __syncthreads();                                         // the tables are in LDS (first batch); the spectra are free
        for (int step = 0; step < n_fr + (pipe ? 1 : 0); ++step) {
            if (wave < nfw && step < n_fr) {
                const long frame = frame_of(step);
                // ── the frame of channel 2 wave + half (an odd C: the last half wave repeats channel C-1 and stores the same values) ──
                const int ch = (2 * wave + half < C) ? 2 * wave + half : C - 1;
                const float* cpcm = pcm + (RING ? ((long)rec * C + ch) * ta.cap : ta.sample_off[(long)rec * C + ch]);
                const long start = frame * ta.hop - LM_NFFT / 2;
                // RING: sample i lives at i % cap while max(0, ns - cap) <= i < ns; `pos` is the frame's first sample in the ring
                const long kept = RING && ns > ta.cap ? ns - ta.cap : 0;
                long pos = 0;
                if (RING) { pos = start % ta.cap; if (pos < 0) pos += ta.cap; }
                const bool fast = (ta.hop & 1) == 0 && (reinterpret_cast<uintptr_t>(cpcm) & 7) == 0 && start >= kept && start + LM_NFFT <= ns &&
                                  (!RING || pos + LM_NFFT <= ta.cap);
                auto sample = [&](int off) -> float {            // sample start + off of the channel, 0 <= off < 2048
                    if (!RING) return pcm_at(cpcm, start + off, ns, pad_mode);
                    const long i = start + off, p = pos + off;   // (cap >= 2048: p < 2 cap)
                    return i >= kept && i < ns ? cpcm[p >= ta.cap ? p - ta.cap : p] : 0.f;
                };
                f2 z[32];                                        // z[n] = (x[2n], x[2n+1]): one complex point per VGPR pair
                if (__all(fast)) {
                    const f2* src = reinterpret_cast<const f2*>(cpcm + (RING ? pos : start)) + r;
#pragma unroll
                    for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
                } else {                                         // edge frames / odd hop / unaligned clips / a frame that wraps
                    fft_load_guarded(z, scr, fl, sample);
                }
                fft2048_passes(z, fl, s_win, s_tw);
                fft2048_spectrum(z, fl, s_pw, s_spec + ((pipe ? (step & 1) : 0) * C + ch) * PHAT_SPEC);
            }
            if (!pipe) __syncthreads();
            // ── Pk of the batch's pairs, added to the accumulators.  Entry idx is read and written by this lane alone, frame
            //    after frame. ──
            const int wf = pipe ? step - 1 : step;               // the frame of the chunk whose spectra are whitened now
            const float2* wspec = s_spec + (pipe ? (wf & 1) : 0) * C * PHAT_SPEC;
            for (int idx = wf >= 0 && tid >= wt0 ? tid - wt0 : nb * 1025; idx < nb * 1025; idx += wstride) {
                const int pb = idx / 1025, k = idx - pb * 1025;
                int i, j;
                phat_pair(p0 + pb, C, i, j);
                const float2 pk = phat_bin(wspec[i * PHAT_SPEC + k], wspec[j * PHAT_SPEC + k], k);
                float2 s = s_acc[pb * PHAT_SPEC + k];
                s.x += pk.x; s.y += pk.y;
                s_acc[pb * PHAT_SPEC + k] = s;
            }
            __syncthreads();                                     // the spectra (of this buffer) may be overwritten
        }
        for (int idx = tid; idx < nb * 1025; idx += TD_THREADS) {
            const int pb = idx / 1025, k = idx - pb * 1025;
            wrow[(long)(p0 + pb) * PHAT_SPEC + k] = s_acc[pb * PHAT_SPEC + k];
        }
        __syncthreads();                                         // the accumulators are zeroed for the next batch
    }
}

// LDS of an accumulate kernel for C channels with `batch` pairs of accumulators resident and 1 or 2 spectra buffers
inline size_t tdoa_lds_bytes(int C, int batch, int buffers) {
    return ((size_t)TD_TAB_WORDS + (size_t)buffers * C * PHAT_SPEC * 2 + (size_t)((C + 1) / 2) * TD_FFT_SCR + (size_t)batch * PHAT_SPEC * 2) * sizeof(float);
}

// chunk slots per event: no event is located on more than min(max_frames, the longest recording's frames) frames
inline long tdoa_chunks_per_event(long max_rec_frames, int max_frames) {
    const long f = max_rec_frames < max_frames ? max_rec_frames : max_frames;
    return (f + TD_CHUNK - 1) / TD_CHUNK;
}

}  // namespace
