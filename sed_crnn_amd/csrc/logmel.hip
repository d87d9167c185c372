// logmel.hip — log-mel front end: framing + window + 2048-point real FFT -> |.|^2 -> mel filterbank -> log.
//
// Replaces librosa.stft / librosa.filters.mel / np.log as called by _mbe at reference feature.py:55-59
// (and, optionally fused, the StandardScaler of feature.py:127-129).
//
// Shape of the kernel (gfx950):
//   * a 2048-sample REAL frame is one 1024-point COMPLEX transform of z[n] = x[2n] + i x[2n+1] plus a pairing pass
//     (X[k] from Z[k] and conj Z[1024-k]) — half the butterflies of the complex transform of the frame;
//   * 1024 = 32 x 32: every lane does a 32-point FFT entirely in registers (compile-time twiddles), the 32 lanes of a
//     HALF wave exchange once through LDS (32x33-float transposes, conflict-free) and do a second 32-point FFT, so a wave
//     transforms TWO frames at a time and needs no workgroup barrier: waves are independent and loop over frame pairs;
//   * window, inter-pass twiddles W_1024^{rq}, pairing twiddles W_2048^k and the mel filterbank live in LDS, loaded once
//     per (persistent) workgroup; the filterbank is applied in its sparse form (a Slaney bank has 2 050 non-zeros of
//     41 000): band-major entry list, 1/32 of it per lane, partial sums combined in a fixed order (deterministic);
//   * HBM traffic is the PCM once (the 50 % overlap of neighbouring frames is re-read by the neighbouring half wave at
//     the same time and comes from L2) + 40 floats per frame.
// Algorithmic bytes per frame: hop*4 read + n_mels*4 written (4 256 B at hop 1024 / 40 mel).
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "fft2048.h"

namespace {

// Batched (SEG): R clips packed back to back in one PCM buffer; the launch walks the frame pairs of all of them, clip by clip.
// Device tables (uploaded by sed_logmel_batch): pair_off [R+1] (first pair of each clip; the last entry is the total),
// sample_off / n_samples / row_off [R] (the clip's first sample, its length and its first output row); n_pairs = pair_off[R].
// Multichannel (MC, sed_logmel_multi): the R clips are the planar channels of R / C recordings.  The C clips of a
// recording share row_off, and col_off [R] says where in a row of row_stride = C n_mels floats the clip's bands go (c n_mels:
// the [N, C F] layout the nets read); scaler_w = C n_mels coefficients of each kind are staged, column col_off + m is band m's.
struct LmBatch {
    const long* pair_off; const long* sample_off; const long* n_samples; const long* row_off; int R; long n_pairs;
    const long* col_off; int row_stride; int scaler_w;
};
// where one frame pair lives: its clip's PCM, length and frame count, the pair's index in the clip, the clip's first row and
// (MC) its first column
struct LmSeg { const float* pcm; long n_samples, n_frames, pair, row0; int col0; };

__device__ __forceinline__ long uniform_long(long v) {       // v is wave-uniform: say so, so that what it addresses stays scalar
    const unsigned long long u = (unsigned long long)v;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return (long)(((unsigned long long)hi << 32) | lo);
}

// Both frames of a pair belong to one clip, so the lookup (a binary search over pair_off) is wave-uniform.
template <bool SEG, bool MC>
__device__ __forceinline__ LmSeg lm_locate(long pair, const float* pcm, long n_samples, long n_frames, const LmBatch& bt, int hop) {
    if (!SEG) return LmSeg{pcm, n_samples, n_frames, pair, 0, 0};
    pair = uniform_long(pair);
    int lo = 0, hi = bt.R - 1;                               // the last clip whose first pair is <= pair
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (bt.pair_off[mid] <= pair) lo = mid;
        else hi = mid - 1;
    }
    const int c = __builtin_amdgcn_readfirstlane(lo);
    const long ns = bt.n_samples[c];
    return LmSeg{pcm + bt.sample_off[c], ns, 1 + ns / hop, pair - bt.pair_off[c], bt.row_off[c], MC ? __builtin_amdgcn_readfirstlane((int)bt.col_off[c]) : 0};
}

// DB: the next pair's PCM goes to a second register set one iteration ahead (needs the 256 registers of <= 8 waves per CU);
// otherwise it is loaded into the FFT registers before the mel pass of the current pair (they are dead by then).
// SEG: the batched launch (LmBatch above; n_samples / n_frames are then unused).  The FFT, mel and scaler code is the same.
// MC (with SEG): the output addressing of sed_logmel_multi — a row stride and a per-clip column offset, and a scaler as wide as
// the row.  A template parameter, so that the instantiations sed_logmel and sed_logmel_batch launch are the code they were.
template <int WPB, bool SEG = false, bool DB = (WPB <= 8), bool MC = false>
__global__ __launch_bounds__(WPB * 64) void logmel_fft_k(const float* __restrict__ pcm, long n_samples,
                                                         const uint32_t* __restrict__ tables, int table_words,
                                                         const float* __restrict__ mu, const float* __restrict__ inv_sigma,
                                                         float* __restrict__ out, long n_frames, int hop, int pad_mode, int n_mels_out,
                                                         LmBatch bt = LmBatch{}) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    fft_stage_tables(lds, tables, table_words, tid, WPB * 64);       // once per workgroup (table_words is a multiple of 4)
    // the fused scaler's coefficients go to LDS too: a global load inside the loop would have to retire IN ORDER behind the
    // PCM prefetch of the next pair (vmcnt counts in order), i.e. wait for exactly the latency the prefetch is there to hide.
    // That holds all the more for the C n_mels coefficients of a multichannel scaler: which slice a wave needs changes with
    // the clip of its pair, so a register copy per wave would have to be reloaded from global memory inside the loop — the
    // whole row of coefficients is staged instead (2 C n_mels floats, counted in the launch's LDS size).
    float* s_mu = lds + table_words + WPB * 2 * LM_FRAME_SCR;
    float* s_is = s_mu + (MC ? bt.scaler_w : LM_MAX_MELS);
    if (mu) {
        if (MC) for (int i = tid; i < bt.scaler_w; i += WPB * 64) { s_mu[i] = mu[i]; s_is[i] = inv_sigma[i]; }
        else for (int i = tid; i < n_mels_out && i < LM_MAX_MELS; i += WPB * 64) { s_mu[i] = mu[i]; s_is[i] = inv_sigma[i]; }
    }
    __syncthreads();
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(lds);
    // the row length of `out` is the caller's n_mels; a blob built for more bands than that never writes past a row
    const int n_mels = (int)hdr[1] < n_mels_out ? (int)hdr[1] : n_mels_out, iters = (int)hdr[2];
    const bool two_band = hdr[5] != 0;                       // which mel plan the blob carries (wave-uniform)
    const f2* s_win = reinterpret_cast<const f2*>(lds + LM_OFF_WIN);
    const f2* s_tw = reinterpret_cast<const f2*>(lds + LM_OFF_TW);
    const f2* s_pw = reinterpret_cast<const f2*>(lds + LM_OFF_PW);
    const float2* s_ent = reinterpret_cast<const float2*>(lds + LM_OFF_ENT);
    const uint32_t* s_band = reinterpret_cast<const uint32_t*>(lds + LM_OFF_ENT + (size_t)iters * 64);

    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, r = lane & 31;
    float* scr = lds + table_words + (wave * 2 + half) * LM_FRAME_SCR;      // this half wave's transpose / power buffer
    float* part = scr + LM_SCR;
    float* wscr = lds + table_words + wave * 2 * LM_FRAME_SCR;               // the wave's whole scratch: the 32 x 65 exchange buffer
    const FftLane fl = fft_lane(lane, wscr - lds);
    const int partner = fl.partner();
    const unsigned xbase = fl.xbase;
    const long n_pairs = SEG ? bt.n_pairs : (n_frames + 1) >> 1;

    // interior frame pairs with an even hop are read by plain 8-byte loads; the loads of the NEXT pair are issued before
    // the mel pass of the current one (the FFT registers are dead by then), so HBM latency hides behind it
    auto fast_ok = [&](const LmSeg& g) -> bool {
        const bool even_hop = (hop & 1) == 0 && (reinterpret_cast<uintptr_t>(g.pcm) & 7) == 0;
        const long first = g.pair * 2 * hop - LM_NFFT / 2, last = first + hop + LM_NFFT;    // span of both frames (wave-uniform)
        return even_hop && first >= 0 && last <= g.n_samples && g.pair * 2 + 1 < g.n_frames;
    };
    f2 z[32];                                                // z[n] = (x[2n], x[2n+1]): one complex point per VGPR pair
    // Where the time goes (round 4, ablation builds on one box, one hour of audio, 12 waves per CU; the full kernel 0.33-0.35 ms):
    // without the mel pass 0.246, without the pairing pass 0.271, without the two FFTs 0.262, without any of the compute phases
    // 0.175, of which the PCM loads are 0.11 (0.062 with the loads replaced by a register fill): the phases ADD UP — each is a
    // chain of LDS round trips (table reads, exchange, bpermute), and neither the vector ALU (36 %) nor the LDS pipe (40-55 %)
    // nor HBM (1.9 of 6.3 TB/s) is saturated.  What was tried on that in round 4: complex points in VGPR pairs (v_pk_* with op_sel:
    // 38 % fewer vector instructions — no change in run time, kept: it is the smaller kernel); table and power-bin reads of the
    // mel and pairing passes issued in batches ahead of the stores that hipcc has to order them behind (-5 %); a second
    // register set for the next pair's PCM, loaded a whole iteration ahead (DB, needs the 256 registers of 8 waves per CU:
    // 0.36 ms, slower than 12 waves with the loads issued before the mel pass; kept for the large-table plans that run with
    // <= 8 waves anyway); de-phasing the waves of a SIMD by a third of an iteration (no change).
    f2 zn[DB ? 32 : 1];
    const long stride = (long)gridDim.x * WPB;
    const long pair0 = (long)blockIdx.x * WPB + wave;
    LmSeg cur = lm_locate<SEG, MC>(pair0 < n_pairs ? pair0 : 0, pcm, n_samples, n_frames, bt, hop);
    bool nloaded = DB && pair0 < n_pairs && fast_ok(cur);
    if (DB && nloaded) {
        const f2* src = reinterpret_cast<const f2*>(cur.pcm + (cur.pair * 2 + half) * hop - LM_NFFT / 2) + r;
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) zn[DB ? n1 : 0] = src[32 * n1];
    }
    for (long pair = pair0; pair < n_pairs; pair += stride) {
        // the next pair (its clip when batched): what the prefetch below loads, and this loop's state one iteration from now
        const LmSeg nxt = lm_locate<SEG, MC>(pair + stride < n_pairs ? pair + stride : pair, pcm, n_samples, n_frames, bt, hop);
        long frame = cur.pair * 2 + half;
        const bool live = frame < cur.n_frames;
        if (!live) frame = cur.n_frames - 1;                 // odd tail: the upper half recomputes the last frame, stores nothing
        const long start = frame * hop - LM_NFFT / 2;
        const float* cpcm = cur.pcm;
        const long cns = cur.n_samples;
        // ── z[32 n1 + r] = (x[64 n1 + 2r], x[64 n1 + 2r + 1]) * window ──
        // (From here to pass 2 this is fft_load_guarded and fft2048_passes of fft2048.h, written out: called as functions they
        // compute the same values, but hipcc simplifies a function before it inlines it and the instantiations then come out with
        // other register assignments — the 12-wave one at 165 instead of 163 of its 168 VGPRs with the guarded load.  The kernel
        // is kept as measured; a change to either copy belongs in both.)
        const bool loaded = nloaded;
        if (DB && loaded) {
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) z[n1] = zn[DB ? n1 : 0];
        }
        if (DB) nloaded = pair + stride < n_pairs && fast_ok(nxt);
        if (DB && nloaded) {                                 // the next pair's PCM: first use is the copy above, one iteration from now
            const f2* src = reinterpret_cast<const f2*>(nxt.pcm + (nxt.pair * 2 + half) * hop - LM_NFFT / 2) + r;
#pragma unroll
            for (int n1 = 0; n1 < 32; ++n1) zn[DB ? n1 : 0] = src[32 * n1];
        }
        if (!loaded) {
            if (!DB && fast_ok(cur)) {
                const f2* src = reinterpret_cast<const f2*>(cpcm + start) + r;
#pragma unroll
                for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
            } else {                                         // edge frames / odd hop: guarded loads, staged through LDS so that
                wave_lds_fence();                            //  this cold path costs no registers (dynamic index, not unrolled)
#pragma unroll 1
                for (int n1 = 0; n1 < 32; ++n1) scr[n1 * 32 + r] = pcm_at(cpcm, start + 64 * n1 + 2 * r, cns, pad_mode);
                wave_lds_fence();
#pragma unroll
                for (int n1 = 0; n1 < 32; ++n1) z[n1].x = scr[n1 * 32 + r];
                wave_lds_fence();
#pragma unroll 1
                for (int n1 = 0; n1 < 32; ++n1) scr[n1 * 32 + r] = pcm_at(cpcm, start + 64 * n1 + 2 * r + 1, cns, pad_mode);
                wave_lds_fence();
#pragma unroll
                for (int n1 = 0; n1 < 32; ++n1) z[n1].y = scr[n1 * 32 + r];
            }
        }
#pragma unroll
        for (int n1 = 0; n1 < 32; ++n1) z[n1] *= s_win[32 * n1 + r];

        // ── pass 1: FFT over n1, twiddle W_1024^{r k1} ──
        fft32(z);
#pragma unroll
        for (int k1 = 1; k1 < 32; ++k1) {
            const int b = brev5(k1);
            z[b] = cmul(z[b], s_tw[k1 * 32 + r]);
        }
        // ── exchange through LDS (real parts, then imaginary parts, the wave's 32 x 65 buffer): lane (half, r) holds
        //    A[r][k1] and stores row k1 lane-linearly; lane (half, c) then needs A[n2][c] = row c, column 32*half + n2 ──
        wave_lds_fence();                                    // the previous frame's mel pass has finished reading the scratch
        exchange_store<0>(xbase, z);
        wave_lds_fence();
        const unsigned xaddr = xbase + (unsigned)(r * LM_ROW_BYTES + 128 * half);          // LDS byte address of xrow
        exchange_load<0>(xaddr, z);                          // (the .y halves — the imaginary parts — are still to be stored)
        wave_lds_fence();
        exchange_store<1>(xbase, z);
        wave_lds_fence();
        exchange_load<1>(xaddr, z);
        wave_lds_fence();
        // ── pass 2: FFT over n2 -> Z[r + 32 k2] = z[brev5(k2)] ──
        fft32(z);
        // ── pairing: 2 X[k] = (Z[k] + conj Z[N-k]) - i W_2048^k (Z[k] - conj Z[N-k]); lane r owns k = r + 32 k2, k2 < 16, and
        //    its mirror N-k, whose Z lives in lane (32 - r) % 32, register 31 - k2 (lane 0: its own register 32 - k2) ──
        // (the 16 pairing twiddles and the 16 mirrored points are fetched before the first power bin is stored: the stores to
        // `scr` would otherwise fence every later table read behind them, one LDS round trip per k2)
        f2 pwv[16], ppv[16];
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const int bp = brev5(31 - k2), b0 = brev5((32 - k2) & 31);
            pwv[k2] = s_pw[r + 32 * k2];
            f2 pp = {__shfl(z[bp].x, partner, 64), __shfl(z[bp].y, partner, 64)};
            if (r == 0) pp = z[b0];
            ppv[k2] = pp;
        }
#pragma unroll
        for (int k2 = 0; k2 < 16; ++k2) {
            const f2 zz = z[brev5(k2)], pp = ppv[k2];
            const int k = r + 32 * k2;
            const f2 e = add_conj(zz, pp);                   // Z[k] + conj Z[N-k]
            const f2 q = rot_sub_conj(zz, pp);               // -i (Z[k] - conj Z[N-k]) = (zi + pi, pr - zr)
            const f2 t = cmul(q, pwv[k2]);
            const f2 a = e + t, bb = e - t;
            const f2 a2 = a * a, b2 = bb * bb;
            scr[k] = a2.x + a2.y;                            // 4 |X[k]|^2   (the 1/4 is folded into the mel weights)
            scr[LM_N - k] = b2.x + b2.y;                     // 4 |X[N-k]|^2
        }
        if (r == 0) { const f2 zz = z[brev5(16)]; scr[512] = 4.f * (zz.x * zz.x + zz.y * zz.y); }
        wave_lds_fence();
        if (!DB) {
            nloaded = pair + stride < n_pairs && fast_ok(nxt);
            if (nloaded) {                                   // single set: the FFT registers are dead here; first use is the next window multiply
                const f2* src = reinterpret_cast<const f2*>(nxt.pcm + (nxt.pair * 2 + half) * hop - LM_NFFT / 2) + r;
#pragma unroll
                for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
            }
        }
        if (two_band) {
            // ── two-band plan: bins 33r .. 33r+32 (bins past 1024 carry zero weights; their slots are cleared so that a
            //    stale non-finite value cannot turn 0*x into NaN) ──
            if (r > 0) scr[LM_N + r] = 0.f;
            if (r == 0) part[LM_PART - 1] = 0.f;             // the always-zero slot the band lists pad with
            wave_lds_fence();
            const f32x4* ent = reinterpret_cast<const f32x4*>(s_ent) + r;
            const float* pb = scr + LM_TRI_BINS * r;
            float lo = 0.f, hi = 0.f;
            // The table entries and power bins of a whole chunk are read BEFORE its first partial sum is stored: hipcc cannot
            // prove that a store to `part` leaves `scr` and the table alone, so with read / use / store per bin (round 2) every
            // bin paid two LDS round trips in sequence — 33 x ~250 cycles, a quarter of the kernel (ablation: 0.11 of 0.40 ms).
            constexpr int CH = DB ? 11 : 3;                   // (12 waves per CU: 168 registers, 64 of them hold the prefetched PCM)
            static_assert(LM_TRI_BINS % CH == 0, "chunks");
#pragma unroll
            for (int c0 = 0; c0 < LM_TRI_BINS; c0 += CH) {
                f32x4 e[CH];
                float pv[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) { e[u] = ent[(c0 + u) * 32]; pv[u] = pb[c0 + u]; }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    lo = fmaf(e[u][0], pv[u], lo);
                    hi = fmaf(e[u][1], pv[u], hi);
                    const uint32_t slot = __float_as_uint(e[u][2]);
                    if ((int32_t)slot >= 0) {
                        *reinterpret_cast<float2*>(part + slot) = make_float2(lo, hi);
                        lo = 0.f; hi = 0.f;
                    }
                }
            }
            wave_lds_fence();
            const uint4* blist = reinterpret_cast<const uint4*>(lds + LM_OFF_ENT + LM_TRI_BINS * 32 * 4);
            for (int m = r; m < n_mels; m += 32) {
                const uint4 l = blist[m];
                float v = part[l.x & 0xffffu];                // fixed summation order: deterministic
                v += part[l.x >> 16];
                v += part[l.y & 0xffffu];
                v += part[l.y >> 16];
                v += part[l.z & 0xffffu];
                v += part[l.z >> 16];
                v += part[l.w & 0xffffu];
                v += part[l.w >> 16];
                v = logf(v);
                if (mu) v = MC ? (v - s_mu[cur.col0 + m]) * s_is[cur.col0 + m] : (v - s_mu[m]) * s_is[m];
                if (live) out[MC ? (cur.row0 + frame) * bt.row_stride + cur.col0 + m : (cur.row0 + frame) * n_mels_out + m] = v;
            }
        } else {
            // ── list plan: lane r walks entries [r*iters, (r+1)*iters) of the band-major list ──
            float acc = 0.f;
            for (int i0 = 0; i0 < iters; i0 += 8) {          // iters is a multiple of 8; 8 independent LDS reads in flight
                float2 e[8];
                float pv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = s_ent[(i0 + u) * 32 + r];
#pragma unroll
                for (int u = 0; u < 8; ++u) pv[u] = scr[__float_as_uint(e[u].y) & 0x7ffu];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t meta = __float_as_uint(e[u].y);
                    acc = fmaf(e[u].x, pv[u], acc);
                    if (meta & 0x800u) { part[meta >> 12] = acc; acc = 0.f; }
                }
            }
            wave_lds_fence();
            for (int m = r; m < n_mels; m += 32) {
                const uint32_t bd = s_band[m];
                const int f0 = (int)(bd & 0xffffu), cnt = (int)(bd >> 16);
                float v = 0.f;
                for (int j = 0; j < cnt; ++j) v += part[f0 + j];
                v = logf(v);
                if (mu) v = MC ? (v - s_mu[cur.col0 + m]) * s_is[cur.col0 + m] : (v - s_mu[m]) * s_is[m];
                if (live) out[MC ? (cur.row0 + frame) * bt.row_stride + cur.col0 + m : (cur.row0 + frame) * n_mels_out + m] = v;
            }
        }
        cur = nxt;
    }
}

struct LmPlan { int n_mels, iters, n_slots, words, tri; std::vector<uint32_t> ent, band; };

// plan 0: band-major non-zero list of a dense [n_mels][1025] bank, 1/32 per lane; returns 0 when it cannot be planned
int plan_list(const float* fb, int n_mels, LmPlan* p) {
    const int nb = LM_NFFT / 2 + 1;
    std::vector<int> ek, eb;
    std::vector<float> ew;
    for (int m = 0; m < n_mels; ++m) {
        bool any = false;
        for (int k = 0; k < nb; ++k)
            if (fb[(size_t)m * nb + k] != 0.f) { ek.push_back(k); eb.push_back(m); ew.push_back(fb[(size_t)m * nb + k]); any = true; }
        if (!any) { ek.push_back(0); eb.push_back(m); ew.push_back(0.f); }     // an empty band still owns a slot (log 0 = -inf)
    }
    const int nnz = (int)ek.size();
    const int iters = ((nnz + 31) / 32 + 7) & ~7;             // per-lane entries, padded to the kernel's unroll of 8
    if (iters > 256) return 0;
    p->ent.assign((size_t)iters * 64, 0u);
    p->band.assign(n_mels, 0u);
    int slot = 0;
    std::vector<int> first(n_mels, -1), cnt(n_mels, 0);
    for (int lane = 0; lane < 32; ++lane) {
        for (int i = 0; i < iters; ++i) {
            const int e = lane * iters + i;
            if (e >= nnz) break;
            const bool emit = (i == iters - 1) || (e == nnz - 1) || (eb[e + 1] != eb[e]);
            const size_t at = ((size_t)i * 32 + lane) * 2;
            const float w = 0.25f * ew[e];
            memcpy(&p->ent[at], &w, 4);
            p->ent[at + 1] = (uint32_t)ek[e] | (emit ? 0x800u : 0u) | ((uint32_t)slot << 12);
            if (emit) {
                const int m = eb[e];
                if (first[m] < 0) first[m] = slot;
                ++cnt[m];
                ++slot;
            }
        }
    }
    if (slot > LM_PART) return 0;
    for (int m = 0; m < n_mels; ++m) p->band[m] = (uint32_t)first[m] | ((uint32_t)cnt[m] << 16);
    p->n_mels = n_mels; p->iters = iters; p->n_slots = slot; p->tri = 0;
    p->words = (LM_OFF_ENT + iters * 64 + n_mels + 3) & ~3;
    return 1;
}

// plan 1: every bin feeds at most two adjacent bands; returns 0 when the bank is not of that shape
int plan_two_band(const float* fb, int n_mels, LmPlan* p) {
    const int nb = LM_NFFT / 2 + 1;
    std::vector<int> lower(nb, 0);                            // band of the "lower" accumulator at bin k (upper = lower + 1)
    int prev = 0;
    for (int k = 0; k < nb; ++k) {
        int b0 = -1, b1 = -1, n = 0;
        for (int m = 0; m < n_mels; ++m)
            if (fb[(size_t)m * nb + k] != 0.f) { if (n == 0) b0 = m; else b1 = m; ++n; }
        if (n > 2 || (n == 2 && b1 != b0 + 1)) return 0;
        if (n == 2) prev = b0;
        else if (n == 1 && b0 != prev && b0 != prev + 1) prev = b0;
        lower[k] = prev;
    }
    p->ent.assign((size_t)LM_TRI_BINS * 32 * 4, 0u);
    std::vector<std::vector<int>> slots(n_mels);
    int pair = 0;
    for (int lane = 0; lane < 32; ++lane) {
        bool used_lo = false, used_hi = false;
        for (int i = 0; i < LM_TRI_BINS; ++i) {
            const int k = LM_TRI_BINS * lane + i;
            const size_t at = ((size_t)i * 32 + lane) * 4;
            p->ent[at + 2] = 0xffffffffu;
            if (k >= nb) continue;
            const int L = lower[k];
            const float wl = 0.25f * fb[(size_t)L * nb + k];
            const float wh = (L + 1 < n_mels) ? 0.25f * fb[(size_t)(L + 1) * nb + k] : 0.f;
            memcpy(&p->ent[at], &wl, 4);
            memcpy(&p->ent[at + 1], &wh, 4);
            used_lo |= wl != 0.f; used_hi |= wh != 0.f;
            const bool last = (i == LM_TRI_BINS - 1) || (k == nb - 1) || (lower[k + 1] != L);
            if (!last) continue;
            if (used_lo || used_hi) {
                p->ent[at + 2] = (uint32_t)(2 * pair);
                if (used_lo) slots[L].push_back(2 * pair);
                if (used_hi) slots[L + 1].push_back(2 * pair + 1);
                ++pair;
            } else {
                p->ent[at + 2] = 0xfffffffeu;                 // nothing accumulated: no store (accumulators are zero anyway)
            }
            used_lo = used_hi = false;
        }
    }
    if (2 * pair > LM_PART - 1) return 0;
    p->band.assign((size_t)n_mels * 4, 0u);
    const uint32_t zero_slot = LM_PART - 1;
    for (int m = 0; m < n_mels; ++m) {
        if (slots[m].size() > 8) return 0;
        uint32_t l[8];
        for (int j = 0; j < 8; ++j) l[j] = j < (int)slots[m].size() ? (uint32_t)slots[m][j] : zero_slot;
        for (int j = 0; j < 4; ++j) p->band[(size_t)m * 4 + j] = l[2 * j] | (l[2 * j + 1] << 16);
    }
    p->n_mels = n_mels; p->iters = LM_TRI_BINS; p->n_slots = 2 * pair; p->tri = 1;
    p->words = (LM_OFF_ENT + LM_TRI_BINS * 32 * 4 + n_mels * 4 + 3) & ~3;
    return 1;
}

int plan_mel(const float* fb, int n_mels, LmPlan* p) {
    if (plan_two_band(fb, n_mels, p)) return 1;
    return plan_list(fb, n_mels, p);
}

}  // namespace

extern "C" size_t sed_logmel_tables_bytes(const float* melfb_host, int n_fft, int n_mels) {
    if (!melfb_host || n_fft != LM_NFFT || n_mels <= 0 || n_mels > LM_MAX_MELS) return 0;
    LmPlan p;
    if (!plan_mel(melfb_host, n_mels, &p)) return 0;
    return (size_t)p.words * 4;
}

extern "C" int sed_logmel_build_tables(const float* window_host, const float* melfb_host, int n_fft, int n_mels,
                                       void* tables_host, size_t tables_bytes) {
    SED_REQUIRE(window_host && melfb_host && tables_host, "logmel_build_tables: null pointer");
    SED_REQUIRE(n_fft == LM_NFFT, "logmel_build_tables: n_fft must be %d (got %d)", LM_NFFT, n_fft);
    SED_REQUIRE(n_mels > 0 && n_mels <= LM_MAX_MELS, "logmel_build_tables: n_mels must be in [1,%d]", LM_MAX_MELS);
    LmPlan p;
    SED_REQUIRE(plan_mel(melfb_host, n_mels, &p),
                "logmel_build_tables: filterbank has too many non-zeros for the LDS-resident sparse plan");
    SED_REQUIRE(tables_bytes >= (size_t)p.words * 4, "logmel_build_tables: buffer too small (%zu < %zu)", tables_bytes, (size_t)p.words * 4);
    uint32_t* t = (uint32_t*)tables_host;
    memset(t, 0, (size_t)p.words * 4);
    t[0] = LM_MAGIC; t[1] = (uint32_t)n_mels; t[2] = (uint32_t)p.iters; t[3] = (uint32_t)p.n_slots; t[4] = (uint32_t)p.words;
    t[5] = (uint32_t)p.tri;
    float* f = (float*)tables_host;
    memcpy(f + LM_OFF_WIN, window_host, LM_NFFT * sizeof(float));
    const double two_pi = 6.283185307179586476925286766559;
    for (int q = 0; q < 32; ++q)
        for (int r = 0; r < 32; ++r) {
            const double a = two_pi * (double)((r * q) % LM_N) / (double)LM_N;
            f[LM_OFF_TW + (q * 32 + r) * 2] = (float)cos(a);
            f[LM_OFF_TW + (q * 32 + r) * 2 + 1] = (float)(-sin(a));
        }
    for (int k = 0; k <= 512; ++k) {
        const double a = two_pi * (double)k / (double)LM_NFFT;
        f[LM_OFF_PW + 2 * k] = (float)cos(a);
        f[LM_OFF_PW + 2 * k + 1] = (float)(-sin(a));
    }
    memcpy(t + LM_OFF_ENT, p.ent.data(), p.ent.size() * 4);
    memcpy(t + LM_OFF_ENT + p.ent.size(), p.band.data(), p.band.size() * 4);
    return 0;
}

// 12 waves per CU: the most that fit beside the tables (12 x 9.7 KB of exchange / power scratch + 38 KB of tables in 160 KB)
#define LM_WPB 12
#define LM_SCALER_BYTES ((size_t)2 * LM_MAX_MELS * sizeof(float))      // mean and 1/sigma of the fused scaler, behind the wave scratch
// scaler_bytes: the LDS behind the wave scratch that holds the scaler (LM_SCALER_BYTES for sed_logmel / sed_logmel_batch, the real
// 2 C n_mels floats — nothing without a scaler — for sed_logmel_multi)
template <int WPB, bool SEG, bool MC>
static int launch_logmel(const float* pcm, long n_samples, const void* tables, int words, const float* mu, const float* inv_sigma,
                         float* out, long frames, int hop, int n_mels, int pad_mode, const LmBatch& bt, size_t scaler_bytes, hipStream_t s) {
    const size_t lds = (size_t)words * 4 + (size_t)WPB * 2 * LM_FRAME_SCR * sizeof(float) + scaler_bytes;
    SED_REQUIRE(lds <= 160 * 1024, "logmel: tables + scratch (%zu B) exceed the 160 KiB LDS", lds);
    hipError_t e = hipFuncSetAttribute((const void*)logmel_fft_k<WPB, SEG, (WPB <= 8), MC>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) { sed_set_error("logmel: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    const long pairs = SEG ? bt.n_pairs : (frames + 1) / 2;
    long blocks = (pairs + WPB - 1) / WPB;
    const long resident = 256;                               // one persistent workgroup per CU: the tables are loaded once each
    if (blocks > resident) blocks = resident;
    SedProfScope prof(SED_K_LOGMEL, s, (double)frames * ((double)hop + n_mels) * 4.0);
    logmel_fft_k<WPB, SEG, (WPB <= 8), MC><<<(unsigned)blocks, WPB * 64, lds, s>>>(pcm, n_samples, (const uint32_t*)tables, words, mu,
                                                                                   inv_sigma, out, frames, hop, pad_mode, n_mels, bt);
    SED_LAUNCH_CHECK("logmel");
    return 0;
}

// 12 waves per workgroup when the tables leave room for their scratch (the two-band plan of a Slaney bank: 38 KB); a large
// list plan (up to 8 192 non-zeros = 67 KB of entries) runs with fewer waves per CU rather than being refused
template <bool SEG, bool MC = false>
static int launch_logmel_any(const float* pcm, long n_samples, const void* tables, int words, const float* mu, const float* inv_sigma,
                             float* out, long frames, int hop, int n_mels, int pad_mode, const LmBatch& bt, hipStream_t s,
                             size_t scaler_bytes = LM_SCALER_BYTES) {
    const size_t per_wave = (size_t)2 * LM_FRAME_SCR * sizeof(float), room = (size_t)160 * 1024 - scaler_bytes;
    const size_t tb = (size_t)words * 4;
    if (tb + 12 * per_wave <= room) return launch_logmel<12, SEG, MC>(pcm, n_samples, tables, words, mu, inv_sigma, out, frames, hop, n_mels, pad_mode, bt, scaler_bytes, s);
    if (tb + 8 * per_wave <= room) return launch_logmel<8, SEG, MC>(pcm, n_samples, tables, words, mu, inv_sigma, out, frames, hop, n_mels, pad_mode, bt, scaler_bytes, s);
    if (tb + 4 * per_wave <= room) return launch_logmel<4, SEG, MC>(pcm, n_samples, tables, words, mu, inv_sigma, out, frames, hop, n_mels, pad_mode, bt, scaler_bytes, s);
    return launch_logmel<2, SEG, MC>(pcm, n_samples, tables, words, mu, inv_sigma, out, frames, hop, n_mels, pad_mode, bt, scaler_bytes, s);
}

// the argument checks both entries share
static int logmel_check_args(const void* tables, size_t tables_bytes, const float* mu, const float* inv_sigma, int n_fft, int hop,
                             int n_mels, int pad_mode, bool multi = false, size_t scaler_bytes = LM_SCALER_BYTES) {
    SED_REQUIRE(n_fft == LM_NFFT, "logmel: n_fft must be %d (got %d)", LM_NFFT, n_fft);
    SED_REQUIRE(hop > 0 && n_mels > 0 && n_mels <= LM_MAX_MELS, "logmel: bad sizes");
    SED_REQUIRE((mu == nullptr) == (inv_sigma == nullptr), "logmel: mu and inv_sigma go together");
    SED_REQUIRE(pad_mode == 0 || pad_mode == 1, "logmel: pad_mode must be 0 (constant) or 1 (reflect)");
    const int words = (int)(tables_bytes / 4);
    SED_REQUIRE(tables_bytes % 16 == 0 && words >= LM_OFF_ENT + 64 + n_mels, "logmel: table blob of %zu bytes is malformed", tables_bytes);
    if (!multi)
        SED_REQUIRE((size_t)words * 4 + (size_t)2 * 2 * LM_FRAME_SCR * sizeof(float) + LM_SCALER_BYTES <= (size_t)160 * 1024,
                    "logmel: a table blob of %zu bytes leaves no room for the FFT scratch in the 160 KiB LDS", tables_bytes);
    else                                                     // sed_logmel_multi: the scaler is as wide as the feature row
        SED_REQUIRE((size_t)words * 4 + (size_t)2 * 2 * LM_FRAME_SCR * sizeof(float) + scaler_bytes <= (size_t)160 * 1024,
                    "logmel_multi: a table blob of %zu bytes and a scaler of %zu bytes leave no room for the FFT scratch of even 2 "
                    "waves (%zu bytes) in the 160 KiB LDS", tables_bytes, scaler_bytes, (size_t)2 * 2 * LM_FRAME_SCR * sizeof(float));
    return 0;
}

extern "C" int sed_logmel(const float* pcm, long n_samples, const void* tables, size_t tables_bytes, const float* mu,
                          const float* inv_sigma, float* out, int n_fft, int hop, int n_mels, int pad_mode, void* stream) {
    SED_REQUIRE(pcm && tables && out, "logmel: null pointer");
    SED_REQUIRE(n_samples > 0, "logmel: bad sizes");
    if (int rc = logmel_check_args(tables, tables_bytes, mu, inv_sigma, n_fft, hop, n_mels, pad_mode)) return rc;
    const long frames = 1 + n_samples / hop;
    return launch_logmel_any<false>(pcm, n_samples, tables, (int)(tables_bytes / 4), mu, inv_sigma, out, frames, hop, n_mels, pad_mode,
                                    LmBatch{}, as_stream(stream));
}

// ───────────────────────── batch: R clips packed in one PCM buffer, one launch ─────────────────────────
// workspace: pair_off [R+1], sample_off [R], n_samples [R], row_off [R] (64-bit), uploaded from the validated host table
extern "C" size_t sed_logmel_batch_workspace_bytes(int R) {
    if (R < 1 || R > (1 << 26)) return 0;
    return ((size_t)4 * R + 1) * sizeof(long);
}

extern "C" int sed_logmel_batch(const float* pcm, long pcm_len, const long* clips_host, int R, const void* tables, size_t tables_bytes,
                                const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop, int n_mels,
                                int pad_mode, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(pcm && clips_host && tables && out && workspace, "logmel_batch: null pointer");
    const size_t need = sed_logmel_batch_workspace_bytes(R);
    SED_REQUIRE(need > 0 && pcm_len > 0, "logmel_batch: bad sizes (R=%d, pcm_len=%ld)", R, pcm_len);
    SED_REQUIRE(workspace_bytes >= need, "logmel_batch: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if (int rc = logmel_check_args(tables, tables_bytes, mu, inv_sigma, n_fft, hop, n_mels, pad_mode)) return rc;
    std::vector<long> h((size_t)4 * R + 1);
    long* pair_off = h.data();
    long *soff = pair_off + R + 1, *slen = soff + R, *roff = slen + R;
    long pairs = 0, rows = 0;
    for (int c = 0; c < R; ++c) {
        const long o = clips_host[2 * c], n = clips_host[2 * c + 1];
        SED_REQUIRE(o >= 0 && n >= 1 && o <= pcm_len && n <= pcm_len - o,
                    "logmel_batch: clip %d (offset %ld, %ld samples) is not inside the PCM buffer of %ld samples", c, o, n, pcm_len);
        const long f = 1 + n / hop;
        pair_off[c] = pairs; soff[c] = o; slen[c] = n; roff[c] = rows;
        pairs += (f + 1) / 2;
        rows += f;
        SED_REQUIRE(rows <= 0x7fffffffL, "logmel_batch: more than 2^31 - 1 feature frames in one batch");
    }
    pair_off[R] = pairs;
    SED_REQUIRE(out_rows == rows, "logmel_batch: out has %ld rows, the clips make %ld", out_rows, rows);
    hipStream_t s = as_stream(stream);
    long* dev = (long*)workspace;
    hipError_t e = hipMemcpyAsync(dev, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("logmel_batch: upload of the clip table: %s", hipGetErrorString(e)); return (int)e; }
    const LmBatch bt{dev, dev + R + 1, dev + 2 * R + 1, dev + 3 * R + 1, R, pairs};
    return launch_logmel_any<true>(pcm, pcm_len, tables, (int)(tables_bytes / 4), mu, inv_sigma, out, rows, hop, n_mels, pad_mode, bt, s);
}

// ───────────────────────── multichannel: R recordings x C planar channels -> one [rows][C n_mels] matrix, one launch ─────────────────────────
// workspace: pair_off [RC+1], sample_off, n_samples, row_off, col_off [RC] (64-bit), uploaded from the validated host table
extern "C" size_t sed_logmel_multi_workspace_bytes(int R, int channels) {
    if (R < 1 || channels < 1 || channels > 64 || (long)R * channels > (1 << 26)) return 0;
    return ((size_t)5 * R * channels + 1) * sizeof(long);
}

// row_stride: the floats of an output row.  sed_logmel_multi's is channels * n_mels; sed_logmel_gcc (gcc.hip) writes the mel
// columns of its wider rows through this same launch (and the first channels * n_mels scaler entries), so they are the same code
int sed_internal_logmel_multi(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                              size_t tables_bytes, const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop,
                              int n_mels, int pad_mode, int row_stride, void* workspace, size_t workspace_bytes,
                              void* stream) {
    SED_REQUIRE(channels >= 1 && channels <= 64, "logmel_multi: 1 to 64 channels, got %d", channels);
    SED_REQUIRE(pcm && clips_host && tables && out && workspace, "logmel_multi: null pointer");
    const size_t need = sed_logmel_multi_workspace_bytes(R, channels);
    SED_REQUIRE(need > 0 && pcm_len > 0, "logmel_multi: bad sizes (R=%d, channels=%d, pcm_len=%ld)", R, channels, pcm_len);
    SED_REQUIRE(workspace_bytes >= need, "logmel_multi: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(n_mels > 0 && n_mels <= LM_MAX_MELS, "logmel: bad sizes");
    SED_REQUIRE(row_stride >= channels * n_mels, "logmel_multi: a row of %d floats does not hold %d channels of %d bands", row_stride, channels, n_mels);
    const size_t scaler_bytes = mu ? (size_t)2 * channels * n_mels * sizeof(float) : 0;
    if (int rc = logmel_check_args(tables, tables_bytes, mu, inv_sigma, n_fft, hop, n_mels, pad_mode, true, scaler_bytes)) return rc;
    const long RC = (long)R * channels;
    std::vector<long> h((size_t)5 * RC + 1);
    long* pair_off = h.data();
    long *soff = pair_off + RC + 1, *slen = soff + RC, *roff = slen + RC, *coff = roff + RC;
    long pairs = 0, rows = 0;
    for (int r = 0; r < R; ++r) {
        const long n0 = clips_host[2 * ((long)r * channels) + 1];
        const long f = n0 >= 1 ? 1 + n0 / hop : 0;
        for (int ch = 0; ch < channels; ++ch) {
            const long c = (long)r * channels + ch, o = clips_host[2 * c], n = clips_host[2 * c + 1];
            SED_REQUIRE(o >= 0 && n >= 1 && o <= pcm_len && n <= pcm_len - o,
                        "logmel_multi: recording %d, channel %d (offset %ld, %ld samples) is not inside the PCM buffer of %ld samples", r, ch,
                        o, n, pcm_len);
            SED_REQUIRE(n == n0, "logmel_multi: recording %d: channel %d has %ld samples, channel 0 has %ld (the channels of a recording "
                        "must have equal length)", r, ch, n, n0);
            pair_off[c] = pairs; soff[c] = o; slen[c] = n; roff[c] = rows; coff[c] = (long)ch * n_mels;
            pairs += (f + 1) / 2;
        }
        rows += f;
        SED_REQUIRE(rows <= 0x7fffffffL, "logmel_multi: more than 2^31 - 1 feature frames in one batch");
    }
    pair_off[RC] = pairs;
    SED_REQUIRE(out_rows == rows, "logmel_multi: out has %ld rows, the recordings make %ld", out_rows, rows);
    hipStream_t s = as_stream(stream);
    long* dev = (long*)workspace;
    hipError_t e = hipMemcpyAsync(dev, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("logmel_multi: upload of the clip table: %s", hipGetErrorString(e)); return (int)e; }
    const LmBatch bt{dev, dev + RC + 1, dev + 2 * RC + 1, dev + 3 * RC + 1, (int)RC, pairs, dev + 4 * RC + 1, row_stride, channels * n_mels};
    return launch_logmel_any<true, true>(pcm, pcm_len, tables, (int)(tables_bytes / 4), mu, inv_sigma, out, rows, hop, n_mels, pad_mode,
                                         bt, s, scaler_bytes);
}

extern "C" int sed_logmel_multi(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                                size_t tables_bytes, const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop,
                                int n_mels, int pad_mode, void* workspace, size_t workspace_bytes, void* stream) {
    return sed_internal_logmel_multi(pcm, pcm_len, clips_host, R, channels, tables, tables_bytes, mu, inv_sigma, out, out_rows, n_fft, hop,
                                     n_mels, pad_mode, channels * n_mels, workspace, workspace_bytes, stream);
}
