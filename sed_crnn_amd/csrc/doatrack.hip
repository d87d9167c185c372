// doatrack.hip — direction tracks: a direction per block of chunks of every located event, and the best path through the block
// maps under a bound on the angular step: sed_event_doa_track.
//
// tdoa_accum_k leaves one whitened cross-spectrum partial per TD_CHUNK = 32 frames of every event of a slice in the workspace;
// doa_steer_k (doa.hip) sums all of them before it steers.  Here the chunks are summed per BLOCK of W chunks and every block is
// steered on its own: no frame is transformed twice.  The block rule (trk_blocks below; localize.track_blocks states it on the
// host) is integer and a function of the event's located frames [f0, f0 + nf) and W alone:
//   nch = ceil(nf / 32), T0 = ceil(nch / W), nl = nf - 32 W (T0 - 1);  T = T0 - 1 where T0 > 1 and nl < 16 W (a short tail joins
//   the block before it), else T0;  block b covers the chunks [b W, (b + 1) W), the last block up to nch.
//
//   doa_track_steer_k   item = (event, block): S_b by phat_sum_chunks over the block's chunks (the first chunk starts the sum,
//                       the others are added in ascending order), then doa_steer_k's text — phat_lag_sum fine lags,
//                       srp[d] = sum_p fine_p[J[d][p]] in ascending p, the first maximum in ascending d, the silence rule —
//                       -> trk_raw, trk_power = best / (P n_b), the block map m_b [D] (workspace, and trk_map_out).  A block of
//                       all the event's chunks is doa_steer_k's event, bit for bit: one more item per event, the whole event,
//                       writes dir, power and srp of sed_event_doa (where T = 1, block 0's item writes both).  A long event
//                       does not serialise on one workgroup: its blocks are items of their own.
//   doa_track_path_k    one workgroup per event, two score rows of D floats in LDS (D <= 16384: 128 KiB):
//                       s_0 = m_0,  s_b[d] = m_b[d] + max_j s_{b-1}[idx[off[d] + j]]  (first maximum in ascending j, one fp32 add
//                       per cell), the predecessor as 16 bits in a [T][D] back table in the workspace; after block T - 1 the
//                       first maximum of s_{T-1} in ascending d, and one walk down the back table.  trk_dir[b] is the path's
//                       direction, -1 where trk_raw[b] is -1 (a silent block has an all-zero map: the path passes through it).
// Both kernels use plain stores and no atomics; an output depends on its event's own frames alone: not on the launch shape,
// the slices or the workspace.
#include <math.h>
#include <stdint.h>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "contrast_shared.h"

#define TRK_WAVES 8
#define TRK_THREADS (TRK_WAVES * 64)
#define TRK_MAX_DIRS 16384
#define TRK_MAX_FINE 2032                         // Q * max_lag
#define TRK_MAX_W 64
#define TRK_MAX_BLOCKS 256
#define TRK_LDS_MAX ((size_t)160 * 1024)

namespace {

struct TrkArgs {
    const int* steer;           // [D][P] fine lag J of every direction and pair
    const float2* trig;         // [512 Q + 1] (cos, sin)(2 pi k / (2048 Q))
    int D, Q, W;
    int Tm;                     // block slots per event in the outputs: ceil(ceil(max_frames / 32) / W)
    int Tw;                     // ... and in the workspace: ceil(cpe / W) <= Tm
    const int *nbr_off, *nbr_idx;                                // [D + 1], [nnz]; both null: no smoothing
    int* ev_dir_out;            // [E] the whole event's direction, power and map (null): what doa_steer_k writes
    float *ev_power_out, *ev_srp_out;
    int *len_out, *raw_out, *dir_out;                            // [E], [E][Tm], [E][Tm]
    float *power_out, *map_out;                                  // [E][Tm], [E][Tm][D] or null
    float* maps;                // workspace tail: [sub][Tw][D] block maps of a sub-slice (null without smoothing)
    uint16_t* back;             // ... and [sub][Tw][D] predecessors
    int sub0, n_sub;            // the sub-slice: events [sub0, sub0 + n_sub) of the TDOA slice
};

// the blocks of an event located on nf frames: their number T, and block b's first chunk, chunks and frames (b < T)
struct TrkBlock { int T, c0, nc, n; };
__device__ __forceinline__ TrkBlock trk_blocks(int nf, int W, int b) {
    TrkBlock r{0, 0, 0, 0};
    if (nf <= 0) return r;
    const int nch = (nf + TD_CHUNK - 1) / TD_CHUNK, T0 = (nch + W - 1) / W;
    const int nl = nf - TD_CHUNK * W * (T0 - 1);
    r.T = (T0 > 1 && nl < (TD_CHUNK / 2) * W) ? T0 - 1 : T0;
    if (b >= r.T) return r;
    const bool last = b == r.T - 1;
    r.c0 = b * W;
    r.nc = (last ? nch : r.c0 + W) - r.c0;
    r.n = last ? nf - TD_CHUNK * W * b : TD_CHUNK * W;
    return r;
}

size_t trk_lds_bytes(int D, int Q, int max_lag) {
    return ((size_t)2 * PHAT_SPEC + (size_t)2 * (512 * Q + 1) + (size_t)(2 * max_lag * Q + 1) + (size_t)D) * sizeof(float);
}

// CT (sed_event_doa_track_contrast): every block of an event with background frames — and the whole event — steers
// S_b - w_b Sb with the event's one Sb and w_b from the block's frames; an event without them, and every event of
// doa_track_steer_k<false>, takes the plain path and gives the plain bits.
template <bool CT>
__global__ __launch_bounds__(TRK_THREADS) void doa_track_steer_k(const float2* __restrict__ ws, TrkArgs ka, TdArgs ta, CtArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float r_best[TRK_WAVES], r_low[TRK_WAVES];
    __shared__ int r_at[TRK_WAVES], r_none;
    const int tid = threadIdx.x;
    const int Q = ka.Q, D = ka.D, P = ta.P, F = ta.max_lag * Q, Tm = ka.Tm;
    const int NQ = 512 * Q, NH = 1024 * Q, N = 2048 * Q;         // a quarter, a half and the whole of the angle table
    float2* s_S = reinterpret_cast<float2*>(lds);                // [PHAT_SPEC]
    float2* s_trig = s_S + PHAT_SPEC;                            // [NQ + 1]
    float* s_fine = reinterpret_cast<float*>(s_trig + NQ + 1);   // [2 F + 1], lag j at F + j
    float* s_srp = s_fine + 2 * F + 1;                           // [D], entry d belongs to thread d % TRK_THREADS
    for (int k = tid; k <= NQ; k += TRK_THREADS) s_trig[k] = ka.trig[k];
    __syncthreads();
    auto angle = [&](int m) -> float2 { return phat_angle<false>(s_trig, m, NQ, NH, N); };      // (cos, sin)(2 pi m / N), 0 <= m < N
    const long items = (long)ka.n_sub * (Tm + 1);                // per event: its Tm block slots, then the whole event
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int es = (int)(item / (Tm + 1)), b = (int)(item - (long)es * (Tm + 1));
        const int el = ka.sub0 + es;
        const long e = ta.e0 + el;
        int rec, nf;
        long f0;
        td_event_range(ta, e, rec, f0, nf);
        TrkBlock tb = trk_blocks(nf, ka.W, b);
        const long row = e * Tm + b;
        // the whole event (doa_steer_k's outputs) is its only block where T = 1: block 0's item writes both
        const bool blk = b < tb.T, evt = b == Tm ? tb.T > 1 : (b == 0 && tb.T == 1);
        if (b == 0 && tid == 0) ka.len_out[e] = tb.T;
        if (b < Tm && !blk) {                                    // (block-uniform) no such block: -1 / 0
            if (tid == 0) {
                ka.raw_out[row] = -1; ka.power_out[row] = 0.f;
                if (!ka.nbr_off) ka.dir_out[row] = -1;
            }
            if (ka.map_out)
                for (int d = tid; d < D; d += TRK_THREADS) ka.map_out[row * D + d] = 0.f;
        }
        if (b == Tm && nf == 0) {                                // an event without frames
            if (tid == 0) { ka.ev_dir_out[e] = -1; ka.ev_power_out[e] = 0.f; }
            if (ka.ev_srp_out)
                for (int d = tid; d < D; d += TRK_THREADS) ka.ev_srp_out[e * D + d] = 0.f;
        }
        if (!blk && !evt) continue;
        if (b == Tm) { tb.c0 = 0; tb.nc = (nf + TD_CHUNK - 1) / TD_CHUNK; tb.n = nf; }
        const float2* wev = ws + ((long)el * ta.cpe + tb.c0) * P * PHAT_SPEC;    // the block's first chunk is chunk 0 of the sum
        const int nb = CT ? ct_bg_frames(ca, e) : 0;             // (block-uniform)
        for (int p = 0; p < P; ++p) {
            if (CT && nb > 0)
                ct_sum_chunks(s_S, wev, ws + ((long)el * ta.cpe + ca.cpo) * P * PHAT_SPEC, p, P, tb.nc, (nb + TD_CHUNK - 1) / TD_CHUNK,
                              ct_weight(ca.weight, tb.n, nb), tid, TRK_THREADS);
            else
                phat_sum_chunks(s_S, wev, p, P, tb.nc, tid, TRK_THREADS);
            __syncthreads();
            // ── fine lags: item = j = 0..F, 8 lanes per item; fine[+j] = A - B, fine[-j] = A + B ──
            const int grp = tid >> 3, j8 = tid & 7;
            for (int it0 = 0; it0 <= F; it0 += TRK_THREADS / 8) {
                const bool valid = it0 + grp <= F;
                const int j = valid ? it0 + grp : 0;
                const float2 ab = phat_lag_sum(s_S, j8, j, N, angle);
                const float A = ab.x, B = ab.y;
                if (valid && j8 < 2) {
                    const float ny = s_S[LM_N].x * angle((LM_N * j) & (N - 1)).x;        // Re S[1024] cos(pi j / Q): +-S[1024] at Q = 1
                    const bool plus = j8 == 0;
                    if (plus || j > 0) s_fine[plus ? F + j : F - j] = (2.f * (plus ? A - B : A + B) + ny) * (1.f / LM_NFFT);
                }
            }
            __syncthreads();
            // ── steering: srp[d] += fine[J[d][p]]; a lag outside the row (no table of the host's has one) reads its nearest end ──
            for (int d = tid; d < D; d += TRK_THREADS) {
                int jj = ka.steer[(long)d * P + p];
                jj = jj < -F ? -F : jj > F ? F : jj;
                const float v = s_fine[F + jj];
                s_srp[d] = p == 0 ? v : s_srp[d] + v;
            }
            __syncthreads();                                     // S and the fine row may be overwritten by the next pair
        }
        // ── the first maximum of srp in ascending d ──
        float* wmap = blk && ka.maps ? ka.maps + ((long)es * ka.Tw + b) * D : nullptr;
        float* omap = blk && ka.map_out ? ka.map_out + row * D : nullptr;
        float* osrp = evt && ka.ev_srp_out ? ka.ev_srp_out + e * D : nullptr;
        FirstMax fm{-INFINITY, INFINITY, 0x7fffffff};
        for (int d = tid; d < D; d += TRK_THREADS) {
            const float v = s_srp[d];
            if (omap) omap[d] = v;
            if (osrp) osrp[d] = v;
            if (wmap) wmap[d] = v;
            if (v > fm.best) { fm.best = v; fm.at = d; }
            fm.low = fminf(fm.low, v);
        }
        fm = first_max_wave(fm);
        float best = fm.best, low = fm.low;
        int at = fm.at;
        if ((tid & 63) == 0) { r_best[tid >> 6] = best; r_low[tid >> 6] = low; r_at[tid >> 6] = at; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < TRK_WAVES; ++w) {                // (the tie rule of first_max_wave, across the waves)
                const float ob = r_best[w];
                const int oa = r_at[w];
                if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
                low = fminf(low, r_low[w]);
            }
            // digital silence (every value 0) and values that compare with nothing (NaN samples): no direction, never NaN
            const bool none = (best == 0.f && low == 0.f) || at >= D;
            const int raw = none ? -1 : at;
            const float power = none ? 0.f : (float)((double)best / ((double)P * (double)tb.n));
            if (blk) {
                ka.raw_out[row] = raw;
                if (!ka.nbr_off) ka.dir_out[row] = raw;
                ka.power_out[row] = power;
            }
            if (evt) { ka.ev_dir_out[e] = raw; ka.ev_power_out[e] = power; }
            r_none = none && at >= D;                            // a map that compares with nothing: the path reads zeros instead
        }
        __syncthreads();                                         // the wave results may be overwritten by the next item
        if (wmap && r_none)
            for (int d = tid; d < D; d += TRK_THREADS) wmap[d] = 0.f;
        __syncthreads();                                         // ... and r_none
    }
}

__global__ __launch_bounds__(TRK_THREADS) void doa_track_path_k(TrkArgs ka, TdArgs ta) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // two score rows [D]
    __shared__ float r_best[TRK_WAVES];
    __shared__ int r_at[TRK_WAVES];
    const int tid = threadIdx.x;
    const int D = ka.D, Tm = ka.Tm;
    for (int es = blockIdx.x; es < ka.n_sub; es += gridDim.x) {
        const long e = ta.e0 + ka.sub0 + es;
        int rec, nf;
        long f0;
        td_event_range(ta, e, rec, f0, nf);
        const int T = trk_blocks(nf, ka.W, 0).T;
        int* dir = ka.dir_out + e * Tm;
        for (int b = T + tid; b < Tm; b += TRK_THREADS) dir[b] = -1;
        if (T == 0) continue;                                    // (block-uniform)
        const float* maps = ka.maps + (long)es * ka.Tw * D;
        uint16_t* back = ka.back + (long)es * ka.Tw * D;
        float *prev = lds, *cur = lds + D;
        for (int d = tid; d < D; d += TRK_THREADS) prev[d] = maps[d];
        __syncthreads();
        for (int b = 1; b < T; ++b) {
            const float* m = maps + (long)b * D;
            uint16_t* bk = back + (long)b * D;
            // item = direction d, 8 lanes per item: lane l8 takes the row's entries j0 + l8, + 8, ... (neighbouring lanes read
            // neighbouring indices), four index loads in flight at a time; the lanes keep (value, j) and are joined by the
            // xor-1, 2, 4 tree, equal values to the lower j: the first maximum in ascending j
            const int grp = tid >> 3, l8 = tid & 7;
            for (int d0 = 0; d0 < D; d0 += TRK_THREADS / 8) {
                const int d = d0 + grp;
                const bool valid = d < D;
                const int j0 = valid ? ka.nbr_off[d] : 0, j1 = valid ? ka.nbr_off[d + 1] : 0;
                float best = -INFINITY;
                int pos = 0x7fffffff, arg = 0;
                for (int j = j0 + l8; j < j1; j += 32) {
                    int i[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int v = j + 8 * u < j1 ? ka.nbr_idx[j + 8 * u] : 0;
                        i[u] = v < 0 ? 0 : v >= D ? D - 1 : v;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float v = prev[i[u]];
                        if (j + 8 * u < j1 && v > best) { best = v; pos = j + 8 * u; arg = i[u]; }
                    }
                }
#pragma unroll
                for (int o = 1; o < 8; o <<= 1) {
                    const float ob = __shfl_xor(best, o, 64);
                    const int op = __shfl_xor(pos, o, 64), oa = __shfl_xor(arg, o, 64);
                    if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; arg = oa; }
                }
                if (valid && l8 == 0) {
                    if (pos == 0x7fffffff) {                     // nothing above -inf: the row's first entry (a row without entries,
                        arg = d;                                 // which no table of the host's has: d itself)
                        if (j1 > j0) { const int v = ka.nbr_idx[j0]; arg = v < 0 ? 0 : v >= D ? D - 1 : v; }
                        best = prev[arg];
                    }
                    cur[d] = m[d] + best;
                    bk[d] = (uint16_t)arg;
                }
            }
            __syncthreads();                                     // the row is whole; the back table's entries are visible to the walk
            float* t = prev; prev = cur; cur = t;
        }
        // ── the first maximum of the last row in ascending d ──
        FirstMax fm{-INFINITY, INFINITY, 0x7fffffff};
        for (int d = tid; d < D; d += TRK_THREADS) {
            const float v = prev[d];
            if (v > fm.best) { fm.best = v; fm.at = d; }
        }
        fm = first_max_wave(fm);
        if ((tid & 63) == 0) { r_best[tid >> 6] = fm.best; r_at[tid >> 6] = fm.at; }
        __syncthreads();
        if (tid == 0) {
            float best = r_best[0];
            int at = r_at[0];
            for (int w = 1; w < TRK_WAVES; ++w) {
                const float ob = r_best[w];
                const int oa = r_at[w];
                if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
            }
            if (at >= D) at = 0;                                 // (scores that compare with nothing)
            const int* raw = ka.raw_out + e * Tm;
            for (int b = T - 1; b >= 0; --b) {                   // one walk down the back table
                dir[b] = raw[b] < 0 ? -1 : at;
                if (b > 0) {
                    at = back[(long)b * D + at];
                    if (at >= D) at = D - 1;
                }
            }
        }
        __syncthreads();                                         // the rows and the wave results may be overwritten by the next event
    }
}

// what the entry works out before it hands the rest to tdoa_entry
struct TrkCtx {
    CtRun* contrast;            // sed_event_doa_track_contrast: the run whose background chunks every slice steers against (else null)
    TrkArgs ka;
    size_t per_event;           // tail bytes per event of a sub-slice (0 without smoothing)
    long fit;                   // events the tail holds
    int cpe;                    // the chunk slots per event the split was made for
};

size_t trk_tail_bytes(int Tw, int D, int smooth) {
    return smooth ? (((size_t)Tw * D * (sizeof(float) + sizeof(uint16_t)) + 15) & ~(size_t)15) : 0;
}

long trk_cpe(long max_rec_frames, int max_frames) {              // (tdoa.hip: the chunk slots per event)
    const long f = max_rec_frames < max_frames ? max_rec_frames : max_frames;
    return (f + TD_CHUNK - 1) / TD_CHUNK;
}

int trk_hook(void* ctx, const TdArgs& ta, const float2* part, hipStream_t s) {
    const TrkCtx& tc = *static_cast<const TrkCtx*>(ctx);
    const char* who = tc.contrast ? "doa_track_contrast" : ta.cap > 0 ? "event_doa_track_ring" : "event_doa_track";
    if (tc.contrast) SED_TRY(ct_accum(who, *tc.contrast, ta, part, s));
    SED_REQUIRE(ta.cpe == tc.cpe && (!tc.ka.nbr_off || tc.fit >= 1), "%s: the slice has %d chunk slots per event, the workspace was split for "
                "%d (%ld events)", who, ta.cpe, tc.cpe, tc.fit);
    hipError_t err = hipFuncSetAttribute(tc.contrast ? (const void*)doa_track_steer_k<true> : (const void*)doa_track_steer_k<false>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)TRK_LDS_MAX - 256);
    if (err == hipSuccess && tc.ka.nbr_off)
        err = hipFuncSetAttribute((const void*)doa_track_path_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TRK_LDS_MAX - 256);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    TrkArgs ka = tc.ka;
    const long step = ka.nbr_off ? tc.fit : ta.n_ev;             // without smoothing nothing is kept: the slice is one sub-slice
    for (long s0 = 0; s0 < ta.n_ev; s0 += step) {
        ka.sub0 = (int)s0;
        ka.n_sub = (int)(ta.n_ev - s0 < step ? ta.n_ev - s0 : step);
        const long items = (long)ka.n_sub * (ka.Tm + 1);
        const unsigned blocks = (unsigned)(items < 2048 ? items : 2048);
        if (tc.contrast)
            doa_track_steer_k<true><<<blocks, TRK_THREADS, trk_lds_bytes(ka.D, ka.Q, ta.max_lag), s>>>(part, ka, ta, tc.contrast->ca);
        else
            doa_track_steer_k<false><<<blocks, TRK_THREADS, trk_lds_bytes(ka.D, ka.Q, ta.max_lag), s>>>(part, ka, ta, CtArgs{});
        SED_LAUNCH_CHECK(tc.contrast ? "doa_track_contrast (steer)" : ta.cap > 0 ? "event_doa_track_ring (steer)" : "event_doa_track (steer)");
        if (ka.nbr_off) {
            doa_track_path_k<<<ka.n_sub < 2048 ? ka.n_sub : 2048, TRK_THREADS, (size_t)2 * ka.D * sizeof(float), s>>>(ka, ta);
            SED_LAUNCH_CHECK(ta.cap > 0 ? "event_doa_track_ring (path)" : "event_doa_track (path)");
        }
    }
    return 0;
}

// the arguments the two entries add to their TDOA siblings, checked before anything is enqueued; and the split of the workspace
int trk_check(const char* who, bool ring, const long* host, long cap, int R, int channels, long E, int hop, int max_lag, int max_frames,
              const int* steer_lags, int D, int Q, const float* trig, int* dir_out, float* power_out, float* srp_out, int block_chunks, const int* nbr_off,
              const int* nbr_idx, int* trk_len_out, int* trk_raw_out, int* trk_dir_out, float* trk_power_out, float* trk_map_out,
              void* workspace, size_t workspace_bytes, TrkCtx& tc, size_t& td_bytes, size_t extra_tab = 0, int extra_chunks = 0) {
    SED_REQUIRE(steer_lags && trig && dir_out && power_out, "%s: null pointer (steering lags, angle table, dir_out or power_out)", who);
    SED_REQUIRE(trk_len_out && trk_raw_out && trk_dir_out && trk_power_out, "%s: null pointer (trk_len_out, trk_raw_out, trk_dir_out or "
                "trk_power_out)", who);
    SED_REQUIRE(D >= 1 && D <= TRK_MAX_DIRS, "%s: 1 to %d directions, got %d", who, TRK_MAX_DIRS, D);
    SED_REQUIRE(Q == 1 || Q == 2 || Q == 4 || Q == 8 || Q == 16, "%s: oversample must be 1, 2, 4, 8 or 16, got %d", who, Q);
    SED_REQUIRE(max_lag >= 1 && max_lag <= TD_MAX_LAG, "%s: max_lag must be in [1,%d], got %d", who, TD_MAX_LAG, max_lag);
    SED_REQUIRE((long)Q * max_lag <= TRK_MAX_FINE, "%s: oversample * max_lag = %ld exceeds %d fine lags a side", who, (long)Q * max_lag,
                TRK_MAX_FINE);
    SED_REQUIRE(((uintptr_t)trig & 7) == 0, "%s: the angle table must be 8-byte aligned", who);
    const size_t lds = trk_lds_bytes(D, Q, max_lag);
    SED_REQUIRE(lds + 256 <= TRK_LDS_MAX, "%s: %d directions at oversample %d need %zu B of the 160 KiB LDS", who, D, Q, lds);
    SED_REQUIRE(block_chunks >= 1 && block_chunks <= TRK_MAX_W, "%s: block_chunks must be in [1,%d], got %d", who, TRK_MAX_W, block_chunks);
    SED_REQUIRE((nbr_off == nullptr) == (nbr_idx == nullptr), "%s: the neighbour table needs both nbr_off and nbr_idx (both null: no smoothing)",
                who);
    SED_REQUIRE(max_frames >= 1, "%s: max_frames must be >= 1, got %d", who, max_frames);
    const long Tm = (((long)max_frames + TD_CHUNK - 1) / TD_CHUNK + block_chunks - 1) / block_chunks;
    SED_REQUIRE(Tm <= TRK_MAX_BLOCKS, "%s: max_frames = %d in blocks of %d chunks is %ld blocks an event, more than %d", who, max_frames,
                block_chunks, Tm, TRK_MAX_BLOCKS);
    tc = TrkCtx{};
    tc.ka = TrkArgs{steer_lags, reinterpret_cast<const float2*>(trig), D, Q, block_chunks, (int)Tm, 0, nbr_off, nbr_idx, dir_out,
                    power_out, srp_out, trk_len_out, trk_raw_out, trk_dir_out, trk_power_out, trk_map_out, nullptr, nullptr, 0, 0};
    td_bytes = workspace_bytes;
    // what tdoa_entry refuses in its own words (or E = 0, where nothing is launched) needs no split
    if (!host || !workspace || R < 1 || channels < 2 || channels > TD_MAX_CH || hop < 1 || E <= 0 || (ring && cap < LM_NFFT)) return 0;
    long longest = 0;
    for (int r = 0; r < R; ++r) {
        const long n = ring ? cap : host[2 * ((long)r * channels) + 1];
        if (n > longest) longest = n;
    }
    const long cpe = trk_cpe(1 + longest / hop, max_frames);
    if (cpe < 1 || cpe > 0x7fffffffL) return 0;                  // (recordings tdoa_entry refuses)
    tc.cpe = (int)cpe + extra_chunks;                            // (an event's background chunks lie behind its own)
    tc.ka.Tw = (int)((cpe + block_chunks - 1) / block_chunks);
    tc.per_event = trk_tail_bytes(tc.ka.Tw, D, nbr_off != nullptr);
    if (!tc.per_event) return 0;                                 // no smoothing: nothing is kept, the workspace is the TDOA one
    const size_t tab = (ring ? rec_ring_table_bytes(R) : rec_table_bytes(R, channels)) + extra_tab;
    const size_t one = (size_t)tc.cpe * (channels * (channels - 1) / 2) * TD_ROW_BYTES + tc.per_event;
    SED_REQUIRE(workspace_bytes >= tab + one, "%s: workspace of %zu bytes, at least %zu needed (one event)", who, workspace_bytes, tab + one);
    const size_t wb = workspace_bytes & ~(size_t)15;             // (the table, a row and an event's tail are multiples of 16 bytes)
    tc.fit = (long)((wb - tab) / one);
    if (tc.fit > E) tc.fit = E;
    if (tc.fit > 65535) tc.fit = 65535;                          // (a TDOA slice has no more events)
    td_bytes = wb - (size_t)tc.fit * tc.per_event;
    tc.ka.maps = reinterpret_cast<float*>((char*)workspace + td_bytes);
    tc.ka.back = reinterpret_cast<uint16_t*>(tc.ka.maps + (size_t)tc.fit * tc.ka.Tw * D);
    return 0;
}

size_t trk_workspace_bytes(size_t td, int channels, long E, long max_rec_frames, int max_frames, int D, int block_chunks, int smooth) {
    if (td == 0 || D < 1 || D > TRK_MAX_DIRS || block_chunks < 1 || block_chunks > TRK_MAX_W) return 0;
    if ((((long)max_frames + TD_CHUNK - 1) / TD_CHUNK + block_chunks - 1) / block_chunks > TRK_MAX_BLOCKS) return 0;
    const long cpe = trk_cpe(max_rec_frames, max_frames);
    return td + (size_t)E * trk_tail_bytes((int)((cpe + block_chunks - 1) / block_chunks), D, smooth);
}

}  // namespace

// the TDOA workspace and, with smoothing, a tail of block maps and back tables: [Tw][D] floats and [Tw][D] 16-bit words an event
extern "C" size_t sed_event_doa_track_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames, int D,
                                                      int block_chunks, int smooth) {
    const size_t td = sed_event_tdoa_workspace_bytes(R, channels, E, max_n_samples, hop, max_frames);
    return td ? trk_workspace_bytes(td, channels, E, 1 + max_n_samples / hop, max_frames, D, block_chunks, smooth) : 0;
}

extern "C" int sed_event_doa_track(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                                   size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                                   const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                                   float* lag_out, float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D,
                                   int Q, const float* trig, int* dir_out, float* power_out, float* srp_out, int block_chunks,
                                   const int* nbr_off, const int* nbr_idx, int* trk_len_out, int* trk_raw_out, int* trk_dir_out,
                                   float* trk_power_out, float* trk_map_out, void* workspace, size_t workspace_bytes, void* stream) {
    TrkCtx tc;
    size_t td_bytes;
    SED_TRY(trk_check("event_doa_track", false, clips_host, 0, R, channels, E, hop, max_lag, max_frames, steer_lags, D, Q, trig, dir_out,
                      power_out, srp_out, block_chunks, nbr_off, nbr_idx, trk_len_out, trk_raw_out, trk_dir_out, trk_power_out, trk_map_out, workspace,
                      workspace_bytes, tc, td_bytes));
    return tdoa_entry("event_doa_track", {pcm, false, 0, pcm_len, R, channels, clips_host},
                      {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                      {tables, tables_bytes, pad_mode, max_lag, 0, 0}, {lag_out, strength_out, frames_out, acc_out}, workspace, td_bytes,
                      stream, trk_hook, &tc);
}

extern "C" size_t sed_event_doa_track_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames, int D,
                                                           int block_chunks, int smooth) {
    const size_t td = sed_event_tdoa_ring_workspace_bytes(R, channels, E, cap, hop, max_frames);
    return td ? trk_workspace_bytes(td, channels, E, 1 + cap / hop, max_frames, D, block_chunks, smooth) : 0;
}

extern "C" int sed_event_doa_track_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                        const void* tables, size_t tables_bytes, const int* ev_rec, const int* ev_onset,
                                        const int* ev_offset, const int* ev_peak_frame, long E, int time_factor, int hop, int max_lag,
                                        int max_frames, int lat_frames, int history_frames, float* lag_out, float* strength_out,
                                        int* frames_out, float* acc_out, const int* steer_lags, int D, int Q, const float* trig,
                                        int* dir_out, float* power_out, float* srp_out, int block_chunks, const int* nbr_off,
                                        const int* nbr_idx, int* trk_len_out, int* trk_raw_out, int* trk_dir_out, float* trk_power_out,
                                        float* trk_map_out, void* workspace, size_t workspace_bytes, void* stream) {
    TrkCtx tc;
    size_t td_bytes;
    SED_TRY(trk_check("event_doa_track_ring", true, n_host, cap, R, channels, E, hop, max_lag, max_frames, steer_lags, D, Q, trig, dir_out,
                      power_out, srp_out, block_chunks, nbr_off, nbr_idx, trk_len_out, trk_raw_out, trk_dir_out, trk_power_out, trk_map_out,
                      workspace, workspace_bytes, tc, td_bytes));
    return tdoa_entry("event_doa_track_ring", {ring, true, cap, ring_len, R, channels, n_host},
                      {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                      {tables, tables_bytes, 0, max_lag, lat_frames, history_frames}, {lag_out, strength_out, frames_out, acc_out},
                      workspace, td_bytes, stream, trk_hook, &tc);
}

// ───────────────────────── contrast SRP-PHAT ─────────────────────────
// the workspace of sed_event_doa_contrast and, with smoothing, the tail of sed_event_doa_track
extern "C" size_t sed_event_doa_track_contrast_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames, int D,
                                                               int block_chunks, int smooth, long mask_frames, int frames) {
    const size_t one = sed_event_tdoa_workspace_bytes(R, channels, 1, max_n_samples, hop, max_frames);
    if (one == 0 || E < 0 || !ct_sizes_ok(R, mask_frames, frames)) return 0;
    const size_t tab = rec_table_bytes(R, channels);
    const size_t bg = (size_t)((frames + TD_CHUNK - 1) / TD_CHUNK) * (channels * (channels - 1) / 2) * TD_ROW_BYTES;
    const size_t td = tab + act_mask_bytes(R, mask_frames) + (size_t)E * (one - tab + bg);
    return trk_workspace_bytes(td, channels, E, 1 + max_n_samples / hop, max_frames, D, block_chunks, smooth);
}

extern "C" int sed_event_doa_track_contrast(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                                            size_t tables_bytes, const int* ev_rec, const int* ev_cls, const int* ev_onset,
                                            const int* ev_offset, const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode,
                                            int max_lag, int max_frames, int n_classes, int frames, int search, int guard, int min_frames,
                                            double weight, float* lag_out, float* strength_out, int* frames_out, float* acc_out,
                                            const int* steer_lags, int D, int Q, const float* trig, int* dir_out, float* power_out,
                                            float* srp_out, int block_chunks, const int* nbr_off, const int* nbr_idx, int* trk_len_out,
                                            int* trk_raw_out, int* trk_dir_out, float* trk_power_out, float* trk_map_out, int* bg_frames_out,
                                            int* bg_sel_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "doa_track_contrast";
    CtRun run{};
    run.cs = CtSettings{ev_cls, n_classes, frames, search, guard, min_frames, weight, bg_frames_out, bg_sel_out};
    SED_TRY(ct_check(who, E, run.cs));
    run.pcm = pcm; run.tables = tables; run.pad_mode = pad_mode;
    run.cpb = (frames + TD_CHUNK - 1) / TD_CHUNK;
    const TdExtra extra{act_mask_bytes(R, act_mask_frames(clips_host, R, channels, time_factor, hop)), run.cpb, ct_pre, &run};
    TrkCtx tc;
    size_t td_bytes;
    SED_TRY(trk_check(who, false, clips_host, 0, R, channels, E, hop, max_lag, max_frames, steer_lags, D, Q, trig, dir_out, power_out, srp_out,
                      block_chunks, nbr_off, nbr_idx, trk_len_out, trk_raw_out, trk_dir_out, trk_power_out, trk_map_out, workspace,
                      workspace_bytes, tc, td_bytes, extra.tab_bytes, extra.chunks));
    tc.contrast = &run;
    return tdoa_entry(who, {pcm, false, 0, pcm_len, R, channels, clips_host},
                      {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                      {tables, tables_bytes, pad_mode, max_lag, 0, 0}, {lag_out, strength_out, frames_out, acc_out}, workspace, td_bytes,
                      stream, trk_hook, &tc, &extra);
}
