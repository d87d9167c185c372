// doa.hip — per-event direction of arrival for a known array: SRP-PHAT over a grid of directions: sed_event_doa.
//
// For a located event (tdoa_shared.h: the frames sed_event_tdoa locates it on) and microphone pair p = (i, j), i < j, with S the
// accumulated whitened cross spectrum of tdoa.hip (the same chunk partials, added in the same order), Q the oversampling factor
// and F = max_lag Q:
//   fine_p[j] = (1/2048) (S[0] + Re S[1024] cos(pi j / Q) + 2 sum_{k=1..1023} Re(S[k] e^{+2 pi i k j / (2048 Q)})),  |j| <= F
//               — the band-limited correlation at the fractional lag j / Q, exactly, not an interpolation of the integer lags —
//   srp[d]    = sum_p fine_p[J[d][p]]            fp32 adds in ascending p; J[d][p] = round(Q tau[d][p]) is made on the host
//   dir       = the first maximum of srp in ascending d;  power = srp[dir] / (P n_frames)
// dir = -1 and power = 0 for an event without frames and for digital silence (every srp value 0).
//
// Shape (gfx950): a third plain launch per slice of the event table, after tdoa_accum_k and tdoa_finish_k (tdoa_shared.h: the
// hook of the shared runner), while the slice's chunk partials are in the workspace.  One persistent workgroup of 8 waves takes
// one event at a time; per pair it re-forms S in LDS, synthesises the 2 F + 1 fine lags into LDS — item = lag j >= 0, 8 lanes
// per item, bins j8 + 8 i in ascending order, the 8 partial sums joined by the xor-1, 2, 4 shuffle tree, +j and -j from the
// same two sums: phat_lag_sum (phat_shared.h), which tdoa_finish_k calls too, with a table of 2048 Q angles — and every thread
// adds fine[J[d][p]] to the srp[d] it owns (LDS).  At Q = 1 the table holds the values of tdoa_finish_k's: fine[j] is acc[j] bit for bit.
// The angle table is the quarter wave (cos, sin)(2 pi k / (2048 Q)), k = 0 .. 512 Q (float64 values rounded once, made on the
// host), unfolded by index at every read (phat_angle): 64 KiB at Q = 16, beside srp (64 KiB at D = 16384), S
// (8 KiB) and one fine row (16 KiB at F = 2032) within the 160 KiB of LDS.  The fine row is contiguous floats: neighbouring j —
// what neighbouring directions read — are neighbouring banks, and equal j is a broadcast.
#include <math.h>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "contrast_shared.h"

#define DOA_WAVES 8
#define DOA_THREADS (DOA_WAVES * 64)
#define DOA_MAX_DIRS 16384
#define DOA_MAX_FINE 2032                         // Q * max_lag
#define DOA_LDS_MAX ((size_t)160 * 1024)

namespace {

struct DoaArgs {
    const int* steer;           // [D][P] fine lag J of every direction and pair
    const float2* trig;         // [512 Q + 1] (cos, sin)(2 pi k / (2048 Q))
    int D, Q;
    int* dir_out;               // [E]
    float* power_out;           // [E]
    float* srp_out;             // [E][D] or null
};

size_t doa_lds_bytes(int D, int Q, int max_lag) {
    return ((size_t)2 * PHAT_SPEC + (size_t)2 * (512 * Q + 1) + (size_t)(2 * max_lag * Q + 1) + (size_t)D) * sizeof(float);
}

// CT (sed_event_doa_contrast): an event with background frames steers S' = S - w Sb, formed in LDS where S is formed; an
// event without them, and every event of doa_steer_k<false>, takes the plain path and gives the plain bits.
template <bool CT>
__global__ __launch_bounds__(DOA_THREADS) void doa_steer_k(const float2* __restrict__ ws, DoaArgs da, TdArgs ta, CtArgs ca) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float r_best[DOA_WAVES], r_low[DOA_WAVES];
    __shared__ int r_at[DOA_WAVES];
    const int tid = threadIdx.x;
    const int Q = da.Q, D = da.D, P = ta.P, F = ta.max_lag * Q;
    const int NQ = 512 * Q, NH = 1024 * Q, N = 2048 * Q;         // a quarter, a half and the whole of the angle table
    float2* s_S = reinterpret_cast<float2*>(lds);                // [PHAT_SPEC]
    float2* s_trig = s_S + PHAT_SPEC;                            // [NQ + 1]
    float* s_fine = reinterpret_cast<float*>(s_trig + NQ + 1);   // [2 F + 1], lag j at F + j
    float* s_srp = s_fine + 2 * F + 1;                           // [D], entry d belongs to thread d % DOA_THREADS
    for (int k = tid; k <= NQ; k += DOA_THREADS) s_trig[k] = da.trig[k];
    __syncthreads();
    auto angle = [&](int m) -> float2 { return phat_angle<false>(s_trig, m, NQ, NH, N); };      // (cos, sin)(2 pi m / N), 0 <= m < N
    for (int el = blockIdx.x; el < ta.n_ev; el += gridDim.x) {
        const long e = ta.e0 + el;
        int rec, nf;
        long f0;
        td_event_range(ta, e, rec, f0, nf);
        if (nf == 0) {                                           // (block-uniform)
            if (tid == 0) { da.dir_out[e] = -1; da.power_out[e] = 0.f; }
            if (da.srp_out)
                for (int d = tid; d < D; d += DOA_THREADS) da.srp_out[e * D + d] = 0.f;
            continue;
        }
        const int nch = (nf + TD_CHUNK - 1) / TD_CHUNK;
        const float2* wev = ws + (long)el * ta.cpe * P * PHAT_SPEC;
        const int nb = CT ? ct_bg_frames(ca, e) : 0;             // (block-uniform)
        for (int p = 0; p < P; ++p) {
            if (CT && nb > 0)
                ct_sum_chunks(s_S, wev, wev + (long)ca.cpo * P * PHAT_SPEC, p, P, nch, (nb + TD_CHUNK - 1) / TD_CHUNK,
                              ct_weight(ca.weight, nf, nb), tid, DOA_THREADS);
            else
                phat_sum_chunks(s_S, wev, p, P, nch, tid, DOA_THREADS);
            __syncthreads();
            // ── fine lags: item = j = 0..F, 8 lanes per item; fine[+j] = A - B, fine[-j] = A + B ──
            const int grp = tid >> 3, j8 = tid & 7;
            for (int it0 = 0; it0 <= F; it0 += DOA_THREADS / 8) {
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
            for (int d = tid; d < D; d += DOA_THREADS) {
                int jj = da.steer[(long)d * P + p];
                jj = jj < -F ? -F : jj > F ? F : jj;
                const float v = s_fine[F + jj];
                s_srp[d] = p == 0 ? v : s_srp[d] + v;
            }
            __syncthreads();                                     // S and the fine row may be overwritten by the next pair
        }
        // ── the first maximum of srp in ascending d ──
        FirstMax fm{-INFINITY, INFINITY, 0x7fffffff};
        for (int d = tid; d < D; d += DOA_THREADS) {
            const float v = s_srp[d];
            if (da.srp_out) da.srp_out[e * D + d] = v;
            if (v > fm.best) { fm.best = v; fm.at = d; }
            fm.low = fminf(fm.low, v);
        }
        fm = first_max_wave(fm);
        float best = fm.best, low = fm.low;
        int at = fm.at;
        if ((tid & 63) == 0) { r_best[tid >> 6] = best; r_low[tid >> 6] = low; r_at[tid >> 6] = at; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < DOA_WAVES; ++w) {                // (the tie rule of first_max_wave, across the waves)
                const float ob = r_best[w];
                const int oa = r_at[w];
                if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
                low = fminf(low, r_low[w]);
            }
            // digital silence (every value 0) and values that compare with nothing (NaN samples): no direction, never NaN
            const bool none = (best == 0.f && low == 0.f) || at >= D;
            da.dir_out[e] = none ? -1 : at;
            da.power_out[e] = none ? 0.f : (float)((double)best / ((double)P * (double)nf));
        }
        __syncthreads();                                         // the wave results may be overwritten by the next event
    }
}

int doa_hook(void* ctx, const TdArgs& ta, const float2* part, hipStream_t s) {
    const DoaArgs& da = *static_cast<const DoaArgs*>(ctx);
    const char* who = ta.cap > 0 ? "event_doa_ring (steer)" : "event_doa (steer)";
    const hipError_t err = hipFuncSetAttribute((const void*)doa_steer_k<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOA_LDS_MAX - 256);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    const int blocks = ta.n_ev < 2048 ? ta.n_ev : 2048;
    doa_steer_k<false><<<blocks, DOA_THREADS, doa_lds_bytes(da.D, da.Q, ta.max_lag), s>>>(part, da, ta, CtArgs{});
    SED_LAUNCH_CHECK(who);
    return 0;
}

// sed_event_doa_contrast: the slice's background chunks behind its own, then the steer launch that subtracts them
struct DoaContrast { DoaArgs da; CtRun run; };

int doa_contrast_hook(void* ctx, const TdArgs& ta, const float2* part, hipStream_t s) {
    DoaContrast& dc = *static_cast<DoaContrast*>(ctx);
    const char* who = "doa_contrast (steer)";
    SED_TRY(ct_accum("doa_contrast", dc.run, ta, part, s));
    const hipError_t err = hipFuncSetAttribute((const void*)doa_steer_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DOA_LDS_MAX - 256);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    const int blocks = ta.n_ev < 2048 ? ta.n_ev : 2048;
    doa_steer_k<true><<<blocks, DOA_THREADS, doa_lds_bytes(dc.da.D, dc.da.Q, ta.max_lag), s>>>(part, dc.da, ta, dc.run.ca);
    SED_LAUNCH_CHECK(who);
    return 0;
}

// the arguments the two entries add to their TDOA siblings, checked before anything is enqueued
int doa_check(const char* who, const int* steer_lags, int D, int Q, const float* trig, int max_lag, int* dir_out, float* power_out,
              float* srp_out, DoaArgs& da) {
    SED_REQUIRE(steer_lags && trig && dir_out && power_out, "%s: null pointer (steering lags, angle table, dir_out or power_out)", who);
    SED_REQUIRE(D >= 1 && D <= DOA_MAX_DIRS, "%s: 1 to %d directions, got %d", who, DOA_MAX_DIRS, D);
    SED_REQUIRE(Q == 1 || Q == 2 || Q == 4 || Q == 8 || Q == 16, "%s: oversample must be 1, 2, 4, 8 or 16, got %d", who, Q);
    SED_REQUIRE(max_lag >= 1 && max_lag <= TD_MAX_LAG, "%s: max_lag must be in [1,%d], got %d", who, TD_MAX_LAG, max_lag);
    SED_REQUIRE((long)Q * max_lag <= DOA_MAX_FINE, "%s: oversample * max_lag = %ld exceeds %d fine lags a side", who, (long)Q * max_lag,
                DOA_MAX_FINE);
    SED_REQUIRE(((uintptr_t)trig & 7) == 0, "%s: the angle table must be 8-byte aligned", who);
    const size_t lds = doa_lds_bytes(D, Q, max_lag);
    SED_REQUIRE(lds + 256 <= DOA_LDS_MAX, "%s: %d directions at oversample %d need %zu B of the 160 KiB LDS", who, D, Q, lds);
    da = DoaArgs{steer_lags, reinterpret_cast<const float2*>(trig), D, Q, dir_out, power_out, srp_out};
    return 0;
}

}  // namespace

// the workspace is the TDOA one: the steering launch reads the slice's chunk partials in place and needs nothing more
extern "C" size_t sed_event_doa_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames) {
    return sed_event_tdoa_workspace_bytes(R, channels, E, max_n_samples, hop, max_frames);
}

extern "C" int sed_event_doa(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                             size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                             const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                             float* lag_out, float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D,
                             int Q, const float* trig, int* dir_out, float* power_out, float* srp_out, void* workspace,
                             size_t workspace_bytes, void* stream) {
    DoaArgs da;
    SED_TRY(doa_check("event_doa", steer_lags, D, Q, trig, max_lag, dir_out, power_out, srp_out, da));
    return tdoa_entry("event_doa", {pcm, false, 0, pcm_len, R, channels, clips_host},
                             {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                             {tables, tables_bytes, pad_mode, max_lag, 0, 0}, {lag_out, strength_out, frames_out, acc_out}, workspace,
                             workspace_bytes, stream, doa_hook, &da);
}

extern "C" size_t sed_event_doa_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames) {
    return sed_event_tdoa_ring_workspace_bytes(R, channels, E, cap, hop, max_frames);
}

extern "C" int sed_event_doa_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                  const void* tables, size_t tables_bytes, const int* ev_rec, const int* ev_onset,
                                  const int* ev_offset, const int* ev_peak_frame, long E, int time_factor, int hop, int max_lag,
                                  int max_frames, int lat_frames, int history_frames, float* lag_out, float* strength_out,
                                  int* frames_out, float* acc_out, const int* steer_lags, int D, int Q, const float* trig, int* dir_out,
                                  float* power_out, float* srp_out, void* workspace, size_t workspace_bytes, void* stream) {
    DoaArgs da;
    SED_TRY(doa_check("event_doa_ring", steer_lags, D, Q, trig, max_lag, dir_out, power_out, srp_out, da));
    return tdoa_entry("event_doa_ring", {ring, true, cap, ring_len, R, channels, n_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                           {tables, tables_bytes, 0, max_lag, lat_frames, history_frames}, {lag_out, strength_out, frames_out, acc_out},
                           workspace, workspace_bytes, stream, doa_hook, &da);
}

// ───────────────────────── contrast SRP-PHAT ─────────────────────────
// workspace: the recording table, mask_off [R] and the mask of mask_frames words, then, for every event, its own chunk slots and
// ceil(frames / 32) more for its background: rows of 1026 float2 per pair
extern "C" size_t sed_event_doa_contrast_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames,
                                                         long mask_frames, int frames) {
    const size_t one = sed_event_tdoa_workspace_bytes(R, channels, 1, max_n_samples, hop, max_frames);
    if (one == 0 || E < 0 || !ct_sizes_ok(R, mask_frames, frames)) return 0;
    const size_t tab = rec_table_bytes(R, channels);
    const size_t bg = (size_t)((frames + TD_CHUNK - 1) / TD_CHUNK) * (channels * (channels - 1) / 2) * TD_ROW_BYTES;
    return tab + act_mask_bytes(R, mask_frames) + (size_t)E * (one - tab + bg);
}

extern "C" int sed_event_doa_contrast(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                                      size_t tables_bytes, const int* ev_rec, const int* ev_cls, const int* ev_onset, const int* ev_offset,
                                      const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                                      int n_classes, int frames, int search, int guard, int min_frames, double weight, float* lag_out,
                                      float* strength_out, int* frames_out, float* acc_out, const int* steer_lags, int D, int Q,
                                      const float* trig, int* dir_out, float* power_out, float* srp_out, int* bg_frames_out,
                                      int* bg_sel_out, void* workspace, size_t workspace_bytes, void* stream) {
    DoaContrast dc{};
    SED_TRY(doa_check("doa_contrast", steer_lags, D, Q, trig, max_lag, dir_out, power_out, srp_out, dc.da));
    dc.run.cs = CtSettings{ev_cls, n_classes, frames, search, guard, min_frames, weight, bg_frames_out, bg_sel_out};
    SED_TRY(ct_check("doa_contrast", E, dc.run.cs));
    dc.run.pcm = pcm; dc.run.tables = tables; dc.run.pad_mode = pad_mode;
    dc.run.cpb = (frames + TD_CHUNK - 1) / TD_CHUNK;
    const TdExtra extra{act_mask_bytes(R, act_mask_frames(clips_host, R, channels, time_factor, hop)), dc.run.cpb, ct_pre, &dc.run};
    return tdoa_entry("doa_contrast", {pcm, false, 0, pcm_len, R, channels, clips_host},
                      {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                      {tables, tables_bytes, pad_mode, max_lag, 0, 0}, {lag_out, strength_out, frames_out, acc_out}, workspace,
                      workspace_bytes, stream, doa_contrast_hook, &dc, &extra);
}
