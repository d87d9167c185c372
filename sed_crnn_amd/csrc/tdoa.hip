// tdoa.hip — per-event time difference of arrival from accumulated GCC-PHAT: sed_event_tdoa.
//
// For a detected event (rec, onset, offset, peak_frame in output frames), the frames [f0, f1) it is located on
// (td_event_range below; sed_crnn_amd/localize.py states the same rule on the host) and microphone pair (i, j), i < j:
//   Pk_f[k] = G_f[k] / |G_f[k]|, G_f = X_i conj X_j of frame f     (phat_bin of phat_shared.h: gcc.hip's Pk)
//   S[k]    = sum_{f = f0}^{f1 - 1} Pk_f[k]
//   acc[tau] = (1/2048) (S[0] + (-1)^tau S[1024] + 2 sum_{k=1..1023} Re(S[k] e^{+2 pi i k tau / 2048})),  |tau| <= max_lag + 1
//   t* = first maximum of acc over |tau| <= max_lag;  lag = t* + 0.5 (l - r) / (l - 2 m + r) where that denominator is < 0;
//   strength = m / (f1 - f0).
// The inverse transform is linear, so the lags are synthesised once per (event, pair) from the summed cross spectra instead of
// once per frame.
//
// Shape (gfx950), two plain launches per slice of the event table; no workgroup waits on another and there are no atomics:
//   tdoa_accum_k   one workgroup of 8 waves owns one CHUNK: TD_CHUNK consecutive frames of one event, counted from the event's
//                  f0.  Per frame: the FFT of the C channels into LDS and the whitening of every pair (steps 1 and 2 of
//                  gcc_phat_k: the functions it calls), added into a per-pair accumulator [pairs of the batch][1026] float2 in LDS in
//                  ascending frame order; every accumulator entry belongs to one lane.  Where the spectra fit LDS twice
//                  (C <= 4) the transforming waves run one frame ahead of the whitening waves.  The chunk's partial sums go
//                  to the workspace.  Where the P accumulators do not fit beside the spectra (C >= 5) the pairs go in batches and the
//                  chunk's frames are transformed again for every batch.
//   tdoa_finish_k  per (event, pair): the chunk partials added in ascending chunk order, the 2 max_lag + 3 lags by the
//                  8-lanes-per-(pair, tau) direct sum against the exact 2048-entry (cos, sin) table (phat_lag_sum), peak and parabola.
// Every output is therefore summed in ONE order that depends on the event's own samples and frame range alone: not on the
// other events, the slice, the clip's place in the buffer, the load path or the launch shape.
//
// Live feeds: sed_stream_ring_write keeps every lane's last cap samples in a ring, and sed_event_tdoa_ring is the same
// two launches with tdoa_accum_k<true>, which loads a frame from the ring — directly where it does not wrap, through the guarded
// loads where it does — and with td_event_range also refusing what the stream's rule or the ring's depth refuses.
//
// The host side of both entries is behind tdoa_entry (tdoa_shared.h), which doa.hip calls with a hook
// that steers every slice while its partials are in the workspace; the entries here pass none.
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "tdoa_accum.h"

#define TD_FIN_THREADS 256                        // (the accumulate kernel's sizes: tdoa_accum.h)

// (TdArgs, td_event_range and the workspace's row layout: tdoa_shared.h, shared with doa.hip)
namespace {

// The chunk's frames are f0 + fc0 .. of the event; the body is td_accum_chunk (tdoa_accum.h), which contrast.hip runs on other frames.
template <bool RING>
__global__ __launch_bounds__(TD_THREADS) void tdoa_accum_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                           float2* __restrict__ ws, int pad_mode, TdArgs ta) {
    const long e = ta.e0 + blockIdx.y;
    int rec, nf;
    long f0;
    td_event_range(ta, e, rec, f0, nf);
    const int fc0 = blockIdx.x * TD_CHUNK;                       // the chunk's first frame, counted from f0
    if (fc0 >= nf) return;                                       // (block-uniform: before any barrier)
    const int fc1 = fc0 + TD_CHUNK < nf ? fc0 + TD_CHUNK : nf;
    float2* wrow = ws + ((long)blockIdx.y * ta.cpe + blockIdx.x) * ta.P * PHAT_SPEC;
    td_accum_chunk<RING>(pcm, tables, wrow, pad_mode, ta, rec, fc1 - fc0, [&](int step) -> long { return f0 + fc0 + step; });
}

// One (persistent) workgroup per event at a time: every pair of the event in turn.
__global__ __launch_bounds__(TD_FIN_THREADS) void tdoa_finish_k(const uint32_t* __restrict__ tables, const float2* __restrict__ ws,
                                                                float* __restrict__ lag_out, float* __restrict__ strength_out,
                                                                int* __restrict__ frames_out, float* __restrict__ acc_out, TdArgs ta) {
    __shared__ __attribute__((aligned(16))) float2 s_lag[LM_NFFT];
    __shared__ __attribute__((aligned(16))) float2 s_S[PHAT_SPEC];
    __shared__ float s_cc[2 * TD_MAX_LAG + 3];
    const int tid = threadIdx.x;
    phat_lag_table(s_lag, reinterpret_cast<const float2*>(tables + LM_OFF_PW), tid, TD_FIN_THREADS);
    __syncthreads();
    const int P = ta.P, ML = ta.max_lag, T = ML + 2, W = 2 * ML + 3;
    for (int el = blockIdx.x; el < ta.n_ev; el += gridDim.x) {
        const long e = ta.e0 + el;
        int rec, nf;
        long f0;
        td_event_range(ta, e, rec, f0, nf);
        if (tid == 0) frames_out[e] = nf;
        if (nf == 0) {                                           // (block-uniform)
            for (int p = tid; p < P; p += TD_FIN_THREADS) { lag_out[e * P + p] = 0.f; strength_out[e * P + p] = 0.f; }
            if (acc_out)
                for (int i = tid; i < P * W; i += TD_FIN_THREADS) acc_out[e * P * W + i] = 0.f;
            continue;
        }
        const int nch = (nf + TD_CHUNK - 1) / TD_CHUNK;
        const float2* wev = ws + (long)el * ta.cpe * P * PHAT_SPEC;
        for (int p = 0; p < P; ++p) {
            phat_sum_chunks(s_S, wev, p, P, nch, tid, TD_FIN_THREADS);
            __syncthreads();
            // ── lag synthesis: item = tau = 0..max_lag+1, 8 lanes per item; cc[+tau] = A - B, cc[-tau] = A + B ──
            const int grp = tid >> 3, j8 = tid & 7;
            for (int it0 = 0; it0 < T; it0 += TD_FIN_THREADS / 8) {
                const bool valid = it0 + grp < T;
                const int tau = valid ? it0 + grp : 0;
                const float2 ab = phat_lag_sum(s_S, j8, tau, LM_NFFT, [&](int m) { return s_lag[m]; });
                const float A = ab.x, B = ab.y;
                if (valid && j8 < 2) {
                    const float ny = s_S[LM_N].x, sgn = (tau & 1) ? -ny : ny;
                    const bool plus = j8 == 0;
                    if (plus || tau > 0) s_cc[plus ? ML + 1 + tau : ML + 1 - tau] = (2.f * (plus ? A - B : A + B) + sgn) * (1.f / LM_NFFT);
                }
            }
            __syncthreads();
            if (acc_out)
                for (int i = tid; i < W; i += TD_FIN_THREADS) acc_out[(e * P + p) * W + i] = s_cc[i];
            if (tid < 64) {
                // ── the first maximum over |tau| <= max_lag (entries 1 .. 2 max_lag + 1 of s_cc), ascending ──
                FirstMax fm{-INFINITY, INFINITY, 0x7fffffff};
                for (int i = 1 + tid; i <= 2 * ML + 1; i += 64) {
                    const float v = s_cc[i];
                    if (v > fm.best) { fm.best = v; fm.at = i; }
                    fm.low = fminf(fm.low, v);
                }
                fm = first_max_wave(fm);
                if (tid == 0) {
                    // digital silence: every lag is 0, the answer is lag 0 (and NaN samples, which compare with nothing, stay in range)
                    const int at = (fm.best == 0.f && fm.low == 0.f) || fm.at > 2 * ML + 1 ? ML + 1 : fm.at;
                    const double l = s_cc[at - 1], m = s_cc[at], rr = s_cc[at + 1];
                    const double den = l - 2.0 * m + rr;
                    double lag = (double)(at - ML - 1);
                    if (den < 0.0) lag += 0.5 * (l - rr) / den;
                    lag_out[e * P + p] = (float)lag;
                    strength_out[e * P + p] = (float)(m / (double)nf);
                }
            }
            __syncthreads();                                     // S and the lags may be overwritten by the next pair
        }
    }
}

// What both entries share once their recordings are checked: the argument checks, the upload of the recording table and the
// two launches per slice of the event table.  A ring's longest "recording" is its capacity: no located event has more than
// 1 + cap / hop frames.
template <bool RING>
int tdoa_run(const char* who, const RecSource& src, const EvTable& ev, const TdSettings& st, const TdOut& out, void* workspace,
             size_t workspace_bytes, void* stream, TdSliceHook hook, void* hook_ctx, const TdExtra* extra) {
    const int channels = src.C, P = channels * (channels - 1) / 2;
    const long E = ev.E;
    const size_t tab = src.tab + (extra ? extra->tab_bytes : 0);  // (the activity mask lies behind the table)
    SED_REQUIRE(ev.onset && ev.offset && ev.peak && out.lag && out.strength && out.frames && workspace, "%s: null pointer", who);
    SED_REQUIRE(ev.rec || src.R == 1, "%s: %d recordings need ev_rec", who, src.R);
    SED_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    const long own = tdoa_chunks_per_event(1 + (RING ? src.cap : src.longest) / ev.hop, ev.max_frames);
    const long cpe = own + (extra ? extra->chunks : 0);           // (... and an event's background chunks behind its own)
    SED_REQUIRE(cpe <= 0x7fffffffL, "%s: too many chunks per event", who);         // (gridDim.x and TdArgs.cpe; frames are < 2^31)
    const size_t per_event = (size_t)cpe * P * TD_ROW_BYTES;
    SED_REQUIRE(workspace_bytes >= tab + per_event, "%s: workspace of %zu bytes, at least %zu needed (one event)", who, workspace_bytes,
                tab + per_event);
    long slice = (long)((workspace_bytes - tab) / per_event);
    if (slice > E) slice = E;
    if (slice > 65535) slice = 65535;                            // gridDim.y; the events of a slice (n_ev below) therefore fit an int

    // every pair's accumulator beside two spectra buffers where that fits (C <= 4); else one buffer and as many pairs of
    // accumulators at a time as LDS holds beside the tables, the C spectra and the FFT scratch
    const int pipelined = tdoa_lds_bytes(channels, P, 2) <= TD_LDS_MAX;
    int batch = P;
    while (!pipelined && batch > 1 && tdoa_lds_bytes(channels, batch, 1) > TD_LDS_MAX) --batch;
    const size_t lds = tdoa_lds_bytes(channels, batch, pipelined ? 2 : 1);
    SED_REQUIRE(lds <= TD_LDS_MAX, "%s: %d spectra and the tables (%zu B) exceed the 160 KiB LDS", who, channels, lds);

    hipStream_t s = as_stream(stream);
    SED_TRY(rec_upload(who, src, workspace, s));
    if (extra && extra->pre) SED_TRY(extra->pre(extra->ctx, src, ev, workspace, s));
    const hipError_t err = hipFuncSetAttribute((const void*)tdoa_accum_k<RING>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TD_LDS_MAX);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    TdArgs ta = td_args(src, ev, workspace);
    ta.pairs_per_batch = batch; ta.max_lag = st.max_lag; ta.cpe = (int)cpe; ta.pipelined = pipelined;
    ta.lat = st.lat; ta.hist = st.hist;
    const uint32_t* tables = (const uint32_t*)st.tables;
    float2* part = (float2*)((char*)workspace + tab);
    for (long e0 = 0; e0 < E; e0 += slice) {
        ta.e0 = e0;
        ta.n_ev = (int)(E - e0 < slice ? E - e0 : slice);
        tdoa_accum_k<RING><<<dim3((unsigned)own, (unsigned)ta.n_ev), TD_THREADS, lds, s>>>(src.x, tables, part, st.pad_mode, ta);
        SED_LAUNCH_CHECK(RING ? "event_tdoa_ring (accumulate)" : "event_tdoa (accumulate)");
        const int blocks = ta.n_ev < 2048 ? ta.n_ev : 2048;
        tdoa_finish_k<<<blocks, TD_FIN_THREADS, 0, s>>>(tables, part, out.lag, out.strength, out.frames, out.acc, ta);
        SED_LAUNCH_CHECK(RING ? "event_tdoa_ring (finish)" : "event_tdoa (finish)");
        if (hook) {                                              // (doa.hip: the slice's partials are still in the workspace)
            const int rc = hook(hook_ctx, ta, part, s);
            if (rc != 0) return rc;
        }
    }
    return 0;
}

// ───────────────────────── a live feed's PCM ring ─────────────────────────
// Lane l keeps its last cap samples: sample i (counted from the start of the feed) at ring[l*cap + i % cap].  A round's new
// samples are at most cap per lane, so no entry is written twice and no thread reads what another writes.
struct RingRec { long src, count, abs; };

__global__ __launch_bounds__(256) void tdoa_ring_write_k(float* __restrict__ ring, long cap, const float* __restrict__ src,
                                                         const RingRec* __restrict__ recs) {
    const RingRec r = recs[blockIdx.y];
    float* lane = ring + (long)blockIdx.y * cap;
    const long p0 = r.abs % cap;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < r.count; i += (long)gridDim.x * 256) {
        const long p = p0 + i;                                   // (count <= cap: p < 2 cap)
        lane[p >= cap ? p - cap : p] = src[r.src + i];
    }
}

}  // namespace

// workspace: sample_off [R*C] and n_samples [R], then, for every event, chunks_per_event x P rows of 1026 float2
extern "C" size_t sed_event_tdoa_workspace_bytes(int R, int channels, long E, long max_n_samples, int hop, int max_frames) {
    if (R < 1 || channels < 2 || channels > TD_MAX_CH || E < 0 || max_n_samples < 1 || hop < 1 || max_frames < 1) return 0;
    const int P = channels * (channels - 1) / 2;
    const long cpe = tdoa_chunks_per_event(1 + max_n_samples / hop, max_frames);
    return rec_table_bytes(R, channels) + (size_t)E * cpe * P * TD_ROW_BYTES;
}

// the host side of sed_event_tdoa / sed_event_tdoa_ring (src.ring) and, with a hook, of their DOA siblings: each form keeps its
// own checks in its own order
int tdoa_entry(const char* who, RecSource src, const EvTable& ev, const TdSettings& st, const TdOut& out, void* workspace,
               size_t workspace_bytes, void* stream, TdSliceHook hook, void* hook_ctx, const TdExtra* extra) {
    SED_REQUIRE(src.C >= 2 && src.C <= TD_MAX_CH, "%s: 2 to %d channels, got %d", who, TD_MAX_CH, src.C);
    SED_REQUIRE(st.max_lag >= 1 && st.max_lag <= TD_MAX_LAG, "%s: max_lag must be in [1,%d], got %d", who, TD_MAX_LAG, st.max_lag);
    SED_REQUIRE(ev.max_frames >= 1, "%s: max_frames must be >= 1, got %d", who, ev.max_frames);
    SED_REQUIRE(ev.tf >= 1 && ev.hop >= 1 && src.R >= 1 && ev.E >= 0, "%s: bad sizes (time_factor=%d, hop=%d, R=%d, E=%ld)", who,
                ev.tf, ev.hop, src.R, ev.E);
    if (!src.ring) {
        SED_REQUIRE(st.pad_mode == 0 || st.pad_mode == 1, "%s: pad_mode must be 0 (constant) or 1 (reflect), got %d", who, st.pad_mode);
        SED_REQUIRE(src.x && src.host && st.tables && src.x_len > 0, "%s: null pointer", who);
    } else {
        SED_REQUIRE(st.lat >= 0 && st.hist >= 1, "%s: need lat_frames >= 0 and history_frames >= 1, got %d, %d", who, st.lat, st.hist);
        SED_REQUIRE(src.x && src.host && st.tables, "%s: null pointer", who);
        SED_TRY(rec_ring_check(who, src));
        SED_REQUIRE(((uintptr_t)src.x & 15) == 0, "%s: the rings must be 16-byte aligned", who);
    }
    SED_REQUIRE(st.tables_bytes % 16 == 0 && st.tables_bytes / 4 >= (size_t)TD_TAB_WORDS, "%s: table blob of %zu bytes is malformed", who,
                st.tables_bytes);
    SED_TRY(!src.ring ? rec_source_linear(who, src, ev.hop) : rec_source_ring(who, src, ev.hop));
    if (ev.E == 0) return 0;                                     // nothing to launch
    return !src.ring ? tdoa_run<false>(who, src, ev, st, out, workspace, workspace_bytes, stream, hook, hook_ctx, extra)
                     : tdoa_run<true>(who, src, ev, st, out, workspace, workspace_bytes, stream, hook, hook_ctx, extra);
}

extern "C" int sed_event_tdoa(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                              size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                              const int* ev_peak_frame, long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames,
                              float* lag_out, float* strength_out, int* frames_out, float* acc_out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return tdoa_entry("event_tdoa", {pcm, false, 0, pcm_len, R, channels, clips_host},
                             {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                             {tables, tables_bytes, pad_mode, max_lag, 0, 0}, {lag_out, strength_out, frames_out, acc_out}, workspace,
                             workspace_bytes, stream, nullptr, nullptr);
}

// ───────────────────────── live feeds ─────────────────────────
extern "C" size_t sed_stream_ring_write_workspace_bytes(int lanes) {
    return lanes < 1 || lanes > 65535 ? 0 : (size_t)lanes * sizeof(RingRec);
}

extern "C" int sed_stream_ring_write(float* ring, long ring_len, int lanes, long cap, const float* src, long src_len,
                                     const long* table_host, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(ring && table_host && workspace, "stream_ring_write: null pointer");
    const size_t need = sed_stream_ring_write_workspace_bytes(lanes);
    SED_REQUIRE(need > 0 && cap >= 4 && cap % 4 == 0 && ring_len >= 0 && cap <= ring_len / lanes && src_len >= 0,
                "stream_ring_write: bad sizes (lanes=%d in 1..65535, cap=%ld a multiple of 4, ring_len=%ld)", lanes, cap, ring_len);
    SED_REQUIRE(workspace_bytes >= need, "stream_ring_write: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(src || src_len == 0, "stream_ring_write: null buffer with a non-zero length");
    std::vector<RingRec> h(lanes);
    long longest = 0;
    for (int l = 0; l < lanes; ++l) {
        const RingRec r{table_host[3 * l], table_host[3 * l + 1], table_host[3 * l + 2]};
        SED_REQUIRE(r.count >= 0 && r.count <= cap, "stream_ring_write: lane %d: %ld new samples, the ring holds %ld", l, r.count, cap);
        SED_REQUIRE(r.count == 0 || (r.src >= 0 && r.src <= src_len && r.count <= src_len - r.src),
                    "stream_ring_write: lane %d: its samples [%ld, +%ld) leave the buffer of %ld", l, r.src, r.count, src_len);
        SED_REQUIRE(r.abs >= 0 && r.abs <= 0x7fffffffffffffffL - r.count, "stream_ring_write: lane %d: bad first sample index %ld", l, r.abs);
        h[l] = r;
        if (r.count > longest) longest = r.count;
    }
    if (longest == 0) return 0;
    hipStream_t st = as_stream(stream);
    const hipError_t err = hipMemcpyAsync(workspace, h.data(), need, hipMemcpyHostToDevice, st);
    if (err != hipSuccess) { sed_set_error("stream_ring_write: upload of the lane table: %s", hipGetErrorString(err)); return (int)err; }
    const long nb = (longest + 255) / 256;
    tdoa_ring_write_k<<<dim3((unsigned)(nb < 1024 ? nb : 1024), (unsigned)lanes), 256, 0, st>>>(ring, cap, src, (const RingRec*)workspace);
    SED_LAUNCH_CHECK("stream_ring_write");
    return 0;
}

// workspace: n [R], then, for every event, chunks_per_event x P rows of 1026 float2 (no located event has more than
// 1 + cap / hop frames: its first sample is still in the ring and its last frame's centre is a sample received)
extern "C" size_t sed_event_tdoa_ring_workspace_bytes(int R, int channels, long E, long cap, int hop, int max_frames) {
    if (R < 1 || channels < 2 || channels > TD_MAX_CH || E < 0 || cap < LM_NFFT || cap % 4 || hop < 1 || max_frames < 1) return 0;
    const int P = channels * (channels - 1) / 2;
    const long cpe = tdoa_chunks_per_event(1 + cap / hop, max_frames);
    return rec_ring_table_bytes(R) + (size_t)E * cpe * P * TD_ROW_BYTES;
}

extern "C" int sed_event_tdoa_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                   const void* tables, size_t tables_bytes, const int* ev_rec, const int* ev_onset,
                                   const int* ev_offset, const int* ev_peak_frame, long E, int time_factor, int hop, int max_lag,
                                   int max_frames, int lat_frames, int history_frames, float* lag_out, float* strength_out,
                                   int* frames_out, float* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
    return tdoa_entry("event_tdoa_ring", {ring, true, cap, ring_len, R, channels, n_host},
                           {ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0},
                           {tables, tables_bytes, 0, max_lag, lat_frames, history_frames}, {lag_out, strength_out, frames_out, acc_out},
                           workspace, workspace_bytes, stream, nullptr, nullptr);
}
