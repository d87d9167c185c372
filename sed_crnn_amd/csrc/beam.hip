// beam.hip — the audio of every located event with the array pointed at it: a steered delay-and-sum beam over the event table
// (DESIGN 5r): sed_event_beam_spans, sed_event_beamform and their ring forms.
//
// An event with dir >= 0 (sed_event_doa: a row of the direction grid) was located on the frames [f0, f0 + loc_frames) that
// tdoa_shared.h picks; its samples are [s0, s1) = [f0 hop, min((f0 + loc_frames) hop, n)).  With M[dir][c] the delay of channel
// c in 1/Q samples (the host's table), taps float32 [Q][2H] the fractional-delay filter (row p evaluates a channel at m + p/Q)
// and, per channel, q = -M[dir][c], i = floor(q / Q), p = q - Q i, output sample j of the event (n = s0 + j) is
//   a_c = sum_{k = 0}^{2H-1} taps[p][k] x_c[n + i + k - H + 1]        an fp32 fma chain from 0 in ascending k
//   y   = (((0 + a_0) + a_1) + ... + a_{C-1}) * float32(1 / C)
// with samples outside [0, n) of the recording read as 0.  Every value depends on the event's own samples and these tables
// alone: no atomic, no host read, no other event.
//
// Shape (gfx950).  beam_spans_k: one workgroup scans the event table 1024 events at a time (wave scans by shuffle, 16 wave totals
// in LDS, a running carry) and writes audio_len, audio_start (the exclusive prefix sum) and the total — integers, any order.
// beam_sum_k: one workgroup of 256 threads per (tile of 2048 outputs, event) on a 2-D grid; a workgroup whose tile starts
// beyond its event returns at once.  Per channel the tile's input segment — 2048 + 2H - 1 samples from s0 + t0 + i - H + 1 —
// is staged into LDS with 16-byte loads from the aligned address below it, shifted so that LDS entry j + k is what output j
// needs at tap k whatever the delay.  A tile whose C segments lie inside [0, n) (and inside what a ring still holds) — all but
// those at the ends of a recording — takes its C x 529 vectors as one list, every thread with 4 loads in flight before it writes
// the first to LDS: one load at a time left the launch waiting on memory latency (1.97 ms against 1.56 for the workload of
// tools/beam_bench.py, the two alternating on one MI355X).  A tile at an end reads every vector behind the bounds check, sample by sample where the vector leaves
// the range: the same values.  Every thread then owns 8 consecutive outputs: it slides a 16-sample register window over its 8 + 2H - 1
// LDS entries, 16-byte LDS reads, 8 taps x 8 outputs = 64 fma per 8 samples read; the tap row is uniform and comes through the
// scalar cache.  The outputs pass through LDS once more so that the stores to the packed buffer, whose start no event aligns,
// are consecutive over the workgroup.  RING = true addresses sample s of lane l at ring[l cap + s % cap] (sed_stream_ring_write);
// the aligned vectors never straddle the wrap (cap is a multiple of 4), so the wrapping tile takes the same loads: the same bits.
#include "common.h"
#include "tdoa_shared.h"
#include "beam_shared.h"

#define BM_THREADS 256
#define BM_PER 8                                  // consecutive outputs of a thread
#define BM_TILE (BM_THREADS * BM_PER)
#define BM_MAX_H 32
#define BM_SEG (BM_TILE + 2 * BM_MAX_H + 8)       // floats per channel row: the tile, the taps' reach and the window's read-ahead
#define BM_NV 532                                 // vectors per row at most ((2048 + 63 + 3 + 3) / 4 = 529), rounded up
#define BM_FLIGHT 4                               // 16-byte loads a thread issues before it writes the first to LDS
#define BM_SCAN 1024

namespace {

struct BmArgs {
    const int *ev_dir, *ev_loc;                  // [E] the direction row (-1: not extracted) and the frames it was located on
    int D;
    const int* delays;                           // [D][C] M
    int Q, lq, H;                                // lq = log2 Q
    const float* taps;                           // [Q][2H]
    const int* audio_len;                        // [E]
    const long* audio_start;                     // [E]
    float* audio;                                // [total]
    long total;
    float inv_c;
};

// (bm_event_span — [s0, s0 + len) of an event — and the host's checks and upload: beam_shared.h, shared with mvdr.hip; the source,
// the event table and the recording table: tdoa_shared.h)
__global__ __launch_bounds__(BM_SCAN) void beam_spans_k(TdArgs ta, const int* __restrict__ ev_dir, const int* __restrict__ ev_loc, int D,
                                                        long E, int* __restrict__ len_out, long* __restrict__ start_out,
                                                        long* __restrict__ total_out) {
    __shared__ long s_wave[BM_SCAN / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    long carry = 0;
    for (long base = 0; base < E; base += BM_SCAN) {
        const long e = base + tid;
        int rec, len = 0;
        long s0;
        if (e < E) {
            bm_event_span(ta, ev_dir, ev_loc, D, e, rec, s0, len);
            len_out[e] = len;
        }
        long v = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long t = __shfl_up(v, o, 64);
            if (lane >= o) v += t;
        }
        if (lane == 63) s_wave[w] = v;
        __syncthreads();
        long before = 0, all = 0;
#pragma unroll
        for (int i = 0; i < BM_SCAN / 64; ++i) {
            const long t = s_wave[i];
            if (i < w) before += t;
            all += t;
        }
        if (e < E) start_out[e] = carry + before + v - len;
        carry += all;
        __syncthreads();                                         // the wave totals may be overwritten by the next round
    }
    if (tid == 0) *total_out = carry;
}

template <bool RING>
__global__ __launch_bounds__(BM_THREADS) void beam_sum_k(const float* __restrict__ x, TdArgs ta, BmArgs ba) {
    extern __shared__ __attribute__((aligned(16))) float lds[];  // [C][BM_SEG]
    const long e = ta.e0 + blockIdx.y;
    int rec, len;
    long s0;
    bm_event_span(ta, ba.ev_dir, ba.ev_loc, ba.D, e, rec, s0, len);
    const long t0 = (long)blockIdx.x * BM_TILE;
    if (t0 >= len) return;                                       // (block-uniform)
    const long start = ba.audio_start[e];
    // a span table that was not made from this event table: nothing is written
    if (ba.audio_len[e] != len || start < 0 || start > ba.total - len) return;
    const int tid = threadIdx.x, C = ta.C, Q = ba.Q, H = ba.H, nt = 2 * H;
    const int cnt = len - t0 < BM_TILE ? (int)(len - t0) : BM_TILE;      // outputs of this tile
    const int need = cnt + nt - 1;                                        // input samples per channel
    const long n = ta.n_samples[rec];
    const long lo = RING ? (n > ta.cap ? n - ta.cap : 0) : 0;            // the samples [lo, n) can be read
    const int* mrow = ba.delays + (long)ba.ev_dir[e] * C;

    // ── per channel: where its row starts.  Row c, entry j = x_c[s0 + t0 + i_c - H + 1 + j], 0 <= j < need ──
    __shared__ long s_a0[TD_MAX_CH];             // the sample of vector 0, entry 0: at or below the row's first, on a 16-byte boundary
    __shared__ long s_x0[TD_MAX_CH];             // where the channel (RING: its lane) starts in x
    __shared__ long s_p0[TD_MAX_CH];             // RING: a0 % cap (a0 >= 0)
    __shared__ int s_sh[TD_MAX_CH];              // entries of vector 0 that lie before the row
    if (tid < C) {
        const int q = -mrow[tid];
        const long first = s0 + t0 + (q >> ba.lq) - H + 1;               // (an arithmetic shift: the floor of q / Q)
        const long x0 = RING ? ((long)rec * C + tid) * ta.cap : ta.sample_off[(long)rec * C + tid];
        const int sh = (int)((RING ? first : x0 + first) & 3);           // (two's complement: a floor as well)
        s_x0[tid] = x0; s_sh[tid] = sh; s_a0[tid] = first - sh;
        s_p0[tid] = RING && first - sh >= 0 ? (first - sh) % ta.cap : 0;
    }
    __syncthreads();
    bool inside = true;                                                   // every vector of every row is samples that can be read
    for (int c = 0; c < C; ++c) inside = inside && s_a0[c] >= lo && s_a0[c] + 4 * (long)((need + s_sh[c] + 3) >> 2) <= n;
    if (inside) {
        // ── the tile's C x nvec vectors as one list, 4 loads in flight per thread before the first is written ──
        const int items = C * BM_NV;
        for (int base = tid; base < items; base += BM_FLIGHT * BM_THREADS) {
            f32x4 val[BM_FLIGHT];
            int row0[BM_FLIGHT], at[BM_FLIGHT];
#pragma unroll
            for (int u = 0; u < BM_FLIGHT; ++u) {
                const int idx = base + u * BM_THREADS;
                const int c = idx < items ? idx / BM_NV : 0;
                const int v = idx - c * BM_NV, sh = s_sh[c];
                const bool ok = idx < items && v < ((need + sh + 3) >> 2);
                const int vv = ok ? v : 0;                                // (a slot without a vector loads vector 0 of row 0 and drops it)
                long s = (RING ? s_p0[c] : s_a0[c]) + 4 * vv;
                if (RING) {                                               // (p0 + 4 v < 3 cap: cap >= 2048)
                    s -= s >= ta.cap ? ta.cap : 0;
                    s -= s >= ta.cap ? ta.cap : 0;
                }
                val[u] = *reinterpret_cast<const f32x4*>(x + s_x0[c] + s);
                row0[u] = c * BM_SEG;
                at[u] = ok ? 4 * v - sh : -8;
            }
#pragma unroll
            for (int u = 0; u < BM_FLIGHT; ++u) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (at[u] + i >= 0) lds[row0[u] + at[u] + i] = val[u][i];     // (at most need + 5: inside the row)
            }
        }
    } else {
        // ── a tile at an end of its recording (or of what the ring holds): every vector behind the bounds check ──
        for (int c = 0; c < C; ++c) {
            const float* xc = x + s_x0[c];
            const long a0 = s_a0[c];
            const int sh = s_sh[c];
            float* row = lds + c * BM_SEG;
            const int nvec = (need + sh + 3) >> 2;
            for (int v = tid; v < nvec; v += BM_THREADS) {
                const long s = a0 + 4 * (long)v;
                float val[4];
                if (s >= lo && s + 3 < n) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(xc + (RING ? s % ta.cap : s));
                    val[0] = t[0]; val[1] = t[1]; val[2] = t[2]; val[3] = t[3];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const long si = s + i;
                        val[i] = si >= lo && si < n ? xc[RING ? si % ta.cap : si] : 0.f;
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int j = 4 * v - sh + i;                         // (at most need + 5: inside the row)
                    if (j >= 0) row[j] = val[i];
                }
            }
        }
    }
    __syncthreads();

    // ── 8 outputs per thread from a sliding register window ──
    float y[BM_PER];
#pragma unroll
    for (int o = 0; o < BM_PER; ++o) y[o] = 0.f;
    if (tid * BM_PER < cnt) {
        for (int c = 0; c < C; ++c) {
            const float* tp = ba.taps + (long)((-mrow[c]) & (Q - 1)) * nt;        // row p = q - Q floor(q / Q), q = -M: Q is a power of two
            const f32x4* win = reinterpret_cast<const f32x4*>(lds + c * BM_SEG + tid * BM_PER);
            float acc[BM_PER], r[2 * BM_PER];
#pragma unroll
            for (int o = 0; o < BM_PER; ++o) acc[o] = 0.f;
            {
                const f32x4 u0 = win[0], u1 = win[1];
#pragma unroll
                for (int i = 0; i < 4; ++i) { r[i] = u0[i]; r[4 + i] = u1[i]; }
            }
            int kb = 0;
            for (; kb + 8 <= nt; kb += 8) {
                const f32x4 u0 = win[kb / 4 + 2], u1 = win[kb / 4 + 3];
#pragma unroll
                for (int i = 0; i < 4; ++i) { r[8 + i] = u0[i]; r[12 + i] = u1[i]; }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const float t = tp[kb + kk];
#pragma unroll
                    for (int o = 0; o < BM_PER; ++o) acc[o] = fmaf(t, r[o + kk], acc[o]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) r[i] = r[8 + i];
            }
            if (kb < nt) {                                                // 2, 4 or 6 taps are left (uniform)
                const f32x4 u0 = win[kb / 4 + 2], u1 = win[kb / 4 + 3];
#pragma unroll
                for (int i = 0; i < 4; ++i) { r[8 + i] = u0[i]; r[12 + i] = u1[i]; }
#pragma unroll
                for (int kk = 0; kk < 6; ++kk) {
                    if (kb + kk < nt) {
                        const float t = tp[kb + kk];
#pragma unroll
                        for (int o = 0; o < BM_PER; ++o) acc[o] = fmaf(t, r[o + kk], acc[o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < BM_PER; ++o) y[o] = y[o] + acc[o];
        }
    }
    __syncthreads();                                                      // every window has been read: row 0 takes the outputs
    {
        f32x4* out = reinterpret_cast<f32x4*>(lds + tid * BM_PER);
        out[0] = f32x4{y[0] * ba.inv_c, y[1] * ba.inv_c, y[2] * ba.inv_c, y[3] * ba.inv_c};
        out[1] = f32x4{y[4] * ba.inv_c, y[5] * ba.inv_c, y[6] * ba.inv_c, y[7] * ba.inv_c};
    }
    __syncthreads();
    float* dst = ba.audio + start + t0;
    for (int j = tid; j < cnt; j += BM_THREADS) dst[j] = lds[j];
}

int beam_spans(const char* who, const RecSource& src, const EvTable& ev, int* len_out, long* start_out, long* total_out,
               void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(total_out && (ev.E == 0 || (len_out && start_out)), "%s: null pointer (an output)", who);
    hipStream_t s = as_stream(stream);
    SED_TRY(beam_upload(who, src, workspace, workspace_bytes, s));
    const TdArgs ta = td_args(src, ev, workspace);
    beam_spans_k<<<1, BM_SCAN, 0, s>>>(ta, ev.dir, ev.loc, ev.D, ev.E, len_out, start_out, total_out);      // (E = 0: the total alone)
    SED_LAUNCH_CHECK(who);
    return 0;
}

// the delays [D][C] in 1/Q samples and the fractional-delay filter [Q][2H] (the host's tables)
struct BmTables { const int* delays; int Q, H; const float* taps; };

template <bool RING>
int beam_run(const char* who, const RecSource& src, const EvTable& ev, const BmTables& bt, const BeamOut& out, void* workspace,
             size_t workspace_bytes, void* stream) {
    const int Q = bt.Q, H = bt.H;
    const long E = ev.E;
    SED_REQUIRE(Q == 1 || Q == 2 || Q == 4 || Q == 8 || Q == 16 || Q == 32 || Q == 64, "%s: oversample must be a power of two up to 64, got %d",
                who, Q);
    SED_REQUIRE(H >= 1 && H <= BM_MAX_H, "%s: half_width must be in [1,%d], got %d", who, BM_MAX_H, H);
    SED_REQUIRE(out.total >= 0, "%s: a total of %ld samples", who, out.total);
    SED_REQUIRE(E == 0 || (bt.delays && bt.taps && out.audio_len && out.audio_start), "%s: null pointer (delays, taps, audio_len or audio_start)",
                who);
    SED_REQUIRE(out.audio || out.total == 0, "%s: null output buffer for %ld samples", who, out.total);
    SED_REQUIRE(((uintptr_t)src.x & 15) == 0, "%s: the samples must be 16-byte aligned", who);
    if (E == 0 || out.total == 0) return 0;                      // nothing to launch
    hipStream_t s = as_stream(stream);
    SED_TRY(beam_upload(who, src, workspace, workspace_bytes, s));
    const size_t lds = (size_t)src.C * BM_SEG * sizeof(float);
    const hipError_t err = hipFuncSetAttribute((const void*)beam_sum_k<RING>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(TD_MAX_CH * BM_SEG * sizeof(float)));
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    TdArgs ta = td_args(src, ev, workspace);
    int lq = 0;
    while ((1 << lq) < Q) ++lq;
    const BmArgs ba{ev.dir, ev.loc, ev.D, bt.delays, Q, lq, H, bt.taps, out.audio_len, out.audio_start, out.audio, out.total,
                    (float)(1.0 / src.C)};
    long most = (long)ev.max_frames * ev.hop;                    // no event has more samples than this, or than its recording
    if (most > src.longest) most = src.longest;
    if (most < 1) return 0;
    const unsigned tiles = (unsigned)((most + BM_TILE - 1) / BM_TILE);
    for (long e0 = 0; e0 < E; e0 += 65535) {                     // gridDim.y
        ta.e0 = e0;
        ta.n_ev = (int)(E - e0 < 65535 ? E - e0 : 65535);
        beam_sum_k<RING><<<dim3(tiles, (unsigned)ta.n_ev), BM_THREADS, lds, s>>>(src.x, ta, ba);
        SED_LAUNCH_CHECK(who);
    }
    return 0;
}

// an entry: the events and the recordings checked, then the launches
template <bool RING>
int beam_spans_entry(const char* who, RecSource src, const EvTable& ev, int* len_out, long* start_out, long* total_out, void* workspace,
                     size_t workspace_bytes, void* stream) {
    SED_TRY((beam_source<RING, false>(who, src, ev)));
    return beam_spans(who, src, ev, len_out, start_out, total_out, workspace, workspace_bytes, stream);
}

template <bool RING>
int beam_entry(const char* who, RecSource src, const EvTable& ev, const BmTables& bt, const BeamOut& out, void* workspace,
               size_t workspace_bytes, void* stream) {
    SED_TRY(beam_source<RING>(who, src, ev));
    return beam_run<RING>(who, src, ev, bt, out, workspace, workspace_bytes, stream);
}

}  // namespace

extern "C" size_t sed_event_beam_workspace_bytes(int R, int channels) {
    return R < 1 || channels < 2 || channels > TD_MAX_CH ? 0 : rec_table_bytes(R, channels);
}

extern "C" size_t sed_event_beam_ring_workspace_bytes(int R) { return R < 1 ? 0 : rec_ring_table_bytes(R); }

extern "C" int sed_event_beam_spans(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_onset,
                                    const int* ev_offset, const int* ev_peak_frame, const int* ev_dir, const int* ev_loc_frames, long E,
                                    int time_factor, int hop, int max_frames, int D, int* len_out, long* start_out, long* total_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    return beam_spans_entry<false>("event_beam_spans", {nullptr, false, 0, pcm_len, R, channels, clips_host},
                                   {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                                   len_out, start_out, total_out, workspace, workspace_bytes, stream);
}

extern "C" int sed_event_beam_spans_ring(const long* n_host, int R, int channels, const int* ev_rec, const int* ev_onset,
                                         const int* ev_offset, const int* ev_peak_frame, const int* ev_dir, const int* ev_loc_frames,
                                         long E, int time_factor, int hop, int max_frames, int D, int* len_out, long* start_out,
                                         long* total_out, void* workspace, size_t workspace_bytes, void* stream) {
    return beam_spans_entry<true>("event_beam_spans_ring", {nullptr, true, 0, 0, R, channels, n_host},
                                  {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                                  len_out, start_out, total_out, workspace, workspace_bytes, stream);
}

extern "C" int sed_event_beamform(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec,
                                  const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, const int* ev_dir,
                                  const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames, const int* delays, int D,
                                  int Q, int H, const float* taps, const int* audio_len, const long* audio_start, float* audio,
                                  long audio_total, void* workspace, size_t workspace_bytes, void* stream) {
    return beam_entry<false>("event_beamform", {pcm, false, 0, pcm_len, R, channels, clips_host},
                             {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                             {delays, Q, H, taps}, {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream);
}

extern "C" int sed_event_beamform_ring(const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                                       const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                                       const int* ev_dir, const int* ev_loc_frames, long E, int time_factor, int hop, int max_frames,
                                       const int* delays, int D, int Q, int H, const float* taps, const int* audio_len,
                                       const long* audio_start, float* audio, long audio_total, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return beam_entry<true>("event_beamform_ring", {ring, true, cap, ring_len, R, channels, n_host},
                            {ev_rec, ev_onset, ev_offset, ev_peak_frame, ev_dir, ev_loc_frames, E, time_factor, hop, max_frames, D},
                            {delays, Q, H, taps}, {audio_len, audio_start, audio, audio_total}, workspace, workspace_bytes, stream);
}
