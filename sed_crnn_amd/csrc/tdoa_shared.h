// tdoa_shared.h — what per-event TDOA (tdoa.hip) and per-event direction of arrival (doa.hip) share.
// Device code: the kernel arguments and the rule that picks the frames an event is located on, so that both files locate an
// event on the SAME frames.  Host code: the layout of the workspace (the recording table, then chunks_per_event x P rows of
// 1026 float2 per event) and the two runners behind sed_event_tdoa / sed_event_tdoa_ring, which check the arguments, upload
// the table and walk the event table in slices.  doa.hip calls the same runners with a hook that is given every slice after
// its accumulate and finish launches, while the slice's chunk partials are still in the workspace: the TDOA outputs of a DOA
// call are therefore the bits of the TDOA call, and the steering reads the cross spectra the lags were made from.
#pragma once
#include "common.h"
#include "fft2048.h"
#include "phat_shared.h"

#define TD_CHUNK 32                               // frames per workgroup of the accumulate launch
#define TD_MAX_CH 8
#define TD_MAX_LAG 127
#define TD_ROW_BYTES ((size_t)PHAT_SPEC * sizeof(float2))

struct TdArgs {
    const long* sample_off;     // [R*C] first sample of every planar channel
    const long* n_samples;      // [R]   samples per channel
    const int *ev_rec, *ev_onset, *ev_offset, *ev_peak;          // [E] (ev_rec may be null: one recording)
    int R, C, P, pairs_per_batch;
    int tf, hop, max_frames, max_lag;
    int cpe;                    // chunk slots per event in the workspace
    int pipelined;              // two spectra buffers: the FFT of frame f+1 runs beside the whitening of frame f
    long e0;                    // first event of the slice
    int n_ev;                   // events of the slice
    long cap;                   // > 0: recording r is a live feed, its channel ch the ring of cap samples at (r*C + ch)*cap
    int lat, hist;              // ... and the stream's latency and history, in feature frames
};

// The frames [f0, f0 + nf) an event is located on; nf = 0: the event names no recording or lies beyond its end (nothing is read).
__device__ __forceinline__ void td_linear_range(const TdArgs& a, long e, int& rec, long& f0, int& nf) {
    rec = a.ev_rec ? a.ev_rec[e] : 0;
    f0 = 0; nf = 0;
    if (rec < 0 || rec >= a.R) return;
    const long n_feat = 1 + a.n_samples[rec] / a.hop;
    const long on = a.ev_onset[e], off = a.ev_offset[e];
    const long lo = on * a.tf;
    long hi = off * a.tf;
    if (hi > n_feat) hi = n_feat;
    if (on < 0 || lo >= n_feat) return;
    if (hi <= lo) { f0 = lo; nf = 1; return; }
    if (hi - lo <= a.max_frames) { f0 = lo; nf = (int)(hi - lo); return; }
    long c = (long)a.ev_peak[e] * a.tf + a.tf / 2 - a.max_frames / 2;
    if (c < lo) c = lo;
    if (c > hi - a.max_frames) c = hi - a.max_frames;
    f0 = c; nf = a.max_frames;
}

// ... of a live feed (a.cap > 0, n_samples = the samples received so far): the same range, and no frames either where the
// stream's rule b*tf + lat - f0 <= history does not hold or where the first sample read is no longer in the ring
__device__ __forceinline__ void td_event_range(const TdArgs& a, long e, int& rec, long& f0, int& nf) {
    td_linear_range(a, e, rec, f0, nf);
    if (a.cap <= 0 || nf == 0) return;
    const long first = f0 * a.hop - LM_NFFT / 2;
    if ((long)a.ev_offset[e] * a.tf + a.lat - f0 > a.hist || (first > 0 ? first : 0) < a.n_samples[rec] - a.cap) { f0 = 0; nf = 0; }
}

// Given every slice of the event table after its two launches, on the same stream: `part` holds the slice's chunk partials,
// event el of the slice (ta.e0 + el of the table) at part + el * ta.cpe * ta.P * PHAT_SPEC, chunk c / pair p at row c * P + p.
// A non-zero return ends the call with that code.
typedef int (*TdSliceHook)(void* ctx, const TdArgs& ta, const float2* part, hipStream_t stream);

// sed_event_tdoa / sed_event_tdoa_ring with the entry's name for the messages and an optional hook (tdoa.hip)
int tdoa_linear_entry(const char* who, const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                      size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak_frame,
                      long E, int time_factor, int hop, int pad_mode, int max_lag, int max_frames, float* lag_out, float* strength_out,
                      int* frames_out, float* acc_out, void* workspace, size_t workspace_bytes, void* stream, TdSliceHook hook,
                      void* hook_ctx);
int tdoa_ring_entry(const char* who, const float* ring, long ring_len, long cap, const long* n_host, int R, int channels,
                    const void* tables, size_t tables_bytes, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                    const int* ev_peak_frame, long E, int time_factor, int hop, int max_lag, int max_frames, int lat_frames,
                    int history_frames, float* lag_out, float* strength_out, int* frames_out, float* acc_out, void* workspace,
                    size_t workspace_bytes, void* stream, TdSliceHook hook, void* hook_ctx);
