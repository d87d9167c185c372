// tdoa_shared.h — what the entries over an event table share: per-event TDOA (tdoa.hip), per-event direction of
// arrival (doa.hip) and, through beam_shared.h, the two beams (beam.hip, mvdr.hip).
// Device code: the kernel arguments and the rule that picks the frames an event is located on, so that every file locates an
// event on the SAME frames.
// Host code, each written once: RecSource, where the samples are (planar PCM or the rings of live feeds) with the recording
// table that goes to the head of the workspace, its checks, size and upload; EvTable, the event columns and the frame grid; and
// td_args, which makes the kernel arguments from the two.  Then the TDOA family's own: the workspace is the recording table
// followed by chunks_per_event x P rows of 1026 float2 per event, and tdoa_entry, behind sed_event_tdoa / sed_event_tdoa_ring,
// checks the arguments, uploads the table and walks the event table in slices.  doa.hip calls it with a hook that is
// given every slice after its accumulate and finish launches, while the slice's chunk partials are still in the workspace: the
// TDOA outputs of a DOA call are therefore the bits of the TDOA call, and the steering reads the cross spectra the lags were
// made from.
#pragma once
#include <vector>
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

// ───────────────────────── host only: where the samples are, and the event table ─────────────────────────
// An entry fills in the first seven fields from its arguments; rec_source_linear / rec_source_ring check them and make the rest.
struct RecSource {
    const float* x;             // planar PCM, or the rings of live feeds (null: a spans call, which reads no samples)
    bool ring;
    long cap;                   // ring: the samples of one ring
    long x_len;                 // floats at x
    int R, C;                   // recordings (feeds) and their channels
    const long* host;           // the caller's table: (offset, samples) per recording and channel; ring: samples received per feed
    std::vector<long> h;        // the recording table as the device gets it: sample_off [R*C] then n_samples [R]; ring: n_samples [R]
    size_t tab;                 // its bytes at the head of the workspace, rounded to 16
    long longest;               // the samples of the longest recording
};

struct EvTable {
    const int *rec, *onset, *offset, *peak;      // [E] (rec may be null: one recording)
    const int *dir, *loc;                        // [E] a located event's direction row and frames (null for TDOA and DOA)
    long E;
    int tf, hop, max_frames, D;
};

inline size_t rec_table_bytes(int R, int C) { return (((size_t)R * C + R) * sizeof(long) + 15) & ~(size_t)15; }
inline size_t rec_ring_table_bytes(int R) { return ((size_t)R * sizeof(long) + 15) & ~(size_t)15; }

// the recordings of a linear call, checked on the host before anything is enqueued: bounds and equal channel lengths
inline int rec_source_linear(const char* who, RecSource& src, int hop) {
    const long pcm_len = src.x_len;
    SED_REQUIRE(src.host && pcm_len > 0, "%s: null pointer (the clip table) or an empty buffer", who);
    const int R = src.R, channels = src.C;
    src.h.assign((size_t)R * channels + R, 0);
    long *soff = src.h.data(), *slen = soff + (size_t)R * channels;
    src.longest = 0;
    for (int r = 0; r < R; ++r) {
        const long n0 = src.host[2 * ((long)r * channels) + 1];
        for (int ch = 0; ch < channels; ++ch) {
            const long c = (long)r * channels + ch, o = src.host[2 * c], n = src.host[2 * c + 1];
            SED_REQUIRE(o >= 0 && n >= 1 && o <= pcm_len && n <= pcm_len - o,
                        "%s: recording %d, channel %d (offset %ld, %ld samples) is not inside the PCM buffer of %ld samples", who, r, ch,
                        o, n, pcm_len);
            SED_REQUIRE(n == n0, "%s: recording %d: channel %d has %ld samples, channel 0 has %ld (the channels of a recording "
                        "must have equal length)", who, r, ch, n, n0);
            soff[c] = o;
        }
        slen[r] = n0;
        SED_REQUIRE(1 + n0 / hop <= 0x7fffffffL, "%s: recording %d has more than 2^31 - 1 feature frames", who, r);
        if (n0 > src.longest) src.longest = n0;
    }
    src.tab = rec_table_bytes(R, channels);
    return 0;
}

// the rings of a ring call that reads samples
inline int rec_ring_check(const char* who, const RecSource& src) {
    SED_REQUIRE(src.x, "%s: null pointer (the rings)", who);
    SED_REQUIRE(src.cap >= LM_NFFT && src.cap % 4 == 0, "%s: a ring holds a multiple of 4 samples and at least one frame of %d, got "
                "cap=%ld", who, LM_NFFT, src.cap);
    SED_REQUIRE(src.x_len >= 0 && src.cap <= src.x_len / ((long)src.R * src.C), "%s: %d feeds of %d rings of %ld samples leave "
                "the buffer of %ld", who, src.R, src.C, src.cap, src.x_len);
    return 0;
}

// the recordings of a ring call (live feeds): the samples every feed has received
inline int rec_source_ring(const char* who, RecSource& src, int hop) {
    SED_REQUIRE(src.host, "%s: null pointer (the sample counts)", who);
    src.h.assign((size_t)src.R, 0);
    src.longest = 0;
    for (int r = 0; r < src.R; ++r) {
        const long n = src.h[r] = src.host[r];
        SED_REQUIRE(n >= 0 && 1 + n / hop <= 0x7fffffffL, "%s: feed %d: %ld samples received (negative, or more than "
                    "2^31 - 1 feature frames)", who, r, n);
        if (n > src.longest) src.longest = n;
    }
    src.tab = rec_ring_table_bytes(src.R);
    return 0;
}

// the table to the head of the workspace, which the caller has checked
inline int rec_upload(const char* who, const RecSource& src, void* workspace, hipStream_t s) {
    const hipError_t err = hipMemcpyAsync(workspace, src.h.data(), src.h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) { sed_set_error("%s: upload of the recording table: %s", who, hipGetErrorString(err)); return (int)err; }
    return 0;
}

// the kernel arguments every entry derives from its source and events; the rest (TDOA: the lags, the chunk layout, the stream's
// rule; every entry: the slice) is the runner's and stays zero where its kernels do not read it
inline TdArgs td_args(const RecSource& src, const EvTable& ev, const void* workspace) {
    const long* dl = (const long*)workspace;
    TdArgs ta{};
    ta.sample_off = src.ring ? nullptr : dl;
    ta.n_samples = src.ring ? dl : dl + (size_t)src.R * src.C;
    ta.ev_rec = ev.rec; ta.ev_onset = ev.onset; ta.ev_offset = ev.offset; ta.ev_peak = ev.peak;
    ta.R = src.R; ta.C = src.C; ta.P = src.C * (src.C - 1) / 2;
    ta.tf = ev.tf; ta.hop = ev.hop; ta.max_frames = ev.max_frames;
    ta.cap = src.ring ? src.cap : 0;
    return ta;
}

// what a TDOA call adds to its source and events (pad_mode: linear; lat, hist: ring), and its outputs
struct TdSettings { const void* tables; size_t tables_bytes; int pad_mode, max_lag, lat, hist; };
struct TdOut { float *lag, *strength; int* frames; float* acc; };

// What an entry may add to the run: `tab_bytes` of its own between the recording table and the partials (a multiple
// of 16), `chunks` more chunk slots behind every event's own (TdArgs.cpe counts both; the accumulate launch fills the own ones),
// and a step `pre` that is run once, on the same stream, after the table's upload and before the first slice.
struct TdExtra {
    size_t tab_bytes;
    int chunks;
    int (*pre)(void* ctx, const RecSource& src, const EvTable& ev, void* workspace, hipStream_t stream);
    void* ctx;
};

// sed_event_tdoa / sed_event_tdoa_ring (src.ring) with the entry's name for the messages, an optional hook and extra (tdoa.hip)
int tdoa_entry(const char* who, RecSource src, const EvTable& ev, const TdSettings& st, const TdOut& out, void* workspace,
               size_t workspace_bytes, void* stream, TdSliceHook hook, void* hook_ctx, const TdExtra* extra = nullptr);
