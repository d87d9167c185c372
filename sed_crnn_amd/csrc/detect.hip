// detect.hip — whole-recording event detection (sed_crnn_amd/detect.py): the per-window outputs of the eval
// forward stitched into one probability track, and that track turned into (class, onset, offset, peak) events.
//
// Frame arithmetic (output frames, tf input frames each): window w covers [start(w), start(w) + win_out) with
// start(w) = min(w * hop_out, last_start_out) — the regular grid 0, hop, 2 hop, ... plus, where the last regular window stops
// short of the end, one extra window aligned to the end (last_start_out + win_out == n_out).  The host planner builds that grid.
//
// The two decoding entries come twice: with one decoder setting for all classes (sed_detect_events, sed_detect_events_batch) and
// with one row per class (…_classwise).  The class-wise ones launch their own bit-track and walk kernels around the
// same device functions and share the peak, offset and scan kernels; the scalar ones launch what they always launched.
#include <algorithm>
#include <vector>
#include "common.h"
#include "detect_shared.h"

// ───────────────────────── stitch: sigmoid, then mean / max over the covering windows ─────────────────────────
// One thread per (output frame, class): stitch_one of detect_shared.h (shared with the streaming step of stream.hip).
__global__ __launch_bounds__(256) void detect_stitch_k(const float* __restrict__ logits, int n_win, int win_out, int K,
                                                       int hop_out, int last_start, int n_out, int combine, int trim,
                                                       float* __restrict__ probs) {
    const long total = (long)n_out * K;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i / K), k = (int)(i - (long)j * K);
        probs[i] = stitch_one(LinearLogits{logits, win_out, K}, n_win, win_out, hop_out, last_start, n_out, combine, trim, j, k);
    }
}

// the grid of one recording of a batch (sed_detect_stitch_batch): its logits start logit_off floats into the packed buffer
struct DetRec { long logit_off; int n_win, win_out, hop_out, last_start, n_out, pad; };

// One thread per (packed output frame, class): its recording by binary search over the output offsets, then exactly the
// arithmetic of detect_stitch_k with that recording's grid (so a recording's track equals sed_detect_stitch of its logits)
__global__ __launch_bounds__(256) void detect_stitch_batch_k(const float* __restrict__ logits, const DetRec* __restrict__ recs,
                                                             const int* __restrict__ out_off, int R, long total_out, int K,
                                                             int combine, int trim, float* __restrict__ probs) {
    const long total = total_out * K;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / K;
        const int k = (int)(i - row * K);
        const int r = find_seg(out_off, R, row);
        const DetRec d = recs[r];
        probs[i] = stitch_one(LinearLogits{logits + d.logit_off, d.win_out, K}, d.n_win, d.win_out, d.hop_out, d.last_start, d.n_out,
                              combine, trim, (int)(row - out_off[r]), k);
    }
}

extern "C" int sed_detect_stitch(const float* logits, long n_win, int win_out, int K, int hop_out, long last_start_out,
                                 long n_out, int combine, int trim, float* probs, void* stream) {
    SED_REQUIRE(logits && probs, "detect_stitch: null pointer");
    SED_REQUIRE(n_win >= 1 && win_out >= 1 && K >= 1 && hop_out >= 1 && last_start_out >= 0 && n_out >= 1 &&
                    n_out <= 0x7fffffffL && n_win <= 0x7fffffffL && (long)n_out * K <= 0x7fffffffL,
                "detect_stitch: bad sizes (n_win=%ld, win_out=%d, K=%d, hop_out=%d, n_out=%ld)", n_win, win_out, K, hop_out, n_out);
    SED_REQUIRE(combine == 0 || combine == 1, "detect_stitch: combine must be 0 (mean) or 1 (max), got %d", combine);
    SED_TRY(detect_check_grid("detect_stitch", -1, n_win, win_out, hop_out, last_start_out, n_out, trim));
    const long total = n_out * K;
    long nb = (total + 255) / 256;
    detect_stitch_k<<<(unsigned)(nb < 8192 ? nb : 8192), 256, 0, as_stream(stream)>>>(
        logits, (int)n_win, win_out, K, hop_out, (int)last_start_out, (int)n_out, combine, trim, probs);
    SED_LAUNCH_CHECK("detect_stitch");
    return 0;
}

// ───────────────────────── events ─────────────────────────
// Phase 1 (all frames in parallel): median filter (a selection: exact), then two bit tracks per class packed by __ballot —
// on = p' > lo and high = p' > hi — as 64-bit words [K][n_words], n_words = n_out/64 + 1 (the extra word holds the fall edge
// of a run that reaches the end).  Phase 2 (one wave per class walking 64-word chunks): edges from the words, the number of
// high bits before every edge from a wave scan of popcounts, so a run [a, b) is kept iff H(b) - H(a) > 0; lane 0 then walks the
// chunk's edge list with the carried state (open run, pending event) to merge and drop.  Run once to count, a one-thread scan
// turns the counts into per-class offsets, run again to write.  Phase 3: peak / first arg-max of the unfiltered track.
template <int M>
__global__ __launch_bounds__(256) void detect_bits_k(const float* __restrict__ probs, int n_out, int K, long n_words, float lo,
                                                     float hi, unsigned long long* __restrict__ on_bits,
                                                     unsigned long long* __restrict__ hi_bits) {
    const int k = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    bool on = false, high = false;
    if (j < n_out) {
        const float p = median_nearest<M>(LinearRows{probs, K}, (int)j, k, n_out - 1);
        on = p > lo;
        high = p > hi;
    }
    const unsigned long long bo = __ballot(on), bh = __ballot(high);      // wave64: bit l = frame (j - lane + l)
    const long w = j >> 6;
    if ((threadIdx.x & 63) == 0 && w < n_words) {
        on_bits[(size_t)k * n_words + w] = bo;
        hi_bits[(size_t)k * n_words + w] = bh;
    }
}

// The class-wise form (sed_detect_events_classwise): grid y walks the classes of one median width, each compared with its own lo, hi
template <int M>
__global__ __launch_bounds__(256) void detect_bits_cw_k(const float* __restrict__ probs, int n_out, int K, long n_words, ClassList list,
                                                        ClassTable tab, unsigned long long* __restrict__ on_bits,
                                                        unsigned long long* __restrict__ hi_bits) {
    const int k = list.k[blockIdx.y];
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    bool on = false, high = false;
    if (j < n_out) {
        const float p = median_nearest<M>(LinearRows{probs, K}, (int)j, k, n_out - 1);
        on = p > tab.c[k].lo;
        high = p > tab.c[k].hi;
    }
    const unsigned long long bo = __ballot(on), bh = __ballot(high);
    const long w = j >> 6;
    if ((threadIdx.x & 63) == 0 && w < n_words) {
        on_bits[(size_t)k * n_words + w] = bo;
        hi_bits[(size_t)k * n_words + w] = bh;
    }
}

// Batched (SEG, sed_detect_events_batch): one wave per (recording r, class k), workgroup r*K + k; recording r's bit tracks
// are [K][n_words_r] at word K*word_off[r] (detect_bits_seg_k), so no run, gap or event crosses recordings.
// The walk itself is detect_walk_body of detect_shared.h (shared with the decoder sweep of tune.hip); here every finished event
// is counted and, in the write pass, stored.
struct DetectEmit {
    int write, max_events, k, r;
    long base;
    int *cls, *onset, *offset, *rec;
    int cnt;
    __device__ __forceinline__ void operator()(int on, int off) {
        if (write && base + cnt < max_events) {
            cls[base + cnt] = k; onset[base + cnt] = on; offset[base + cnt] = off;
            if (rec) rec[base + cnt] = r;
        }
        ++cnt;
    }
};

template <bool SEG = false>
__global__ __launch_bounds__(64) void detect_walk_k(const unsigned long long* __restrict__ on_bits,
                                                    const unsigned long long* __restrict__ hi_bits, long n_words, int min_gap,
                                                    int min_len, int write, int max_events, int* __restrict__ counts,
                                                    const int* __restrict__ offsets, int* __restrict__ cls,
                                                    int* __restrict__ onset, int* __restrict__ offset,
                                                    const int* __restrict__ word_off = nullptr, int K = 0, int* __restrict__ rec = nullptr) {
    __shared__ int epos[DETECT_EDGE_CAP], eh[DETECT_EDGE_CAP];
    const int r = SEG ? (int)blockIdx.x / K : 0;
    const int k = SEG ? (int)blockIdx.x - r * K : (int)blockIdx.x;
    size_t track0 = 0;
    if (SEG) {
        track0 = (size_t)K * word_off[r];
        n_words = word_off[r + 1] - word_off[r];
    }
    DetectEmit emit{write, max_events, k, r, write ? (long)offsets[blockIdx.x] : 0l, cls, onset, offset, SEG ? rec : nullptr, 0};
    detect_walk_body(on_bits + track0 + (size_t)k * n_words, hi_bits + track0 + (size_t)k * n_words, n_words, min_gap, min_len,
                     epos, eh, emit);
    if (threadIdx.x == 0 && !write) counts[blockIdx.x] = emit.cnt;
}

// detect_walk_k with class k's own min_gap and min_len, read from the by-value table (k is workgroup-uniform)
template <bool SEG = false>
__global__ __launch_bounds__(64) void detect_walk_cw_k(const unsigned long long* __restrict__ on_bits,
                                                       const unsigned long long* __restrict__ hi_bits, long n_words, ClassTable tab, int write,
                                                       int max_events, int* __restrict__ counts, const int* __restrict__ offsets,
                                                       int* __restrict__ cls, int* __restrict__ onset, int* __restrict__ offset,
                                                       const int* __restrict__ word_off = nullptr, int K = 0, int* __restrict__ rec = nullptr) {
    __shared__ int epos[DETECT_EDGE_CAP], eh[DETECT_EDGE_CAP];
    const int r = SEG ? (int)blockIdx.x / K : 0;
    const int k = SEG ? (int)blockIdx.x - r * K : (int)blockIdx.x;
    size_t track0 = 0;
    if (SEG) {
        track0 = (size_t)K * word_off[r];
        n_words = word_off[r + 1] - word_off[r];
    }
    DetectEmit emit{write, max_events, k, r, write ? (long)offsets[blockIdx.x] : 0l, cls, onset, offset, SEG ? rec : nullptr, 0};
    detect_walk_body(on_bits + track0 + (size_t)k * n_words, hi_bits + track0 + (size_t)k * n_words, n_words, tab.c[k].min_gap,
                     tab.c[k].min_len, epos, eh, emit);
    if (threadIdx.x == 0 && !write) counts[blockIdx.x] = emit.cnt;
}

__global__ void detect_offsets_k(const int* __restrict__ counts, int K, int* __restrict__ offsets, int* __restrict__ total) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int t = 0;
    for (int k = 0; k < K; ++k) { offsets[k] = t; t += counts[k]; }
    *total = t;
}

// the batch: detect_scan_k of detect_shared.h turns the R*K counts into offsets [R*K] and event_off [R+1]

// one workgroup per event (grid-stride over the events): max of the unfiltered track over [onset, offset), first arg-max.
// SEG: event e belongs to recording rec[e], whose track starts at packed row out_off[rec[e]]
template <bool SEG = false>
__global__ __launch_bounds__(256) void detect_peaks_k(const float* __restrict__ probs, int K, const int* __restrict__ total,
                                                      int max_events, const int* __restrict__ cls, const int* __restrict__ onset,
                                                      const int* __restrict__ offset, float* __restrict__ peak,
                                                      int* __restrict__ peak_frame, const int* __restrict__ rec = nullptr,
                                                      const int* __restrict__ out_off = nullptr) {
    __shared__ float sv[4];
    __shared__ int si[4];
    const int n = *total < max_events ? *total : max_events;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const int k = cls[e], a = onset[e], b = offset[e];
        const float* pr = SEG ? probs + (size_t)out_off[rec[e]] * K : probs;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = a + (int)threadIdx.x; j < b; j += 256) {
            const float v = pr[(size_t)j * K + k];
            if (v > bv) { bv = v; bi = j; }                       // ascending j: the first maximum of this thread's frames
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int q = 1; q < 4; ++q)
                if (sv[q] > bv || (sv[q] == bv && si[q] < bi)) { bv = sv[q]; bi = si[q]; }
            peak[e] = bv;
            peak_frame[e] = bi;
        }
        __syncthreads();
    }
}

extern "C" size_t sed_detect_workspace_bytes(long n_out, int K, int max_events) {
    if (n_out < 1 || n_out > 0x7fffffffL || K < 1 || K > 32 || max_events < 0 || n_out * K > 0x7fffffffL) return 0;
    return (size_t)2 * K * detect_words(n_out) * sizeof(unsigned long long) + (size_t)2 * K * sizeof(int);
}

extern "C" int sed_detect_events(const float* probs, long n_out, int K, int median, float lo, float hi, int min_gap, int min_len,
                                 int max_events, void* workspace, size_t workspace_bytes, int* cls, int* onset, int* offset,
                                 float* peak, int* peak_frame, int* count, void* stream) {
    SED_REQUIRE(probs && workspace && count, "detect_events: null pointer");
    const size_t need = sed_detect_workspace_bytes(n_out, K, max_events);
    SED_REQUIRE(need > 0, "detect_events: bad sizes (n_out=%ld, K=%d in 1..32, max_events=%d >= 0)", n_out, K, max_events);
    SED_REQUIRE(workspace_bytes >= need, "detect_events: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_TRY(detect_check_decoder("detect_events", -1, median, lo, hi, min_gap, min_len));
    SED_REQUIRE(max_events == 0 || (cls && onset && offset && peak && peak_frame), "detect_events: null output pointer");
    hipStream_t s = as_stream(stream);
    const long nw = detect_words(n_out);
    unsigned long long* ob = (unsigned long long*)workspace;
    unsigned long long* hb = ob + (size_t)K * nw;
    int* counts = (int*)(hb + (size_t)K * nw);
    int* offs = counts + K;
    detect_with_median(median, [&](auto m) {
        detect_bits_k<decltype(m)::value><<<dim3((unsigned)cdiv(nw * 64, 256), (unsigned)K), 256, 0, s>>>(probs, (int)n_out, K, nw, lo, hi, ob,
                                                                                                   hb);
    });
    SED_LAUNCH_CHECK("detect_bits");
    detect_walk_k<<<K, 64, 0, s>>>(ob, hb, nw, min_gap, min_len, 0, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk(count)");
    detect_offsets_k<<<1, 64, 0, s>>>(counts, K, offs, count);
    SED_LAUNCH_CHECK("detect_offsets");
    if (max_events == 0) return 0;
    detect_walk_k<<<K, 64, 0, s>>>(ob, hb, nw, min_gap, min_len, 1, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk(write)");
    detect_peaks_k<<<max_events < 1024 ? max_events : 1024, 256, 0, s>>>(probs, K, count, max_events, cls, onset, offset, peak, peak_frame);
    SED_LAUNCH_CHECK("detect_peaks");
    return 0;
}

// Class-wise settings: classes_host [K] rows {median, lo, hi, min_gap, min_len}, class k decoded with row k.  The same
// workspace, outputs and phases as sed_detect_events; the bit tracks are packed by one launch per distinct median width.
extern "C" int sed_detect_events_classwise(const float* probs, long n_out, int K, const sed_tune_setting* classes_host, int max_events,
                                           void* workspace, size_t workspace_bytes, int* cls, int* onset, int* offset, float* peak,
                                           int* peak_frame, int* count, void* stream) {
    SED_REQUIRE(probs && classes_host && workspace && count, "detect_events_classwise: null pointer");
    const size_t need = sed_detect_workspace_bytes(n_out, K, max_events);
    SED_REQUIRE(need > 0, "detect_events_classwise: bad sizes (n_out=%ld, K=%d in 1..32, max_events=%d >= 0)", n_out, K, max_events);
    SED_REQUIRE(workspace_bytes >= need, "detect_events_classwise: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    ClassTable tab;
    int widest;
    SED_TRY(detect_class_table("detect_events_classwise", classes_host, K, tab, &widest));
    SED_REQUIRE(max_events == 0 || (cls && onset && offset && peak && peak_frame), "detect_events_classwise: null output pointer");
    hipStream_t s = as_stream(stream);
    const long nw = detect_words(n_out);
    unsigned long long* ob = (unsigned long long*)workspace;
    unsigned long long* hb = ob + (size_t)K * nw;
    int* counts = (int*)(hb + (size_t)K * nw);
    int* offs = counts + K;
    detect_for_widths(tab, K, [&](auto m, const ClassList& list) {
        detect_bits_cw_k<decltype(m)::value><<<dim3((unsigned)cdiv(nw * 64, 256), (unsigned)list.n), 256, 0, s>>>(probs, (int)n_out, K, nw, list,
                                                                                                           tab, ob, hb);
    });
    SED_LAUNCH_CHECK("detect_bits_classwise");
    detect_walk_cw_k<<<K, 64, 0, s>>>(ob, hb, nw, tab, 0, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk_classwise(count)");
    detect_offsets_k<<<1, 64, 0, s>>>(counts, K, offs, count);
    SED_LAUNCH_CHECK("detect_offsets");
    if (max_events == 0) return 0;
    detect_walk_cw_k<<<K, 64, 0, s>>>(ob, hb, nw, tab, 1, max_events, counts, offs, cls, onset, offset);
    SED_LAUNCH_CHECK("detect_walk_classwise(write)");
    detect_peaks_k<<<max_events < 1024 ? max_events : 1024, 256, 0, s>>>(probs, K, count, max_events, cls, onset, offset, peak, peak_frame);
    SED_LAUNCH_CHECK("detect_peaks");
    return 0;
}

// ───────────────────────── batch: R recordings packed back to back ─────────────────────────
// Phase 1 of the batch is detect_bits_seg_k of detect_shared.h (shared with the decoder sweep) with the two thresholds lo, hi:
// track 0 = on, track 1 = high.
//
// workspace of the batch entries (16-byte aligned regions): the stitch's DetRec [R] and output offsets [R+1]; the decoder's output
// and word offsets [R+1] each, counts [R*K], offsets [R*K]; then the two bit tracks [K][words], words <= n_total/64 + R
struct DetBatchWs {
    DetRec* recs; int* s_out_off; int* out_off; int* word_off; int* counts; int* offs; unsigned long long* ob; unsigned long long* hb;
};
static DetBatchWs det_batch_layout(void* ws, int R, int K, long words) {
    char* p = (char*)ws;
    DetBatchWs w;
    w.recs = (DetRec*)p; p += al16((size_t)R * sizeof(DetRec));
    w.s_out_off = (int*)p; p += al16((size_t)(R + 1) * 4);
    w.out_off = (int*)p; p += al16((size_t)(R + 1) * 8);           // out_off [R+1] then word_off [R+1]: one upload
    w.word_off = w.out_off + R + 1;
    w.counts = (int*)p; p += al16((size_t)R * K * 4);
    w.offs = (int*)p; p += al16((size_t)R * K * 4);
    w.ob = (unsigned long long*)p;
    w.hb = w.ob + (size_t)K * words;
    return w;
}

extern "C" size_t sed_detect_batch_workspace_bytes(long n_total, int K, int R, int max_events) {
    if (R < 1 || n_total < R || n_total > 0x7fffffffL || K < 1 || K > 32 || max_events < 0 || n_total * K > 0x7fffffffL) return 0;
    const long words = n_total / 64 + R;
    return al16((size_t)R * sizeof(DetRec)) + al16((size_t)(R + 1) * 4) + al16((size_t)(R + 1) * 8) + 2 * al16((size_t)R * K * 4) +
           (size_t)2 * K * words * sizeof(unsigned long long);
}

extern "C" int sed_detect_stitch_batch(const float* logits, long logits_len, const long* recs_host, int R, int K, int combine, int trim,
                                       float* probs, long n_total, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(logits && recs_host && probs && workspace, "detect_stitch_batch: null pointer");
    const size_t need = sed_detect_batch_workspace_bytes(n_total, K, R, 0);
    SED_REQUIRE(need > 0 && logits_len >= 1, "detect_stitch_batch: bad sizes (R=%d, K=%d in 1..32, n_total=%ld)", R, K, n_total);
    SED_REQUIRE(workspace_bytes >= need, "detect_stitch_batch: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(combine == 0 || combine == 1, "detect_stitch_batch: combine must be 0 (mean) or 1 (max), got %d", combine);
    SED_REQUIRE(trim >= 0, "detect_stitch_batch: trim must be >= 0 (got %d)", trim);
    std::vector<DetRec> h(R);
    std::vector<int> off(R + 1);
    struct Ext { long lo, hi; int r; };
    std::vector<Ext> ext(R);
    long rows = 0;
    for (int r = 0; r < R; ++r) {
        const long* d = recs_host + 6 * r;
        const long lo = d[0], n_win = d[1], win_out = d[2], hop_out = d[3], last = d[4], n_out = d[5];
        SED_REQUIRE(n_win >= 1 && win_out >= 1 && hop_out >= 1 && last >= 0 && n_out >= 1 && n_win <= 0x7fffffffL &&
                        win_out <= 0x7fffffffL && hop_out <= 0x7fffffffL && n_out <= n_total,
                    "detect_stitch_batch: recording %d: bad sizes (n_win=%ld, win_out=%ld, hop_out=%ld, n_out=%ld)", r, n_win, win_out,
                    hop_out, n_out);
        SED_TRY(detect_check_grid("detect_stitch_batch", r, n_win, win_out, hop_out, last, n_out, trim));
        // the logits [n_win][win_out][K] of the recording: inside the buffer (overlaps are checked below)
        SED_REQUIRE(lo >= 0 && lo <= logits_len && n_win * win_out <= (logits_len - lo) / K,
                    "detect_stitch_batch: recording %d: logits [%ld, +%ld x %ld x %d) leave the buffer of %ld floats", r, lo, n_win,
                    win_out, K, logits_len);
        ext[r] = {lo, lo + n_win * win_out * K, r};
        h[r] = DetRec{lo, (int)n_win, (int)win_out, (int)hop_out, (int)last, (int)n_out, 0};
        off[r] = (int)rows;
        rows += n_out;
        SED_REQUIRE(rows <= n_total, "detect_stitch_batch: the recordings have more than n_total=%ld output frames", n_total);
    }
    SED_REQUIRE(rows == n_total, "detect_stitch_batch: the recordings have %ld output frames, probs has %ld", rows, n_total);
    std::sort(ext.begin(), ext.end(), [](const Ext& a, const Ext& b) { return a.lo < b.lo; });
    for (int i = 1; i < R; ++i)
        SED_REQUIRE(ext[i].lo >= ext[i - 1].hi, "detect_stitch_batch: the logits of recordings %d and %d overlap", ext[i - 1].r, ext[i].r);
    off[R] = (int)rows;
    hipStream_t s = as_stream(stream);
    const DetBatchWs w = det_batch_layout(workspace, R, K, n_total / 64 + R);
    SED_TRY(detect_upload("detect_stitch_batch", w.recs, h.data(), (size_t)R * sizeof(DetRec), s));
    SED_TRY(detect_upload("detect_stitch_batch", w.s_out_off, off.data(), (size_t)(R + 1) * 4, s));
    const long nb = (n_total * K + 255) / 256;
    detect_stitch_batch_k<<<(unsigned)(nb < 8192 ? nb : 8192), 256, 0, s>>>(logits, w.recs, w.s_out_off, R, n_total, K, combine, trim,
                                                                              probs);
    SED_LAUNCH_CHECK("detect_stitch_batch");
    return 0;
}

extern "C" int sed_detect_events_batch(const float* probs, const long* n_out_host, int R, int K, int median, float lo, float hi,
                                       int min_gap, int min_len, int max_events, void* workspace, size_t workspace_bytes, int* rec,
                                       int* cls, int* onset, int* offset, float* peak, int* peak_frame, int* event_off, void* stream) {
    SED_REQUIRE(probs && n_out_host && workspace && event_off, "detect_events_batch: null pointer");
    SED_REQUIRE(R >= 1 && K >= 1 && K <= 32 && max_events >= 0, "detect_events_batch: bad sizes (R=%d, K=%d in 1..32, max_events=%d)",
                R, K, max_events);
    SED_TRY(detect_check_decoder("detect_events_batch", -1, median, lo, hi, min_gap, min_len));
    SED_REQUIRE(max_events == 0 || (rec && cls && onset && offset && peak && peak_frame), "detect_events_batch: null output pointer");
    std::vector<int> h(2 * (size_t)(R + 1));                          // out_off [R+1] then word_off [R+1]
    long rows, words;
    SED_TRY(detect_seg_tables("detect_events_batch", n_out_host, R, K, h.data(), h.data() + R + 1, &rows, &words));
    const size_t need = sed_detect_batch_workspace_bytes(rows, K, R, max_events);
    SED_REQUIRE(need > 0, "detect_events_batch: bad sizes (R=%d, K=%d, %ld output frames)", R, K, rows);
    SED_REQUIRE(workspace_bytes >= need, "detect_events_batch: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const DetBatchWs w = det_batch_layout(workspace, R, K, rows / 64 + R);
    SED_TRY(detect_upload("detect_events_batch", w.out_off, h.data(), h.size() * 4, s));
    launch_bits_seg(median, probs, w.out_off, w.word_off, R, K, words, TwoThresholds{lo, hi}, (size_t)(w.hb - w.ob), w.ob, s);
    SED_LAUNCH_CHECK("detect_bits_seg");
    const unsigned groups = (unsigned)((long)R * K);
    detect_walk_k<true><<<groups, 64, 0, s>>>(w.ob, w.hb, 0, min_gap, min_len, 0, max_events, w.counts, w.offs, cls, onset, offset,
                                             w.word_off, K, rec);
    SED_LAUNCH_CHECK("detect_walk_batch(count)");
    detect_scan_k<<<1, 1024, 0, s>>>(w.counts, R * K, K, w.offs, event_off);
    SED_LAUNCH_CHECK("detect_scan");
    if (max_events == 0) return 0;
    detect_walk_k<true><<<groups, 64, 0, s>>>(w.ob, w.hb, 0, min_gap, min_len, 1, max_events, w.counts, w.offs, cls, onset, offset,
                                             w.word_off, K, rec);
    SED_LAUNCH_CHECK("detect_walk_batch(write)");
    detect_peaks_k<true><<<max_events < 1024 ? max_events : 1024, 256, 0, s>>>(probs, K, event_off + R, max_events, cls, onset, offset,
                                                                              peak, peak_frame, rec, w.out_off);
    SED_LAUNCH_CHECK("detect_peaks_batch");
    return 0;
}

// sed_detect_events_batch with class-wise settings (classes_host [K]): the same workspace, tables, outputs and phases
extern "C" int sed_detect_events_batch_classwise(const float* probs, const long* n_out_host, int R, int K,
                                                 const sed_tune_setting* classes_host, int max_events, void* workspace,
                                                 size_t workspace_bytes, int* rec, int* cls, int* onset, int* offset, float* peak,
                                                 int* peak_frame, int* event_off, void* stream) {
    SED_REQUIRE(probs && n_out_host && classes_host && workspace && event_off, "detect_events_batch_classwise: null pointer");
    SED_REQUIRE(R >= 1 && K >= 1 && K <= 32 && max_events >= 0,
                "detect_events_batch_classwise: bad sizes (R=%d, K=%d in 1..32, max_events=%d)", R, K, max_events);
    ClassTable tab;
    int widest;
    SED_TRY(detect_class_table("detect_events_batch_classwise", classes_host, K, tab, &widest));
    SED_REQUIRE(max_events == 0 || (rec && cls && onset && offset && peak && peak_frame),
                "detect_events_batch_classwise: null output pointer");
    std::vector<int> h(2 * (size_t)(R + 1));                          // out_off [R+1] then word_off [R+1]
    long rows, words;
    SED_TRY(detect_seg_tables("detect_events_batch_classwise", n_out_host, R, K, h.data(), h.data() + R + 1, &rows, &words));
    const size_t need = sed_detect_batch_workspace_bytes(rows, K, R, max_events);
    SED_REQUIRE(need > 0, "detect_events_batch_classwise: bad sizes (R=%d, K=%d, %ld output frames)", R, K, rows);
    SED_REQUIRE(workspace_bytes >= need, "detect_events_batch_classwise: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const DetBatchWs w = det_batch_layout(workspace, R, K, rows / 64 + R);
    SED_TRY(detect_upload("detect_events_batch_classwise", w.out_off, h.data(), h.size() * 4, s));
    detect_for_widths(tab, K, [&](auto m, const ClassList& list) {
        detect_bits_seg_cw_k<decltype(m)::value><<<dim3((unsigned)cdiv(words, 4), (unsigned)list.n), 256, 0, s>>>(
            probs, w.out_off, w.word_off, R, K, list, tab, (size_t)(w.hb - w.ob), w.ob);
    });
    SED_LAUNCH_CHECK("detect_bits_seg_classwise");
    const unsigned groups = (unsigned)((long)R * K);
    detect_walk_cw_k<true><<<groups, 64, 0, s>>>(w.ob, w.hb, 0, tab, 0, max_events, w.counts, w.offs, cls, onset, offset, w.word_off, K, rec);
    SED_LAUNCH_CHECK("detect_walk_batch_classwise(count)");
    detect_scan_k<<<1, 1024, 0, s>>>(w.counts, R * K, K, w.offs, event_off);
    SED_LAUNCH_CHECK("detect_scan");
    if (max_events == 0) return 0;
    detect_walk_cw_k<true><<<groups, 64, 0, s>>>(w.ob, w.hb, 0, tab, 1, max_events, w.counts, w.offs, cls, onset, offset, w.word_off, K, rec);
    SED_LAUNCH_CHECK("detect_walk_batch_classwise(write)");
    detect_peaks_k<true><<<max_events < 1024 ? max_events : 1024, 256, 0, s>>>(probs, K, event_off + R, max_events, cls, onset, offset,
                                                                              peak, peak_frame, rec, w.out_off);
    SED_LAUNCH_CHECK("detect_peaks_batch");
    return 0;
}
