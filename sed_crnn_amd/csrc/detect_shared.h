// detect_shared.h — what the offline detector (detect.hip), the streaming step (stream.hip) and the decoder sweep (tune.hip)
// share.  Device code: the stitch of one (output frame, class) cell, the median by selection, the segmented bit-track kernel,
// the edge walk of the event decoder and the exclusive scan of per-(segment, class) event counts.  The files call the SAME
// functions, so a streamed track row is bit for bit the row sed_detect_stitch writes, a streamed filtered frame is the frame the
// offline decoder thresholds, and the events a sweep scores are the events sed_detect_events_batch writes.  Host code: the
// checks that several entries make (decoder settings, window grid, segment tables), the table upload, the dispatch from a
// runtime median width to its instantiation and, for the class-wise entries, the by-value table of per-class settings and the
// lists of classes that share a width.
#pragma once
#include <type_traits>
#include "common.h"

// 64-bit words of one bit track of n_out frames: the extra word holds the fall edge of a run that reaches the end
static inline long detect_words(long n_out) { return n_out / 64 + 1; }
static inline size_t al16(size_t b) { return (b + 15) & ~(size_t)15; }

// ───────────────────────── host: checks, upload, width dispatch ─────────────────────────
// Every check takes the entry's name for the message prefix and returns the error code (SED_TRY); none of them touches HIP.

// the message prefix "entry" or, with an index i >= 0, "entry: what i"; called only when a check fails
static const char* detect_who(const char* entry, const char* what, long i) {
    static thread_local char s[96];
    if (i >= 0) snprintf(s, sizeof s, "%s: %s %ld", entry, what, i);
    return i >= 0 ? s : entry;
}

// the decoder's settings; setting >= 0: the index of the setting in a sweep (or, what = "class", of the class in a class-wise table)
static int detect_check_decoder(const char* entry, long setting, int median, float lo, float hi, int min_gap, int min_len,
                                const char* what = "setting") {
    const auto who = [&] { return detect_who(entry, what, setting); };
    SED_REQUIRE(median >= 1 && median <= 31 && (median & 1), "%s: median width must be odd, 1..31 (got %d)", who(), median);
    SED_REQUIRE(hi >= lo, "%s: need hi >= lo (got lo=%g, hi=%g)", who(), (double)lo, (double)hi);
    SED_REQUIRE(min_gap >= 0 && min_len >= 1, "%s: min_gap >= 0 and min_len >= 1 (got %d, %d)", who(), min_gap, min_len);
    return 0;
}

// trim output frames dropped at interior window edges must leave every frame covered (one window has no interior edge)
static int detect_check_trim(const char* entry, long rec, long n_win, long win_out, long hop_out, int trim) {
    SED_REQUIRE(trim >= 0 && (n_win == 1 || hop_out + 2L * trim <= win_out),
                "%s: trim=%d leaves output frames uncovered (hop_out=%ld, win_out=%ld)", detect_who(entry, "recording", rec), trim,
                hop_out, win_out);
    return 0;
}

// the window grid of one recording, start(w) = min(w hop_out, last): the last window ends at n_out and starts at `last`, every
// earlier one strictly before it; rec >= 0: the index of the recording in a batch
static int detect_check_grid(const char* entry, long rec, long n_win, long win_out, long hop_out, long last, long n_out, int trim) {
    const auto who = [&] { return detect_who(entry, "recording", rec); };
    SED_REQUIRE(last + win_out == n_out, "%s: the last window must end at the recording's end", who());
    SED_REQUIRE((n_win - 1) * hop_out >= last && (n_win < 2 || (n_win - 2) * hop_out < last),
                "%s: last_start_out=%ld is not the last start of a %ld-window grid with hop %ld", who(), last, n_win, hop_out);
    return detect_check_trim(entry, rec, n_win, win_out, hop_out, trim);
}

// n_out_host [R] -> out_off [R+1] (first packed row of every recording) and word_off [R+1] (first word of its bit tracks, per
// class); *rows and *words receive the totals.  Rows and (frame, class) cells are int32 on the device.
static int detect_seg_tables(const char* entry, const long* n_out_host, int R, int K, int* out_off, int* word_off, long* rows,
                             long* words) {
    *rows = *words = 0;
    for (int r = 0; r < R; ++r) {
        const long n = n_out_host[r];
        SED_REQUIRE(n >= 1 && n <= 0x7fffffffL - *rows, "%s: recording %d has %ld output frames", entry, r, n);
        out_off[r] = (int)*rows;
        word_off[r] = (int)*words;
        *rows += n;
        *words += detect_words(n);
        SED_REQUIRE(*rows * K <= 0x7fffffffL, "%s: more than 2^31 - 1 (frame, class) cells in one batch", entry);
    }
    out_off[R] = (int)*rows;
    word_off[R] = (int)*words;
    return 0;
}

// a host table into the workspace, in stream order before the kernels that read it
static int detect_upload(const char* entry, void* dst, const void* src, size_t bytes, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("%s: upload of the host tables: %s", entry, hipGetErrorString(e)); return (int)e; }
    return 0;
}

// f(std::integral_constant<int, M>) with M = median, for every width the decoder accepts (detect_check_decoder)
template <class F>
static void detect_with_median(int median, F&& f) {
    switch (median) {
#define DETECT_MED(m) case m: f(std::integral_constant<int, m>{}); break;
        DETECT_MED(1) DETECT_MED(3) DETECT_MED(5) DETECT_MED(7) DETECT_MED(9) DETECT_MED(11) DETECT_MED(13) DETECT_MED(15)
        DETECT_MED(17) DETECT_MED(19) DETECT_MED(21) DETECT_MED(23) DETECT_MED(25) DETECT_MED(27) DETECT_MED(29) DETECT_MED(31)
#undef DETECT_MED
    }
}

// Class-wise decoder settings (the *_classwise entries).  K <= 32, so the K rows travel BY VALUE as a kernel
// argument (640 bytes): no upload, no workspace.  The bit-track kernels are launched once per distinct median width over the
// list of classes that have it, so the width stays a template argument and no wave ever chooses among instantiations.
struct ClassTable { sed_tune_setting c[32]; };
struct ClassList { int n; unsigned char k[32]; };                  // the classes that share one median width, ascending

// classes_host [K] (K already checked to be 1..32) -> tab, every row checked like the scalar entry's five values;
// *widest = the largest median width
static int detect_class_table(const char* entry, const sed_tune_setting* classes_host, int K, ClassTable& tab, int* widest) {
    tab = ClassTable{};
    *widest = 1;
    for (int k = 0; k < K; ++k) {
        const sed_tune_setting c = classes_host[k];
        SED_TRY(detect_check_decoder(entry, k, c.median, c.lo, c.hi, c.min_gap, c.min_len, "class"));
        tab.c[k] = c;
        *widest = c.median > *widest ? c.median : *widest;
    }
    return 0;
}

// f(std::integral_constant<int, M>, ClassList) for every median width M that a class has, in increasing width
template <class F>
static void detect_for_widths(const ClassTable& tab, int K, F&& f) {
    for (int m = 1; m <= 31; m += 2) {
        ClassList l{};
        for (int k = 0; k < K; ++k)
            if (tab.c[k].median == m) l.k[l.n++] = (unsigned char)k;
        if (l.n) detect_with_median(m, [&](auto mm) { f(mm, l); });
    }
}

// ───────────────────────── device ─────────────────────────
// last r with off[r] <= x (off[0] = 0 <= x, off ascending)
__device__ __forceinline__ int find_seg(const int* __restrict__ off, int R, long x) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// where row t (class 0) of a track lives: rows back to back, or the streaming step's ring of TR rows
struct LinearRows {
    const float* base; int K;
    __device__ __forceinline__ const float* at(int t) const { return base + (size_t)t * K; }
};
struct RingRows {
    const float* base; int TR, K;
    __device__ __forceinline__ const float* at(int t) const { return base + (size_t)(t % TR) * K; }
};

// median of the M frames around j of class k, edges 'nearest': the left edge clamps at frame 0, the right one at `last` (the
// last frame of a finished track; INT_MAX while a stream goes on); a selection (exact, ties included)
template <int M, class Rows>
__device__ __forceinline__ float median_nearest(const Rows& rows, int j, int k, int last) {
    if (M == 1) return rows.at(j)[k];
    float v[M];
#pragma unroll
    for (int d = 0; d < M; ++d) {
        int t = j + d - M / 2;
        t = t < 0 ? 0 : (t > last ? last : t);
        v[d] = rows.at(t)[k];
    }
    float med = v[0];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        int less = 0, leq = 0;
#pragma unroll
        for (int d = 0; d < M; ++d) { less += v[d] < v[i]; leq += v[d] <= v[i]; }
        if (less <= M / 2 && M / 2 < leq) med = v[i];                 // v[i] is the (M/2)-th smallest
    }
    return med;
}

// The thresholds a bit-track launch compares the filtered value with: the detector's two, by value, or a sweep's list
struct TwoThresholds {
    float lo, hi;
    __device__ __forceinline__ int n() const { return 2; }
    __device__ __forceinline__ float at(int t) const { return t ? hi : lo; }
};
struct ThresholdList {
    const float* thr; int n_thr;
    __device__ __forceinline__ int n() const { return n_thr; }
    __device__ __forceinline__ float at(int t) const { return thr[t]; }
};

// Bit tracks of R recordings packed back to back (sed_detect_events_batch, sed_tune_sweep): one wave per (packed word, class).
// A wave's 64 frames are one word of one recording's track (tracks start on word boundaries), so the recording is wave-uniform;
// the median clamps at that recording's own ends.  The filtered value is computed once and compared with every threshold t:
// track t = bits + t*track_stride, recording r's words [K][n_words_r] at word K*word_off[r] of it (one spare word per
// recording), so no run, gap or event crosses recordings.
template <int M, class Thr>
__global__ __launch_bounds__(256) void detect_bits_seg_k(const float* __restrict__ probs, const int* __restrict__ out_off,
                                                         const int* __restrict__ word_off, int R, int K, Thr thr, size_t track_stride,
                                                         unsigned long long* __restrict__ bits) {
    const int k = blockIdx.y, lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= word_off[R]) return;                                    // wave-uniform
    const int r = __builtin_amdgcn_readfirstlane(find_seg(word_off, R, gw));
    const int n_out = out_off[r + 1] - out_off[r], nw = word_off[r + 1] - word_off[r], lw = gw - word_off[r];
    const int j = lw * 64 + lane;
    const bool in = j < n_out;
    const float p = in ? median_nearest<M>(LinearRows{probs + (size_t)out_off[r] * K, K}, j, k, n_out - 1) : 0.f;
    const size_t at = (size_t)K * word_off[r] + (size_t)k * nw + lw;
    for (int t = 0; t < thr.n(); ++t) {
        const unsigned long long b = __ballot(in && p > thr.at(t));
        if (lane == 0) bits[(size_t)t * track_stride + at] = b;
    }
}

// The class-wise form (sed_detect_events_batch_classwise): grid y walks the classes of ONE median width (ClassList) and class k's
// filtered value — the same median_nearest<M> call — is compared with its own lo (track 0) and hi (track 1), into the same words.
template <int M>
__global__ __launch_bounds__(256) void detect_bits_seg_cw_k(const float* __restrict__ probs, const int* __restrict__ out_off,
                                                            const int* __restrict__ word_off, int R, int K, ClassList list, ClassTable tab,
                                                            size_t track_stride, unsigned long long* __restrict__ bits) {
    const int k = list.k[blockIdx.y], lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= word_off[R]) return;                                    // wave-uniform
    const int r = __builtin_amdgcn_readfirstlane(find_seg(word_off, R, gw));
    const int n_out = out_off[r + 1] - out_off[r], nw = word_off[r + 1] - word_off[r], lw = gw - word_off[r];
    const int j = lw * 64 + lane;
    const bool in = j < n_out;
    const float p = in ? median_nearest<M>(LinearRows{probs + (size_t)out_off[r] * K, K}, j, k, n_out - 1) : 0.f;
    const size_t at = (size_t)K * word_off[r] + (size_t)k * nw + lw;
    const unsigned long long bo = __ballot(in && p > tab.c[k].lo), bh = __ballot(in && p > tab.c[k].hi);
    if (lane == 0) {
        bits[at] = bo;
        bits[track_stride + at] = bh;
    }
}

// words = word_off[R] on the host
template <class Thr>
static void launch_bits_seg(int median, const float* probs, const int* out_off, const int* word_off, int R, int K, long words, Thr thr,
                            size_t track_stride, unsigned long long* bits, hipStream_t s) {
    detect_with_median(median, [&](auto m) {
        detect_bits_seg_k<decltype(m)::value><<<dim3((unsigned)cdiv(words, 4), (unsigned)K), 256, 0, s>>>(probs, out_off, word_off, R, K, thr,
                                                                                                   track_stride, bits);
    });
}

// The edge walk of the event decoder, run by ONE wave over the two bit tracks of one (recording, class): ob = p' > lo,
// hb = p' > hi, n_words 64-bit words each.  64-word chunks: edges from on ^ (on << 1), the number of high bits before every
// edge from a wave scan of popcounts, so a run [a, b) is kept iff H(b) - H(a) > 0; lane 0 then walks the chunk's edge list with
// the carried state (open run, pending event) to merge across gaps of <= min_gap frames and drop events shorter than min_len.
// emit(onset, offset) is called by lane 0 for every finished event, in increasing onset.  epos / eh: DETECT_EDGE_CAP ints of
// LDS each; the workgroup is the one wave (the barriers are the wave's own).
#define DETECT_EDGE_CAP 4096                                      // 64 words x 64 bits: every edge of a chunk
template <class Emit>
__device__ __forceinline__ void detect_walk_body(const unsigned long long* __restrict__ ob, const unsigned long long* __restrict__ hb,
                                                 long n_words, int min_gap, int min_len, int* epos, int* eh, Emit& emit) {
    const int lane = threadIdx.x;
    unsigned carry_top = 0;                      // bit 63 of the previous chunk's last word
    long hbase = 0;                              // high bits before this chunk
    // lane 0's walk state
    bool open = false, have = false;
    int r_on = 0, p_on = 0, p_off = 0;
    long r_h = 0;
    for (long w0 = 0; w0 < n_words; w0 += 64) {
        const long w = w0 + lane;
        const unsigned long long on = w < n_words ? ob[w] : 0ull, hi = w < n_words ? hb[w] : 0ull;
        unsigned prev = __shfl((unsigned)(on >> 63), (lane + 63) & 63, 64);
        if (lane == 0) prev = carry_top;
        const unsigned long long sh = (on << 1) | prev;
        const unsigned long long edges = on ^ sh;                // rises (on & ~sh) and falls (~on & sh) alternate globally
        int hc = __popcll(hi), ne = __popcll(edges);
        int hpre = hc, epre = ne;                                // inclusive wave scans
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int a = __shfl_up(hpre, o, 64), b = __shfl_up(epre, o, 64);
            if (lane >= o) { hpre += a; epre += b; }
        }
        const int n_edges = __shfl(epre, 63, 64), n_high = __shfl(hpre, 63, 64);
        hpre -= hc;
        epre -= ne;
        for (unsigned long long m = edges; m; m &= m - 1) {
            const int b = __ffsll((long long)m) - 1;
            epos[epre] = (int)(w * 64 + b);
            eh[epre] = (int)(hbase + hpre + __popcll(hi & ((1ull << b) - 1ull)));
            ++epre;
        }
        __syncthreads();
        if (lane == 0) {
            for (int e = 0; e < n_edges; ++e) {
                if (!open) { open = true; r_on = epos[e]; r_h = eh[e]; continue; }
                open = false;
                const int r_off = epos[e];
                if (eh[e] - r_h <= 0) continue;                  // no frame of the run above hi
                if (have && r_on - p_off <= min_gap) { p_off = r_off; continue; }
                if (have && p_off - p_on >= min_len) emit(p_on, p_off);
                have = true; p_on = r_on; p_off = r_off;
            }
        }
        __syncthreads();
        carry_top = (unsigned)__shfl((unsigned)(on >> 63), 63, 64);
        hbase += n_high;
    }
    if (lane == 0 && have && p_off - p_on >= min_len) emit(p_on, p_off);
}

// where the logits of window w, output row `row` (of win_out), class 0 live: the offline paths keep every window back to back
struct LinearLogits {
    const float* base; int win_out, K;
    __device__ __forceinline__ const float* at(int w, int row) const { return base + ((size_t)w * win_out + row) * K; }
};

// One (output frame j, class k): the covering windows are a contiguous range of w (start(w) = min(w hop_out, last_start) is
// strictly increasing); they are visited in increasing w, so the sum has one fixed order (bitwise deterministic, no atomics).
template <class Logits>
__device__ __forceinline__ float stitch_one(const Logits& logits, int n_win, int win_out, int hop_out, int last_start, int n_out,
                                            int combine, int trim, int j, int k) {
    // last window whose start is <= j
    int whi = j >= last_start ? n_win - 1 : j / hop_out;
    if (whi > n_win - 1) whi = n_win - 1;
    int wlo = whi;
    while (wlo > 0) {                                                // first window that still reaches j
        const long s = (long)(wlo - 1) * hop_out < last_start ? (long)(wlo - 1) * hop_out : last_start;
        if (s + win_out <= j) break;
        --wlo;
    }
    float acc = combine ? -INFINITY : 0.f;
    int cnt = 0;
    for (int w = wlo; w <= whi; ++w) {
        const long s = (long)w * hop_out < last_start ? (long)w * hop_out : last_start;
        const long lo = s + (s > 0 ? trim : 0);
        const long hi = s + win_out - (s + win_out < n_out ? trim : 0);
        if (j < lo || j >= hi) continue;
        const float x = logits.at(w, (int)(j - s))[k];
        const float p = 1.0f / (1.0f + expf(-x));
        if (combine) acc = fmaxf(acc, p);
        else acc += p;
        ++cnt;
    }
    return combine ? acc : acc / (float)cnt;                          // cnt >= 1: the host checked coverage
}

// exclusive scan of the n = R*K counts by one workgroup (wave scans + the 16 wave totals, 1 024 counts per step) ->
// offsets [R*K]; event_off [R+1] = the offset of each segment's first class, and the total
static __global__ __launch_bounds__(1024) void detect_scan_k(const int* __restrict__ counts, int n, int K, int* __restrict__ offsets,
                                                             int* __restrict__ event_off) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + tid;
        const int c = i < n ? counts[i] : 0;
        int x = c;                                                    // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        int pre = 0, step = 0;
        for (int w = 0; w < 16; ++w) {
            pre += w < wv ? wsum[w] : 0;
            step += wsum[w];
        }
        const int excl = carry + pre + x - c;
        if (i < n) {
            offsets[i] = excl;
            if (i % K == 0) event_off[i / K] = excl;
        }
        carry += step;
        __syncthreads();                                              // wsum is rewritten by the next step
    }
    if (tid == 0) event_off[n / K] = carry;
}
