// stream.hip — live streams (sed_crnn_amd/stream.py): the state that S feeds keep on the device between pushes and
// the step that advances all of them in one pass — stitch the newly final track frames, filter, walk every (stream, class)
// state machine over its new decided frames, emit events sorted by (stream, class, onset).
//
// Frame arithmetic (output frames).  With n_out_now output frames received, regular window w (start w hop_out) is complete iff
// w hop_out + win_out <= n_out_now; track frame j is FINAL iff j < n_out_now - win_out (every window that covers it is then
// complete, exists in the offline grid and does not touch the recording's end); filtered frame g is DECIDED iff track frame
// g + median/2 is final.  At the end of a stream n_out is known: the offline grid's last window (end-aligned, or the single
// short window of a stream shorter than win_out) arrives with the step and everything left becomes final.
//
// sed_stream_step_classwise is the same step with one row of decoder values per class.  `median` is then the WIDEST
// class median: it sizes the rings and sets the ONE frontier of a feed (frame g of every class is decided once track frame
// g + median/2 is final); class k filters with its own width and walks with its own lo, hi, min_gap and min_len.
#include <vector>
#include "common.h"
#include "detect_shared.h"

// ───────────────────────── state layout ─────────────────────────
// [S][WR] window-logit slots of win_out*K floats (window w lives in slot w % WR), [S][TR][K] track rows (frame j in row
// j % TR), [S][K] decoder states.  The step validates on the host that everything it still reads is inside the rings.
struct DecState {
    int open, r_on, kept; float r_pk; int r_pkf;        // the open run: first frame, one frame above hi seen, peak so far
    int have, p_on, p_off; float p_pk; int p_pkf;       // the pending event [p_on, p_off) and its peak
    float g_pk; int g_pkf;                              // peak of the frames since p_off (folds in iff a run merges)
    int G, pad0, pad1, pad2;                            // decided filtered frames
};
static_assert(sizeof(DecState) == 64, "DecState is 16 words");

struct StreamDims { int S, K, win_out, hop_out, median, max_new, WR, TR; size_t slot, track_off, dec_off, bytes; };

static bool stream_dims(int S, int K, int win_out, int hop_out, int median, int max_new, StreamDims& d) {
    if (S < 1 || S > 65535 || K < 1 || K > 32 || win_out < 1 || win_out > (1 << 16) || hop_out < 1 || hop_out > win_out ||
        median < 1 || median > 31 || !(median & 1) || max_new < 1 || max_new > 1024)
        return false;
    d.S = S; d.K = K; d.win_out = win_out; d.hop_out = hop_out; d.median = median; d.max_new = max_new;
    d.WR = 2 * ((win_out + hop_out - 1) / hop_out) + max_new + 2;
    d.TR = (median - 1) + win_out + (max_new + 1) * hop_out + 2;
    d.slot = (size_t)win_out * K;
    d.track_off = (size_t)S * d.WR * d.slot * sizeof(float);
    d.dec_off = (d.track_off + (size_t)S * d.TR * K * sizeof(float) + 63) & ~(size_t)63;
    d.bytes = d.dec_off + (size_t)S * K * sizeof(DecState);
    return true;
}

extern "C" size_t sed_stream_state_bytes(int S, int K, int win_out, int hop_out, int median, int max_new_windows) {
    StreamDims d;
    return stream_dims(S, K, win_out, hop_out, median, max_new_windows, d) ? d.bytes : 0;
}

extern "C" int sed_stream_reset(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median,
                                int max_new_windows, const int* streams_host, int n_streams, void* stream) {
    SED_REQUIRE(state, "stream_reset: null pointer");
    StreamDims d;
    SED_REQUIRE(stream_dims(S, K, win_out, hop_out, median, max_new_windows, d),
                "stream_reset: bad sizes (S=%d, K=%d in 1..32, win_out=%d, hop_out=%d, median=%d odd 1..31, max_new_windows=%d)", S, K,
                win_out, hop_out, median, max_new_windows);
    SED_REQUIRE(state_bytes >= d.bytes, "stream_reset: state of %zu bytes, %zu needed", state_bytes, d.bytes);
    SED_REQUIRE(n_streams >= 0 && (n_streams == 0 || streams_host), "stream_reset: null stream list");
    for (int i = 0; i < n_streams; ++i)
        SED_REQUIRE(streams_host[i] >= 0 && streams_host[i] < S, "stream_reset: stream %d of %d", streams_host[i], S);
    DecState* dec = (DecState*)((char*)state + d.dec_off);
    if (!streams_host) {                                            // every stream: the rings need no clearing (written before read)
        const hipError_t e = hipMemsetAsync(dec, 0, (size_t)S * K * sizeof(DecState), as_stream(stream));
        if (e != hipSuccess) { sed_set_error("stream_reset: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    for (int i = 0; i < n_streams; ++i) {
        const hipError_t e = hipMemsetAsync(dec + (size_t)streams_host[i] * K, 0, (size_t)K * sizeof(DecState), as_stream(stream));
        if (e != hipSuccess) { sed_set_error("stream_reset: %s", hipGetErrorString(e)); return (int)e; }
    }
    return 0;
}

extern "C" int sed_stream_init(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median,
                               int max_new_windows, void* stream) {
    return sed_stream_reset(state, state_bytes, S, K, win_out, hop_out, median, max_new_windows, nullptr, 0, stream);
}

// ───────────────────────── carry: keep a tail, append what is new ─────────────────────────
// Per stream: concat = [buf[src, src + n_keep) | fresh[new, new + n_new)]; all of it goes to work[work ...) (when there is a
// work buffer) and its last n_tail floats to buf[dst ...).  The PCM carry (work = the clip the log-mel runs on, tail = the next
// carry) and the feature rows (no work buffer, tail = everything) are both this; src and dst are the two halves of a stream's
// region, so no thread reads what another writes.
struct AppendRec { long src, n_keep, fresh, n_new, work, dst, n_tail; };

__global__ __launch_bounds__(256) void stream_append_k(float* __restrict__ buf, const float* __restrict__ fresh,
                                                       float* __restrict__ work, const AppendRec* __restrict__ recs) {
    const AppendRec r = recs[blockIdx.y];
    const long total = r.n_keep + r.n_new;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float v = i < r.n_keep ? buf[r.src + i] : fresh[r.fresh + (i - r.n_keep)];
        if (work) work[r.work + i] = v;
        if (i >= total - r.n_tail) buf[r.dst + (i - (total - r.n_tail))] = v;
    }
}

extern "C" size_t sed_stream_append_workspace_bytes(int S) {
    return S < 1 || S > 65535 ? 0 : (size_t)S * sizeof(AppendRec);
}

extern "C" int sed_stream_append(float* buf, long buf_len, long stride, const float* fresh, long fresh_len, float* work, long work_len,
                                 const long* table_host, int S, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(buf && table_host && workspace, "stream_append: null pointer");
    const size_t need = sed_stream_append_workspace_bytes(S);
    SED_REQUIRE(need > 0 && stride >= 1 && buf_len >= 0 && stride <= buf_len / S && fresh_len >= 0 && work_len >= 0,
                "stream_append: bad sizes (S=%d in 1..65535, stride=%ld, buf_len=%ld)", S, stride, buf_len);
    SED_REQUIRE(workspace_bytes >= need, "stream_append: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE((fresh || fresh_len == 0) && (work || work_len == 0), "stream_append: null buffer with a non-zero length");
    std::vector<AppendRec> h(S);
    long longest = 0, work_at = 0;
    for (int s = 0; s < S; ++s) {
        const long* t = table_host + 7 * s;
        const AppendRec r{t[0], t[1], t[2], t[3], t[4], t[5], t[6]};
        const long lo = (long)s * stride, hi = lo + stride, total = r.n_keep + r.n_new;
        SED_REQUIRE(r.n_keep >= 0 && r.n_new >= 0 && r.n_tail >= 0 && r.n_tail <= total && total <= 0x7fffffffL,
                    "stream_append: stream %d: bad counts (keep %ld, new %ld, tail %ld)", s, r.n_keep, r.n_new, r.n_tail);
        SED_REQUIRE(r.n_keep == 0 || (r.src >= lo && r.src + r.n_keep <= hi), "stream_append: stream %d: the kept floats leave its region", s);
        SED_REQUIRE(r.n_tail == 0 || (r.dst >= lo && r.dst + r.n_tail <= hi), "stream_append: stream %d: the tail leaves its region", s);
        SED_REQUIRE(r.n_keep == 0 || r.n_tail == 0 || r.dst >= r.src + r.n_keep || r.dst + r.n_tail <= r.src,
                    "stream_append: stream %d: source and destination overlap", s);
        SED_REQUIRE(r.n_new == 0 || (r.fresh >= 0 && r.fresh + r.n_new <= fresh_len), "stream_append: stream %d: the new floats leave their buffer", s);
        if (work && total) {
            SED_REQUIRE(r.work >= work_at && r.work + total <= work_len, "stream_append: stream %d: its work floats [%ld, +%ld) overlap "
                        "the previous stream's or leave the buffer of %ld", s, r.work, total, work_len);
            work_at = r.work + total;
        }
        h[s] = r;
        longest = total > longest ? total : longest;
    }
    if (longest == 0) return 0;
    hipStream_t st = as_stream(stream);
    SED_TRY(detect_upload("stream_append", workspace, h.data(), need, st));
    const long nb = (longest + 255) / 256;
    stream_append_k<<<dim3((unsigned)(nb < 1024 ? nb : 1024), (unsigned)S), 256, 0, st>>>(buf, fresh, work, (const AppendRec*)workspace);
    SED_LAUNCH_CHECK("stream_append");
    return 0;
}

// ───────────────────────── the step ─────────────────────────
struct StreamRec {
    long logit_off;
    int n_new, w_first, win_out_s, F_prev, F_now, G_prev, G_now, end, n_out, n_win, last_start, prob_off;
};

// window w of a stream: slot w % WR of its ring
struct RingLogits {
    const float* ring; int WR, slot, K;
    __device__ __forceinline__ const float* at(int w, int row) const { return ring + (size_t)(w % WR) * slot + (size_t)row * K; }
};

// the step's new windows into their slots (a short stream's single window fills the head of slot 0)
__global__ __launch_bounds__(256) void stream_store_k(const float* __restrict__ logits, const StreamRec* __restrict__ recs,
                                                      float* __restrict__ ring, int WR, int slot, int K) {
    const StreamRec r = recs[blockIdx.y];
    const int per = r.win_out_s * K;
    const long total = (long)r.n_new * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i / per), rem = (int)(i - (long)w * per);
        ring[((size_t)blockIdx.y * WR + (r.w_first + w) % WR) * slot + rem] = logits[r.logit_off + i];
    }
}

// one thread per (stream, newly final frame, class): stitch_one on the ring.  Before the end the grid is open to the right
// (no last window, no end of the recording in sight): exactly what the final grid gives for a frame below its last start.
__global__ __launch_bounds__(256) void stream_stitch_k(const StreamRec* __restrict__ recs, const float* __restrict__ ring, int WR,
                                                       int slot, int K, int win_out, int hop_out, int combine, int trim,
                                                       float* __restrict__ track, int TR, float* __restrict__ probs) {
    const StreamRec r = recs[blockIdx.y];
    const long total = (long)(r.F_now - r.F_prev) * K;
    const RingLogits lg{ring + (size_t)blockIdx.y * WR * slot, WR, slot, K};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int jj = (int)(i / K), k = (int)(i - (long)jj * K), j = r.F_prev + jj;
        const float p = r.end ? stitch_one(lg, r.n_win, r.win_out_s, hop_out, r.last_start, r.n_out, combine, trim, j, k)
                              : stitch_one(lg, 0x7fffffff, win_out, hop_out, 0x7fffffff, 0x7fffffff, combine, trim, j, k);
        track[((size_t)blockIdx.y * TR + j % TR) * K + k] = p;
        if (probs) probs[((size_t)r.prob_off + jj) * K + k] = p;
    }
}

// one thread per (stream, newly decided frame, class): median_nearest of detect_shared.h (the offline decoder's) over the track
// ring; the right edge clamps only at the end of the stream, where the last frame is known
template <int M>
__global__ __launch_bounds__(256) void stream_median_k(const StreamRec* __restrict__ recs, const float* __restrict__ track, int TR,
                                                       int K, int max_dg, float* __restrict__ filt) {
    const StreamRec r = recs[blockIdx.y];
    const long total = (long)(r.G_now - r.G_prev) * K;
    const RingRows rows{track + (size_t)blockIdx.y * TR * K, TR, K};
    const int last = r.end ? r.n_out - 1 : 0x7fffffff;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int gg = (int)(i / K), k = (int)(i - (long)gg * K);
        filt[((size_t)blockIdx.y * max_dg + gg) * K + k] = median_nearest<M>(rows, r.G_prev + gg, k, last);
    }
}

// one lane per (stream, class) walks its new decided frames.  WRITE = false counts the events this step emits; a scan turns
// the counts into offsets; WRITE = true walks again from the same state, writes them and commits the state (once).
// the walk of (stream s, class k), i = s*K + k, with that class's four decoder values
template <bool WRITE>
__device__ __forceinline__ void stream_walk_one(const StreamRec* __restrict__ recs, const float* __restrict__ filt,
                                                const float* __restrict__ track, int TR, int K, int max_dg, int i, int s, int k, float lo,
                                                float hi, int min_gap, int min_len, DecState* __restrict__ dec, int* __restrict__ counts,
                                                const int* __restrict__ offsets, int max_events, int* __restrict__ ev_stream,
                                                int* __restrict__ cls, int* __restrict__ onset, int* __restrict__ offset,
                                                float* __restrict__ peak, int* __restrict__ peak_frame) {
    const StreamRec r = recs[s];
    DecState st = dec[i];
    const int base = WRITE ? offsets[i] : 0;
    int cnt = 0;
    auto emit = [&]() {
        if (st.p_off - st.p_on >= min_len) {
            const int e = base + cnt;
            if (WRITE && e < max_events) {
                ev_stream[e] = s; cls[e] = k; onset[e] = st.p_on; offset[e] = st.p_off; peak[e] = st.p_pk; peak_frame[e] = st.p_pkf;
            }
            ++cnt;
        }
        st.have = 0;
    };
    auto close = [&](int g) {                                        // the open run ends before frame g
        st.open = 0;
        if (!st.kept) return;
        if (st.have && st.r_on - st.p_off <= min_gap) {              // merge: the frames since p_off (gap and run) join the event
            st.p_off = g;
            if (st.g_pk > st.p_pk) { st.p_pk = st.g_pk; st.p_pkf = st.g_pkf; }
        } else {
            if (st.have) emit();
            st.have = 1; st.p_on = st.r_on; st.p_off = g; st.p_pk = st.r_pk; st.p_pkf = st.r_pkf;
        }
        st.g_pk = -INFINITY; st.g_pkf = g;
    };
    const float* tr = track + (size_t)s * TR * K;
    const float* fl = filt + (size_t)s * max_dg * K;
    for (int g = r.G_prev; g < r.G_now; ++g) {
        const float pf = fl[(size_t)(g - r.G_prev) * K + k], p = tr[(size_t)(g % TR) * K + k];
        if (pf > lo) {
            if (!st.open) { st.open = 1; st.r_on = g; st.kept = 0; st.r_pk = -INFINITY; st.r_pkf = g; }
            st.kept |= pf > hi;
            if (p > st.r_pk) { st.r_pk = p; st.r_pkf = g; }
        } else if (st.open) {
            close(g);
        }
        if (st.have && p > st.g_pk) { st.g_pk = p; st.g_pkf = g; }
    }
    if (r.end) {
        if (st.open) close(r.n_out);
        if (st.have) emit();
        st = DecState{};                                             // the stream restarts at frame 0
    } else {
        // final once no later run can merge: frames up to p_off + min_gap decided, and no run that began there still open
        if (st.have && r.G_now > st.p_off + min_gap && !(st.open && st.r_on <= st.p_off + min_gap)) emit();
        st.G = r.G_now;
    }
    if (WRITE) dec[i] = st;
    else counts[i] = cnt;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void stream_walk_k(const StreamRec* __restrict__ recs, const float* __restrict__ filt,
                                                     const float* __restrict__ track, int TR, int S, int K, int max_dg, float lo,
                                                     float hi, int min_gap, int min_len, DecState* __restrict__ dec,
                                                     int* __restrict__ counts, const int* __restrict__ offsets, int max_events,
                                                     int* __restrict__ ev_stream, int* __restrict__ cls, int* __restrict__ onset,
                                                     int* __restrict__ offset, float* __restrict__ peak, int* __restrict__ peak_frame) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * K) return;
    const int s = i / K, k = i - s * K;
    stream_walk_one<WRITE>(recs, filt, track, TR, K, max_dg, i, s, k, lo, hi, min_gap, min_len, dec, counts, offsets, max_events,
                           ev_stream, cls, onset, offset, peak, peak_frame);
}

// Class-wise settings (sed_stream_step_classwise): the lane of class k walks with row k of the by-value table.  The
// frontier G is the feed's (decided once track frame g + widest/2 is final), so the walk is the scalar one with other constants.
template <bool WRITE>
__global__ __launch_bounds__(256) void stream_walk_cw_k(const StreamRec* __restrict__ recs, const float* __restrict__ filt,
                                                        const float* __restrict__ track, int TR, int S, int K, int max_dg, ClassTable tab,
                                                        DecState* __restrict__ dec, int* __restrict__ counts,
                                                        const int* __restrict__ offsets, int max_events, int* __restrict__ ev_stream,
                                                        int* __restrict__ cls, int* __restrict__ onset, int* __restrict__ offset,
                                                        float* __restrict__ peak, int* __restrict__ peak_frame) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * K) return;
    const int s = i / K, k = i - s * K;
    const sed_tune_setting c = tab.c[k];
    stream_walk_one<WRITE>(recs, filt, track, TR, K, max_dg, i, s, k, c.lo, c.hi, c.min_gap, c.min_len, dec, counts, offsets, max_events,
                           ev_stream, cls, onset, offset, peak, peak_frame);
}

// stream_median_k for the classes of ONE median width (ClassList): one thread per (stream, newly decided frame, listed class)
template <int M>
__global__ __launch_bounds__(256) void stream_median_cw_k(const StreamRec* __restrict__ recs, const float* __restrict__ track, int TR,
                                                          int K, int max_dg, ClassList list, float* __restrict__ filt) {
    const StreamRec r = recs[blockIdx.y];
    const long total = (long)(r.G_now - r.G_prev) * list.n;
    const RingRows rows{track + (size_t)blockIdx.y * TR * K, TR, K};
    const int last = r.end ? r.n_out - 1 : 0x7fffffff;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int gg = (int)(i / list.n), k = list.k[i - (long)gg * list.n];
        filt[((size_t)blockIdx.y * max_dg + gg) * K + k] = median_nearest<M>(rows, r.G_prev + gg, k, last);
    }
}

static inline size_t st_al(size_t b) { return (b + 63) & ~(size_t)63; }

extern "C" size_t sed_stream_step_workspace_bytes(int S, int K, int max_new_decided) {
    if (S < 1 || S > 65535 || K < 1 || K > 32 || max_new_decided < 0 || max_new_decided > (1 << 20)) return 0;
    return st_al((size_t)S * sizeof(StreamRec)) + 2 * st_al((size_t)S * K * 4) + st_al((size_t)S * (max_new_decided > 0 ? max_new_decided : 1) * K * 4);
}

static inline long n_regular(long n_out, int win_out, int hop_out) { return n_out >= win_out ? (n_out - win_out) / hop_out + 1 : 0; }

// Both step entries.  `median` sizes the rings and sets the frontier; tab = nullptr: the scalar entry, one decoder setting
// (median, lo, hi, min_gap, min_len) for every class; otherwise the class-wise entry (`median` = the widest class's width, the
// four scalars unused).  `who` prefixes the messages.
static int stream_step_impl(const char* who, const ClassTable* tab, void* state, size_t state_bytes, int S, int K, int win_out,
                            int hop_out, int median, int max_new_windows, int combine, int trim, float lo, float hi, int min_gap,
                            int min_len, const float* logits, long logits_len, const long* table_host, int max_new_decided, float* probs,
                            long probs_rows, int max_events, int* ev_stream, int* cls, int* onset, int* offset, float* peak,
                            int* peak_frame, int* event_off, void* workspace, size_t workspace_bytes, void* stream) {
    StreamDims d;
    SED_REQUIRE(stream_dims(S, K, win_out, hop_out, median, max_new_windows, d),
                "%s: bad sizes (S=%d, K=%d in 1..32, win_out=%d, hop_out=%d, median=%d odd 1..31, max_new_windows=%d)", who, S, K,
                win_out, hop_out, median, max_new_windows);
    SED_REQUIRE(state_bytes >= d.bytes, "%s: state of %zu bytes, %zu needed", who, state_bytes, d.bytes);
    const size_t need = sed_stream_step_workspace_bytes(S, K, max_new_decided);
    SED_REQUIRE(need > 0, "%s: bad max_new_decided=%d", who, max_new_decided);
    SED_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    SED_REQUIRE(combine == 0 || combine == 1, "%s: combine must be 0 (mean) or 1 (max), got %d", who, combine);
    SED_TRY(detect_check_trim(who, -1, 2, win_out, hop_out, trim));        // n_win = 2: a stream may always grow past one window
    if (!tab) SED_TRY(detect_check_decoder(who, -1, median, lo, hi, min_gap, min_len));
    SED_REQUIRE(max_events >= 0 && (max_events == 0 || (ev_stream && cls && onset && offset && peak && peak_frame)),
                "%s: null output pointer", who);
    SED_REQUIRE(logits_len >= 0 && (logits || logits_len == 0) && probs_rows >= 0 && (probs || probs_rows == 0),
                "%s: null buffer with a non-zero length", who);
    const int r = median / 2;
    std::vector<StreamRec> h(S);
    long most_new = 0, most_df = 0, most_dg = 0;
    for (int s = 0; s < S; ++s) {
        const long* t = table_host + 8 * s;
        const long n_new = t[0], lg = t[1], w_first = t[2], prev = t[3], now = t[4], end = t[5], wos = t[6], poff = t[7];
        SED_REQUIRE(prev >= 0 && now >= 0 && now <= 0x3fffffffL && (end == 0 || end == 1), "%s: stream %d: bad frame counts", who, s);
        SED_REQUIRE(now >= prev, "%s: stream %d: n_out goes backwards (%ld after %ld)", who, s, now, prev);
        SED_REQUIRE(w_first == n_regular(prev, win_out, hop_out), "%s: stream %d: %ld windows done do not match n_out=%ld", who, s, w_first, prev);
        long n_win = n_regular(now, win_out, hop_out), want_wos = win_out, last_start = 0;
        if (end) {
            SED_REQUIRE(now >= 1, "%s: stream %d ends without one output frame", who, s);
            if (now >= win_out) {
                last_start = now - win_out;
                if ((n_win - 1) * hop_out != last_start) ++n_win;    // the end-aligned window
            } else {
                n_win = 1; want_wos = now;                           // one short window
            }
        }
        SED_REQUIRE(n_new == n_win - w_first && wos == want_wos && n_new <= max_new_windows + end,
                    "%s: stream %d: %ld new windows of %ld frames, the grid has %ld of %ld (at most %d per step)", who, s, n_new, wos,
                    n_win - w_first, want_wos, max_new_windows);
        SED_REQUIRE(n_new == 0 || (lg >= 0 && lg <= logits_len && n_new * wos * K <= logits_len - lg),
                    "%s: stream %d: logits [%ld, +%ld x %ld x %d) leave the buffer of %ld floats", who, s, lg, n_new, wos, K, logits_len);
        StreamRec& q = h[s];
        q.logit_off = lg; q.n_new = (int)n_new; q.w_first = (int)w_first; q.win_out_s = (int)wos; q.end = (int)end;
        q.n_out = (int)now; q.n_win = (int)n_win; q.last_start = (int)last_start; q.prob_off = (int)poff;
        q.F_prev = (int)(prev > win_out ? prev - win_out : 0);
        q.F_now = (int)(end ? now : (now > win_out ? now - win_out : 0));
        q.G_prev = q.F_prev > r ? q.F_prev - r : 0;
        q.G_now = end ? (int)now : (q.F_now > r ? q.F_now - r : 0);
        // everything still read is inside the rings
        const long w_lo = q.F_prev >= win_out ? (q.F_prev - win_out) / hop_out + 1 : 0;
        SED_REQUIRE(w_first + n_new - w_lo <= d.WR, "%s: stream %d: %ld live windows, the ring holds %d", who, s, w_first + n_new - w_lo, d.WR);
        SED_REQUIRE(q.F_now - (q.G_prev > r ? q.G_prev - r : 0) <= d.TR, "%s: stream %d: %d live track frames, the ring holds %d", who, s,
                    q.F_now - (q.G_prev > r ? q.G_prev - r : 0), d.TR);
        SED_REQUIRE(q.G_now - q.G_prev <= max_new_decided, "%s: stream %d decides %d frames, max_new_decided=%d", who, s,
                    q.G_now - q.G_prev, max_new_decided);
        SED_REQUIRE(!probs || (poff >= 0 && poff + (q.F_now - q.F_prev) <= probs_rows && poff <= 0x7fffffffL),
                    "%s: stream %d: its %d new rows at %ld leave probs [%ld]", who, s, q.F_now - q.F_prev, poff, probs_rows);
        most_new = n_new * wos * K > most_new ? n_new * wos * K : most_new;
        most_df = (long)(q.F_now - q.F_prev) * K > most_df ? (long)(q.F_now - q.F_prev) * K : most_df;
        most_dg = (long)(q.G_now - q.G_prev) * K > most_dg ? (long)(q.G_now - q.G_prev) * K : most_dg;
    }
    hipStream_t st = as_stream(stream);
    char* p = (char*)workspace;
    StreamRec* recs = (StreamRec*)p; p += st_al((size_t)S * sizeof(StreamRec));
    int* counts = (int*)p; p += st_al((size_t)S * K * 4);
    int* offs = (int*)p; p += st_al((size_t)S * K * 4);
    float* filt = (float*)p;
    SED_TRY(detect_upload(who, recs, h.data(), (size_t)S * sizeof(StreamRec), st));
    float* ring = (float*)state;
    float* track = (float*)((char*)state + d.track_off);
    DecState* dec = (DecState*)((char*)state + d.dec_off);
    const int slot = (int)d.slot;
    auto blocks = [](long n) { const long b = (n + 255) / 256; return (unsigned)(b < 256 ? b : 256); };
    if (most_new) {
        stream_store_k<<<dim3(blocks(most_new), (unsigned)S), 256, 0, st>>>(logits, recs, ring, d.WR, slot, K);
        SED_LAUNCH_CHECK("stream_store");
    }
    if (most_df) {
        stream_stitch_k<<<dim3(blocks(most_df), (unsigned)S), 256, 0, st>>>(recs, ring, d.WR, slot, K, win_out, hop_out, combine, trim,
                                                                           track, d.TR, probs);
        SED_LAUNCH_CHECK("stream_stitch");
    }
    if (most_dg) {
        if (tab) {
            detect_for_widths(*tab, K, [&](auto m, const ClassList& list) {
                stream_median_cw_k<decltype(m)::value><<<dim3(blocks(most_dg / K * list.n), (unsigned)S), 256, 0, st>>>(
                    recs, track, d.TR, K, max_new_decided, list, filt);
            });
        } else {
            detect_with_median(median, [&](auto m) {
                stream_median_k<decltype(m)::value><<<dim3(blocks(most_dg), (unsigned)S), 256, 0, st>>>(recs, track, d.TR, K, max_new_decided, filt);
            });
        }
        SED_LAUNCH_CHECK("stream_median");
    }
    const unsigned wb = (unsigned)cdiv((long)S * K, 256);
    if (tab)
        stream_walk_cw_k<false><<<wb, 256, 0, st>>>(recs, filt, track, d.TR, S, K, max_new_decided, *tab, dec, counts, offs, max_events,
                                                   ev_stream, cls, onset, offset, peak, peak_frame);
    else
        stream_walk_k<false><<<wb, 256, 0, st>>>(recs, filt, track, d.TR, S, K, max_new_decided, lo, hi, min_gap, min_len, dec, counts, offs,
                                                max_events, ev_stream, cls, onset, offset, peak, peak_frame);
    SED_LAUNCH_CHECK("stream_walk(count)");
    detect_scan_k<<<1, 1024, 0, st>>>(counts, S * K, K, offs, event_off);
    SED_LAUNCH_CHECK("stream_scan");
    if (tab)
        stream_walk_cw_k<true><<<wb, 256, 0, st>>>(recs, filt, track, d.TR, S, K, max_new_decided, *tab, dec, counts, offs, max_events,
                                                  ev_stream, cls, onset, offset, peak, peak_frame);
    else
        stream_walk_k<true><<<wb, 256, 0, st>>>(recs, filt, track, d.TR, S, K, max_new_decided, lo, hi, min_gap, min_len, dec, counts, offs,
                                               max_events, ev_stream, cls, onset, offset, peak, peak_frame);
    SED_LAUNCH_CHECK("stream_walk(write)");
    return 0;
}

extern "C" int sed_stream_step(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median, int max_new_windows,
                               int combine, int trim, float lo, float hi, int min_gap, int min_len, const float* logits,
                               long logits_len, const long* table_host, int max_new_decided, float* probs, long probs_rows,
                               int max_events, int* ev_stream, int* cls, int* onset, int* offset, float* peak, int* peak_frame,
                               int* event_off, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(state && table_host && event_off && workspace, "stream_step: null pointer");
    return stream_step_impl("stream_step", nullptr, state, state_bytes, S, K, win_out, hop_out, median, max_new_windows, combine, trim, lo,
                            hi, min_gap, min_len, logits, logits_len, table_host, max_new_decided, probs, probs_rows, max_events, ev_stream,
                            cls, onset, offset, peak, peak_frame, event_off, workspace, workspace_bytes, stream);
}

// sed_stream_step with class-wise settings (classes_host [K]).  `median` is the width the state was sized with and must
// be the widest of the K classes: ONE frontier per feed, filtered frame g of every class decided once track frame g + median/2 is
// final.  A refusal (a bad class row included) comes before any launch, so the state is left as it was.
extern "C" int sed_stream_step_classwise(void* state, size_t state_bytes, int S, int K, int win_out, int hop_out, int median,
                                         int max_new_windows, int combine, int trim, const sed_tune_setting* classes_host,
                                         const float* logits, long logits_len, const long* table_host, int max_new_decided, float* probs,
                                         long probs_rows, int max_events, int* ev_stream, int* cls, int* onset, int* offset, float* peak,
                                         int* peak_frame, int* event_off, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(state && classes_host && table_host && event_off && workspace, "stream_step_classwise: null pointer");
    SED_REQUIRE(K >= 1 && K <= 32, "stream_step_classwise: bad sizes (K=%d in 1..32)", K);
    ClassTable tab;
    int widest;
    SED_TRY(detect_class_table("stream_step_classwise", classes_host, K, tab, &widest));
    SED_REQUIRE(median == widest, "stream_step_classwise: median=%d must be the widest median of the classes (%d): the state is sized with it",
                median, widest);
    return stream_step_impl("stream_step_classwise", &tab, state, state_bytes, S, K, win_out, hop_out, median, max_new_windows, combine,
                            trim, 0.f, 0.f, 0, 1, logits, logits_len, table_host, max_new_decided, probs, probs_rows, max_events,
                            ev_stream, cls, onset, offset, peak, peak_frame, event_off, workspace, workspace_bytes, stream);
}
