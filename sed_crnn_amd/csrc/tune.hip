// tune.hip — the decoder sweep (sed_crnn_amd/tune.py): for a whole grid of decoder settings (median, lo, hi, min_gap,
// min_len), the events sed_detect_events_batch would produce on a packed track are scored against reference events WITHOUT being
// written: event-based matches (onset / offset collar) and per-recording segment-based block counts, summed over recordings into
// counts [G][K][6] = (ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref), int64.  Integer work throughout: exact and repeatable.
//
//   1. detect_bits_seg_k<M> of detect_shared.h — the bit-track kernel of sed_detect_events_batch — with a list of thresholds,
//      one launch per distinct median width: the track is filtered once per width and one bit track is packed per distinct
//      (width, threshold value); lo and hi of every setting index into that pool.
//   2. tune_refblocks_k: per (recording, class) the prefix count of reference-active blocks, P[b] = active blocks before block b.
//   3. tune_walk_k, one wave per (setting, class, group of recordings): detect_walk_body of detect_shared.h — the walk of
//      detect_walk_k — whose finished events go through the matcher and the block counter instead of being stored; the wave sums
//      its recordings in registers and adds six integers to counts[g][k] at the end.
#include <vector>
#include "common.h"
#include "detect_shared.h"

// One wave per (recording, class).  Block b = frames [b block, (b+1) block) is reference-active when a reference event covers one
// of its frames: the events are sorted and disjoint, so that is the first event whose offset lies beyond the block's start.
// P [n_blk + 1] at K*blk_off[r] + k*(n_blk + 1): exclusive prefix counts, P[n_blk] = the number of active blocks.
__global__ __launch_bounds__(64) void tune_refblocks_k(const int* __restrict__ out_off, const int* __restrict__ blk_off, int K, int block,
                                                       const int* __restrict__ ref_off, const int* __restrict__ ref_onset,
                                                       const int* __restrict__ ref_offset, int* __restrict__ P) {
    const int lane = threadIdx.x, r = (int)blockIdx.x / K, k = (int)blockIdx.x - r * K;
    const int n_out = out_off[r + 1] - out_off[r];
    const int n_blk = blk_off[r + 1] - blk_off[r] - 1;
    int* p = P + (size_t)K * blk_off[r] + (size_t)k * (n_blk + 1);
    const int j0 = ref_off[blockIdx.x], j1 = ref_off[blockIdx.x + 1];
    int carry = 0;
    for (int b0 = 0; b0 < n_blk; b0 += 64) {
        const int b = b0 + lane;
        int act = 0;
        if (b < n_blk) {
            const long start = (long)b * block;
            long end = start + block;
            if (end > n_out) end = n_out;
            int lo = j0, hi = j1;                                     // first event with offset > start
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (ref_offset[mid] > start) hi = mid;
                else lo = mid + 1;
            }
            act = lo < j1 && ref_onset[lo] < end;
        }
        int x = act;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (b < n_blk) p[b] = carry + x - act;
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) p[n_blk] = carry;
}

// a setting on the device: which bit tracks it reads and the constants of its walk
struct TuneSet { int lo_track, hi_track, min_gap, min_len; };

// What lane 0 does with every finished event of one (setting, recording, class): the matcher and the block counter.  The first
// TUNE_REF_LDS reference events and TUNE_P_LDS block prefix counts of the (recording, class) are staged in LDS by the whole wave
// (lane 0's walk is serial: a dependent global load per step would be its whole cost); what lies beyond is read from memory.
#define TUNE_REF_LDS 64
#define TUNE_P_LDS 512
struct TuneEmit {
    const int *ron, *roff, *rtol, *P;            // reference events (global indices) and the block prefix of this (r, k)
    const int *s_on, *s_off, *s_tol, *s_P;       // their staged heads
    int j0;                                      // first reference event of this (r, k) = s_on[0]
    int jp, j1;                                  // first reference event that can still match, one past the last
    unsigned long long matched;                  // bit i: reference event jp + i is taken (candidates span <= 2 collar + 1 <= 63)
    int collar, block, last_blk;
    long ev_tp, n_sys, seg_tp, seg_sys;
    __device__ __forceinline__ int on_of(int j) const { return j - j0 < TUNE_REF_LDS ? s_on[j - j0] : ron[j]; }
    __device__ __forceinline__ int off_of(int j) const { return j - j0 < TUNE_REF_LDS ? s_off[j - j0] : roff[j]; }
    __device__ __forceinline__ int tol_of(int j) const { return j - j0 < TUNE_REF_LDS ? s_tol[j - j0] : rtol[j]; }
    __device__ __forceinline__ int P_of(int b) const { return b < TUNE_P_LDS ? s_P[b] : P[b]; }
    __device__ __forceinline__ void operator()(int on, int off) {
        ++n_sys;
        // onsets of the system events increase: a reference event left of on - collar is out of reach for good
        while (jp < j1 && on_of(jp) < on - collar) { ++jp; matched >>= 1; }
        for (int j = jp; j < j1 && on_of(j) <= on + collar; ++j) {
            if ((matched >> (j - jp)) & 1ull) continue;
            const int tol = tol_of(j);
            const int d = off - off_of(j);
            if (tol >= 0 && (d < 0 ? -d : d) > tol) continue;
            matched |= 1ull << (j - jp);
            ++ev_tp;
            break;
        }
        // events arrive sorted and disjoint: the blocks covered so far are [0, last_blk] as far as later events can tell
        const int b1 = (off - 1) / block;
        int b0 = on / block;
        if (b0 <= last_blk) b0 = last_blk + 1;
        if (b0 <= b1) {
            seg_sys += b1 - b0 + 1;
            seg_tp += P_of(b1 + 1) - P_of(b0);
            last_blk = b1;
        }
    }
};

#define TUNE_REC_PER_WAVE 8
// workgroup (one wave) = (g, k, rs): recordings rs, rs + RS, ... of setting g and class k
__global__ __launch_bounds__(64) void tune_walk_k(const unsigned long long* __restrict__ bits, size_t track_words,
                                                  const TuneSet* __restrict__ sets, const int* __restrict__ word_off,
                                                  const int* __restrict__ blk_off, int R, int K, int RS,
                                                  const int* __restrict__ ref_off, const int* __restrict__ ref_onset,
                                                  const int* __restrict__ ref_offset, const int* __restrict__ ref_tol,
                                                  const int* __restrict__ P, int collar, int block,
                                                  unsigned long long* __restrict__ counts) {
    __shared__ int epos[DETECT_EDGE_CAP], eh[DETECT_EDGE_CAP];
    __shared__ int s_on[TUNE_REF_LDS], s_off[TUNE_REF_LDS], s_tol[TUNE_REF_LDS], s_P[TUNE_P_LDS];
    const int lane = threadIdx.x;
    const int rs = (int)(blockIdx.x % RS);
    const int gk = (int)(blockIdx.x / RS);
    const int g = gk / K, k = gk - g * K;
    const TuneSet st = sets[g];
    const unsigned long long* lo_t = bits + (size_t)st.lo_track * track_words;
    const unsigned long long* hi_t = bits + (size_t)st.hi_track * track_words;
    long ev_tp = 0, n_sys = 0, n_ref = 0, seg_tp = 0, seg_sys = 0, seg_ref = 0;      // lane 0's sums
    for (int r = rs; r < R; r += RS) {
        const int nw = word_off[r + 1] - word_off[r];
        const size_t at = (size_t)K * word_off[r] + (size_t)k * nw;
        const int n_blk = blk_off[r + 1] - blk_off[r] - 1;
        const int* p = P + (size_t)K * blk_off[r] + (size_t)k * (n_blk + 1);
        const int j0 = ref_off[r * K + k], j1 = ref_off[r * K + k + 1];
        if (j0 + lane < j1) {                                         // TUNE_REF_LDS == the wave's 64 lanes
            s_on[lane] = ref_onset[j0 + lane]; s_off[lane] = ref_offset[j0 + lane]; s_tol[lane] = ref_tol[j0 + lane];
        }
        for (int b = lane; b <= n_blk && b < TUNE_P_LDS; b += 64) s_P[b] = p[b];
        // (the walk's first barrier comes before lane 0 emits anything: nw >= 1)
        TuneEmit emit{ref_onset, ref_offset, ref_tol, p, s_on, s_off, s_tol, s_P, j0, j0, j1, 0ull, collar, block, -1, 0, 0, 0, 0};
        detect_walk_body(lo_t + at, hi_t + at, nw, st.min_gap, st.min_len, epos, eh, emit);
        __syncthreads();                                              // lane 0's last emit is done before the next staging
        ev_tp += emit.ev_tp; n_sys += emit.n_sys; seg_tp += emit.seg_tp; seg_sys += emit.seg_sys;
        n_ref += j1 - j0;
        seg_ref += p[n_blk];
    }
    if (threadIdx.x == 0) {
        unsigned long long* c = counts + ((size_t)g * K + k) * 6;
        atomicAdd(c + 0, (unsigned long long)ev_tp);
        atomicAdd(c + 1, (unsigned long long)n_sys);
        atomicAdd(c + 2, (unsigned long long)n_ref);
        atomicAdd(c + 3, (unsigned long long)seg_tp);
        atomicAdd(c + 4, (unsigned long long)seg_sys);
        atomicAdd(c + 5, (unsigned long long)seg_ref);
    }
}

// workspace (16-byte aligned regions): out_off, word_off, blk_off [R+1] each (one upload); the settings [G]; the thresholds
// [n_tracks]; the block prefix counts, at most K (n_total + R) ints (block >= 1); then n_tracks bit tracks of K words each,
// words <= n_total/64 + R
#define TUNE_MAX_G (1 << 20)

extern "C" size_t sed_tune_workspace_bytes(long n_total, int K, int R, int n_tracks, int G) {
    if (R < 1 || n_total < R || n_total > 0x7fffffffL || K < 1 || K > 32 || n_total * K > 0x7fffffffL) return 0;
    if (G < 1 || G > TUNE_MAX_G || n_tracks < 1 || n_tracks > 2 * (long)G) return 0;
    if (n_total / 64 + R > 0x7fffffffL) return 0;
    const size_t words = (size_t)(n_total / 64 + R);
    return al16((size_t)3 * (R + 1) * 4) + al16((size_t)G * sizeof(TuneSet)) + al16((size_t)n_tracks * 4) +
           al16((size_t)K * ((size_t)n_total + R) * 4) + (size_t)n_tracks * K * words * sizeof(unsigned long long);
}

extern "C" int sed_tune_sweep(const float* probs, const long* n_out_host, int R, int K, const sed_tune_setting* settings_host, int G,
                              const int* ref_off, const int* ref_onset, const int* ref_offset, const int* ref_tol, int collar,
                              int block, void* workspace, size_t workspace_bytes, long* counts, void* stream) {
    SED_REQUIRE(R >= 1 && K >= 1 && K <= 32, "tune_sweep: bad sizes (R=%d, K=%d in 1..32)", R, K);
    SED_REQUIRE(G >= 0 && G <= TUNE_MAX_G, "tune_sweep: G=%d settings (0..%d in one call)", G, TUNE_MAX_G);
    SED_REQUIRE(collar >= 0 && collar <= 31, "tune_sweep: collar must be in 0..31 output frames (got %d)", collar);
    SED_REQUIRE(block >= 1, "tune_sweep: block must be >= 1 output frame (got %d)", block);
    SED_REQUIRE(n_out_host, "tune_sweep: null pointer (n_out_host)");
    std::vector<int> h(3 * (size_t)(R + 1));
    int *out_off = h.data(), *word_off = out_off + R + 1, *blk_off = word_off + R + 1;
    long rows, words, blks = 0;
    SED_TRY(detect_seg_tables("tune_sweep", n_out_host, R, K, out_off, word_off, &rows, &words));
    for (int r = 0; r < R; ++r) {
        blk_off[r] = (int)blks;
        blks += (n_out_host[r] + block - 1) / block + 1;              // n_blk + 1 prefix counts
    }
    blk_off[R] = (int)blks;
    if (G == 0) return 0;
    SED_REQUIRE(settings_host, "tune_sweep: null pointer (settings_host)");
    // the pool of bit tracks: distinct (median, threshold value), grouped by median in order of first appearance
    std::vector<int> med_of;                                          // distinct medians
    std::vector<std::vector<float>> thr_of;                           // their distinct thresholds
    std::vector<int> lo_m(G), lo_i(G), hi_i(G);
    for (int g = 0; g < G; ++g) {
        const sed_tune_setting& t = settings_host[g];
        SED_TRY(detect_check_decoder("tune_sweep", g, t.median, t.lo, t.hi, t.min_gap, t.min_len));
        size_t m = 0;
        while (m < med_of.size() && med_of[m] != t.median) ++m;
        if (m == med_of.size()) { med_of.push_back(t.median); thr_of.emplace_back(); }
        auto slot = [&](float v) {
            std::vector<float>& th = thr_of[m];
            size_t i = 0;
            while (i < th.size() && !(th[i] == v)) ++i;
            if (i == th.size()) th.push_back(v);
            return (int)i;
        };
        lo_m[g] = (int)m;
        lo_i[g] = slot(t.lo);
        hi_i[g] = slot(t.hi);
    }
    std::vector<int> first(med_of.size() + 1, 0);
    for (size_t m = 0; m < med_of.size(); ++m) first[m + 1] = first[m] + (int)thr_of[m].size();
    const int n_tracks = first.back();
    std::vector<float> thr(n_tracks);
    for (size_t m = 0; m < med_of.size(); ++m)
        for (size_t i = 0; i < thr_of[m].size(); ++i) thr[first[m] + i] = thr_of[m][i];
    std::vector<TuneSet> sets(G);
    for (int g = 0; g < G; ++g)
        sets[g] = TuneSet{first[lo_m[g]] + lo_i[g], first[lo_m[g]] + hi_i[g], settings_host[g].min_gap, settings_host[g].min_len};

    const size_t need = sed_tune_workspace_bytes(rows, K, R, n_tracks, G);
    SED_REQUIRE(need > 0, "tune_sweep: bad sizes (R=%d, K=%d, %ld output frames, G=%d)", R, K, rows, G);
    SED_REQUIRE(workspace, "tune_sweep: null pointer (workspace)");
    SED_REQUIRE(workspace_bytes >= need, "tune_sweep: workspace of %zu bytes, %zu needed (%d bit tracks)", workspace_bytes, need, n_tracks);
    SED_REQUIRE(probs && ref_off && ref_onset && ref_offset && ref_tol && counts, "tune_sweep: null pointer");
    const int RS = (R + TUNE_REC_PER_WAVE - 1) / TUNE_REC_PER_WAVE;
    SED_REQUIRE((long)G * K * RS <= 0x7fffffffL, "tune_sweep: G*K*R = %d*%d*%d is too large for one call", G, K, R);

    char* p = (char*)workspace;
    int* d_off = (int*)p; p += al16((size_t)3 * (R + 1) * 4);
    TuneSet* d_sets = (TuneSet*)p; p += al16((size_t)G * sizeof(TuneSet));
    float* d_thr = (float*)p; p += al16((size_t)n_tracks * 4);
    int* d_P = (int*)p; p += al16((size_t)K * ((size_t)rows + R) * 4);
    unsigned long long* d_bits = (unsigned long long*)p;
    const int *d_out_off = d_off, *d_word_off = d_off + R + 1, *d_blk_off = d_off + 2 * (R + 1);
    const size_t track_words = (size_t)K * words;                     // words <= rows/64 + R: inside the workspace

    hipStream_t s = as_stream(stream);
    SED_TRY(detect_upload("tune_sweep", d_off, h.data(), h.size() * 4, s));
    SED_TRY(detect_upload("tune_sweep", d_sets, sets.data(), sets.size() * sizeof(TuneSet), s));
    SED_TRY(detect_upload("tune_sweep", d_thr, thr.data(), thr.size() * 4, s));
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)G * K * 6 * sizeof(long), s);
    if (e != hipSuccess) { sed_set_error("tune_sweep: clearing counts: %s", hipGetErrorString(e)); return (int)e; }
    for (size_t m = 0; m < med_of.size(); ++m) {
        launch_bits_seg(med_of[m], probs, d_out_off, d_word_off, R, K, words, ThresholdList{d_thr + first[m], (int)thr_of[m].size()},
                        track_words, d_bits + (size_t)first[m] * track_words, s);
        SED_LAUNCH_CHECK("tune_bits");
    }
    tune_refblocks_k<<<(unsigned)((long)R * K), 64, 0, s>>>(d_out_off, d_blk_off, K, block, ref_off, ref_onset, ref_offset, d_P);
    SED_LAUNCH_CHECK("tune_refblocks");
    tune_walk_k<<<(unsigned)((long)G * K * RS), 64, 0, s>>>(d_bits, track_words, d_sets, d_word_off, d_blk_off, R, K, RS, ref_off,
                                                           ref_onset, ref_offset, ref_tol, d_P, collar, block,
                                                           (unsigned long long*)counts);
    SED_LAUNCH_CHECK("tune_walk");
    return 0;
}
