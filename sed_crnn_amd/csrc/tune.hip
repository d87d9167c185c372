// tune.hip — the decoder sweep (sed_crnn_amd/tune.py): for a whole grid of decoder settings (median, lo, hi, min_gap,
// min_len), the events sed_detect_events_batch would produce on a packed track are scored against reference events WITHOUT being
// written: event-based matches (onset / offset collar) and per-recording segment-based block counts, summed over recordings into
// counts [G][K][6] = (ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref), int64.  Integer work throughout: exact and repeatable.
//
//   1. detect_bits_seg_k<M> of detect_shared.h — the bit-track kernel of sed_detect_events_batch — with a list of thresholds,
//      one launch per distinct median width: the track is filtered once per width and one bit track is packed per distinct
//      (width, threshold value); lo and hi of every setting index into that pool.
//   2. tune_refblocks_k of tune_shared.h: per (recording, class) the prefix count of reference-active blocks, P[b] = active
//      blocks before block b.
//   3. tune_walk_k, one wave per (setting, class, group of recordings): detect_walk_body of detect_shared.h — the walk of
//      detect_walk_k — whose finished events go through the matcher and the block counter instead of being stored; the wave sums
//      its recordings in registers and adds six integers to counts[g][k] at the end.
#include <vector>
#include "common.h"
#include "detect_shared.h"
#include "tune_shared.h"

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

// the workspace is tune_shared.h's: the offset tables, the settings, the thresholds, the block prefix counts, the bit tracks
extern "C" size_t sed_tune_workspace_bytes(long n_total, int K, int R, int n_tracks, int G) {
    return tune_workspace_bytes(n_total, K, R, n_tracks, G);
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
    TunePool pool;                                                    // distinct (median, threshold value) -> one bit track
    SED_TRY(tune_track_pool("tune_sweep", settings_host, G, pool));
    const int n_tracks = pool.n_tracks;

    const size_t need = sed_tune_workspace_bytes(rows, K, R, n_tracks, G);
    SED_REQUIRE(need > 0, "tune_sweep: bad sizes (R=%d, K=%d, %ld output frames, G=%d)", R, K, rows, G);
    SED_REQUIRE(workspace, "tune_sweep: null pointer (workspace)");
    SED_REQUIRE(workspace_bytes >= need, "tune_sweep: workspace of %zu bytes, %zu needed (%d bit tracks)", workspace_bytes, need, n_tracks);
    SED_REQUIRE(probs && ref_off && ref_onset && ref_offset && ref_tol && counts, "tune_sweep: null pointer");
    const int RS = (R + TUNE_REC_PER_WAVE - 1) / TUNE_REC_PER_WAVE;
    SED_REQUIRE((long)G * K * RS <= 0x7fffffffL, "tune_sweep: G*K*R = %d*%d*%d is too large for one call", G, K, R);

    const TuneWorkspace w = tune_carve(workspace, rows, K, R, n_tracks, G);
    const size_t track_words = (size_t)K * words;                     // words <= rows/64 + R: inside the workspace

    hipStream_t s = as_stream(stream);
    SED_TRY(detect_upload("tune_sweep", w.out_off, h.data(), h.size() * 4, s));
    SED_TRY(detect_upload("tune_sweep", w.sets, pool.sets.data(), pool.sets.size() * sizeof(TuneSet), s));
    SED_TRY(detect_upload("tune_sweep", w.thr, pool.thr.data(), pool.thr.size() * 4, s));
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)G * K * 6 * sizeof(long), s);
    if (e != hipSuccess) { sed_set_error("tune_sweep: clearing counts: %s", hipGetErrorString(e)); return (int)e; }
    for (size_t m = 0; m < pool.med_of.size(); ++m) {
        launch_bits_seg(pool.med_of[m], probs, w.out_off, w.word_off, R, K, words, ThresholdList{w.thr + pool.first[m], pool.n_thr[m]},
                        track_words, w.bits + (size_t)pool.first[m] * track_words, s);
        SED_LAUNCH_CHECK("tune_bits");
    }
    tune_refblocks_k<<<(unsigned)((long)R * K), 64, 0, s>>>(w.out_off, w.blk_off, K, block, ref_off, ref_onset, ref_offset, w.P);
    SED_LAUNCH_CHECK("tune_refblocks");
    tune_walk_k<<<(unsigned)((long)G * K * RS), 64, 0, s>>>(w.bits, track_words, w.sets, w.word_off, w.blk_off, R, K, RS, ref_off,
                                                           ref_onset, ref_offset, ref_tol, w.P, collar, block,
                                                           (unsigned long long*)counts);
    SED_LAUNCH_CHECK("tune_walk");
    return 0;
}
