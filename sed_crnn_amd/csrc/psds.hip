// psds.hip — the intersection criteria of the polyphonic sound detection score (sed_crnn_amd/tune.py): for a whole
// grid of decoder settings, the events sed_detect_events_batch would produce on a packed track are judged against reference
// events by how much of them INTERSECTS the reference, WITHOUT being written, and summed over recordings into
// counts [G][K][4] = (tp, n_ref, n_sys, fp) and, with a cross-trigger criterion, ct [G][K][K], int64.  Criteria in thousandths,
// every comparison a 64-bit integer one: exact and repeatable.
//
//   1. detect_bits_seg_k<M> of detect_shared.h with a list of thresholds, one launch per distinct median width: the pool of bit
//      tracks of tune_shared.h, the one sed_tune_sweep packs.
//   2. tune_refblocks_k of tune_shared.h with block = 1: per (recording, class) the prefix A[t] = frames before t that a
//      reference event of the class covers, so |[a, b) ∩ G_c| = A_c[b] - A_c[a] for any class c.
//   3. psds_walk_k, one wave per (setting, class, group of recordings): detect_walk_body of detect_shared.h — the walk of
//      detect_walk_k — whose finished events go through PsdsEmit; the wave sums its recordings and adds 4 (+K) integers at the end.
#include <vector>
#include "common.h"
#include "detect_shared.h"
#include "tune_shared.h"

// What lane 0 does with every finished event [on, off) of one (setting, recording, class k).  The first PSDS_REF_LDS reference
// events of the (recording, class) are staged in LDS by the whole wave (lane 0's walk is serial: a dependent global load per
// step would be its whole cost); what lies beyond is read from memory.
//   relevant (1000 |d ∩ G_k| >= dtc |d|): merge walk over the class-k reference list.  Detections and reference events are each
//   sorted and disjoint, so only the last reference event a detection touches can be touched by a later one: ONE open coverage
//   sum and a pointer are the whole state; a reference event is finalised (the gtc test) when the pointer leaves it.
//   not relevant: a false positive and, when CT, a cross trigger on every other class c with 1000 |d ∩ G_c| >= cttc |d|.
#define PSDS_REF_LDS 64
template <bool CT>
struct PsdsEmit {
    const int *ron, *roff;                       // reference events (global indices)
    const int *s_on, *s_off;                     // their staged heads
    const int* A;                                // the K frame prefixes of this recording, class c at A + c (n_out + 1)
    int* s_ct;                                   // the wave's cross-trigger row (LDS, K ints)
    int j0, jp, j1;                              // first reference event of this (r, k), the open one, one past the last
    int k, K, stride;                            // stride = n_out + 1
    int dtc, gtc, cttc;
    long cov;                                    // frames of reference event jp covered by relevant detections so far
    long tp, n_sys, fp;
    __device__ __forceinline__ int on_of(int j) const { return j - j0 < PSDS_REF_LDS ? s_on[j - j0] : ron[j]; }
    __device__ __forceinline__ int off_of(int j) const { return j - j0 < PSDS_REF_LDS ? s_off[j - j0] : roff[j]; }
    // the pointer leaves reference event jp = [a, b)
    __device__ __forceinline__ void finalise(int a, int b) {
        if (1000L * cov >= (long)gtc * (b - a)) ++tp;
        cov = 0;
        ++jp;
    }
    __device__ __forceinline__ void operator()(int on, int off) {
        ++n_sys;
        const long len = off - on;
        const int* Ak = A + (size_t)k * stride;
        if (1000L * (Ak[off] - Ak[on]) >= (long)dtc * len) {
            while (jp < j1) {
                const int a = on_of(jp), b = off_of(jp);
                if (a >= off) break;                                  // a later detection may still reach it
                if (b > on) cov += (b < off ? b : off) - (a > on ? a : on);
                if (b > off) break;                                   // open: the next detection may cover more of it
                finalise(a, b);
            }
            return;
        }
        ++fp;
        if (CT) {
            for (int c = 0; c < K; ++c) {
                if (c == k) continue;
                const int* Ac = A + (size_t)c * stride;
                if (1000L * (Ac[off] - Ac[on]) >= (long)cttc * len) ++s_ct[c];
            }
        }
    }
    // after the walk: the open reference event; the ones behind it were touched by no relevant detection (gtc >= 1: no tp)
    __device__ __forceinline__ void finish() {
        if (jp < j1) finalise(on_of(jp), off_of(jp));
    }
};

// workgroup (one wave) = (g, k, rs): recordings rs, rs + RS, ... of setting g and class k (the grid of tune_walk_k)
template <bool CT>
__global__ __launch_bounds__(64) void psds_walk_k(const unsigned long long* __restrict__ bits, size_t track_words,
                                                  const TuneSet* __restrict__ sets, const int* __restrict__ word_off,
                                                  const int* __restrict__ blk_off, int R, int K, int RS,
                                                  const int* __restrict__ ref_off, const int* __restrict__ ref_onset,
                                                  const int* __restrict__ ref_offset, const int* __restrict__ P, int dtc, int gtc,
                                                  int cttc, unsigned long long* __restrict__ counts,
                                                  unsigned long long* __restrict__ ct) {
    __shared__ int epos[DETECT_EDGE_CAP], eh[DETECT_EDGE_CAP];
    __shared__ int s_on[PSDS_REF_LDS], s_off[PSDS_REF_LDS], s_ct[32];
    const int lane = threadIdx.x;
    const int rs = (int)(blockIdx.x % RS);
    const int gk = (int)(blockIdx.x / RS);
    const int g = gk / K, k = gk - g * K;
    const TuneSet st = sets[g];
    const unsigned long long* lo_t = bits + (size_t)st.lo_track * track_words;
    const unsigned long long* hi_t = bits + (size_t)st.hi_track * track_words;
    if (CT && lane < 32) s_ct[lane] = 0;
    long tp = 0, n_ref = 0, n_sys = 0, fp = 0;                        // lane 0's sums
    for (int r = rs; r < R; r += RS) {
        const int nw = word_off[r + 1] - word_off[r];
        const size_t at = (size_t)K * word_off[r] + (size_t)k * nw;
        const int stride = blk_off[r + 1] - blk_off[r];               // n_out + 1 prefix counts per class
        const int j0 = ref_off[r * K + k], j1 = ref_off[r * K + k + 1];
        if (j0 + lane < j1) {                                         // PSDS_REF_LDS == the wave's 64 lanes
            s_on[lane] = ref_onset[j0 + lane]; s_off[lane] = ref_offset[j0 + lane];
        }
        // (the walk's first barrier comes before lane 0 emits anything: nw >= 1)
        PsdsEmit<CT> emit{ref_onset, ref_offset, s_on, s_off, P + (size_t)K * blk_off[r], s_ct, j0, j0, j1, k, K, stride,
                          dtc, gtc, cttc, 0, 0, 0, 0};
        detect_walk_body(lo_t + at, hi_t + at, nw, st.min_gap, st.min_len, epos, eh, emit);
        if (lane == 0) emit.finish();
        __syncthreads();                                              // lane 0 is done with the staged events before the next staging
        tp += emit.tp; n_sys += emit.n_sys; fp += emit.fp;
        n_ref += j1 - j0;
    }
    if (lane == 0) {
        unsigned long long* c = counts + ((size_t)g * K + k) * 4;
        atomicAdd(c + 0, (unsigned long long)tp);
        atomicAdd(c + 1, (unsigned long long)n_ref);
        atomicAdd(c + 2, (unsigned long long)n_sys);
        atomicAdd(c + 3, (unsigned long long)fp);
        if (CT) {
            unsigned long long* row = ct + ((size_t)g * K + k) * K;
            for (int c2 = 0; c2 < K; ++c2)
                if (s_ct[c2]) atomicAdd(row + c2, (unsigned long long)s_ct[c2]);
        }
    }
}

extern "C" size_t sed_psds_workspace_bytes(long n_total, int K, int R, int n_tracks, int G) {
    return tune_workspace_bytes(n_total, K, R, n_tracks, G);          // the prefix is per frame: all K (n_total + R) ints of it
}

extern "C" int sed_psds_sweep(const float* probs, const long* n_out_host, int R, int K, const sed_tune_setting* settings_host, int G,
                              const int* ref_off, const int* ref_onset, const int* ref_offset, int dtc_milli, int gtc_milli,
                              int cttc_milli, void* workspace, size_t workspace_bytes, long* counts, long* ct, void* stream) {
    SED_REQUIRE(R >= 1 && K >= 1 && K <= 32, "psds_sweep: bad sizes (R=%d, K=%d in 1..32)", R, K);
    SED_REQUIRE(G >= 0 && G <= TUNE_MAX_G, "psds_sweep: G=%d settings (0..%d in one call)", G, TUNE_MAX_G);
    SED_REQUIRE(dtc_milli >= 1 && dtc_milli <= 1000, "psds_sweep: dtc must be in 1..1000 thousandths (got %d)", dtc_milli);
    SED_REQUIRE(gtc_milli >= 1 && gtc_milli <= 1000, "psds_sweep: gtc must be in 1..1000 thousandths (got %d)", gtc_milli);
    SED_REQUIRE(cttc_milli >= 0 && cttc_milli <= 1000, "psds_sweep: cttc must be in 1..1000 thousandths, or 0 for no cross triggers (got %d)",
                cttc_milli);
    SED_REQUIRE(n_out_host, "psds_sweep: null pointer (n_out_host)");
    std::vector<int> h(3 * (size_t)(R + 1));
    int *out_off = h.data(), *word_off = out_off + R + 1, *blk_off = word_off + R + 1;
    long rows, words;
    SED_TRY(detect_seg_tables("psds_sweep", n_out_host, R, K, out_off, word_off, &rows, &words));
    for (int r = 0; r <= R; ++r) blk_off[r] = out_off[r] + r;         // n_out + 1 prefix counts per (recording, class)
    if (G == 0) return 0;
    SED_REQUIRE(settings_host, "psds_sweep: null pointer (settings_host)");
    TunePool pool;                                                    // distinct (median, threshold value) -> one bit track
    SED_TRY(tune_track_pool("psds_sweep", settings_host, G, pool));
    const int n_tracks = pool.n_tracks;

    const size_t need = sed_psds_workspace_bytes(rows, K, R, n_tracks, G);
    SED_REQUIRE(need > 0, "psds_sweep: bad sizes (R=%d, K=%d, %ld output frames, G=%d)", R, K, rows, G);
    SED_REQUIRE(workspace, "psds_sweep: null pointer (workspace)");
    SED_REQUIRE(workspace_bytes >= need, "psds_sweep: workspace of %zu bytes, %zu needed (%d bit tracks)", workspace_bytes, need, n_tracks);
    SED_REQUIRE(probs && ref_off && ref_onset && ref_offset && counts, "psds_sweep: null pointer");
    SED_REQUIRE(ct || cttc_milli == 0, "psds_sweep: null pointer (ct, with cttc=%d)", cttc_milli);
    const int RS = (R + TUNE_REC_PER_WAVE - 1) / TUNE_REC_PER_WAVE;
    SED_REQUIRE((long)G * K * RS <= 0x7fffffffL, "psds_sweep: G*K*R = %d*%d*%d is too large for one call", G, K, R);

    const TuneWorkspace w = tune_carve(workspace, rows, K, R, n_tracks, G);
    const size_t track_words = (size_t)K * words;                     // words <= rows/64 + R: inside the workspace

    hipStream_t s = as_stream(stream);
    SED_TRY(detect_upload("psds_sweep", w.out_off, h.data(), h.size() * 4, s));
    SED_TRY(detect_upload("psds_sweep", w.sets, pool.sets.data(), pool.sets.size() * sizeof(TuneSet), s));
    SED_TRY(detect_upload("psds_sweep", w.thr, pool.thr.data(), pool.thr.size() * 4, s));
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)G * K * 4 * sizeof(long), s);
    if (e == hipSuccess && cttc_milli) e = hipMemsetAsync(ct, 0, (size_t)G * K * K * sizeof(long), s);
    if (e != hipSuccess) { sed_set_error("psds_sweep: clearing counts: %s", hipGetErrorString(e)); return (int)e; }
    for (size_t m = 0; m < pool.med_of.size(); ++m) {
        launch_bits_seg(pool.med_of[m], probs, w.out_off, w.word_off, R, K, words, ThresholdList{w.thr + pool.first[m], pool.n_thr[m]},
                        track_words, w.bits + (size_t)pool.first[m] * track_words, s);
        SED_LAUNCH_CHECK("psds_bits");
    }
    tune_refblocks_k<<<(unsigned)((long)R * K), 64, 0, s>>>(w.out_off, w.blk_off, K, 1, ref_off, ref_onset, ref_offset, w.P);
    SED_LAUNCH_CHECK("psds_prefix");
    const unsigned n_wg = (unsigned)((long)G * K * RS);
    if (cttc_milli)
        psds_walk_k<true><<<n_wg, 64, 0, s>>>(w.bits, track_words, w.sets, w.word_off, w.blk_off, R, K, RS, ref_off, ref_onset, ref_offset,
                                              w.P, dtc_milli, gtc_milli, cttc_milli, (unsigned long long*)counts,
                                              (unsigned long long*)ct);
    else
        psds_walk_k<false><<<n_wg, 64, 0, s>>>(w.bits, track_words, w.sets, w.word_off, w.blk_off, R, K, RS, ref_off, ref_onset, ref_offset,
                                               w.P, dtc_milli, gtc_milli, 0, (unsigned long long*)counts, nullptr);
    SED_LAUNCH_CHECK("psds_walk");
    return 0;
}
