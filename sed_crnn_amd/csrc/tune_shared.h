// tune_shared.h — what the decoder sweep (tune.hip) and the PSDS sweep (psds.hip) share: the pool of bit
// tracks of a grid of settings (one track per distinct (median, threshold value), built on the host and packed by
// launch_bits_seg of detect_shared.h), the prefix kernel over the reference events and the workspace layout.  Both entries call
// the SAME functions, so the system events the PSDS criteria judge are the events the sweep scores.
#pragma once
#include <vector>
#include "common.h"
#include "detect_shared.h"

#define TUNE_MAX_G (1 << 20)
#define TUNE_REC_PER_WAVE 8

// a setting on the device: which bit tracks it reads and the constants of its walk
struct TuneSet { int lo_track, hi_track, min_gap, min_len; };

// The pool of bit tracks of G settings: distinct (median, threshold value), grouped by median in order of first appearance.
// med_of [n_med] the distinct medians, n_thr / first [n_med] how many tracks each has and where they start in thr [n_tracks];
// sets [G] index into the pool.
struct TunePool {
    std::vector<int> med_of, n_thr, first;
    std::vector<float> thr;
    std::vector<TuneSet> sets;
    int n_tracks = 0;
};

// settings_host [G] (non-NULL, G >= 1) -> pool; every setting is checked like the detector's five values
static int tune_track_pool(const char* entry, const sed_tune_setting* settings_host, int G, TunePool& pool) {
    std::vector<std::vector<float>> thr_of;                           // the distinct thresholds of every median
    std::vector<int> lo_m(G), lo_i(G), hi_i(G);
    for (int g = 0; g < G; ++g) {
        const sed_tune_setting& t = settings_host[g];
        SED_TRY(detect_check_decoder(entry, g, t.median, t.lo, t.hi, t.min_gap, t.min_len));
        size_t m = 0;
        while (m < pool.med_of.size() && pool.med_of[m] != t.median) ++m;
        if (m == pool.med_of.size()) { pool.med_of.push_back(t.median); thr_of.emplace_back(); }
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
    int at = 0;
    for (size_t m = 0; m < pool.med_of.size(); ++m) {
        pool.first.push_back(at);
        pool.n_thr.push_back((int)thr_of[m].size());
        pool.thr.insert(pool.thr.end(), thr_of[m].begin(), thr_of[m].end());
        at += (int)thr_of[m].size();
    }
    pool.n_tracks = at;
    pool.sets.resize(G);
    for (int g = 0; g < G; ++g)
        pool.sets[g] = TuneSet{pool.first[lo_m[g]] + lo_i[g], pool.first[lo_m[g]] + hi_i[g], settings_host[g].min_gap,
                               settings_host[g].min_len};
    return 0;
}

// workspace of both sweeps (16-byte aligned regions): out_off, word_off, blk_off [R+1] each (one upload); the settings [G]; the
// thresholds [n_tracks]; the prefix counts, at most K (n_total + R) ints (block >= 1); then n_tracks bit tracks of K words each,
// words <= n_total/64 + R.  0 = bad sizes.
static size_t tune_workspace_bytes(long n_total, int K, int R, int n_tracks, int G) {
    if (R < 1 || n_total < R || n_total > 0x7fffffffL || K < 1 || K > 32 || n_total * K > 0x7fffffffL) return 0;
    if (G < 1 || G > TUNE_MAX_G || n_tracks < 1 || n_tracks > 2 * (long)G) return 0;
    if (n_total / 64 + R > 0x7fffffffL) return 0;
    const size_t words = (size_t)(n_total / 64 + R);
    return al16((size_t)3 * (R + 1) * 4) + al16((size_t)G * sizeof(TuneSet)) + al16((size_t)n_tracks * 4) +
           al16((size_t)K * ((size_t)n_total + R) * 4) + (size_t)n_tracks * K * words * sizeof(unsigned long long);
}

// the regions of that workspace
struct TuneWorkspace {
    int *out_off, *word_off, *blk_off, *P;
    TuneSet* sets;
    float* thr;
    unsigned long long* bits;
};
static TuneWorkspace tune_carve(void* workspace, long rows, int K, int R, int n_tracks, int G) {
    char* p = (char*)workspace;
    TuneWorkspace w;
    w.out_off = (int*)p; w.word_off = w.out_off + R + 1; w.blk_off = w.out_off + 2 * (R + 1);
    p += al16((size_t)3 * (R + 1) * 4);
    w.sets = (TuneSet*)p; p += al16((size_t)G * sizeof(TuneSet));
    w.thr = (float*)p; p += al16((size_t)n_tracks * 4);
    w.P = (int*)p; p += al16((size_t)K * ((size_t)rows + R) * 4);
    w.bits = (unsigned long long*)p;
    return w;
}

// One wave per (recording, class).  Block b = frames [b block, (b+1) block) is reference-active when a reference event covers one
// of its frames: the events are sorted and disjoint, so that is the first event whose offset lies beyond the block's start.
// P [n_blk + 1] at K*blk_off[r] + k*(n_blk + 1): exclusive prefix counts, P[n_blk] = the number of active blocks.  With
// block = 1 (psds.hip) a block is a frame: P[t] = the frames before t that a reference event of the class covers.
static __global__ __launch_bounds__(64) void tune_refblocks_k(const int* __restrict__ out_off, const int* __restrict__ blk_off, int K,
                                                              int block, const int* __restrict__ ref_off,
                                                              const int* __restrict__ ref_onset, const int* __restrict__ ref_offset,
                                                              int* __restrict__ P) {
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
