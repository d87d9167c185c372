// activity_shared.h — the class activity of an event table and the walk that picks an event's frames before its onset by it:
// what the quiet-frame MVDR (mvdr.hip) and the contrast SRP-PHAT (contrast.hip) share.  All integer.
// With H = tf hop and L_r = n_r / H + 1 output frames, mask[r][t] holds bit cls of every row of the table for
// onset <= t < min(offset, L_r), located or not; rows that name no recording, no class of n_classes or a negative onset mark
// nothing (event_activity_k, activity.hip).
// The walk: candidate q = 0 .. S-1 of an event exists iff origin - lead - q stride >= 0 and is eligible when no output frame that
// the samples [origin - before - q stride, origin + after - q stride) touch — the low end clamped to 0, the frames
// lo / H .. min(ceil(hi / H), L_r) - 1 — has a bit of `excl` set.  The first N eligible candidates in ascending q are kept, none
// where they are fewer than M, and written in summation order: descending q, ascending time, -1 behind them.
//                 origin                       stride  before         after  lead        N        S              M
//   quiet MVDR    s0 (bm_event_span)           1024    (2 G + 2) 1024 0      (G + 2) 1024 Kn      noise_search   noise_min
//   contrast      (onset tf - G - 1) hop       hop     1024           1024   0            frames  search         min_frames
#pragma once
#include <stdint.h>
#include "common.h"
#include "tdoa_shared.h"

#define ACT_MAX_SEL 256                           // the entries a walk keeps at most: MV_MAX_NOISE (mvdr.hip), CT_MAX_FRAMES

struct ActMask {
    const int* ev_cls;          // [E]
    long E;                     // rows of the whole table
    int n_classes;
    const long* mask_off;       // [R] recording r's first word of mask
    uint32_t* mask;             // [sum L_r] the class bits of every output frame
};
struct ActWindow { long origin, stride, before, after, lead; };       // the windows of an event's candidates, in samples (above)

namespace {

// One wave walks the candidates of its event 64 at a time; the ballot's prefix count ranks the eligible ones, nearest first.
// Called by the 64 threads of the workgroup for every event, block-uniformly; an event that does not take part gets 0 and a row of -1.
__device__ __forceinline__ void act_select_walk(const TdArgs& ta, const ActMask& am, bool takes, int rec, uint32_t excl, const ActWindow& w,
                                                int N, int S, int M, int* sel, int* count_out) {
    __shared__ int s_q[ACT_MAX_SEL];
    const int lane = threadIdx.x;
    int count = 0;
    if (takes) {                                                 // (block-uniform)
        const long H = (long)ta.tf * ta.hop;
        const uint32_t* row = am.mask + am.mask_off[rec];
        const long L = ta.n_samples[rec] / H + 1;
        for (int q0 = 0; q0 < S && count < N && w.origin - w.lead - q0 * w.stride >= 0; q0 += 64) {
            const int q = q0 + lane;
            const long at = w.origin - q * w.stride;
            bool ok = q < S && at - w.lead >= 0;
            if (ok) {
                long lo = at - w.before;
                if (lo < 0) lo = 0;
                long t1 = (at + w.after + H - 1) / H;            // (an existing candidate ends after sample 0 and starts inside the recording)
                if (t1 > L) t1 = L;
                for (long t = lo / H; t < t1 && ok; ++t) ok = (row[t] & excl) == 0;
            }
            const unsigned long long m = __ballot(ok);
            const int rank = count + __popcll(m & ((1ull << lane) - 1ull));
            if (ok && rank < N) s_q[rank] = q;
            count += __popcll(m);
        }
        if (count > N) count = N;
        if (count < M) count = 0;
    }
    __syncthreads();
    for (int i = lane; i < N; i += 64) sel[i] = i < count ? s_q[count - 1 - i] : -1;
    if (lane == 0) *count_out = count;
    __syncthreads();                                             // s_q is free for the next event
}

}  // namespace

// ── host (activity.hip) ──
// the bytes behind the recording table: mask_off [R], then the mask of `frames` words, each rounded to 16 bytes
size_t act_mask_bytes(int R, long frames);
bool act_mask_ok(int R, long frames);
// the mask's words, sum_r L_r: of a checked source, and of a caller's clip table — 0 where the shared checks will refuse the call
long act_mask_frames(const RecSource& src, const EvTable& ev);
long act_mask_frames(const long* clips_host, int R, int channels, int tf, int hop);
// The activity of the whole table into the mask behind the recording table (which is uploaded): mask_off to workspace + src.tab,
// the mask cleared, event_activity_k launched (`label`: its name in a launch error), *out filled.  The caller has checked the size.
int act_mask_build(const char* who, const char* label, const RecSource& src, const EvTable& ev, const int* cls, int n_classes,
                   void* workspace, hipStream_t s, ActMask* out);
