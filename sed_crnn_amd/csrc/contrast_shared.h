// contrast_shared.h — contrast SRP-PHAT: what contrast.hip (the selection of an event's background frames and their
// accumulate launch), doa.hip and doatrack.hip (the steer kernels that subtract the background's share) agree on.
// Device code: the kernel arguments and the one place where S' = S - w Sb is formed.  Host code: the settings of an entry, their
// checks, and the two steps an entry hands to the shared runner (tdoa_shared.h): ct_pre, once per call, and ct_accum, once per
// slice in front of the steer launch.  The activity mask behind the recording table — its bytes, its bounds, its build — and the
// selection walk are activity_shared.h's, shared with the quiet-frame MVDR.
#pragma once
#include <stdint.h>
#include "common.h"
#include "tdoa_shared.h"
#include "activity_shared.h"

#define CT_MAX_FRAMES 256                         // localize.Contrast: frames
#define CT_MAX_SEARCH 4096                        //                    search
#define CT_MAX_GUARD 64                           //                    guard
#define CT_MAX_CLASSES 32                         // the bits of a mask word
#define CT_MAX_WEIGHT 4.0
static_assert(CT_MAX_FRAMES <= ACT_MAX_SEL, "act_select_walk keeps at most ACT_MAX_SEL entries");

struct CtArgs {
    ActMask act;                // the event classes, the rows of the whole table and the activity mask
    int Nb, search, guard, min_frames;
    double weight;
    int* bg_frames;             // [E] nb: the background frames of every event (0: its map is the plain one)
    int* bg_sel;                // [E][Nb] their candidates q in summation order, -1 behind them
    int cpo;                    // an event's own chunk slots: its background chunks are the rows cpo .. of its TdArgs.cpe
};

// what an entry takes beside its DOA sibling's arguments
struct CtSettings {
    const int* cls;
    int n_classes, frames, search, guard, min_frames;
    double weight;
    int *frames_out, *sel_out;
};

// an entry's run: filled by the entry (cs, pcm, tables, pad_mode, cpb), by ct_pre (the mask) and by ct_accum (cpo)
struct CtRun {
    CtSettings cs;
    const float* pcm;
    const void* tables;
    int pad_mode;
    int cpb;                    // background chunk slots per event: ceil(frames / 32)
    CtArgs ca;
};

namespace {

// w of an event (or track block) summed over n frames beside nb background frames
__device__ __forceinline__ float ct_weight(double weight, int n, int nb) { return (float)(weight * (double)n / (double)nb); }

// S [1025] (LDS) = S_own - w Sb for pair p: S_own as phat_sum_chunks makes it from the nch chunks at `wev`, Sb the same sum over
// the nbc background chunks at `wbg`, one fmaf per component.  Entry k is made by one thread; DC and Nyquist stay real.
__device__ __forceinline__ void ct_sum_chunks(float2* S, const float2* __restrict__ wev, const float2* __restrict__ wbg, int p, int P,
                                              int nch, int nbc, float w, int tid, int threads) {
    for (int k = tid; k < 1025; k += threads) {
        float2 s = wev[(long)p * PHAT_SPEC + k];
        for (int c = 1; c < nch; ++c) {
            const float2 v = wev[((long)c * P + p) * PHAT_SPEC + k];
            s.x += v.x; s.y += v.y;
        }
        float2 b = wbg[(long)p * PHAT_SPEC + k];
        for (int c = 1; c < nbc; ++c) {
            const float2 v = wbg[((long)c * P + p) * PHAT_SPEC + k];
            b.x += v.x; b.y += v.y;
        }
        S[k] = make_float2(fmaf(-w, b.x, s.x), fmaf(-w, b.y, s.y));
    }
}

// the background frames of event e as the steer kernels read them: 0 .. Nb
__device__ __forceinline__ int ct_bg_frames(const CtArgs& ca, long e) {
    const int nb = ca.bg_frames[e];
    return nb < 0 ? 0 : nb > ca.Nb ? ca.Nb : nb;
}

}  // namespace

// ── host (contrast.hip) ──
// the settings, checked before anything is enqueued
int ct_check(const char* who, long E, const CtSettings& cs);
// act_mask_ok and the bound of `frames`
bool ct_sizes_ok(int R, long mask_frames, int frames);
// TdExtra.pre (ctx: a CtRun): the activity of the whole table, then every event's background frames into frames_out / sel_out
int ct_pre(void* ctx, const RecSource& src, const EvTable& ev, void* workspace, hipStream_t s);
// the background chunks of a slice's events into the rows behind their own
int ct_accum(const char* who, CtRun& run, const TdArgs& ta, const float2* part, hipStream_t s);
