// contrast.hip — contrast SRP-PHAT: the background frames of every located event and their whitened cross spectra:
// sed_event_contrast_frames, and the steps that sed_event_doa_contrast (doa.hip) and sed_event_doa_track_contrast (doatrack.hip) run
// in front of their steer launches.
//
// An event that sounds over a louder source of another class gets that source's direction from sed_event_doa: the whitening
// gives every bin to whichever source is loudest in it.  In the frames before the onset in which the event's own class is silent
// the other source sounds and the event does not, and the inverse transform and the steering are linear in the cross spectrum:
//   S'[k] = S[k] - w Sb[k],   w = (float)((double)weight nf / nb)
// with S the event's sum over its nf located frames and Sb the sum over nb background frames.  The bins the other source wins
// cancel, the bins the event wins stay.
//
// The rule is integer and reads the event table and the settings alone.  With H = tf hop and L_r = n_r / H + 1 output frames:
//   mask[r][t]  bit cls of every row of the table for onset <= t < min(offset, L_r), located or not (DESIGN 5w's, activity.hip)
//   candidate q = 0 .. S-1 of an event of class k whose first feature frame is a = onset tf: feature frame g = a - G - 1 - q,
//   which exists when g >= 0 and is eligible when bit k of mask[r][t] is clear in every output frame its 2048 samples
//   [g hop - 1024, g hop + 1024) touch: t = max(g hop - 1024, 0) / H .. min(ceil((g hop + 1024) / H), L_r) - 1
//   the first Nb eligible candidates in ascending q are the event's background frames, nb of them; fewer than M: none (nb = 0)
//   bg_sel[e][0 .. nb) lists them in summation order: descending q, ascending time; -1 behind them
//
// Shape (gfx950), plain launches, no workgroup waits on another, no atomics but the mask's OR (event_activity_k's atomicOr):
//   contrast_select_k     a wave per event gives its window to the shared walk (act_select_walk, activity_shared.h) over the
//                         candidates 64 at a time; a ballot and its prefix count rank the eligible ones; the first Nb are written
//                         out reversed.  Once per call, over the whole table, behind the activity launch, before the first slice.
//   contrast_accum_k      per slice: one workgroup per chunk of 32 consecutive entries of an event's list, the body of
//                         tdoa_accum_k (td_accum_chunk, tdoa_accum.h) on the frames a - G - 1 - bg_sel[e][j]; its partial goes to
//                         the chunk rows behind the event's own.  A frame is loaded, transformed and whitened exactly as the
//                         located frame of that index is; the pipelined (C <= 4) and the pair-batch (C >= 5) paths are the body's.
// The steer kernels add the chunk partials in ascending chunk order, as they add S's (ct_sum_chunks, contrast_shared.h): every
// sum has one order, which depends on the event and its selected frames alone.
#include <math.h>
#include <cmath>
#include "common.h"
#include "fft2048.h"
#include "tdoa_shared.h"
#include "tdoa_accum.h"
#include "contrast_shared.h"

namespace {

// other classes never block: they are what is subtracted; the window of candidate q is feature frame g0 - q's 2048 samples
__global__ __launch_bounds__(64) void contrast_select_k(TdArgs ta, CtArgs ca) {
    for (long e = blockIdx.x; e < ca.act.E; e += gridDim.x) {
        int rec, nf;
        long f0;
        td_linear_range(ta, e, rec, f0, nf);
        const int cls = ca.act.ev_cls[e];
        const bool takes = nf != 0 && cls >= 0 && cls < ca.act.n_classes;            // (block-uniform)
        const ActWindow w{((long)ta.ev_onset[e] * ta.tf - ca.guard - 1) * ta.hop, ta.hop, LM_NFFT / 2, LM_NFFT / 2, 0};
        act_select_walk(ta, ca.act, takes, rec, takes ? 1u << cls : 0u, w, ca.Nb, ca.search, ca.min_frames, ca.bg_sel + e * ca.Nb,
                        ca.bg_frames + e);
    }
}

// The chunk's frames are entries fc0 .. of the event's list; the body is tdoa_accum_k's.  An event with a list was located
// (nf > 0), so its recording is in range; a list entry that the selection did not write (none is read: the chunk ends at nb)
// would still name a frame whose every load is guarded.
__global__ __launch_bounds__(TD_THREADS) void contrast_accum_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                               float2* __restrict__ ws, int pad_mode, TdArgs ta, CtArgs ca) {
    const long e = ta.e0 + blockIdx.y;
    const int nb = ct_bg_frames(ca, e);
    const int fc0 = blockIdx.x * TD_CHUNK;                       // the chunk's first entry of the list
    if (fc0 >= nb) return;                                       // (block-uniform: before any barrier)
    const int fc1 = fc0 + TD_CHUNK < nb ? fc0 + TD_CHUNK : nb;
    int rec = ta.ev_rec ? ta.ev_rec[e] : 0;
    if (rec < 0 || rec >= ta.R) return;
    const long g0 = (long)ta.ev_onset[e] * ta.tf - ca.guard - 1;
    const int* sel = ca.bg_sel + e * ca.Nb + fc0;
    float2* wrow = ws + ((long)blockIdx.y * ta.cpe + ca.cpo + blockIdx.x) * ta.P * PHAT_SPEC;
    td_accum_chunk<false>(pcm, tables, wrow, pad_mode, ta, rec, fc1 - fc0, [&](int step) -> long { return g0 - sel[step]; });
}

}  // namespace

bool ct_sizes_ok(int R, long mask_frames, int frames) { return act_mask_ok(R, mask_frames) && frames >= 1 && frames <= CT_MAX_FRAMES; }

int ct_check(const char* who, long E, const CtSettings& cs) {
    SED_REQUIRE(cs.frames >= 1 && cs.frames <= CT_MAX_FRAMES, "%s: frames must be in [1, %d], got %d", who, CT_MAX_FRAMES, cs.frames);
    SED_REQUIRE(cs.search >= cs.frames && cs.search <= CT_MAX_SEARCH, "%s: search must be in [frames = %d, %d], got %d", who, cs.frames,
                CT_MAX_SEARCH, cs.search);
    SED_REQUIRE(cs.guard >= 0 && cs.guard <= CT_MAX_GUARD, "%s: guard must be in [0, %d], got %d", who, CT_MAX_GUARD, cs.guard);
    SED_REQUIRE(cs.min_frames >= 1 && cs.min_frames <= cs.frames, "%s: min_frames must be in [1, frames = %d], got %d", who, cs.frames,
                cs.min_frames);
    SED_REQUIRE(std::isfinite(cs.weight) && cs.weight > 0.0 && cs.weight <= CT_MAX_WEIGHT, "%s: weight must be finite and in (0, %g], got %g",
                who, CT_MAX_WEIGHT, cs.weight);
    SED_REQUIRE(cs.n_classes >= 1 && cs.n_classes <= CT_MAX_CLASSES, "%s: n_classes must be in [1, %d], got %d", who, CT_MAX_CLASSES,
                cs.n_classes);
    SED_REQUIRE(E == 0 || (cs.cls && cs.frames_out && cs.sel_out), "%s: null pointer (ev_cls, bg_frames_out or bg_sel_out)", who);
    return 0;
}

int ct_pre(void* ctx, const RecSource& src, const EvTable& ev, void* workspace, hipStream_t s) {
    CtRun& run = *static_cast<CtRun*>(ctx);
    const CtSettings& cs = run.cs;
    run.ca = CtArgs{{}, cs.frames, cs.search, cs.guard, cs.min_frames, cs.weight, cs.frames_out, cs.sel_out, 0};
    SED_TRY(act_mask_build("contrast", "contrast (activity)", src, ev, cs.cls, cs.n_classes, workspace, s, &run.ca.act));
    const long cap = 1L << 20;
    contrast_select_k<<<(unsigned)(ev.E < cap ? ev.E : cap), 64, 0, s>>>(td_args(src, ev, workspace), run.ca);
    SED_LAUNCH_CHECK("contrast (selection)");
    return 0;
}

int ct_accum(const char* who, CtRun& run, const TdArgs& ta, const float2* part, hipStream_t s) {
    SED_REQUIRE(ta.cpe > run.cpb && ta.cap == 0, "%s: the slice has %d chunk slots per event, %d of them for the background", who, ta.cpe,
                run.cpb);
    run.ca.cpo = ta.cpe - run.cpb;
    const hipError_t err = hipFuncSetAttribute((const void*)contrast_accum_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TD_LDS_MAX);
    if (err != hipSuccess) { sed_set_error("%s: hipFuncSetAttribute: %s", who, hipGetErrorString(err)); return (int)err; }
    const size_t lds = tdoa_lds_bytes(ta.C, ta.pairs_per_batch, ta.pipelined ? 2 : 1);
    contrast_accum_k<<<dim3((unsigned)run.cpb, (unsigned)ta.n_ev), TD_THREADS, lds, s>>>(run.pcm, (const uint32_t*)run.tables,
                                                                                          const_cast<float2*>(part), run.pad_mode, ta, run.ca);
    SED_LAUNCH_CHECK("contrast (accumulate)");
    return 0;
}

// workspace: sample_off [R*C] and n_samples [R], then mask_off [R] and the mask
extern "C" size_t sed_event_contrast_frames_workspace_bytes(int R, int channels, long mask_frames, int frames) {
    if (R < 1 || channels < 2 || channels > TD_MAX_CH || !ct_sizes_ok(R, mask_frames, frames)) return 0;
    return rec_table_bytes(R, channels) + act_mask_bytes(R, mask_frames);
}

// the activity and the selection alone; no sample is read
extern "C" int sed_event_contrast_frames(long pcm_len, const long* clips_host, int R, int channels, const int* ev_rec, const int* ev_cls,
                                         const int* ev_onset, const int* ev_offset, const int* ev_peak_frame, long E, int time_factor,
                                         int hop, int max_frames, int n_classes, int frames, int search, int guard, int min_frames,
                                         int* bg_frames_out, int* bg_sel_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "contrast_frames";
    RecSource src{nullptr, false, 0, pcm_len, R, channels, clips_host};
    const EvTable ev{ev_rec, ev_onset, ev_offset, ev_peak_frame, nullptr, nullptr, E, time_factor, hop, max_frames, 0};
    SED_REQUIRE(channels >= 2 && channels <= TD_MAX_CH, "%s: 2 to %d channels, got %d", who, TD_MAX_CH, channels);
    SED_REQUIRE(max_frames >= 1, "%s: max_frames must be >= 1, got %d", who, max_frames);
    SED_REQUIRE(time_factor >= 1 && hop >= 1 && R >= 1 && E >= 0, "%s: bad sizes (time_factor=%d, hop=%d, R=%d, E=%ld)", who, time_factor,
                hop, R, E);
    SED_REQUIRE(E == 0 || (ev_onset && ev_offset && ev_peak_frame), "%s: null pointer (an event column)", who);
    SED_REQUIRE(E == 0 || ev_rec || R == 1, "%s: %d recordings need ev_rec", who, R);
    CtRun run{};
    run.cs = CtSettings{ev_cls, n_classes, frames, search, guard, min_frames, 1.0, bg_frames_out, bg_sel_out};
    SED_TRY(ct_check(who, E, run.cs));
    SED_TRY(rec_source_linear(who, src, hop));
    if (E == 0) return 0;
    const size_t need = src.tab + act_mask_bytes(R, act_mask_frames(src, ev));
    SED_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device buffer", who);
    SED_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    SED_TRY(rec_upload(who, src, workspace, s));
    return ct_pre(&run, src, ev, workspace, s);
}
