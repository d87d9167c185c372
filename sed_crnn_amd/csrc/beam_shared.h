// beam_shared.h — what the two ways to extract a located event's audio share: the delay-and-sum beam (beam.hip) and the
// adaptive MVDR beam (mvdr.hip).  Device code: the rule that gives an event its samples, so that both extract the SAME
// samples and both agree with sed_event_beam_spans.  Host code: the packed output, the checks of the event columns, the step
// that turns an entry's arguments into a checked source (RecSource, EvTable and the recording table are tdoa_shared.h's, shared
// with the TDOA family) and the upload of the table behind the beams' own workspace checks.
#pragma once
#include "common.h"
#include "tdoa_shared.h"

namespace {

// [s0, s0 + len) of event e and its recording; len = 0: the event is not extracted (localize.event_samples)
__device__ __forceinline__ void bm_event_span(const TdArgs& a, const int* ev_dir, const int* ev_loc, int D, long e, int& rec, long& s0,
                                              int& len) {
    rec = 0; s0 = 0; len = 0;
    const int d = ev_dir[e];
    if (d < 0 || d >= D) return;
    long f0;
    int nf;
    td_linear_range(a, e, rec, f0, nf);
    if (nf == 0) return;
    int lf = ev_loc[e];
    lf = lf < 0 ? 0 : lf > nf ? nf : lf;
    const long n = a.n_samples[rec];
    long s1 = (f0 + lf) * a.hop;
    if (s1 > n) s1 = n;
    s0 = f0 * a.hop;
    len = s1 > s0 ? (int)(s1 - s0) : 0;          // (at most max_frames hop, which the entries hold below 2^31)
}

// the packed output both beams write: sed_event_beam_spans' table ([E] each) and the buffer of `total` samples it lays out
struct BeamOut { const int* audio_len; const long* audio_start; float* audio; long total; };

// what the entries share: the sizes and the event columns
int beam_check_events(const char* who, const RecSource& src, const EvTable& ev) {
    SED_REQUIRE(src.C >= 2 && src.C <= TD_MAX_CH, "%s: 2 to %d channels, got %d", who, TD_MAX_CH, src.C);
    SED_REQUIRE(ev.max_frames >= 1, "%s: max_frames must be >= 1, got %d", who, ev.max_frames);
    SED_REQUIRE(ev.tf >= 1 && ev.hop >= 1 && src.R >= 1 && ev.E >= 0, "%s: bad sizes (time_factor=%d, hop=%d, R=%d, E=%ld)", who, ev.tf,
                ev.hop, src.R, ev.E);
    SED_REQUIRE((long)ev.max_frames * ev.hop <= 0x7fffffffL, "%s: max_frames * hop = %ld samples per event exceed 2^31 - 1", who,
                (long)ev.max_frames * ev.hop);
    SED_REQUIRE(ev.D >= 1, "%s: at least one direction, got %d", who, ev.D);
    SED_REQUIRE(ev.E == 0 || (ev.onset && ev.offset && ev.peak && ev.dir && ev.loc), "%s: null pointer (an event column)", who);
    SED_REQUIRE(ev.E == 0 || ev.rec || src.R == 1, "%s: %d recordings need ev_rec", who, src.R);
    return 0;
}

// the events and the recordings of an entry, checked; SAMPLES: the entry reads them (the spans entries do not)
template <bool RING, bool SAMPLES = true>
int beam_source(const char* who, RecSource& src, const EvTable& ev) {
    SED_TRY(beam_check_events(who, src, ev));
    if (RING) {
        if (SAMPLES) SED_TRY(rec_ring_check(who, src));
        return rec_source_ring(who, src, ev.hop);
    }
    SED_REQUIRE(!SAMPLES || src.x, "%s: null pointer (the samples)", who);
    return rec_source_linear(who, src, ev.hop);
}

int beam_upload(const char* who, const RecSource& src, void* workspace, size_t workspace_bytes, hipStream_t s) {
    SED_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device buffer", who);
    SED_REQUIRE(workspace_bytes >= src.tab, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, src.tab);
    return rec_upload(who, src, workspace, s);
}

}  // namespace
