// beam_shared.h — what the two ways to extract a located event's audio share: the delay-and-sum beam (beam.hip) and the
// adaptive MVDR beam (mvdr.hip).  Device code: the rule that gives an event its samples, so that both extract the SAME
// samples and both agree with sed_event_beam_spans.  Host code: the checks of the event columns and of the recordings of a linear
// call, the recording table (sample_off [R*C] and n_samples [R], 64-bit; a ring call: n_samples [R] alone) at the head of the
// workspace and its upload.
#pragma once
#include <vector>
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

size_t beam_table_bytes(int R, int channels) { return (((size_t)R * channels + R) * sizeof(long) + 15) & ~(size_t)15; }

// what the entries share: the sizes and the event columns
int beam_check_events(const char* who, int R, int channels, const int* ev_rec, const int* ev_onset, const int* ev_offset, const int* ev_peak,
                      const int* ev_dir, const int* ev_loc, long E, int time_factor, int hop, int max_frames, int D) {
    SED_REQUIRE(channels >= 2 && channels <= TD_MAX_CH, "%s: 2 to %d channels, got %d", who, TD_MAX_CH, channels);
    SED_REQUIRE(max_frames >= 1, "%s: max_frames must be >= 1, got %d", who, max_frames);
    SED_REQUIRE(time_factor >= 1 && hop >= 1 && R >= 1 && E >= 0, "%s: bad sizes (time_factor=%d, hop=%d, R=%d, E=%ld)", who,
                time_factor, hop, R, E);
    SED_REQUIRE((long)max_frames * hop <= 0x7fffffffL, "%s: max_frames * hop = %ld samples per event exceed 2^31 - 1", who,
                (long)max_frames * hop);
    SED_REQUIRE(D >= 1, "%s: at least one direction, got %d", who, D);
    SED_REQUIRE(E == 0 || (ev_onset && ev_offset && ev_peak && ev_dir && ev_loc), "%s: null pointer (an event column)", who);
    SED_REQUIRE(E == 0 || ev_rec || R == 1, "%s: %d recordings need ev_rec", who, R);
    return 0;
}

// the recordings of a linear call, checked on the host: h = sample_off [R*C], n_samples [R]
int beam_linear_table(const char* who, long pcm_len, const long* clips_host, int R, int channels, int hop, std::vector<long>& h,
                      long& longest) {
    SED_REQUIRE(clips_host && pcm_len > 0, "%s: null pointer (the clip table) or an empty buffer", who);
    h.assign((size_t)R * channels + R, 0);
    long *soff = h.data(), *slen = soff + (size_t)R * channels;
    longest = 0;
    for (int r = 0; r < R; ++r) {
        const long n0 = clips_host[2 * ((long)r * channels) + 1];
        for (int ch = 0; ch < channels; ++ch) {
            const long c = (long)r * channels + ch, o = clips_host[2 * c], n = clips_host[2 * c + 1];
            SED_REQUIRE(o >= 0 && n >= 1 && o <= pcm_len && n <= pcm_len - o,
                        "%s: recording %d, channel %d (offset %ld, %ld samples) is not inside the PCM buffer of %ld samples", who, r, ch,
                        o, n, pcm_len);
            SED_REQUIRE(n == n0, "%s: recording %d: channel %d has %ld samples, channel 0 has %ld (the channels of a recording "
                        "must have equal length)", who, r, ch, n, n0);
            soff[c] = o;
        }
        slen[r] = n0;
        SED_REQUIRE(1 + n0 / hop <= 0x7fffffffL, "%s: recording %d has more than 2^31 - 1 feature frames", who, r);
        if (n0 > longest) longest = n0;
    }
    return 0;
}

// the recordings of a ring call (live feeds): h = n_samples [R], the samples every feed has received
size_t beam_ring_table_bytes(int R) { return ((size_t)R * sizeof(long) + 15) & ~(size_t)15; }

int beam_ring_table(const char* who, const long* n_host, int R, int hop, std::vector<long>& h, long& longest) {
    SED_REQUIRE(n_host, "%s: null pointer (the sample counts)", who);
    h.assign((size_t)R, 0);
    longest = 0;
    for (int r = 0; r < R; ++r) {
        h[r] = n_host[r];
        SED_REQUIRE(h[r] >= 0 && 1 + h[r] / hop <= 0x7fffffffL, "%s: feed %d: %ld samples received (negative, or more than "
                    "2^31 - 1 feature frames)", who, r, h[r]);
        if (h[r] > longest) longest = h[r];
    }
    return 0;
}

int beam_upload(const char* who, const std::vector<long>& h, size_t tab, void* workspace, size_t workspace_bytes, hipStream_t s) {
    SED_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be a 16-byte aligned device buffer", who);
    SED_REQUIRE(workspace_bytes >= tab, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, tab);
    const hipError_t err = hipMemcpyAsync(workspace, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (err != hipSuccess) { sed_set_error("%s: upload of the recording table: %s", who, hipGetErrorString(err)); return (int)err; }
    return 0;
}

TdArgs beam_args(bool ring, const void* workspace, int R, int channels, const int* ev_rec, const int* ev_onset, const int* ev_offset,
                 const int* ev_peak, int time_factor, int hop, int max_frames, long cap) {
    const long* dl = (const long*)workspace;
    TdArgs ta{};
    ta.sample_off = ring ? nullptr : dl;
    ta.n_samples = ring ? dl : dl + (size_t)R * channels;
    ta.ev_rec = ev_rec; ta.ev_onset = ev_onset; ta.ev_offset = ev_offset; ta.ev_peak = ev_peak;
    ta.R = R; ta.C = channels; ta.P = channels * (channels - 1) / 2;
    ta.tf = time_factor; ta.hop = hop; ta.max_frames = max_frames;
    ta.cap = ring ? cap : 0;
    return ta;
}

}  // namespace
