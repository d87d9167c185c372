// activity.hip — the class activity of an event table (activity_shared.h): the mask's size, its bounds, its word count and its
// build, for the quiet-frame MVDR (mvdr.hip) and the contrast SRP-PHAT (contrast.hip).
// Shape (gfx950): event_activity_k, one plain launch per call over the whole table: a wave per row, a lane per output frame, an
// atomic OR from vector lanes.  The OR does not depend on the order, so nothing depends on the launch shape.
#include <vector>
#include "common.h"
#include "activity_shared.h"

namespace {

// every row counts, located or not; out-of-range rows mark nothing; onset and offset are clamped to [0, L_rec]
__global__ __launch_bounds__(256) void event_activity_k(TdArgs ta, ActMask am) {
    const int lane = threadIdx.x & 63;
    const long H = (long)ta.tf * ta.hop;
    for (long e = (long)blockIdx.x * 4 + (threadIdx.x >> 6); e < am.E; e += (long)gridDim.x * 4) {
        const int rec = ta.ev_rec ? ta.ev_rec[e] : 0, cls = am.ev_cls[e];
        const long on = ta.ev_onset[e];
        if (rec < 0 || rec >= ta.R || cls < 0 || cls >= am.n_classes || on < 0) continue;
        const long L = ta.n_samples[rec] / H + 1;
        long off = ta.ev_offset[e];
        if (off > L) off = L;
        uint32_t* row = am.mask + am.mask_off[rec];
        for (long t = on + lane; t < off; t += 64) atomicOr(row + t, 1u << cls);
    }
}

size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

// the R sample counts n[0], n[step], ..: the words of their mask, recording r's first word to off[r]; 0 where a count is < 1
long mask_words(const long* n, long step, int R, long H, long* off) {
    long frames = 0;
    for (int r = 0; r < R; ++r) {
        if (n[r * step] < 1) return 0;
        if (off) off[r] = frames;
        frames += n[r * step] / H + 1;
    }
    return frames;
}

}  // namespace

size_t act_mask_bytes(int R, long frames) { return round16((size_t)R * sizeof(long)) + round16((size_t)frames * 4); }
bool act_mask_ok(int R, long frames) { return R >= 1 && frames >= R && frames <= (1L << 40); }

long act_mask_frames(const RecSource& src, const EvTable& ev) {
    return mask_words(src.h.data() + (size_t)src.R * src.C, 1, src.R, (long)ev.tf * ev.hop, nullptr);
}

long act_mask_frames(const long* clips_host, int R, int channels, int tf, int hop) {
    if (!clips_host || R < 1 || channels < 1 || tf < 1 || hop < 1) return 0;
    return mask_words(clips_host + 1, 2L * channels, R, (long)tf * hop, nullptr);
}

int act_mask_build(const char* who, const char* label, const RecSource& src, const EvTable& ev, const int* cls, int n_classes,
                   void* workspace, hipStream_t s, ActMask* out) {
    std::vector<long> off((size_t)src.R);
    const long frames = mask_words(src.h.data() + (size_t)src.R * src.C, 1, src.R, (long)ev.tf * ev.hop, off.data());
    long* d_off = (long*)((char*)workspace + src.tab);
    uint32_t* d_mask = (uint32_t*)((char*)d_off + round16((size_t)src.R * sizeof(long)));
    hipError_t err = hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipMemsetAsync(d_mask, 0, (size_t)frames * 4, s);
    if (err != hipSuccess) { sed_set_error("%s: upload of the mask offsets: %s", who, hipGetErrorString(err)); return (int)err; }
    *out = ActMask{cls, ev.E, n_classes, d_off, d_mask};
    const long cap = 1L << 20;
    event_activity_k<<<(unsigned)((ev.E + 3) / 4 < cap ? (ev.E + 3) / 4 : cap), 256, 0, s>>>(td_args(src, ev, workspace), *out);
    SED_LAUNCH_CHECK(label);
    return 0;
}
