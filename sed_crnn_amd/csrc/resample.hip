// resample.hip — rational-ratio polyphase resampler with the sample-format conversion and the channel downmix fused into its
// load.  One launch takes R clips packed in one input buffer and writes R mono float32 clips into one output
// buffer laid out the way sed_logmel_batch reads it.  A row may instead KEEP one channel of the interleaved frames
// (sed_resample_select): it then stages the converted sample itself, bit for bit what the mono path stages for x[:, c].
//
// Output m (absolute index) of a clip: u = m M, i_c = u div L, p = u mod L, y[m] = sum_k h[p][k] x[i_c - half + 1 + k], x = 0
// outside what the clip has.  The sum runs in ONE fixed fp32 order that depends on (p, k) only (rs_dot): four chains over
// k mod 4, joined as (a0 + a1) + (a2 + a3).  Nothing in it depends on where a tile, a chunk or a workgroup begins, which is
// what makes a stream's output bit for bit the offline output.
//
// Staging: persistent workgroups of 1024 threads (one output per thread and tile of RS_TILE outputs).  The tap table
// [L][K] is copied to LDS once per workgroup, its rows in the order consecutive outputs visit them (row m mod L) and with an odd
// row stride K + 1, so that the lanes of a wave read rows that lie on distinct banks; the input span of a tile — converted, downmixed, history and zero
// padding resolved — is staged in LDS too, so the inner loop is two LDS reads and one FMA per tap.
#include "common.h"
#include <vector>

#define RS_TILE 1024                 // outputs per tile = threads per workgroup
#define RS_SPAN_MAX 8192             // floats of staged input per tile
#define RS_TAPS_MAX 26624            // floats of the padded tap table in LDS (441 x 55 = 24 255 for 16 / 32 / 8 kHz -> 44.1 kHz)
#define RS_ROW 9                     // longs per row of the host table (sed_resample)
#define RS_ROW_SELECT 10             // ... of sed_resample_select: the tenth column is the row's channel (-1 = downmix)

// a clip as the kernel sees it (uploaded by sed_resample from the validated host table)
struct RsClip {
    long in_off, n_in;               // first sample frame in x and how many there are
    long in_base;                    // absolute index of that first frame in the clip's own time line
    long out_first, n_out, out_off;  // absolute index of the first output, how many, where they go in out
    long hist_off, n_hist;           // mono float32 samples [in_base - n_hist, in_base) in hist
    long carry_dst;                  // where the last 2 half samples of (hist | x) go in hist, or -1
    long tile_first;                 // first tile of this clip in the launch
};

__host__ __device__ static inline long rs_span(long n_outputs, int L, int M, int half) {
    // input samples that n_outputs consecutive outputs can touch, whatever the phase of the first
    return ((n_outputs - 1) * (long)M + L - 1) / L + 2L * half;
}

// sample frame `f` of x as mono float32: int16 scaled by 1/32768, channels summed in channel order, times 1/C; with a kept
// channel ch >= 0 (wave-uniform: it belongs to the row) that channel's converted sample alone, no multiplication by 1/C
template <int FMT>
__device__ __forceinline__ float rs_load(const void* __restrict__ x, long f, int C, float inv_c, bool pair_ok, int ch) {
    if (FMT == 1) {
        const short* s = reinterpret_cast<const short*>(x);
        if (ch >= 0) return (float)s[f * C + ch] * (1.0f / 32768.0f);
        if (C == 2 && pair_ok) {                                     // one 4-byte load per stereo frame
            const unsigned v = reinterpret_cast<const unsigned*>(x)[f];
            const float a = (float)(short)(v & 0xffffu) * (1.0f / 32768.0f), b = (float)(short)(v >> 16) * (1.0f / 32768.0f);
            return (a + b) * inv_c;
        }
        float acc = (float)s[f * C] * (1.0f / 32768.0f);
        for (int c = 1; c < C; ++c) acc += (float)s[f * C + c] * (1.0f / 32768.0f);
        return C == 1 ? acc : acc * inv_c;
    }
    const float* s = reinterpret_cast<const float*>(x);
    if (ch >= 0) return s[f * C + ch];
    float acc = s[f * C];
    for (int c = 1; c < C; ++c) acc += s[f * C + c];
    return C == 1 ? acc : acc * inv_c;
}

// absolute sample `i` of a clip: fresh frames, then the history in front of them, zero elsewhere
template <int FMT>
__device__ __forceinline__ float rs_sample(const RsClip& c, long i, const void* __restrict__ x, const float* __restrict__ hist, int C,
                                           float inv_c, bool pair_ok, int ch) {
    const long rel = i - c.in_base;
    if (rel >= 0) return rel < c.n_in ? rs_load<FMT>(x, c.in_off + rel, C, inv_c, pair_ok, ch) : 0.f;
    return rel >= -c.n_hist ? hist[c.hist_off + c.n_hist + rel] : 0.f;
}

// THE summation order: taps k = 0 .. K-1 of one phase against K consecutive samples (K is even)
__device__ __forceinline__ float rs_dot(const float* __restrict__ h, const float* __restrict__ xs, int K) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int k = 0;
    for (; k + 4 <= K; k += 4) {
        a0 = fmaf(h[k], xs[k], a0);
        a1 = fmaf(h[k + 1], xs[k + 1], a1);
        a2 = fmaf(h[k + 2], xs[k + 2], a2);
        a3 = fmaf(h[k + 3], xs[k + 3], a3);
    }
    if (k < K) {                                                     // K mod 4 == 2
        a0 = fmaf(h[k], xs[k], a0);
        a1 = fmaf(h[k + 1], xs[k + 1], a1);
    }
    return (a0 + a1) + (a2 + a3);
}

template <int FMT>
__global__ __launch_bounds__(RS_TILE) void resample_k(const void* __restrict__ x, int C, const float* __restrict__ hist,
                                                      const float* __restrict__ taps, int L, int M, int half,
                                                      const RsClip* __restrict__ clips, const int* __restrict__ chan, int R,
                                                      long n_tiles, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, K = 2 * half, stride = K + 1;
    float* s_tap = lds;
    float* s_x = lds + (size_t)L * stride;
    // row r of the LDS table holds phase (r M) mod L, the phase of every output m with m mod L = r: consecutive outputs (the
    // lanes of a wave) then read consecutive rows, which the odd stride puts on distinct banks
    const unsigned Mr = (unsigned)(M % L);                           // r * Mr < L^2 < 2^28 (L (K + 1) <= RS_TAPS_MAX)
    for (int e = tid; e < L * K; e += RS_TILE) {
        const int r = e / K;
        const unsigned p = ((unsigned)r * Mr) % (unsigned)L;
        s_tap[r * stride + (e - r * K)] = taps[p * K + (e - r * K)];
    }
    const float inv_c = 1.0f / (float)C;
    const bool pair_ok = (reinterpret_cast<uintptr_t>(x) & 3) == 0;
    for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        int lo = 0, hi = R - 1;                                      // the last clip whose first tile is <= tile (wave-uniform)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (clips[mid].tile_first <= tile) lo = mid;
            else hi = mid - 1;
        }
        const RsClip c = clips[lo];
        const int ch = chan ? chan[lo] : -1;                         // the row's kept channel (null table: every row downmixes)
        const long j0 = (tile - c.tile_first) * RS_TILE;             // first output of the tile within the clip
        const long left = c.n_out - j0;
        const int n = left < RS_TILE ? (int)left : RS_TILE;
        const long m_first = c.out_first + j0;
        const long u0 = m_first * (long)M;                           // 64-bit once per tile; per thread 32 bits are enough
        const unsigned row0 = (unsigned)(m_first % L);
        const long q0 = u0 / L;
        const unsigned r0 = (unsigned)(u0 - q0 * L);
        const long a0 = q0 - half + 1;                               // absolute index of the tile's first staged sample
        const int span = (int)rs_span(n, L, M, half);                // <= RS_SPAN_MAX (checked on the host)
        __syncthreads();                                             // the taps are there / the previous tile is done with s_x
        for (int i = tid; i < span; i += RS_TILE) s_x[i] = rs_sample<FMT>(c, a0 + i, x, hist, C, inv_c, pair_ok, ch);
        __syncthreads();
        if (tid < n) {
            const unsigned v = (unsigned)tid * (unsigned)M + r0;     // < RS_TILE * M + L < 2^31 (M, L <= 2^20)
            const unsigned dq = v / (unsigned)L;
            const unsigned row = (row0 + (unsigned)tid) % (unsigned)L;       // = m mod L: the table row of phase v mod L
            out[c.out_off + j0 + tid] = rs_dot(s_tap + row * stride, s_x + dq, K);
        }
    }
}

// the carry of a stream: the last n_carry samples of (hist | x), zero where the clip has nothing, to hist[carry_dst, ...)
template <int FMT>
__global__ void resample_carry_k(const void* __restrict__ x, int C, float* __restrict__ hist, const RsClip* __restrict__ clips,
                                 const int* __restrict__ chan, int n_carry) {
    const RsClip c = clips[blockIdx.x];
    if (c.carry_dst < 0) return;
    const int ch = chan ? chan[blockIdx.x] : -1;
    const float inv_c = 1.0f / (float)C;
    const bool pair_ok = (reinterpret_cast<uintptr_t>(x) & 3) == 0;
    const long first = c.in_base + c.n_in - n_carry;
    for (int i = threadIdx.x; i < n_carry; i += blockDim.x)
        hist[c.carry_dst + i] = rs_sample<FMT>(c, first + i, x, hist, C, inv_c, pair_ok, ch);
}

// ───────────────────────── host side ─────────────────────────
static int rs_check_plan(int L, int M, int half) {
    SED_REQUIRE(L >= 1 && M >= 1 && L <= (1 << 20) && M <= (1 << 20) && half >= 1 && half <= 2048,
                "resample: bad plan (L=%d, M=%d, half=%d)", L, M, half);
    SED_REQUIRE((long)L * (2 * half + 1) <= RS_TAPS_MAX,
                "resample: a tap table of %d phases x %d taps exceeds the %d floats that stay in LDS", L, 2 * half, RS_TAPS_MAX);
    SED_REQUIRE(rs_span(RS_TILE, L, M, half) <= RS_SPAN_MAX,
                "resample: a tile of %d outputs at M/L = %d/%d reads %ld samples, more than the %d that are staged", RS_TILE, M, L,
                rs_span(RS_TILE, L, M, half), RS_SPAN_MAX);
    return 0;
}

// workspace: R RsClip records
extern "C" size_t sed_resample_workspace_bytes(int R) {
    if (R < 1 || R > (1 << 24)) return 0;
    return (size_t)R * sizeof(RsClip);
}

// workspace of sed_resample_select: the R RsClip records, then the R channels (32-bit)
extern "C" size_t sed_resample_select_workspace_bytes(int R) {
    if (R < 1 || R > (1 << 24)) return 0;
    return (size_t)R * sizeof(RsClip) + (((size_t)R * sizeof(int) + 7) & ~(size_t)7);
}

// row_len = RS_ROW: every row downmixes; RS_ROW_SELECT: column 9 is the row's channel, in [-1, channels)
static int rs_check_table(const long* t, int R, int row_len, int channels, long x_frames, long hist_len, long out_len, int L, int M,
                          int half, std::vector<RsClip>* recs, std::vector<int>* chans, long* n_tiles) {
    SED_REQUIRE(t, "resample: null pointer");
    SED_REQUIRE(sed_resample_workspace_bytes(R) > 0 && x_frames >= 0 && hist_len >= 0 && out_len >= 0,
                "resample: bad sizes (R=%d, %ld frames, %ld history samples, %ld outputs)", R, x_frames, hist_len, out_len);
    if (int rc = rs_check_plan(L, M, half)) return rc;
    const long lim = 1L << 42, n_carry = 2L * half;                  // m M and n L stay far inside 64 bits
    long out_end = 0, tiles = 0;
    for (int r = 0; r < R; ++r) {
        const long* q = t + (size_t)r * row_len;
        if (row_len == RS_ROW_SELECT) {
            SED_REQUIRE(q[9] >= -1 && q[9] < channels, "resample: clip %d: channel %ld is outside [-1, %d) (-1 = downmix)", r, q[9], channels);
            if (chans) chans->push_back((int)q[9]);
        }
        RsClip c{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], tiles};
        SED_REQUIRE(c.in_off >= 0 && c.n_in >= 0 && c.in_off <= x_frames && c.n_in <= x_frames - c.in_off,
                    "resample: clip %d (first frame %ld, %ld frames) is not inside the input buffer of %ld frames", r, c.in_off, c.n_in, x_frames);
        SED_REQUIRE(c.in_base >= 0 && c.in_base < lim && c.out_first >= 0 && c.out_first < lim && c.n_out >= 0 && c.n_out < (1L << 40),
                    "resample: clip %d: bad counts (input base %ld, first output %ld, %ld outputs)", r, c.in_base, c.out_first, c.n_out);
        SED_REQUIRE(c.out_off >= out_end && (c.out_off & 3) == 0 && c.out_off <= out_len && c.n_out <= out_len - c.out_off,
                    "resample: clip %d: outputs [%ld, +%ld) must follow the previous clip's, start on a 16-byte boundary and lie inside "
                    "the buffer of %ld samples", r, c.out_off, c.n_out, out_len);
        SED_REQUIRE(c.n_hist >= 0 && c.n_hist <= c.in_base && c.hist_off >= 0 && c.hist_off <= hist_len && c.n_hist <= hist_len - c.hist_off,
                    "resample: clip %d: history [%ld, +%ld) is not inside the buffer of %ld samples (or reaches before sample 0)", r,
                    c.hist_off, c.n_hist, hist_len);
        // what lies before the history is read as zero: that is only right before the clip's sample 0
        if (c.n_out > 0 && c.in_base - c.n_hist > 0)
            SED_REQUIRE(c.out_first * M / L - half + 1 >= c.in_base - c.n_hist,
                        "resample: clip %d: output %ld needs sample %ld, the history begins at %ld", r, c.out_first,
                        c.out_first * M / L - half + 1, c.in_base - c.n_hist);
        if (c.carry_dst != -1) {
            SED_REQUIRE(c.carry_dst >= 0 && c.carry_dst <= hist_len && n_carry <= hist_len - c.carry_dst,
                        "resample: clip %d: carry [%ld, +%ld) is not inside the history buffer of %ld samples", r, c.carry_dst, n_carry, hist_len);
            SED_REQUIRE(c.n_hist == 0 || c.carry_dst + n_carry <= c.hist_off || c.hist_off + c.n_hist <= c.carry_dst,
                        "resample: clip %d: the carry would overwrite the history it is made from", r);
            SED_REQUIRE(c.n_hist == c.in_base || c.in_base + c.n_in - n_carry >= c.in_base - c.n_hist,
                        "resample: clip %d: the carry reaches before its history", r);
        }
        out_end = c.out_off + c.n_out;
        tiles += (c.n_out + RS_TILE - 1) / RS_TILE;
        if (recs) recs->push_back(c);
    }
    if (n_tiles) *n_tiles = tiles;
    return 0;
}

// the host table as the launch will see it: no GPU call
extern "C" int sed_resample_check_table(const long* rows_host, int R, long x_frames, long hist_len, long out_len, int L, int M, int half) {
    return rs_check_table(rows_host, R, RS_ROW, 1, x_frames, hist_len, out_len, L, M, half, nullptr, nullptr, nullptr);
}

// ... of sed_resample_select's table [R][10]: additionally refuses a channel outside [-1, channels)
extern "C" int sed_resample_select_check_table(const long* rows_host, int R, int channels, long x_frames, long hist_len, long out_len,
                                               int L, int M, int half) {
    SED_REQUIRE(channels >= 1 && channels <= 64, "resample: 1 to 64 interleaved channels, got %d", channels);
    return rs_check_table(rows_host, R, RS_ROW_SELECT, channels, x_frames, hist_len, out_len, L, M, half, nullptr, nullptr, nullptr);
}

static int rs_run(const void* x, long x_frames, int format, int channels, float* hist, long hist_len, const float* taps, long taps_len,
                  int L, int M, int half, const long* rows_host, int row_len, int R, float* out, long out_len, void* workspace,
                  size_t workspace_bytes, void* stream) {
    const bool select = row_len == RS_ROW_SELECT;
    SED_REQUIRE(taps && rows_host && workspace, "resample: null pointer");
    SED_REQUIRE(format == 0 || format == 1, "resample: format must be 0 (float32) or 1 (int16), got %d", format);
    SED_REQUIRE(channels >= 1 && channels <= 64, "resample: 1 to 64 interleaved channels, got %d", channels);
    std::vector<RsClip> recs;
    std::vector<int> chans;
    long n_tiles = 0;
    if (int rc = rs_check_table(rows_host, R, row_len, channels, x_frames, hist_len, out_len, L, M, half, &recs, &chans, &n_tiles)) return rc;
    const size_t need = select ? sed_resample_select_workspace_bytes(R) : sed_resample_workspace_bytes(R);
    SED_REQUIRE(workspace_bytes >= need, "resample: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE((x || x_frames == 0) && (hist || hist_len == 0) && (out || out_len == 0), "resample: null pointer");
    SED_REQUIRE(taps_len == (long)L * 2 * half, "resample: the tap table has %ld floats, %d phases x %d taps make %ld", taps_len, L, 2 * half,
                (long)L * 2 * half);
    SED_REQUIRE(n_tiles <= 0x7fffffffL, "resample: more than 2^31 - 1 tiles in one launch");
    bool any_carry = false;
    for (const RsClip& c : recs) any_carry |= c.carry_dst >= 0;
    if (n_tiles == 0 && !any_carry) return 0;
    hipStream_t s = as_stream(stream);
    RsClip* dev = (RsClip*)workspace;
    hipError_t e = hipMemcpyAsync(dev, recs.data(), recs.size() * sizeof(RsClip), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("resample: upload of the clip table: %s", hipGetErrorString(e)); return (int)e; }
    const int* chan = nullptr;                                       // sed_resample: no channel table, every row downmixes
    if (select) {
        chan = reinterpret_cast<const int*>(dev + R);
        e = hipMemcpyAsync((void*)chan, chans.data(), chans.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { sed_set_error("resample: upload of the channel table: %s", hipGetErrorString(e)); return (int)e; }
    }
    if (n_tiles) {
        const size_t lds = ((size_t)L * (2 * half + 1) + (size_t)rs_span(RS_TILE, L, M, half)) * sizeof(float);
        const void* fn = format ? (const void*)resample_k<1> : (const void*)resample_k<0>;
        e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) { sed_set_error("resample: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        const long resident = 256L * (2 * lds <= (size_t)160 * 1024 ? 2 : 1);      // persistent: the taps are loaded once each
        const unsigned blocks = (unsigned)(n_tiles < resident ? n_tiles : resident);
        if (format) resample_k<1><<<blocks, RS_TILE, lds, s>>>(x, channels, hist, taps, L, M, half, dev, chan, R, n_tiles, out);
        else resample_k<0><<<blocks, RS_TILE, lds, s>>>(x, channels, hist, taps, L, M, half, dev, chan, R, n_tiles, out);
        SED_LAUNCH_CHECK("resample");
    }
    if (any_carry) {
        if (format) resample_carry_k<1><<<(unsigned)R, 128, 0, s>>>(x, channels, hist, dev, chan, 2 * half);
        else resample_carry_k<0><<<(unsigned)R, 128, 0, s>>>(x, channels, hist, dev, chan, 2 * half);
        SED_LAUNCH_CHECK("resample_carry");
    }
    return 0;
}

extern "C" int sed_resample(const void* x, long x_frames, int format, int channels, float* hist, long hist_len, const float* taps,
                            long taps_len, int L, int M, int half, const long* rows_host, int R, float* out, long out_len, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return rs_run(x, x_frames, format, channels, hist, hist_len, taps, taps_len, L, M, half, rows_host, RS_ROW, R, out, out_len, workspace,
                  workspace_bytes, stream);
}

// sed_resample with a tenth column per row: the channel the row keeps (-1 = the downmix of sed_resample)
extern "C" int sed_resample_select(const void* x, long x_frames, int format, int channels, float* hist, long hist_len, const float* taps,
                                   long taps_len, int L, int M, int half, const long* rows_host, int R, float* out, long out_len,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return rs_run(x, x_frames, format, channels, hist, hist_len, taps, taps_len, L, M, half, rows_host, RS_ROW_SELECT, R, out, out_len,
                  workspace, workspace_bytes, stream);
}
