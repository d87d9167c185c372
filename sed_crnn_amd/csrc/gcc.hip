// gcc.hip — GCC-PHAT spatial features beside the multichannel log-mel: sed_logmel_gcc.
//
// For a recording of C >= 2 channels, frame f and microphone pair (i, j), i < j in lexicographic order:
//   G[k] = X_i[k] conj X_j[k],  Pk[k] = G[k] / |G[k]| (0 where |G|^2 < 1e-30),
//   cc[tau] = (1/2048) (Pk[0] + (-1)^tau Pk[1024] + 2 sum_{k=1..1023} Re(Pk[k] e^{+2 pi i k tau / 2048})),  tau = -L/2 .. L/2-1,
// stacked behind the C mel images: out [rows][C n_mels + P n_lags], column C n_mels + p n_lags + tau + L/2.
//
// Shape (gfx950).  The mel columns are written by the multichannel log-mel launch itself with a wider row stride
// (sed_internal_logmel_multi): they are that kernel's code and bits.  The GCC columns come from a second kernel in which ONE
// workgroup of 8 waves owns one frame at a time:
//   1. FFT: wave w < ceil(C/2) transforms channels 2w and 2w+1 of the frame, one per half wave, with the register-resident
//      2048-point real FFT of fft2048.h, and leaves the C spectra (1025 complex floats each) in LDS;
//   2. for as many pairs at a time as fit in LDS: all 512 lanes turn spectra into the whitened cross spectra Pk (one v_rsq per
//      bin), then
//   3. lag synthesis as a direct sum: only L of the 2048 inverse-transform outputs are wanted, and cc[+tau] and cc[-tau] share
//      their products (A = sum Re Pk cos, B = sum Im Pk sin: cc[+-tau] = A -+ B).  Eight neighbouring lanes own one (pair, tau):
//      lane j sums the bins k = j, j+8, ... in ascending order against a 2048-entry cos/sin table in LDS (exact table values at
//      index k tau mod 2048: no recurrences), the eight partial sums are combined by three xor-shuffles.
// Steps 2 and 3 are phat_bin and phat_lag_sum of phat_shared.h, which per-event TDOA and DOA call too.
// Every output is therefore summed in one fixed order that depends on nothing but the frame's samples: not on the batch, the
// clip's place in the buffer or the launch shape.
#include <math.h>
#include <string.h>
#include <vector>
#include "common.h"
#include "fft2048.h"
#include "phat_shared.h"

#define GC_WAVES 8                                // (4 waves: 27.2 ms instead of 24.8 for the hour of 4-channel audio of DESIGN 5m)
#define GC_THREADS (GC_WAVES * 64)
#define GC_MAX_CH 8
#define GC_TAB_WORDS LM_OFF_ENT                   // of the log-mel blob: header, window, inter-pass and pairing twiddles
#define GC_LAG_WORDS (2 * LM_NFFT)                // LDS floats of the lag table (cos, sin)(2 pi m / 2048), m = 0..2047
#define GC_FFT_SCR (2 * LM_SCR)                   // floats of exchange scratch per transforming wave (>= 32 x 65)
#define GC_LDS_MAX ((size_t)160 * 1024)

namespace {

struct GcArgs {
    const long* row_off;        // [R+1] first output row of each recording; the last entry is the total
    const long* sample_off;     // [R*C] first sample of every planar channel
    const long* n_samples;      // [R]   samples per channel
    int R, C, P, pairs_per_batch;
    long rows;
    int col0, row_stride, n_lags;
};

__global__ __launch_bounds__(GC_THREADS) void gcc_phat_k(const float* __restrict__ pcm, const uint32_t* __restrict__ tables,
                                                         const float* __restrict__ mu, const float* __restrict__ inv_sigma,
                                                         float* __restrict__ out, int hop, int pad_mode, GcArgs ga) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    fft_stage_tables(lds, tables, GC_TAB_WORDS, tid, GC_THREADS);     // once per (persistent) workgroup
    __syncthreads();
    // the lag table, unfolded from the blob's pairing twiddles: nothing is computed or uploaded per call
    phat_lag_table(reinterpret_cast<float2*>(lds + GC_TAB_WORDS), reinterpret_cast<const float2*>(lds + LM_OFF_PW), tid, GC_THREADS);
    __syncthreads();
    const f2* s_win = reinterpret_cast<const f2*>(lds + LM_OFF_WIN);
    const f2* s_tw = reinterpret_cast<const f2*>(lds + LM_OFF_TW);
    const f2* s_pw = reinterpret_cast<const f2*>(lds + LM_OFF_PW);
    const float2* s_lag = reinterpret_cast<const float2*>(lds + GC_TAB_WORDS);
    float2* s_spec = reinterpret_cast<float2*>(lds + GC_TAB_WORDS + GC_LAG_WORDS);           // [C][PHAT_SPEC]
    float* s_uni = lds + GC_TAB_WORDS + GC_LAG_WORDS + ga.C * PHAT_SPEC * 2;                 // FFT scratch, then Pk [batch][PHAT_SPEC]
    float2* s_pk = reinterpret_cast<float2*>(s_uni);

    const int C = ga.C, P = ga.P, L = ga.n_lags, T = L / 2 + 1;
    const int wave = tid >> 6;
    const int nfw = (C + 1) >> 1;                                // waves that transform
    float* wscr = s_uni + wave * GC_FFT_SCR;                     // (only used by waves < nfw)
    const FftLane fl = fft_lane(tid & 63, wscr - lds);
    const int half = fl.half(), r = fl.r();
    float* scr = wscr + half * LM_SCR;

    for (long row = blockIdx.x; row < ga.rows; row += gridDim.x) {
        int lo = 0, hi = ga.R - 1;                               // the last recording whose first row is <= row (block-uniform)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ga.row_off[mid] <= row) lo = mid;
            else hi = mid - 1;
        }
        const int rec = lo;
        const long frame = row - ga.row_off[rec];
        const long ns = ga.n_samples[rec];

        if (wave < nfw) {
            // ── the frame of channel 2 wave + half (an odd C: the last half wave repeats channel C-1 and stores the same values) ──
            const int ch = (2 * wave + half < C) ? 2 * wave + half : C - 1;
            const float* cpcm = pcm + ga.sample_off[(long)rec * C + ch];
            const long start = frame * hop - LM_NFFT / 2;
            const bool fast = (hop & 1) == 0 && (reinterpret_cast<uintptr_t>(cpcm) & 7) == 0 && start >= 0 && start + LM_NFFT <= ns;
            f2 z[32];                                            // z[n] = (x[2n], x[2n+1]): one complex point per VGPR pair
            if (__all(fast)) {
                const f2* src = reinterpret_cast<const f2*>(cpcm + start) + r;
#pragma unroll
                for (int n1 = 0; n1 < 32; ++n1) z[n1] = src[32 * n1];
            } else {                                             // edge frames / odd hop / unaligned clips
                fft_load_guarded(z, scr, fl, [&](int off) { return pcm_at(cpcm, start + off, ns, pad_mode); });
            }
            fft2048_passes(z, fl, s_win, s_tw);
            fft2048_spectrum(z, fl, s_pw, s_spec + ch * PHAT_SPEC);
        }
        __syncthreads();

        for (int p0 = 0; p0 < P; p0 += ga.pairs_per_batch) {
            const int nb = (P - p0 < ga.pairs_per_batch) ? P - p0 : ga.pairs_per_batch;
            // ── Pk of the batch's pairs ──
            for (int idx = tid; idx < nb * 1025; idx += GC_THREADS) {
                const int pb = idx / 1025, k = idx - pb * 1025;
                int i, j;
                phat_pair(p0 + pb, C, i, j);
                s_pk[pb * PHAT_SPEC + k] = phat_bin(s_spec[i * PHAT_SPEC + k], s_spec[j * PHAT_SPEC + k], k);
            }
            __syncthreads();
            // ── lag synthesis: item = (pair of the batch, tau = 0..L/2), 8 lanes per item ──
            const int grp = tid >> 3, j8 = tid & 7, n_items = nb * T;
            for (int it0 = 0; it0 < n_items; it0 += GC_THREADS / 8) {
                const bool valid = it0 + grp < n_items;
                const int item = valid ? it0 + grp : 0;
                const int pb = item / T, tau = item - pb * T;
                const float2* pk = s_pk + pb * PHAT_SPEC;
                const float2 ab = phat_lag_sum(pk, j8, tau, LM_NFFT, [&](int m) { return s_lag[m]; });
                const float A = ab.x, B = ab.y;
                // lane 0 of the group stores cc[+tau] = A - B, lane 1 cc[-tau] = A + B
                if (valid && j8 < 2) {
                    const float ny = pk[LM_N].x, sgn = (tau & 1) ? -ny : ny;
                    const bool plus = j8 == 0;
                    const int col = plus ? L / 2 + tau : L / 2 - tau;
                    if (plus ? (tau < L / 2) : (tau > 0)) {
                        float v = (2.f * (plus ? A - B : A + B) + sgn) * (1.f / LM_NFFT);
                        const int c = ga.col0 + (p0 + pb) * L + col;
                        if (mu) v = (v - mu[c]) * inv_sigma[c];
                        out[row * ga.row_stride + c] = v;
                    }
                }
            }
            __syncthreads();                                     // Pk (and, behind the last batch, the spectra) may be overwritten
        }
    }
}

// LDS of the kernel for C channels with `batch` pairs of Pk resident
size_t gcc_lds_bytes(int C, int batch) {
    const size_t fft = (size_t)((C + 1) / 2) * GC_FFT_SCR, pk = (size_t)batch * PHAT_SPEC * 2;
    return ((size_t)GC_TAB_WORDS + GC_LAG_WORDS + (size_t)C * PHAT_SPEC * 2 + (fft > pk ? fft : pk)) * sizeof(float);
}

// 64-bit words of row_off [R+1], sample_off [R*C] and n_samples [R]
size_t gcc_table_longs(int R, int channels) { return (size_t)R + 1 + (size_t)R * channels + R; }

}  // namespace

// workspace: sed_logmel_multi's clip tables, then row_off [R+1], sample_off [R*C], n_samples [R] (64-bit)
extern "C" size_t sed_logmel_gcc_workspace_bytes(int R, int channels) {
    if (channels < 2 || channels > GC_MAX_CH) return 0;
    const size_t multi = sed_logmel_multi_workspace_bytes(R, channels);
    if (multi == 0) return 0;
    return ((multi + 15) & ~(size_t)15) + gcc_table_longs(R, channels) * sizeof(long);
}

extern "C" int sed_logmel_gcc(const float* pcm, long pcm_len, const long* clips_host, int R, int channels, const void* tables,
                              size_t tables_bytes, const float* mu, const float* inv_sigma, float* out, long out_rows, int n_fft, int hop,
                              int n_mels, int n_lags, int pad_mode, void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(channels >= 2 && channels <= GC_MAX_CH, "logmel_gcc: 2 to %d channels, got %d", GC_MAX_CH, channels);
    SED_REQUIRE(n_lags >= 2 && n_lags <= LM_MAX_MELS && (n_lags & 1) == 0, "logmel_gcc: n_lags must be even and in [2,%d], got %d",
                LM_MAX_MELS, n_lags);
    SED_REQUIRE(n_fft == LM_NFFT, "logmel_gcc: n_fft must be %d (got %d)", LM_NFFT, n_fft);
    SED_REQUIRE(hop > 0 && n_mels > 0 && n_mels <= LM_MAX_MELS, "logmel_gcc: bad sizes");
    SED_REQUIRE(pcm && clips_host && tables && out && workspace, "logmel_gcc: null pointer");
    const size_t need = sed_logmel_gcc_workspace_bytes(R, channels);
    SED_REQUIRE(need > 0 && pcm_len > 0, "logmel_gcc: bad sizes (R=%d, channels=%d, pcm_len=%ld)", R, channels, pcm_len);
    SED_REQUIRE(workspace_bytes >= need, "logmel_gcc: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(((uintptr_t)workspace & 7) == 0, "logmel_gcc: workspace must be 8-byte aligned");
    SED_REQUIRE(tables_bytes % 16 == 0 && tables_bytes / 4 >= (size_t)GC_TAB_WORDS, "logmel_gcc: table blob of %zu bytes is malformed", tables_bytes);
    const int P = channels * (channels - 1) / 2;
    const int row_stride = channels * n_mels + P * n_lags;

    // the recordings: bounds and equal channel lengths, on the host, before anything is enqueued
    const size_t n_long = gcc_table_longs(R, channels);
    std::vector<long> h(n_long);
    long *row_off = h.data(), *soff = row_off + R + 1, *slen = soff + (size_t)R * channels;
    long rows = 0;
    for (int r = 0; r < R; ++r) {
        const long n0 = clips_host[2 * ((long)r * channels) + 1];
        for (int ch = 0; ch < channels; ++ch) {
            const long c = (long)r * channels + ch, o = clips_host[2 * c], n = clips_host[2 * c + 1];
            SED_REQUIRE(o >= 0 && n >= 1 && o <= pcm_len && n <= pcm_len - o,
                        "logmel_gcc: recording %d, channel %d (offset %ld, %ld samples) is not inside the PCM buffer of %ld samples", r, ch,
                        o, n, pcm_len);
            SED_REQUIRE(n == n0, "logmel_gcc: recording %d: channel %d has %ld samples, channel 0 has %ld (the channels of a recording "
                        "must have equal length)", r, ch, n, n0);
            soff[c] = o;
        }
        row_off[r] = rows; slen[r] = n0;
        rows += 1 + n0 / hop;
        SED_REQUIRE(rows <= 0x7fffffffL, "logmel_gcc: more than 2^31 - 1 feature frames in one batch");
    }
    row_off[R] = rows;
    SED_REQUIRE(out_rows == rows, "logmel_gcc: out has %ld rows, the recordings make %ld", out_rows, rows);

    // as many pairs of Pk at a time as LDS holds beside the tables and the C spectra
    int batch = P;
    while (batch > 1 && gcc_lds_bytes(channels, batch) > GC_LDS_MAX) --batch;
    const size_t lds = gcc_lds_bytes(channels, batch);
    SED_REQUIRE(lds <= GC_LDS_MAX, "logmel_gcc: %d spectra and the tables (%zu B) exceed the 160 KiB LDS", channels, lds);

    // mel columns: the multichannel log-mel launch with this matrix's row stride
    const size_t multi = (sed_logmel_multi_workspace_bytes(R, channels) + 15) & ~(size_t)15;
    if (int rc = sed_internal_logmel_multi(pcm, pcm_len, clips_host, R, channels, tables, tables_bytes, mu, inv_sigma, out, out_rows, n_fft,
                                           hop, n_mels, pad_mode, row_stride, workspace, multi, stream)) return rc;

    hipStream_t s = as_stream(stream);
    char* dev = (char*)workspace + multi;
    hipError_t e = hipMemcpyAsync(dev, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("logmel_gcc: upload of the recording table: %s", hipGetErrorString(e)); return (int)e; }
    const long* dl = (const long*)dev;
    GcArgs ga{dl, dl + R + 1, dl + R + 1 + (size_t)R * channels, R, channels, P, batch, rows,
              channels * n_mels, row_stride, n_lags};
    e = hipFuncSetAttribute((const void*)gcc_phat_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GC_LDS_MAX);
    if (e != hipSuccess) { sed_set_error("logmel_gcc: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    const long resident = 256 * (lds <= GC_LDS_MAX / 2 ? 2 : 1);  // persistent workgroups: the tables are loaded once each
    const long blocks = rows < resident ? rows : resident;
    SedProfScope prof(SED_K_LOGMEL, s, (double)rows * ((double)hop * channels + (double)P * n_lags) * 4.0);
    gcc_phat_k<<<(unsigned)blocks, GC_THREADS, lds, s>>>(pcm, (const uint32_t*)tables, mu, inv_sigma, out, hop, pad_mode, ga);
    SED_LAUNCH_CHECK("logmel_gcc");
    return 0;
}
