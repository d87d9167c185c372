// pcen.hip — per-channel energy normalisation of log-mel columns, in place.
//
// A column of log-mel values x[t] is one chain: E[t] = scale * exp(x[t]), the smoother M[t] = (1-b) M[t-1] + b E[t] with
// M[0] = E[0], and pcen[t] = (E[t] (eps + M[t])^-gain + bias)^power - bias^power, then the scaler.
//
// The smoother is evaluated in blocks of PC_L frames ALIGNED TO THE ABSOLUTE FRAME INDEX, so that the fp32 operations behind
// M[t] are a function of t and the data alone — never of where a call starts or ends:
//   loc[t] = a loc[t-1] + b E[t]            from 0 at every block start kL            (pass 1 and 3, one lane per block and column)
//   C_k    = a^L C_{k-1} + loc[kL - 1]      C_0 = E[0]                                (pass 2, one lane per chain)
//   M[t]   = a^(t - kL + 1) C_k + loc[t]                                              (pass 3)
// A chain's state between calls is (C_k, loc[t]) of its last frame.  Three plain launches; no workgroup waits on another.
#include <math.h>

#include <vector>

#include "common.h"

namespace {

constexpr int PC_L = 64;              // frames per block; tests/test_gpu_pcen.py reads the same number from feature.PCEN_BLOCK
constexpr int PC_THREADS = 256;
constexpr int PC_MAX_W = 1 << 16, PC_MAX_R = 1 << 24;

struct PcArgs {
    const long* unit_off;             // [R+1] first work unit (= touched block) of every recording
    const long* recs;                 // [R][3] first row, n rows, absolute index of the first frame
    long units;
    int R, W, col0, stride;
    float b, gain, bias, power, eps, scale;
    float pw[PC_L];                   // pw[j] = (1-b)^(j+1), rounded from double
};

__device__ __forceinline__ float pc_energy(const PcArgs& a, float x) { return __fmul_rn(a.scale, expf(x)); }

// Pass 1 (APPLY = false): loc at the last processed frame of every (block, column) -> blockend; the loc a call starts from
// (the state's, or 0 at a block start) -> loc0.  Pass 3 (APPLY = true): the same recurrence again, M and the output.
// Lanes run along columns: lane = unit * W + column.
template <bool APPLY>
__global__ __launch_bounds__(PC_THREADS) void pcen_pass_k(float* __restrict__ x, const float* __restrict__ state, float* __restrict__ loc0,
                                                          float* __restrict__ blockend, const float* __restrict__ carry,
                                                          const float* __restrict__ mu, const float* __restrict__ inv_sigma, const PcArgs a) {
    const long idx = (long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (idx >= a.units * a.W) return;
    const long u = idx / a.W;
    const int c = (int)(idx - u * a.W);
    int lo = 0, hi = a.R;                                        // unit_off[lo] <= u < unit_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.unit_off[mid] <= u) lo = mid; else hi = mid;
    }
    const int r = lo;
    const long row0 = a.recs[3 * r], n = a.recs[3 * r + 1], t0 = a.recs[3 * r + 2];
    const bool first = u == a.unit_off[r];
    const long tb = (t0 / PC_L + (u - a.unit_off[r])) * PC_L;    // absolute frame of j = 0
    const int j0 = t0 > tb ? (int)(t0 - tb) : 0;
    const int j1 = t0 + n < tb + PC_L ? (int)(t0 + n - tb) : PC_L;
    const long chain = (long)r * a.W + c;

    float loc = 0.f;
    if (APPLY) {
        if (first) loc = loc0[chain];
    } else if (first) {
        if (j0 > 0) loc = state[2 * chain + 1];                  // the call continues a block (host: state is not NULL then)
        loc0[chain] = loc;
    }
    const float C = APPLY ? carry[idx] : 0.f;
    const float bp = APPLY ? powf(a.bias, a.power) : 0.f;
    float* p = x + (row0 + (tb - t0)) * (long)a.stride + a.col0 + c;   // row of j = 0 (only rows j0 <= j < j1 are touched)

    for (int jo = 0; jo < PC_L; jo += 8) {
        if (jo + 8 <= j0 || jo >= j1) continue;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = jo + i;
            v[i] = (j >= j0 && j < j1) ? p[(long)j * a.stride] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = jo + i;
            if (j >= j0 && j < j1) {
                const float E = pc_energy(a, v[i]);
                loc = __fmaf_rn(a.pw[0], loc, __fmul_rn(a.b, E));
                if (APPLY) {
                    const float M = __fmaf_rn(a.pw[j], C, loc);
                    // E = 0 (digital silence) is 0 whatever the gain term: eps^-gain may be inf for a large gain
                    const float g = E == 0.f ? 0.f : __fmul_rn(E, powf(a.eps + M, -a.gain));
                    float y = powf(g + a.bias, a.power) - bp;
                    if (mu) y = (y - mu[c]) * inv_sigma[c];
                    p[(long)j * a.stride] = y;
                }
            }
        }
    }
    if (!APPLY) blockend[idx] = loc;
}

// Pass 2: the per-block carries of every chain, in block order; then the chain's new state.
__global__ __launch_bounds__(PC_THREADS) void pcen_carry_k(const float* __restrict__ x, float* __restrict__ state,
                                                           const float* __restrict__ blockend, float* __restrict__ carry, const PcArgs a) {
    const long chain = (long)blockIdx.x * PC_THREADS + threadIdx.x;
    if (chain >= (long)a.R * a.W) return;
    const int r = (int)(chain / a.W), c = (int)(chain - (long)r * a.W);
    const long row0 = a.recs[3 * r], n = a.recs[3 * r + 1], t0 = a.recs[3 * r + 2];
    if (n == 0) return;
    const long u0 = a.unit_off[r], nu = a.unit_off[r + 1] - u0;
    const float aL = a.pw[PC_L - 1];
    float C;
    if (t0 == 0) {
        C = pc_energy(a, x[row0 * (long)a.stride + a.col0 + c]);               // C_0 = E[0]; the state is not read
    } else {
        C = state[2 * chain];
        if (t0 % PC_L == 0) C = __fmaf_rn(aL, C, state[2 * chain + 1]);        // the call starts a block
    }
    const float* be = blockend + u0 * a.W + c;
    float* cy = carry + u0 * a.W + c;
    cy[0] = C;
#pragma unroll 8
    for (long i = 1; i < nu; ++i) {
        C = __fmaf_rn(aL, C, be[(i - 1) * a.W]);
        cy[i * a.W] = C;
    }
    if (state) {
        state[2 * chain] = C;
        state[2 * chain + 1] = be[(nu - 1) * a.W];
    }
}

size_t pc_table_bytes(int R) { return (((size_t)R + 1 + 3 * (size_t)R) * sizeof(long) + 15) & ~(size_t)15; }

}  // namespace

// workspace: unit_off [R+1] and recs [R][3] (64-bit), then blockend and carry [units][W] for at most rows/PC_L + 2R units
// (a recording of n >= 1 rows touches at most (n - 1)/PC_L + 2 blocks) and loc0 [R][W]
extern "C" size_t sed_pcen_workspace_bytes(long rows, int R, int W) {
    if (rows < 0 || rows > 0x7fffffffL || R < 0 || R > PC_MAX_R || W < 1 || W > PC_MAX_W) return 0;
    const size_t units = (size_t)rows / PC_L + 2 * (size_t)R;
    return pc_table_bytes(R) + (2 * units + (size_t)R) * (size_t)W * sizeof(float);
}

extern "C" int sed_pcen(float* x, long rows, int stride, int col0, int W, const long* recs_host, int R, float* state, double smooth_b,
                        float gain, float bias, float power, float eps, float scale, const float* mu, const float* inv_sigma,
                        void* workspace, size_t workspace_bytes, void* stream) {
    SED_REQUIRE(x && recs_host && workspace, "pcen: null pointer");
    SED_REQUIRE(rows >= 0 && rows <= 0x7fffffffL && R >= 0 && R <= PC_MAX_R, "pcen: bad sizes (rows=%ld, R=%d)", rows, R);
    SED_REQUIRE(stride >= 1 && col0 >= 0 && W >= 1 && W <= PC_MAX_W && (long)col0 + W <= (long)stride,
                "pcen: columns [%d, %d + %d) are not inside a row of %d floats", col0, col0, W, stride);
    SED_REQUIRE((mu == nullptr) == (inv_sigma == nullptr), "pcen: give both mu and inv_sigma (%d wide) or neither", W);
    SED_REQUIRE(smooth_b > 0.0 && smooth_b <= 1.0, "pcen: the smoothing coefficient must lie in (0, 1], got %g", smooth_b);
    SED_REQUIRE(gain > 0.f && gain < INFINITY && bias >= 0.f && bias < INFINITY && power > 0.f && power < INFINITY && eps > 0.f &&
                eps < INFINITY && scale > 0.f && scale < INFINITY,
                "pcen: need finite gain > 0, bias >= 0, power > 0, eps > 0, scale > 0 (got %g, %g, %g, %g, %g)", gain, bias, power, eps, scale);
    const size_t need = sed_pcen_workspace_bytes(rows, R, W);
    SED_REQUIRE(need > 0 && workspace_bytes >= need, "pcen: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    SED_REQUIRE(((uintptr_t)workspace & 7) == 0, "pcen: workspace must be 8-byte aligned");

    // the recordings: inside the matrix, disjoint, in increasing order; on the host, before anything is enqueued
    std::vector<long> h((size_t)R + 1 + 3 * (size_t)R);
    long *unit_off = h.data(), *recs = unit_off + R + 1;
    long units = 0, end = 0;
    for (int r = 0; r < R; ++r) {
        const long first = recs_host[3 * (long)r], n = recs_host[3 * (long)r + 1], t0 = recs_host[3 * (long)r + 2];
        SED_REQUIRE(first >= 0 && n >= 0 && first <= rows && n <= rows - first,
                    "pcen: recording %d (first row %ld, %ld rows) is not inside the matrix of %ld rows", r, first, n, rows);
        SED_REQUIRE(t0 >= 0 && t0 <= (1L << 46), "pcen: recording %d: the absolute index of its first frame must lie in [0, 2^46], got %ld", r, t0);
        SED_REQUIRE(n == 0 || first >= end, "pcen: recording %d (first row %ld) overlaps the one before it, which ends at row %ld "
                    "(the recordings must be disjoint and in increasing order)", r, first, end);
        SED_REQUIRE(n == 0 || t0 == 0 || state, "pcen: recording %d continues at frame %ld and needs the state buffer", r, t0);
        unit_off[r] = units;
        recs[3 * r] = first; recs[3 * r + 1] = n; recs[3 * r + 2] = t0;
        if (n > 0) {
            units += (t0 + n - 1) / PC_L - t0 / PC_L + 1;
            end = first + n;
        }
    }
    unit_off[R] = units;
    if (units == 0) return 0;
    SED_REQUIRE((size_t)units <= (size_t)rows / PC_L + 2 * (size_t)R, "pcen: internal: %ld work units exceed the workspace plan", units);
    SED_REQUIRE(units * W < (1L << 39) && (long)R * W < (1L << 39), "pcen: %ld blocks / %d recordings of %d columns are more than one launch takes",
                units, R, W);

    hipStream_t s = as_stream(stream);
    char* dev = (char*)workspace;
    hipError_t e = hipMemcpyAsync(dev, h.data(), h.size() * sizeof(long), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { sed_set_error("pcen: upload of the recording table: %s", hipGetErrorString(e)); return (int)e; }
    const long* dl = (const long*)dev;
    const size_t max_units = (size_t)rows / PC_L + 2 * (size_t)R;
    float* blockend = (float*)(dev + pc_table_bytes(R));
    float* carry = blockend + max_units * W;
    float* loc0 = carry + max_units * W;

    PcArgs a;
    a.unit_off = dl; a.recs = dl + R + 1; a.units = units;
    a.R = R; a.W = W; a.col0 = col0; a.stride = stride;
    a.b = (float)smooth_b; a.gain = gain; a.bias = bias; a.power = power; a.eps = eps; a.scale = scale;
    for (int j = 0; j < PC_L; ++j) a.pw[j] = (float)pow(1.0 - smooth_b, (double)(j + 1));

    const unsigned grid = (unsigned)((units * W + PC_THREADS - 1) / PC_THREADS);
    const unsigned grid_c = (unsigned)(((long)R * W + PC_THREADS - 1) / PC_THREADS);
    pcen_pass_k<false><<<grid, PC_THREADS, 0, s>>>(x, state, loc0, blockend, nullptr, nullptr, nullptr, a);
    SED_LAUNCH_CHECK("pcen (local pass)");
    pcen_carry_k<<<grid_c, PC_THREADS, 0, s>>>(x, state, blockend, carry, a);
    SED_LAUNCH_CHECK("pcen (carries)");
    pcen_pass_k<true><<<grid, PC_THREADS, 0, s>>>(x, nullptr, loc0, nullptr, carry, mu, inv_sigma, a);
    SED_LAUNCH_CHECK("pcen (apply)");
    return 0;
}
