// gemm.hip — dense fp32 GEMM on v_mfma_f32_32x32x2_f32 + the small time-distributed dense head.
//
// Replaces aten::mm / addmm under nn.GRU's input projections and nn.Linear (reference
// sed.py:101-103,111-112; crnn_lightning.py:61-64,71-73) and their autograd transposes.
// The GRU input projection (M=B*T', K=C*F, N=3H) is the one genuine dense GEMM of the path, hence MFMA.
// fp32 in / fp32 accumulate, no reduced precision.  The chain of an output element is NOT k-ordered: within each group of 8
// the MFMA takes k = 8g+j from lanes 0-31 and k = 8g+4+j from lanes 32-63 (j = 0..3).  What holds is one fixed order of
// summation, the same for every tile, layout and FULL / guarded path, so a row's bits do not depend on the plan its call got
// (tests/test_gpu_gemm_tiles.py: test_one_summation_order_whatever_the_tile).
#include <type_traits>
#include "common.h"

#define GM_BK 32
#define GM_LDK 36   // k-contiguous LDS row: 32 + 4 pad floats (16-B slot stride 9) -> conflict-free ds_read_b128

// A_KC / B_KC: operand is contiguous along k (true) or along m/n (false).
// Block tile (32*WM*WVM) x (32*WN*WVN), 4 waves as WVM x WVN, each wave WM x WN tiles of 32x32 (v_mfma_f32_32x32x2_f32).
// Three-stage pipeline per K-step of 32: registers hold step k+1 (global loads issued a whole step earlier), LDS buffer
// `cur` holds step k.  Each iteration first writes the registers to the other LDS buffer and issues the loads of step
// k+2, then runs the MFMA block of step k, so the LDS writes and the global latency are covered by MFMA work and the one
// barrier per step has nothing outstanding.  Inside a step the fragments of k-group g+1 are read while the MFMAs of
// group g issue.  FULL = interior tile with aligned operands and K a multiple of 32: loads without range tests (the
// guarded variant costs ~1000 scalar/branch instructions per step, which a lone wave per SIMD cannot hide).
template <bool KC, int NR, int TILE>
__device__ __forceinline__ void gm_load(f32x4* reg, const float* __restrict__ P, long s_mn, long s_k, int mn0, int MN,
                                        int K, int vec, int k0, int tid) {
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        int i = tid + u * 256;
        f32x4 v = {0, 0, 0, 0};
        if (KC) {
            int row = i >> 3, kq = i & 7;
            int m = mn0 + row, k = k0 + kq * 4;
            const float* p = P + (long)m * s_mn + k;
            if (m < MN) {
                if (vec && k + 3 < K) v = *(const f32x4*)p;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (k + e < K) v[e] = p[e];
            }
        } else {
            int kk = i / (TILE / 4), mq = i - kk * (TILE / 4);
            int m = mn0 + mq * 4, k = k0 + kk;
            const float* p = P + (long)k * s_k + m;
            if (k < K) {
                if (vec && m + 3 < MN) v = *(const f32x4*)p;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (m + e < MN) v[e] = p[e];
            }
        }
        reg[u] = v;
    }
}
template <bool KC, int NR, int TILE>
__device__ __forceinline__ void gm_store(const f32x4* reg, float* S, int tid) {
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        int i = tid + u * 256;
        if (KC) { int row = i >> 3, kq = i & 7; *(f32x4*)(S + row * GM_LDK + kq * 4) = reg[u]; }
        else { int kk = i / (TILE / 4), mq = i - kk * (TILE / 4); *(f32x4*)(S + kk * TILE + mq * 4) = reg[u]; }
    }
}

template <int WVM, int WVN, int WM, int WN, bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) void gemm_f32_k(
    const float* __restrict__ A, long a_si, long a_sk, const float* __restrict__ Bm, long b_sk, long b_sj,
    float* __restrict__ C, long ldc, const float* __restrict__ bias, float beta, int M, int N, int Kfull,
    int a_vec, int b_vec, int k_len, long slab_stride) {
    static_assert(WVM * WVN == 4, "four waves per workgroup");
    constexpr int BM = 32 * WM * WVM, BN = 32 * WN * WVN;
    // split-K: blockIdx.z owns k in [kb, K) and writes its partial product to slab z of C
    const int kb = blockIdx.z * k_len;
    const int K = (kb + k_len < Kfull) ? kb + k_len : Kfull;
    C += (long)blockIdx.z * slab_stride;
    constexpr int A_FLOATS = A_KC ? BM * GM_LDK : GM_BK * BM;
    constexpr int B_FLOATS = B_KC ? BN * GM_LDK : GM_BK * BN;
    constexpr int NA = BM / 32, NB = BN / 32;         // float4 per thread per K-step (BM*32 floats / 256 threads / 4)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As0 = smem;                                // [2][A_FLOATS]
    float* Bs0 = smem + 2 * A_FLOATS;                 // [2][B_FLOATS]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2) in launch order, so the
    // launch index is mapped to a tile such that every XCD walks a contiguous run of tiles in row-major order: the column
    // tiles that share an A row-tile meet in one L2 instead of eight.
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int total = gridDim.x * gridDim.y, id = by * gridDim.x + bx;
        const int q = total >> 3, rr = total & 7, xcd = id & 7, seq = id >> 3;
        const int v = (xcd < rr) ? xcd * (q + 1) + seq : rr * (q + 1) + (xcd - rr) * q + seq;
        by = v / (int)gridDim.x;
        bx = v - by * (int)gridDim.x;
    }
    const int m0 = by * BM, n0 = bx * BN;
    const int wm0 = (wave / WVN) * 32 * WM, wn0 = (wave % WVN) * 32 * WN;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
        for (int u = 0; u < WN; ++u)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[t][u][j] = 0.f;

    auto read_frags = [&](const float* As, const float* Bs, int g, f32x4* af, f32x4* bf) {
#pragma unroll
        for (int t = 0; t < WM; ++t) {
            if (A_KC) af[t] = *(const f32x4*)(As + (wm0 + t * 32 + r) * GM_LDK + g * 8 + 4 * h);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j) af[t][j] = As[(g * 8 + 4 * h + j) * BM + wm0 + t * 32 + r];
        }
#pragma unroll
        for (int u = 0; u < WN; ++u) {
            if (B_KC) bf[u] = *(const f32x4*)(Bs + (wn0 + u * 32 + r) * GM_LDK + g * 8 + 4 * h);
            else
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[u][j] = Bs[(g * 8 + 4 * h + j) * BN + wn0 + u * 32 + r];
        }
    };
    auto mfma_group = [&](const f32x4* af, const f32x4* bf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < WM; ++t)
#pragma unroll
                for (int u = 0; u < WN; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t][j], bf[u][j], acc[t][u], 0, 0, 0);
    };

    auto run = [&](auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        f32x4 ra[NA], rb[NB];
        // FULL: per-thread source pointers, advanced by one K-step per load (two VALU adds instead of the full index math)
        const float* pa[NA];
        const float* pb[NB];
        const long a_step = A_KC ? GM_BK : GM_BK * a_sk, b_step = B_KC ? GM_BK : GM_BK * b_sk;
        if (FULL) {
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                int i = tid + u * 256;
                if (A_KC) pa[u] = A + (long)(m0 + (i >> 3)) * a_si + kb + (i & 7) * 4;
                else { int kk = i / (BM / 4), mq = i - kk * (BM / 4); pa[u] = A + (long)(kb + kk) * a_sk + m0 + mq * 4; }
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                int i = tid + u * 256;
                if (B_KC) pb[u] = Bm + (long)(n0 + (i >> 3)) * b_sj + kb + (i & 7) * 4;
                else { int kk = i / (BN / 4), mq = i - kk * (BN / 4); pb[u] = Bm + (long)(kb + kk) * b_sk + n0 + mq * 4; }
            }
        }
        auto load = [&](int k0) {
            if (FULL) {
#pragma unroll
                for (int u = 0; u < NA; ++u) { ra[u] = *(const f32x4*)pa[u]; pa[u] += a_step; }
#pragma unroll
                for (int u = 0; u < NB; ++u) { rb[u] = *(const f32x4*)pb[u]; pb[u] += b_step; }
            } else {
                gm_load<A_KC, NA, BM>(ra, A, a_si, a_sk, m0, M, K, a_vec, k0, tid);
                gm_load<B_KC, NB, BN>(rb, Bm, b_sj, b_sk, n0, N, K, b_vec, k0, tid);
            }
        };
        auto store = [&](int buf) {
            gm_store<A_KC, NA, BM>(ra, As0 + buf * A_FLOATS, tid);
            gm_store<B_KC, NB, BN>(rb, Bs0 + buf * B_FLOATS, tid);
        };
        auto compute = [&](int buf) {
            const float* As = As0 + buf * A_FLOATS;
            const float* Bs = Bs0 + buf * B_FLOATS;
            f32x4 af0[WM], bf0[WN], af1[WM], bf1[WN];
            read_frags(As, Bs, 0, af0, bf0);
            read_frags(As, Bs, 1, af1, bf1);
            mfma_group(af0, bf0);
            read_frags(As, Bs, 2, af0, bf0);
            mfma_group(af1, bf1);
            read_frags(As, Bs, 3, af1, bf1);
            mfma_group(af0, bf0);
            mfma_group(af1, bf1);
        };
        const int nsteps = (K - kb + GM_BK - 1) / GM_BK;
        load(kb);
        store(0);
        if (nsteps > 1) load(kb + GM_BK);
        __syncthreads();
        int cur = 0, step = 0;
        for (; step + 2 < nsteps; ++step) {           // steady state, branch-free
            store(cur ^ 1);                            // step+1: registers -> the other LDS buffer
            load(kb + (step + 2) * GM_BK);             // step+2: global -> registers
            // The loads must LEAVE here, a whole MFMA block before the next iteration's LDS stores wait for them.  Left to itself
            // hipcc sinks them below the MFMA block (shorter live ranges), to just in front of the barrier: the next iteration then
            // waited for an L2 / HBM round trip at its first ds_write with nothing but the barrier in between (round 4, found
            // in the ISA of every instantiation).  Measured: no change at the GRU shapes (dX 0.270 ms, two-slice dW 0.292 ms) —
            // the second workgroup of the CU was hiding that wait — but this is the order the pipeline was designed around.
            __builtin_amdgcn_sched_barrier(0);
            compute(cur);
            __syncthreads();
            cur ^= 1;
        }
        for (; step < nsteps; ++step) {                // last two steps
            if (step + 1 < nsteps) store(cur ^ 1);
            compute(cur);
            __syncthreads();
            cur ^= 1;
        }
    };
    const bool full = a_vec && b_vec && m0 + BM <= M && n0 + BN <= N && ((K - kb) % GM_BK == 0);
    if (full) run(std::true_type{});
    else run(std::false_type{});

#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
        for (int u = 0; u < WN; ++u) {
            int col = n0 + wn0 + u * 32 + r;
            if (col >= N) continue;
            float bv = bias ? bias[col] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                int row = m0 + wm0 + t * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
                if (row < M) {
                    float* cp = C + (long)row * ldc + col;
                    float v = acc[t][u][j] + bv;
                    if (beta != 0.f) v += beta * (*cp);
                    *cp = v;
                }
            }
        }
}

template <int WVM, int WVN, int WM, int WN, bool AKC, bool BKC>
static int launch_gemm2(dim3 grid, hipStream_t s, const float* A, long a_si, long a_sk, const float* B, long b_sk,
                        long b_sj, float* C, long ldc, const float* bias, float beta, int M, int N, int K, int av, int bv,
                        int k_len, long slab) {
    constexpr int BM = 32 * WM * WVM, BN = 32 * WN * WVN;
    constexpr size_t lds = 2 * ((AKC ? BM * GM_LDK : GM_BK * BM) + (BKC ? BN * GM_LDK : GM_BK * BN)) * sizeof(float);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)gemm_f32_k<WVM, WVN, WM, WN, AKC, BKC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { sed_set_error("gemm_f32: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
    }
    gemm_f32_k<WVM, WVN, WM, WN, AKC, BKC><<<grid, 256, lds, s>>>(A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, av, bv, k_len, slab);
    return 0;
}

template <int WVM, int WVN, int WM, int WN>
static int launch_gemm(bool akc, bool bkc, hipStream_t s, const float* A, long a_si, long a_sk,
                       const float* B, long b_sk, long b_sj, float* C, long ldc, const float* bias, float beta,
                       int M, int N, int K, int av, int bv, int splits = 1, int k_len = 0, long slab = 0) {
    dim3 grid(cdiv(N, 32 * WN * WVN), cdiv(M, 32 * WM * WVM), splits);
    if (k_len == 0) k_len = K;
    if (akc && bkc) return launch_gemm2<WVM, WVN, WM, WN, true, true>(grid, s, A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, av, bv, k_len, slab);
    if (akc && !bkc) return launch_gemm2<WVM, WVN, WM, WN, true, false>(grid, s, A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, av, bv, k_len, slab);
    if (!akc && bkc) return launch_gemm2<WVM, WVN, WM, WN, false, true>(grid, s, A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, av, bv, k_len, slab);
    return launch_gemm2<WVM, WVN, WM, WN, false, false>(grid, s, A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, av, bv, k_len, slab);
}

// C[i][j] = sum_z slab[z][i][j] in slab order (+ bias); four consecutive elements per thread when the row length allows
__global__ __launch_bounds__(256) void gemm_splitk_reduce_k(const float* __restrict__ slabs, int splits, int M, int N,
                                                            float* __restrict__ C, long ldc, const float* __restrict__ bias) {
    const long n = (long)M * N;
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if ((N & 3) == 0 && (ldc & 3) == 0 && (((uintptr_t)C | (uintptr_t)bias | (uintptr_t)slabs) & 15) == 0) {       // the 4 elements share a row; aligned 16-B accesses
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int z = 0; z < splits; ++z) a += *reinterpret_cast<const f32x4*>(slabs + (size_t)z * n + i);
        const long row = i / N, col = i - row * N;
        if (bias) a += *reinterpret_cast<const f32x4*>(bias + col);
        *reinterpret_cast<f32x4*>(C + row * ldc + col) = a;
        return;
    }
    for (long e = i; e < i + 4 && e < n; ++e) {
        float a = 0.f;
        for (int z = 0; z < splits; ++z) a += slabs[(size_t)z * n + e];
        if (bias) a += bias[e % N];
        C[(e / N) * ldc + (e % N)] = a;
    }
}

// Tile + split-K plan.
//  * tile: per-tile efficiency (register / LDS reuse) x how evenly the tiles fill whole rounds of the 256 CUs;
//  * small-output / long-K products (the GRU weight gradients dW_hh, dW_ih of upper layers): 64x64 tiles and enough
//    K-slices to give every CU one;
//  * a product whose best tiling yields at most ~one tile per CU (the layer-0 weight gradient 768x5120x4096 = 240 tiles of
//    128x128) runs one 4-wave workgroup per CU, i.e. ONE wave per SIMD with nothing to cover its barrier and its LDS round
//    trips (91 TFLOP/s against 117 for the 1280-tile data gradient that keeps several workgroups per CU): two K-slices make
//    two co-resident workgroups per CU (113 TFLOP/s incl. the slice sum).  Weight gradients only (sed_gemm_f32_wgrad): their K
//    axis is the batch x time axis, so no caller can expect the result to be independent of how that axis is cut.  The
//    forward input projection (same shape class, +15 % with two slices) is NOT sliced by this rule: it looks at the tile count,
//    i.e. at M, and the eval forward of a batch should not depend on how the batch is cut into chunks.
//  Slices are summed in slice order by gemm_splitk_reduce_k: deterministic.
struct GemmPlan { int cand, splits, k_len; };
static const struct { int bm, bn; double eff; } kCands[5] = {{128, 128, 1.00}, {128, 96, 0.95}, {128, 64, 0.88}, {64, 128, 0.88}, {64, 64, 0.78}};

// policy 0: never split; 1: small-output split only; 2: also the two-slice rule (weight gradients)
static GemmPlan gemm_plan(int M, int N, int K, int policy) {
    const bool may_split = policy >= 1;
    GemmPlan p = {4, 1, K};
    const long blocks64 = (long)cdiv(M, 64) * cdiv(N, 64);
    if (may_split && blocks64 < 96 && K >= 1024) {
        int s = (int)(256 / blocks64);
        const int maxs = K / 128;
        if (s > maxs) s = maxs;
        if (s > 32) s = 32;
        if (s >= 2) {
            p.k_len = ((cdiv(K, s) + GM_BK - 1) / GM_BK) * GM_BK;
            p.splits = cdiv(K, p.k_len);
            return p;
        }
    }
    double best_score = -1.0;
    long best_tiles = 0;
    for (int i = 0; i < 5; ++i) {
        if (kCands[i].bm > 64 && M <= 64) continue;
        if (kCands[i].bn > 64 && N <= 64) continue;
        const long tiles = (long)cdiv(M, kCands[i].bm) * cdiv(N, kCands[i].bn);
        const double useful = ((double)M * N) / ((double)tiles * kCands[i].bm * kCands[i].bn);     // edge waste
        const double rounds = (double)((tiles + 255) / 256);
        double fill = tiles / (rounds * 256.0);
        if (tiles >= 4 * 256) fill = fill > 0.9 ? fill : 0.9;                                      // many rounds: tail matters little
        const double score = kCands[i].eff * useful * fill;
        if (score > best_score) { best_score = score; p.cand = i; best_tiles = tiles; }
    }
    if (policy >= 2 && best_tiles > 128 && best_tiles <= 256 && K >= 2048 && (long)M * N >= (1L << 20)) {
        p.k_len = ((cdiv(K, 2) + GM_BK - 1) / GM_BK) * GM_BK;
        p.splits = cdiv(K, p.k_len);
    }
    // forward projections (policy 1): two K-slices for a long K and a narrow output, decided by N and K ALONE — the same
    // split for every M that reaches this point, so a sample's result does not depend on the batch it is evaluated in (the
    // rule above looks at the tile count, i.e. at M, which is why it is reserved for weight gradients).  At N <= 1024 the usual
    // batches give at most one workgroup per CU (one wave per SIMD); two co-resident slices hide each other's waits.
    // NOT every M reaches this point: the small-output rule at the top of this function also applies to policy 1 and does
    // look at M (blocks64 < 96 && K >= 1024).  For the 128-channel net (K = 5120, N = 768, 8 rows per 64-frame window) a chunk of
    // at most 56 windows sums K in up to 21 slices, a larger one in these two, so logits of small and large chunks differ by
    // rounding (<= 2e-6, measured 6e-8) and are bitwise equal only between chunks of 57 windows or more
    // (tests/test_gpu_detect.py: test_chunking_of_the_128_channel_net_...; DESIGN 2 "Batch separability", 5f).
    if (policy == 1 && K >= 4096 && N <= 1024) {
        p.k_len = ((cdiv(K, 2) + GM_BK - 1) / GM_BK) * GM_BK;
        p.splits = cdiv(K, p.k_len);
    }
    return p;
}

extern "C" size_t sed_gemm_f32_workspace_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    size_t best = 0;
    for (int policy = 1; policy <= 2; ++policy) {
        const GemmPlan p = gemm_plan(M, N, K, policy);
        const size_t b = p.splits > 1 ? (size_t)p.splits * M * N * sizeof(float) : 0;
        if (b > best) best = b;
    }
    return best;
}

// What gemm_impl would use for (M, N, K) under a policy (0: sed_gemm_f32, 1: sed_gemm_f32_ws, 2: sed_gemm_f32_wgrad), from the
// gemm_plan and the kCands the launches read, so the report and the dispatch cannot drift apart.  Host only.
extern "C" int sed_gemm_f32_plan(int M, int N, int K, int policy, int* bm, int* bn, int* splits, int* k_len) {
    SED_REQUIRE(bm && bn && splits && k_len, "gemm_f32_plan: null pointer");
    SED_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_f32_plan: bad sizes M=%d N=%d K=%d", M, N, K);
    SED_REQUIRE(policy >= 0 && policy <= 2, "gemm_f32_plan: policy %d is not 0 (gemm_f32), 1 (gemm_f32_ws) or 2 (gemm_f32_wgrad)", policy);
    const GemmPlan p = gemm_plan(M, N, K, policy);
    *bm = kCands[p.cand].bm; *bn = kCands[p.cand].bn; *splits = p.splits; *k_len = p.k_len;
    return 0;
}

static int gemm_impl(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj, float* C,
                     long ldc, const float* bias, float beta, int M, int N, int K, void* workspace, int policy, void* stream) {
    SED_REQUIRE(A && B && C, "gemm_f32: null pointer");
    SED_REQUIRE(M > 0 && N > 0 && K > 0 && ldc >= N, "gemm_f32: bad sizes M=%d N=%d K=%d ldc=%ld", M, N, K, ldc);
    SED_REQUIRE(a_si == 1 || a_sk == 1, "gemm_f32: A must be contiguous along i or k (strides %ld,%ld)", a_si, a_sk);
    SED_REQUIRE(b_sk == 1 || b_sj == 1, "gemm_f32: B must be contiguous along k or j (strides %ld,%ld)", b_sk, b_sj);
    bool akc = (a_sk == 1), bkc = (b_sk == 1);
    // when both strides are 1 (a vector) either reading is valid; prefer k-contiguous
    int av = (((uintptr_t)A & 15) == 0) && ((akc ? a_si : a_sk) % 4 == 0);
    int bv = (((uintptr_t)B & 15) == 0) && ((bkc ? b_sj : b_sk) % 4 == 0);
    hipStream_t s = as_stream(stream);
    SedProfScope prof(SED_K_GEMM, s, 2.0 * M * (double)N * K);
    const GemmPlan p = gemm_plan(M, N, K, workspace ? policy : 0);
    const bool split = p.splits > 1;
    SED_REQUIRE(!split || beta == 0.f, "gemm_f32: split-K path takes no beta");
    float* out = split ? (float*)workspace : C;
    const long ldo = split ? N : ldc;
    const float* ob = split ? nullptr : bias;
    const long slab = split ? (long)M * N : 0;
    int rc;
    switch (p.cand) {
        case 0: rc = launch_gemm<2, 2, 2, 2>(akc, bkc, s, A, a_si, a_sk, B, b_sk, b_sj, out, ldo, ob, beta, M, N, K, av, bv, p.splits, p.k_len, slab); break;
        case 1: rc = launch_gemm<4, 1, 1, 3>(akc, bkc, s, A, a_si, a_sk, B, b_sk, b_sj, out, ldo, ob, beta, M, N, K, av, bv, p.splits, p.k_len, slab); break;
        case 2: rc = launch_gemm<2, 2, 2, 1>(akc, bkc, s, A, a_si, a_sk, B, b_sk, b_sj, out, ldo, ob, beta, M, N, K, av, bv, p.splits, p.k_len, slab); break;
        case 3: rc = launch_gemm<2, 2, 1, 2>(akc, bkc, s, A, a_si, a_sk, B, b_sk, b_sj, out, ldo, ob, beta, M, N, K, av, bv, p.splits, p.k_len, slab); break;
        default: rc = launch_gemm<2, 2, 1, 1>(akc, bkc, s, A, a_si, a_sk, B, b_sk, b_sj, out, ldo, ob, beta, M, N, K, av, bv, p.splits, p.k_len, slab); break;
    }
    if (rc) return rc;
    SED_LAUNCH_CHECK("gemm_f32");
    if (split) {
        const long n4 = ((long)M * N + 3) / 4;
        gemm_splitk_reduce_k<<<cdiv(n4, 256), 256, 0, s>>>((const float*)workspace, p.splits, M, N, C, ldc, bias);
        SED_LAUNCH_CHECK("gemm_splitk_reduce");
    }
    return 0;
}

extern "C" int sed_gemm_f32(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj, float* C,
                            long ldc, const float* bias, float beta, int M, int N, int K, void* stream) {
    return gemm_impl(A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, beta, M, N, K, nullptr, 0, stream);
}

extern "C" int sed_gemm_f32_ws(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj, float* C,
                               long ldc, const float* bias, int M, int N, int K, void* workspace, void* stream) {
    return gemm_impl(A, a_si, a_sk, B, b_sk, b_sj, C, ldc, bias, 0.f, M, N, K, workspace, 1, stream);
}

extern "C" int sed_gemm_f32_wgrad(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj, float* C,
                                  long ldc, int M, int N, int K, void* workspace, void* stream) {
    return gemm_impl(A, a_si, a_sk, B, b_sk, b_sj, C, ldc, nullptr, 0.f, M, N, K, workspace, 2, stream);
}

// ───────────────────────── small dense head ─────────────────────────
// y[m][n] = act(b[n] + sum_k x[m][k] W[n][k]); one wave per row m, lanes split k.
__global__ __launch_bounds__(256) void linear_fwd_k(const float* __restrict__ x, const float* __restrict__ W,
                                                    const float* __restrict__ b, float* __restrict__ y, int M,
                                                    int K, int N, int relu) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    for (int n = 0; n < N; ++n) {
        float a = 0.f;
        for (int k = lane; k < K; k += 64) a += x[(size_t)m * K + k] * W[(size_t)n * K + k];
        a = wave_sum(a);
        if (lane == 0) {
            a += b ? b[n] : 0.f;
            if (relu) a = fmaxf(a, 0.f);
            y[(size_t)m * N + n] = a;
        }
    }
}

extern "C" int sed_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int K, int N,
                              int relu, void* stream) {
    SED_REQUIRE(x && W && y && M > 0 && K > 0 && N > 0, "linear_fwd: bad arguments");
    linear_fwd_k<<<cdiv(M, 4), 256, 0, as_stream(stream)>>>(x, W, b, y, M, K, N, relu);
    SED_LAUNCH_CHECK("linear_fwd");
    return 0;
}

#define LIN_CHUNK 64   // rows per partial block in the weight gradient

__global__ void linear_relu_mask_k(const float* __restrict__ y, float* __restrict__ dy, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !(y[i] > 0.f)) dy[i] = 0.f;
}
// dx[m][k] = sum_n dy[m][n] W[n][k]
__global__ void linear_dx_k(const float* __restrict__ dy, const float* __restrict__ W, float* __restrict__ dx,
                            int M, int K, int N) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * K) return;
    int k = (int)(i % K);
    long m = i / K;
    float a = 0.f;
    for (int n = 0; n < N; ++n) a += dy[m * N + n] * W[(size_t)n * K + k];
    dx[i] = a;
}
// partial[chunk][n*K + k] = sum_{m in chunk} dy[m][n] x[m][k];  partial_b[chunk][n] = sum dy[m][n]
__global__ void linear_dw_partial_k(const float* __restrict__ dy, const float* __restrict__ x,
                                    float* __restrict__ part, int M, int K, int N) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    int tot = N * K + N;
    if (i >= tot) return;
    int m_lo = blockIdx.y * LIN_CHUNK, m_hi = m_lo + LIN_CHUNK < M ? m_lo + LIN_CHUNK : M;
    float a = 0.f;
    if (i < N * K) {
        int n = i / K, k = i - n * K;
        for (int m = m_lo; m < m_hi; ++m) a += dy[(size_t)m * N + n] * x[(size_t)m * K + k];
    } else {
        int n = i - N * K;
        for (int m = m_lo; m < m_hi; ++m) a += dy[(size_t)m * N + n];
    }
    part[(size_t)blockIdx.y * tot + i] = a;
}
__global__ void linear_dw_reduce_k(const float* __restrict__ part, int chunks, int tot, int NK,
                                   float* __restrict__ dW, float* __restrict__ db) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tot) return;
    double a = 0.0;
#pragma unroll 8
    for (int c = 0; c < chunks; ++c) a += (double)part[(size_t)c * tot + i];
    if (i < NK) dW[i] = (float)a;
    else if (db) db[i - NK] = (float)a;
}

extern "C" size_t sed_linear_bwd_workspace_bytes(int M, int K, int N) {
    return (size_t)cdiv(M, LIN_CHUNK) * ((size_t)N * K + N) * sizeof(float);
}

extern "C" int sed_linear_bwd(const float* x, const float* W, const float* y, float* dy, float* dx, float* dW,
                              float* db, void* workspace, int M, int K, int N, int relu, void* stream) {
    SED_REQUIRE(x && W && dy && dW && workspace && M > 0 && K > 0 && N > 0, "linear_bwd: bad arguments");
    SED_REQUIRE(!relu || y, "linear_bwd: relu=1 needs the forward output y");
    hipStream_t s = as_stream(stream);
    if (relu) {
        long n = (long)M * N;
        linear_relu_mask_k<<<cdiv(n, 256), 256, 0, s>>>(y, dy, n);
        SED_LAUNCH_CHECK("linear_relu_mask");
    }
    if (dx) {
        long n = (long)M * K;
        linear_dx_k<<<cdiv(n, 256), 256, 0, s>>>(dy, W, dx, M, K, N);
        SED_LAUNCH_CHECK("linear_dx");
    }
    int tot = N * K + N, chunks = cdiv(M, LIN_CHUNK);
    linear_dw_partial_k<<<dim3(cdiv(tot, 256), chunks), 256, 0, s>>>(dy, x, (float*)workspace, M, K, N);
    SED_LAUNCH_CHECK("linear_dw_partial");
    linear_dw_reduce_k<<<cdiv(tot, 256), 256, 0, s>>>((const float*)workspace, chunks, tot, N * K, dW, db);
    SED_LAUNCH_CHECK("linear_dw_reduce");
    return 0;
}
