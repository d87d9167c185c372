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
#define GM_LDK 36   // LDS row of one m (or n): 32 k + 4 pad floats (16-B slot stride 9) -> conflict-free ds_read_b128

// A_KC / B_KC: operand is contiguous along k (true) or along m/n (false).  The flag decides how a K-step is STAGED, nothing else:
// either kind ends up in the same LDS image [row m or n][GM_LDK], k-contiguous, and every fragment is one ds_read_b128.
// Block tile (32*WM*WVM) x (32*WN*WVN), 4 waves as WVM x WVN, each wave WM x WN tiles of 32x32 (v_mfma_f32_32x32x2_f32).
// Three-stage pipeline per K-step of 32: registers hold step k+1 (global loads issued a whole step earlier), LDS buffer
// `cur` holds step k, and one barrier per step has nothing outstanding.  FULL = interior tile with aligned operands and K a
// multiple of 32: loads without range tests (the guarded variant costs ~1000 scalar/branch instructions per step, which a lone
// wave per SIMD cannot hide).  The FULL steady state is issued in ONE pinned order (sched_group_barrier in `compute`): the
// fragment reads of k-groups 0 and 1, group 0's MFMAs, the reads of group g + 2 one per MFMA behind the last MFMA of group g,
// and behind the last read the LDS stores of step k+1 and the global loads of step k+2, one of each per MFMA.  A wave thus
// issues everything that is not an MFMA under its own MFMAs; only the reads of groups 0 and 1 behind the barrier stand bare.
// (Before, stores and loads stood in a block in front of the MFMAs that only the CU's other workgroup could cover, and how
// well it did depended on details as small as the addressing form of one operand: 0.268 against 0.303 ms for the same loop.)
// The guarded path and tiles too small for the interleave keep stores and loads in front of the MFMA block.
//
// Staging a k-contiguous operand: float4 i = tid + 256 u of the tile is (row i / 8, k-quad i % 8), TILE / 32 per thread, written
// to the image as it was loaded.
// Staging an m/n-contiguous operand (source [k][m]): the 32 x TILE step is cut into 4 x 4 blocks, block (bq, bk) = k rows
// 4 bk .. 4 bk + 3 of m columns 4 bq .. 4 bq + 3, 8 x TILE / 4 of them.  A thread owns ONE block: four 16-byte loads, one per k
// row, whose 16 registers regrouped by column are the four 16-byte image rows (m = 4 bq + c, k = 4 bk .. 4 bk + 3).  The regrouping
// is NOT free: a load fills four consecutive registers and a ds_write_b128 takes four consecutive ones, so it costs up to 16
// v_mov per operand and step (15 after coalescing) — but no LDS traffic, where the [k][m] image cost four 4-byte reads per fragment
// (hipcc paired them: 2 ds_read2_b32).
// A 128-wide tile has exactly 256 blocks; a 96-wide one has 192 and its last wave stages nothing.  A 64-wide tile would leave two
// waves idle with the other two staging twice as much in front of 16 MFMAs (measured: the 64 x 64 weight gradients of the upper
// GRU layers 19.1 -> 25.3 us), so there a thread owns HALF a block, 2 k rows x 4 columns: two loads, four ds_write_b64.
// Lane -> block, wave w, lane l (96 and 128 wide):   bq = 8 w + (l & 3) + 4 ((l >> 3) & 1),   bk = ((l >> 2) & 1) + 2 (l >> 4).
//  * global side: a wave covers m quads 8 w .. 8 w + 7 (128 bytes) of k blocks 0 .. 7, so each of its four loads (k row 4 bk + e) is
//    eight whole 128-byte row segments, and the four lanes of a quad read 64 consecutive bytes;
//  * LDS side: ds_write_b128 is served in 8 groups of 8 consecutive lanes on 32 banks, i.e. 8 slots of 16 B.  The slot of the
//    store of column c is (4 bq + c) * 9 + bk, mod 8 = (4 (bq & 1) + bk + c) mod 8.  Inside a group bit 0 of bq and bit 0 of bk
//    vary (4 slots) and so does bit 1 of bq, which the slot does not see: two-way, 16 LDS-array cycles against the 13 the
//    instruction needs to hand over its data anyway.  (Conflict-free needs all four bk & 3 inside a group, i.e. pairs of
//    lanes on 32-byte pieces of four different rows; measured equal: dX 0.303 / 0.302 ms, two-slice dW 0.272 / 0.270.)
// 64 wide:   bq = 8 (w & 1) + (l & 3) + 4 ((l >> 4) & 1),   bk = (l >> 2 & 3) + 4 (l >> 5) + 8 (w >> 1)   (bk counts pairs of rows).
//  * a wave covers 8 m quads (128 bytes) of 8 row pairs; ds_write_b64 is served in 4 groups of 16 consecutive lanes on 32
//    banks: dword (4 bq + c) * 36 + 2 bk, mod 32 = 16 (bq & 1) + 2 bk + 4 c.  Inside a group bits 0, 1 of bk and bit 0 of bq vary
//    (8 bank pairs) and bit 1 of bq, unseen: two-way, 8 LDS-array cycles against 6 for the data.
#define gm_global __attribute__((address_space(1)))

template <int TILE> constexpr int gm_rows() { return TILE >= 96 ? 4 : 2; }     // k rows of a thread's block
template <int TILE>
__device__ __forceinline__ bool gm_block(int wave, int lane, int& bq, int& bk) {
    static_assert(TILE == 128 || TILE == 96 || TILE == 64, "tile widths of kCands");
    if (TILE >= 96) {
        bq = 8 * wave + (lane & 3) + 4 * ((lane >> 3) & 1);
        bk = ((lane >> 2) & 1) + 2 * (lane >> 4);
        return TILE >= 128 || wave < TILE / 32;        // wave-uniform
    }
    bq = 8 * (wave & 1) + (lane & 3) + 4 * ((lane >> 4) & 1);                // 64 wide: 2 x 4 half blocks, 16 x 16 of them
    bk = ((lane >> 2) & 3) + 4 * (lane >> 5) + 8 * (wave >> 1);
    return true;
}
template <bool KC, int NR, int TILE>
__device__ __forceinline__ void gm_load(f32x4* reg, const float* __restrict__ P, long s_mn, long s_k, int mn0, int MN,
                                        int K, int vec, int k0, int tid, int wave) {
    if (KC) {
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            int i = tid + u * 256;
            f32x4 v = {0, 0, 0, 0};
            int row = i >> 3, kq = i & 7;
            int m = mn0 + row, k = k0 + kq * 4;
            const float* p = P + (long)m * s_mn + k;
            if (m < MN) {
                if (vec && k + 3 < K) v = *(const f32x4*)p;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (k + e < K) v[e] = p[e];
            }
            reg[u] = v;
        }
    } else {
        int bq, bk;
        const bool mine = gm_block<TILE>(wave, tid & 63, bq, bk);
#pragma unroll
        for (int e = 0; e < NR; ++e) {                 // NR == gm_rows<TILE>(): the block's k rows
            f32x4 v = {0, 0, 0, 0};
            int m = mn0 + bq * 4, k = k0 + bk * NR + e;
            const float* p = P + (long)k * s_k + m;
            if (mine && k < K) {
                if (vec && m + 3 < MN) v = *(const f32x4*)p;
                else
#pragma unroll
                    for (int c = 0; c < 4; ++c) if (m + c < MN) v[c] = p[c];
            }
            reg[e] = v;
        }
    }
}
template <bool KC, int NR, int TILE>
__device__ __forceinline__ void gm_store(const f32x4* reg, float* S, int tid, int wave) {
    if (KC) {
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            int i = tid + u * 256;
            int row = i >> 3, kq = i & 7;
            *(f32x4*)(S + row * GM_LDK + kq * 4) = reg[u];
        }
    } else {
        int bq, bk;
        if (!gm_block<TILE>(wave, tid & 63, bq, bk)) return;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float* d = S + (bq * 4 + c) * GM_LDK + bk * NR;
            if (NR == 4) { const f32x4 t = {reg[0][c], reg[1][c], reg[2][c], reg[3][c]}; *(f32x4*)d = t; }
            else { const f32x2 t = {reg[0][c], reg[1][c]}; *(f32x2*)d = t; }
        }
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
    constexpr int A_FLOATS = BM * GM_LDK, B_FLOATS = BN * GM_LDK;
    // float4 per thread per K-step: BM*32 floats / 256 threads / 4 of a k-contiguous operand, the k rows of its block otherwise
    constexpr int NA = A_KC ? BM / 32 : gm_rows<BM>(), NB = B_KC ? BN / 32 : gm_rows<BN>();
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
        for (int t = 0; t < WM; ++t) af[t] = *(const f32x4*)(As + (wm0 + t * 32 + r) * GM_LDK + g * 8 + 4 * h);
#pragma unroll
        for (int u = 0; u < WN; ++u) bf[u] = *(const f32x4*)(Bs + (wn0 + u * 32 + r) * GM_LDK + g * 8 + 4 * h);
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
        // FULL: the address of a load is a workgroup-uniform base (the tile's corner at the current K-step, in scalar registers,
        // advanced once per step by scalar adds) plus a loop-invariant 32-bit byte offset per lane and load: the K loop carries no
        // vector address arithmetic between its MFMAs (per-thread 64-bit pointers cost two vector adds per load and step).
        // `full` below admits only tiles whose extent times the leading stride fits the 32-bit offset.
        const char* ga = (const char*)(A + (A_KC ? (long)m0 * a_si + kb : (long)kb * a_sk + m0));
        const char* gb = (const char*)(Bm + (B_KC ? (long)n0 * b_sj + kb : (long)kb * b_sk + n0));
        const long a_step = (A_KC ? GM_BK : GM_BK * a_sk) * (long)sizeof(float), b_step = (B_KC ? GM_BK : GM_BK * b_sk) * (long)sizeof(float);
        unsigned oa[NA], ob[NB];
        int aq = 0, ak = 0, bq = 0, bk = 0;            // this thread's block of an m/n-contiguous A, B
        const bool a_mine = A_KC || gm_block<BM>(wave, lane, aq, ak), b_mine = B_KC || gm_block<BN>(wave, lane, bq, bk);
        if (FULL) {
#pragma unroll
            for (int u = 0; u < NA; ++u) {
                int i = tid + u * 256;
                oa[u] = (unsigned)((A_KC ? (long)(i >> 3) * a_si + (i & 7) * 4 : (long)(ak * NA + u) * a_sk + aq * 4) * (long)sizeof(float));
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                int i = tid + u * 256;
                ob[u] = (unsigned)((B_KC ? (long)(i >> 3) * b_sj + (i & 7) * 4 : (long)(bk * NB + u) * b_sk + bq * 4) * (long)sizeof(float));
            }
        }
        auto load = [&](int k0) {
            if (FULL) {
                // opaque to the optimiser: left to itself, loop strength reduction folds base + offset back into one 64-bit
                // vector pointer per load and advances each of them with a vector add.  (The constraint also hides that the
                // pointer is to global memory, hence the explicit address space: a generic pointer would load with flat_load.  The
                // offsets are hidden too: hoisted out of the loop as 64-bit values, they would no longer be seen as the
                // zero-extended 32-bit register that the scalar-base form of global_load takes, and cost a vector add again.)
                asm("" : "+s"(ga));
                asm("" : "+s"(gb));
                if (a_mine) {
#pragma unroll
                    for (int u = 0; u < NA; ++u) { asm("" : "+v"(oa[u])); ra[u] = *(const gm_global f32x4*)((const gm_global char*)ga + oa[u]); }
                }
                if (b_mine) {
#pragma unroll
                    for (int u = 0; u < NB; ++u) { asm("" : "+v"(ob[u])); rb[u] = *(const gm_global f32x4*)((const gm_global char*)gb + ob[u]); }
                }
                ga += a_step;
                gb += b_step;
            } else {
                gm_load<A_KC, NA, BM>(ra, A, a_si, a_sk, m0, M, K, a_vec, k0, tid, wave);
                gm_load<B_KC, NB, BN>(rb, Bm, b_sj, b_sk, n0, N, K, b_vec, k0, tid, wave);
            }
        };
        auto store = [&](int buf) {
            gm_store<A_KC, NA, BM>(ra, As0 + buf * A_FLOATS, tid, wave);
            gm_store<B_KC, NB, BN>(rb, Bs0 + buf * B_FLOATS, tid, wave);
        };
        auto compute = [&](int buf, auto ilv_tag) {
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
            // The order above, pinned.  Left alone hipcc moves the reads of groups 2 and 3 down to where their MFMAs start and
            // waits for all of them there (seen in the 128 x 128 loops once every fragment was a b128 read): the LDS latency
            // is then exposed in the middle of every step.  A group's reads reuse the registers of the group two back, so they
            // follow its last MFMA, one per MFMA, and have the rest of a group (NM - NF MFMAs) to arrive.
            // ILV (steady state of the FULL path): the LDS stores of step + 1 and the global loads of step + 2 follow this block in
            // the source and are dealt out behind the MFMAs that follow the last fragment read, one store and one load per
            // MFMA: a wave issues them under its own MFMAs instead of in a block that only the CU's other workgroup can cover.
            // (Behind the reads, not in front: hipcc cannot tell that the stores go to the other buffer and keeps LDS order.)
            constexpr bool ILV = decltype(ilv_tag)::value;
            constexpr int NF = WM + WN, NM = 4 * WM * WN, NW = NA + NB;
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * NF, 0);          // groups 0 and 1: DS reads
            __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);              // group 0: MFMAs
#pragma unroll
            for (int g = 0; g < 2; ++g) {
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                if (g == 0 || !ILV) __builtin_amdgcn_sched_group_barrier(0x008, NM - NF, 0);
            }
            if (ILV) {
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);      // DS write
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // global load
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - NF - NW, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);          // group 3
            }
        };
        const int nsteps = (K - kb + GM_BK - 1) / GM_BK;
        load(kb);
        store(0);
        if (nsteps > 1) load(kb + GM_BK);
        __syncthreads();
        int cur = 0, step = 0;
        for (; step + 2 < nsteps; ++step) {           // steady state, branch-free
            constexpr bool ILV = FULL && NA + NB <= 8 * WM * WN - (WM + WN);
            if (ILV) {
                compute(cur, std::true_type{});
                store(cur ^ 1);                        // step+1: registers -> the other LDS buffer
                load(kb + (step + 2) * GM_BK);         // step+2: global -> registers
            } else {
                store(cur ^ 1);
                load(kb + (step + 2) * GM_BK);
                // The loads must LEAVE here, a whole MFMA block before the next iteration's LDS stores wait for them.  Left to itself
                // hipcc sinks them below the MFMA block (shorter live ranges), to just in front of the barrier: the next iteration
                // then waited for an L2 / HBM round trip at its first ds_write with nothing but the barrier in between (round 4,
                // found in the ISA of every instantiation).
                __builtin_amdgcn_sched_barrier(0);
                compute(cur, std::false_type{});
            }
            // ... and the barrier stays behind the MFMA block: hipcc waits for every outstanding LDS read in front of a barrier,
            // and hoisted to the last read it would expose the latency of group 3's fragments
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            cur ^= 1;
        }
        for (; step < nsteps; ++step) {                // last two steps
            if (step + 1 < nsteps) store(cur ^ 1);
            compute(cur, std::false_type{});
            __syncthreads();
            cur ^= 1;
        }
    };
    const bool full = a_vec && b_vec && m0 + BM <= M && n0 + BN <= N && ((K - kb) % GM_BK == 0);
    // the FULL path's 32-bit lane offsets span a tile's rows: BM (BN) rows of a k-contiguous operand, GM_BK rows of the other kind.
    // A leading stride of 4M floats and more (no caller has one) goes the guarded way, which indexes in 64 bits.
    const bool fits = (A_KC ? BM * a_si : GM_BK * a_sk) < (1L << 29) && (B_KC ? BN * b_sj : GM_BK * b_sk) < (1L << 29);
    if (full && fits) run(std::true_type{});
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
    constexpr size_t lds = 2 * (BM + BN) * GM_LDK * sizeof(float);         // 128 x 128: 72 KB, two workgroups per CU (147 of 160 KB)
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

// sed_linear_bwd in its two halves.  _dx: what the layer below waits for (the ReLU mask on dy, then dx).  _dw: the weight and
// bias gradient, which feed only the optimiser — the whole-network backward issues it on its auxiliary stream, behind an event
// recorded after _dx (it reads the masked dy).
int sed_internal_linear_bwd_dx(const float* W, const float* y, float* dy, float* dx, int M, int K, int N, int relu, void* stream) {
    SED_REQUIRE(W && dy && M > 0 && K > 0 && N > 0, "linear_bwd: bad arguments");
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
    return 0;
}
int sed_internal_linear_bwd_dw(const float* x, const float* dy, float* dW, float* db, void* workspace, int M, int K, int N, void* stream) {
    SED_REQUIRE(x && dy && dW && workspace && M > 0 && K > 0 && N > 0, "linear_bwd: bad arguments");
    hipStream_t s = as_stream(stream);
    int tot = N * K + N, chunks = cdiv(M, LIN_CHUNK);
    linear_dw_partial_k<<<dim3(cdiv(tot, 256), chunks), 256, 0, s>>>(dy, x, (float*)workspace, M, K, N);
    SED_LAUNCH_CHECK("linear_dw_partial");
    linear_dw_reduce_k<<<cdiv(tot, 256), 256, 0, s>>>((const float*)workspace, chunks, tot, N * K, dW, db);
    SED_LAUNCH_CHECK("linear_dw_reduce");
    return 0;
}

extern "C" int sed_linear_bwd(const float* x, const float* W, const float* y, float* dy, float* dx, float* dW,
                              float* db, void* workspace, int M, int K, int N, int relu, void* stream) {
    SED_REQUIRE(x && W && dy && dW && workspace && M > 0 && K > 0 && N > 0, "linear_bwd: bad arguments");
    SED_TRY(sed_internal_linear_bwd_dx(W, y, dy, dx, M, K, N, relu, stream));
    return sed_internal_linear_bwd_dw(x, dy, dW, db, workspace, M, K, N, stream);
}
