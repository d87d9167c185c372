// conv_bf16.hip — the opt-in bf16 inference plan (sed_net_cfg.conv_mode = 2): a direct 3x3 conv with BatchNorm folded
// into bf16 weights and the ReLU + (1,2) time pool in its epilogue, and the bf16 GEMM of the first GRU layer's input projection.
// Both run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; nothing here is used by training or by the exact-fp32 plans.
//
// Rounding points (and only these): the folded weights w' = w * gamma / sqrt(var + eps) (fp32, then bf16), the conv input
// (stored bf16 by the bf16 block below, or rounded while staging when the producer is an fp32 block), and both operands of the
// projection.  Bias, ReLU and the pool run on the fp32 accumulators; the pooled output is rounded to bf16 once, when stored.
//
// No hand-counted waits: the loads of one LDS chunk's (tap, k-group) steps form a fully unrolled straight line, so hipcc's own
// vmcnt bookkeeping is exact and the weight fragments run CB_PF steps ahead of their MFMAs.
#include "conv_shared.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define CB_MTW 5      // 32-row tiles per wave (a wave owns all rows of its 32 output channels)
#define CB_PF 4       // weight-fragment steps in flight ahead of the MFMAs
#define CB_LDS_MAX (64 * 1024)

namespace {

// ───────────────────────── conv: tile choice ─────────────────────────
struct Bf16Plan {
    int ok, nw, cch, TT, FT, nft, tblocks;
    int pp, tp;         // LDS bytes per halo position / per halo time row
    size_t lds;
};

// bytes of one halo position: CCH bf16 + 16 (an odd number of 16-byte slots: 32 consecutive positions are ds_read_b128
// conflict-free); a halo time row adds the pad that keeps the slot sequence going across the mel wrap-around of a 32-row tile
inline int pos_pitch(int cch) { return cch * 2 + 16; }
inline int row_pitch(int FT, int cch) {
    const int s = pos_pitch(cch) / 16;
    return (FT + 2) * pos_pitch(cch) + 16 * ((16 - (2 * s) % 16) % 16);
}

Bf16Plan bf16_plan(int B, int Cin, int F, int T, int Cout) {
    Bf16Plan p{};
    if (B <= 0 || F <= 0 || T < 2 || Cin <= 0 || Cin % 32 || Cout <= 0 || Cout % 64) return p;
    if ((size_t)B * T * F * Cin >= ((size_t)1 << 31) || (size_t)B * T * F * Cout >= ((size_t)1 << 31)) return p;
    p.nw = (Cout % 128 == 0) ? 4 : 2;
    p.cch = (Cin % 128 == 0) ? 128 : (Cin % 64 == 0 ? 64 : 32);
    // the pooling epilogue: an even number of time rows (a pair never straddles two workgroups), at most 32 mel columns (a
    // pair lies in two consecutive 32-row tiles); score as conv.hip's conv_tile (used rows x coverage, halo share discounted)
    const int limit = 32 * CB_MTW;
    double best = -1.0;
    for (int nft = 1; nft <= F; ++nft) {
        const int FT = cdiv(F, nft);
        if (FT > 32) continue;
        if (nft > 1 && cdiv(F, nft - 1) == FT) continue;
        for (int TT = 2; TT <= 16 && TT <= T + (T & 1); TT += 2) {
            if (TT * FT > limit) break;
            const size_t halo = (size_t)(TT + 2) * row_pitch(FT, p.cch);
            size_t lds = halo > (size_t)p.nw * 8192 ? halo : (size_t)p.nw * 8192;
            if (lds > CB_LDS_MAX) continue;
            const double util = ((double)(TT * FT) / limit) * ((double)F / ((double)nft * FT)) * ((double)T / ((double)cdiv(T, TT) * TT));
            const double score = util / (1.0 + 0.25 * ((double)(TT + 2) * (FT + 2) / (TT * FT) - 1.0));
            if (score > best) { best = score; p.TT = TT; p.FT = FT; p.nft = nft; p.lds = lds; }
        }
    }
    if (best <= 0.0) return p;
    p.ok = 1;
    p.pp = pos_pitch(p.cch);
    p.tp = row_pitch(p.FT, p.cch);
    p.tblocks = cdiv(T, p.TT);
    return p;
}

// ───────────────────────── conv: kernel ─────────────────────────
// grid (tblocks * nft, B, Cout / (32 NW)); NW waves, wave w owns output channels co0 + 32 w .. + 31 and every row of the tile
// (TT time rows x FT mel columns, rows p = tl * FT + f).  A = halo positions (bf16 in LDS, CCH channels per chunk), B = the
// folded weight fragments streamed from L2 in MFMA order, accumulators start at the folded bias.
template <int NW, int CCH, bool XBF>
__global__ __launch_bounds__(64 * NW) void conv3x3_bf16_eval_k(
    const void* __restrict__ xv, const bf16x8* __restrict__ wq, const float* __restrict__ bias, __bf16* __restrict__ y,
    int Cin, int F, int T, int Cout, int TT, int FT, int nft, int TP) {
    constexpr int PP = CCH * 2 + 16;
    constexpr int NG = CCH / 16;                  // 16-channel k-groups per chunk
    constexpr int NS = 9 * NG;                    // (tap, k-group) steps per chunk
    constexpr int Q = CCH / 8;                    // 16-byte units of a position per chunk
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int tb = blockIdx.x / nft, f0 = (blockIdx.x - tb * nft) * FT;
    const int b = blockIdx.y, t0 = tb * TT;
    const int cot = blockIdx.z * NW + wave, co0 = cot * 32;
    const int MROWS = TT * FT, F2 = FT + 2, HP = (TT + 2) * F2;
    const int ncot = Cout >> 5, nkg = Cin >> 4;

    int abase[CB_MTW];
#pragma unroll
    for (int i = 0; i < CB_MTW; ++i) {
        int p = i * 32 + r;
        if (p >= MROWS) p = MROWS - 1;            // tiles past the tile's rows read a valid row and are never stored
        const int tl = p / FT, f = p - tl * FT;
        abase[i] = tl * TP + f * PP + h * 16;
    }
    const float bv = bias[co0 + r];
    f32x16 acc[CB_MTW];
#pragma unroll
    for (int i = 0; i < CB_MTW; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[i][j] = bv;

    const bf16x8* wl = wq + (size_t)cot * 64 + lane;
    for (int c0 = 0; c0 < Cin; c0 += CCH) {
        if (c0) __syncthreads();                  // every wave is done with the previous chunk
        for (int i = tid; i < HP * Q; i += 64 * NW) {
            const int pos = i / Q, q = i - pos * Q;
            const int tt = pos / F2, ff = pos - tt * F2;
            const int t = t0 + tt - 1, f = f0 + ff - 1;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (t >= 0 && t < T && f >= 0 && f < F) {
                const size_t e = (((size_t)b * T + t) * F + f) * Cin + c0 + q * 8;
                if (XBF) {
                    v = *(const u32x4*)((const __bf16*)xv + e);
                } else {
                    const f32x4 a0 = *(const f32x4*)((const float*)xv + e), a1 = *(const f32x4*)((const float*)xv + e + 4);
                    bf16x8 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { o[k] = (__bf16)a0[k]; o[4 + k] = (__bf16)a1[k]; }     // round to nearest even
                    v = __builtin_bit_cast(u32x4, o);
                }
            }
            *(u32x4*)(lds + tt * TP + ff * PP + q * 16) = v;
        }
        __syncthreads();
        const int kg0 = c0 >> 4;
        auto wfrag = [&](int s) {                 // step s = tap * NG + g
            const int tap = s / NG, g = s - tap * NG;
            return wl[((size_t)tap * nkg + kg0 + g) * ncot * 64];
        };
        bf16x8 wr[CB_PF];
#pragma unroll
        for (int s = 0; s < CB_PF; ++s) wr[s] = wfrag(s);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bf16x8 bcur = wr[s % CB_PF];
            if (s + CB_PF < NS) wr[s % CB_PF] = wfrag(s + CB_PF);
            const int tap = s / NG, g = s - tap * NG, kh = tap / 3, kw = tap - 3 * kh;
            const int off = kw * TP + kh * PP + g * 32;      // kh walks mel, kw walks time (weight [co][ci][kh][kw])
            bf16x8 a[CB_MTW];
#pragma unroll
            for (int i = 0; i < CB_MTW; ++i) a[i] = *(const bf16x8*)(lds + abase[i] + off);
#pragma unroll
            for (int i = 0; i < CB_MTW; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bcur, acc[i], 0, 0, 0);
        }
    }
    __syncthreads();                              // the halo is free: each wave's 8 KB two-tile ring lives there

    // Epilogue.  Tile i goes through the ring transposed (lane (rq, c4) then holds four channels of rows rq + 8 k); a row that is
    // the SECOND of a kept time pair (tl odd, inside T & ~1) meets its partner FT <= 32 rows back, in this tile or the previous one.
    float* ring = (float*)lds + wave * 2048;
    const int rq = lane >> 3, c4 = (lane & 7) * 4;
    const int Tp = T >> 1;
    __bf16* const yb = y + (size_t)b * Tp * F * Cout + co0 + c4;
#pragma unroll
    for (int i = 0; i < CB_MTW; ++i) {
        if (i * 32 >= MROWS) break;
        const int slot = (i & 1) * 1024;
#pragma unroll
        for (int j = 0; j < 16; ++j) ring[slot + ((j & 3) + 8 * (j >> 2) + 4 * h) * 32 + r] = acc[i][j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pb = i * 32 + rq + 8 * k;
            const int tl = pb / FT, f = pb - tl * FT;
            if (pb < MROWS && (tl & 1) && t0 + tl < 2 * Tp && f0 + f < F) {
                const f32x4 vb = *(const f32x4*)(ring + (pb & 63) * 32 + c4);
                const f32x4 va = *(const f32x4*)(ring + ((pb - FT) & 63) * 32 + c4);
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (__bf16)fmaxf(fmaxf(va[e], vb[e]), 0.f);
                *(bf16x4*)(yb + ((size_t)((t0 + tl) >> 1) * F + f0 + f) * Cout) = o;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int NW, int CCH, bool XBF>
int launch_conv(const Bf16Plan& p, const void* x, const __bf16* wf, const float* bias, __bf16* y, int B, int Cin, int F, int T,
                int Cout, hipStream_t s) {
    auto k = conv3x3_bf16_eval_k<NW, CCH, XBF>;
    if (p.lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) { sed_set_error("hipFuncSetAttribute(%zu B LDS): %s", p.lds, hipGetErrorString(e)); return (int)e; }
    }
    dim3 grid(p.tblocks * p.nft, B, Cout / (32 * NW));
    k<<<grid, 64 * NW, p.lds, s>>>(x, (const bf16x8*)wf, bias, y, Cin, F, T, Cout, p.TT, p.FT, p.nft, p.tp);
    return 0;
}

template <int NW, bool XBF>
int launch_conv_c(const Bf16Plan& p, const void* x, const __bf16* wf, const float* bias, __bf16* y, int B, int Cin, int F, int T,
                  int Cout, hipStream_t s) {
    switch (p.cch) {
        case 128: return launch_conv<NW, 128, XBF>(p, x, wf, bias, y, B, Cin, F, T, Cout, s);
        case 64: return launch_conv<NW, 64, XBF>(p, x, wf, bias, y, B, Cin, F, T, Cout, s);
        default: return launch_conv<NW, 32, XBF>(p, x, wf, bias, y, B, Cin, F, T, Cout, s);
    }
}

// ───────────────────────── GEMM ─────────────────────────
// C[M][N] = A[M][K] B[N][K]^T + bias (A, B bf16 row-major, C fp32 with leading dimension ldc), K % 32 == 0.  Workgroup tile 128 x 128,
// k-tiles of 32 through LDS (the next one prefetched into registers under the MFMAs of the current one); wave w computes the
// 64 x 64 quadrant (w / 2, w % 2) as 2 x 2 MFMA tiles.  No split-K: every element sums its k-tiles in one fixed order whatever M,
// so a batch equals its chunks bit for bit.  Rows of A / B past M / N are read clamped and never stored.
#define GB_PITCH 80   // bytes per LDS row of 32 bf16 (+16: conflict-free ds_read_b128 columns)
__global__ __launch_bounds__(256) void gemm_bf16_nt_k(const __bf16* __restrict__ A, const __bf16* __restrict__ Bm,
                                                      const float* __restrict__ bias, float* __restrict__ Cm, int M, int N, int K, long ldc) {
    __shared__ __attribute__((aligned(16))) char sa[128 * GB_PITCH];
    __shared__ __attribute__((aligned(16))) char sb[128 * GB_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * 128, n0 = blockIdx.x * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    // staging: 128 rows x 4 16-byte units per operand, two units per thread
    int srow[2], sq[2];
    const __bf16* pa[2];
    const __bf16* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = tid + u * 256;
        srow[u] = i >> 2; sq[u] = i & 3;
        const int am = m0 + srow[u] < M ? m0 + srow[u] : M - 1, bn = n0 + srow[u] < N ? n0 + srow[u] : N - 1;
        pa[u] = A + (size_t)am * K + sq[u] * 8;
        pb[u] = Bm + (size_t)bn * K + sq[u] * 8;
    }
    u32x4 ra[2], rb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { ra[u] = *(const u32x4*)pa[u]; rb[u] = *(const u32x4*)pb[u]; }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int nk = K >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            *(u32x4*)(sa + srow[u] * GB_PITCH + sq[u] * 16) = ra[u];
            *(u32x4*)(sb + srow[u] * GB_PITCH + sq[u] * 16) = rb[u];
        }
        __syncthreads();
        if (kt + 1 < nk) {
#pragma unroll
            for (int u = 0; u < 2; ++u) { ra[u] = *(const u32x4*)(pa[u] + (size_t)(kt + 1) * 32); rb[u] = *(const u32x4*)(pb[u] + (size_t)(kt + 1) * 32); }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = *(const bf16x8*)(sa + (wm + i * 32 + r) * GB_PITCH + ks * 32 + h * 16);
                fb[i] = *(const bf16x8*)(sb + (wn + i * 32 + r) * GB_PITCH + ks * 32 + h * 16);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
    // lane holds column n = wn + 32 j + r of rows (e & 3) + 8 (e >> 2) + 4 h of each 32-row tile
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + j * 32 + r;
        if (n >= N) continue;
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m < M) Cm[(size_t)m * ldc + n] = acc[i][j][e] + bn;
            }
    }
}

}  // namespace

extern "C" int sed_conv3x3_bf16_eval_supported(int B, int Cin, int F, int T, int Cout) {
    return bf16_plan(B, Cin, F, T, Cout).ok;
}

extern "C" int sed_conv3x3_bf16_pack_weights_bn_folded(const float* w, const float* bias, const float* gamma, const float* beta,
                                                       const float* running_mean, const float* running_var, float eps,
                                                       void* wf_bf16, float* bias_folded, int Cout, int Cin, void* stream) {
    SED_REQUIRE(w && gamma && beta && running_mean && running_var && wf_bf16 && bias_folded, "conv3x3_bf16_pack_weights_bn_folded: null pointer");
    SED_REQUIRE(Cout > 0 && Cin > 0 && Cout % 32 == 0 && Cin % 16 == 0, "conv3x3_bf16_pack_weights_bn_folded: Cout=%d Cin=%d (need Cout %% 32, Cin %% 16 == 0)", Cout, Cin);
    const float* ws[1] = {w}; const float* bs[1] = {bias}; const float* gm[1] = {gamma}; const float* bt[1] = {beta};
    const float* rm[1] = {running_mean}; const float* rv[1] = {running_var};
    float* wf[1] = {nullptr}; float* sc[1] = {nullptr}; float* sh[1] = {nullptr}; float* bf[1] = {bias_folded};
    void* wb[1] = {wf_bf16};
    const int fold[1] = {1}, wn[1] = {0}, co[1] = {Cout}, ci[1] = {Cin};
    return sed_internal_conv_pack_eval(1, ws, bs, gm, bt, rm, rv, eps, wf, sc, sh, bf, fold, wn, co, ci, nullptr, nullptr, nullptr, 0, 0, 0,
                                       wb, 0, stream);
}

extern "C" int sed_conv3x3_bf16_bn_relu_pool_eval(const void* x, int x_is_bf16, const void* wf_bf16, const float* bias_folded,
                                                  void* pooled_bf16, int B, int Cin, int F, int T, int Cout, void* stream) {
    SED_REQUIRE(x && wf_bf16 && bias_folded && pooled_bf16, "conv3x3_bf16_bn_relu_pool_eval: null pointer");
    const Bf16Plan p = bf16_plan(B, Cin, F, T, Cout);
    SED_REQUIRE(p.ok, "conv3x3_bf16_bn_relu_pool_eval: shape B=%d Cin=%d F=%d T=%d Cout=%d is not supported "
                "(sed_conv3x3_bf16_eval_supported: Cin %% 32 == 0, Cout %% 64 == 0, T >= 2)", B, Cin, F, T, Cout);
    hipStream_t s = as_stream(stream);
    SedProfScope prof(SED_K_CONV_MFMA_FWD, s, 2.0 * 9.0 * Cin * Cout * (double)B * T * F);
    const __bf16* wf = (const __bf16*)wf_bf16;
    __bf16* y = (__bf16*)pooled_bf16;
    int rc;
    if (p.nw == 4) rc = x_is_bf16 ? launch_conv_c<4, true>(p, x, wf, bias_folded, y, B, Cin, F, T, Cout, s)
                                  : launch_conv_c<4, false>(p, x, wf, bias_folded, y, B, Cin, F, T, Cout, s);
    else rc = x_is_bf16 ? launch_conv_c<2, true>(p, x, wf, bias_folded, y, B, Cin, F, T, Cout, s)
                        : launch_conv_c<2, false>(p, x, wf, bias_folded, y, B, Cin, F, T, Cout, s);
    SED_TRY(rc);
    SED_LAUNCH_CHECK("conv3x3_bf16_bn_relu_pool_eval");
    return 0;
}

extern "C" int sed_gemm_bf16_nt(const void* A, const void* B, const float* bias, float* C, long ldc, int M, int N, int K, void* stream) {
    SED_REQUIRE(A && B && C, "gemm_bf16_nt: null pointer");
    SED_REQUIRE(M > 0 && N > 0 && K > 0 && K % 32 == 0 && ldc >= N, "gemm_bf16_nt: M=%d N=%d K=%d ldc=%ld (need K %% 32 == 0, ldc >= N)", M, N, K, ldc);
    SED_REQUIRE(M <= 65535 * 128, "gemm_bf16_nt: M=%d exceeds the grid", M);
    hipStream_t s = as_stream(stream);
    SedProfScope prof(SED_K_GEMM, s, 2.0 * M * N * (double)K);
    gemm_bf16_nt_k<<<dim3(cdiv(N, 128), cdiv(M, 128)), 256, 0, s>>>((const __bf16*)A, (const __bf16*)B, bias, C, M, N, K, ldc);
    SED_LAUNCH_CHECK("gemm_bf16_nt");
    return 0;
}
