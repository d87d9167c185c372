// fft2048.h — the register-resident 2048-point real FFT of logmel.hip, gcc.hip and tdoa.hip: the layout of the constant blob
// (window, inter-pass and pairing twiddles) and its staging into LDS, the lane geometry, complex points in VGPR pairs, the
// 32-point transform, the half-wave exchange through LDS (store and read-back), the guarded frame load, the two passes from
// samples to Z (fft2048_passes) and the pairing pass from Z to the complex half spectrum (fft2048_spectrum) — and, for mvdr.hip,
// the way back from a half spectrum to the windowed frame (ifft2048_unpair, ifft2048_passes).  Everything is
// force-inlined into the kernels that use it; what a kernel keeps for itself is its fast (unguarded) load path and, in
// logmel.hip, a pairing pass of its own that produces power bins.
#pragma once
#include "common.h"

#define LM_NFFT 2048
#define LM_N 1024                     // complex points
#define LM_TSTRIDE 33                 // floats per row of the 32x32 transpose (conflict-free both ways)
#define LM_SCR (32 * LM_TSTRIDE)      // 1056 floats >= 1025 power bins
#define LM_MAX_MELS 128
#define LM_PART (32 + LM_MAX_MELS)    // partial-sum slots per frame (plan 1: 2 per stored pair + the zero slot)
#define LM_TRI_BINS 33
#define LM_FRAME_SCR (LM_SCR + LM_PART)
#define LM_HDR 8                      // table header words

// table blob (32-bit words):  [0] magic  [1] n_mels  [2] iters  [3] n_slots  [4] total words  [5] plan (0 list, 1 two-band)  [6..7] 0
//   win  [2048]            window, natural order
//   tw   [32][32] float2   tw[q][r] = exp(-2 pi i r q / 1024)
//   pw   [513]   float2    exp(-2 pi i k / 2048), k = 0..512 (+ 1 pad float2)
//  plan 0 (any sparse bank): band-major list of the non-zeros, 1/32 of it per lane
//   ent  [iters][32] {float weight*0.25, u32 meta}    meta = k | emit << 11 | slot << 12
//   band [n_mels] u32      first_slot | count << 16
//  plan 1 (every bin feeds at most two ADJACENT bands — triangular banks such as librosa's): lane r owns the 33
//  consecutive bins 33r .. 33r+32, keeps one accumulator for the lower and one for the upper band of the current bin and
//  stores the pair whenever the band pair changes (iters = 33)
//   ent  [33][32] {float w_lower*0.25, float w_upper*0.25, u32 pair_slot (float index into part, even) or ~0, 0}
//   band [n_mels][8] u16   float indices into part of the partial sums of the band (unused = the always-zero slot)
#define LM_MAGIC 0x4C4D3332u
#define LM_OFF_WIN LM_HDR
#define LM_OFF_TW (LM_OFF_WIN + 2048)
#define LM_OFF_PW (LM_OFF_TW + 2048)
#define LM_OFF_ENT (LM_OFF_PW + 1028)

namespace {

__device__ __forceinline__ constexpr int brev5(int k) {
    return ((k & 1) << 4) | ((k & 2) << 2) | (k & 4) | ((k & 8) >> 2) | ((k & 16) >> 4);
}

// A complex point lives in ONE aligned VGPR pair (re, im): the butterfly's u + v / u - v are one v_pk_add_f32 each and a twiddle
// multiply (dr C + di S, di C - dr S) = d * (C, C) + swap(d) * (S, -S) is v_pk_mul_f32 + v_pk_fma_f32 — hipcc folds the swap into the
// instruction's op_sel bits, so there is no register shuffling: 259 vector instructions per 32-point transform instead of 456
// with separate re[] / im[] arrays (round 2 found the SLP vectoriser's packing of those arrays useless: it paid for every packed
// add with moves that built the pairs; here the pairs are how the data is loaded — global_load_dwordx2 of (x[2n], x[2n+1])).
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 swp(f2 a) { return __builtin_shufflevector(a, a, 1, 0); }
// The forms hipcc does not find by itself (it negates and moves halves with v_xor / v_mov instead) are written with the VOP3P
// modifiers spelled out: op_sel[i] = 1 takes the HIGH half of source i for the low result, op_sel_hi[i] = 0 the LOW half for the
// high result; neg_lo / neg_hi negate source i for the low / high result.  Plain (non-volatile) asm: free to be scheduled.
__device__ __forceinline__ f2 cmul(f2 x, f2 w) {               // x * w (complex): (xr wr - xi wi, xr wi + xi wr)
    f2 t, d;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "v"(x), "v"(w));                                   // (xr wr, xi wr)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[0,1,0]" : "=v"(d) : "v"(x), "v"(w), "v"(t));   // + (-xi wi, xr wi)
    return d;
}
__device__ __forceinline__ f2 sub_rot(f2 a, f2 b) {            // -i (a - b) = (a.y - b.y, b.x - a.x)
    f2 d;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f2 add_conj(f2 a, f2 b) {           // a + conj(b) = (a.x + b.x, a.y - b.y)
    f2 d;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f2 rot_sub_conj(f2 a, f2 b) {       // -i (a - conj(b)) = (a.y + b.y, b.x - a.x)
    f2 d;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[0,0] neg_hi:[1,0]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// 32-point DIF FFT in registers, forward sign; result X[k] = z[brev5(k)].  All indices are compile-time constants.
__device__ __forceinline__ void fft32(f2 (&z)[32]) {
    constexpr float C32[16] = {1.0f, 0.98078528040323044913f, 0.92387953251128675613f, 0.83146961230254523708f,
                               0.70710678118654752440f, 0.55557023301960222474f, 0.38268343236508977173f,
                               0.19509032201612826785f, 0.0f, -0.19509032201612826785f, -0.38268343236508977173f,
                               -0.55557023301960222474f, -0.70710678118654752440f, -0.83146961230254523708f,
                               -0.92387953251128675613f, -0.98078528040323044913f};
    constexpr float S32[16] = {0.0f, 0.19509032201612826785f, 0.38268343236508977173f, 0.55557023301960222474f,
                               0.70710678118654752440f, 0.83146961230254523708f, 0.92387953251128675613f,
                               0.98078528040323044913f, 1.0f, 0.98078528040323044913f, 0.92387953251128675613f,
                               0.83146961230254523708f, 0.70710678118654752440f, 0.55557023301960222474f,
                               0.38268343236508977173f, 0.19509032201612826785f};
#pragma unroll
    for (int h = 16; h >= 1; h >>= 1) {
#pragma unroll
        for (int blk = 0; blk < 32; blk += 2 * h) {
#pragma unroll
            for (int j = 0; j < h; ++j) {
                const int i0 = blk + j, i1 = i0 + h;
                const int m = j * (16 / h);                 // twiddle W_32^m = C32[m] - i S32[m]
                const f2 u = z[i0], v = z[i1];
                z[i0] = u + v;
                if (m == 0) z[i1] = u - v;
                else if (m == 8) z[i1] = sub_rot(u, v);      // W_32^8 = -i
                else { const f2 d = u - v; z[i1] = d * (f2){C32[m], C32[m]} + swp(d) * (f2){S32[m], -S32[m]}; }
            }
        }
    }
}

__device__ __forceinline__ void wave_lds_fence() {
    // LDS operations of ONE wave are executed in order by the hardware; this only stops the compiler from moving
    // them across the point where another lane of the same wave takes over the data
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Eight rows of the pass-1 -> pass-2 exchange in one statement: ds_write_addtid_b32 stores 4 B per lane at
// M0 + offset + 4*lane without an address register and at twice the rate of ds_write_b32 (MI355X_MICROARCH.md, LDS).  Row k
// of the wave's 32 x 65-float exchange buffer starts at byte 260*k (the odd row stride makes the column reads of pass 2
// conflict-free).  M0 is compiler-reserved: saved and restored inside the statement; the s_nop covers the
// SALU-writes-M0 -> LDS-add-TID wait state.  No VGPR is written, so the statement needs no completion count of its own
// (LDS operations of one wave complete in order).
#define LM_ROW_BYTES 260
template <int K0>
__device__ __forceinline__ void addtid_store8(unsigned base, float a0, float a1, float a2, float a3, float a4, float a5,
                                              float a6, float a7) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %9\n\ts_nop 0\n\t"
                 "ds_write_addtid_b32 %1 offset:%10\n\tds_write_addtid_b32 %2 offset:%11\n\t"
                 "ds_write_addtid_b32 %3 offset:%12\n\tds_write_addtid_b32 %4 offset:%13\n\t"
                 "ds_write_addtid_b32 %5 offset:%14\n\tds_write_addtid_b32 %6 offset:%15\n\t"
                 "ds_write_addtid_b32 %7 offset:%16\n\tds_write_addtid_b32 %8 offset:%17\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(a0), "v"(a1), "v"(a2), "v"(a3), "v"(a4), "v"(a5), "v"(a6), "v"(a7), "s"(base),
                   "i"((K0 + 0) * LM_ROW_BYTES), "i"((K0 + 1) * LM_ROW_BYTES), "i"((K0 + 2) * LM_ROW_BYTES),
                   "i"((K0 + 3) * LM_ROW_BYTES), "i"((K0 + 4) * LM_ROW_BYTES), "i"((K0 + 5) * LM_ROW_BYTES),
                   "i"((K0 + 6) * LM_ROW_BYTES), "i"((K0 + 7) * LM_ROW_BYTES)
                 : "memory");
}
// rows k1 = 0..31 of one component (IMAG = 0: real parts, 1: imaginary parts): row k1 holds X[k1] = z[brev5(k1)] of every lane
template <int IMAG>
__device__ __forceinline__ void exchange_store(unsigned base, const f2 (&z)[32]) {
#define LM_C(k) (IMAG ? z[brev5(k)].y : z[brev5(k)].x)
    addtid_store8<0>(base, LM_C(0), LM_C(1), LM_C(2), LM_C(3), LM_C(4), LM_C(5), LM_C(6), LM_C(7));
    addtid_store8<8>(base, LM_C(8), LM_C(9), LM_C(10), LM_C(11), LM_C(12), LM_C(13), LM_C(14), LM_C(15));
    addtid_store8<16>(base, LM_C(16), LM_C(17), LM_C(18), LM_C(19), LM_C(20), LM_C(21), LM_C(22), LM_C(23));
    addtid_store8<24>(base, LM_C(24), LM_C(25), LM_C(26), LM_C(27), LM_C(28), LM_C(29), LM_C(30), LM_C(31));
#undef LM_C
}

__device__ __forceinline__ float pcm_at(const float* __restrict__ pcm, long n, long n_samples, int pad_mode) {
    if (n >= 0 && n < n_samples) return pcm[n];
    if (pad_mode == 1 && n_samples > 1) {                    // numpy 'reflect' (no edge repeat)
        const long period = 2 * (n_samples - 1);
        long r = n % period;
        if (r < 0) r += period;
        if (r >= n_samples) r = period - r;
        return pcm[r];
    }
    return 0.f;
}

// ── what a kernel sets up once per workgroup ──
// the constant blob (`words` 32-bit words, a multiple of 4): global -> LDS word 0; the caller's barrier makes it visible
__device__ __forceinline__ void fft_stage_tables(float* lds, const uint32_t* __restrict__ tables, int words, int tid, int threads) {
    const f32x4* src = reinterpret_cast<const f32x4*>(tables);
    f32x4* dst = reinterpret_cast<f32x4*>(lds);
    for (int i = tid; i < words / 4; i += threads) dst[i] = src[i];
}
// A half wave (32 lanes) transforms one frame.  Lane (half, r) holds column r of the frame's 32 x 32 points; `partner` is the
// lane of the same half that holds column (32 - r) % 32, the mirror the pairing pass reads; `xbase` is the LDS byte address
// (wave-uniform, in an SGPR) of the wave's 32 x 65-float exchange buffer, which starts `wscr_off` floats into the dynamic LDS
// array.  (The caller subtracts the array itself, wscr - lds: behind a pointer parameter hipcc no longer folds the difference.)
// half, r and partner are functions of `lane` and not stored values so that every function below that takes an FftLane
// spells out r = lane & 31 in its own body: hipcc simplifies a function before it inlines it, and what it makes of an index
// such as 1024 - (r + 32 k2) depends on whether it knows r < 32 at that point.
struct FftLane {
    int lane;
    unsigned xbase;
    __device__ __forceinline__ int half() const { return lane >> 5; }
    __device__ __forceinline__ int r() const { return lane & 31; }
    __device__ __forceinline__ int partner() const { return (lane & 32) | ((32 - r()) & 31); }
};
__device__ __forceinline__ FftLane fft_lane(int lane, ptrdiff_t wscr_off) {
    const unsigned xbase = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)wscr_off * 4u +
                                                          (unsigned)__builtin_amdgcn_groupstaticsize());
    return FftLane{lane, xbase};
}

// The read-back of the exchange: z[n2].x (IMAG = 0) or .y (IMAG = 1) = column 32 half + n2 of row r, xaddr = its byte address.
// Single-dword reads straight into the halves of the register pairs: left to hipcc these become ds_read2_b32 into scratch
// pairs + 64 v_mov to split them — LDS issue slots are cheaper here than vector ones.
// THE HAZARD.  To the compiler an asm output is valid the moment its statement ends, but a ds_read_b32's data arrives only
// behind the s_waitcnt below, which hipcc does not know belongs to the reads.  Anything it places between a read and the wait
// that touches a destination — a v_mov, a spill, a copy to an AGPR — captures stale data, and the returning read then lands
// in a register that may have been given to something else.  What guards against it: every statement is volatile (kept in
// order, nothing of them is duplicated or dropped), the empty "+v" statements behind the wait pin each destination pair as
// live and in a VGPR there, the build refuses scratch in every kernel that uses this (build.py, NO_SCRATCH_KERNELS), and
// tests/test_cpu_fft_exchange_isa.py asserts on the compiled code that nothing but the 32 reads stands between the first
// read and the wait.  (One asm statement with 32 early-clobber outputs would make it structural; it changes register
// allocation and is to be measured on its own.)
template <int IMAG>
__device__ __forceinline__ void exchange_load(unsigned xaddr, f2 (&z)[32]) {
#pragma unroll
    for (int n2 = 0; n2 < 32; ++n2) {
        float t;
        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(t) : "v"(xaddr), "i"(n2 * 4));
        if (IMAG) z[n2].y = t;
        else z[n2].x = t;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int n2 = 0; n2 < 32; ++n2) asm volatile("" : "+v"(z[n2]));
}

// The guarded frame load (edge frames, odd hop, unaligned clips, a ring that wraps): z[n1] = (x[64 n1 + 2r], x[64 n1 + 2r + 1])
// with x[off] = sample(off), 0 <= off < 2048, staged through the half wave's 1024 floats `scr` so that this cold path costs
// no registers (dynamic index, not unrolled).
template <typename Sample>
__device__ __forceinline__ void fft_load_guarded(f2 (&z)[32], float* scr, const FftLane& fl, Sample sample) {
    const int r = fl.r();
    wave_lds_fence();
#pragma unroll 1
    for (int n1 = 0; n1 < 32; ++n1) scr[n1 * 32 + r] = sample(64 * n1 + 2 * r);
    wave_lds_fence();
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) z[n1].x = scr[n1 * 32 + r];
    wave_lds_fence();
#pragma unroll 1
    for (int n1 = 0; n1 < 32; ++n1) scr[n1 * 32 + r] = sample(64 * n1 + 2 * r + 1);
    wave_lds_fence();
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) z[n1].y = scr[n1 * 32 + r];
}

// Samples to Z: z[n1] = (x[64 n1 + 2r], x[64 n1 + 2r + 1]) on entry, Z[r + 32 k2] = z[brev5(k2)] on return.
__device__ __forceinline__ void fft2048_passes(f2 (&z)[32], const FftLane& fl, const f2* s_win, const f2* s_tw) {
    const int r = fl.r(), half = fl.half();
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) z[n1] *= s_win[32 * n1 + r];
    // ── pass 1: FFT over n1, twiddle W_1024^{r k1} ──
    fft32(z);
#pragma unroll
    for (int k1 = 1; k1 < 32; ++k1) {
        const int b = brev5(k1);
        z[b] = cmul(z[b], s_tw[k1 * 32 + r]);
    }
    // ── exchange through LDS (real parts, then imaginary parts, the wave's 32 x 65 buffer): lane (half, r) holds
    //    A[r][k1] and stores row k1 lane-linearly; lane (half, c) then needs A[n2][c] = row c, column 32*half + n2 ──
    wave_lds_fence();                                        // whatever read the buffer before (a mel pass, a guarded load) is done
    exchange_store<0>(fl.xbase, z);
    wave_lds_fence();
    const unsigned xaddr = fl.xbase + (unsigned)(r * LM_ROW_BYTES + 128 * half);
    exchange_load<0>(xaddr, z);                              // (the .y halves — the imaginary parts — are still to be stored)
    wave_lds_fence();
    exchange_store<1>(fl.xbase, z);
    wave_lds_fence();
    exchange_load<1>(xaddr, z);
    wave_lds_fence();
    // ── pass 2: FFT over n2 ──
    fft32(z);
}

// Z to the complex half spectrum spec[0..1024] of the real frame (LDS):
// 2 X[k] = (Z[k] + conj Z[N-k]) - i W_2048^k (Z[k] - conj Z[N-k]) = e + t, and 2 X[N-k] = conj(e - t); lane r owns k = r + 32 k2,
// k2 < 16, and its mirror N-k, whose Z lives in lane (32 - r) % 32, register 31 - k2 (lane 0: its own register 32 - k2).
__device__ __forceinline__ void fft2048_spectrum(const f2 (&z)[32], const FftLane& fl, const f2* s_pw, float2* spec) {
    const int r = fl.r(), partner = fl.partner();
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) {
        const int bp = brev5(31 - k2), b0 = brev5((32 - k2) & 31);
        f2 pp = {__shfl(z[bp].x, partner, 64), __shfl(z[bp].y, partner, 64)};
        if (r == 0) pp = z[b0];
        const f2 zz = z[brev5(k2)];
        const int k = r + 32 * k2;
        const f2 e = add_conj(zz, pp);
        const f2 q = rot_sub_conj(zz, pp);
        const f2 t = cmul(q, s_pw[k]);
        const f2 a = e + t, bb = e - t;
        spec[k] = make_float2(0.5f * a.x, 0.5f * a.y);
        spec[LM_N - k] = make_float2(0.5f * bb.x, -0.5f * bb.y);
    }
    if (r == 0) { const f2 zz = z[brev5(16)]; spec[512] = make_float2(zz.x, -zz.y); }      // X[512] = conj Z[512]
}

// ── the inverse: a half spectrum back to its real frame (mvdr.hip), from the pieces above ──
// The forward pairing read backwards.  With z[n] = x[2n] + i x[2n+1] and Z = FFT_1024(z), the half spectrum Y[0..1024] of the real
// frame x gives 2 conj Z[k] = (a + b) - i W_2048^k (a - b) with a = conj Y[k], b = Y[N-k]; x is then conj(FFT_1024(2 conj Z)) / 2048:
// the SAME two forward 32-point passes.  Lane r takes k = r + 32 n1 into register n1 — the order the passes read — and reads its own
// 2 x 32 bins of `spec` (LDS): no shuffles.  W^k for k > 512 is -conj W^(1024-k), from the 513 pairing twiddles.  The imaginary
// parts of Y[0] and Y[1024] must be 0 in `spec` (a real frame has none; the caller drops them).
__device__ __forceinline__ void ifft2048_unpair(f2 (&z)[32], const FftLane& fl, const f2* s_pw, const float2* spec) {
    const int r = fl.r();
#pragma unroll
    for (int n1 = 0; n1 < 32; ++n1) {
        const int k = r + 32 * n1;
        const float2 ya = spec[k], yb = spec[LM_N - k];
        const f2 a = {ya.x, -ya.y}, b = {yb.x, yb.y};
        f2 w;
        if (n1 < 16) w = s_pw[k];                                // (k <= 511)
        else { const f2 t = s_pw[LM_N - k]; w = (f2){-t.x, t.y}; }   // (k = 512: -conj W^512 = W^512)
        const f2 e = a + b, u = cmul(a - b, w);
        z[n1] = e + (f2){u.y, -u.x};                             // e - i u
    }
}

// 2 conj Z (register n1 of lane r = point r + 32 n1) to the frame, windowed for the overlap-add: on return
// z[brev5(k2)] = (win[2m] x[2m], win[2m+1] x[2m+1]), m = r + 32 k2.  fft2048_passes without its window on the way in; the scale
// 1/2048 is a power of two, so every output is the transform's value times the window's, rounded once.
__device__ __forceinline__ void ifft2048_passes(f2 (&z)[32], const FftLane& fl, const f2* s_win, const f2* s_tw) {
    const int r = fl.r(), half = fl.half();
    fft32(z);
#pragma unroll
    for (int k1 = 1; k1 < 32; ++k1) {
        const int b = brev5(k1);
        z[b] = cmul(z[b], s_tw[k1 * 32 + r]);
    }
    wave_lds_fence();                                        // whatever read the buffer before (the forward transform) is done
    exchange_store<0>(fl.xbase, z);
    wave_lds_fence();
    const unsigned xaddr = fl.xbase + (unsigned)(r * LM_ROW_BYTES + 128 * half);
    exchange_load<0>(xaddr, z);
    wave_lds_fence();
    exchange_store<1>(fl.xbase, z);
    wave_lds_fence();
    exchange_load<1>(xaddr, z);
    wave_lds_fence();
    fft32(z);
#pragma unroll
    for (int k2 = 0; k2 < 32; ++k2) {
        const int b = brev5(k2);
        z[b] = (z[b] * (f2){1.0f / LM_NFFT, -1.0f / LM_NFFT}) * s_win[r + 32 * k2];
    }
}

}  // namespace
