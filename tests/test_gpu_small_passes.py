"""The small streaming and reduction kernels of the fit step (csrc/bnpool.hip, csrc/misc.hip), each on its own against the numpy
float64 restatement of tests/small_passes_ref.py, at the smallest shapes that make a workgroup walk past its grid cap, iterate
its row loops and reach its tails.

No tolerance is chosen: every bound is k * 2^-24 * magnitude, k the counted fp32 roundings on the kernel's path (the length of a
per-thread fp32 accumulation included) and magnitude the float64 sum of the absolute operands (small_passes_ref.bound; the
count stands beside each use).  Chains with a division, root, logarithm or power (Adam, the losses) carry their roundings
through the first-order error arithmetic of class V instead, one rounding per operation.  expf, logf, log1pf, powf and sqrtf
are allowed 4 ulp (= 8 * 2^-24 relative) each: the ROCm install here carries no table of their errors.  Every test prints
max(error / bound) as a `[ratio]` line and asserts it <= 1.

Inputs of the BatchNorm/pool passes go through repair_near_ties, so no arg-max or ReLU decision of the float64 reference is
within 1e-4 of flipping: every element is compared, none is masked out."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_passes_ref as R  # noqa: E402
from small_passes_ref import TINY, U, bound  # noqa: E402

pytestmark = pytest.mark.gpu
SLACK = 1.0 + 2.0 ** -20            # the second-order terms the first-order propagations below drop
D = 2.0 ** -53                      # unit roundoff of the double accumulators


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ratio(name, got, want, bnd):
    """max(|got - want| / bound), printed; non-finite device values count as infinite"""
    got, want, bnd = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bnd, np.float64), np.shape(want))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = np.where(np.isfinite(got), np.abs(got - want), np.inf)
    r = float(np.max(err / bnd)) if err.size else 0.0
    print(f"[ratio] {name}: {r:.4f}")
    return r


def hold(name, got, want, bnd):
    r = ratio(name, got, want, bnd)
    if not r <= 1.0:
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / np.broadcast_to(bnd, np.shape(want))
        i = np.unravel_index(int(np.nanargmax(np.where(np.isfinite(err), err, np.inf))), err.shape)
        raise AssertionError(f"{name}: error / bound = {r:.4g} at {i}: got {np.asarray(got)[i]!r}, want {np.asarray(want)[i]!r}")
    return r


# ═════════════════════════ A. reductions that accumulate in double ═════════════════════════
def _partials(rng, rows, C, mean):
    """[rows,2,C] fp32 partial sums (sum x, sum x^2 of 8 samples x = mean + randn each) -> (partials, count)"""
    x = (mean + rng.standard_normal((rows, 8, C))).astype(np.float32).astype(np.float64)
    return np.stack([x.sum(1), (x * x).sum(1)], 1).astype(np.float32), rows * 8.0


def _finaliser_bounds(ref, gamma, beta, rm0, rv0, mom, eps, count, dm, dvar):
    """what the kernel's fp32 tail may add to errors dm, dvar of the mean and the variance it starts from (sed_bn_train_channel):
    mean = fl(m): 1 rounding.  rstd = fl(1 / sqrt(var + eps)), double until the cast: the variance error through the exact
    function, then 1.  scale = fl(g rstd): 1 more.  shift = fl(bt - fl(fl(m) scale)): product rule, 1 for the product, 1 for the
    difference.  running = fl(fl(fl(1 - mom) r) + fl(mom fl(x))): 2 on the first term, 1 on the second, 1 for the sum."""
    m, var, r, sc = ref["mean"], ref["var"], ref["rstd"], ref["scale"]
    g, bt = np.abs(np.asarray(gamma, np.float64)), np.abs(np.asarray(beta, np.float64))
    b = {"mean": dm + U * np.abs(m)}
    r_hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    r_lo = 1.0 / np.sqrt(var + dvar + eps)
    b["rstd"] = np.maximum(r_hi - r, r - r_lo) + U * r_hi
    b["scale"] = g * b["rstd"] + U * g * r_hi
    b["shift"] = np.abs(m) * b["scale"] + np.abs(sc) * b["mean"] + b["mean"] * b["scale"] + U * np.abs(m * sc) + U * (bt + np.abs(m * sc))
    dunb = dvar * (count / (count - 1.0) if count > 1 else 1.0)
    b["rmean"] = 3 * U * np.abs((1 - mom) * rm0) + mom * b["mean"] + 2 * U * mom * np.abs(m)
    b["rvar"] = 3 * U * np.abs((1 - mom) * rv0) + mom * (dunb + U * ref["unb"]) + 2 * U * mom * ref["unb"]
    return {k: v * SLACK + TINY for k, v in b.items()}


def _hold_finaliser(tag, outs, rm, rv, ref, bnds):
    got = dict(zip(("mean", "rstd", "scale", "shift"), map(host, outs)), rmean=host(rm), rvar=host(rv))
    return max(hold(f"{tag} {k}", got[k], ref[k], bnds[k]) for k in ("mean", "rstd", "scale", "shift", "rmean", "rvar"))


FIN_ROWS, FIN_C = (1, 2, 511, 512, 513, 1061, 4096), (1, 2, 7, 128)


@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_finalize_train_is_the_fp32_rounding_of_the_float64_statistics(ops, rows):
    """sed_bn_finalize_train over rows that leave, fill and overrun the 512 row slices of its two-channel workgroup (rows 513,
    1061, 4096 iterate the slice loop; 4096 fills its unroll by 8), odd C for the half-dead workgroup.  The partials come from
    data with mean/sd = 30, so Q/n - m^2 cancels three digits.  The kernel sums in double: against the float64 sums of the same
    fp32 partials its mean and variance may differ by the double accumulation alone ((rows + 8) * 2^-53 of the absolute terms),
    then the fp32 tail of _finaliser_bounds.  rows == 1 also runs with count == 1 (no unbiasing)."""
    worst = 0.0
    for C in FIN_C:
        for count1 in ((False, True) if rows == 1 else (False,)):
            rng = np.random.default_rng([rows, C, count1])
            part, count = _partials(rng, rows, C, 30.0)
            if count1:
                x = (30.0 + rng.standard_normal(C)).astype(np.float32).astype(np.float64)
                part, count = np.stack([x, x * x])[None].astype(np.float32), 1.0
            gamma, beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.3).astype(np.float32)
            rm0, rv0 = (rng.standard_normal(C) * 3).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
            mom, eps = float(np.float32(0.1)), float(np.float32(1e-5))
            p64 = part.astype(np.float64)
            ref = R.bn_finalize(p64[:, 0].sum(0), p64[:, 1].sum(0), count, gamma, beta, rm0, rv0, 0.1, 1e-5)
            qn = p64[:, 1].sum(0) / count
            dm = (rows + 8) * D * np.abs(p64[:, 0]).sum(0) / count
            dvar = 2 * (rows + 8) * D * (qn + ref["mean"] ** 2)
            rm, rv = dev(rm0), dev(rv0)
            outs = ops.bn_finalize_train(dev(part), count, dev(gamma), dev(beta), rm, rv, 0.1, 1e-5)
            bnds = _finaliser_bounds(ref, gamma, beta, rm0.astype(np.float64), rv0.astype(np.float64), mom, eps, count, dm, dvar)
            worst = max(worst, _hold_finaliser(f"A1 rows={rows} C={C} count={count:g}", outs, rm, rv, ref, bnds))
    print(f"[ratio] A1 bn_finalize_train rows={rows}: {worst:.4f}")


@pytest.mark.parametrize("rows", (1, 31, 32, 33, 1000))
def test_bn_stat_sums_then_finalize_from_sums(ops, rows):
    """the multi-rank statistics path: sed_bn_stat_sums (32 row slices x 32 channels per workgroup) and sed_bn_finalize_from_sums.
    The sums are the fp32 rounding of the float64 sums: 1 rounding (+ the double accumulation).  The finaliser is run on those
    fp32 sums and held against the float64 statistics of the unrounded ones: the mean carries the rounding of sum x, and the
    variance Q/n - m^2 the rounding of sum x^2, 2^-24 (m^2 + var), plus the rounding of sum x inside m^2, 2 * 2^-24 m^2 (the
    bound 2^-24 (m^2 + var) alone leaves that second rounding out).  mean/sd = 3 here."""
    worst = 0.0
    for C in (1, 31, 32, 33, 130):
        rng = np.random.default_rng([rows, C, 2])
        part, count = _partials(rng, rows, C, 3.0)
        p64 = part.astype(np.float64)
        A, Q = p64[:, 0].sum(0), p64[:, 1].sum(0)
        sums = ops.bn_stat_sums(dev(part))
        slack = (rows + 8) * D * np.stack([np.abs(p64[:, 0]).sum(0), p64[:, 1].sum(0)])
        worst = max(worst, hold(f"A2 sums rows={rows} C={C}", host(sums), np.stack([A, Q]), bound(1, np.stack([np.abs(A), Q])) + slack))
        gamma, beta = (rng.random(C) + 0.5).astype(np.float32), (rng.standard_normal(C) * 0.3).astype(np.float32)
        rm0, rv0 = (rng.standard_normal(C) * 3).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)
        ref = R.bn_finalize(A, Q, count, gamma, beta, rm0, rv0, 0.1, 1e-5)
        m2, var = ref["mean"] ** 2, Q / count - ref["mean"] ** 2
        dm = U * np.abs(ref["mean"]) + slack[0] / count
        dvar = (U * (m2 + var) + 2 * U * m2) * SLACK + 2 * slack[1] / count
        rm, rv = dev(rm0), dev(rv0)
        outs = ops.bn_finalize_from_sums(sums, count, dev(gamma), dev(beta), rm, rv, 0.1, 1e-5)
        bnds = _finaliser_bounds(ref, gamma, beta, rm0.astype(np.float64), rv0.astype(np.float64), float(np.float32(0.1)),
                                 float(np.float32(1e-5)), count, dm, dvar)
        worst = max(worst, _hold_finaliser(f"A2 finalize rows={rows} C={C}", outs, rm, rv, ref, bnds))
    print(f"[ratio] A2 bn_stat_sums + bn_finalize_from_sums rows={rows}: {worst:.4f}")


@pytest.mark.parametrize("rows", (1, 31, 96, 97, 128, 129, 1000, 1024))
def test_reduce_rows_is_the_fp32_rounding_of_the_float64_sum(ops, rows):
    """sed_reduce_rows: 32 row slices x 8 channels; its 4-way unrolled body runs from 97 rows on.  Double accumulation, so
    1 rounding (+ (rows + 8) * 2^-53 of the absolute terms); the columns past C of a wider row stride hold 1e6 and must stay out."""
    worst = 0.0
    for C in (1, 7, 8, 9, 128):
        for stride in (C, C + 5):
            rng = np.random.default_rng([rows, C, stride])
            part = np.full((rows, stride), 1e6, np.float32)
            part[:, :C] = rng.standard_normal((rows, C)) * 2 + 0.5
            p64 = part[:, :C].astype(np.float64)
            got = ops.reduce_rows(dev(part), C)
            bnd = bound(1, np.abs(p64.sum(0))) + (rows + 8) * D * np.abs(p64).sum(0)
            worst = max(worst, hold(f"A3 rows={rows} C={C} stride={stride}", host(got), p64.sum(0), bnd))
    print(f"[ratio] A3 reduce_rows rows={rows}: {worst:.4f}")


@pytest.mark.parametrize("rows", (1, 513, 1024))
@pytest.mark.parametrize("with_grads", (True, False))
def test_bn_bwd_finalize_sums_its_partial_rows_in_double(ops, rows, with_grads):
    """sed_bn_bwd_finalize (the two-channel workgroup of the forward finaliser over [rows][2][C]): sum_g, sum_gx, and dbeta, dgamma
    as their copies when the pointers are given.  1 rounding (+ the double accumulation)."""
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    worst = 0.0
    for C in (2, 7, 128):
        rng = np.random.default_rng([rows, C, 4])
        part = (rng.standard_normal((rows, 2, C)) * 0.3 + 0.05).astype(np.float32)
        p64 = part.astype(np.float64)
        want = p64.sum(0)
        bnd = bound(1, np.abs(want)) + (rows + 8) * D * np.abs(p64).sum(0)
        sg, sgx, dgm, dbt = (torch.full((C,), float("nan")).cuda() for _ in range(4))
        pd = dev(part)
        check(lib().sed_bn_bwd_finalize(ptr(pd), rows, C, ptr(sg), ptr(sgx), ptr(dgm) if with_grads else None,
                                        ptr(dbt) if with_grads else None, stream_ptr()), "bn_bwd_finalize")
        worst = max(worst, hold(f"A4 sum_g rows={rows} C={C}", host(sg), want[0], bnd[0]), hold(f"A4 sum_gx rows={rows} C={C}", host(sgx), want[1], bnd[1]))
        if with_grads:
            assert torch.equal(dbt, sg) and torch.equal(dgm, sgx)
        else:
            assert bool(torch.isnan(dbt).all()) and bool(torch.isnan(dgm).all())
    print(f"[ratio] A4 bn_bwd_finalize rows={rows} grads={with_grads}: {worst:.4f}")


# ═════════════════════════ B. BatchNorm / ReLU / pool / dropout passes ═════════════════════════
SEED = 0x1234567890ABCDEF


def _block_lib():
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    return check, lib(), ptr, stream_ptr


def _forward(shape, d, tcf, p, state=None, salt=None, want_route=True):
    """the forward (and the route codes) on the device against bn_block_fwd -> worst ratio.
    k = 4: z = fl(fl(y scale) + shift) 2 (an fma has 1), inv_keep = fl(1 / fl(1 - p)) and the product 2 (1 / (1 - p) enters as one
    factor, its own two roundings relative to the product); magnitude (|y scale| + |shift|) / (1 - p) of the winner.  Where the
    reference is 0 by the mask the magnitude is 0 and the device must give an exact 0; the masks are compared on their own."""
    check, L, ptr, stream_ptr = _block_lib()
    B, T, F, C, pf, pt = shape
    Tp, Fp = T // pt, F // pf
    y, sc, sh = dev(d["y"]), dev(d["scale"]), dev(d["shift"])
    keep = R.keep_for((B, Tp, Fp, C), SEED, p, salt)
    ref = R.bn_block_fwd(d["y"], d["scale"], d["shift"], pf, pt, keep, p)
    out = torch.full((B, Tp, C, Fp) if tcf else (B, Tp, Fp, C), float("nan")).cuda()
    check(L.sed_bn_relu_pool_drop_fwd(ptr(y), ptr(sc), ptr(sh), ptr(out), B, T, F, C, pf, pt, int(tcf), p, SEED,
                                      ptr(state), stream_ptr()), "bn_relu_pool_drop_fwd")
    got = host(out.permute(0, 1, 3, 2) if tcf else out)
    tag = f"{'x'.join(map(str, shape))} tcf={int(tcf)} p={p}"
    assert np.array_equal(got != 0, ref["out"] != 0), f"{tag}: the kept / open-gate pattern differs from keep_mask and the gate"
    worst = hold(f"B fwd {tag}", got, ref["out"], bound(4, ref["mag"]))
    if want_route:
        route = torch.full((B, Tp, Fp, C), 255, dtype=torch.uint8).cuda()
        check(L.sed_bn_relu_pool_route(ptr(y), ptr(sc), ptr(sh), ptr(route), B, T, F, C, pf, pt, stream_ptr()), "bn_relu_pool_route")
        assert np.array_equal(route.cpu().numpy(), ref["route"]), f"{tag}: route codes differ"
    return worst


def _backward(shape, d, tcf, p, state=None, salt=None):
    """the backward entries one by one against bn_block_bwd -> worst ratio.
    1. reduce + finalize: a thread adds L = ceil(rows / grid) * ceil(F' / nslots) terms in fp32, the block then adds nslots
       slots, the finaliser sums in double and rounds once.  A term of sum g is fl(dout fl(1 / fl(1 - p))): 2 (with L, the slots
       and the cast: k = L + nslots + 3); a term of sum g xhat adds xhat = fl(fl(y - mean) rstd) 2 and the product 1
       (k = L + nslots + 6), magnitude with |y| + |mean| for the centred value.
    2. apply, fed the REFERENCE sums rounded to fp32: dy = fl(scale (gk - sg - xhat sgx)), sg = fl(sum fl(1 / N)) 2, xhat 2,
       fl(xhat sgx) 1 -> 5 on that term; gk 2; two differences and the product with scale 3: k = 8 on the absolute operands.
    3. sed_reduce_rows of the dbias partials against sum dy: the 8 of each dy, La + nslots fp32 additions (La the dy values a
       thread writes: pf pt per window plus its share of both tails), 1 for the cast: k = 8 + La + nslots + 1 on sum |operands|."""
    check, L, ptr, stream_ptr = _block_lib()
    B, T, F, C, pf, pt = shape
    Tp, Fp = T // pt, F // pf
    rng = np.random.default_rng(list(shape) + [7])
    dout = (rng.standard_normal((B, Tp, Fp, C)) * 0.1).astype(np.float32)
    keep = R.keep_for((B, Tp, Fp, C), SEED, p, salt)
    first = R.bn_block_bwd(d["y"], dout, d["scale"], d["shift"], d["mean"], d["rstd"], pf, pt, keep, d["N"], p)
    sums32 = (first["sum_g"].astype(np.float32), first["sum_gx"].astype(np.float32))
    ref = R.bn_block_bwd(d["y"], dout, d["scale"], d["shift"], d["mean"], d["rstd"], pf, pt, keep, d["N"], p, sums=sums32)
    y, sc, sh, mu, rs = (dev(d[k]) for k in ("y", "scale", "shift", "mean", "rstd"))
    dd = dev(dout.transpose(0, 1, 3, 2) if tcf else dout)
    rows, grid = B * Tp, L.sed_bn_bwd_rows(B, T, pt)
    assert grid == min(rows, 1024)
    per, nslots = -(-rows // grid), max(256 // (C // 4), 1)
    tag = f"{'x'.join(map(str, shape))} tcf={int(tcf)} p={p}"

    part = torch.full((grid, 2, C), float("nan")).cuda()
    check(L.sed_bn_relu_pool_drop_bwd_reduce(ptr(y), ptr(dd), ptr(sc), ptr(sh), ptr(mu), ptr(rs), ptr(part), B, T, F, C, pf, pt,
                                             int(tcf), p, SEED, ptr(state), stream_ptr()), "bn_bwd_reduce")
    sg, sgx = torch.empty(C).cuda(), torch.empty(C).cuda()
    check(L.sed_bn_bwd_finalize(ptr(part), grid, C, ptr(sg), ptr(sgx), None, None, stream_ptr()), "bn_bwd_finalize")
    Lr = per * -(-Fp // nslots)
    worst = hold(f"B sum_g {tag}", host(sg), first["sum_g"], bound(Lr + nslots + 3, first["mag_g"]))
    worst = max(worst, hold(f"B sum_gx {tag}", host(sgx), first["sum_gx"], bound(Lr + nslots + 6, first["mag_gx"])))

    dy = torch.full((B, T, F, C), float("nan")).cuda()
    dbp = torch.full((grid, C), float("nan")).cuda()
    sg_ref, sgx_ref = dev(sums32[0]), dev(sums32[1])
    check(L.sed_bn_relu_pool_drop_bwd_apply(ptr(y), ptr(dd), ptr(sc), ptr(sh), ptr(mu), ptr(rs), ptr(sg_ref), ptr(sgx_ref),
                                            ptr(dy), ptr(dbp), B, T, F, C, pf, pt, int(tcf), p, SEED, ptr(state), stream_ptr()), "bn_bwd_apply")
    worst = max(worst, hold(f"B dy {tag}", host(dy), ref["dy"], bound(8, ref["mag_dy"])))

    from sed_crnn_amd import ops as o
    La = per * (-(-Fp // nslots) * pf * pt + -(-(pt * (F - Fp * pf)) // nslots) + -(-((T - Tp * pt) * F) // nslots))
    worst = max(worst, hold(f"B sum_dy {tag}", host(o.reduce_rows(dbp)), ref["sum_dy"], bound(8 + La + nslots + 1, ref["mag_dy"].sum((0, 1, 2)))))
    return worst


def test_channels_last_forward_and_route_walk_past_8192_blocks(ops):
    """bn_relu_pool_drop_fwd_k / bn_relu_pool_route_k at 2 176 000 float4 against the 2 097 152 one grid stride covers: the
    last 78 848 are reached only by the `i += gridDim.x * 256` walk.  Output (mask from keep_mask) and route codes, all elements."""
    shape = R.B1_FWD_CL[0]
    assert shape[0] * shape[1] * shape[2] * shape[3] // 4 > 8192 * 256
    r = _forward(shape, R.block_inputs(shape), False, 0.5)
    print(f"[ratio] B1 forward past 8192 blocks: {r:.4f}")


@pytest.mark.parametrize("p", (0.0, 0.5))
def test_gru_order_forward_walks_past_4096_rows(ops, p):
    """bn_relu_pool_drop_fwd_tcf_k: 4350 (b, t') rows on 4096 blocks, T and F both ragged under the (2,2) pool"""
    shape = R.B2_FWD_TCF[0]
    assert shape[0] * (shape[1] // shape[5]) > 4096
    r = _forward(shape, R.block_inputs(shape), True, p, want_route=False)
    print(f"[ratio] B2 tcf forward past 4096 rows p={p}: {r:.4f}")


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("tcf", (False, True))
@pytest.mark.parametrize("shape", R.B3_BWD, ids=lambda s: "x".join(map(str, s)))
def test_backward_passes_walk_past_1024_rows(ops, shape, tcf, p):
    """both modes of bn_relu_pool_drop_bwd_k past BN_MAX_BLOCKS: 2565 rows on the P12 template (a block walks 2-3 rows, the ragged
    T tail belongs to one that walks others too) and 1200 rows on the generic template with both tails"""
    assert shape[0] * (shape[1] // shape[5]) > 1024
    r = _backward(shape, R.block_inputs(shape), tcf, p)
    print(f"[ratio] B3 backward past 1024 rows {shape} tcf={int(tcf)} p={p}: {r:.4f}")


@pytest.mark.parametrize("tcf", (False, True))
@pytest.mark.parametrize("shape", R.B4_CHANNELS, ids=lambda s: "x".join(map(str, s)))
def test_channel_counts_that_leave_threads_idle_or_one_slot(ops, shape, tcf):
    """C = 4 (256 slots), 12 and 100 (C/4 does not divide 256: idle threads), 516 and 1024 (one slot), forward and both backward
    modes, p = 0.3 (1 - p is not exact in fp32)"""
    d = R.block_inputs(shape)
    r = max(_forward(shape, d, tcf, 0.3), _backward(shape, d, tcf, 0.3))
    print(f"[ratio] B4 channel edges {shape} tcf={int(tcf)}: {r:.4f}")


@pytest.mark.parametrize("tcf", (False, True))
def test_device_step_state_salts_the_dropout_seed(ops, tcf):
    """forward, reduce and apply handed a device int64[2] {salt, step}: the mask is keep_mask of seed + salt * 0x9E3779B97F4A7C15
    mod 2^64 (a salt whose product overflows 64 bits), and not the unsalted one"""
    shape, p, salt = R.B5_SEED_DEV[0], 0.5, (1 << 62) + 12345
    d = R.block_inputs(shape)
    state = torch.tensor([salt, 77], dtype=torch.int64).cuda()
    r = max(_forward(shape, d, tcf, p, state, salt), _backward(shape, d, tcf, p, state, salt))
    assert not np.array_equal(R.keep_for((2, 4, 4, 12), SEED, p), R.keep_for((2, 4, 4, 12), SEED, p, salt))
    assert state.tolist() == [salt, 77]
    print(f"[ratio] B5 seed_dev tcf={int(tcf)}: {r:.4f}")


@pytest.mark.parametrize("shape", R.B6_POOLED, ids=lambda s: "x".join(map(str, s)))
def test_pooled_output_reduction_at_every_instantiation(ops, shape):
    """sed_bn_bwd_reduce_pooled<BPK, NT> for BPK 1..8 at 256 threads (C = 128 k - 4, F' = 8) and 3, 4 at 1024 (C = 1500, 2000), one
    case past the 1024-row cap; pooled and dout come from the reference (rounded to fp32), not from the device forward.  Every
    per-thread slot k holds a planted channel (small_passes_ref.pooled_special_channels), so the slow-channel search runs in each
    accumulator pair.  Against pooled_sums.
    k: a thread adds ceil(rows / grid) rows of 4 values each in fp32 and the channel sum adds F'/4 float4 columns; then
    sum g: fl(1 - p), its reciprocal, the product and the finaliser's cast, 4: k = ceil(rows / grid) 4 + F'/4 + 4;
    sum g xhat: xhat = fl(fl(q kr) + nb) with kr = fl(fl(1 - p) fl(1 / gamma)) 3, the product 1, nb = fl(-beta fl(1 / gamma)) 2,
    the sum 1 (at most 5 on either operand), fl(g xhat) 1, and the 4 above: k = ceil(rows / grid) 4 + F'/4 + 10, magnitude with
    |q (1 - p) / gamma| + |beta / gamma| (a slow channel's (|y| + |mean|) rstd takes fewer roundings).
    gamma == 0, beta < 0 channels must give exact zeros."""
    B, T, F, C, pf, pt = shape
    p, Tp, Fp = 0.3, T // pt, F // pf
    d = R.block_inputs(shape, True)
    keep = R.keep_for((B, Tp, Fp, C), SEED, p)
    pooled = R.bn_block_fwd(d["y"], d["scale"], d["shift"], pf, pt, keep, p)["out"].transpose(0, 1, 3, 2).astype(np.float32)
    dout = (np.random.default_rng(list(shape) + [9]).standard_normal(pooled.shape) * 0.1).astype(np.float32)
    ref = R.pooled_sums(pooled, dout, d["gamma"], d["beta"], d["y"], d["mean"], d["rstd"], d["scale"], d["shift"], pf, pt, p)
    n4 = C * Fp // 4
    nt = 256 if n4 <= 2048 else 1024
    kinds = R.pooled_special_channels(C)
    assert len(kinds) == -(-n4 // nt) and all((c * Fp // 4) // nt == j for j, (c, _) in enumerate(kinds))      # one per accumulator slot
    slow = R.slow_channels(d["gamma"], d["beta"])
    assert all(bool(slow[c]) == (kind != 1) for c, kind in kinds)
    sg, sgx = ops.bn_bwd_sums_from_pooled(dev(pooled), dev(dout), dev(d["gamma"]), dev(d["beta"]), dev(d["y"]), dev(d["mean"]), dev(d["rstd"]),
                                          pf, pt, drop_p=p, scale=dev(d["scale"]), shift=dev(d["shift"]))
    rows = B * Tp
    per = -(-rows // min(rows, 1024))
    r = max(hold(f"B6 sum_g {shape}", host(sg), ref["sum_g"], bound(per * 4 + Fp // 4 + 4, ref["mag_g"])),
            hold(f"B6 sum_gx {shape}", host(sgx), ref["sum_gx"], bound(per * 4 + Fp // 4 + 10, ref["mag_gx"])))
    for c, kind in kinds:
        if kind == 1:
            assert float(sg[c]) == 0.0 and float(sgx[c]) == 0.0 and ref["sum_g"][c] == 0.0
        else:
            assert ref["mag_gx"][c] > 0 and float(sgx[c]) != 0.0
    print(f"[ratio] B6 pooled reduction {shape}: {r:.4f}")


# ═════════════════════════ C. misc.hip ═════════════════════════
class V:
    """a float64 value with a first-order bound on the absolute error of its fp32 counterpart.  Every operation propagates
    the operands' errors through the exact derivative and adds ONE rounding (2^-24 of the result, and one denormal); the
    library functions add 4 ulp = 8 roundings instead."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    @staticmethod
    def rounded(v, e, k=1):
        return V(v, e + k * U * np.abs(v) + TINY)

    def __add__(self, o):
        o = V.of(o)
        return V.rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        return V.rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = V.of(o)
        return V.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = V.of(o)
        lo = np.abs(o.v) - o.e
        assert (lo > 0).all()
        q = self.v / o.v
        return V.rounded(q, self.e / lo + np.abs(q) * o.e / lo)

    def __neg__(self):
        return V(-self.v, self.e)

    def fn(self, f, slope):
        """a library function: |f'| <= slope over the operand's error interval, 4 ulp of the result"""
        return V.rounded(f(self.v), slope * self.e, 8)

    def where(self, mask, o):
        return V(np.where(mask, self.v, o.v), np.where(mask, self.e, o.e))


def _v_sigmoid(x):
    """1.f / (1.f + expf(-x)) with exact x: expf 4 ulp, the sum 1, the quotient 1"""
    e = V(-x).fn(np.exp, 0.0)
    return V(1.0) / (V(1.0) + e)


def _adam_bounds(p, g, m, v, lr, b1, b2, eps, wd, t, gs):
    """first-order bounds on one step of adam_k, one rounding per operation as the kernel writes them:
    gi = fl(fl(g gs) + fl(wd p));  m' = fl(fl(b1 m) + fl(fl(1 - b1) gi));  v' = fl(fl(b2 v) + fl(fl(fl(1 - b2) gi) gi));
    denom = fl(fl(sqrtf(v') / bc2s) + eps) with bc2s = fl(sqrt(bc2)) and sqrtf at 4 ulp, a root moving by at most
    min(sqrt(dv), dv / sqrt(v')) under an error dv of its operand;  p' = fl(p - fl(step fl(m' / denom))), step = fl(lr / fl(bc1)).
    -> (dp, dm, dv)"""
    gi = V(g) * gs + V(p) * wd
    m2 = V(m) * b1 + (V(1.0) - b1) * gi
    v2 = V(v) * b2 + (V(1.0) - b2) * gi * gi
    s = np.sqrt(v2.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s > 0, np.minimum(np.sqrt(v2.e), v2.e / s), np.sqrt(v2.e))
    root = V.rounded(s, ds, 8)
    bc1 = V.rounded(1.0 - b1 ** float(t), 0.0)
    bc2s = V.rounded(math.sqrt(1.0 - b2 ** float(t)), 0.0)
    p2 = V(p) - (V(lr) / bc1) * (m2 / (root / bc2s + eps))
    return p2.e * SLACK, m2.e * SLACK, v2.e * SLACK


ADAM_N = (1, 255, 257, 2 * 2 ** 20 + 4099)
ADAM_STEPS = [("host", 1), ("host", 2), ("host", 1000), ("device", 1), ("device", 1000), ("device", 10 ** 6)]


@pytest.mark.parametrize("mode,t0", ADAM_STEPS, ids=lambda a: str(a))
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_moves_p_m_and_v_as_float64_adam_does(ops, n, mode, t0):
    """adam_k over three consecutive steps from t0: the largest n walks 2 to 3 grid strides of its 4096 blocks; weight decay
    0 and 1e-4, with and without a device grad scale; bias corrections from the host step or, with the device step state
    {salt, step} (advanced by sed_step_advance between the steps), computed in the kernel.  Each step is held against one
    float64 step from the state the device held before it, p, m and v alike."""
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    f32 = lambda a: float(np.float32(a))                                # noqa: E731
    lr, b1, b2, eps = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8)
    worst = 0.0
    for wd, gs in ((0.0, None), (1e-4, 0.37), (1e-4, None), (0.0, 0.37)):
        rng = np.random.default_rng([n, t0, int(wd > 0), int(gs is not None)])
        p = dev(rng.standard_normal(n))
        m = dev(rng.standard_normal(n) * 0.1)
        v = dev(rng.random(n) * 0.01)
        gsd = None if gs is None else dev(np.array([gs]))
        state = torch.tensor([5, t0], dtype=torch.int64).cuda() if mode == "device" else None
        for k in range(3):
            g = rng.standard_normal(n).astype(np.float32)
            g[::97] = 0.0
            before = [host(a) for a in (p, m, v)]
            ops.adam_step(p, dev(g), m, v, lr, b1, b2, eps, f32(wd), 0 if state is not None else t0 + k, gsd, state)
            args = (before[0], g.astype(np.float64), before[1], before[2], lr, b1, b2, eps, f32(wd), t0 + k, f32(1.0 if gs is None else gs))
            want = R.adam_step(*args)
            bnds = _adam_bounds(*args)
            for name, got, w, b in sorted(zip("pmv", (p, m, v), want, bnds), key=lambda e: "mvp".index(e[0])):   # the state first
                worst = max(worst, hold(f"C1 {name} n={n} {mode} t={t0 + k} wd={wd} gs={gs}", host(got), w, b + TINY))
            if state is not None:
                check(lib().sed_step_advance(ptr(state), stream_ptr()), "step_advance")
        if state is not None:
            assert state.tolist() == [8, t0 + 3]
    print(f"[ratio] C1 adam n={n} {mode} t0={t0}: {worst:.4f}")


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 1023, 10007, 3 * 524288 + 3))
def test_grad_norm_and_clip_coefficient_with_the_scalar_tail(ops, n):
    """sqnorm_partial_k on an unpadded, 16-byte aligned gradient: n % 4 elements go through its scalar tail, the largest n walks
    3 strides of its 512 blocks.  A float4's squares are paired in fp32 (a product and a sum: 2 roundings relative to the pair),
    everything else is double: the squared norm is within 2 * 2^-24, the root halves that, the cast adds 1: k = 2 on the norm.
    coef = fl(max_norm / fl(norm + 1e-6)) adds 2: k = 4; exactly 1 without a limit and with one above the norm."""
    rng = np.random.default_rng(n)
    g = (rng.standard_normal(n) * 0.7).astype(np.float32)
    gd = dev(g)
    assert gd.data_ptr() % 16 == 0 and gd.numel() == n
    nrm = R.norm_and_clip(g, 0.0)[0]
    worst = 0.0
    for which, mx in (("none", 0.0), ("below", float(np.float32(0.5 * nrm))), ("above", float(np.float32(2.0 * nrm)))):
        out = host(ops.grad_norm_clip_coef(gd, mx))
        want = R.norm_and_clip(g, mx)
        worst = max(worst, hold(f"C2 norm n={n} {which}", out[0], want[0], bound(2, want[0]) + n * D * want[0]),
                    hold(f"C2 coef n={n} {which}", out[1], want[1], bound(4, want[1])))
        if which != "below":
            assert out[1] == 1.0
        else:
            assert 0.49 < out[1] < 0.51
    print(f"[ratio] C2 norm and clip n={n}: {worst:.4f}")


def _loss_bounds(x, t, kind, alpha, gamma, mean):
    """loss_fwd_bwd_k restated operation by operation in the error arithmetic of V -> (V loss terms, V dx, V probs, V scale)"""
    n = x.size
    scale = V.rounded(1.0 / n, 0.0) if mean else V(1.0)
    p = _v_sigmoid(x)
    if kind == "bce":
        e = V(-np.abs(x)).fn(np.exp, 0.0)
        l = (V(np.maximum(x, 0.0)) - V(x) * t) + e.fn(np.log1p, 1.0)          # |log1p'| <= 1 on e >= 0
        d = p - t
    else:
        pos = t == 1.0
        pt = p.where(pos, V(1.0) - p)
        om = V(1.0) - pt
        arg = pt + float(np.float32(1e-12))
        lg = arg.fn(np.log, 1.0 / (arg.v - arg.e))

        def power(b, ex):                                  # powf(b, ex), ex = 0 (exactly 1) or ex >= 1 (slope largest at b + e)
            return V(np.ones_like(b.v)) if ex == 0 else b.fn(lambda a: a ** ex, ex * (b.v + b.e) ** (ex - 1.0))

        pw = power(om, gamma)
        l = (V(-alpha) * pw) * lg
        dpw = V(gamma) * power(om, gamma - 1.0)
        dl = V(-alpha) * ((-dpw) * lg + pw / arg)
        pq = p * (V(1.0) - p)
        d = dl * pq.where(pos, -pq)
    return l, d * scale, p, scale


def _focal_x(rng, n):
    x = np.clip(rng.standard_normal(n) * 3, -8, 8).astype(np.float32)
    sp = np.array([0.0, 8.0, -8.0, 7.5, -7.5, 1e-3], np.float32)
    x[:min(n, sp.size)] = sp[:n]
    return x


@pytest.mark.parametrize("n", (1, 63, 1023, 1024, 1025, 5000, 20011))
def test_losses_gradients_and_probabilities(ops, n):
    """loss_fwd_bwd_k, one block that walks n / 1024 elements per thread: BCE-with-logits with logits out to +-100 and exact zeros,
    mean and sum; the focal loss for gamma 1, 2, 3, alpha 0.25 and 1, mean and sum, logits within +-8 (outside, 1 - p saturates
    in fp32 as it does in the fp32 model this loss restates, which a float64 reference does not reproduce; gamma < 1 is not
    run).  Loss, dlogits and probabilities against float64, with the roundings of every operation carried by V; the loss is
    a double sum: the elements' bounds add up, then scale's rounding and the cast.  One call per n passes null dlogits / probs."""
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    rng = np.random.default_rng(n)
    xb = (rng.standard_normal(n) * 4).astype(np.float32)
    sp = np.array([-100.0, 0.0, 100.0, 88.0, -88.0, -0.0, 50.0, -89.5, 30.0, -30.0], np.float32)
    xb[:min(n, sp.size)] = sp[:n]
    if n > 20:
        xb[n - 1], xb[n // 2] = 100.0, 0.0
    tb = np.where(rng.random(n) < 0.5, (rng.random(n) < 0.4).astype(np.float32), rng.random(n).astype(np.float32)).astype(np.float32)
    xf, tf = _focal_x(rng, n), (rng.random(n) < 0.4).astype(np.float32)
    cases = [("bce", xb, tb, 0.25, 2.0, mean) for mean in (True, False)]
    cases += [("focal", xf, tf, a, gm, mean) for gm in (1.0, 2.0, 3.0) for a in (0.25, 1.0) for mean in (True, False)]
    worst = 0.0
    for kind, x, t, alpha, gamma, mean in cases:
        loss, dx, pr = ops.loss_fwd_bwd(dev(x), dev(t), kind, alpha, gamma, "mean" if mean else "sum")
        x64, t64, a32 = x.astype(np.float64), t.astype(np.float64), float(np.float32(alpha))
        want = R.bce_with_logits(x64, t64, mean) if kind == "bce" else R.focal_loss(x64, t64, alpha, gamma, mean)
        l, d, p, scale = _loss_bounds(x64, t64, kind, a32, gamma, mean)
        lb = (l.e.sum() * scale.v + np.abs(l.v).sum() * (scale.e + (n + 2) * D * scale.v) + U * abs(want[0])) * SLACK + TINY
        tag = f"n={n} {kind} a={alpha} g={gamma} mean={mean}"
        worst = max(worst, hold(f"C3 loss {tag}", host(loss)[0], want[0], lb), hold(f"C3 dx {tag}", host(dx), want[1], d.e * SLACK),
                    hold(f"C3 probs {tag}", host(pr), want[2], p.e * SLACK))
    kind, x, t, alpha, gamma, mean = cases[3]
    loss, xd, td = torch.empty(1).cuda(), dev(x), dev(t)
    check(lib().sed_loss_fwd_bwd(ptr(xd), ptr(td), n, 1, alpha, gamma, int(mean), ptr(loss), None, None, stream_ptr()), "loss_fwd_bwd")
    assert float(loss) == float(ops.loss_fwd_bwd(dev(x), dev(t), kind, alpha, gamma, "sum")[0])
    print(f"[ratio] C3 losses n={n}: {worst:.4f}")


@pytest.mark.parametrize("n", (1, 255, 256, 257, 70001))
def test_sigmoid_and_scale(ops, n):
    """sed_sigmoid (expf 4 ulp, a sum, a quotient: V) and sed_scale (x *= alpha in place: 1 rounding), one thread per element,
    at sizes around the 256-thread workgroup"""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 6).astype(np.float32)
    sp = np.array([0.0, 100.0, -100.0, 88.0, -88.0, -89.5], np.float32)
    x[:min(n, sp.size)] = sp[:n]
    p = _v_sigmoid(x.astype(np.float64))
    r1 = hold(f"C4 sigmoid n={n}", host(ops.sigmoid(dev(x))), R.sigmoid(x), p.e * SLACK)
    alpha = float(np.float32(0.37))
    xd = dev(x)
    guard = torch.cat([xd, torch.full((3,), 7.0).cuda()])                       # the elements after n stay as they are
    ops.scale_(guard[:n], alpha)
    r2 = hold(f"C4 scale n={n}", host(guard[:n]), x.astype(np.float64) * alpha, bound(1, np.abs(x.astype(np.float64) * alpha)))
    assert guard[n:].tolist() == [7.0, 7.0, 7.0]
    print(f"[ratio] C4 sigmoid and scale n={n}: {max(r1, r2):.4f}")
