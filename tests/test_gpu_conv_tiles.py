"""conv3x3_mfma_fwd2_k (csrc/conv.hip) on every block tile its plan can pick, with the XCD-aware workgroup order off and on,
through all five of its jobs: forward with statistics, plain data gradient, data gradient + BatchNorm-backward sums (BNR),
+ the first block's tap sums (RG), inference with folded BatchNorm, ReLU and time pool (EV).

The rows come from conv_cases.py (test_cpu_conv_plan.py proves that each is on the tile it claims).  Every reference is torch in
float64 on the CPU and shares nothing with the library.
  * integers (x in [-3, 3], w in {-1, 0, 1}, integer bias): |y| <= 9 * Cin * 3 + 3 < 2^24, every summation order is exact, so y,
    dx and every statistic partial row must EQUAL the float64 value; outputs start as NaN (a tile never visited shows) between
    guard regions that must stay untouched; a batch of 8 (order on) must give sequence by sequence what a batch of 3 (off) gives;
  * N(0,1) data at the tolerance test_conv3x3_fwd_stats_dgrad_wgrad holds this kernel to (atol 2e-5, rtol 1e-4);
  * the epilogues at the bounds the project already holds them to (2e-6 / 6e-6 * mag for the BatchNorm sums, 2e-5 * max|dW|)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc  # noqa: E402
from conv_ref import _bn_sums_ref, _dx_ref, _first_block_grads_ref, _fp32_formula_error  # noqa: E402

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0D1CE          # a quiet NaN with a payload: what every output and guard element starts as
GUARD = 4096                   # elements in front of and behind every output
CIN = cc.CV_CIC
BS = (cc.B_PLAIN, cc.B_XCD)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def g(t):
    return t.cuda().contiguous()


def cl(t):
    """[B,C,F,T] -> channels-last [B,T,F,C]"""
    return t.permute(0, 3, 2, 1).contiguous()


def _guarded(*shape):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(torch.float32).view(*shape)


def _assert_guards(buf, what):
    assert bool((buf[:GUARD] == NAN_BITS).all()), f"{what}: written in front of the buffer"
    assert bool((buf[-GUARD:] == NAN_BITS).all()), f"{what}: written behind the buffer"


def _run_conv(L, x, wp, bias, Cout, want_stats, what):
    """sed_conv3x3_fwd_ex on channels-last x into NaN-filled, guarded y (and statistic rows) -> (y, stat) on the CPU"""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    B, T, Fm, Cin = x.shape
    ybuf, y = _guarded(B, T, Fm, Cout)
    rows = L.sed_conv3x3_stat_rows(B, Cin, Fm, T, Cout, 0)
    sbuf, stat = _guarded(rows, 2, Cout) if want_stats else (None, None)
    check(L.sed_conv3x3_fwd_ex(ptr(x), 0, ptr(wp), ptr(bias), ptr(y), ptr(stat), B, Cin, Fm, T, Cout, 0, stream_ptr()), what)
    torch.cuda.synchronize()
    _assert_guards(ybuf, what + " y")
    if want_stats:
        _assert_guards(sbuf, what + " stat")
    return y.cpu(), (stat.cpu() if want_stats else None)


def _differing_tiles(got, ref, plan):
    """(b, time block, mel tile) of every block tile with an element that is not the reference's"""
    B, T, Fm, _ = ref.shape
    bad = (got.double() != ref).any(-1)
    out = []
    for tb in range(plan["tblocks"]):
        for fi in range(plan["nft"]):
            ts, fs = cc.tile_slices(plan, Fm, T, tb, fi)
            out += [(b, tb, fi) for b in range(B) if bool(bad[b, ts, fs].any())]
    return sorted(out)


def _assert_equal(got, ref, plan, what):
    if not torch.equal(got.double(), ref):
        tiles = _differing_tiles(got, ref, plan)
        nan = int(torch.isnan(got).sum())
        raise AssertionError(f"{what}: {int((got.double() != ref).sum())} of {ref.numel()} elements differ ({nan} still NaN) in {len(tiles)} tiles "
                             f"(sequence, time block, mel tile): {tiles[:24]}; tile {plan['TT']}x{plan['FT']}, nft {plan['nft']}, tblocks {plan['tblocks']}")


def _stat_rows_ref(yref, plan):
    """[rows][2][Cout] in float64: (sum y, sum y^2) of each tile's own positions, in the row the tile writes; + the largest
    sum |y| and sum y^2 of any tile and channel (the exactness precondition)"""
    B, T, Fm, Cout = yref.shape
    out = torch.full((B * plan["tblocks"] * plan["nft"], 2, Cout), float("nan"), dtype=torch.float64)
    big = 0.0
    bs = torch.arange(B)
    for tb in range(plan["tblocks"]):
        for fi in range(plan["nft"]):
            ts, fs = cc.tile_slices(plan, Fm, T, tb, fi)
            v = yref[:, ts, fs]
            r = torch.tensor([cc.stat_row(plan, int(b), tb, fi) for b in bs])
            out[r, 0], out[r, 1] = v.sum((1, 2)), (v * v).sum((1, 2))
            big = max(big, float(v.abs().sum((1, 2)).max()), float((v * v).sum((1, 2)).max()))
    assert not bool(torch.isnan(out).any())
    return out, big


# ───────────────────────── a, b: integers, exact ─────────────────────────
INT_ROWS = [r["name"] for r in cc.rows(which=0)]


@pytest.mark.parametrize("name", INT_ROWS)
def test_forward_statistic_rows_and_data_gradient_are_exact_on_integers(ops, name):
    L = ops.lib()
    r = cc.row(name)
    Fm, T, Cout = r["F"], r["T"], cc.COUT_OF_NCT[r["nct"]]
    gen = torch.Generator().manual_seed(1000 * Fm + T + Cout)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).float()
    B8 = cc.B_XCD
    x, w, bias = ri(-3, 3, B8, CIN, Fm, T), ri(-1, 1, Cout, CIN, 3, 3), ri(-3, 3, Cout)
    yref = cl(F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    assert float(yref.abs().max()) <= 9 * CIN * 3 + 3
    # the data gradient on the same tile: the kernel's output width is the gradient's channel count, so the layer is Cout -> CIN
    wg, dy = ri(-1, 1, CIN, Cout, 3, 3), ri(-3, 3, B8, T, Fm, CIN)
    dxref = _dx_ref(dy, wg)
    wf, _ = ops.conv3x3_pack(g(w))
    _, wd = ops.conv3x3_pack(g(wg))
    xg, bg, dyg = g(cl(x)), g(bias), g(dy)
    ys = {}
    for B in BS:
        plan = ops.conv3x3_plan(B, CIN, Fm, T, Cout)
        assert (plan["TT"], plan["FT"]) == r["tile"] and plan["xcd_order"] == int(B % 8 == 0)
        y, stat = _run_conv(L, xg[:B].contiguous(), wf, bg, Cout, True, f"{name} forward B={B}")
        ys[B] = y
        _assert_equal(y, yref[:B], plan, f"{name} forward, B = {B}")
        sref, big = _stat_rows_ref(yref[:B], plan)
        assert big < 2 ** 24, "the sums of a tile leave the range in which float32 adds integers exactly"
        if not torch.equal(stat.double(), sref):
            rows = sorted(set(torch.nonzero((stat.double() != sref).any(-1).any(-1)).flatten().tolist()))
            raise AssertionError(f"{name} B = {B}: statistic rows {rows[:32]} of {sref.shape[0]} are not their own tile's sums "
                                 f"(row = (b * {plan['tblocks']} + tb) * {plan['nft']} + fi)")
        dx, _ = _run_conv(L, dyg[:B].contiguous(), wd, None, Cout, False, f"{name} dgrad B={B}")
        _assert_equal(dx, dxref[:B], plan, f"{name} data gradient, B = {B}")
    assert torch.equal(ys[cc.B_XCD][:cc.B_PLAIN], ys[cc.B_PLAIN]), "a sequence's output depends on the workgroup order"


def test_batch_of_16_walks_two_rounds_of_sequences_per_xcd(ops):
    """B = 16: launch index xcd + 8 j reaches sequence xcd + 8 (j / tiles) with j / tiles = 1 as well (B = 8 only ever has 0)"""
    L = ops.lib()
    r = cc.find(4, 0, (5, 32), "grid")
    Fm, T, Cout, B = r["F"], r["T"], 128, 16
    gen = torch.Generator().manual_seed(16)
    x = torch.randint(-3, 4, (B, CIN, Fm, T), generator=gen).float()
    w = torch.randint(-1, 2, (Cout, CIN, 3, 3), generator=gen).float()
    yref = cl(F.conv2d(x.double(), w.double(), None, padding=1))
    plan = ops.conv3x3_plan(B, CIN, Fm, T, Cout)
    assert plan["xcd_order"] == 1 and plan["nft"] * plan["tblocks"] == 4 and B * T * Fm * Cout <= cc.MAX_OUT_ELEMS
    wf, _ = ops.conv3x3_pack(g(w))
    y, stat = _run_conv(L, g(cl(x)), wf, None, Cout, True, "B=16")
    _assert_equal(y, yref, plan, "forward, B = 16")
    assert torch.equal(stat.double(), _stat_rows_ref(yref, plan)[0])


# ───────────────────────── c: real values ─────────────────────────
REAL_ROWS = ([cc.find(4, 0, t, "grid")["name"] for t in ((5, 32), (1, 82), (35, 4), (2, 62), (8, 20), (20, 8))] +
             [cc.find(4, 0, t, "interior")["name"] for t in ((4, 40), (16, 10), (10, 16))] +
             [cc.find(4, 0, t)["name"] for t in ((6, 26), (3, 44), (2, 50))] +
             [r["name"] for nct in (2, 1) for r in cc.rows(nct, 0, "grid")] + [cc.find(nct, 0, (20, 8))["name"] for nct in (2, 1)])


@pytest.mark.parametrize("name", REAL_ROWS)
def test_forward_statistics_and_data_gradient_on_real_values(ops, name):
    """N(0,1) inputs, 128 input channels (the K = 1152 sums of the network) against float64 at atol 2e-5, rtol 1e-4; the summed
    statistic rows at the existing rtol 1e-4, atol 2e-3"""
    L = ops.lib()
    r = cc.row(name)
    assert cc.halo_edge((2, 62)) and cc.halo_edge((6, 30)) and cc.halo_edge((14, 14))
    Fm, T, Cout, Ci = r["F"], r["T"], cc.COUT_OF_NCT[r["nct"]], 128
    gen = torch.Generator().manual_seed(7000 + 10 * Fm + T + Cout)
    B8 = cc.B_XCD
    x = torch.randn(B8, Ci, Fm, T, generator=gen)
    w = torch.randn(Cout, Ci, 3, 3, generator=gen) / np.sqrt(9 * Ci)
    bias = torch.randn(Cout, generator=gen)
    wg = torch.randn(Ci, Cout, 3, 3, generator=gen) / np.sqrt(9 * Ci)
    dy = torch.randn(B8, T, Fm, Ci, generator=gen)
    yref = cl(F.conv2d(x.double(), w.double(), bias.double(), padding=1))
    dxref = _dx_ref(dy, wg)
    wf, _ = ops.conv3x3_pack(g(w))
    _, wd = ops.conv3x3_pack(g(wg))
    xg, bg, dyg = g(cl(x)), g(bias), g(dy)
    for B in BS:
        plan = ops.conv3x3_plan(B, Ci, Fm, T, Cout)
        assert (plan["TT"], plan["FT"]) == r["tile"]
        y, stat = _run_conv(L, xg[:B].contiguous(), wf, bg, Cout, True, f"{name} forward B={B}")
        dx, _ = _run_conv(L, dyg[:B].contiguous(), wd, None, Cout, False, f"{name} dgrad B={B}")
        s, yr = stat.double().sum(0), yref[:B]
        e = [float((y.double() - yr).abs().max()), float((dx.double() - dxref[:B]).abs().max()),
             float((s[0] - yr.sum((0, 1, 2))).abs().max()), float((s[1] - (yr * yr).sum((0, 1, 2))).abs().max())]
        print(f"{name} B={B}: max |y - ref| {e[0]:.2e}, max |dx - ref| {e[1]:.2e} (atol 2e-5 + 1e-4 |ref|); sum y {e[2]:.2e}, sum y^2 {e[3]:.2e} (atol 2e-3 + 1e-4 |ref|)")
        np.testing.assert_allclose(y.double().numpy(), yr.numpy(), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(dx.double().numpy(), dxref[:B].numpy(), atol=2e-5, rtol=1e-4)
        np.testing.assert_allclose(s[0].numpy(), yr.sum((0, 1, 2)).numpy(), rtol=1e-4, atol=2e-3)
        np.testing.assert_allclose(s[1].numpy(), (yr * yr).sum((0, 1, 2)).numpy(), rtol=1e-4, atol=2e-3)


# ───────────────────────── d: the BatchNorm-backward epilogue ─────────────────────────
C = 128


@functools.lru_cache(maxsize=None)
def _bnr_data(Fm, T):
    """dy, w and the float64 data gradient of the largest batch, shared by every pool / dropout / batch variant of a shape"""
    gen = torch.Generator().manual_seed(500 + 10 * Fm + T)
    dy = torch.randn(cc.B_XCD, T, Fm, C, generator=gen) * 0.1
    w = torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    return dy, w, _dx_ref(dy, w)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("pf,pt", [(1, 2), (2, 1)])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("Fm,T,tile,rf,rt", cc.BNR_SHAPES)
def test_dgrad_bn_backward_sums_vs_float64(ops, Fm, T, tile, rf, rt, B, pf, pt, p):
    """sed_conv3x3_dgrad_bnred: dx against conv2d_input, the partial rows summed in float64 against sum g and sum g*xhat formed in
    float64 from the float64 dx and the forward's pooled output.  gamma == 0 of both beta signs, a negative gamma and
    |gamma| * 64 < |beta| (zero in sum g*xhat by specification: the finalising kernel finishes them from the conv output) as in
    test_dgrad_with_fused_bn_backward_reduction_matches_the_two_pass_form."""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    L = ops.lib()
    plan = ops.conv3x3_plan(B, C, Fm, T, C)
    assert (plan["TT"], plan["FT"]) == tile and (plan["nft"] * plan["FT"] > Fm, T % plan["TT"] != 0) == (rf, rt) and plan["xcd_order"] == int(B == 8)
    dy8, w, dref8 = _bnr_data(Fm, T)
    dy, dref = dy8[:B], dref8[:B]
    Ty, Fy = T * pt, Fm * pf
    gen = torch.Generator().manual_seed(B * 100 + Ty + Fy)
    yb = torch.randn(B, Ty, Fy, C, generator=gen).cuda()
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[3], beta[3] = 0.0, 0.5
    gamma[77], beta[77] = 0.0, -0.2
    gamma[100] = -0.7
    gamma[8], beta[8] = 1e-3, 0.5
    gamma[9], beta[9] = -1e-5, 0.4
    gamma[10], beta[10] = 1e-5, 0.6
    gamma[11], beta[11] = 0.02, 0.9
    gamma, beta = gamma.cuda(), beta.cuda()
    flat = yb.reshape(-1, C)
    part0 = torch.stack([flat.sum(0), (flat ** 2).sum(0)]).reshape(1, 2, C).contiguous()
    mean, rstd, scale, shift = ops.bn_finalize_train(part0, B * Ty * Fy, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda())
    pooled = ops.bn_relu_pool_drop_fwd(yb, scale, shift, pf, pt, drop_p=p, seed=99)
    assert pooled.shape == (B, T, Fm, C)
    _, wd = ops.conv3x3_pack(g(w))
    rows = L.sed_conv3x3_dgrad_bnred_rows(B, C, Fm, T, C)
    assert rows == plan["rows"]
    dbuf, dx = _guarded(B, T, Fm, C)
    pbuf, part = _guarded(rows, 2, C)
    dyg = g(dy)
    check(L.sed_conv3x3_dgrad_bnred(ptr(dyg), ptr(wd), ptr(dx), ptr(part), ptr(pooled), ptr(gamma), ptr(beta), ptr(yb), ptr(mean), ptr(rstd),
                                    p, pf, pt, Fy, Ty, B, C, Fm, T, C, stream_ptr()), "dgrad_bnred")
    torch.cuda.synchronize()
    _assert_guards(dbuf, "dx")
    _assert_guards(pbuf, "partial rows")
    keep = 1.0 - p
    _, sg_ref, sgx_ref, zero = _bn_sums_ref(dref, pooled, gamma, beta, keep, True)
    mag = float((dref.abs() / keep).sum(dim=(0, 1, 2)).max())
    e1, e2 = _fp32_formula_error(dref, pooled, gamma, beta, keep, zero, sg_ref, sgx_ref)
    print(f"float32 formula on these inputs: sum g {e1:.2e} of {2e-6 * mag:.2e}, sum g*xhat {e2:.2e} of {6e-6 * mag:.2e}")
    assert e1 < 2e-6 * mag and e2 < 6e-6 * mag
    np.testing.assert_allclose(dx.cpu().double().numpy(), dref.numpy(), atol=2e-5, rtol=1e-4)
    assert bool(torch.isfinite(part).all()), "a partial row was never written"
    s = part.double().sum(0).cpu()
    k1, k2 = float((s[0] - sg_ref).abs().max()), float((s[1] - sgx_ref).abs().max())
    print(f"kernel: max |dx - ref| {float((dx.cpu().double() - dref).abs().max()):.2e}; sum g {k1:.2e} = {k1 / mag:.1e} mag, sum g*xhat {k2:.2e} = {k2 / mag:.1e} mag")
    np.testing.assert_allclose(s[0].numpy(), sg_ref.numpy(), atol=2e-6 * mag, rtol=1e-4)
    np.testing.assert_allclose(s[1].numpy(), sgx_ref.numpy(), atol=6e-6 * mag, rtol=1e-4)
    assert set(torch.nonzero(zero).flatten().tolist()) == {3, 77, 8, 9, 10} and bool((s[1][zero] == 0).all())
    assert float(s[0][77].abs()) == 0.0                        # gamma 0, beta < 0: the gate is shut everywhere
    # each partial row holds its own tile's sum g (the rows are not merely right in total)
    gg = torch.where(pooled.cpu() > 0, dref / keep, torch.zeros_like(dref))
    rref, _ = _stat_rows_ref(gg, plan)
    assert float((part.cpu().double()[:, 0] - rref[:, 0]).abs().max()) <= 2e-6 * mag
    # the entry the network-level wrapper uses: the same dx bit for bit, every channel's sum g
    dx2, sum_g, _ = ops.conv3x3_dgrad_bnred(dyg, wd, pooled, gamma, beta, yb, mean, rstd, pf, pt, drop_p=p, scale=scale, shift=shift)
    assert torch.equal(dx2, dx)
    np.testing.assert_allclose(sum_g.cpu().double().numpy(), sg_ref.numpy(), atol=2e-6 * mag, rtol=1e-4)


# ───────────────────────── e: the pooled inference epilogue and the tap-sum epilogue ─────────────────────────
@pytest.mark.parametrize("name", [r["name"] for r in cc.rows(4, 1)])
def test_inference_epilogue_on_every_pooled_tile_vs_float64(ops, name):
    """sed_conv3x3_bn_relu_pool_eval against max_pool2d(relu(batch_norm(conv2d))) in float64 at the tolerance of
    test_inference_conv_with_folded_batchnorm_relu_and_pool_in_the_epilogue; negative and zero gamma; the rows' odd T drop a frame"""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    L = ops.lib()
    r = cc.row(name)
    Fm, T, Cout = r["F"], r["T"], 128
    gen = torch.Generator().manual_seed(3000 + 10 * Fm + T)
    x = torch.randn(cc.B_XCD, CIN, Fm, T, generator=gen)
    w = torch.randn(Cout, CIN, 3, 3, generator=gen) / (3.0 * CIN ** 0.5)
    bias, beta, rm = (torch.randn(Cout, generator=gen) * 0.3 for _ in range(3))
    gamma = torch.rand(Cout, generator=gen) + 0.5
    gamma[1], gamma[5] = -0.8, 0.0
    rv = torch.rand(Cout, generator=gen) + 0.5
    ref = cl(F.max_pool2d(torch.relu(F.batch_norm(F.conv2d(x.double(), w.double(), bias.double(), padding=1), rm.double(), rv.double(),
                                                  gamma.double(), beta.double(), training=False, eps=1e-5)), (1, 2)))
    wf, bf = torch.empty(9, Cout, CIN).cuda(), torch.empty(Cout).cuda()
    args = [g(t) for t in (w, bias, gamma, beta, rm, rv)]
    check(L.sed_conv3x3_pack_weights_bn_folded(*[ptr(t) for t in args], 1e-5, ptr(wf), ptr(bf), Cout, CIN, stream_ptr()), "pack")
    xg = g(cl(x))
    outs = {}
    for B in BS:
        plan = ops.conv3x3_plan(B, CIN, Fm, T, Cout, False, 1)
        assert (plan["TT"], plan["FT"]) == r["tile"] and L.sed_conv3x3_bn_relu_pool_eval_supported(B, CIN, Fm, T, Cout)
        obuf, out = _guarded(B, T // 2, Fm, Cout)
        xb = xg[:B].contiguous()
        check(L.sed_conv3x3_bn_relu_pool_eval(ptr(xb), ptr(wf), ptr(bf), ptr(out), B, CIN, Fm, T, Cout, stream_ptr()), "eval")
        torch.cuda.synchronize()
        _assert_guards(obuf, f"{name} B={B}")
        outs[B] = out.cpu()
        print(f"{name} B={B}: max |out - ref| {float((outs[B].double() - ref[:B]).abs().max()):.2e}")
        np.testing.assert_allclose(outs[B].double().numpy(), ref[:B].numpy(), atol=2e-5 * max(1.0, float(ref.abs().max())), rtol=1e-5)
    assert torch.equal(outs[cc.B_XCD][:cc.B_PLAIN], outs[cc.B_PLAIN]), "a sequence's output depends on the workgroup order"


RG_ROWS = cc.rg_rows()


@pytest.mark.parametrize("name", [r["name"] for r in RG_ROWS])
def test_tap_sum_epilogue_on_the_pooled_table_vs_float64(ops, name):
    """sed_conv3x3_dgrad_bnred_rg behind the real first-block forward (its pooled output and arg-max bits), one and two input
    channels, batches of 3 and 8: dx, sum g, sum g*xhat and — after sed_bn_bwd_finalize + sed_conv1_bwd_wgrad_assemble — dW, dgamma
    and dbias of the first block against the float64 chain of test_winograd_dgrad_tap_sums_without_dx_and_vs_float64."""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    L = ops.lib()
    r = cc.row(name)
    Fm, Tp = r["F"], r["T"]
    T = 2 * Tp
    gen = torch.Generator().manual_seed(9000 + 10 * Fm + Tp)
    x2 = torch.randn(cc.B_XCD, 2, Fm, T, generator=gen)
    w12 = torch.randn(C, 2, 3, 3, generator=gen) * 0.4
    b1 = torch.randn(C, generator=gen) * 0.1
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[5], beta[5] = 0.0, 0.4
    gamma[9], beta[9] = 0.0, -0.3
    gamma[64] = -0.8
    gamma[33], beta[33] = 1e-3, 2e-3
    w2 = torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    dy8 = torch.randn(cc.B_XCD, Tp, Fm, C, generator=gen) * 0.1
    dref8 = _dx_ref(dy8, w2)
    _, wd2 = ops.conv3x3_pack(g(w2))
    b1g, gg, bg = g(b1), g(gamma), g(beta)
    seed = 11
    for B, cin, p in [(cc.B_PLAIN, 1, 0.5), (cc.B_XCD, 1, 0.0), (cc.B_PLAIN, 2, 0.0), (cc.B_XCD, 2, 0.3)]:
        rows = L.sed_conv3x3_dgrad_bnred_rg_rows(B, C, Fm, Tp, C, cin)
        assert rows > 0 and rows == ops.conv3x3_plan(B, C, Fm, Tp, C)["rows"], "the listed shape does not take the fused path"
        x, w1, dy, dref = x2[:B, :cin].contiguous(), w12[:, :cin].contiguous(), dy8[:B], dref8[:B]
        # forward of the first block (statistics from the input moments, arg-max bits)
        wf1, _ = ops.conv3x3_pack(g(w1))
        stat = torch.empty(1, 2, C).cuda()
        sws = torch.empty(L.sed_conv1_stats_workspace_bytes(B, cin, T) // 4 + 1).cuda()
        mom = torch.empty(L.sed_conv1_moments_doubles(cin), dtype=torch.float64).cuda()
        xg = g(x)
        check(L.sed_conv1_stats(ptr(xg), ptr(wf1), ptr(b1g), ptr(stat), ptr(sws), B, cin, Fm, T, C, ptr(mom), stream_ptr()), "conv1_stats")
        mean, rstd, scale, shift = ops.bn_finalize_train(stat, B * T * Fm, gg, bg, torch.zeros(C).cuda(), torch.ones(C).cuda())
        pooled = torch.empty(B, Tp, Fm, C).cuda()
        bits = torch.empty(pooled.numel() // 4, dtype=torch.uint8).cuda()
        check(L.sed_conv1_bn_relu_pool_drop_fwd(ptr(xg), ptr(wf1), ptr(b1g), ptr(scale), ptr(shift), ptr(pooled), B, cin, Fm, T, C, 1, 2, p, seed,
                                                None, ptr(bits), stream_ptr()), "conv1_fwd")
        dbuf, dx = _guarded(B, Tp, Fm, C)
        pbuf, part = _guarded(rows, 2, C)
        rbuf, rgp = _guarded(rows, C, 1 + 9 * cin)
        dyg = g(dy)
        check(L.sed_conv3x3_dgrad_bnred_rg(ptr(dyg), ptr(wd2), ptr(dx), ptr(part), ptr(pooled), ptr(gg), ptr(bg), ptr(mean), ptr(rstd), p,
                                           ptr(xg), cin, ptr(bits), ptr(rgp), B, C, Fm, Tp, C, stream_ptr()), "dgrad_bnred_rg")
        torch.cuda.synchronize()
        for buf, what in ((dbuf, "dx"), (pbuf, "partial rows"), (rbuf, "tap-sum rows")):
            _assert_guards(buf, what)
        assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(rgp).all())
        keep = 1.0 - p
        gref, sg_ref, sgx_ref, zero = _bn_sums_ref(dref, pooled, gg, bg, keep, False)
        mag = float((dref.abs() / keep).sum(dim=(0, 1, 2)).max())
        e1, e2 = _fp32_formula_error(dref, pooled, gg, bg, keep, zero, sg_ref, sgx_ref)
        assert e1 < 2e-6 * mag and e2 < 6e-6 * mag, (e1, e2, mag)
        np.testing.assert_allclose(dx.cpu().double().numpy(), dref.numpy(), atol=2e-5, rtol=1e-4)
        s = part.double().sum(0).cpu()
        np.testing.assert_allclose(s[0].numpy(), sg_ref.numpy(), atol=2e-6 * mag, rtol=1e-4)
        np.testing.assert_allclose(s[1].numpy(), sgx_ref.numpy(), atol=6e-6 * mag, rtol=1e-4)
        np.testing.assert_allclose(rgp.double().sum(0)[:, 0].cpu().numpy(), sg_ref.numpy(), atol=2e-6 * mag, rtol=1e-4)
        assert float(s[1][5]) == 0.0 and float(s[1][9]) == 0.0
        dw_ref, dgam_ref = _first_block_grads_ref(x, w1, b1, mean, rstd, scale, gref, bits)
        sum_g, sum_gx, dgam, dbet = (torch.empty(C).cuda() for _ in range(4))
        check(L.sed_bn_bwd_finalize(ptr(part), rows, C, ptr(sum_g), ptr(sum_gx), ptr(dgam), ptr(dbet), stream_ptr()), "fin")
        dw, db = torch.empty(C, cin, 3, 3).cuda(), torch.empty(C).cuda()
        check(L.sed_conv1_bwd_wgrad_assemble(ptr(rgp), rows, ptr(mom), ptr(wf1), ptr(b1g), ptr(mean), ptr(rstd), ptr(scale), ptr(sum_g), None,
                                             ptr(dw), ptr(db), B, cin, Fm, T, C, ptr(gg), ptr(bg), ptr(dgam), stream_ptr()), "assemble")
        wmax = float(dw_ref.abs().max())
        print(f"{name} B={B} cin={cin}: sum g {float((s[0] - sg_ref).abs().max()) / mag:.1e} mag, sum g*xhat {float((s[1] - sgx_ref).abs().max()) / mag:.1e} mag, "
              f"dW {float((dw.cpu().double() - dw_ref).abs().max()):.2e} of {2e-5 * wmax:.2e}")
        np.testing.assert_allclose(dw.cpu().double().numpy(), dw_ref.numpy(), atol=2e-5 * wmax, rtol=1e-4)
        np.testing.assert_allclose(dgam.cpu().double().numpy(), dgam_ref.numpy(), atol=2e-5 * float(dgam_ref.abs().max()) + 1e-6, rtol=1e-4)
        assert float(db.abs().max()) < 1e-4 * max(1.0, wmax)                         # analytically zero in front of BatchNorm
