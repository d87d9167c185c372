"""The epilogues of the Winograd data gradient (wino.hip: BatchNorm-backward sums of the block below, the first block's tap sums)
and the kernel that assembles the first block's gradients from them (conv1_wgrad_assemble_k), against float64.

Until here these kernels were only compared with the direct HIP kernels that share their epilogue code.  The float64 reference
shares nothing with them: dx from torch's conv2d_input, g = dx / keep where the forward's pooled output is positive,
sum g, sum g*xhat (xhat = (keep * pooled - beta) / gamma, the quantity the epilogue is specified to form from the pooled output)
and the first block's gradients from conv -> BatchNorm backward -> conv2d_weight, all in float64.  Tolerances are the ones the
existing tests hold the direct kernels to (test_gpu_kernels.py): 2e-6 * mag for sum g, 6e-6 * mag for sum g*xhat (mag = the
largest per-channel sum |g|), 2e-5 * max|dW| for the assembled weight gradient.  Each test first shows on the CPU that the
epilogue's own formula evaluated per element in float32 stays inside the bound on its inputs, so the bound is one the kernel can
meet."""
import numpy as np
import pytest
import torch

from conv_ref import _bn_sums_ref, _dx_ref, _first_block_grads_ref, _fp32_formula_error  # noqa: E402

pytestmark = pytest.mark.gpu

C = 128


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def g(t):
    return t.cuda().contiguous()


def close(a, b, atol, rtol=1e-4, msg=""):
    np.testing.assert_allclose(a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy(), atol=atol, rtol=rtol, err_msg=msg)


# ───────────────────────── the BatchNorm-backward epilogue alone ─────────────────────────
@pytest.mark.parametrize("B,Ty,Fy,pf,pt,p", [(3, 16, 40, 1, 2, 0.5), (2, 12, 40, 1, 2, 0.0), (2, 8, 64, 1, 2, 0.5), (1, 8, 40, 2, 1, 0.25)])
def test_winograd_dgrad_bn_backward_sums_vs_float64(ops, B, Ty, Fy, pf, pt, p):
    """sed_conv3x3_wino_dgrad_bnred: dx and the partial rows (sum g, sum g*xhat) of the block below, summed over the rows in
    float64, against the float64 reference.  Inputs as test_winograd_dgrad_with_fused_bn_backward_reduction: gamma == 0, a
    negative gamma, |gamma| << |beta| (zeroed by specification, see _bn_sums_ref), dropout on and off, pools (1,2) and (2,1), a
    mel width of two column halves (64)."""
    from sed_crnn_amd._lib import lib, ptr, check, stream_ptr
    L = lib()
    gen = torch.Generator().manual_seed(B * 100 + Ty + Fy)
    yb = torch.randn(B, Ty, Fy, C, generator=gen).cuda()
    gamma = (torch.rand(C, generator=gen) + 0.5)
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[3], beta[3] = 0.0, 0.5
    gamma[17], beta[17] = 0.0, -0.2
    gamma[100] = -0.7
    gamma[8], beta[8] = 1e-3, 0.5
    gamma, beta = gamma.cuda(), beta.cuda()
    flat = yb.reshape(-1, C)
    part0 = torch.stack([flat.sum(0), (flat ** 2).sum(0)]).reshape(1, 2, C).contiguous()
    mean, rstd, scale, shift = ops.bn_finalize_train(part0, B * Ty * Fy, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda())
    pooled = ops.bn_relu_pool_drop_fwd(yb, scale, shift, pf, pt, drop_p=p, seed=99)
    T, Fm = Ty // pt, Fy // pf
    dy = torch.randn(B, T, Fm, C, generator=gen) * 0.1
    w = torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    _, ud = ops.conv3x3_wino_pack(w.cuda())
    rows = L.sed_conv3x3_wino_rows(B, C, Fm, T, C)
    assert rows > 0
    dx, part = torch.empty(B, T, Fm, C).cuda(), torch.full((rows, 2, C), float("nan")).cuda()
    dyg = g(dy)
    check(L.sed_conv3x3_wino_dgrad_bnred(ptr(dyg), ptr(ud), ptr(dx), ptr(part), ptr(pooled), ptr(gamma), ptr(beta), ptr(yb), ptr(mean), ptr(rstd),
                                         p, pf, pt, Fy, Ty, B, C, Fm, T, C, stream_ptr()), "wino_dgrad_bnred")
    keep = 1.0 - p
    dref = _dx_ref(dy, w)
    _, sg_ref, sgx_ref, zero = _bn_sums_ref(dref, pooled, gamma, beta, keep, True)
    mag = float((dref.abs() / keep).sum(dim=(0, 1, 2)).max())
    e1, e2 = _fp32_formula_error(dref, pooled, gamma, beta, keep, zero, sg_ref, sgx_ref)
    print(f"float32 formula on these inputs: sum g {e1:.2e} of {2e-6 * mag:.2e}, sum g*xhat {e2:.2e} of {6e-6 * mag:.2e}")
    assert e1 < 2e-6 * mag and e2 < 6e-6 * mag
    assert float((dx.cpu().double() - dref).abs().max()) < 2e-5 * float(dref.abs().mean()) * 10      # the Winograd forward's bound
    s = part.double().sum(0).cpu()
    assert bool(torch.isfinite(s).all())
    print(f"kernel: sum g {float((s[0] - sg_ref).abs().max()):.2e}, sum g*xhat {float((s[1] - sgx_ref).abs().max()):.2e}")
    close(s[0], sg_ref, atol=2e-6 * mag, rtol=1e-4)
    close(s[1], sgx_ref, atol=6e-6 * mag, rtol=1e-4)
    assert float(s[1][3]) == 0.0 and float(s[1][17]) == 0.0 and float(s[1][8]) == 0.0


# ───────────────────────── + the first block's tap sums ─────────────────────────
RG_CASES = [(3, 40, 12, 0.5, 1),      # 60 tiles: one ragged block
            (8, 40, 16, 0.5, 1),      # two blocks, the second with 16 tiles; B = 8: the XCD-ordered workgroup mapping
            (2, 24, 12, 0.0, 1),
            (2, 128, 16, 0.5, 1),     # two column groups
            (3, 40, 12, 0.5, 2), (8, 40, 16, 0.3, 2)]      # two input channels: the rolling prefetch


@pytest.mark.parametrize("B,Fm,T,p,cin", RG_CASES)
def test_winograd_dgrad_tap_sums_without_dx_and_vs_float64(ops, B, Fm, T, p, cin):
    """sed_conv3x3_wino_dgrad_bnred_rg behind the real first-block forward (its pooled output and arg-max bits):
    1. dx = NULL against dx given: the BatchNorm partial rows and the tap-sum rows are the same bit for bit;
    2. dx, sum g, sum g*xhat against float64, and dW / dbias / dgamma of the first block after sed_bn_bwd_finalize +
       sed_conv1_bwd_wgrad_assemble against conv -> BatchNorm backward (the forward's mean / rstd / scale) -> conv2d_weight in
       float64, with g routed by the arg-max bits.
    gamma == 0 with both signs of beta, a negative gamma and a tiny gamma (1e-3, with a beta of its size: xhat from the pooled
    output keeps its precision); edge tiles in time and mel, ragged blocks, one and two column groups, dropout on and off."""
    from sed_crnn_amd._lib import lib, ptr, check, stream_ptr
    L = lib()
    Tp = T // 2
    rows = L.sed_conv3x3_wino_rg_rows(B, C, Fm, Tp, C, cin)
    if not rows:
        pytest.skip("shape does not take the fused Winograd path")
    gen = torch.Generator().manual_seed(B * 1000 + Fm * 10 + T + cin)
    x = torch.randn(B, cin, Fm, T, generator=gen)
    w1 = torch.randn(C, cin, 3, 3, generator=gen) * 0.4
    b1 = torch.randn(C, generator=gen) * 0.1
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[5], beta[5] = 0.0, 0.4
    gamma[9], beta[9] = 0.0, -0.3
    gamma[64] = -0.8
    gamma[33], beta[33] = 1e-3, 2e-3
    w2 = torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    dy = torch.randn(B, Tp, Fm, C, generator=gen) * 0.1
    seed = 11
    # forward of the first block (statistics from the input moments, arg-max bits)
    wf1, _ = ops.conv3x3_pack(g(w1))
    stat = torch.empty(1, 2, C).cuda()
    sws = torch.empty(L.sed_conv1_stats_workspace_bytes(B, cin, T) // 4 + 1).cuda()
    mom = torch.empty(L.sed_conv1_moments_doubles(cin), dtype=torch.float64).cuda()
    xg, b1g, gg, bg = g(x), g(b1), g(gamma), g(beta)
    check(L.sed_conv1_stats(ptr(xg), ptr(wf1), ptr(b1g), ptr(stat), ptr(sws), B, cin, Fm, T, C, ptr(mom), stream_ptr()), "conv1_stats")
    mean, rstd, scale, shift = ops.bn_finalize_train(stat, B * T * Fm, gg, bg, torch.zeros(C).cuda(), torch.ones(C).cuda())
    pooled = torch.empty(B, Tp, Fm, C).cuda()
    bits = torch.empty(pooled.numel() // 4, dtype=torch.uint8).cuda()
    check(L.sed_conv1_bn_relu_pool_drop_fwd(ptr(xg), ptr(wf1), ptr(b1g), ptr(scale), ptr(shift), ptr(pooled), B, cin, Fm, T, C, 1, 2, p, seed,
                                            None, ptr(bits), stream_ptr()), "conv1_fwd")
    _, ud2 = ops.conv3x3_wino_pack(g(w2))
    dyg = g(dy)

    def run(with_dx):
        dx = torch.full((B, Tp, Fm, C), float("nan")).cuda()
        part = torch.full((rows, 2, C), float("nan")).cuda()
        rgp = torch.full((rows, C, 1 + 9 * cin), float("nan")).cuda()
        check(L.sed_conv3x3_wino_dgrad_bnred_rg(ptr(dyg), ptr(ud2), ptr(dx) if with_dx else None, ptr(part), ptr(pooled), ptr(gg), ptr(bg), ptr(mean),
                                                ptr(rstd), p, ptr(xg), cin, ptr(bits), ptr(rgp), B, C, Fm, Tp, C, stream_ptr()), "wino_dgrad_bnred_rg")
        return dx, part, rgp

    dx, part, rgp = run(True)
    dx_n, part_n, rgp_n = run(False)
    # 1. without dx: nothing else changes, and dx is not touched
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(rgp).all())
    assert torch.equal(part, part_n) and torch.equal(rgp, rgp_n)
    assert bool(torch.isnan(dx_n).all())
    # 2. float64
    keep = 1.0 - p
    dref = _dx_ref(dy, w2)
    gref, sg_ref, sgx_ref, zero = _bn_sums_ref(dref, pooled, gg, bg, keep, False)
    mag = float((dref.abs() / keep).sum(dim=(0, 1, 2)).max())
    e1, e2 = _fp32_formula_error(dref, pooled, gg, bg, keep, zero, sg_ref, sgx_ref)
    print(f"float32 formula on these inputs: sum g {e1:.2e} of {2e-6 * mag:.2e}, sum g*xhat {e2:.2e} of {6e-6 * mag:.2e}")
    assert e1 < 2e-6 * mag and e2 < 6e-6 * mag
    assert float((dx.cpu().double() - dref).abs().max()) < 2e-5 * float(dref.abs().mean()) * 10
    s = part.double().sum(0).cpu()
    print(f"kernel: sum g {float((s[0] - sg_ref).abs().max()):.2e}, sum g*xhat {float((s[1] - sgx_ref).abs().max()):.2e}")
    close(s[0], sg_ref, atol=2e-6 * mag, rtol=1e-4)
    close(s[1], sgx_ref, atol=6e-6 * mag, rtol=1e-4)
    close(rgp.double().sum(0)[:, 0], sg_ref, atol=2e-6 * mag, rtol=1e-4)
    assert float(s[1][5]) == 0.0 and float(s[1][9]) == 0.0
    # the first block's gradients: the gradient of the selected conv output is g at time 2 t' + (arg-max bit), zero elsewhere
    dw_ref, dgam_ref = _first_block_grads_ref(x, w1, b1, mean, rstd, scale, gref, bits)
    sum_g, sum_gx, dgam, dbet = (torch.empty(C).cuda() for _ in range(4))
    check(L.sed_bn_bwd_finalize(ptr(part), rows, C, ptr(sum_g), ptr(sum_gx), ptr(dgam), ptr(dbet), stream_ptr()), "fin")
    dw, db = torch.empty(C, cin, 3, 3).cuda(), torch.empty(C).cuda()
    check(L.sed_conv1_bwd_wgrad_assemble(ptr(rgp), rows, ptr(mom), ptr(wf1), ptr(b1g), ptr(mean), ptr(rstd), ptr(scale), ptr(sum_g), None,
                                         ptr(dw), ptr(db), B, cin, Fm, T, C, ptr(gg), ptr(bg), ptr(dgam), stream_ptr()), "assemble")
    wmax = float(dw_ref.abs().max())
    print(f"kernel: dW {float((dw.cpu().double() - dw_ref).abs().max()):.2e} of {2e-5 * wmax:.2e}")
    close(dw, dw_ref, atol=2e-5 * wmax, rtol=1e-4)
    close(dgam, dgam_ref, atol=2e-5 * float(dgam_ref.abs().max()) + 1e-6, rtol=1e-4)
    assert float(db.abs().max()) < 1e-4 * max(1.0, wmax)                             # analytically zero in front of BatchNorm


# ───────────────────────── the assembling kernel ─────────────────────────
def _assemble_ref(part, gram, wp, bias, mean, rstd, scale, sum_g, sum_gx, count, cin):
    """conv1_wgrad_assemble_k's closed form in float64 (numpy), the partial rows summed by numpy"""
    rows, Cc, NV = part.shape
    NK = 9 * cin
    sv = part.astype(np.float64).sum(0)                                              # [C][NV]
    gidx = lambda k, k2: NK + k * NK - (k * (k - 1)) // 2 + (k2 - k)
    Gm = np.array([[gram[gidx(min(k, k2), max(k, k2))] for k2 in range(NK)] for k in range(NK)])
    dw, db, dgam = np.zeros((Cc, cin, 9)), np.zeros(Cc), np.zeros(Cc)
    for co in range(Cc):
        w2 = np.array([wp[((k2 // cin) * Cc + co) * cin + (k2 % cin)] for k2 in range(NK)], dtype=np.float64)
        b, mu, rs, sc = float(bias[co]), float(mean[co]), float(rstd[co]), float(scale[co])
        ws1, wr = float(w2 @ gram[:NK]), float(w2 @ sv[co, 1:])
        sgx_sum = rs * (b * sv[co, 0] + wr - mu * sv[co, 0])
        sg = float(sum_g[co]) / count
        sgx = (sgx_sum if sum_gx is None else float(sum_gx[co])) / count
        for k in range(NK):
            wg, s1 = float(w2 @ Gm[k]), gram[k]
            dw[co, k % cin, k // cin] = sc * (sv[co, 1 + k] - sg * s1 - sgx * rs * (b * s1 + wg - mu * s1))
        db[co] = sc * (sv[co, 0] - count * sg - sgx * rs * ((count * b + ws1) - count * mu))
        dgam[co] = sgx_sum
    return dw, db, dgam


@pytest.mark.parametrize("rows,cin,own", [(1, 1, True), (255, 1, True), (256, 1, False), (257, 1, True), (2560, 1, True), (2560, 1, False),
                                          (257, 2, True), (2560, 2, True), (1300, 3, True), (700, 4, False)])
def test_first_block_gradient_assembly_vs_float64(ops, rows, cin, own):
    """sed_conv1_bwd_wgrad_assemble on partial rows from a seeded generator: fewer rows than threads, one row short of / exactly /
    one past a round of the workgroup, ten rounds (the training shape), every input-channel count (each keeps another number of
    rows in flight), with the block's own sum g*xhat and with a given one.  The kernel sums the rows in float64 in a fixed
    order that is not numpy's, and hipcc contracts the closed form's multiply-adds: equality with the float64 evaluation rounded
    once to float32 cannot be had for every element, so each must lie within ONE float32 ulp of it (and most are equal)."""
    from sed_crnn_amd._lib import lib, ptr, check, stream_ptr
    L = lib()
    Cc, B, Fm, T = 8, 4, 40, 16
    rng = np.random.default_rng(rows * 10 + cin)
    NV = 1 + 9 * cin
    part = rng.standard_normal((rows, Cc, NV)).astype(np.float32)
    nmom = L.sed_conv1_moments_doubles(cin)
    assert nmom >= 9 * cin + (9 * cin) * (9 * cin + 1) // 2
    gram = rng.standard_normal(nmom) * 3.0
    wp = (rng.standard_normal(9 * Cc * cin) * 0.4).astype(np.float32)
    bias, mean = (rng.standard_normal(Cc) * 0.1).astype(np.float32), (rng.standard_normal(Cc) * 0.2).astype(np.float32)
    rstd, scale = (rng.random(Cc) + 0.5).astype(np.float32), (rng.standard_normal(Cc)).astype(np.float32)
    sum_g, sum_gx = (rng.standard_normal(Cc) * 5).astype(np.float32), (rng.standard_normal(Cc) * 5).astype(np.float32)
    dev = lambda a: torch.from_numpy(a).cuda()
    t = {k: dev(v) for k, v in dict(part=part, gram=gram, wp=wp, bias=bias, mean=mean, rstd=rstd, scale=scale, sum_g=sum_g, sum_gx=sum_gx).items()}
    dw, db, dgam = torch.full((Cc, cin, 3, 3), float("nan")).cuda(), torch.full((Cc,), float("nan")).cuda(), torch.full((Cc,), float("nan")).cuda()
    gamma, beta = torch.ones(Cc).cuda(), torch.ones(Cc).cuda()
    check(L.sed_conv1_bwd_wgrad_assemble(ptr(t["part"]), rows, ptr(t["gram"]), ptr(t["wp"]), ptr(t["bias"]), ptr(t["mean"]), ptr(t["rstd"]), ptr(t["scale"]),
                                         ptr(t["sum_g"]), None if own else ptr(t["sum_gx"]), ptr(dw), ptr(db), B, cin, Fm, T, Cc, ptr(gamma), ptr(beta),
                                         ptr(dgam), stream_ptr()), "assemble")
    dw_ref, db_ref, dgam_ref = _assemble_ref(part, gram, wp, bias, mean, rstd, scale, sum_g, None if own else sum_gx, float(B * T * Fm), cin)
    pairs = [("dW", dw.cpu().numpy().reshape(Cc, cin, 9), dw_ref), ("dbias", db.cpu().numpy(), db_ref)]
    if own:                                                     # (a given sum g*xhat: dgamma is left to the caller except for gamma == 0)
        pairs.append(("dgamma", dgam.cpu().numpy(), dgam_ref))
    for name, got, ref in pairs:
        r32 = ref.astype(np.float32)
        ulp = np.spacing(np.abs(r32))
        bad = np.abs(got.astype(np.float64) - r32.astype(np.float64)) > ulp
        print(f"{name}: {int((got != r32).sum())} of {got.size} differ from the rounded float64 value")
        assert not bad.any(), (name, got[bad], r32[bad])
