"""The Winograd kernel's prologue (wino.hip: workgroup mapping by reciprocal multiplies, the patch-DMA offsets by a carry per KiB
block) on the GPU, at shapes of a few workgroups that take every path of the walk: a mel width whose patch row (F2 = 2 Fw + 2) is
far below the 32 positions of a block (several row wraps per step), around it (30: F2 = 32, 40: F2 = 42), above it (62: F2 = 64),
two column groups (128), batch sizes on (8) and off (1, 2, 3, 9) the XCD-ordered mapping, ragged blocks.

Every instantiation against the direct kernel with the same epilogue on the same data — forward, data gradient with the
BatchNorm-backward sums, with the first block's tap sums of one and two input channels on top, and the inference epilogue — with
the bounds test_gpu_kernels.py holds the Winograd forms to.  The tensor the DMA reads lies in the middle of a NaN-filled
allocation, each sequence at its own level (tests/test_gpu_wino_patch_dma.py): one padding lane with a real offset, or one offset
into a neighbouring row or sequence, poisons or shifts the output."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 128
GUARD = 1 << 16
SHAPES = [(3, 4, 6), (9, 14, 10), (8, 30, 4), (8, 40, 6), (1, 62, 2), (2, 128, 4)]           # (B, F, T)
EPILOGUE_SHAPES = [(9, 14, 10), (8, 40, 6), (2, 128, 4)]


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


def guarded(t):
    """t on the GPU as a view in the middle of a NaN-filled allocation; returns (view, allocation)"""
    big = torch.full((2 * GUARD + t.numel(),), float("nan"), device="cuda")
    v = big[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v, big


def guards_intact(big, n):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + n:]).all()) and not bool(torch.isnan(big[GUARD:GUARD + n]).any())


def levelled(B, T, Fm, gen, amp=1.0):
    return (torch.randn(B, T, Fm, C, generator=gen) + torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1)) * amp


@pytest.mark.parametrize("B,Fm,T", SHAPES)
def test_forward_against_the_direct_kernel(ops, B, Fm, T):
    """sed_conv3x3_wino_fwd next to sed_conv3x3_fwd, both against float64: 4 x the direct kernel's error + an ulp term
    (test_conv3x3_winograd_forward_and_data_gradient), values and statistic rows"""
    gen = torch.Generator().manual_seed(B * 1000 + Fm * 10 + T)
    x = levelled(B, T, Fm, gen)
    w = torch.randn(C, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)
    bias = torch.randn(C, generator=gen)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 2, 1).double(), w.double(), bias.double(), padding=1).permute(0, 3, 2, 1).contiguous()
    xg, big = guarded(x)
    uf, _ = ops.conv3x3_wino_pack(g(w))
    y, stat = ops.conv3x3_wino_fwd(xg, uf, g(bias), C)
    wf0, _ = ops.conv3x3_pack(g(w))
    y0, _ = ops.conv3x3_fwd(xg, wf0, g(bias), False)
    scale = float(ref.abs().mean())
    err, err0 = (y.cpu().double() - ref).abs(), (y0.cpu().double() - ref).abs()
    print(f"fwd B={B} F={Fm} T={T}: max err {float(err.max()):.2e} mean {float(err.mean()):.2e} | direct max {float(err0.max()):.2e} "
          f"mean {float(err0.mean()):.2e} | scale {scale:.2e}")
    assert not bool(torch.isnan(y).any())
    assert float(err.max()) < 4.0 * float(err0.max()) + 2e-6 * scale and float(err.mean()) < 4.0 * float(err0.mean()) + 2e-7 * scale
    assert float(err.max()) < 2e-5 * scale * 10
    s = stat.sum(0).cpu().double()
    torch.testing.assert_close(s[0], ref.sum((0, 1, 2)), rtol=1e-4, atol=2e-5 * scale * B * T * Fm)
    assert torch.equal(y, ops.conv3x3_wino_fwd(xg, uf, g(bias), C)[0])
    assert guards_intact(big, x.numel())


@pytest.mark.parametrize("B,Fm,T", EPILOGUE_SHAPES)
def test_data_gradient_with_bn_backward_sums_against_the_direct_kernel(ops, B, Fm, T):
    """sed_conv3x3_wino_dgrad_bnred against sed_conv3x3_dgrad_bnred (test_winograd_dgrad_with_fused_bn_backward_reduction)"""
    pf, pt, p = 1, 2, 0.5
    Ty, Fy = T * pt, Fm * pf
    gen = torch.Generator().manual_seed(B * 100 + Ty + Fy)
    yb = torch.randn(B, Ty, Fy, C, generator=gen).cuda()
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[3], beta[3] = 0.0, 0.5
    gamma[100] = -0.7
    gamma[8], beta[8] = 1e-3, 0.5
    gamma, beta = gamma.cuda(), beta.cuda()
    flat = yb.reshape(-1, C)
    part = torch.stack([flat.sum(0), (flat ** 2).sum(0)]).reshape(1, 2, C).contiguous()
    mean, rstd, scale, shift = ops.bn_finalize_train(part, B * Ty * Fy, gamma, beta, torch.zeros(C).cuda(), torch.ones(C).cuda())
    pooled = ops.bn_relu_pool_drop_fwd(yb, scale, shift, pf, pt, drop_p=p, seed=99)
    dy = levelled(B, T, Fm, gen, 0.1)
    dyg, big = guarded(dy)
    w = (torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)).cuda()
    _, wd = ops.conv3x3_pack(w)
    _, ud = ops.conv3x3_wino_pack(w)
    dx0, sg0, sgx0 = ops.conv3x3_dgrad_bnred(dyg, wd, pooled, gamma, beta, yb, mean, rstd, pf, pt, drop_p=p, scale=scale, shift=shift)
    dx, sg, sgx = ops.conv3x3_dgrad_bnred(dyg, ud, pooled, gamma, beta, yb, mean, rstd, pf, pt, drop_p=p, scale=scale, shift=shift, wino=True)
    assert not bool(torch.isnan(dx).any())
    close(dx, dx0, atol=2e-6 * float(dx0.abs().mean()) * 10, rtol=1e-5)
    mag = float((dx0.abs() / (1.0 - p)).sum(dim=(0, 1, 2)).max())
    close(sg, sg0, atol=2e-6 * mag, rtol=1e-4)
    close(sgx, sgx0, atol=6e-6 * mag, rtol=1e-4)
    assert guards_intact(big, dy.numel())


@pytest.mark.parametrize("cin", [1, 2])
@pytest.mark.parametrize("B,Fm,Tp", EPILOGUE_SHAPES)
def test_data_gradient_with_tap_sums_against_the_direct_kernel(ops, B, Fm, Tp, cin):
    """sed_conv3x3_wino_dgrad_bnred_rg against sed_conv3x3_dgrad_bnred_rg behind the real first-block forward, the first block's
    gradients assembled from either (test_first_block_weight_gradient_sums_from_the_data_gradient_epilogue)"""
    from sed_crnn_amd._lib import lib, ptr, check, stream_ptr
    L = lib()
    T, p, seed = 2 * Tp, 0.5, 11
    rows = L.sed_conv3x3_dgrad_bnred_rg_rows(B, C, Fm, Tp, C, cin)
    rows_w = L.sed_conv3x3_wino_rg_rows(B, C, Fm, Tp, C, cin)
    assert rows > 0 and rows_w > 0
    gen = torch.Generator().manual_seed(B * 1000 + Fm * 10 + T + cin)
    x = torch.randn(B, cin, Fm, T, generator=gen)
    w1 = torch.randn(C, cin, 3, 3, generator=gen) * 0.4
    b1 = torch.randn(C, generator=gen) * 0.1
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.3
    gamma[5], beta[5] = 0.0, 0.4
    gamma[9], beta[9] = 0.0, -0.3
    gamma[64] = -0.8
    w2 = torch.randn(C, C, 3, 3, generator=gen) / np.sqrt(9 * C)
    dy = levelled(B, Tp, Fm, gen, 0.1)
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
    _, wd2 = ops.conv3x3_pack(g(w2))
    _, ud2 = ops.conv3x3_wino_pack(g(w2))
    dyg, big = guarded(dy)

    def assembled(part, rgp, n):
        sum_g, sum_gx, dgam, dbet = (torch.empty(C).cuda() for _ in range(4))
        check(L.sed_bn_bwd_finalize(ptr(part), n, C, ptr(sum_g), ptr(sum_gx), ptr(dgam), ptr(dbet), stream_ptr()), "fin")
        dw, db = torch.empty(C, cin, 3, 3).cuda(), torch.empty(C).cuda()
        check(L.sed_conv1_bwd_wgrad_assemble(ptr(rgp), n, ptr(mom), ptr(wf1), ptr(b1g), ptr(mean), ptr(rstd), ptr(scale), ptr(sum_g), ptr(sum_gx),
                                             ptr(dw), ptr(db), B, cin, Fm, T, C, ptr(gg), ptr(bg), ptr(dgam), stream_ptr()), "assemble")
        return sum_g, dw, db, dgam

    dx_a, part_a = torch.empty(B, Tp, Fm, C).cuda(), torch.empty(rows, 2, C).cuda()
    rgp = torch.full((rows, C, 1 + 9 * cin), float("nan")).cuda()
    check(L.sed_conv3x3_dgrad_bnred_rg(ptr(dyg), ptr(wd2), ptr(dx_a), ptr(part_a), ptr(pooled), ptr(gg), ptr(bg), ptr(mean), ptr(rstd), p,
                                       ptr(xg), cin, ptr(bits), ptr(rgp), B, C, Fm, Tp, C, stream_ptr()), "dgrad_bnred_rg")
    sg_a, dw_a, db_a, dgam_a = assembled(part_a, rgp, rows)
    dx_w, part_w = torch.full((B, Tp, Fm, C), float("nan")).cuda(), torch.empty(rows_w, 2, C).cuda()
    rgw = torch.full((rows_w, C, 1 + 9 * cin), float("nan")).cuda()
    check(L.sed_conv3x3_wino_dgrad_bnred_rg(ptr(dyg), ptr(ud2), ptr(dx_w), ptr(part_w), ptr(pooled), ptr(gg), ptr(bg), ptr(mean), ptr(rstd), p,
                                            ptr(xg), cin, ptr(bits), ptr(rgw), B, C, Fm, Tp, C, stream_ptr()), "wino_dgrad_bnred_rg")
    _, dw_w, db_w, dgam_w = assembled(part_w, rgw, rows_w)
    assert bool(torch.isfinite(rgw).all()) and not bool(torch.isnan(dx_w).any())
    mag = float(dw_a.abs().max())
    close(dx_w, dx_a, atol=2e-5 * float(dx_a.abs().mean()), rtol=1e-5)
    close(dw_w, dw_a, atol=2e-5 * mag, rtol=1e-4)
    close(db_w, db_a, atol=4e-6 * float((sg_a.abs() * scale.abs()).max()) + 1e-6, rtol=1e-4)
    close(dgam_w, dgam_a, atol=2e-5 * float(dgam_a.abs().max()) + 1e-6, rtol=1e-4)
    assert guards_intact(big, dy.numel())


@pytest.mark.parametrize("B,Fm,T", EPILOGUE_SHAPES)
def test_inference_epilogue_against_the_direct_kernel(ops, B, Fm, T):
    """sed_conv3x3_wino_bn_relu_pool_eval next to sed_conv3x3_bn_relu_pool_eval, both within the bound
    test_conv3x3_bn_relu_pool_eval holds them to against float64 — so within twice that of each other"""
    import torch.nn.functional as F
    from sed_crnn_amd._lib import lib
    assert lib().sed_conv3x3_bn_relu_pool_eval_supported(B, C, Fm, T, C)
    gen = torch.Generator().manual_seed(B * 1000 + T * 10 + Fm)
    x = levelled(B, T, Fm, gen)
    w = torch.randn(C, C, 3, 3, generator=gen) / (3.0 * C ** 0.5)
    bias, beta, rm = (torch.randn(C, generator=gen) * 0.3 for _ in range(3))
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[1], gamma[5] = -0.8, 0.0
    rv = torch.rand(C, generator=gen) + 0.5
    ref = F.max_pool2d(torch.relu(F.batch_norm(F.conv2d(x.permute(0, 3, 2, 1).double(), w.double(), bias.double(), padding=1), rm.double(),
                                               rv.double(), gamma.double(), beta.double(), training=False, eps=1e-5)), (1, 2)).permute(0, 3, 2, 1).contiguous()
    xg, big = guarded(x)
    args = [g(t) for t in (w, bias, gamma, beta, rm, rv)]
    out0 = ops.conv3x3_bn_relu_pool_eval(xg, *args)
    out = ops.conv3x3_bn_relu_pool_eval(xg, *args, wino=True)
    assert out.shape == (B, T // 2, Fm, C) and not bool(torch.isnan(out).any())
    atol = 2e-5 * max(1.0, float(ref.abs().max()))
    close(out0, ref, atol=atol, rtol=1e-5)
    close(out, ref, atol=atol, rtol=1e-5)
    assert torch.equal(out, ops.conv3x3_bn_relu_pool_eval(xg, *args, wino=True))
    assert guards_intact(big, x.numel())
