"""The Winograd kernel's patch DMA (wino.hip: buffer_load ... lds through a descriptor of the workgroup's sequence) at the edges.

A lane whose patch position is zero padding — the frame around the (time, mel) plane, the column halo of a column group at the
plane's border, the positions past a ragged block's patch — carries an offset beyond the descriptor's num_records; the range
check has to answer 0 INTO LDS and the lane must reach no neighbouring row, sequence or allocation.  So: the input is a view in
the middle of a larger NaN-filled allocation (a read outside the tensor poisons the output), every sequence is filled differently
(level b + 1: a read from the neighbouring sequence is far outside the bound), and forward, data gradient and the inference
epilogue are compared with torch in float64.  Bounds: the ones test_gpu_kernels.py holds these kernels to (the direct kernel's own
error on the same inputs x 4 + an ulp term of the output scale; inference 2e-5 of the output magnitude).  The data gradient runs
where the kernel takes it (128 channels on both sides)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CIN = 128
GUARD = 1 << 16           # floats of NaN on either side of the input (a multiple of 4: the DMA moves 16-byte pieces)
SHAPES = [(3, 40, 12),    # one ragged block, all four edges
          (8, 40, 16),    # two blocks, XCD-ordered workgroup mapping
          (2, 128, 16),   # two column groups: a column halo between the groups, padding outside
          (1, 2, 2),      # the smallest the geometry takes
          (2, 24, 12)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def guarded(t):
    """t on the GPU as a view in the middle of a NaN-filled allocation; returns (view, allocation)"""
    big = torch.full((2 * GUARD + t.numel(),), float("nan"), device="cuda")
    v = big[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v, big


def guards_intact(big, n):
    return bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[GUARD + n:]).all()) and not bool(torch.isnan(big[GUARD:GUARD + n]).any())


def levelled(B, T, Fm, gen):
    return torch.randn(B, T, Fm, CIN, generator=gen) + torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1)


@pytest.mark.parametrize("Cout", [64, 128])
@pytest.mark.parametrize("B,Fm,T", SHAPES)
def test_forward_and_data_gradient_at_the_edges(ops, B, Fm, T, Cout):
    gen = torch.Generator().manual_seed(B * 1000 + Fm * 10 + T + Cout)
    x = levelled(B, T, Fm, gen)
    w = torch.randn(Cout, CIN, 3, 3, generator=gen) / (3.0 * CIN ** 0.5)
    bias = torch.randn(Cout, generator=gen)
    ref = F.conv2d(x.permute(0, 3, 2, 1).double(), w.double(), bias.double(), padding=1).permute(0, 3, 2, 1).contiguous()
    xg, big = guarded(x)
    uf, ud = ops.conv3x3_wino_pack(w.cuda())
    y, _ = ops.conv3x3_wino_fwd(xg, uf, bias.cuda(), Cout)
    wf0, wd0 = ops.conv3x3_pack(w.cuda())
    y0, _ = ops.conv3x3_fwd(xg, wf0, bias.cuda(), False)
    scale = float(ref.abs().mean())
    err, err0 = (y.cpu().double() - ref).abs(), (y0.cpu().double() - ref).abs()
    print(f"fwd B={B} F={Fm} T={T} Cout={Cout}: max err {float(err.max()):.2e} mean {float(err.mean()):.2e} | direct max {float(err0.max()):.2e} "
          f"mean {float(err0.mean()):.2e} | scale {scale:.2e}")
    assert not bool(torch.isnan(y).any())
    assert float(err.max()) < 4.0 * float(err0.max()) + 2e-6 * scale and float(err.mean()) < 4.0 * float(err0.mean()) + 2e-7 * scale
    assert float(err.max()) < 2e-5 * scale * 10
    assert torch.equal(y, ops.conv3x3_wino_fwd(xg, uf, bias.cuda(), Cout)[0])
    assert guards_intact(big, x.numel())
    if Cout != CIN:
        return
    dy = levelled(B, T, Fm, gen)
    dref = torch.nn.grad.conv2d_input((B, CIN, Fm, T), w.double(), dy.permute(0, 3, 2, 1).contiguous().double(), padding=1).permute(0, 3, 2, 1)
    dyg, dbig = guarded(dy)
    dx, _ = ops.conv3x3_wino_fwd(dyg, ud, None, CIN, want_stats=False)
    dx0, _ = ops.conv3x3_fwd(dyg, wd0, None, False, want_stats=False)
    derr, derr0 = (dx.cpu().double() - dref).abs(), (dx0.cpu().double() - dref).abs()
    print(f"dgrad: max err {float(derr.max()):.2e} | direct max {float(derr0.max()):.2e} | scale {float(dref.abs().mean()):.2e}")
    assert not bool(torch.isnan(dx).any())
    assert float(derr.max()) < 4.0 * float(derr0.max()) + 2e-6 * float(dref.abs().mean()), (float(derr.max()), float(derr0.max()))
    assert torch.equal(dx, ops.conv3x3_wino_fwd(dyg, ud, None, CIN, want_stats=False)[0])
    assert guards_intact(dbig, dy.numel())


def test_inference_epilogue_at_the_edges(ops):
    B, Fm, T, Cout = 2, 40, 12, 128
    gen = torch.Generator().manual_seed(2040)
    x = levelled(B, T, Fm, gen)
    w = torch.randn(Cout, CIN, 3, 3, generator=gen) / (3.0 * CIN ** 0.5)
    bias, beta, rm = (torch.randn(Cout, generator=gen) * 0.3 for _ in range(3))
    gamma = torch.rand(Cout, generator=gen) + 0.5
    gamma[1], gamma[5] = -0.8, 0.0
    rv = torch.rand(Cout, generator=gen) + 0.5
    ref = F.max_pool2d(torch.relu(F.batch_norm(F.conv2d(x.permute(0, 3, 2, 1).double(), w.double(), bias.double(), padding=1), rm.double(),
                                               rv.double(), gamma.double(), beta.double(), training=False, eps=1e-5)), (1, 2)).permute(0, 3, 2, 1)
    xg, big = guarded(x)
    args = [t.cuda() for t in (w, bias, gamma, beta, rm, rv)]
    out = ops.conv3x3_bn_relu_pool_eval(xg, *args, wino=True)
    assert out.shape == (B, T // 2, Fm, Cout) and not bool(torch.isnan(out).any())
    torch.testing.assert_close(out.cpu().double(), ref.contiguous(), atol=2e-5 * max(1.0, float(ref.abs().max())), rtol=1e-5)
    assert torch.equal(out, ops.conv3x3_bn_relu_pool_eval(xg, *args, wino=True))
    assert guards_intact(big, x.numel())
