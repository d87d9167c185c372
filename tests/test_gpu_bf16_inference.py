"""The opt-in bf16 inference plan (model.set_inference_precision("bf16"), sed_net_cfg.conv_mode = 2) against the CPU float64
emulation of tests/bf16_emul.py, which rounds to bf16 at exactly the plan's three points.  Tolerances: one bf16 ulp of the
reference plus the fp32 accumulation floor K 2^-23 (|w'| * |x| + |b'|) per element (bf16_emul.block_floor); the share of elements that differ from
bf16(reference) at all is bounded and printed.  The fp32 plan must not move at all."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emul as emu  # noqa: E402

pytestmark = pytest.mark.gpu

MISMATCH_BOUND = 0.02          # share of elements != bf16(ref); observed values are printed (expected ~0.1-0.5 %)


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


@pytest.fixture(scope="module")
def ops(sed):
    from sed_crnn_amd import ops as o
    return o


def _block_modules(Cin, Cout, gen):
    conv, bn = nn.Conv2d(Cin, Cout, 3, padding=1), nn.BatchNorm2d(Cout)
    with torch.no_grad():
        conv.weight.copy_((torch.rand(conv.weight.shape, generator=gen) * 2 - 1) / np.sqrt(9 * Cin))
        conv.bias.copy_(torch.rand(Cout, generator=gen) * 0.2 - 0.1)
        bn.weight.copy_(torch.rand(Cout, generator=gen) + 0.5)
        bn.bias.copy_(torch.rand(Cout, generator=gen) * 0.4 - 0.2)
        bn.running_mean.copy_(torch.rand(Cout, generator=gen) * 0.2 - 0.1)
        bn.running_var.copy_(torch.rand(Cout, generator=gen) + 0.5)
    return conv, bn


class _OneBlock:                 # what emu.blocks() reads from a reference model
    def __init__(self, conv, bn):
        self.convs, self.bns, self.time_pool = [conv], [bn], (2,)
        self.drop = nn.Dropout(0.0)


def _check_block(hip_cl, x_nchw, model, l, tag):
    """hip_cl: HIP's bf16 output [B,Tp,F,C]; x_nchw: the input it ran on (float64 view of it)"""
    ref = emu.block(model, l, x_nchw, True).permute(0, 3, 2, 1)                 # [B,Tp,F,C]
    flo = emu.block_floor(model, l, x_nchw, True).permute(0, 3, 2, 1)
    got = hip_cl.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    tol = emu.bf16_ulp(ref) + flo
    bad = (err > tol).sum().item()
    frac = (got != emu.bf16(ref)).double().mean().item()
    print(f"{tag}: max err / tol {(err / tol).max().item():.3f}, share != bf16(ref) {100 * frac:.3f} % (bound {100 * MISMATCH_BOUND:.1f} %)")
    assert bad == 0, f"{tag}: {bad} elements beyond one bf16 ulp + the fp32 floor"
    assert frac <= MISMATCH_BOUND, tag


CONV_CASES = [  # B, Cin, Cout, F, T, input bf16
    (1, 32, 64, 20, 2, False), (2, 32, 128, 37, 9, True), (3, 64, 64, 40, 16, True), (2, 64, 256, 64, 7, False),
    (4, 128, 128, 40, 32, True), (1, 128, 128, 128, 12, False), (2, 128, 64, 37, 5, True), (16, 128, 128, 40, 16, True),
    (1, 256, 128, 20, 10, True), (2, 256, 256, 40, 6, False), (5, 128, 256, 128, 3, True), (8, 32, 128, 64, 33, False),
]


@pytest.mark.parametrize("B,Cin,Cout,Fm,T,xbf", CONV_CASES)
def test_bf16_conv_block_against_float64(ops, B, Cin, Cout, Fm, T, xbf):
    gen = torch.Generator().manual_seed(B * 7919 + Cin * 31 + Cout + Fm * 3 + T)
    conv, bn = _block_modules(Cin, Cout, gen)
    x = torch.randn(B, T, Fm, Cin, generator=gen)                               # channels-last
    xg = x.cuda().to(torch.bfloat16) if xbf else x.cuda()
    wf, bf = ops.conv3x3_bf16_pack_folded(*(t.detach().cuda().contiguous() for t in (conv.weight, conv.bias, bn.weight, bn.bias,
                                                                                       bn.running_mean, bn.running_var)), eps=bn.eps)
    y = ops.conv3x3_bf16_bn_relu_pool_eval(xg, wf, bf, Cout)
    y2 = ops.conv3x3_bf16_bn_relu_pool_eval(xg, wf, bf, Cout)
    torch.cuda.synchronize()
    assert torch.equal(y, y2), "run-to-run"
    x_in = xg.cpu().double().permute(0, 3, 2, 1)                               # NCHW [B,Cin,F,T]
    _check_block(y, x_in, _OneBlock(conv, bn), 0, f"conv B{B} {Cin}->{Cout} F{Fm} T{T} {'bf16' if xbf else 'fp32'} in")


GEMM_CASES = [(1, 768, 640), (37, 768, 5120), (128, 1536, 16384), (4096, 768, 5120), (300, 96, 1280), (1000, 200, 2048)]


@pytest.mark.parametrize("M,N,K", GEMM_CASES)
def test_bf16_gemm_against_float64(ops, M, N, K):
    gen = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(M, K, generator=gen)).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=gen) / np.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn(N, generator=gen)
    out = ops.gemm_bf16_nt(A.cuda(), W.cuda(), bias.cuda())
    out2 = ops.gemm_bf16_nt(A.cuda(), W.cuda(), bias.cuda())
    assert torch.equal(out, out2)
    ref = A.double() @ W.double().t() + bias.double()
    flo = K * 2.0 ** -24 * (A.double().abs() @ W.double().abs().t() + bias.double().abs()) + 2.0 ** -24 * ref.abs()
    err = (out.cpu().double() - ref).abs()
    print(f"gemm {M}x{N}x{K}: max err / floor {(err / flo).max().item():.3f}")
    assert (err <= flo).all()
    # rows are independent: a slice of the rows gives the same bits
    if M > 8:
        part = ops.gemm_bf16_nt(A[3:M - 2].contiguous().cuda(), W.cuda(), bias.cuda())
        assert torch.equal(part, out[3:M - 2])


def _nets(sed, cfg):
    from oracle import crnn_ref
    if cfg == 2:
        kw, B, T, Cin, Fm = dict(conv_channels=128, gru_hidden=128), 128, 256, 1, 40
    elif cfg == 3:
        kw, B, T, Cin, Fm = dict(conv_channels=128, gru_hidden=128, in_channels=2), 128, 256, 2, 40
    else:
        kw, B, T, Cin, Fm = dict(conv_channels=128, gru_hidden=256, in_channels=4, n_mels=128), 2, 512, 4, 128
    ref = crnn_ref.SedNetRef(dropout=0.5, **kw)
    ref.load_state_dict(crnn_ref.rs_state_dict(ref, 100 + cfg))
    ref.eval()
    m = sed.TimePooledCRNN(dropout=0.5, **kw)
    m.load_state_dict(ref.state_dict())
    m.cuda().eval()
    g = torch.Generator().manual_seed(cfg)
    x = torch.randn(B, Cin, Fm, T, generator=g)
    return ref, m, x


@pytest.mark.parametrize("cfg", [2, 3, 5])
def test_network_block_by_block(sed, cfg):
    ref, m, x = _nets(sed, cfg)
    m.set_inference_precision("bf16")
    plan = m.inference_plan(x.shape[0], x.shape[3])
    assert plan == {"conv": ["f32", "bf16", "bf16"], "proj": "bf16"}
    with torch.no_grad():
        lg = m(x.cuda())
    torch.cuda.synchronize()
    pooled = [m.eval_workspace_view("pooled", l).clone() for l in range(3)]
    assert pooled[0].dtype == torch.float32 and pooled[1].dtype == torch.bfloat16 and pooled[2].dtype == torch.bfloat16
    B, T, Fm = x.shape[0], x.shape[3], x.shape[2]
    for l in (1, 2):
        Tin, Tout = T >> l, T >> (l + 1)
        xin = pooled[l - 1].view(B, Tin, Fm, 128).cpu().double().permute(0, 3, 2, 1)
        _check_block(pooled[l].view(B, Tout, Fm, 128), xin, ref, l, f"config {cfg} block {l}")
    # the head fed with HIP's last pooled output: projection rounding is part of the emulation, the rest float64
    last = pooled[2].view(B, T >> 3, Fm, 128).cpu().double().permute(0, 3, 2, 1)
    want = emu.head(ref, last, True)
    d = (lg.cpu().double() - want).abs().max().item()
    print(f"config {cfg}: logits vs emulated head on HIP's pooled output: max |d| {d:.2e}")
    assert d < 2e-3 * max(1.0, want.abs().max().item())


def _accuracy(ref, hip_logits, x, plan, tag):
    with torch.no_grad():
        p64 = torch.sigmoid(ref.double()(x.double()))
    ref.float()
    _, lg_e = emu.forward(ref, x, plan)
    pe = torch.sigmoid(lg_e)
    dist = (pe - p64).abs().max().item()
    ph = torch.sigmoid(hip_logits.cpu().double())
    dp = (ph - p64).abs().max().item()
    rel = ((hip_logits.cpu().double() - torch.logit(p64)).norm() / torch.logit(p64).norm()).item()
    sure = (p64 - 0.5).abs() > 3 * dist
    flips = ((ph > 0.5) != (p64 > 0.5)) & sure
    print(f"{tag}: emulated bf16 vs float64 max |dp| {dist:.2e}; HIP bf16 vs float64 max |dp| {dp:.2e}, logit rel L2 {rel:.2e}, "
          f"{int(sure.sum())}/{sure.numel()} decisions sure by > 3x, {int(flips.sum())} flipped")
    assert int(flips.sum()) == 0
    return dist, dp


def test_accuracy_statement_against_float64(sed, golden_dir):
    from oracle import crnn_ref
    g5 = dict(np.load(os.path.join(golden_dir, "g5_sed_c128.npz")))
    ref = crnn_ref.SedNetRef(conv_channels=128, dropout=0.5, gru_hidden=32)
    ref.load_state_dict(crnn_ref.rs_state_dict(ref, int(g5["weight_seed"])))
    ref.eval()
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=32)
    m.load_state_dict(ref.state_dict())
    m.cuda().eval().set_inference_precision("bf16")
    x = torch.from_numpy(g5["x"])
    with torch.no_grad():
        lg = m(x.cuda())
    _accuracy(ref, lg, x, m.inference_plan(x.shape[0], x.shape[3]), "golden g5")
    ref2, m2, x2 = _nets(sed, 2)
    m2.set_inference_precision("bf16")
    with torch.no_grad():
        lg2 = m2(x2.cuda())
    _accuracy(ref2, lg2, x2, m2.inference_plan(x2.shape[0], x2.shape[3]), "config 2")


def test_nothing_else_moves(sed):
    from oracle import crnn_ref
    ref, m, x = _nets(sed, 2)
    xg = x[:64].cuda()
    never = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
    never.load_state_dict(ref.state_dict())
    never.cuda().eval()
    with torch.no_grad():
        want = never(xg)
        m.set_inference_precision("bf16")
        lb = m(xg)
        lb2 = m(xg)
        chunks = torch.cat([m(xg[i:i + 32]) for i in range(0, 64, 32)])
        m.set_inference_precision("f32")
        back = m(xg)
    assert torch.equal(lb, lb2), "two bf16 runs differ"
    assert torch.equal(lb, chunks), "the batch differs from its 32-sample chunks"
    assert torch.equal(back, want), "f32 after bf16 differs from a model never switched"
    assert not torch.equal(lb, want)
    # a training step with bf16 set equals one without it, bit for bit
    outs = []
    for prec in ("f32", "bf16"):
        torch.manual_seed(5)
        t = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
        t.load_state_dict(ref.state_dict())
        t.cuda().train().set_inference_precision(prec)
        opt = sed.FusedAdam(t.parameters(), lr=1e-3)
        y = (torch.rand(16, 32, 1, generator=torch.Generator().manual_seed(1)) > 0.8).float().cuda()
        opt.zero_grad()
        lg = t(x[:16].cuda())
        loss = sed.BCEWithLogitsLoss()(lg, y)
        loss.backward()
        grads = [p.grad.clone() for p in t.parameters()]
        opt.step()
        torch.cuda.synchronize()
        outs.append((loss.item(), grads, [p.detach().clone() for p in t.parameters()]))
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert all(torch.equal(a, b) for a, b in zip(outs[0][2], outs[1][2]))


def test_unsupported_blocks_stay_fp32_and_long_sequences_run(sed):
    from oracle import crnn_ref
    lref = crnn_ref.LightningNetRef()
    lref.load_state_dict(crnn_ref.rs_state_dict(lref, 11))
    lref.eval()
    lm = sed.LightningTimePooledCRNN()
    lm.load_state_dict(lref.state_dict())
    lm.cuda().eval()
    x = torch.randn(4, 1, 40, 64, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a = lm(x.cuda())
        lm.set_inference_precision("bf16")
        assert lm.inference_plan(4, 64) == {"conv": ["f32"] * 3, "proj": "f32"}
        b = lm(x.cuda())
    assert torch.equal(a, b)                      # nothing qualifies: the bf16 setting runs the fp32 plan itself
    _, want = emu.forward(lref, x, lm.inference_plan(4, 64))
    assert (b.cpu().double() - want).abs().max().item() < 1e-3
    # one long sequence (B = 1, T = 2048) through the bf16 plan
    ref, m, _ = _nets(sed, 2)
    m.set_inference_precision("bf16")
    xl = torch.randn(1, 1, 40, 2048, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        lg = m(xl.cuda())
    torch.cuda.synchronize()
    assert lg.shape == (1, 256, 1) and torch.isfinite(lg).all()
    _, want = emu.forward(ref, xl, m.inference_plan(1, 2048))
    d = (torch.sigmoid(lg.cpu().double()) - torch.sigmoid(want)).abs().max().item()
    print(f"B=1 T=2048: HIP bf16 vs emulation max |dp| {d:.2e}")
    assert d < 2e-2
