"""The float64 restatements of tests/small_passes_ref.py held against independent yardsticks, without a GPU: the BatchNorm /
ReLU / pool / dropout block against torch float64 autograd, Adam against torch.optim.Adam, the losses against autograd, the
dropout hash against its own contract, and the near-tie repair's cap at every shape the GPU tests run."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_passes_ref as R  # noqa: E402

BLOCK_CASES = [  # B, T, F, C, pf, pt, p
    (2, 8, 6, 4, 1, 2, 0.0), (2, 9, 6, 4, 1, 2, 0.3), (1, 4, 11, 8, 5, 1, 0.3), (2, 5, 7, 4, 2, 2, 0.0), (2, 7, 8, 4, 3, 2, 0.3),
    (3, 6, 4, 12, 2, 2, 0.3)]


@pytest.mark.parametrize("B,T,Fm,C,pf,pt,p", BLOCK_CASES)
def test_block_forward_and_backward_match_float64_autograd(B, T, Fm, C, pf, pt, p):
    """batch_norm(training) -> relu -> max_pool2d -> * keep / (1 - p) in float64 autograd against bn_block_fwd / bn_block_bwd fed
    the unrounded float64 statistics: outputs, dy, sum g (= dbeta), sum g xhat (= dgamma), sum dy to 1e-12; ragged T and F are
    dropped by the pool and still receive the statistics terms."""
    rng = np.random.default_rng([B, T, Fm, C, pf, pt])
    y = rng.standard_normal((B, T, Fm, C)) * 1.5 + 0.3
    gamma, beta = rng.random(C) + 0.5, rng.standard_normal(C) * 0.3
    Tp, Fp = T // pt, Fm // pf
    dout = rng.standard_normal((B, Tp, Fp, C))
    keep = R.keep_for((B, Tp, Fp, C), 77, p)
    eps = 1e-5
    flat = y.reshape(-1, C)
    mean = flat.mean(0)
    rstd = 1.0 / np.sqrt(flat.var(0) + eps)
    scale = gamma * rstd
    shift = beta - mean * scale

    x = torch.tensor(y.transpose(0, 3, 2, 1).copy(), requires_grad=True)            # [B,C,F,T]: H = F, W = T
    w, b = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    o = F.max_pool2d(F.relu(F.batch_norm(x, None, None, w, b, True, 0.1, eps)), (pf, pt))
    o = o * torch.tensor(keep.transpose(0, 3, 2, 1) / (1.0 - float(np.float32(p))))
    (o * torch.tensor(dout.transpose(0, 3, 2, 1).copy())).sum().backward()

    fwd = R.bn_block_fwd(y, scale, shift, pf, pt, keep, p)
    bwd = R.bn_block_bwd(y, dout, scale, shift, mean, rstd, pf, pt, keep, B * T * Fm, p)
    np.testing.assert_allclose(fwd["out"], o.detach().numpy().transpose(0, 3, 2, 1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(bwd["dy"], x.grad.numpy().transpose(0, 3, 2, 1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(bwd["sum_g"], b.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(bwd["sum_gx"], w.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(bwd["sum_dy"], x.grad.numpy().sum((0, 2, 3)), rtol=0, atol=1e-12)
    assert int(fwd["route"].max()) == pf * pt and ((fwd["route"] == 0).any() or pf * pt > 2)   # closed gates are rare in large windows
    if T % pt or Fm % pf:                                                           # tail positions: statistics terms only
        tail = np.ones((T, Fm), bool)
        tail[:Tp * pt, :Fp * pf] = False
        want = scale * (-bwd["sum_g"] / (B * T * Fm) - (y - mean) * rstd * bwd["sum_gx"] / (B * T * Fm))
        np.testing.assert_allclose(bwd["dy"][:, tail], want[:, tail], rtol=0, atol=1e-15)


def test_pooled_identity_gives_the_sums_of_the_block_backward():
    """pooled_sums (gate q > 0, xhat from q) against bn_block_bwd (arg-max search, xhat from y) where both are exact in
    float64: the unrounded pooled output of the block itself; a gamma == 0 channel of either sign and a small gamma included"""
    rng = np.random.default_rng(5)
    B, T, Fm, C, pf, pt, p = 2, 6, 8, 8, 2, 2, 0.3
    y = rng.standard_normal((B, T, Fm, C)) * 1.5 + 0.3
    gamma, beta = rng.random(C) + 0.5, rng.standard_normal(C) * 0.3
    gamma[1], beta[1] = 0.0, 0.5
    gamma[2], beta[2] = 0.0, -0.2
    gamma[3], beta[3] = 1e-5, 0.6
    gamma[4] = -0.7
    flat = y.reshape(-1, C)
    mean, rstd = flat.mean(0), 1.0 / np.sqrt(flat.var(0) + 1e-5)
    scale = gamma * rstd
    shift = beta - mean * scale
    keep = R.keep_for((B, T // pt, Fm // pf, C), 3, p)
    dout = rng.standard_normal(keep.shape)
    q = R.bn_block_fwd(y, scale, shift, pf, pt, keep, p)["out"]
    bwd = R.bn_block_bwd(y, dout, scale, shift, mean, rstd, pf, pt, keep, B * T * Fm, p)
    ps = R.pooled_sums(q.transpose(0, 1, 3, 2), dout.transpose(0, 1, 3, 2), gamma, beta, y, mean, rstd, scale, shift, pf, pt, p)
    assert list(np.flatnonzero(R.slow_channels(gamma, beta))) == [1, 3]
    np.testing.assert_allclose(ps["sum_g"], bwd["sum_g"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ps["sum_gx"], bwd["sum_gx"], rtol=0, atol=1e-9)          # (z - beta) / gamma loses digits in float64 too
    assert ps["sum_g"][2] == 0.0 and ps["sum_gx"][2] == 0.0 and ps["sum_gx"][1] != 0.0


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 0.37)])
def test_adam_reference_matches_torch_optim_adam(wd, gs):
    rng = np.random.default_rng(11)
    p0, lr, b1, b2, eps = rng.standard_normal(257), 1e-3, 0.9, 0.999, 1e-8
    f32 = lambda a: float(np.float32(a))                                            # noqa: E731  (the reference rounds its scalars to fp32)
    tp = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=f32(lr), betas=(f32(b1), f32(b2)), eps=f32(eps), weight_decay=f32(wd))
    p, m, v = p0.copy(), np.zeros(257), np.zeros(257)
    for t in (1, 2, 3):
        g = rng.standard_normal(257)
        tp.grad = torch.tensor(g * f32(gs))
        opt.step()
        p, m, v = R.adam_step(p, g, m, v, lr, b1, b2, eps, wd, t, gs)
        st = opt.state[tp]
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=0, atol=1e-13)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=0, atol=1e-14)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=0, atol=1e-14)


@pytest.mark.parametrize("mean", [True, False])
def test_loss_references_match_float64_autograd(mean):
    rng = np.random.default_rng(13)
    x0 = np.concatenate([rng.standard_normal(61) * 3, [0.0, 8.0, -8.0]])
    t0 = (rng.random(64) < 0.4).astype(np.float64)
    red = "mean" if mean else "sum"
    x = torch.tensor(x0, requires_grad=True)
    l = F.binary_cross_entropy_with_logits(x, torch.tensor(t0), reduction=red)
    l.backward()
    loss, dx, pr = R.bce_with_logits(x0, t0, mean)
    assert abs(loss - l.item()) < 1e-12 * max(1.0, abs(l.item()))
    np.testing.assert_allclose(dx, x.grad.numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(pr, torch.sigmoid(x).detach().numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.sigmoid(np.array([-800.0, 0.0, 800.0])), [0.0, 0.5, 1.0], rtol=0, atol=0)
    for gamma in (1.0, 2.0, 3.0):
        for alpha in (0.25, 1.0):
            x = torch.tensor(x0, requires_grad=True)
            pt_ = torch.where(torch.tensor(t0) == 1, torch.sigmoid(x), 1 - torch.sigmoid(x))
            li = -float(np.float32(alpha)) * (1 - pt_) ** gamma * torch.log(pt_ + float(np.float32(1e-12)))
            l = li.mean() if mean else li.sum()
            l.backward()
            loss, dx, _ = R.focal_loss(x0, t0, alpha, gamma, mean)
            assert abs(loss - l.item()) < 1e-12 * max(1.0, abs(l.item()))
            np.testing.assert_allclose(dx, x.grad.numpy(), rtol=0, atol=1e-12)


def test_norm_and_clip_reference():
    g = np.array([3.0, 4.0])
    assert R.norm_and_clip(g, 0.0) == (5.0, 1.0) and R.norm_and_clip(g, 10.0) == (5.0, 1.0)
    assert abs(R.norm_and_clip(g, 2.5)[1] - 2.5 / (5.0 + float(np.float32(1e-6)))) < 1e-16


def test_keep_mask_is_a_deterministic_seeded_hash_with_the_right_keep_fraction():
    idx = np.arange(10 ** 6, dtype=np.uint64)
    for p in (0.3, 0.5):
        a = R.keep_mask(1234, idx, p)
        assert np.array_equal(a, R.keep_mask(1234, idx, p))
        assert not np.array_equal(a, R.keep_mask(1235, idx, p))
        assert not np.array_equal(a, R.keep_mask(1234 + (1 << 32), idx, p))         # the seed's high word takes part
        sigma = np.sqrt(p * (1 - p) / idx.size)
        assert abs(a.mean() - (1 - p)) < 4 * sigma, (p, a.mean())
    # idx >= 2^32: the high word of the index changes the draw, and the fraction still holds
    hi = idx + np.uint64(1 << 32)
    b = R.keep_mask(1234, hi, 0.5)
    assert not np.array_equal(b, R.keep_mask(1234, idx, 0.5)) and abs(b.mean() - 0.5) < 4 * np.sqrt(0.25 / idx.size)
    assert not np.array_equal(b, R.keep_mask(1234, idx + np.uint64(2 << 32), 0.5))
    # the device step state's salt: seed + salt * GOLD mod 2^64, salt 0 = no salt
    assert R.salted_seed(7, 0) == 7 and R.salted_seed(7, 3) == (7 + 3 * 0x9E3779B97F4A7C15) % (1 << 64)
    assert R.salted_seed((1 << 64) - 1, 1) == 0x9E3779B97F4A7C15 - 1
    assert np.array_equal(R.keep_mask(7, idx, 0.5, salt=3), R.keep_mask(R.salted_seed(7, 3), idx, 0.5))
    assert not np.array_equal(R.keep_mask(7, idx, 0.5, salt=3), R.keep_mask(7, idx, 0.5))
    u = R.uniform(99, idx)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u * 16777216.0, np.floor(u * 16777216.0))


def test_fmix32_is_the_murmur3_finaliser():
    # published test values of MurmurHash3's fmix32
    assert [int(v) for v in R.fmix32(np.array([0, 1, 0xFFFFFFFF], np.uint32))] == [0, 0x514E28B7, 0x81F16F39]


@pytest.mark.parametrize("shape", R.BLOCK_SHAPES + R.B6_POOLED, ids=lambda s: "x".join(map(str, s)))
def test_near_tie_repair_touches_at_most_a_thousandth_of_the_windows(shape):
    """every shape the GPU tests run: after the repair no window decision is within 1e-4 (1 + |z_max|) of flipping, and the
    repaired share stays under the cap, so the data is still what it was drawn as"""
    pooled = shape in R.B6_POOLED
    d = R.block_inputs(shape, pooled)
    assert d["share"] <= R.REPAIR_CAP, d["share"]
    look = None
    if pooled:
        look = np.ones(shape[3], bool)
        look[[c for c, _ in R.pooled_special_channels(shape[3])]] = False
    bad, _ = R.near_ties(d["y"], d["scale"], d["shift"], shape[4], shape[5], look)
    assert not bad.any()
    if pooled:                                                       # the planted channels: window elements at least 2^-4 apart
        for c, _ in R.pooled_special_channels(shape[3]):
            w = R._windows(d["y"][..., c:c + 1].astype(np.float64), shape[4], shape[5])
            assert np.abs(w[:, :, :, 0] - w[:, :, :, 1]).min() >= 0.0625


def test_repair_moves_a_planted_tie_and_a_planted_zero():
    y = np.zeros((1, 2, 2, 4), np.float32)
    y[0, :, :, 0] = [[1.0, 2.0], [1.0, 3.0]]                          # pool (1,2): windows over t; equal winners at f = 0
    y[0, :, :, 1] = [[-1.0, 0.5], [-2.0, 1.0]]                        # margins fine
    y[0, :, :, 2] = [[0.0, -5.0], [-1.0, -6.0]]                       # z_max == 0 at f = 0
    y[0, :, :, 3] = [[1.0, 1.0], [1.0, 1.0]]                          # ties under a negative scale
    scale, shift = np.array([1, 1, 1, -1], np.float32), np.zeros(4, np.float32)
    out, share = R.repair_near_ties(y, scale, shift, 1, 2)
    assert share == 4 / 8
    assert out[0, 0, 0, 0] == 1.0625 and out[0, 1, 0, 0] == 1.0 and out[0, 0, 0, 2] == 0.0625
    assert out[0, 0, 0, 3] == 0.9375 and out[0, 0, 1, 3] == 0.9375
    assert np.array_equal(out[..., 1], y[..., 1])
