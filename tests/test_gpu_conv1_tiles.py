"""The recomputed first conv block (csrc/conv1.hip: conv -> BatchNorm -> ReLU -> max-pool -> dropout with the convolution
recomputed in every pass) on every path its launchers can take, through the C ABI, against torch float64 on the CPU.

The rows come from conv1_cases.py (test_cpu_conv1_plan.py proves that each is in the regime it claims): workgroups that walk two
or three tiles and cross into the next sequence, ragged mel groups and ragged time tiles on the matrix-core kernels, both rgrad
kernels for 3 and 4 input channels, 4 and 512 output channels, the generic window loop.  Per row:
  a. the fp64 moment vector (S1 and the upper triangle of G) of sed_conv1_stats against float64 sums of the shifted inputs, every
     entry within n_serial * 2^-23 * sum |terms|; the statistics row against float64 sums at the bounds of
     test_conv1_stats_from_input_moments_vs_float64_sums
  b. the pooled output against float64 (atol 3e-5, rtol 1e-4), the arg-max bits against the float64 decision away from near-ties
     (at most 0.1 % left out), every element written; the walking batch bit for bit what each sequence gives alone
  c. the partial rows (sum g~, R_k) of sed_conv1_bwd_wgrad: rows [0, grid) finite, nothing behind them written, their float64
     column sums against float64 sums formed from the DEVICE's pooled output and bits — the test that isolates both rgrad kernels
  d. dW, dbias, dgamma, dbeta of the moments path, and of the recomputing passes for one and two input channels, against float64
     autograd with a gamma == 0 / beta > 0 channel and dropout 0.5, at the tolerances of
     test_conv1_backward_from_pooled_output_bits_and_moments_vs_float64
  e. the routing codes of the two rows with another pool against the float64 window arg-max.
A failure names the worst element with the tile, workgroup and visit that wrote it."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv1_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1024
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


def g(t):
    return t.cuda().contiguous()


def _guarded(shape, dtype, fill):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf, fill, what):
    edge = torch.cat([buf[:GUARD], buf[-GUARD:]])
    ok = torch.isnan(edge).all() if fill != fill else (edge == fill).all()
    assert bool(ok), f"{what}: written outside the buffer"


class Dev:
    """a row's inputs on the device, its batch statistics (sed_conv1_stats with gram_out, workspace NaN-filled) and the BatchNorm
    scale / shift they give"""

    def __init__(self, ops, name, zero_gamma):
        from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
        self.c = cc.case(name)
        self.name = name
        B, Cin, Fm, T, C = self.c["shape"]
        self.host = cc.inputs(name, zero_gamma)
        self.x, self.bias, self.gamma, self.beta = (g(self.host[k]) for k in ("x", "bias", "gamma", "beta"))
        self.wf, _ = ops.conv3x3_pack(g(self.host["w"]))
        L = lib()
        self.stat = torch.full((1, 2, C), NAN, device="cuda")
        nws = L.sed_conv1_stats_workspace_bytes(B, Cin, T) // 4
        wbuf, ws = _guarded((nws,), torch.float32, NAN)
        self.mom = torch.full((L.sed_conv1_moments_doubles(Cin),), NAN, dtype=torch.float64, device="cuda")
        check(L.sed_conv1_stats(ptr(self.x), ptr(self.wf), ptr(self.bias), ptr(self.stat), ptr(ws), B, Cin, Fm, T, C, ptr(self.mom), stream_ptr()),
              "conv1_stats")
        torch.cuda.synchronize()
        _guards_intact(wbuf, NAN, f"{name} conv1_stats workspace")
        self.mean, self.rstd, self.scale, self.shift = ops.bn_finalize_train(self.stat, B * T * Fm, self.gamma, self.beta,
                                                                             torch.zeros(C).cuda(), torch.ones(C).cuda(), eps=cc.EPS)


@functools.lru_cache(maxsize=None)
def _dev(ops, name, zero_gamma=False):
    return Dev(ops, name, zero_gamma)


def _forward(d, drop, x=None, scale=None, shift=None, want_bits=True):
    """sed_conv1_bn_relu_pool_drop_fwd into a NaN-filled, guarded output (and 0xFF-filled bit bytes for the (1,2) pool) -> (pooled, bits)"""
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    _, Cin, Fm, T, C = d.c["shape"]
    pf, pt = d.c["pool"]
    x = d.x if x is None else x
    B = x.shape[0]
    obuf, out = _guarded((B, T // pt, Fm // pf, C), torch.float32, NAN)
    bbuf = bits = None
    if want_bits and (pf, pt) == (1, 2):
        bbuf, bits = _guarded((out.numel() // 4,), torch.uint8, 0xFF)
    check(lib().sed_conv1_bn_relu_pool_drop_fwd(ptr(x), ptr(d.wf), ptr(d.bias), ptr(d.scale if scale is None else scale),
                                                ptr(d.shift if shift is None else shift), ptr(out), B, Cin, Fm, T, C, pf, pt, drop, cc.SEED, None,
                                                ptr(bits), stream_ptr()), "conv1_fwd")
    torch.cuda.synchronize()
    _guards_intact(obuf, NAN, f"{d.name} pooled output")
    if bits is not None:
        _guards_intact(bbuf, 0xFF, f"{d.name} arg-max bits")
    return out, bits


def _sel(bits, shape):
    """bit k of a quad's byte = channel 4 cg + k -> [B][T'][F][C] of 0 / 1"""
    return torch.stack([(bits >> k) & 1 for k in range(4)], -1).reshape(shape)


def _within(got, ref, atol, rtol):
    """-> the excess over atol + rtol |ref| (0 where within; NaN stays NaN)"""
    return ((got.double() - ref).abs() - (atol + rtol * ref.abs())).clamp_min(0)


# ───────────────────────── a. moments ─────────────────────────
@pytest.mark.parametrize("name", cc.NAMES)
def test_moments_and_statistics_row_vs_float64_sums(ops, name):
    d = _dev(ops, name)
    B, Cin, Fm, T, C = d.c["shape"]
    ref, mag = cc.ref_moments(d.host["x"])
    got = d.mom.cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: moment vector not fully written"
    n = cc.n_serial_moments(B, Cin, Fm, T)
    bound = n * 2.0 ** -23 * mag
    err = (got - ref).abs()
    i = int((err / bound).argmax())
    print(f"{name}: moments n_serial {n}, worst error {float(err[i]):.3e} = {float(err[i] / bound[i]):.3f} of its bound {float(bound[i]):.3e} "
          f"(entry {i} of {ref.numel()}, {float(err[i] / mag[i]):.2e} of sum |terms|)")
    assert bool((err <= bound).all()), f"{name}: moment entry {i} (S1 for i < {9 * Cin}, then G row by row) off by {float(err[i]):.3e}, bound {float(bound[i]):.3e}"
    r = cc.ref_forward(name)
    mean, rstd = d.mean.cpu().double(), d.rstd.cpu().double()
    e_m = float(((mean - r["mean"]).abs() / r["q"].sqrt()).max())
    e_v = float(((1.0 / rstd ** 2 - cc.EPS - r["var"]).abs() / r["q"]).max())
    e_r = float((rstd * (r["var"] + cc.EPS).sqrt() - 1.0).abs().max())
    print(f"{name}: mean err / rms {e_m:.1e}, var err / E[y^2] {e_v:.1e}, rstd rel err {e_r:.1e}")
    assert e_m <= 1e-6 and e_v <= 1e-5 and e_r <= 1e-4


# ───────────────────────── b. forward, bits, walk invariance ─────────────────────────
@pytest.mark.parametrize("name", cc.NAMES)
def test_pooled_output_and_argmax_bits_vs_float64(ops, name):
    d = _dev(ops, name)
    r = cc.ref_forward(name)
    out, bits = _forward(d, 0.0)
    out = out.cpu()
    assert not bool(torch.isnan(out).any()), cc.worst(d.c, torch.isnan(out).float(), "pooled elements never written")
    over = _within(out, r["pooled"], 3e-5, 1e-4)
    assert not bool((over > 0).any()), cc.worst(d.c, over, "pooled output beyond atol 3e-5, rtol 1e-4")
    if bits is None:
        return
    bits = bits.cpu()
    assert bool((bits < 16).all()), f"{name}: {int((bits >= 16).sum())} bit bytes never written"
    sel = _sel(bits, out.shape).bool()
    share = float(r["near"].double().mean())
    wrong = (sel != r["bit"]) & ~r["near"]
    print(f"{name}: near-tie share {share:.2e} (cap {cc.TIE_CAP:.0e}), bits off inside the near-ties {int(((sel != r['bit']) & r['near']).sum())}")
    assert share <= cc.TIE_CAP
    assert not bool(wrong.any()), cc.worst(d.c, wrong.float(), "arg-max bits against the float64 decision")


@pytest.mark.parametrize("name", cc.NAMES)
def test_walking_batch_equals_every_sequence_alone(ops, name):
    """fixed scale and shift, no dropout: sequence b of the batch (tiles b * tblocks .., spread over the visits of many workgroups) bit
    for bit the run of that sequence as a batch of one, which has fewer tiles than workgroups"""
    d = _dev(ops, name)
    B = d.c["shape"][0]
    out, bits = _forward(d, 0.0)
    for b in range(B):
        o1, b1 = _forward(d, 0.0, x=d.x[b:b + 1].contiguous())
        diff = (out[b:b + 1].view(torch.int32) != o1.view(torch.int32)).cpu()
        if bool(diff.any()):
            full = torch.zeros(out.shape)
            full[b] = diff[0].float()
            raise AssertionError(cc.worst(d.c, full, f"sequence {b} in the batch differs from the sequence alone"))
        if bits is not None:
            assert torch.equal(bits.view(B, -1)[b], b1), f"{name}: arg-max bits of sequence {b} differ from the sequence alone"


# ───────────────────────── c. the partial rows of the rgrad kernels ─────────────────────────
@pytest.mark.parametrize("drop", cc.DROPS)
@pytest.mark.parametrize("name", cc.P12_NAMES)
def test_rgrad_partial_rows_sum_to_float64_sums_over_the_devices_own_decisions(ops, name, drop):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    d = _dev(ops, name)
    B, Cin, Fm, T, C = d.c["shape"]
    L = lib()
    NK, NV = 9 * Cin, 1 + 9 * Cin
    plan = cc.rgrad_plan(B, Cin, Fm, T, C)
    out, bits = _forward(d, drop)
    dout = cc.dout_of(name)
    dg = g(dout)
    rows = L.sed_conv1_bwd_wgrad_workspace_bytes(B, Cin, T, C) // (4 * NV * C)
    assert rows == cc.fused_rows(B, T) >= plan["grid"]
    wbuf, ws = _guarded((rows, C, NV), torch.float32, NAN)
    dw, db, sum_g = torch.empty(C, Cin, 3, 3).cuda(), torch.empty(C).cuda(), torch.zeros(C).cuda()
    check(L.sed_conv1_bwd_wgrad(ptr(d.x), ptr(dg), ptr(out), ptr(bits), ptr(d.mom), ptr(d.wf), ptr(d.bias), ptr(d.mean), ptr(d.rstd), ptr(d.scale),
                                ptr(sum_g), None, ptr(dw), ptr(db), ptr(ws), B, Cin, Fm, T, C, drop, None, None, None, stream_ptr()),
          "conv1_bwd_wgrad")
    torch.cuda.synchronize()
    _guards_intact(wbuf, NAN, f"{name} rgrad workspace")
    part = ws.cpu()
    fin = torch.isfinite(part[:plan["grid"]])
    assert bool(fin.all()), (f"{name}: {int((~fin).sum())} values of the {plan['grid']} partial rows not written; first in row (workgroup) "
                             f"{int((~fin).flatten(1).any(1).nonzero()[0])}")
    assert bool(torch.isnan(part[plan["grid"]:]).all()), f"{name}: partial rows behind the grid of {plan['grid']} were written"
    got = part[:plan["grid"]].double().sum(0)                                             # [C][NV]
    # float64 sums from the device's pooled output and bits: g~ = dout / (1-p) where the pooled output is > 0, routed to the arg-max row
    pv, sel = out.cpu(), _sel(bits.cpu(), out.shape)
    inv_keep = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(drop, dtype=torch.float32)))
    gt = torch.where(pv > 0, dout.double() * inv_keep, torch.zeros((), dtype=torch.float64))
    V = cc.taps(d.host["x"])                                                              # [B][NK][F][T]
    want = torch.empty(C, NV, dtype=torch.float64)
    mag = torch.empty(C, NV, dtype=torch.float64)
    want[:, 0], mag[:, 0] = gt.sum((0, 1, 2)), gt.abs().sum((0, 1, 2))
    R = torch.zeros(NK, C, dtype=torch.float64)
    M = torch.zeros(NK, C, dtype=torch.float64)
    for row in (0, 1):
        v = V[..., row::2].permute(0, 3, 2, 1).reshape(-1, NK)                            # [B T' F][NK]: the window's row `row`
        gr = (gt * (sel == row)).reshape(-1, C)
        R += v.T @ gr
        M += v.abs().T @ gr.abs()
    want[:, 1:], mag[:, 1:] = R.T, M.T
    n = cc.n_serial_rgrad(B, Cin, Fm, T, C)
    bound = n * 2.0 ** -23 * mag
    err = (got - want).abs()
    i = int((err / bound.clamp_min(1e-300)).argmax())
    ch, v = divmod(i, NV)
    print(f"{name} p={drop}: {plan['kernel']} rgrad, {plan['grid']} rows, n_serial {n}, worst R_k error {float(err[ch, v]):.3e} = "
          f"{float(err[ch, v] / bound[ch, v]):.3f} of its bound {float(bound[ch, v]):.3e} (channel {ch}, value {v}: 0 = sum g~, 1 + k = R_k)")
    assert bool((err <= bound).all()), (f"{name}: {int((err > bound).sum())} of {err.numel()} column sums beyond their bound; worst channel {ch} value {v}: "
                                        f"got {float(got[ch, v])!r}, want {float(want[ch, v])!r}")
    assert float((pv > 0).float().mean()) > 0.1 and 0.3 < float(sel.float().mean()) < 0.7


# ───────────────────────── d. gradients ─────────────────────────
def _ref_grads(d, mask, dout):
    """float64 autograd of conv -> BatchNorm(train) -> ReLU -> MaxPool -> the kernel's own dropout mask -> (pooled, dW, dbias, dgamma, dbeta)"""
    pf, pt = d.c["pool"]
    h = d.host
    w, b, ga, be = (h[k].double().requires_grad_(True) for k in ("w", "bias", "gamma", "beta"))
    y = F.conv2d(h["x"].double(), w, b, padding=1)
    z = F.batch_norm(y, None, None, ga, be, training=True, eps=cc.EPS)
    o = F.max_pool2d(torch.relu(z), (pf, pt)).permute(0, 3, 2, 1) * mask.double()
    o.backward(dout.double())
    return o.detach(), w.grad, b.grad, ga.grad, be.grad


def _assert_grads(d, what, got, ref):
    dw, db, dgamma, dbeta = (t.cpu() for t in got)
    rw, _, rg, rb = ref
    wmax = float(rw.abs().max())
    for nm, a, r in (("dW", dw, rw), ("dgamma", dgamma, rg), ("dbeta", dbeta, rb)):
        over = _within(a, r, 2e-5 * float(r.abs().max()) + 1e-6, 2e-4)
        i = int(torch.nan_to_num(over, nan=float("inf")).argmax())
        print(f"{d.name} {what} {nm}: max |err| {float((a.double() - r).abs().max()):.3e}, max |ref| {float(r.abs().max()):.3e}")
        assert not bool((torch.nan_to_num(over, nan=1.0) > 0).any()), (f"{d.name} {what}: {nm} beyond 2e-5 max|ref| + 1e-6, rtol 2e-4; worst flat index {i}: "
                                                                         f"got {float(a.flatten()[i])!r}, want {float(r.flatten()[i])!r}")
    assert float(db.abs().max()) < 1e-4 * max(1.0, wmax), f"{d.name} {what}: dbias {float(db.abs().max()):.3e} (analytically zero in front of BatchNorm)"


@pytest.mark.parametrize("name", cc.NAMES)
def test_gradients_vs_float64_autograd(ops, name):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    d = _dev(ops, name, True)
    B, Cin, Fm, T, C = d.c["shape"]
    pf, pt = d.c["pool"]
    L = lib()
    drop = 0.5
    out, bits = _forward(d, drop)
    # the kernel's own dropout mask: the same pass on scale 0, shift 1 (every pooled element 1 before the mask)
    mask, _ = _forward(d, drop, scale=torch.zeros(C).cuda(), shift=torch.ones(C).cuda(), want_bits=False)
    mask = mask.cpu()
    assert set(mask.unique().tolist()) == {0.0, 2.0}
    dout = cc.dout_of(name)
    dg = g(dout)
    o, *ref = _ref_grads(d, mask, dout)
    over = _within(out.cpu(), o, 3e-5, 1e-4)
    assert not bool((torch.nan_to_num(over, nan=1.0) > 0).any()), cc.worst(d.c, over, "pooled output (dropout 0.5) beyond atol 3e-5, rtol 1e-4")
    assert float(d.host["gamma"][1]) == 0.0 and float(d.host["beta"][1]) > 0
    sum_g, sum_gx, dgamma, dbeta = (torch.full((C,), NAN).cuda() for _ in range(4))
    if Cin <= 2:
        rows = L.sed_conv1_fused_rows(B, T)
        part = torch.full((rows, 2, C), NAN).cuda()
        check(L.sed_conv1_bwd_reduce(ptr(d.x), ptr(d.wf), ptr(d.bias), ptr(dg), ptr(d.scale), ptr(d.shift), ptr(d.mean), ptr(d.rstd), ptr(part),
                                     B, Cin, Fm, T, C, pf, pt, drop, cc.SEED, None, stream_ptr()), "conv1_bwd_reduce")
        check(L.sed_bn_bwd_finalize(ptr(part), rows, C, ptr(sum_g), ptr(sum_gx), ptr(dgamma), ptr(dbeta), stream_ptr()), "bn_bwd_finalize")
        assert bool(torch.isfinite(part).all())
    else:                                          # no recomputing reduce pass beyond two input channels: the two sums from the reference
        dgamma, dbeta = g(ref[2].float()), g(ref[3].float())
        sum_g, sum_gx = dbeta.clone(), dgamma.clone()
    if (pf, pt) == (1, 2):
        dw, db = torch.full((C, Cin, 3, 3), NAN).cuda(), torch.full((C,), NAN).cuda()
        dgam = dgamma.clone()
        dgam[1] = NAN                                  # the gamma == 0 channel: dgamma is this pass's own (the rest stays what it was given)
        ws = torch.full((L.sed_conv1_bwd_wgrad_workspace_bytes(B, Cin, T, C) // 4,), NAN).cuda()
        check(L.sed_conv1_bwd_wgrad(ptr(d.x), ptr(dg), ptr(out), ptr(bits), ptr(d.mom), ptr(d.wf), ptr(d.bias), ptr(d.mean), ptr(d.rstd), ptr(d.scale),
                                    ptr(sum_g), ptr(sum_gx), ptr(dw), ptr(db), ptr(ws), B, Cin, Fm, T, C, drop, ptr(d.gamma), ptr(d.beta), ptr(dgam),
                                    stream_ptr()), "conv1_bwd_wgrad")
        _assert_grads(d, "moments path", (dw, db, dgam, dbeta), ref)
    if Cin <= 2:
        dw, db = torch.full((C, Cin, 3, 3), NAN).cuda(), torch.full((C,), NAN).cuda()
        dgam = dgamma.clone()
        dgam[1] = NAN                                  # the gamma == 0 channel: dgamma is this pass's own (the rest stays what it was given)
        ws = torch.full((L.sed_conv1_bwd_apply_workspace_bytes(B, Cin, T, C) // 4,), NAN).cuda()
        check(L.sed_conv1_bwd_apply_wgrad(ptr(d.x), ptr(d.wf), ptr(d.bias), ptr(dg), ptr(d.scale), ptr(d.shift), ptr(d.mean), ptr(d.rstd), ptr(sum_g),
                                          ptr(sum_gx), ptr(dw), ptr(db), ptr(ws), B, Cin, Fm, T, C, pf, pt, drop, cc.SEED, None, ptr(d.gamma), ptr(d.beta),
                                          ptr(dgam), stream_ptr()), "conv1_bwd_apply_wgrad")
        assert bool(torch.isfinite(ws).all())
        _assert_grads(d, "recompute path", (dw, db, dgam, dbeta), ref)


# ───────────────────────── e. routing ─────────────────────────
@pytest.mark.parametrize("name", cc.POOL_NAMES)
def test_routing_codes_vs_float64_window_argmax(ops, name):
    from sed_crnn_amd._lib import check, lib, ptr, stream_ptr
    d = _dev(ops, name)
    B, Cin, Fm, T, C = d.c["shape"]
    pf, pt = d.c["pool"]
    r = cc.ref_forward(name)
    rbuf, route = _guarded((B, T // pt, Fm // pf, C), torch.uint8, 0xFF)
    check(lib().sed_conv1_route(ptr(d.x), ptr(d.wf), ptr(d.bias), ptr(d.scale), ptr(d.shift), ptr(route), B, Cin, Fm, T, C, pf, pt, stream_ptr()), "conv1_route")
    torch.cuda.synchronize()
    _guards_intact(rbuf, 0xFF, f"{name} routing codes")
    route = route.cpu()
    assert bool((route <= pf * pt).all()), cc.worst(d.c, (route > pf * pt).float(), "routing codes never written")
    share = float(r["near"].double().mean())
    wrong = (route != r["code"]) & ~r["near"]
    print(f"{name}: near-tie share {share:.2e} (cap {cc.TIE_CAP:.0e}), codes off inside the near-ties {int(((route != r['code']) & r['near']).sum())}")
    assert share <= cc.TIE_CAP
    assert not bool(wrong.any()), cc.worst(d.c, wrong.float(), "routing codes against the float64 window arg-max")
