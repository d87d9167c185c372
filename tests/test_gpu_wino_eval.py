"""conv3x3_wino_k<.., EV> (csrc/wino.hip: the Winograd kernel with BatchNorm folded into the transformed weights and ReLU + the (1,2)
time pool in the epilogue — what every 128-channel conv block above the first runs in the eval forward) on every geometry it can
take, and the eval plan that packs and launches it.

The rows come from wino_cases.py (test_cpu_wino_geo.py proves that each is in the regime it claims and that the integer inputs
are exact in float32).  Every reference is torch in float64 on the CPU and shares nothing with the library.
  a. integers (x in [-2, 2], w in {-1, 0, 1}, power-of-two BatchNorm scales of both signs and 0, eps = 0): the fold and every sum
     behind it are exact, so the pooled output must EQUAL max_pool2d(relu(batch_norm(conv2d(x))), (1,2)).  The input is a view
     inside a NaN-filled allocation, the output starts as a payload NaN between guards; a dropped, doubled or misplaced tile, a
     halo column from the wrong group or a row written to the wrong sequence changes integers.  Every sequence is offset by its
     own level, as in test_gpu_wino_patch_dma.py: -1, 0 or 1 on top of {-1, 0, 1}, which stays inside the range of the bound;
     the real-valued inputs of c carry a quarter per sequence.
  b. workgroup order: a batch of 8 (XCD-aware order) gives, sequence by sequence, the bits a batch of 3 (plain order) gives, and a
     second call gives the same bits — on the integer and on the real-valued inputs; one batch of 16 (two sequences per XCD).
  c. N(0,1) inputs with non-trivial statistics at the tolerance test_inference_conv_with_folded_batchnorm_relu_and_pool_in_the_epilogue
     holds this epilogue to: atol 2e-5 * max(1, max |ref|), rtol 1e-5; the direct kernel's error beside it where it takes the shape.
  d. 64, 192 and 256 output channels (1, 3, 4 channel halves per tile block) on three rows, through a, b and c.
  e. a whole-recording sequence (T = 512: 80 blocks), one sequence, 64 channels.
  f. a shape the geometry refuses: refused by the row query, the Python entry and the C entry (host side, nothing launched), and the
     eval plan runs a block of that shape on another kernel, against float64.
  g. the plain forward (sed_conv3x3_wino_fwd) on the two rows with eight column groups, which no other test reaches.
  Then three networks in eval(): every block against the float64 block applied to the plan's own output of the block below, the
  GRU input projection (the re-ordered input weights, through their effect), the logits against the float64 oracle.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wino_cases as wc  # noqa: E402
from test_gpu_conv_tiles import NAN_BITS, _assert_guards, _guarded, cl, g  # noqa: E402
from test_gpu_wino_patch_dma import guarded, guards_intact  # noqa: E402

pytestmark = pytest.mark.gpu

CIN = wc.WN_CIN
BS = (wc.B_PLAIN, wc.B_XCD)
I32 = torch.int32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import ops as o
    return o


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def _pack(L, d, Cout):
    """sed_conv3x3_wino_pack_weights_bn_folded on w, bias, gamma, beta, running mean / variance and eps of d -> (uf, folded bias)"""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    uf = torch.empty(L.sed_conv3x3_wino_packed_floats(Cout, CIN), device="cuda")
    bf = torch.empty(Cout, device="cuda")
    args = [g(torch.as_tensor(d[k]).float()) for k in ("w", "bias", "gamma", "beta", "rm", "rv")]
    check(L.sed_conv3x3_wino_pack_weights_bn_folded(*[ptr(t) for t in args], float(d["eps"]), ptr(uf), ptr(bf), Cout, CIN, stream_ptr()), "pack")
    torch.cuda.synchronize()
    return uf, bf


def _eval(L, xv, uf, bf, Cout, what):
    """sed_conv3x3_wino_bn_relu_pool_eval on the channels-last view xv into a payload-NaN output between guards -> the output (CPU)"""
    from sed_crnn_amd._lib import check, ptr, stream_ptr
    B, T, Fm, _ = xv.shape
    obuf, out = _guarded(B, T // 2, Fm, Cout)
    check(L.sed_conv3x3_wino_bn_relu_pool_eval(ptr(xv), ptr(uf), ptr(bf), ptr(out), B, CIN, Fm, T, Cout, stream_ptr()), what)
    torch.cuda.synchronize()
    _assert_guards(obuf, what)
    return out.cpu()


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def _run_batches(L, x_cl, uf, bf, Cout, batches, what):
    """-> {B: output}; per batch: the input inside a NaN-filled allocation of its own, no NaN in the output, a second call the
    same bits; the sequences of the smaller batch bit for bit those of the larger (part b)"""
    outs = {}
    for B in batches:
        xv, big = guarded(x_cl[:B])
        out = _eval(L, xv, uf, bf, Cout, f"{what} B={B}")
        assert guards_intact(big, xv.numel()), f"{what} B={B}: the input or the NaN around it was written"
        assert not bool(torch.isnan(out).any()), f"{what} B={B}: {int(torch.isnan(out).sum())} output elements never written"
        assert _same_bits(out, _eval(L, xv, uf, bf, Cout, f"{what} B={B} again")), f"{what} B={B}: a second call gives other bits"
        outs[B] = out
    if len(batches) == 2:
        lo, hi = sorted(batches)
        assert _same_bits(outs[hi][:lo], outs[lo]), f"{what}: a sequence's output depends on the workgroup order\n" + \
            wc.first_difference(outs[hi][:lo].numpy(), outs[lo].numpy(), wc.wino_geo(lo, CIN, x_cl.shape[2], x_cl.shape[1], Cout))
    return outs


# ───────────────────────── a, b, d, e: integers, exact ─────────────────────────
def _exact(ops, name, Cout, batches):
    L = ops.lib()
    c = wc.case(name)
    Fm, T = c["F"], c["T"]
    d = wc.int_inputs(Fm, T, Cout, B=max(batches))
    ref = wc.ref_pooled(d)                                        # the largest batch, sliced for the smaller
    uf, bf = _pack(L, d, Cout)
    x_cl = cl(torch.from_numpy(d["x"]).float())
    for B in batches:
        geo = wc.wino_geo(B, CIN, Fm, T, Cout)
        assert tuple(geo[k] for k in wc.REGIME_KEYS) == c["claims"] and L.sed_conv3x3_wino_rows(B, CIN, Fm, T, Cout) == geo["rows"]
    outs = _run_batches(L, x_cl, uf, bf, Cout, batches, f"{name} Cout={Cout} integers")
    for B, out in outs.items():
        if not torch.equal(out.double(), ref[:B]):
            raise AssertionError(f"{name} Cout={Cout} B={B} ({'XCD-aware' if B % 8 == 0 else 'plain'} order): " +
                                 wc.first_difference(out.double().numpy(), ref[:B].numpy(), wc.wino_geo(B, CIN, Fm, T, Cout)))
    print(f"{name} Cout={Cout}: exact at B = {list(outs)}; {float((ref > 0).double().mean()):.2f} of the outputs positive, max {float(ref.max()):.0f}")


@pytest.mark.parametrize("name,Cout", wc.RUNS)
def test_pooled_output_equals_float64_on_integers(ops, name, Cout):
    _exact(ops, name, Cout, BS)


def test_long_sequence_equals_float64_on_integers(ops):
    _exact(ops, *wc.LONG, (1,))


def test_batch_of_16_walks_two_rounds_of_sequences_per_xcd(ops):
    """B = 16: launch index xcd + 8 j reaches sequence xcd + 8 (j / workgroups per sequence) with a quotient of 1 as well (B = 8
    only ever has 0) — on two column groups of two blocks and three channel halves, so every factor of the index is above 1"""
    _exact(ops, "same-F-two-groups", 192, (16,))


# ───────────────────────── b, c, d, e: real values ─────────────────────────
def real_inputs(Fm, T, Cout, B):
    """N(0,1) inputs, every sequence offset by its own level (a quarter per sequence: a value read from the neighbouring sequence
    is wrong by far more than the bound, and max |ref| — the tolerance — stays that of N(0,1) data); gamma in [0.5, 1.5] with
    channels at -0.8, 0 and 1e-3 in every 64-channel half, running variance log-uniform in [0.05, 20] with both ends present"""
    gen = torch.Generator().manual_seed(5000 + 100 * Fm + 10 * T + Cout)
    x = torch.randn(B, CIN, Fm, T, generator=gen) + 0.25 * torch.arange(1, B + 1, dtype=torch.float32).view(B, 1, 1, 1)
    w = torch.randn(Cout, CIN, 3, 3, generator=gen) / (3.0 * CIN ** 0.5)
    bias, beta, rm = (torch.randn(Cout, generator=gen) * 0.3 for _ in range(3))
    gamma = torch.rand(Cout, generator=gen) + 0.5
    rv = torch.exp(torch.rand(Cout, generator=gen) * float(np.log(20 / 0.05)) + float(np.log(0.05)))
    for h in range(Cout // 64):
        gamma[h * 64 + 1], gamma[h * 64 + 5], gamma[h * 64 + 9] = -0.8, 0.0, 1e-3
        rv[h * 64 + 2], rv[h * 64 + 3] = 0.05, 20.0
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, rm=rm, rv=rv, eps=1e-5)


def _over_bound(got, ref):
    """max of |got - ref| / (atol + rtol |ref|) with atol = 2e-5 * max(1, max |ref|), rtol = 1e-5; and max |got - ref|"""
    atol = 2e-5 * max(1.0, float(ref.abs().max()))
    err = (got.double() - ref).abs()
    return float((err / (atol + 1e-5 * ref.abs())).max()), float(err.max())


def _rounding(ops, name, Cout, batches):
    L = ops.lib()
    c = wc.case(name)
    Fm, T = c["F"], c["T"]
    d = real_inputs(Fm, T, Cout, max(batches))
    ref = wc.ref_pooled(d)
    uf, bf = _pack(L, d, Cout)
    x_cl = cl(d["x"])
    outs = _run_batches(L, x_cl, uf, bf, Cout, batches, f"{name} Cout={Cout} N(0,1)")
    fails = []
    for B, out in outs.items():
        r, e = _over_bound(out, ref[:B])
        line = f"{name} Cout={Cout} B={B}: winograd max |out - ref| {e:.2e} = {r:.3f} of the bound (max |ref| {float(ref[:B].abs().max()):.1f})"
        if L.sed_conv3x3_bn_relu_pool_eval_supported(B, CIN, Fm, T, Cout):
            direct = ops.conv3x3_bn_relu_pool_eval(g(x_cl[:B]), *[g(d[k]) for k in ("w", "bias", "gamma", "beta", "rm", "rv")], eps=d["eps"])
            r0, e0 = _over_bound(direct.cpu(), ref[:B])
            line += f" | direct kernel {e0:.2e} = {r0:.3f}"
        print(line)
        if not r <= 1.0:
            k = int((out.double() - ref[:B]).abs().argmax())
            b, t, f, ch = np.unravel_index(k, tuple(ref[:B].shape))
            fails.append(line + f"; worst at (b, t', f, c) = ({b}, {t}, {f}, {ch}): {wc.locate(wc.wino_geo(B, CIN, Fm, T, Cout), int(t), int(f), int(ch))}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,Cout", wc.RUNS)
def test_pooled_output_vs_float64_on_real_values(ops, name, Cout):
    _rounding(ops, name, Cout, BS)


def test_long_sequence_vs_float64_on_real_values(ops):
    _rounding(ops, *wc.LONG, (1,))


# ───────────────────────── g: the plain forward on eight column groups ─────────────────────────
@pytest.mark.parametrize("name", ["eight-groups", "eight-groups-two-blocks"])
def test_plain_forward_and_statistic_rows_on_eight_column_groups(ops, name):
    """sed_conv3x3_wino_fwd: y and the statistic rows under the bound of test_conv3x3_winograd_forward_and_data_gradient (the direct
    kernel's own error on the same inputs x 4 + an ulp term of the output scale)"""
    c = wc.case(name)
    Fm, T, Cout = c["F"], c["T"], 128
    assert c["claims"][0] == 8
    gen = torch.Generator().manual_seed(800 + Fm + T)
    x = torch.randn(wc.B_XCD, T, Fm, CIN, generator=gen)
    w = torch.randn(Cout, CIN, 3, 3, generator=gen) / (3.0 * CIN ** 0.5)
    bias = torch.randn(Cout, generator=gen)
    ref8 = F.conv2d(x.permute(0, 3, 2, 1).double(), w.double(), bias.double(), padding=1).permute(0, 3, 2, 1).contiguous()
    uf, _ = ops.conv3x3_wino_pack(g(w))
    wf0, _ = ops.conv3x3_pack(g(w))
    ys = {}
    for B in BS:
        ref = ref8[:B]
        xv, big = guarded(x[:B])
        y, stat = ops.conv3x3_wino_fwd(xv, uf, g(bias), Cout)
        assert stat.shape[0] == B * c["claims"][2] * 8 and not bool(torch.isnan(y).any()) and guards_intact(big, xv.numel())
        y0, _ = ops.conv3x3_fwd(xv, wf0, g(bias), False)
        scale = float(ref.abs().mean())
        err, err0 = (y.cpu().double() - ref).abs(), (y0.cpu().double() - ref).abs()
        print(f"winograd fwd {name} B={B}: max err {float(err.max()):.2e} mean {float(err.mean()):.2e} | direct max {float(err0.max()):.2e} "
              f"mean {float(err0.mean()):.2e} | scale {scale:.2e}")
        assert float(err.max()) < 4.0 * float(err0.max()) + 2e-6 * scale and float(err.mean()) < 4.0 * float(err0.mean()) + 2e-7 * scale
        assert float(err.max()) < 2e-5 * scale * 10
        s = stat.sum(0).cpu().double()
        torch.testing.assert_close(s[0], ref.sum((0, 1, 2)), rtol=1e-4, atol=2e-5 * scale * B * T * Fm)
        torch.testing.assert_close(s[1], (ref * ref).sum((0, 1, 2)), rtol=1e-4, atol=1e-4)
        assert torch.equal(y, ops.conv3x3_wino_fwd(xv, uf, g(bias), Cout)[0])
        ys[B] = y.cpu()
    assert _same_bits(ys[wc.B_XCD][:wc.B_PLAIN], ys[wc.B_PLAIN]), "a sequence's output depends on the workgroup order"


# ───────────────────────── f: a shape the geometry refuses ─────────────────────────
def test_refused_shape_is_refused_on_the_host_by_every_entry(ops):
    from sed_crnn_amd._lib import ptr, stream_ptr
    L = ops.lib()
    c = wc.case("refused")
    Fm, T, Cout, B = c["F"], c["T"], 128, 2
    assert c["claims"] is None and wc.wino_geo(B, CIN, Fm, T, Cout) is None
    for Fr, Tr in wc.REFUSED:
        assert L.sed_conv3x3_wino_rows(B, CIN, Fr, Tr, Cout) == 0
    d = real_inputs(Fm, T, Cout, B)
    xg = g(cl(d["x"]))
    args = [g(d[k]) for k in ("w", "bias", "gamma", "beta", "rm", "rv")]
    with pytest.raises(ValueError):
        ops.conv3x3_bn_relu_pool_eval(xg, *args, wino=True)
    # the C entry: only now that the row query has shown that the host refuses the shape (a host-side check in front of the launch)
    assert L.sed_conv3x3_wino_rows(B, CIN, Fm, T, Cout) == 0
    uf, bf = _pack(L, d, Cout)
    obuf, out = _guarded(B, T // 2, Fm, Cout)
    rc = L.sed_conv3x3_wino_bn_relu_pool_eval(ptr(xg), ptr(uf), ptr(bf), ptr(out), B, CIN, Fm, T, Cout, stream_ptr())
    msg = L.sed_last_error_string()
    assert rc < 0 and b"not supported" in msg and b"launch" not in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((obuf == NAN_BITS).all()), "the refused call wrote to its output"


# ───────────────────────── the eval plan that packs and launches it ─────────────────────────
#        name                 in_channels n_mels  B   T   kernels of blocks 1 and 2
NETS = [("config-5 width",           4,    128,   3, 32, ("winograd EV", "winograd EV")),
        ("mel 40, XCD order",        1,     40,   8, 32, ("winograd EV", "winograd EV")),
        ("too wide for channels-last", 1,  256,   2, 16, ("winograd EV", "direct conv + BN/pool pass")),
        ("refused block",            1,     70,   2, 16, (None, "winograd EV"))]      # block 1 is (F, T) = (70, 8)


def _build_net(sed, cin, mel, seed):
    """TimePooledCRNN and its float32 oracle on rs_state_dict weights, BatchNorm of every block overwritten: gamma in [0.5, 1.5]
    with -0.8, 0 (beta > 0), 0 (beta < 0) and 1e-3; running variance log-uniform over [0.05, 20], both ends present"""
    from oracle import crnn_ref
    kw = dict(conv_channels=128, dropout=0.0, in_channels=cin, n_mels=mel, gru_hidden=32)
    r, m = crnn_ref.SedNetRef(**kw), sed.TimePooledCRNN(**kw)
    sd = crnn_ref.rs_state_dict(r, seed)
    gen = torch.Generator().manual_seed(seed)
    for l in range(3):
        gamma = torch.rand(128, generator=gen) + 0.5
        beta = torch.randn(128, generator=gen) * 0.3
        rv = torch.exp(torch.rand(128, generator=gen) * float(np.log(20 / 0.05)) + float(np.log(0.05)))
        gamma[1] = -0.8
        gamma[5], beta[5] = 0.0, 0.4
        gamma[70], beta[70] = 0.0, -0.3
        gamma[9] = 1e-3
        rv[2], rv[3] = 0.05, 20.0
        sd[f"bns.{l}.weight"], sd[f"bns.{l}.bias"], sd[f"bns.{l}.running_var"] = gamma, beta, rv
        sd[f"bns.{l}.running_mean"] = torch.randn(128, generator=gen) * 0.3
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    return r.eval(), m.cuda().eval(), sd


def _block_kernels(L, m, cfg):
    """which kernel each conv block of the eval layout runs, from the host queries the plan itself is built from"""
    from sed_crnn_amd._lib import lib
    out = []
    Fm, T, Ci = cfg.F, cfg.T, cfg.Cin
    off, n = C.c_size_t(), C.c_size_t()
    for l in range(cfg.n_conv):
        stored = lib().sed_net_workspace_region(C.byref(cfg), 0, b"conv_out", l, C.byref(off), C.byref(n)) == 0
        wino = l > 0 and L.sed_conv3x3_wino_rows(cfg.B, Ci, Fm, T, cfg.C[l]) > 0
        if l == 0:
            out.append("conv + BN/pool pass" if stored else "first block, recomputed (conv1)")
        elif stored:
            out.append("direct conv + BN/pool pass")
        else:
            out.append("winograd EV" if wino else "direct EV")
        Ci, T, Fm = cfg.C[l], T // cfg.pool_t[l], Fm // cfg.pool_f[l]
    return out


@pytest.mark.parametrize("name", [n[0] for n in NETS])
def test_eval_plan_blocks_projection_and_logits_vs_float64(ops, sed, name):
    L = ops.lib()
    _, cin, mel, B, T, want = next(n for n in NETS if n[0] == name)
    r32, m, sd = _build_net(sed, cin, mel, 40 + mel)
    r64 = copy.deepcopy(r32).double()
    x = torch.randn(B, cin, mel, T, generator=torch.Generator().manual_seed(mel + T))
    assert m.inference_plan(B, T) == {"conv": ["f32"] * 3, "proj": "f32"}
    with torch.no_grad():
        logits = m(x.cuda()).cpu()
        l64, l32 = r64(x.double()), r32(x).double()
    cfg = m._last_eval[0]
    kernels = _block_kernels(L, m, cfg)
    print(f"{name}: blocks run {kernels}")
    for l in (1, 2):
        if want[l - 1] is not None:
            assert kernels[l] == want[l - 1], (l, kernels)
    if name == "refused block":
        assert L.sed_conv3x3_wino_rows(B, 128, 70, 8, 128) == 0
        assert kernels[1] == ("direct EV" if L.sed_conv3x3_bn_relu_pool_eval_supported(B, 128, 70, 8, 128) else "direct conv + BN/pool pass")
    if name == "config-5 width":
        assert 128 * mel * 4 == 64 * 1024                       # the re-ordered GRU input row: exactly the 64 KiB both host checks allow
    # blocks: each against the float64 block on the plan's own output of the block below
    fails = []
    below, Tl = x.double(), T
    for l in range(3):
        Tl //= 2
        flat = m.eval_workspace_view("pooled", l).cpu()
        gru_order = l == 2 and kernels[l] == "direct conv + BN/pool pass"       # [B][T'][C][F]: the reference's feature order c * F + f
        got = flat.view(B, Tl, 128, mel).permute(0, 2, 3, 1) if gru_order else flat.view(B, Tl, mel, 128).permute(0, 3, 2, 1)
        with torch.no_grad():
            ref = F.max_pool2d(torch.relu(r64.bns[l](r64.convs[l](below))), (1, 2))
        assert ref.shape == got.shape == (B, 128, mel, Tl)
        err = (got.double() - ref).abs()
        if l == 0:
            bound = 3e-5 + 1e-4 * ref.abs()
        else:
            bound = 2e-5 * max(1.0, float(ref.abs().max())) + 1e-5 * ref.abs()
        ratio = float((err / bound).max())
        print(f"{name} block {l} ({kernels[l]}): max |out - ref| {float(err.max()):.2e} = {ratio:.3f} of the bound (max |ref| {float(ref.abs().max()):.1f})")
        if not ratio <= 1.0:
            fails.append(f"block {l}: {ratio:.3f} of the bound")
        assert not bool(torch.isnan(got).any())
        below = got.double().contiguous()
    # the GRU input projection on the plan's own last block: W_ih re-ordered to the layout that block was written in
    H = 32
    x_seq = below.permute(0, 3, 1, 2).reshape(B * Tl, 128 * mel)                  # feature = c * F + f
    w_ih = torch.cat([sd["gru.weight_ih_l0"], sd["gru.weight_ih_l0_reverse"]]).double()
    b_ih = torch.cat([sd["gru.bias_ih_l0"], sd["gru.bias_ih_l0_reverse"]]).double()
    gi_ref = x_seq @ w_ih.t() + b_ih
    gi = m.eval_workspace_view("gi", 0).cpu().view(B * Tl, 6 * H).double()
    tol = 2e-6 * (128 * mel) ** 0.5 * 10 * 4
    gerr = float((gi - gi_ref).abs().max())
    gratio = float(((gi - gi_ref).abs() / (tol + 1e-4 * gi_ref.abs())).max())
    print(f"{name} GRU input projection: max |gi - ref| {gerr:.2e} = {gratio:.3f} of the bound (max |ref| {float(gi_ref.abs().max()):.2f})")
    if not gratio <= 1.0:
        fails.append(f"GRU input projection: {gratio:.3f} of the bound")
    # logits
    dp = float((torch.sigmoid(logits.double()) - torch.sigmoid(l64)).abs().max())
    den = float(l64.norm())
    e_h, e_t = float((logits.double() - l64).norm()) / den, float((l32 - l64).norm()) / den
    print(f"{name} logits: max |dp| {dp:.2e}; rel L2 hip {e_h:.2e} torch-f32 {e_t:.2e} ratio {e_h / (e_t + 1e-300):.2f} bound use {e_h / (3.0 * e_t + 2e-6):.2f}")
    if not dp <= 1e-3:
        fails.append(f"max |dp| {dp:.3e} > 1e-3")
    if not e_h <= 3.0 * e_t + 2e-6:
        fails.append(f"logit rel L2 {e_h:.3e} > 3 * {e_t:.3e} + 2e-6")
    assert not fails, name + ":\n  " + "\n  ".join(fails)
