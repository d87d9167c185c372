"""The 3x3 weight-gradient kernels of conv.hip where a workgroup walks SEVERAL tiles (capped grids: 64 groups for the MFMA kernels,
1024 for the small ones) — the regime of every production launch, which the shapes of test_gpu_kernels.py (at most 24 tiles) never
reach.  The cases and the proof that each is in its regime are in wgrad_plan_ref.py / test_cpu_wgrad_plan.py.

sed_conv3x3_wgrad_ex is called through ctypes, so the test owns the workspace (what it holds before the call, the slabs after it).

* exact: x and dy are integers in [-2, 2]; every product, every partial sum in any order and every Winograd-domain quantity is
  then an integer or a multiple of 1/4 below 2^24 (asserted in test_cpu_wgrad_plan.py) and exact in float32, so dw must EQUAL the
  float64 torch.nn.grad.conv2d_weight — no tolerance.  A dropped or doubled tile, or a halo row taken from the wrong place,
  changes integers.  On failure the worst entries are attributed to a group and a tile from the slabs.
* the same with workspace and dw full of NaN (empty groups must write their slabs; the entry's own zero-row memset must do), and
  with SED_WGRAD_ZERO_ROW_CLEAN where the test clears the zero row itself.
* run to run: two calls on unit-normal inputs, different workspace contents, identical bits.
* rounding against float64 on unit normals: one case per kernel family and form plus a seeded sweep of position-contiguous
  shapes.  The bound is taken from a yardstick, torch's CPU float32 conv2d_weight on ONE thread on the same inputs (E32_max,
  E32_rms against float64): direct forms max <= 3 E32_max + 2^-23 rms(dW), rms <= 3 E32_rms (3x: this suite's "is an fp32
  implementation", test_gpu_model.py); the Winograd form 4x that (what the Winograd forward test grants: the transforms only add
  and halve).  The bf16x3 experiment (mode 1) is not an fp32 implementation; it keeps the bound its own test holds it to
  (test_conv3x3_bf16x3_experiment_weight_gradient: 2e-4 / 2e-5 of mean |dW|, which like the error grows with sqrt(B*T*F)).
  Every case prints kernel error / yardstick."""
import functools

import numpy as np
import pytest
import torch

import wgrad_plan_ref as wp  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 256                                  # floats behind the workspace that no kernel may touch


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sed_crnn_amd import _lib
    yield _lib.lib()
    _data.cache_clear()
    _ref64.cache_clear()


def _reference(x_cl, dy, Cin, Cout, dtype):
    return torch.nn.grad.conv2d_weight(x_cl.permute(0, 3, 2, 1).to(dtype), (Cout, Cin, 3, 3), dy.permute(0, 3, 2, 1).to(dtype), padding=1)


@functools.lru_cache(maxsize=None)
def _data(shape, nchw, kind):
    """seeded operands of a shape (CPU, channels-last, float32) and the same on the device in the layout the case uses — made once
    per shape and shared by every test and mode; nobody writes to them"""
    B, Cin, F, T, Cout = shape
    gen = torch.Generator().manual_seed(sum(s * m for s, m in zip(shape, (1, 7, 131, 1009, 3))) + (kind == "int"))
    if kind == "int":
        x_cl = torch.randint(-2, 3, (B, T, F, Cin), generator=gen).float()
        dy = torch.randint(-2, 3, (B, T, F, Cout), generator=gen).float()
    else:
        x_cl, dy = torch.randn(B, T, F, Cin, generator=gen), torch.randn(B, T, F, Cout, generator=gen)
    xg = (x_cl.permute(0, 3, 2, 1) if nchw else x_cl).contiguous().cuda()
    return x_cl, dy, xg, dy.cuda()


@functools.lru_cache(maxsize=None)
def _ref64(shape, nchw, kind):
    """the float64 reference of _data's operands, computed once"""
    x_cl, dy, _, _ = _data(shape, nchw, kind)
    return _reference(x_cl, dy, shape[1], shape[4], torch.float64)


def _call(L, shape, nchw, mode, xg, dyg, fill):
    """one call with the workspace (exactly the queried bytes, + a guard) and dw pre-filled with `fill` -> (dw on the CPU, workspace)"""
    from sed_crnn_amd._lib import ptr, check, stream_ptr
    B, Cin, F, T, Cout = shape
    nbytes = L.sed_conv3x3_wgrad_workspace_bytes(B, Cin, F, T, Cout)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + GUARD,), fill, device="cuda")
    ws[nbytes // 4:] = 12345.0
    if mode & wp.SED_WGRAD_ZERO_ROW_CLEAN:
        zb = L.sed_conv3x3_wgrad_zero_row_bytes(B, Cin, F, T, Cout)
        assert zb > 0 and zb % 4 == 0
        ws[:zb // 4] = 0.0
    dw = torch.full((Cout, Cin, 3, 3), fill, device="cuda")
    check(L.sed_conv3x3_wgrad_ex(ptr(xg), int(nchw), ptr(dyg), ptr(dw), ptr(ws), B, Cin, F, T, Cout, mode, stream_ptr()), "conv3x3_wgrad_ex")
    torch.cuda.synchronize()
    assert bool((ws[nbytes // 4:] == 12345.0).all()), "the kernel wrote behind its workspace"
    return dw.cpu(), ws[:nbytes // 4]


def _assert_exact(c, label, mode, dw, ws, x_cl, dy, ref):
    if torch.equal(dw.double(), ref):
        return
    p = wp.plan_for(c, mode)
    slabs = ws[p.zrow_floats:].cpu().numpy()
    report = wp.attribute(p, c, label == "wino", x_cl.double().numpy(), dy.double().numpy(), dw.numpy(), ref.numpy(), slabs)
    print("\n".join(report))
    raise AssertionError("dw differs from the float64 reference on integer inputs\n" + "\n".join(report))


# ───────────────────────── a. exact on integers ─────────────────────────
@pytest.mark.parametrize("name,label", wp.RUNS)
def test_weight_gradient_is_exact_on_small_integers(L, name, label):
    c = wp.case(name)
    mode = wp.mode_bits(name, label)
    x_cl, dy, xg, dyg = _data(c["shape"], c["nchw"], "int")
    ref = _ref64(c["shape"], c["nchw"], "int")
    dw, ws = _call(L, c["shape"], c["nchw"], mode, xg, dyg, 0.0)
    _assert_exact(c, label, mode, dw, ws, x_cl, dy, ref)


# ───────────────────────── b. poisoned workspace ─────────────────────────
@pytest.mark.parametrize("name,label", wp.RUNS)
def test_weight_gradient_ignores_what_the_workspace_held(L, name, label):
    """workspace and dw full of NaN: empty groups write their (zero) slabs, every dw entry is written, the zero row is cleared by
    the entry; the position-contiguous kernel once more with SED_WGRAD_ZERO_ROW_CLEAN and only the zero row cleared by the test"""
    c = wp.case(name)
    mode = wp.mode_bits(name, label)
    x_cl, dy, xg, dyg = _data(c["shape"], c["nchw"], "int")
    ref = _ref64(c["shape"], c["nchw"], "int")
    dw, ws = _call(L, c["shape"], c["nchw"], mode, xg, dyg, float("nan"))
    assert bool(torch.isfinite(dw).all())
    _assert_exact(c, label, mode, dw, ws, x_cl, dy, ref)
    if c["kernel"].startswith("wgrad2") and label != "bf16x3":
        dw2, ws2 = _call(L, c["shape"], c["nchw"], mode | wp.SED_WGRAD_ZERO_ROW_CLEAN, xg, dyg, float("nan"))
        assert bool(torch.isfinite(dw2).all())
        _assert_exact(c, label, mode, dw2, ws2, x_cl, dy, ref)
        assert torch.equal(dw2.view(torch.int32), dw.view(torch.int32))
        p = wp.plan_for(c, mode)
        assert bool((ws2[:p.zrow_floats] == 0).all())                   # the kernel only reads the zero row


# ───────────────────────── c. run to run ─────────────────────────
@pytest.mark.parametrize("name,label", wp.RUNS)
def test_weight_gradient_is_the_same_from_run_to_run(L, name, label):
    """fixed-order reduction: a second call on the same unit-normal inputs, with another workspace content, gives the same bits"""
    c = wp.case(name)
    mode = wp.mode_bits(name, label)
    _, _, xg, dyg = _data(c["shape"], c["nchw"], "normal")
    dw1, _ = _call(L, c["shape"], c["nchw"], mode, xg, dyg, 0.0)
    dw2, _ = _call(L, c["shape"], c["nchw"], mode, xg, dyg, float("nan"))
    assert bool(torch.isfinite(dw1).all())
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32))


# ───────────────────────── d. rounding against float64 ─────────────────────────
def _yardstick(x_cl, dy, Cin, Cout, ref):
    """torch's CPU float32 conv2d_weight on one thread against float64 -> (E32_max, E32_rms)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        e = (_reference(x_cl, dy, Cin, Cout, torch.float32).double() - ref).abs()
    finally:
        torch.set_num_threads(n)
    return float(e.max()), float((e ** 2).mean().sqrt())


def _check_rounding(L, tag, shape, nchw, label, mode, data, ref, yard):
    x_cl, dy, xg, dyg = data
    e32_max, e32_rms = yard
    dw, _ = _call(L, shape, nchw, mode, xg, dyg, float("nan"))
    err = (dw.double() - ref).abs()
    emax, erms = float(err.max()), float((err ** 2).mean().sqrt())
    rms_dw = float((ref ** 2).mean().sqrt())
    if label == "bf16x3":
        scale = float(ref.abs().mean())
        bmax, brms = 2e-4 * scale, None
        print(f"{tag} {label}: max {emax:.3e} (bound {bmax:.3e}), mean {float(err.mean()):.3e} (bound {2e-5 * scale:.3e}); "
              f"yardstick E32 max {e32_max:.3e} rms {e32_rms:.3e}: ratio max {emax / e32_max:.3f} rms {erms / e32_rms:.3f}")
        assert emax <= bmax and float(err.mean()) <= 2e-5 * scale
        return
    k = 4.0 if label == "wino" else 1.0
    bmax, brms = k * (3.0 * e32_max + 2.0 ** -23 * rms_dw), k * 3.0 * e32_rms
    print(f"{tag} {label}: max {emax:.3e} (bound {bmax:.3e}), rms {erms:.3e} (bound {brms:.3e}); yardstick E32 max {e32_max:.3e} rms "
          f"{e32_rms:.3e}: ratio max {emax / e32_max:.3f} rms {erms / e32_rms:.3f}")
    assert emax <= bmax, (tag, label, emax, bmax)
    assert erms <= brms, (tag, label, erms, brms)


ROUNDING_CASES = ["w40_seq_step", "w32_per3_nft2", "w40_per3_2co", "mfma_tt4", "mfma_mt_ragged", "small_cin1", "small_c2", "small_c3",
                  "small_c4_cl", "small_cin16"]


@pytest.mark.parametrize("name", ROUNDING_CASES)
def test_weight_gradient_rounding_against_float64(L, name):
    """one case per kernel family, every form it runs in"""
    c = wp.case(name)
    _, Cin, _, _, Cout = c["shape"]
    data, ref = _data(c["shape"], c["nchw"], "normal"), _ref64(c["shape"], c["nchw"], "normal")
    yard = _yardstick(data[0], data[1], Cin, Cout, ref)
    for label, mode in wp.case_modes(c):
        _check_rounding(L, name, c["shape"], c["nchw"], label, mode, data, ref, yard)


def _sweep_shapes(n=12, seed=20240611):
    """B from {1,2,3,5,7}, F from {32,...,160}, T from 20-60 (odd values too), Cin 32, Cout 128; kept: more tiles than the 64 groups"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        B, F, T = int(rng.choice([1, 2, 3, 5, 7])), int(rng.choice([32, 40, 64, 80, 120, 128, 160])), int(rng.integers(20, 61))
        p = wp.wgrad_plan(B, 32, F, T, 128, False)
        assert p.v2
        if p.ntiles > 64 and (B, 32, F, T, 128) not in out:
            out.append((B, 32, F, T, 128))
    return out


SWEEP = _sweep_shapes()


@pytest.mark.parametrize("shape", SWEEP, ids=lambda s: "B%d_F%d_T%d" % (s[0], s[2], s[3]))
def test_position_contiguous_weight_gradient_sweep_against_float64(L, shape):
    """seeded shapes of the position-contiguous kernel with more tiles than groups, Winograd and direct form"""
    p = wp.wgrad_plan(*shape, False)
    assert p.v2 and p.ntiles > p.ngroups == 64
    data, ref = _data(shape, False, "normal"), _ref64(shape, False, "normal")
    yard = _yardstick(data[0], data[1], shape[1], shape[4], ref)
    tag = f"B{shape[0]} F{shape[2]} T{shape[3]} ({p.ntiles} tiles, {p.per} per run, {p.busy} busy)"
    for label, mode in (("wino", 0), ("direct", wp.SED_WGRAD_DIRECT)):
        _check_rounding(L, tag, shape, False, label, mode, data, ref, yard)
