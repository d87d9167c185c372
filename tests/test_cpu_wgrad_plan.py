"""The shapes test_gpu_wgrad_tiles.py runs really are where a weight-gradient workgroup walks several tiles: a restatement of
wgrad_plan (wgrad_plan_ref.py) is held against the library's workspace query, every case is shown to be in the regime its row
claims, and the attribution helper the GPU test prints on failure is shown to name a dropped tile.  No GPU."""
import numpy as np
import pytest

import wgrad_plan_ref as wp  # noqa: E402


def _kernel_name(c, p):
    """the dispatch of sed_conv3x3_wgrad_ex (mode 0), restated"""
    _, Cin, F, _, _ = c["shape"]
    if p.kind == 1:
        return f"wgrad2<{p.FT}>" if p.v2 else f"mfma_wgrad<{'true' if p.nft > 1 else 'false'}>"
    lds_c = ((((p.TT + 2) * (F + 2) * Cin + 3) & ~3) + 256 * 36) * 4
    return f"small_c<{Cin}>" if Cin in (2, 3, 4) and lds_c <= 150 * 1024 else "small"


@pytest.mark.parametrize("name", [c["name"] for c in wp.CASES])
def test_workspace_query_matches_the_restated_plan(name):
    from sed_crnn_amd import _lib
    L = _lib.lib()
    c = wp.case(name)
    B, Cin, F, T, Cout = c["shape"]
    p = wp.plan_for(c)
    got = L.sed_conv3x3_wgrad_workspace_bytes(B, Cin, F, T, Cout)
    assert got == wp.workspace_bytes(B, Cin, F, T, Cout)
    assert L.sed_conv3x3_wgrad_zero_row_bytes(B, Cin, F, T, Cout) == p.zrow_floats * 4
    if p.kind == 1:
        # the capped grid: 64 slabs of 16 (position-contiguous kernel: the Winograd form's components) or 9 taps, behind the zero row
        assert p.ngroups == 64 and (p.zrow_floats > 0) == bool(p.v2)
        capped = (64 * (16 if p.v2 else 9) * Cin * Cout + p.zrow_floats) * 4
        # the query also covers the same shape given as NCHW (the small kernel: one slab of 9 taps per 4-row tile, up to 1024)
        nchw = min(1024, B * wp.cdiv(T, min(4, T))) * 9 * Cin * Cout * 4
        assert got == max(capped, nchw + p.zrow_floats * 4)
        if p.v2:
            assert got == capped                # every position-contiguous case: the 64 x 16 slabs are the larger area
    else:
        assert p.ngroups == 1024 and got == 1024 * 9 * Cin * Cout * 4


@pytest.mark.parametrize("name", [c["name"] for c in wp.CASES])
def test_case_is_in_the_regime_its_row_claims(name):
    c = wp.case(name)
    B, Cin, F, T, Cout = c["shape"]
    p = wp.plan_for(c)
    assert _kernel_name(c, p) == c["kernel"]
    assert p.ntiles > p.ngroups and p.per >= 2              # the point of the table: more tiles than workgroups
    facts = dict(p._asdict(), **wp.regime(p, T))
    for key, want in c["claims"].items():
        assert facts[key] == want, (name, key, facts[key], want)
    # every tile belongs to exactly one group, whichever walk
    seen = sorted(t for g in range(p.ngroups) for t in wp.group_tiles(p, g))
    assert seen == list(range(p.ntiles))
    assert all(wp.group_of(p, t) == g for g in range(p.ngroups) for t in wp.group_tiles(p, g))
    if p.v2:
        assert facts["empty_groups"] == 64 - p.busy > 0     # trailing groups without a tile, whose slabs are still summed
    # exactness precondition of the integer test
    assert wp.exactness_bound(c) < 2 ** 24
    # operands of a few MB
    assert (B * T * F * (Cin + Cout) * 4) <= 12.5e6


def test_the_table_covers_every_property_of_the_walk():
    """each property the contiguous walk can get wrong is claimed by at least one case of each tile width, each strided kernel
    has a case where only some groups take a second tile, and the bf16x3 walk (two tiles ahead) has groups with three"""
    for ft in (40, 32):
        rows = [c for c in wp.CASES if c["kernel"] == f"wgrad2<{ft}>"]
        for key in ("crosses_sequence", "ragged_last_run", "ragged_last_time_tile"):
            assert any(c["claims"].get(key) for c in rows), (ft, key)
        assert any(c["claims"].get("per") == 3 for c in rows) and any(wp.plan_for(c).nft > 1 for c in rows)
    assert any(c["claims"].get("crosses_mel_row") for c in wp.CASES)
    assert any(c["shape"][1] == 128 for c in wp.CASES if c["kernel"].startswith("wgrad2"))      # four ci blocks
    assert any(c["shape"][4] == 256 for c in wp.CASES if c["kernel"].startswith("wgrad2"))      # two co blocks
    assert {c["kernel"] for c in wp.CASES} == {"wgrad2<40>", "wgrad2<32>", "mfma_wgrad<false>", "mfma_wgrad<true>", "small", "small_c<2>",
                                               "small_c<3>", "small_c<4>"}
    c = wp.case(wp.BF16X3_CASE)
    p = wp.plan_for(c, 1)
    r = wp.regime(p, c["shape"][3])
    assert (p.v2, p.TT, p.FT, p.ntiles, p.ngroups, p.walk) == (0, 2, 40, 135, 64, "stride")
    assert (r["max_tiles"], r["groups_with_max"]) == (3, 7) and p.zrow_floats == 0
    assert len(wp.RUNS) == len(wp.CASES) + 10 + 1           # ten position-contiguous cases run in both forms, one also on bf16x3


def _emulated_slabs(p, c, wino, x_cl, dy, drop=None, twice=None):
    """per-group slabs in the layout the kernels write, from float64 per-tile sums (direct) or 2x2 Winograd tiles of the
    transformed operands (Winograd form, position-contiguous tiles only); `drop` / `twice`: a tile left out / added once more"""
    B, Cin, F, T, Cout = c["shape"]
    xp = np.zeros((B, p.tblocks * p.TT + 2, p.nft * p.FT + 2, Cin))
    xp[:, 1:T + 1, 1:F + 1] = x_cl
    dp = np.zeros((B, p.tblocks * p.TT, p.nft * p.FT, Cout))
    dp[:, :T, :F] = dy
    small = c["kernel"].startswith("small")
    comps = 16 if wino else 9
    slabs = np.zeros((p.ngroups, comps, Cin, Cout))
    Bt = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
    A = np.array([[1, 0], [1, 1], [1, -1], [0, -1]], dtype=np.float64)
    sign = np.array([1., 1., 1., -1.])
    for g in range(p.ngroups):
        tiles = [t for t in wp.group_tiles(p, g) if t != drop]
        tiles += [t for t in tiles if t == twice]
        for t in tiles:
            b, tb, mel = wp.tile_coords(p, t)
            t0, f0 = tb * p.TT, mel * p.FT
            d = dp[b, t0:t0 + p.TT, f0:f0 + p.FT]                                  # [TT][FT][Cout]
            if not wino:
                for kh in range(3):
                    for kw in range(3):
                        slabs[g, kh * 3 + kw] += np.einsum("tfi,tfo->io", xp[b, t0 + kw:t0 + kw + p.TT, f0 + kh:f0 + kh + p.FT], d)
                continue
            for j in range(p.FT // 2):                                             # one 2 x 2 output tile: 4 x 4 patch, time first
                patch = xp[b, t0:t0 + 4, f0 + 2 * j:f0 + 2 * j + 4]                # [4 time][4 mel][Cin]
                v = np.einsum("xa,abi,nb->xni", Bt, patch, Bt)
                z = np.einsum("xa,abo,nb->xno", A, d[:, 2 * j:2 * j + 2], A)
                # the kernel leaves the sign of A's last row / column to the reduction
                z = z * sign[:, None, None] * sign[None, :, None]
                slabs[g] += np.einsum("xni,xno->xnio", v, z).reshape(16, Cin, Cout)
    if small:
        slabs = slabs.transpose(0, 2, 1, 3)                                        # [g][ci][tap][co]
    return slabs.astype(np.float32).reshape(-1)


@pytest.mark.parametrize("kernel,wino", [("wgrad2<40>", True), ("wgrad2<40>", False), ("mfma_wgrad<true>", False), ("small", False)])
def test_attribution_names_the_group_and_tile(kernel, wino):
    """the failure report of the GPU test, on emulated slabs of a narrowed copy of a table row (fewer channels; same tiling): a
    correct set of slabs reduces to the float64 reference exactly (which also checks the restated slab layouts, the Winograd
    transforms and the signs left to the reduction), and a dropped / doubled tile is named with its group"""
    import torch
    base = next(c for c in wp.CASES if c["kernel"] == kernel)
    B, Cin, F, T, Cout = base["shape"]
    Cin, Cout = min(Cin, 2), 4
    c = dict(base, shape=(B, Cin, F, T, Cout))
    p = wp.wgrad_plan(*base["shape"], base["nchw"])                                # the tiling of the real row
    rng = np.random.default_rng(5)
    x_cl = rng.integers(-2, 3, (B, T, F, Cin)).astype(np.float64)
    dy = rng.integers(-2, 3, (B, T, F, Cout)).astype(np.float64)
    ref = torch.nn.grad.conv2d_weight(torch.from_numpy(x_cl).permute(0, 3, 2, 1), (Cout, Cin, 3, 3), torch.from_numpy(dy).permute(0, 3, 2, 1),
                                      padding=1).numpy()

    def reduce(slabs):
        return np.stack([wp.slab_entry(p, slabs, kernel, wino, Cin, Cout, co, ci, tap).sum()
                         for co in range(Cout) for ci in range(Cin) for tap in range(9)]).reshape(Cout, Cin, 3, 3)

    good = _emulated_slabs(p, c, wino, x_cl, dy)
    assert np.array_equal(reduce(good), ref)
    victim = wp.group_tiles(p, 3)[-1]
    for kw, word in ((dict(drop=victim), "dropped"), (dict(twice=victim), "counted twice")):
        bad = _emulated_slabs(p, c, wino, x_cl, dy, **kw)
        dw = reduce(bad).astype(np.float32)
        assert not np.array_equal(dw, ref)
        text = "\n".join(wp.attribute(p, c, wino, x_cl, dy, dw, ref, bad))
        assert f"group 3 tiles {wp.group_tiles(p, 3)}" in text and f"tile {victim} " in text and word in text, text
        assert "group 2 " not in text and "group 4 " not in text
