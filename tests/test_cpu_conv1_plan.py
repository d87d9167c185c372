"""The shapes test_gpu_conv1_tiles.py runs really are in the regimes their rows claim.  conv1_cases.py restates the launch geometry of
the recomputed first conv block (csrc/conv1.hip); here the restatement is held against the library's host-only entry points on a
dense grid, every row of the table against the regime it names, and the table as a whole against the list of paths it has to reach.
The float64 reference alone is shown to leave out fewer near-ties than the GPU test allows.  No GPU."""
import pytest

import conv1_cases as cc  # noqa: E402

POOLS = [(1, 2), (5, 1), (2, 2), (1, 1), (1, 4), (2, 1)]          # the routing test's pools, the statistics pass's (1,1), two more
CINS = range(0, 6)
FS = list(range(1, 131)) + [200, 405, 406, 407, 408, 409, 410, 512, 1000, 1598, 1599, 3198, 3199, 6398, 6399]
TS = list(range(4, 4097, 4))
CS = list(range(4, 1033, 4)) + [0, 1, 2, 3, 5, 6, 7, 9, 30, 66, 127, 129, 1025, 1028, 2048]
BS = (1, 2, 3, 5, 16, 128, 511, 512, 513)


@pytest.fixture(scope="module")
def L():
    from sed_crnn_amd import _lib
    return _lib.lib()


def _same_answers(L, Cin, F, T, C, pf, pt):
    assert bool(L.sed_conv1_fused_supported(Cin, F, T, C, pf, pt)) == cc.fused_supported(Cin, F, T, C, pf, pt), (Cin, F, T, C, pf, pt)
    assert bool(L.sed_conv1_rgrad_supported(Cin, F, T, C, pf, pt)) == cc.rgrad_supported(Cin, F, T, C, pf, pt), (Cin, F, T, C, pf, pt)
    return cc.fused_supported(Cin, F, T, C, pf, pt), cc.rgrad_supported(Cin, F, T, C, pf, pt)


def test_restated_support_equals_the_library_on_a_dense_grid(L):
    """c1_shape_ok is a conjunction of conditions on Cin, on C, on (T, pool_t), on (F, pool_f) and on Cin * F (the LDS image), so the
    grid is dense along every axis and crossed where two of them meet in one condition: every Cin 0..5 x every F of FS x every pool x
    a few T and C; every T in steps of 4 up to 4096 (and the values between, around a few of them) x every pool; every C that is a
    multiple of 4 up to 1032 and some that are not"""
    n = {(a, b): 0 for a in (False, True) for b in (False, True)}
    for Cin in CINS:
        for F in FS:
            for pf, pt in POOLS:
                for T in (4, 6, 8, 20, 3300):
                    for C in (4, 12, 64, 512, 1024):
                        n[_same_answers(L, Cin, F, T, C, pf, pt)] += 1
    for pf, pt in POOLS:
        for Cin in (1, 2, 3, 4):
            for F in (10, 40):
                for T in TS + [1, 2, 3, 5, 6, 7, 9, 10, 3298, 3299, 3301, 3302]:
                    n[_same_answers(L, Cin, F, T, 64, pf, pt)] += 1
                for C in CS:
                    n[_same_answers(L, Cin, F, 8, C, pf, pt)] += 1
    assert all(v > 0 for v in n.values()), n                 # every pair of answers occurs: (fused, rgrad) = (yes, no) under the other pools
    print({k: v for k, v in n.items()})


def test_fused_implies_rgrad_only_under_the_12_pool(L):
    for pf, pt in POOLS:
        for Cin in (1, 2, 3, 4):
            f, r = _same_answers(L, Cin, 8, 8, 16, pf, pt)
            assert r == ((pf, pt) == (1, 2)) and f == (Cin <= 2 and 8 % pf == 0 and 4 % pt == 0)
    ok = sorted(C for C in CS if cc.fused_supported(1, 8, 8, C, 1, 2))
    assert ok == [4, 8, 16, 32, 64, 128, 256, 512, 1024]                   # C / 4 divides 256: every slot count 256 .. 1
    assert [cc.nslots(C) for C in ok] == [256, 128, 64, 32, 16, 8, 4, 2, 1]
    # the widest mel axis the LDS image of the apply pass admits, per input-channel count
    for Cin in (1, 2, 3, 4):
        fmax = cc.LDS_MAX // (24 * Cin) - 2
        assert cc.rgrad_supported(Cin, fmax, 8, 64, 1, 2) and not cc.rgrad_supported(Cin, fmax + 1, 8, 64, 1, 2)
        assert bool(L.sed_conv1_rgrad_supported(Cin, fmax, 8, 64, 1, 2)) and not L.sed_conv1_rgrad_supported(Cin, fmax + 1, 8, 64, 1, 2)


def test_restated_row_counts_and_workspaces_equal_the_library(L):
    for B in BS:
        for T in TS + [1, 2, 3, 5, 7, 17]:
            assert L.sed_conv1_fused_rows(B, T) == cc.fused_rows(B, T) == cc.fused_plan(B, T)["grid"], (B, T)
    for B in BS:
        for Cin in (1, 2, 3, 4):
            assert L.sed_conv1_moments_doubles(Cin) == cc.moments_doubles(Cin)
            for T in TS[::7] + [3300, 2752]:
                assert L.sed_conv1_stats_workspace_bytes(B, Cin, T) == cc.stats_workspace_bytes(B, Cin, T), (B, Cin, T)
                for C in (4, 8, 64, 512, 1024):
                    assert L.sed_conv1_bwd_apply_workspace_bytes(B, Cin, T, C) == cc.bwd_apply_workspace_bytes(B, Cin, T, C), (B, Cin, T, C)
                    assert L.sed_conv1_bwd_wgrad_workspace_bytes(B, Cin, T, C) == cc.bwd_wgrad_workspace_bytes(B, Cin, T, C), (B, Cin, T, C)
    assert [cc.moments_doubles(c) for c in (1, 2, 3, 4)] == [54, 189, 405, 702]


def test_workspaces_hold_what_the_restated_grids_write():
    """the partial rows every kernel writes, from the restated grid, fit the workspace the library asks for"""
    for B in BS:
        for T in TS[::5] + [3300]:
            for Cin in (1, 2, 3, 4):
                ng = cc.moments_doubles(Cin)
                if Cin <= 2:
                    assert cc.gram_plan(B, T)["grid"] * ng * 4 <= cc.stats_workspace_bytes(B, Cin, T)
                else:
                    nt = cc.cdiv(9 * Cin + 1, 16)
                    assert cc.moments_mfma_plan(B, T)["grid"] * (nt * (nt + 1) // 2) * 256 * 4 + ng * 8 <= cc.stats_workspace_bytes(B, Cin, T)
                for F, C in ((8, 64), (8, 32), (408, 64)):
                    p = cc.rgrad_plan(B, Cin, F, T, C)
                    assert p["grid"] * (1 + 9 * Cin) * C * 4 <= cc.bwd_wgrad_workspace_bytes(B, Cin, T, C)
                    assert p["grid"] * p["visits"] >= p["tiles"] > p["grid"] * (p["visits"] - 1)


@pytest.mark.parametrize("name", cc.NAMES)
def test_row_is_accepted_and_in_the_regime_its_name_claims(L, name):
    c = cc.case(name)
    B, Cin, F, T, C = c["shape"]
    pf, pt = c["pool"]
    got = cc.regime(c)
    assert c["claims"] and {k: got[k] for k in c["claims"]} == c["claims"], (name, got)
    # what the GPU test calls on this row is accepted by the library (host side) and by the restatement
    assert cc.fwd_supported(Cin, F, T, C, pf, pt) and cc.stats_supported(Cin, F, T, C)
    assert bool(L.sed_conv1_fused_supported(Cin, F, T, C, pf, pt)) == (Cin <= 2)
    assert bool(L.sed_conv1_rgrad_supported(Cin, F, T, C, pf, pt)) == ((pf, pt) == (1, 2))
    assert L.sed_conv1_fused_supported(min(Cin, 2), F, T, C, 1, 1)                      # the statistics pass checks the shape with pool (1,1)
    assert L.sed_conv1_fused_rows(B, T) == got["fused_grid"]
    assert B * T * F <= 163840                                                           # the gradient tolerances were set at this count
    assert B * (T // pt) * (F // pf) * C * 4 <= 17 * 2 ** 20 and B * Cin * F * T * 4 <= 17 * 2 ** 20
    # the walk-invariance test compares with every sequence alone: that run does not walk
    assert cc.fused_plan(1, T)["visits"] == 1 and cc.fused_plan(1, T)["tiles"] == cc.cdiv(T, 4)


def test_the_table_reaches_every_path_of_the_launchers():
    R = {c["name"]: cc.regime(c) for c in cc.CASES}
    rows = list(R.values())

    def reached(pred):
        return {(r["cin"], walks) for r in rows for walks in (False, True) if pred(r, walks)}

    both = lambda cins: {(ci, w) for ci in cins for w in (False, True)}
    # every CIN x {walks, does not walk} of each persistent kernel
    assert reached(lambda r, w: r["p12"] and (r["fused_visits"] > 1) == w) == both((1, 2, 3, 4))                                   # conv1_fused_k, forward
    assert reached(lambda r, w: r["stats_kernel"] == "gram" and r["p12"] and (r["stats_visits"] > 1) == w) == both((1, 2))           # conv1_gram_k
    assert reached(lambda r, w: r["stats_kernel"] == "mfma" and (r["stats_visits"] > 1) == w) == both((3, 4))                       # conv1_moments_mfma_k
    assert reached(lambda r, w: r["rgrad_kernel"] == "scalar" and (r["rgrad_visits"] > 1) == w) == both((1, 2, 3, 4))               # conv1_rgrad_k
    assert reached(lambda r, w: r["rgrad_kernel"] == "mfma" and (r["rgrad_visits"] > 1) == w) == both((3, 4))                       # conv1_rgrad_mfma_k
    assert {(1, True), (2, True)} <= reached(lambda r, w: not r["p12"] and (r["fused_visits"] > 1) == w)                             # the generic window loop
    # a walk crosses into another sequence: more tiles than workgroups AND more than one sequence AND tiles per sequence no multiple of the grid
    for c in cc.CASES:
        r = R[c["name"]]
        if r["fused_visits"] > 1:
            assert c["shape"][0] > 1 and r["fused_grid"] % cc.fused_plan(1, c["shape"][3])["tiles"] != 0
    # the gram staging round with tiles beyond the last one
    assert any(r["stats_kernel"] == "gram" and r["gram_last_round"] < cc.GR and r["stats_visits"] > 1 for r in rows)
    # both rgrad kernels for 3 and 4 input channels, both causes of the scalar fallback
    assert {(r["cin"], r["rgrad_kernel"]) for r in rows if r["cin"] > 2} == {(3, "scalar"), (3, "mfma"), (4, "scalar"), (4, "mfma")}
    assert {r["rgrad_cause"] for r in rows if r["cin"] > 2 and r["rgrad_kernel"] == "scalar"} == {"channels", "lds"}
    assert R["scalar-4ch-wide"]["rgrad_cause"] == "lds" and cc.rgrad_kernel(4, 407, 64) == ("mfma", None)                          # 408: the first F beyond 64 KiB
    assert any(r["rgrad_grid_y"] == 2 for r in rows)
    # ragged mel groups on the matrix-core kernels: the mask of the moment kernel (groups of 4), the clamp of the rgrad kernel (groups of 8),
    # below one group and behind full groups
    mm = [r for r in rows if r["stats_kernel"] == "mfma"]
    assert any(r["F_mod4"] == 0 for r in mm) and any(r["F_mod4"] != 0 for r in mm)
    rm = [r for r in rows if r["rgrad_kernel"] == "mfma"]
    assert any(r["F_mod8"] == 0 for r in rm) and any(r["F_mod8"] != 0 and r["F"] < 8 for r in rm) and any(r["F_mod8"] != 0 and r["F"] > 8 for r in rm)
    # ragged time tiles behind full ones: 16 rows in both moment kernels, 8 rows (waves without a pooled row) in the MFMA rgrad
    for kern in ("gram", "mfma"):
        assert any(r["stats_kernel"] == kern and r["T_mod16"] != 0 and r["full16"] for r in rows)
    assert any(r["T_mod8"] != 0 and r["full8"] and r["rgrad_last_waves"] == 2 for r in rm)
    # slot counts: more slots than pooled positions in a tile, and one or two
    assert any(r["nslots"] == 256 and r["nslots"] > r["slot_positions"] for r in rows) and any(r["nslots"] in (1, 2) for r in rows)
    # n_serial is what the comment says at the two extremes
    assert cc.n_serial_gram(5, 8, 3300) == 2 * 2 + 9 and cc.n_serial_moments_mfma(1, 408, 8) == 16 * 102 + 2
    assert cc.n_serial_rgrad(2, 1, 8, 12, 4) == 2 * 1 * 1 + 1 + 256 and cc.n_serial_rgrad(5, 4, 8, 3300, 64) == 2 * 8 * 2 + 3


def test_locate_names_the_workgroup_of_a_pooled_row():
    import torch
    c = cc.case("walk-1ch")                                   # 825 tiles per sequence on 2048 workgroups
    assert cc.locate(c, 0, 0) == dict(tile=0, wg=0, visit=0, visits=3, tile8=0, wg8=0, visit8=0, wave8=0)
    w = cc.locate(c, 2, 799)                                  # sequence 2, rows 1598 / 1599: tile 2 * 825 + 399 = 2049: the second visit of workgroup 1
    assert (w["tile"], w["wg"], w["visit"]) == (2049, 1, 1) and (w["tile8"], w["wave8"]) == (2 * 413 + 199, 3)
    w = cc.locate(c, 4, 1649)
    assert (w["tile"], w["wg"], w["visit"]) == (4124, 28, 2)  # the last tile: a third visit
    err = torch.zeros(5, 1650, 8, 16)
    err[2, 799, 3, 5] = float("nan")
    assert "(2, 799, 3, 5): 4-row tile 2049 = visit 1 (of 3) of workgroup 1" in cc.worst(c, err, "x")
    assert cc.locate(cc.case("walk-pool51"), 1, 5)["tile"] == 688 + 1


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_float64_reference_alone_leaves_out_fewer_near_ties_than_the_cap(name):
    r = cc.ref_forward(name)
    share = float(r["near"].double().mean())
    print(f"{name}: near-ties in float64 {share:.2e} of {r['near'].numel()}")
    assert share <= cc.TIE_CAP / 2                            # half the cap: the device may see a few more on its side of the bound
    if "bit" in r:
        assert 0.3 < float(r["bit"].double().mean()) < 0.7
    else:
        codes = set(r["code"].unique().tolist())
        assert codes == set(range(0, 1 + cc.case(name)["pool"][0] * cc.case(name)["pool"][1]))


def test_reference_moments_are_the_sums_their_names_say():
    import torch
    x = cc.inputs("scalar-3ch-odd")["x"]
    m, a = cc.ref_moments(x)
    nk = 27
    assert m.numel() == a.numel() == cc.moments_doubles(3) and bool((a >= m.abs() - 1e-9).all())
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1))
    B, Cin, F, T = x.shape
    v = lambda k: xp[:, k % Cin, (k // Cin) // 3:(k // Cin) // 3 + F, (k // Cin) % 3:(k // Cin) % 3 + T]      # k = (kh * 3 + kw) * Cin + ci
    for k, k2 in ((0, 0), (4, 17), (26, 26), (3, 5)):
        idx = nk + k * nk - (k * (k - 1)) // 2 + (k2 - k)
        assert abs(float(m[idx]) - float((v(k) * v(k2)).sum())) < 1e-9 * float(a[idx])
        assert abs(float(m[k]) - float(v(k).sum())) < 1e-9 * float(a[k])
