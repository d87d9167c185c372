"""The shapes test_gpu_wino_eval.py runs really are in the regimes their rows claim.  wino_cases.py restates wino_geo (csrc/wino.hip);
here the restatement is held against sed_conv3x3_wino_rows (host-only: the row count every Winograd launch allocates by) on a
dense grid, every row of the table against the regime it names, and the integer inputs of the exact GPU test are shown to be
exact in float32: a numpy float32 emulation of the whole folded Winograd chain equals the float64 reference bit for bit.  No GPU."""
import numpy as np
import pytest

import wino_cases as wc  # noqa: E402

GRID_T = list(range(2, 131, 2)) + [256, 512, 1024]


@pytest.fixture(scope="module")
def L():
    from sed_crnn_amd import _lib
    return _lib.lib()


def test_restated_geometry_equals_the_library_on_a_dense_grid(L):
    """every even F in 2..512 x every even T in 2..130 and 256, 512, 1024, batches of 1, 3, 8, 64 / 128 / 256 output channels:
    rows == B * nblk * ncg, and 0 exactly where the restatement refuses"""
    taken = refused = 0
    groups = set()
    for F in range(2, 513, 2):
        for T in GRID_T:
            for B in (1, 3, 8):
                for Cout in (64, 128, 256):
                    g = wc.wino_geo(B, 128, F, T, Cout)
                    got = L.sed_conv3x3_wino_rows(B, 128, F, T, Cout)
                    assert got == (B * g["nblk"] * g["ncg"] if g else 0), (B, F, T, Cout, got, g)
            if g:
                taken += 1
                groups.add(g["ncg"])
                assert g["NH"] <= wc.WN_NHMAX and g["TR"] <= g["Tw"] and g["ncg"] * g["Fw"] * 2 == F
            else:
                refused += 1
    assert groups == {1, 2, 4, 8} and taken > 0 and refused > 0          # both answers and every group count occur
    print(f"{taken} of {taken + refused} even (F, T) taken, {refused} refused")


def test_what_the_geometry_refuses_off_the_grid(L):
    """odd sizes, other channel counts, the 32-bit limits of the patch DMA: the same answer from both"""
    for B, Cin, F, T, Cout in [(2, 128, 41, 8, 128), (2, 128, 40, 7, 128), (2, 64, 40, 8, 128), (2, 128, 40, 8, 96), (0, 128, 40, 8, 128),
                               (2, 128, 0, 8, 128), (2, 128, 40, 0, 128), (2, 128, 40, 8, 0), (1, 128, 2048, 2048, 64), (1, 128, 512, 8192, 64),
                               (16, 128, 512, 4096, 64), (1, 128, 512, 4096, 64), (1, 128, 512, 4096, 512), (2, 128, 40, 8, 320)]:
        assert L.sed_conv3x3_wino_rows(B, Cin, F, T, Cout) == wc.wino_rows(B, Cin, F, T, Cout), (B, Cin, F, T, Cout)
    for F, T in wc.REFUSED:
        assert F % 2 == 0 and T % 2 == 0 and wc.regime(F, T) is None and L.sed_conv3x3_wino_rows(3, 128, F, T, 128) == 0
        # ... because the row of F / 2 tiles does not fit one block's patch and cannot be halved (again)
        half = F // 2
        while half % 2 == 0:
            half //= 2
        assert half > 1 and wc.regime(F, 2) is not None


@pytest.mark.parametrize("name", [c["name"] for c in wc.CASES])
def test_row_is_in_the_regime_its_name_claims(L, name):
    c = wc.case(name)
    got = wc.regime(c["F"], c["T"])
    assert got == c["claims"], (name, dict(zip(wc.REGIME_KEYS, got)) if got else None)
    for B in (1, wc.B_PLAIN, wc.B_XCD):
        for Cout in (64, 128, 192, 256):
            want = 0 if got is None else B * got[2] * got[0]
            assert L.sed_conv3x3_wino_rows(B, 128, c["F"], c["T"], Cout) == want


def test_the_table_covers_what_the_epilogue_addressing_can_get_wrong():
    reg = {c["name"]: c["claims"] for c in wc.CASES if c["claims"]}
    assert {r[0] for r in reg.values()} == {1, 2, 4, 8}                                   # every number of column groups
    assert any(r[4] == wc.WN_NHMAX for r in reg.values())                                 # the patch at the LDS limit
    assert any(r[1] % 2 == 1 and r[0] > 1 for r in reg.values())                          # an odd tile row inside a column group
    assert any(r[2] > 1 and 64 % r[1] for r in reg.values())                              # blocks that start in the middle of a tile row
    assert any(r[5] < 32 for r in reg.values()) and any(r[5] == 64 for r in reg.values())  # a last block with an empty m-tile, a full one
    assert reg["same-F-one-group"][0] == 1 and reg["same-F-two-groups"][0] == 2           # the group count depends on T too
    assert wc.case("same-F-one-group")["F"] == wc.case("same-F-two-groups")["F"]
    assert reg["tallest"][3] == 32 and reg["tallest"][5] == 64                            # 32 tile rows in one block
    # a few seconds per case: the largest float64 reference of the grid rows
    assert max(wc.B_XCD * wc.case(n)["F"] * wc.case(n)["T"] for n in wc.GRID_ROWS) <= 8 * 192 * 16
    assert wc.case(wc.LONG[0])["F"] * wc.case(wc.LONG[0])["T"] == 20480
    assert len(wc.RUNS) == len(wc.GRID_ROWS) + 9 and len(set(wc.RUNS)) == len(wc.RUNS)


def test_locate_names_the_workgroup_of_an_output_element():
    g = wc.wino_geo(3, 128, 48, 16, 128)                     # two groups of 12 tiles, 8 tile rows: 96 tiles, two blocks per group
    seen = {}
    for t in range(8):
        for f in range(48):
            w = wc.locate(g, t, f, 70)
            assert w["half"] == 1 and w["group"] == f // 24 and w["tile"] == t * 12 + (f % 24) // 2 and w["block"] == w["tile"] // 64
            seen.setdefault((w["block"], w["group"]), set()).add(w["slot"])
    assert {k: len(v) for k, v in seen.items()} == {(0, 0): 64, (0, 1): 64, (1, 0): 32, (1, 1): 32}
    ref = np.zeros((2, 8, 48, 128))
    got = ref.copy()
    got[1, 6, 30, 5] = np.nan
    text = wc.first_difference(got, ref, g)
    assert "(1, 6, 30, 5)" in text and "tile 75 " in text and "slot 11 of block 1, column group 1 of 2, channel half 0" in text and "(1 NaN)" in text


# ───────────────────────── the integer inputs are exact in float32 ─────────────────────────
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float32)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float32)


def _is_pow2_or_zero(v):
    m, _ = np.frexp(np.abs(v))
    return bool(np.all((v == 0) | (m == 0.5)))


def test_the_bound_of_the_integer_inputs_is_below_2_to_the_24():
    assert wc.exactness_bound() == 9 * 128 * 144 * 8 + 16 * 18 < 2 ** 24
    assert set(wc.GAMMAS) == {-2, -1, -0.5, 0, 0.5, 1, 2} and set(wc.VARS) == {0.25, 1, 4}
    for name, Cout in wc.RUNS + [wc.LONG]:
        c = wc.case(name)
        d = wc.int_inputs(c["F"], c["T"], Cout, B=1)
        assert np.abs(d["x"]).max() <= wc.X_MAX and np.abs(d["w"]).max() <= wc.W_MAX and d["eps"] == 0.0
        assert all(np.array_equal(d[k], np.round(d[k])) and np.abs(d[k]).max() <= wc.P_MAX for k in ("bias", "beta", "rm"))
        for h in range(Cout // 64):
            assert set(d["gamma"][h * 64:(h + 1) * 64]) == set(wc.GAMMAS)                # gamma = 0 and < 0 in every channel half
        sc = d["gamma"] / np.sqrt(d["rv"])
        assert _is_pow2_or_zero(sc) and np.abs(sc).max() <= 4 and np.abs(sc[sc != 0]).min() >= 0.25
        u = np.einsum("xa,oiab,yb->oixy", G.astype(np.float64), d["w"] * sc[:, None, None, None], G.astype(np.float64))
        assert np.array_equal(u * 16, np.round(u * 16)) and np.abs(u * 16).max() <= 144  # every transformed weight: a multiple of 1/16


def _emulate_f32(d):
    """fold -> G g G^T -> B^T d B -> sum over 128 channels -> A^T M A -> + bias -> max -> relu, every array float32;
    -> [B][T/2][F][Cout] and the largest |value| * 16 any stage held"""
    f32 = np.float32
    x, w = d["x"].astype(f32), d["w"].astype(f32)
    gamma, beta, rm, rv, bias = (d[k].astype(f32) for k in ("gamma", "beta", "rm", "rv", "bias"))
    sc = gamma / np.sqrt(rv + f32(d["eps"]))
    bias_f = bias * sc + (beta - rm * sc)
    u = np.einsum("xa,oiab,yb->oixy", G, w * sc[:, None, None, None], G)
    B, Ci, F, T = x.shape
    xp = np.zeros((B, Ci, F + 2, T + 2), dtype=f32)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.empty((B, T // 2, F, w.shape[0]), dtype=f32)
    big = float(np.abs(u).max())
    for n in range(F // 2):
        for m in range(T // 2):
            v = np.einsum("xa,biac,yc->bixy", BT, xp[:, :, 2 * n:2 * n + 4, 2 * m:2 * m + 4], BT)
            M = np.einsum("oixy,bixy->boxy", u, v)
            y = np.einsum("px,boxy,qy->bopq", AT, M, AT) + bias_f[None, :, None, None]
            assert u.dtype == v.dtype == M.dtype == y.dtype == f32
            big = max(big, float(np.abs(v).max()), float(np.abs(M).max()), float(np.abs(y).max()))
            out[:, m, 2 * n:2 * n + 2, :] = np.maximum(np.maximum(y[..., 0], y[..., 1]), f32(0)).transpose(0, 2, 1)
    return out, big * 16


@pytest.mark.parametrize("name,Cout", [("odd-row-ragged", 128), ("one-tile", 64)])
def test_float32_emulation_of_the_folded_winograd_chain_equals_float64_bit_for_bit(name, Cout):
    c = wc.case(name)
    d = wc.int_inputs(c["F"], c["T"], Cout, B=2)
    got, big = _emulate_f32(d)
    assert big <= wc.exactness_bound() < 2 ** 24
    ref = wc.ref_pooled(d).numpy()
    assert got.dtype == np.float32 and ref.dtype == np.float64
    assert np.array_equal(got.astype(np.float64), ref), wc.first_difference(got.astype(np.float64), ref, wc.wino_geo(2, 128, c["F"], c["T"], Cout))
    assert (ref > 0).mean() > 0.2 and (ref == 0).mean() > 0.2            # both sides of the ReLU
    zero = d["gamma"] == 0
    want0 = np.maximum(d["beta"][zero], 0)                               # gamma = 0: relu(beta) everywhere
    assert zero.any() and np.array_equal(ref[..., zero], np.broadcast_to(want0, ref[..., zero].shape))
