"""The Winograd kernel's prologue index math on the host (no GPU needed): sed_internal_wino_patch_offsets[_grid] run the kernel's own
helpers (wino.hip: wino_workgroup, WinoWalk — reciprocal multiplies for the workgroup mapping, one decode + a carry per KiB block
for the 14 patch-DMA offsets) for every workgroup, wave and lane of a launch.  Reference: the closed form the kernel used before —
integer division and remainder per position, restated here with // and % — which is what every lane has to end up with, padding
lanes (0x80000000) included.  Exhaustive over the geometries: a carry bug shows at one (F2, wave, lane) and nowhere else."""
import ctypes as C

import numpy as np
import pytest

from sed_crnn_amd import _lib

CIN, NH, OOB = 128, 14, 0x80000000
FS = [2, 4, 6, 14, 30, 40, 62, 64, 128]        # F2 below, equal to and above 32, several wraps per block, two column groups at 128
TS = [2, 4, 6, 10, 64]
BS = [1, 3, 8, 9, 16]                          # both branches of the XCD-ordered mapping
COUTS = [64, 128]


def cdiv(a, b):
    return -(-a // b)


def geometry(F, T):
    """wino_geo's column groups and tile rows per block (the shapes here all fit: sed_conv3x3_wino_rows says which do)"""
    Tw = T // 2
    ncg = 1
    while ncg <= 8:
        if (F // 2) % ncg:
            return None
        Fw = F // 2 // ncg
        ntile = Fw * Tw
        nblk = cdiv(ntile, 64)
        TR = max(min(blk * 64 + 63, ntile - 1) // Fw - (blk * 64) // Fw + 1 for blk in range(nblk))
        F2 = 2 * Fw + 2
        HR = (2 * TR + 2) * F2
        if cdiv(cdiv(HR, 8), 4) <= NH:
            return dict(ncg=ncg, Fw=Fw, nblk=nblk, TR=TR, F2=F2, H2=F2 // 2, HR=HR)
        ncg *= 2
    return None


def reference_offsets(g, F, T, blka):
    """[4 waves][64 lanes][14] offsets of block x column group `blka`: the former closed form, position by position"""
    blk, cgp = blka // g["ncg"], blka % g["ncg"]
    fg0 = 2 * cgp * g["Fw"]
    ty0 = (blk * 64) // g["Fw"]
    wave = np.arange(4).reshape(4, 1, 1)
    lane = np.arange(64).reshape(1, 64, 1)
    u = np.arange(NH).reshape(1, 1, NH)
    Q, pp = lane >> 3, lane & 7
    P = (u * 4 + wave) * 8 + pp
    tt, cx = P // g["F2"], P % g["F2"]
    ff = np.where(cx < g["H2"], 2 * cx, 2 * (cx - g["H2"]) + 1)
    t, f = 2 * ty0 - 1 + tt, fg0 + ff - 1
    ok = (P < g["HR"]) & (t >= 0) & (t < T) & (f >= 0) & (f < F)
    off = ((t * F + f) * CIN + Q * 4) * 4
    return np.where(ok, off, OOB).astype(np.uint32)


def reference_map(g, B, ncoh, bx, by):
    nba = g["nblk"] * g["ncg"]
    if B & 7 == 0:
        idx = by * (nba * ncoh) + bx
        xcd, j = idx & 7, idx >> 3
        coh, jj = j % ncoh, j // ncoh
        return xcd + 8 * (jj // nba), jj % nba, coh
    return by, bx // ncoh, bx % ncoh


@pytest.fixture(scope="module")
def entries():
    L = _lib.lib()
    one = L.sed_internal_wino_patch_offsets
    one.restype, one.argtypes = C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_uint), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    grid = L.sed_internal_wino_patch_offsets_grid
    grid.restype, grid.argtypes = C.c_int, [C.c_int] * 4 + [C.c_void_p, C.c_void_p]
    return L, one, grid


@pytest.mark.parametrize("F", FS)
def test_every_lane_of_every_workgroup(entries, F):
    L, one, grid = entries
    seen = 0
    for T in TS:
        g = geometry(F, T)
        for Cout in COUTS:
            for B in BS:
                rows = L.sed_conv3x3_wino_rows(B, CIN, F, T, Cout)
                if rows == 0:
                    continue
                assert g is not None and rows == B * g["nblk"] * g["ncg"], (B, F, T, Cout)
                ncoh, nba = Cout // 64, g["nblk"] * g["ncg"]
                gx = nba * ncoh
                out = np.empty((B, gx, 4, 64, NH), dtype=np.uint32)
                mp = np.empty((B, gx, 3), dtype=np.int32)
                assert grid(B, F, T, Cout, out.ctypes.data, mp.ctypes.data) == 0, L.sed_last_error_string()
                want_map = np.array([[reference_map(g, B, ncoh, bx, by) for bx in range(gx)] for by in range(B)], dtype=np.int32)
                assert np.array_equal(mp, want_map), (B, F, T, Cout)
                # every (sequence, block, channel half) is some workgroup's, once
                assert len({tuple(m) for m in want_map.reshape(-1, 3)}) == B * gx
                ref = np.stack([reference_offsets(g, F, T, blka) for blka in range(nba)])
                want = ref[mp[..., 1]]
                bad = np.argwhere(out != want)
                assert bad.size == 0, f"B={B} F={F} T={T} Cout={Cout}: (block_y, block_x, wave, lane, u) = {bad[0].tolist()}: " \
                                      f"{int(out[tuple(bad[0])]):#x} instead of {int(want[tuple(bad[0])]):#x}"
                seen += 1
    assert seen > 0, f"no geometry with F={F} was accepted"


def test_single_lane_entry_agrees_with_the_grid_form(entries):
    L, one, grid = entries
    B, F, T, Cout = 8, 40, 10, 128
    g = geometry(F, T)
    gx = g["nblk"] * g["ncg"] * (Cout // 64)
    out = np.empty((B, gx, 4, 64, NH), dtype=np.uint32)
    mp = np.empty((B, gx, 3), dtype=np.int32)
    assert grid(B, F, T, Cout, out.ctypes.data, mp.ctypes.data) == 0
    hp = (C.c_uint * NH)()
    b, blka, coh = C.c_int(), C.c_int(), C.c_int()
    for by, bx, wave, lane in [(0, 0, 0, 0), (7, gx - 1, 3, 63), (3, 1, 2, 17), (5, gx // 2, 1, 40)]:
        assert one(B, F, T, Cout, bx, by, wave, lane, hp, C.byref(b), C.byref(blka), C.byref(coh)) == 0
        assert list(hp) == out[by, bx, wave, lane].tolist()
        assert [b.value, blka.value, coh.value] == mp[by, bx].tolist()
    assert one(B, F, T, Cout, gx, 0, 0, 0, hp, C.byref(b), C.byref(blka), C.byref(coh)) < 0          # outside the launch
    assert one(B, 41, T, Cout, 0, 0, 0, 0, hp, C.byref(b), C.byref(blka), C.byref(coh)) < 0          # a shape the kernel refuses


def test_reciprocal_division_at_large_indices(entries):
    """the mapping divides by reciprocal multiplication, exact below 2^31: a batch large enough that the workgroup index passes 2^20
    (where the kernel's float reciprocal would no longer be exact) still maps every sampled workgroup as // and % do"""
    L, one, grid = entries
    B, F, T, Cout = 1200000, 6, 4, 192          # B a multiple of 8: XCD-ordered; 3 channel parts; B T F 128 < 2^32
    assert L.sed_conv3x3_wino_rows(B, CIN, F, T, Cout) > 0
    g = geometry(F, T)
    ncoh = Cout // 64
    gx = g["nblk"] * g["ncg"] * ncoh
    assert B * gx > 1 << 20
    hp = (C.c_uint * NH)()
    b, blka, coh = C.c_int(), C.c_int(), C.c_int()
    rng = np.random.default_rng(0)
    picks = [(B - 1, gx - 1), (B - 1, 0), (B // 2, gx // 2)] + [(int(rng.integers(B)), int(rng.integers(gx))) for _ in range(2000)]
    for by, bx in picks:
        assert one(B, F, T, Cout, bx, by, 1, 9, hp, C.byref(b), C.byref(blka), C.byref(coh)) == 0
        assert (b.value, blka.value, coh.value) == reference_map(g, B, ncoh, bx, by), (by, bx)
        assert list(hp) == reference_offsets(g, F, T, blka.value)[1, 9].tolist()
