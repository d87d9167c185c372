"""A Python restatement of wgrad_plan (conv.hip) and of how each 3x3 weight-gradient kernel hands tiles to workgroups, shared by
test_cpu_wgrad_plan.py (which proves that every case below is in the regime its row claims) and test_gpu_wgrad_tiles.py (which
runs them).  Nothing here calls the library: if the tiling is retuned, the workspace check of the CPU test fails and this file
and the table are revisited together.

Layouts: x channels-last [B,T,F,Cin] or NCHW [B,Cin,F,T], dy [B,T,F,Cout], dw [Cout,Cin,3,3] with tap = kh*3 + kw, kh along
mel (F), kw along time (T).  A tile is TT time rows x FT mel columns; tile index = (b * tblocks + tb) * nft + mel."""
from collections import namedtuple

import numpy as np

WG_FT, WG_NX = 40, 6                       # conv.hip: widest mel tile of conv3x3_mfma_wgrad_k, its DMA items per thread
SED_WGRAD_ZERO_ROW_CLEAN, SED_WGRAD_DIRECT = 0x100, 0x200      # include/sedcrnn.h

Plan = namedtuple("Plan", "kind v2 mode TT FT nft tblocks ntiles ngroups per busy slab_comps slab_floats zrow_floats walk")


def cdiv(a, b):
    return -(-a // b)


def _bf16x3_lds(TT, FT):
    HR, MPAD = (TT + 2) * (FT + 2), cdiv(TT * FT, 16) * 16
    if HR * 8 > 256 * 8 or MPAD * 32 > 256 * 14:
        return 1 << 30
    return 2 * (HR * 128 + MPAD * 640)


def wgrad_plan(B, Cin, F, T, Cout, nchw, mode=0):
    """mode: 0 or 1 (the flag bits are stripped before the plan is made, as the entry does)"""
    mode &= ~(SED_WGRAD_ZERO_ROW_CLEAN | SED_WGRAD_DIRECT)
    kind = 1 if (not nchw and Cin % 32 == 0 and Cout % 128 == 0) else 0
    v2, FT, nft = 0, F, 1
    if kind == 1:
        nft = cdiv(F, WG_FT)
        FT = cdiv(F, nft)
        FT += FT & 1
        TT = 2
        while TT + 2 <= 62 and TT + 2 <= T + (T & 1) and (TT + 2) * FT <= 2 * WG_FT and (TT + 4) * (FT + 2) * 8 <= 256 * WG_NX:
            TT += 2
        if mode == 0 and T >= 2:
            ft = 40 if (F % 8 == 0 and cdiv(F, 40) * 40 == F) else (32 if (F % 8 == 0 and cdiv(F, 32) * 32 == F) else 0)
            if ft:
                v2, FT, nft, TT = 1, ft, F // ft, 2
        if mode == 1:
            TT = 1
            while TT + 1 <= 62 and TT + 1 <= T and _bf16x3_lds(TT + 1, FT) <= 160 * 1024:
                TT += 1
    else:
        TT = min(4, T)
    tblocks = cdiv(T, TT)
    ntiles = B * tblocks * nft
    ngroups = min(ntiles, 64 if kind == 1 else 1024)
    per = cdiv(ntiles, ngroups)                         # tiles of the busiest group
    # the position-contiguous kernel walks contiguous runs of `per` tiles (trailing groups stay empty), the others stride by the grid
    walk = "run" if v2 else "stride"
    busy = cdiv(ntiles, per) if v2 else ngroups
    comps = 16 if v2 else 9                             # the workspace holds the Winograd form's 16 components for every v2 shape
    zrow = cdiv((FT + 4) * max(Cin, Cout) + 64, 64) * 64 if v2 else 0
    return Plan(kind, v2, mode, TT, FT, nft, tblocks, ntiles, ngroups, per, busy, comps, ngroups * comps * Cin * Cout, zrow, walk)


def workspace_bytes(B, Cin, F, T, Cout):
    """sed_conv3x3_wgrad_workspace_bytes: the larger slab area of the channels-last and the NCHW plan, behind the zero row"""
    a, b = wgrad_plan(B, Cin, F, T, Cout, False), wgrad_plan(B, Cin, F, T, Cout, True)
    return (max(a.slab_floats, b.slab_floats) + a.zrow_floats) * 4


def group_tiles(p, g):
    """the tiles workgroup g walks, in its order"""
    if p.walk == "run":
        return list(range(g * p.per, min((g + 1) * p.per, p.ntiles)))
    return list(range(g, p.ntiles, p.ngroups))


def tile_coords(p, tile):
    b, rem = divmod(tile, p.tblocks * p.nft)
    tb, mel = divmod(rem, p.nft)
    return b, tb, mel


def group_of(p, tile):
    return tile // p.per if p.walk == "run" else tile % p.ngroups


def regime(p, T):
    """what the walk of this plan reaches (the properties the table's rows claim)"""
    runs = [group_tiles(p, g) for g in range(p.ngroups)]
    steps = [(tile_coords(p, a), tile_coords(p, b)) for r in runs for a, b in zip(r, r[1:])]
    return {
        "empty_groups": sum(1 for r in runs if not r),
        "max_tiles": max(len(r) for r in runs),
        "groups_with_max": sum(1 for r in runs if len(r) == p.per),
        "ragged_last_run": p.walk == "run" and p.ntiles % p.per != 0,
        # contiguous walk only: a run steps from the last tile of sequence b to the first tile of b + 1 / over the end of a mel row
        "crosses_sequence": p.walk == "run" and any(a[0] != b[0] for a, b in steps),
        "crosses_mel_row": p.walk == "run" and any(a[0] == b[0] and a[1] != b[1] and a[2] == p.nft - 1 and b[2] == 0 and p.nft > 1 for a, b in steps),
        "start_mels": sorted({tile_coords(p, r[0])[2] for r in runs if r}),
        "ragged_last_time_tile": T % p.TT != 0,
    }


# ───────────────────────── the cases ─────────────────────────
# name, (B, Cin, F, T, Cout), x given as NCHW, the kernel the entry picks, and what the row claims: fields of the plan and of
# regime(), each asserted by test_cpu_wgrad_plan.py
def _c(name, shape, nchw, kernel, **claims):
    return dict(name=name, shape=shape, nchw=nchw, kernel=kernel, claims=claims)


CASES = [
    _c("w40_seq_step", (4, 32, 40, 42, 128), False, "wgrad2<40>", ntiles=84, per=2, busy=42, empty_groups=22, crosses_sequence=True),
    _c("w40_odd_t_4ci", (3, 128, 40, 43, 128), False, "wgrad2<40>", ntiles=66, per=2, busy=33, ragged_last_time_tile=True),
    _c("w40_per3_2co", (5, 32, 40, 54, 256), False, "wgrad2<40>", ntiles=135, per=3, busy=45),
    _c("w40_nft5", (1, 32, 200, 28, 128), False, "wgrad2<40>", ntiles=70, per=2, busy=35, crosses_mel_row=True),
    _c("w40_nft2", (3, 32, 80, 30, 128), False, "wgrad2<40>", ntiles=90, per=2, busy=45),
    # not in the issue's table: a last run of ONE tile, and a run that steps into the next sequence behind an odd-T tile
    _c("w40_ragged_run", (3, 32, 40, 45, 128), False, "wgrad2<40>", ntiles=69, per=2, busy=35, ragged_last_run=True, crosses_sequence=True,
       ragged_last_time_tile=True),
    _c("w32_per3_nft2", (3, 32, 64, 46, 128), False, "wgrad2<32>", ntiles=138, per=3, busy=46, start_mels=[0, 1], crosses_sequence=True,
       crosses_mel_row=True),
    _c("w32_nft4", (1, 128, 128, 36, 128), False, "wgrad2<32>", ntiles=72, per=2, busy=36, crosses_mel_row=False),
    _c("w32_odd_t", (5, 32, 32, 27, 128), False, "wgrad2<32>", ntiles=70, per=2, busy=35, ragged_last_time_tile=True),
    _c("w32_ragged_run", (3, 32, 32, 45, 128), False, "wgrad2<32>", ntiles=69, per=2, busy=35, ragged_last_run=True, crosses_sequence=True),
    _c("mfma_tt4", (3, 32, 20, 90, 128), False, "mfma_wgrad<false>", ntiles=69, TT=4, max_tiles=2, groups_with_max=5, ragged_last_time_tile=True),
    _c("mfma_tall", (2, 32, 8, 330, 128), False, "mfma_wgrad<false>", ntiles=66, TT=10, max_tiles=2, groups_with_max=2),
    _c("mfma_t1", (66, 32, 40, 1, 128), False, "mfma_wgrad<false>", ntiles=66, TT=2, max_tiles=2, groups_with_max=2, ragged_last_time_tile=True),
    _c("mfma_mt_ragged", (2, 32, 50, 34, 128), False, "mfma_wgrad<true>", ntiles=68, FT=26, nft=2, max_tiles=2, groups_with_max=4),
    _c("mfma_mt_4", (1, 64, 130, 46, 128), False, "mfma_wgrad<true>", ntiles=92, FT=34, nft=4, max_tiles=2, groups_with_max=28),
    _c("small_cin1", (5, 1, 8, 824, 8), True, "small", ntiles=1030, max_tiles=2, groups_with_max=6),
    _c("small_c2", (3, 2, 40, 1370, 8), True, "small_c<2>", ntiles=1029, max_tiles=2, groups_with_max=5, ragged_last_time_tile=True),
    _c("small_c3", (2, 3, 12, 2052, 16), True, "small_c<3>", ntiles=1026, max_tiles=2, groups_with_max=2),
    _c("small_c4_cl", (2, 4, 8, 2052, 32), False, "small_c<4>", ntiles=1026, max_tiles=2, groups_with_max=2),
    _c("small_cin16", (2, 16, 8, 2052, 16), False, "small", ntiles=1026, max_tiles=2, groups_with_max=2),
]
BF16X3_CASE = "w40_per3_2co"                # also runs with mode 1: 135 tiles of 2 x 40 on 64 groups, groups 0-6 take three


def case(name):
    return next(c for c in CASES if c["name"] == name)


def case_modes(c):
    """the modes a case runs with: (label, mode bits)"""
    if c["kernel"].startswith("wgrad2"):
        m = [("wino", 0), ("direct", SED_WGRAD_DIRECT)]
        if c["name"] == BF16X3_CASE:
            m.append(("bf16x3", 1))
        return m
    return [("plain", 0)]


RUNS = [(c["name"], label) for c in CASES for label, _ in case_modes(c)]


def mode_bits(name, label):
    return dict(case_modes(case(name)))[label]


def plan_for(c, mode=0):
    B, Cin, F, T, Cout = c["shape"]
    return wgrad_plan(B, Cin, F, T, Cout, c["nchw"], mode)


def exactness_bound(c):
    """16 * B*T*F * 4: integers in [-2, 2] give direct products <= 4 and Winograd-domain products <= 8 * 8 = 16 * 4, summed over
    B*T*F positions (one Winograd tile per four of them), and the halves of G make every quantity a multiple of 1/4"""
    B, _, F, T, _ = c["shape"]
    return 16 * B * T * F * 4


# ───────────────────────── attribution of a wrong entry to a group and a tile ─────────────────────────
G_WINO = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])


def tile_contributions(p, x_cl, dy, co, ci, tap):
    """float64 contribution of every tile to dw[co][ci][tap]; x_cl [B,T,F,Cin], dy [B,T,F,Cout] (numpy) -> [ntiles]"""
    B, T, F, _ = x_cl.shape
    kh, kw = divmod(tap, 3)
    xp = np.zeros((B, T + 2, F + 2))
    xp[:, 1:-1, 1:-1] = x_cl[..., ci]
    prod = xp[:, kw:kw + T, kh:kh + F] * dy[..., co].astype(np.float64)
    full = np.zeros((B, p.tblocks * p.TT, p.nft * p.FT))
    full[:, :T, :F] = prod
    return full.reshape(B, p.tblocks, p.TT, p.nft, p.FT).sum((2, 4)).reshape(-1)


def slab_entry(p, slabs, kernel, wino, Cin, Cout, co, ci, tap):
    """what each group's slab holds for dw[co][ci][tap] -> float64 [ngroups]; slabs: the float32 area behind the zero row"""
    g = p.ngroups
    if kernel.startswith("small"):
        return slabs[:g * Cin * 9 * Cout].reshape(g, Cin, 9, Cout)[:, ci, tap, co].astype(np.float64)
    if not wino:
        return slabs[:g * 9 * Cin * Cout].reshape(g, 9, Cin, Cout)[:, tap, ci, co].astype(np.float64)
    u = slabs[:g * 16 * Cin * Cout].reshape(g, 4, 4, Cin, Cout)[:, :, :, ci, co].astype(np.float64)     # [g][xi][nu]
    s = np.array([1., 1., 1., -1.])
    u = u * s[None, :, None] * s[None, None, :]
    kh, kw = divmod(tap, 3)
    return np.einsum("gxn,x,n->g", u, G_WINO[:, kw], G_WINO[:, kh])


def attribute(p, c, wino, x_cl, dy, dw, ref, slabs, top=4):
    """lines that name, for the worst entries of dw, the groups whose slab differs from the float64 sum of their tiles and the
    tile(s) of that group whose contribution explains the difference (dropped: -c, counted twice: +c)"""
    _, Cin, _, _, Cout = c["shape"]
    dw, ref = dw.reshape(Cout, Cin, 9), ref.reshape(Cout, Cin, 9)
    err = np.abs(dw.astype(np.float64) - ref)
    err[~np.isfinite(err)] = np.inf
    lines = [f"{c['name']} ({c['kernel']}{', Winograd form' if wino else ''}): {int((err > 0).sum())} of {err.size} entries differ; "
             f"{p.ntiles} tiles of {p.TT}x{p.FT} on {p.ngroups} groups ({p.walk}, up to {p.per} per group, {p.busy} busy)"]
    for flat in np.argsort(-err.reshape(-1), kind="stable")[:top]:
        co, ci, tap = np.unravel_index(flat, (Cout, Cin, 9))
        if err[co, ci, tap] == 0:
            break
        lines.append(f"  dw[co={co}][ci={ci}][tap={tap} (kh={tap // 3}, kw={tap % 3})] = {dw[co, ci, tap]!r}, float64 {ref[co, ci, tap]!r}")
        contrib = tile_contributions(p, x_cl, dy, co, ci, tap)
        got = slab_entry(p, slabs, c["kernel"], wino, Cin, Cout, co, ci, tap)
        for g in range(p.ngroups):
            tiles = group_tiles(p, g)
            want = float(contrib[tiles].sum()) if tiles else 0.0
            if got[g] == want:
                continue
            d = got[g] - want
            hit = [f"tile {t} (b, time block, mel tile = {tile_coords(p, t)}) {'dropped' if contrib[t] == -d else 'counted twice'}"
                   for t in tiles if contrib[t] != 0 and abs(contrib[t]) == abs(d)]
            lines.append(f"    group {g} tiles {tiles}: slab {got[g]!r}, its tiles sum to {want!r}, difference {d!r}"
                         + ("; " + ", ".join(hit) if hit else "; no single tile of the group explains it (a halo row?): per tile "
                            + str([(t, tile_coords(p, t), float(contrib[t])) for t in tiles])))
    return lines
