"""The case table of the direct 3x3 conv MFMA kernel (conv3x3_mfma_fwd2_k, csrc/conv.hip), shared by test_cpu_conv_plan.py
(which holds the restatement below against sed_conv3x3_plan on a dense sweep and every row against that query) and
test_gpu_conv_tiles.py (which runs the rows).

Restated here in plain Python: conv_tile / conv_plan / conv_eval_plan (the block tile TT time rows x FT mel columns, the mel
tiles, the 32-wide output-channel tiles per workgroup), the statistic row a tile writes and the XCD-aware workgroup order.  The
table is not written by hand: it is enumerated from the restatement over F <= 256, T <= 128 (build_table), so a retuned
conv_tile moves the rows with it and the CPU test says which claims no longer hold.

A row: name, F, T, nct (4 / 2 / 1: Cout = 128 / 64 / 32), which (0: conv_plan, 1: the pooled inference plan) and what it claims:
tile (TT, FT), nft, tblocks, ragged_f (the last mel tile hangs over F), ragged_t (the last time block hangs over T).  Its kind
says why it is listed: "tile" (the smallest shape on that tile, ragged where one is near), "interior" (every tile wholly inside
the output and made of whole 32-row MFMA tiles: the epilogue's unchecked path), "grid" (three or more tiles per sequence).
"""
import functools

import numpy as np

CV_NH, CV_LD, CV_TPAD, CV_MTW, CV_CIC = 8, 36, 56, 5, 32
SWEEP_F, SWEEP_T = 256, 128
COUT_OF_NCT = {4: 128, 2: 64, 1: 32}
# one GPU case stays far below a second: at most this many output elements (B * T * F * Cout) in the largest batch a row runs at
MAX_OUT_ELEMS = 1 << 21
B_PLAIN, B_XCD = 3, 8                      # remap off / on (B % 8 == 0)


def cdiv(a, b):
    return -(-a // b)


def nct_of(Cout):
    return 4 if Cout % 128 == 0 else (2 if Cout % 64 == 0 else 1)


def limit_of(nct):
    """MFMA rows (output positions) a workgroup holds: CV_MTW 32-row tiles per wave, 4 / nct row parts"""
    return 32 * CV_MTW * (4 // nct)


# ───────────────────────── conv_tile ─────────────────────────
@functools.lru_cache(maxsize=None)
def _candidates(F, limit, pooled):
    """conv_tile's loops without T: (TT, FT, nf, tile fill x mel coverage, halo discount) in the order the loops visit them"""
    out, last = [], -1
    for nft in range(1, F + 1):
        FT = cdiv(F, nft)
        FT += FT & 1
        if FT == last:
            continue
        last = FT
        nf = cdiv(F, FT)
        tt_max = 64 if nft == 1 else 8
        for TT in range(1, tt_max + 1):
            if TT * FT > limit or (TT + 2) * (FT + 2) * 8 > 256 * CV_NH:
                continue
            if pooled and ((TT & 1) or FT > 32):
                continue
            if TT > 8 and 2 * (TT + 2) * ((FT + 2) * CV_LD + CV_TPAD) * 4 > 80 * 1024:
                continue
            out.append((TT, FT, nf, ((TT * FT) / limit) * (F / (nf * FT)), 1.0 + 0.25 * (((TT + 2) * (FT + 2)) / (TT * FT) - 1.0)))
        if FT <= 2:
            break
    return tuple(out)


def conv_tile(F, T, limit, pooled=False):
    """-> (TT, FT, nft, score) or None: the first candidate of the best score (the C loop replaces on `>` only)"""
    best, res = -1.0, None
    for TT, FT, nf, fill_cov, halo in _candidates(F, limit, pooled):
        if TT > T:
            continue
        score = (fill_cov * (T / (cdiv(T, TT) * TT))) / halo
        if score > best:
            best, res = score, (TT, FT, nf, score)
    return res if best > 0.0 else None


def tile_sweep(limit, pooled=False, Fmax=SWEEP_F, Tmax=SWEEP_T):
    """conv_tile for every F <= Fmax, T <= Tmax at once -> TT, FT, nft (int arrays [Fmax + 1][Tmax + 1], TT = 0: no tile) and
    the score; the same double-precision operations in the same order, numpy's argmax takes the first of equal scores"""
    TTs, FTs, NFs = (np.zeros((Fmax + 1, Tmax + 1), dtype=np.int64) for _ in range(3))
    SC = np.full((Fmax + 1, Tmax + 1), -1.0)
    Ts = np.arange(1, Tmax + 1, dtype=np.int64)[:, None]
    for F in range(1, Fmax + 1):
        c = _candidates(F, limit, pooled)
        if not c:
            continue
        tt, ft, nf = (np.array([k[i] for k in c], dtype=np.int64) for i in range(3))
        fill_cov, halo = (np.array([k[i] for k in c]) for i in (3, 4))
        score = (fill_cov[None, :] * (Ts / (-(-Ts // tt[None, :]) * tt[None, :]))) / halo[None, :]
        score[Ts < tt[None, :]] = -1.0
        k = score.argmax(1)
        best = score[np.arange(Tmax), k]
        ok = best > 0.0
        TTs[F, 1:], FTs[F, 1:], NFs[F, 1:], SC[F, 1:] = np.where(ok, tt[k], 0), np.where(ok, ft[k], 0), np.where(ok, nf[k], 0), best
    return TTs, FTs, NFs, SC


# ───────────────────────── conv_plan / conv_eval_plan ─────────────────────────
def _halo_lds(TT, FT):
    return 2 * (TT + 2) * ((FT + 2) * CV_LD + CV_TPAD) * 4


def conv_plan(B, Cin, F, T, Cout, x_is_nchw=False, pooled=False):
    """-> dict(kind, TT, FT, nft, nct, tblocks, rows, xcd_order, score, lds); kind -1: everything else 0"""
    none = dict(kind=-1, TT=0, FT=0, nft=0, nct=0, tblocks=0, rows=0, xcd_order=0, score=-1.0, lds=0)
    if min(B, Cin, F, T, Cout) <= 0:
        return none
    p = None
    if not x_is_nchw and Cin % CV_CIC == 0 and Cout % 32 == 0:
        nct = nct_of(Cout)
        limit = limit_of(nct)
        t = conv_tile(F, T, limit, pooled)
        if t is None:
            return none
        TT, FT, nft, score = t
        p = dict(kind=1, TT=TT, FT=FT, nft=nft, nct=nct, score=score, lds=max(_halo_lds(TT, FT), (4 * 1024 + 256) * 4) + limit * 4)
    if p is None:                           # the small-channel kernels: 4 time rows, the whole mel axis
        if Cout % 4 != 0:
            return none
        TT = min(4, T)
        nco = min(Cout, 64)
        if (144 * 1024) // ((9 * nco + (TT + 2) * (F + 2)) * 4) < 1:
            return none
        p = dict(kind=0, TT=TT, FT=F, nft=1, nct=0, score=0.0, lds=0)
    p["tblocks"] = cdiv(T, p["TT"])
    p["rows"] = B * p["tblocks"] * p["nft"]
    p["xcd_order"] = int(p["kind"] == 1 and B % 8 == 0)
    return p


def _eval_lds(TT, FT):
    return max(_halo_lds(TT, FT), (8 * 1024 + 256) * 4) + 32 * CV_MTW * 4


def conv_eval_plan(B, Cin, F, T, Cout):
    """the plan of the inference kernel with the (1,2) time pool in its epilogue: the free tile where it has an even number of
    time rows and at most 32 mel columns, else the best such tile if it scores within 2 % of the free one, else none"""
    none = conv_plan(0, 0, 0, 0, 0)
    if min(B, Cin, F, Cout) <= 0 or T < 2:
        return none
    nat = conv_plan(B, Cin, F, T, Cout)
    if nat["kind"] != 1 or nat["nct"] != 4:
        return none
    p = nat
    if (p["TT"] & 1) or p["FT"] > 32:
        p = conv_plan(B, Cin, F, T, Cout, pooled=True)
        if p["kind"] != 1 or p["score"] < 0.98 * nat["score"]:
            return none
    return p if _eval_lds(p["TT"], p["FT"]) <= 80 * 1024 else none


def eval_sweep(Fmax=SWEEP_F, Tmax=SWEEP_T):
    """conv_eval_plan's tile for every F <= Fmax, T <= Tmax (Cout % 128 == 0) -> TT, FT, nft arrays, TT = 0: not supported"""
    nTT, nFT, nNF, nSC = tile_sweep(limit_of(4), False, Fmax, Tmax)
    pTT, pFT, pNF, pSC = tile_sweep(limit_of(4), True, Fmax, Tmax)
    free_ok = (nTT > 0) & ((nTT & 1) == 0) & (nFT <= 32)
    pooled_ok = (nTT > 0) & ~free_ok & (pTT > 0) & ~(pSC < 0.98 * nSC)
    TT, FT, NF = (np.where(free_ok, a, np.where(pooled_ok, b, 0)) for a, b in ((nTT, pTT), (nFT, pFT), (nNF, pNF)))
    lds = np.maximum(2 * (TT + 2) * ((FT + 2) * CV_LD + CV_TPAD) * 4, (8 * 1024 + 256) * 4) + 32 * CV_MTW * 4
    bad = (lds > 80 * 1024) | (np.arange(Tmax + 1)[None, :] < 2)
    return tuple(np.where(bad, 0, a) for a in (TT, FT, NF))


# the data gradient that also forms the first block's tap sums (RG): it keeps two more tables and the input patch in LDS, and
# its tap-sum exchange must not reach them (dgrad_rg_lds / dgrad_rg_tile_ok)
def rg_supported(plan, cin1):
    if plan["kind"] != 1 or plan["nct"] != 4 or cin1 not in (1, 2):
        return False
    TT, FT = plan["TT"], plan["FT"]
    lds = plan["lds"] + 32 * CV_MTW * 4 + (cin1 * (2 * TT + 2) * (FT + 2) + 4) * 4
    return lds <= 80 * 1024 and _halo_lds(TT, FT) // 4 >= 4 * 1024 + 256 + 4 * 9 * cin1 * 32


# ───────────────────────── what the kernel does with a plan ─────────────────────────
def stat_row(plan, b, tb, fi):
    """the partial row the tile (sequence b, time block tb, mel tile fi) writes"""
    return b * plan["tblocks"] * plan["nft"] + tb * plan["nft"] + fi


def tile_slices(plan, F, T, tb, fi):
    """the output positions of a tile: (time slice, mel slice)"""
    return slice(tb * plan["TT"], min(T, (tb + 1) * plan["TT"])), slice(fi * plan["FT"], min(F, (fi + 1) * plan["FT"]))


def xcd_remap(ntiles, B):
    """launch order -> (b, tile): workgroup (blockIdx.x = tile, blockIdx.y = sequence) has launch index i = y * ntiles + x; with
    B % 8 == 0 index i = xcd + 8 j works on sequence xcd + 8 (j // ntiles), tile j % ntiles, else on (y, x)"""
    out = []
    for by in range(B):
        for bx in range(ntiles):
            if B % 8 == 0:
                i = by * ntiles + bx
                xcd, j = i & 7, i >> 3
                out.append((xcd + 8 * (j // ntiles), j % ntiles))
            else:
                out.append((by, bx))
    return out


# ───────────────────────── the table ─────────────────────────
def _shapes_by_tile(TT, FT, NF):
    by = {}
    for F, T in zip(*np.nonzero(TT)):
        by.setdefault((int(TT[F, T]), int(FT[F, T])), []).append((int(F), int(T), int(NF[F, T])))
    return by


def _ragged(F, T, TT, FT, nf):
    return nf * FT > F, T % TT != 0


def _pick(tile, shapes):
    """the (F, T) of smallest F * T that yields the tile; within twice that size one with more ragged edges is preferred"""
    TT, FT = tile
    smallest = min(F * T for F, T, _ in shapes)
    near = [s for s in shapes if s[0] * s[1] <= 2 * smallest]
    return min(near, key=lambda s: (-sum(_ragged(s[0], s[1], TT, FT, s[2])), s[0] * s[1], s[0], s[1]))


def _pick_interior(tile, shapes):
    """the smallest (F, T) whose every tile lies wholly inside the output (the epilogue's unchecked path also needs TT * FT to be
    a multiple of 32), with more than one tile where there is such a shape within twice the smallest"""
    TT, FT = tile
    whole = [s for s in shapes if _ragged(s[0], s[1], TT, FT, s[2]) == (False, False)]
    if not whole or (TT * FT) % 32:
        return None
    smallest = min(F * T for F, T, _ in whole)
    return min((s for s in whole if s[0] * s[1] <= 2 * smallest), key=lambda s: (s[2] * cdiv(s[1], TT) < 2, s[0] * s[1], s[0], s[1]))


def _pick_grid(tile, shapes):
    """the smallest (F, T) with at least three tiles per sequence (the smallest shapes have one: statistic row = sequence), with
    more than one mel tile AND more than one time block where the tile allows it (a tall tile spans the mel axis)"""
    many = [s for s in shapes if s[2] * cdiv(s[1], tile[0]) >= 3 and s[0] * s[1] * B_XCD * 128 <= MAX_OUT_ELEMS]
    if not many:
        return None
    return min(many, key=lambda s: (not (s[2] > 1 and cdiv(s[1], tile[0]) > 1), s[0] * s[1], s[0], s[1]))


def _row(kind, nct, which, tile, shape):
    F, T, nf = shape
    rf, rt = _ragged(F, T, tile[0], tile[1], nf)
    tag = {0: f"nct{nct}", 1: "pool"}[which]
    return dict(name=f"{tag}-{kind}-{tile[0]}x{tile[1]}-F{F}-T{T}", F=F, T=T, nct=nct, which=which, tile=tile, nft=nf, tblocks=cdiv(T, tile[0]),
                ragged_f=rf, ragged_t=rt, kind=kind)


# the shapes of the BatchNorm-backward epilogue test (128 -> 128 channels): F, T, tile, ragged last mel tile, ragged last time
# block; two time blocks each, and two or four mel tiles where the tile does not span the mel axis
BNR_SHAPES = [(40, 16, (8, 20), False, False), (128, 10, (5, 32), False, False), (8, 40, (20, 8), False, False),
              (61, 10, (5, 32), True, False), (40, 13, (8, 20), False, True)]
NAMED_TILES = ((5, 32), (8, 20), (20, 8), (35, 4))      # the model's F = 128 / F = 40 tiles and the tall tiles of the mel-pooled nets


def halo_edge(tile):
    """the halo tile fills the staging budget of the kernel exactly: (TT + 2)(FT + 2) float4 x 8 = 256 threads x CV_NH"""
    return (tile[0] + 2) * (tile[1] + 2) * 8 == 256 * CV_NH


@functools.lru_cache(maxsize=None)
def build_table():
    """-> (rows, returned): rows as described in the module docstring; returned = {(nct, which): set of tiles the sweep returns}"""
    rows, returned = [], {}
    by160 = _shapes_by_tile(*tile_sweep(limit_of(4))[:3])
    returned[(4, 0)] = set(by160)
    widest = max(t for t in by160 if t[0] == 1)
    for tile in sorted(by160):
        rows.append(_row("tile", 4, 0, tile, _pick(tile, by160[tile])))
        inner = _pick_interior(tile, by160[tile])
        if inner is not None:
            rows.append(_row("interior", 4, 0, tile, inner))
        grid = _pick_grid(tile, by160[tile]) if tile in NAMED_TILES or tile == widest or halo_edge(tile) else None
        if grid is not None:
            rows.append(_row("grid", 4, 0, tile, grid))
    for nct in (2, 1):
        by = _shapes_by_tile(*tile_sweep(limit_of(nct))[:3])
        returned[(nct, 0)] = set(by)
        for tile in sorted(by):
            if tile not in by160 or tile in NAMED_TILES:
                rows.append(_row("tile", nct, 0, tile, _pick(tile, by[tile])))
                grid = _pick_grid(tile, by[tile]) if tile in NAMED_TILES or halo_edge(tile) else None
                if grid is not None:
                    rows.append(_row("grid", nct, 0, tile, grid))
    byp = _shapes_by_tile(*eval_sweep())
    returned[(4, 1)] = set(byp)
    for tile in sorted(byp):
        rows.append(_row("tile", 4, 1, tile, _pick(tile, byp[tile])))
    return tuple(rows), returned


def rows(nct=None, which=0, kind=None):
    return [r for r in build_table()[0] if r["which"] == which and (nct is None or r["nct"] == nct) and (kind is None or r["kind"] == kind)]


def row(name):
    return next(r for r in build_table()[0] if r["name"] == name)


def find(nct, which, tile, kind="tile"):
    return next(r for r in build_table()[0] if (r["nct"], r["which"], r["tile"], r["kind"]) == (nct, which, tuple(tile), kind))


def rg_rows():
    """the pooled-plan rows whose (F, T) — read as the pooled extent of the first block, whose conv output has 2 T frames — the
    data gradient with the tap-sum epilogue takes for one and for two input channels (it runs on conv_plan's tile there).  The
    fused first block that feeds it walks 4 frames at a time, so 2 T must be a multiple of 4: rows of odd T have no forward
    that could produce their pooled output and arg-max bits, in the tests or in the network."""
    return [r for r in rows(4, 1) if r["T"] % 2 == 0 and
            all(rg_supported(conv_plan(B, 128, r["F"], r["T"], 128), cin) for B in (B_PLAIN, B_XCD) for cin in (1, 2))]
