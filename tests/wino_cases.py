"""The case table of the Winograd conv kernel (conv3x3_wino_k, csrc/wino.hip) with the pooled inference epilogue, shared by
test_cpu_wino_geo.py (which holds the restatement below against sed_conv3x3_wino_rows on a dense grid, and every row against the
regime it claims) and test_gpu_wino_eval.py (which runs the rows).

Restated here in plain Python: wino_geo — the number of column groups ncg the mel axis is cut into, the tiles per row of a group
Fw, the tile rows Tw, tiles and 64-tile blocks per sequence and group, the tile rows TR a block touches, the patch positions HR
and the KiB blocks NH of the patch per wave that have to fit WN_NHMAX — or None where the geometry refuses the shape; the
workgroup a pooled output element belongs to (what the GPU test prints on failure); and the integer inputs of the exact test with
the bound under which every float32 sum of the kernel is exact.

A row: name, F, T (128 input channels) and what it claims: (ncg, Fw, nblk, TR, NH, tiles in the last block), or None: refused.
"""
import functools

import numpy as np

WN_CIN, WN_NHMAX = 128, 14
B_PLAIN, B_XCD = 3, 8                      # workgroup order: plain / XCD-aware (gridDim.y % 8 == 0)


def cdiv(a, b):
    return -(-a // b)


# ───────────────────────── wino_geo ─────────────────────────
@functools.lru_cache(maxsize=None)
def _geo_ft(F, T):
    """the part of wino_geo that depends on (F, T) only -> dict or None"""
    Tw = T // 2
    ncg = 1
    while ncg <= 8:
        if (F // 2) % ncg:
            return None
        Fw = F // 2 // ncg
        ntile = Fw * Tw
        nblk = cdiv(ntile, 64)
        q0 = np.arange(nblk, dtype=np.int64) * 64
        q1 = np.minimum(q0 + 63, ntile - 1)
        TR = int((q1 // Fw - q0 // Fw + 1).max())
        F2 = 2 * Fw + 2
        HR = (2 * TR + 2) * F2
        nb8 = cdiv(HR, 8)
        NH = cdiv(nb8, 4)
        if NH <= WN_NHMAX:
            return dict(ncg=ncg, Fw=Fw, Tw=Tw, ntile=ntile, nblk=nblk, TR=TR, F2=F2, H2=F2 // 2, HR=HR, nb8=nb8, NH=NH,
                        last=ntile - (nblk - 1) * 64)
        ncg *= 2
    return None


def wino_geo(B, Cin, F, T, Cout):
    """-> dict(ncg, Fw, Tw, ntile, nblk, TR, F2, H2, HR, nb8, NH (what the patch needs; the launch always uses WN_NHMAX), last
    (tiles in the last block), ncoh, rows) or None: refused"""
    if B <= 0 or Cin != WN_CIN or Cout <= 0 or Cout % 64 or F < 2 or T < 2 or (F & 1) or (T & 1):
        return None
    if B * T * F * Cin >= 1 << 32 or T * F * Cout >= 1 << 30 or T * F * Cin * 4 >= 1 << 31:
        return None
    g = _geo_ft(F, T)
    if g is None:
        return None
    fl = max(2 * WN_NHMAX * 1024, 32768 + 512)
    if (fl + 64) * 4 > 160 * 1024:
        return None
    return dict(g, ncoh=Cout // 64, rows=B * g["nblk"] * g["ncg"], lds=(fl + 64) * 4)


def wino_rows(B, Cin, F, T, Cout):
    g = wino_geo(B, Cin, F, T, Cout)
    return g["rows"] if g else 0


# ───────────────────────── the table ─────────────────────────
#        name                       F    T   (ncg, Fw, nblk, TR, NH, tiles in the last block)
_TABLE = [
    ("one-tile",                     2,   2, (1, 1, 1, 1, 1, 1)),
    ("odd-row-ragged",               6,   6, (1, 3, 1, 3, 2, 9)),
    ("mel40-one-block",             40,   6, (1, 20, 1, 3, 11, 60)),
    ("mel40-lds-limit",             40,  16, (1, 20, 3, 4, 14, 32)),
    ("last-block-4-tiles",          34,   8, (1, 17, 2, 4, 12, 4)),
    ("tallest",                      4,  64, (1, 2, 1, 32, 13, 64)),
    ("tall-two-blocks",              6,  64, (1, 3, 2, 22, 12, 32)),
    ("two-full-rows",               64,   4, (1, 32, 1, 2, 13, 64)),
    ("widest-one-group",            70,   6, (1, 35, 2, 2, 14, 41)),
    ("refused",                     70,   8, None),
    ("same-F-one-group",            48,   8, (1, 24, 2, 3, 13, 32)),
    ("same-F-two-groups",           48,  16, (2, 12, 2, 6, 12, 32)),
    ("odd-Fw-two-groups",          100,   8, (2, 25, 2, 3, 13, 36)),
    ("mel128-one-block",           128,   4, (2, 32, 1, 2, 13, 64)),
    ("mel128-ragged",              128,   6, (2, 32, 2, 2, 13, 32)),
    ("four-groups",                 96,  16, (4, 12, 2, 6, 12, 32)),
    ("four-groups-T2",             256,   2, (4, 32, 1, 1, 9, 32)),
    ("eight-groups",               320,   4, (8, 20, 1, 2, 8, 40)),
    ("eight-groups-two-blocks",    192,  16, (8, 12, 2, 6, 12, 32)),
    ("long-sequence",               40, 512, (1, 20, 80, 4, 14, 64)),
]
CASES = [dict(name=n, F=F, T=T, claims=c) for n, F, T, c in _TABLE]
REGIME_KEYS = ("ncg", "Fw", "nblk", "TR", "NH", "last")
# the rows that run at both batch sizes with 128 output channels; three of them also at 64, 192 and 256 (ncoh = 1, 3, 4)
GRID_ROWS = [c["name"] for c in CASES if c["claims"] is not None and c["name"] != "long-sequence"]
COUT_ROWS = ["mel40-lds-limit", "mel128-ragged", "eight-groups"]
RUNS = [(n, 128) for n in GRID_ROWS] + [(n, co) for n in COUT_ROWS for co in (64, 192, 256)]
LONG = ("long-sequence", 64)               # B = 1 only
# the geometry refuses these although F and T are even: F / 2 is odd, or leaves an odd half, and cannot be split further
REFUSED = [(70, 8), (100, 16), (200, 16)]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def regime(F, T):
    g = wino_geo(1, WN_CIN, F, T, 64)
    return None if g is None else tuple(g[k] for k in REGIME_KEYS)


# ───────────────────────── who writes a pooled output element ─────────────────────────
def locate(g, t, f, c):
    """pooled output (t', f, c) of a sequence -> dict(tile q = ty * Fw + tf of its column group, ty, tf, block, slot in the block,
    column group, channel half, blka = block * ncg + group: the workgroup's index inside the sequence)"""
    cg, fin = divmod(f, 2 * g["Fw"])
    tf = fin // 2
    q = t * g["Fw"] + tf                    # the pooled row t' IS the tile row: the tile's two time rows are the pooling pair
    return dict(tile=q, ty=t, tf=tf, block=q // 64, slot=q % 64, group=cg, half=c // 64, blka=(q // 64) * g["ncg"] + cg)


def first_difference(got, ref, g):
    """got, ref [B][T'][F][C] (numpy) -> a line naming the first differing element and the workgroup it belongs to"""
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    if len(bad) == 0:
        return "no difference"
    b, t, f, c = (int(v) for v in bad[0])
    w = locate(g, t, f, c)
    return (f"{len(bad)} of {ref.size} elements differ ({int(np.isnan(got).sum())} NaN); first at (b, t', f, c) = ({b}, {t}, {f}, {c}): "
            f"got {got[b, t, f, c]!r}, want {ref[b, t, f, c]!r}; tile {w['tile']} (row {w['ty']}, column {w['tf']}) = slot {w['slot']} of "
            f"block {w['block']}, column group {w['group']} of {g['ncg']}, channel half {w['half']}")


# ───────────────────────── the integer inputs of the exact test ─────────────────────────
GAMMAS = (-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
VARS = (0.25, 1.0, 4.0)
X_MAX, W_MAX, P_MAX = 2, 1, 2              # |x|, |w|, |bias| = |beta| = |running mean| at most


def int_inputs(F, T, Cout, B=B_XCD):
    """x [B][128][F][T] integer in [-2, 2] (sequence b: {-1, 0, 1} + its level b % 3 - 1), w in {-1, 0, 1}, integer bias / beta / running mean in [-2, 2], gamma from GAMMAS (every value in
    every 64-channel half, so gamma = 0 and negative gammas occur in each), running variance from VARS; eps is 0.  float64 numpy."""
    rng = np.random.default_rng(100000 + 1000 * F + 10 * T + Cout)
    # every sequence on a level of its own, inside the range: {-1, 0, 1} + (b % 3 - 1), so neighbouring sequences never share one
    x = (rng.integers(-1, 2, (B, WN_CIN, F, T)) + (np.arange(B) % 3 - 1).reshape(B, 1, 1, 1)).astype(np.float64)
    w = rng.integers(-W_MAX, W_MAX + 1, (Cout, WN_CIN, 3, 3)).astype(np.float64)
    bias, beta, rm = (rng.integers(-P_MAX, P_MAX + 1, Cout).astype(np.float64) for _ in range(3))
    gamma = rng.choice(GAMMAS, Cout)
    for h in range(Cout // 64):
        gamma[h * 64 + rng.permutation(64)[:len(GAMMAS)]] = GAMMAS
    rv = rng.choice(VARS, Cout)
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta, rm=rm, rv=rv, eps=0.0)


def exactness_bound():
    """the largest magnitude, in units of 1/16, that any float32 sum of the kernel can hold on int_inputs, in any order:
    U = G g' G^T of the folded weights g' = w * scale (|scale| <= 2 / sqrt(0.25) = 4, |U| <= 9/4 * 4, a multiple of scale / 4 with
    |scale| >= 1/4: a multiple of 1/16), V = B^T d B of the input (integers, |V| <= 4 * 2), M = sum over 128 channels of U V,
    Y = A^T M A (at most 9 of the 16 components) + the folded bias"""
    scale = max(abs(g) for g in GAMMAS) / min(VARS) ** 0.5
    u16 = 16 * 2.25 * W_MAX * scale
    v = 4 * X_MAX
    m16 = WN_CIN * u16 * v
    bias16 = 16 * (P_MAX * scale + P_MAX + P_MAX * scale)
    return 9 * m16 + bias16


def ref_pooled(d):
    """max_pool2d(relu(batch_norm(conv2d(x))), (1, 2)) on running statistics in torch float64 -> channels-last [B][T/2][F][Cout];
    d: a dict of x [B][Cin][F][T], w, bias, gamma, beta, rm, rv (numpy or torch) and eps"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.as_tensor(v).double() for k, v in d.items() if k != "eps"}
    y = F.conv2d(t["x"], t["w"], t["bias"], padding=1)
    v = lambda k: t[k].view(1, -1, 1, 1)
    if float(d["eps"]) > 0:
        y = F.batch_norm(y, t["rm"], t["rv"], t["gamma"], t["beta"], training=False, eps=float(d["eps"]))
    else:                                   # torch refuses eps = 0: BatchNorm on running statistics, written out
        y = (y - v("rm")) / torch.sqrt(v("rv")) * v("gamma") + v("beta")
    return F.max_pool2d(torch.relu(y), (1, 2)).permute(0, 3, 2, 1).contiguous()
