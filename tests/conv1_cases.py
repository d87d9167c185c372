"""The case table of the recomputed first conv block (csrc/conv1.hip), shared by test_cpu_conv1_plan.py (which holds the
restatement below against the library's host-only entry points on a dense grid, and every row against the regime it claims) and
test_gpu_conv1_tiles.py (which runs the rows against float64).

Restated here in plain Python: c1_shape_ok and the three `supported` answers built on it; the tile count, grid and visits per
workgroup of every persistent kernel (conv1_fused_k and conv1_rgrad_k: 4-row tiles on at most 2048 workgroups; conv1_gram_k:
16-row tiles, four per round, at most 256 workgroups; conv1_moments_mfma_k: 16-row tiles on at most 1024; conv1_rgrad_mfma_k:
8-row tiles on at most the fused row count); which rgrad kernel sed_conv1_bwd_wgrad launches and why; nslots; the workspace
sizes; and n_serial, the height of the fp32 summation each kernel performs before its partial sums are added in fp64.

n_serial.  A sum of products formed in fp32 in ANY order has an error of at most h * u * sum |terms| (to first order, u = 2^-24)
where h is the largest number of roundings a single term goes through: the additions of the accumulator it enters after it, the
levels of the reduction tree behind that, and one rounding of its own where the product (or a factor of it) is rounded before
it is added.  The GPU test bounds every moment and every R_k by n_serial * 2^-23 * sum |terms| (2^-23 = 2 u: a factor of two
on a worst-case bound); the fp64 stages behind the partial rows add nothing visible at that scale.
  conv1_gram_k          a thread adds ceil(64 F / 256) positions per round of four tiles, over its workgroup's rounds;
                        then 6 levels of the wave reduction and 2 additions across the four waves; + 1 (the product)
  conv1_moments_mfma_k  an accumulator element takes 4 products per MFMA, one MFMA per group of four mel positions, 4 of the
                        16 rows of a tile per wave, over the workgroup's tiles; then 2 additions across the waves
  conv1_rgrad_k         2 fused multiply-adds per position (one per row of the window), ceil(2 F / nslots) positions per tile
                        and slot, over the workgroup's tiles; one rounding by 1 / (1-p); then nslots additions in slot order
  conv1_rgrad_mfma_k    2 products per MFMA, one MFMA per mel position padded to groups of 8, one pooled row per wave and tile;
                        one rounding of g / (1-p); then 2 additions across the waves
  conv1_fused_k         (passes 2 and 3, not used for a bound here) pf * pt window elements per pooled position

A row: name, (B, Cin, F, T, C), pool, and the regime it claims as a dict of keys of regime().
"""
import functools
import zlib

TT, MAXBLOCKS = 4, 2048                    # C1_TT, C1_MAXBLOCKS
GT, GR, GRAM_BLOCKS = 16, 4, 256           # C1_GT, C1_GR, the grid cap of conv1_gram_k
MM_BLOCKS = 1024                           # C1_MM_BLOCKS
RM_GT, RM_CT, RM_D = 8, 2, 8               # C1_RM_GT, C1_RM_CT, C1_RM_D
LDS_MAX = 150 * 1024
EPS = 1e-5


def cdiv(a, b):
    return -(-a // b)


# ───────────────────────── what the library accepts ─────────────────────────
def c1_lds(Cin, F, C, mode):
    halo = (TT + 2) * (F + 2) * Cin * 4
    red = 256 * 4 * (5 if mode == 3 else 2) * 4
    return max(halo, red)


def shape_ok(Cin, F, T, C, pf, pt, max_cin):
    if Cin < 1 or Cin > max_cin or C < 4 or F < 1 or T < 1 or C % 4 or C // 4 > 256 or 256 % (C // 4):
        return False
    if pt < 1 or pf < 1 or TT % pt or T % TT or F % pf or T % pt:
        return False
    return c1_lds(Cin, F, C, 3) <= LDS_MAX


def fused_supported(Cin, F, T, C, pf, pt):
    return shape_ok(Cin, F, T, C, pf, pt, 2)


def rgrad_supported(Cin, F, T, C, pf, pt):
    return pf == 1 and pt == 2 and shape_ok(Cin, F, T, C, pf, pt, 4)


def fwd_supported(Cin, F, T, C, pf, pt):
    """sed_conv1_bn_relu_pool_drop_fwd and sed_conv1_route: 3 and 4 input channels with the (1,2) pool only"""
    return shape_ok(Cin, F, T, C, pf, pt, 4 if (pf, pt) == (1, 2) else 2)


def stats_lds(Cin, F):
    if Cin > 2:
        nk = 9 * Cin
        nt = cdiv(nk + 1, 16)
        return max(((GT + 2) * (F + 2) * Cin + 4) * 4, 4 * (nt * (nt + 1) // 2) * 256 * 4)
    return GR * (GT + 2) * (F + 2) * Cin * 4          # the launch takes the larger of this and the reduction buffer; this is what is limited


def stats_supported(Cin, F, T, C):
    """sed_conv1_stats"""
    return shape_ok(Cin, F, T, C, 1, 1, 4) and stats_lds(Cin, F) <= LDS_MAX


def fused_rows(B, T):
    return min(B * cdiv(T, TT), MAXBLOCKS)


def moments_doubles(Cin):
    nk = 9 * Cin
    return nk + nk * (nk + 1) // 2


def stats_workspace_bytes(B, Cin, T):
    nk = 9 * Cin
    if Cin > 2:
        nt = cdiv(nk + 1, 16)
        return MM_BLOCKS * (nt * (nt + 1) // 2) * 256 * 4 + moments_doubles(Cin) * 8
    return 256 * moments_doubles(Cin) * 4


def bwd_apply_workspace_bytes(B, Cin, T, C):
    return fused_rows(B, T) * (2 + 9 * Cin) * C * 4


def bwd_wgrad_workspace_bytes(B, Cin, T, C):
    return fused_rows(B, T) * (1 + 9 * Cin) * C * 4


def nslots(C):
    return 256 // (C // 4)


# ───────────────────────── the walks ─────────────────────────
def _walk(tiles, grid):
    """-> (most visits of a workgroup, workgroups with that many)"""
    most = cdiv(tiles, grid)
    return most, tiles - (most - 1) * grid


def fused_plan(B, T):
    """conv1_fused_k (every mode) and conv1_rgrad_k"""
    tiles = B * cdiv(T, TT)
    grid = min(tiles, MAXBLOCKS)
    most, at_most = _walk(tiles, grid)
    return dict(tiles=tiles, grid=grid, visits=most, wgs_at_most=at_most, tblocks=cdiv(T, TT))


def gram_plan(B, T):
    """conv1_gram_k: a workgroup stages GR tiles per round"""
    tiles = B * cdiv(T, GT)
    rounds = cdiv(tiles, GR)
    grid = min(rounds, GRAM_BLOCKS)
    return dict(tiles=tiles, rounds=rounds, grid=grid, visits=cdiv(rounds, grid), last_round=tiles - (rounds - 1) * GR, tblocks=cdiv(T, GT))


def moments_mfma_plan(B, T):
    tiles = B * cdiv(T, GT)
    grid = min(tiles, MM_BLOCKS)
    return dict(tiles=tiles, grid=grid, visits=cdiv(tiles, grid), tblocks=cdiv(T, GT))


def rgrad_lds_m(Cin, F):
    return max(((RM_GT + 2) * (F + 2) * Cin + 4) * 4, 4096 * 4)


def rgrad_kernel(Cin, F, C):
    """-> ("mfma", None) or ("scalar", why): "cin" (1 or 2 input channels), "channels" (C % 64), "lds" (the halo tile of the MFMA
    kernel beyond 64 KiB)"""
    if Cin < 3:
        return "scalar", "cin"
    if C % (32 * RM_CT):
        return "scalar", "channels"
    if rgrad_lds_m(Cin, F) > 64 * 1024:
        return "scalar", "lds"
    return "mfma", None


def rgrad_plan(B, Cin, F, T, C):
    """what sed_conv1_bwd_wgrad launches -> dict(kernel, cause, tiles, grid (= partial rows written), grid_y, visits,
    last_waves: the waves of the MFMA kernel that have a pooled row in a sequence's last tile)"""
    kernel, cause = rgrad_kernel(Cin, F, C)
    rows = fused_rows(B, T)
    if kernel == "mfma":
        tb = cdiv(T, RM_GT)
        tiles = B * tb
        grid = min(tiles, rows)
        return dict(kernel=kernel, cause=cause, tiles=tiles, grid=grid, grid_y=C // (32 * RM_CT), visits=cdiv(tiles, grid),
                    tblocks=tb, last_waves=min(4, T // 2 - (tb - 1) * (RM_GT // 2)))
    p = fused_plan(B, T)
    return dict(kernel=kernel, cause=cause, tiles=p["tiles"], grid=p["grid"], grid_y=1, visits=p["visits"], tblocks=p["tblocks"], last_waves=None)


# ───────────────────────── n_serial ─────────────────────────
def n_serial_gram(B, F, T):
    p = gram_plan(B, T)
    return cdiv(GR * GT * F, 256) * p["visits"] + 6 + 2 + 1


def n_serial_moments_mfma(B, F, T):
    p = moments_mfma_plan(B, T)
    return 4 * cdiv(F, 4) * (GT // 4) * p["visits"] + 2


def n_serial_moments(B, Cin, F, T):
    return n_serial_moments_mfma(B, F, T) if Cin > 2 else n_serial_gram(B, F, T)


def n_serial_rgrad(B, Cin, F, T, C):
    p = rgrad_plan(B, Cin, F, T, C)
    if p["kernel"] == "mfma":
        return 2 * RM_D * cdiv(F, RM_D) * p["visits"] + 1 + 2
    return 2 * cdiv((TT // 2) * F, nslots(C)) * p["visits"] + 1 + nslots(C)


def n_serial_fused(B, F, T, C, pf, pt):
    p = fused_plan(B, T)
    return pf * pt * cdiv((TT // pt) * (F // pf), nslots(C)) * p["visits"] + nslots(C)


# ───────────────────────── the table ─────────────────────────
#   name                    (B, Cin, F, T, C)         pool    claims
_TABLE = [
    ("walk-1ch",            (5, 1, 8, 3300, 16),      (1, 2), dict(cin=1, fused_tiles=4125, fused_grid=2048, fused_visits=3, fused_wgs_at_most=29,
                                                                   stats_kernel="gram", stats_tiles=1035, gram_rounds=259, stats_grid=256, stats_visits=2,
                                                                   gram_last_round=3, T_mod16=4, rgrad_kernel="scalar", rgrad_visits=3)),
    ("walk-2ch",            (5, 2, 8, 3300, 32),      (1, 2), dict(cin=2, fused_tiles=4125, fused_grid=2048, fused_visits=3, fused_wgs_at_most=29,
                                                                   stats_kernel="gram", stats_tiles=1035, gram_rounds=259, stats_grid=256, stats_visits=2,
                                                                   gram_last_round=3, T_mod16=4, rgrad_kernel="scalar", rgrad_visits=3)),
    ("walk-4ch-mfma",       (5, 4, 8, 3300, 64),      (1, 2), dict(cin=4, fused_visits=3, stats_kernel="mfma", stats_tiles=1035, stats_grid=1024, stats_visits=2,
                                                                   rgrad_kernel="mfma", rgrad_tiles=2065, rgrad_grid=2048, rgrad_visits=2, T_mod8=4,
                                                                   rgrad_last_waves=2, F_mod4=0, F_mod8=0, F=8)),
    ("walk-3ch-ragged-mel", (5, 3, 7, 3300, 64),      (1, 2), dict(cin=3, fused_visits=3, stats_kernel="mfma", stats_tiles=1035, stats_grid=1024, stats_visits=2,
                                                                   rgrad_kernel="mfma", rgrad_tiles=2065, rgrad_grid=2048, rgrad_visits=2, T_mod8=4,
                                                                   rgrad_last_waves=2, F_mod4=3, F_mod8=7, F=7)),
    ("scalar-4ch",          (2, 4, 7, 20, 32),        (1, 2), dict(cin=4, rgrad_kernel="scalar", rgrad_cause="channels", rgrad_visits=1, fused_visits=1,
                                                                   stats_kernel="mfma", stats_visits=1, F_mod4=3, T_mod16=4, full16=True)),
    ("scalar-4ch-wide",     (1, 4, 408, 8, 64),       (1, 2), dict(cin=4, rgrad_kernel="scalar", rgrad_cause="lds", rgrad_visits=1, stats_kernel="mfma",
                                                                   stats_lds=118096, F_mod4=0)),
    ("scalar-3ch-odd",      (2, 3, 13, 12, 16),       (1, 2), dict(cin=3, rgrad_kernel="scalar", rgrad_cause="channels", rgrad_visits=1, fused_visits=1,
                                                                   stats_visits=1, F_mod4=1)),
    ("c4",                  (2, 1, 8, 12, 4),         (1, 2), dict(cin=1, nslots=256, slot_positions=16, fused_visits=1, stats_visits=1, rgrad_visits=1)),
    ("c512",                (2, 2, 8, 12, 512),       (1, 2), dict(cin=2, nslots=2, fused_visits=1, stats_visits=1, rgrad_visits=1)),
    ("walk-pool22",         (5, 1, 8, 3300, 8),       (2, 2), dict(cin=1, p12=False, fused_tiles=4125, fused_visits=3, rgrad_kernel=None)),
    ("walk-pool51",         (3, 2, 10, 2752, 8),      (5, 1), dict(cin=2, p12=False, fused_tiles=2064, fused_grid=2048, fused_visits=2, fused_wgs_at_most=16,
                                                                   rgrad_kernel=None)),
    # added: the regimes the rows above leave out
    #   conv1_rgrad_k<3> and <4> carrying their accumulators across tiles (the scalar rows above have one tile per workgroup)
    ("walk-3ch-scalar",     (5, 3, 7, 3300, 16),      (1, 2), dict(cin=3, rgrad_kernel="scalar", rgrad_cause="channels", rgrad_visits=3, rgrad_grid=2048)),
    ("walk-4ch-scalar",     (5, 4, 8, 3300, 32),      (1, 2), dict(cin=4, rgrad_kernel="scalar", rgrad_cause="channels", rgrad_visits=3, rgrad_grid=2048)),
    #   conv1_rgrad_mfma_k without a walk; a second 64-channel group (blockIdx.y = 1); mel counts that are no multiple of 8 beyond
    #   the first group of 8 (the clamp after full groups), T % 16 and T % 8 behind full tiles at one tile per workgroup
    ("mfma-4ch-small",      (2, 4, 13, 20, 64),       (1, 2), dict(cin=4, rgrad_kernel="mfma", rgrad_visits=1, rgrad_tiles=6, rgrad_grid=6, rgrad_grid_y=1,
                                                                   rgrad_last_waves=2, stats_visits=1, fused_visits=1, F_mod4=1, F_mod8=5, T_mod16=4, T_mod8=4)),
    ("mfma-3ch-two-groups", (2, 3, 9, 12, 128),       (1, 2), dict(cin=3, rgrad_kernel="mfma", rgrad_visits=1, rgrad_grid_y=2, rgrad_last_waves=2, stats_visits=1,
                                                                   fused_visits=1, F_mod4=1, F_mod8=1, T_mod8=4)),
]
CASES = [dict(name=n, shape=s, pool=p, claims=c) for n, s, p, c in _TABLE]
NAMES = [c["name"] for c in CASES]
P12_NAMES = [c["name"] for c in CASES if c["pool"] == (1, 2)]
POOL_NAMES = [c["name"] for c in CASES if c["pool"] != (1, 2)]
DROPS = (0.0, 0.5)
SEED = 20240


def case(name):
    return next(c for c in CASES if c["name"] == name)


def regime(c):
    """everything a row can claim, from the restatement above"""
    B, Cin, F, T, C = c["shape"]
    pf, pt = c["pool"]
    p12 = (pf, pt) == (1, 2)
    fp = fused_plan(B, T)
    r = dict(cin=Cin, p12=p12, F=F, fused_tiles=fp["tiles"], fused_grid=fp["grid"], fused_visits=fp["visits"], fused_wgs_at_most=fp["wgs_at_most"],
             F_mod4=F % 4, F_mod8=F % 8, T_mod16=T % 16, T_mod8=T % 8, full16=T > GT, full8=T > RM_GT, nslots=nslots(C),
             slot_positions=(TT // pt) * (F // pf), stats_lds=stats_lds(Cin, F))
    if Cin > 2:
        sp = moments_mfma_plan(B, T)
        r.update(stats_kernel="mfma", stats_tiles=sp["tiles"], stats_grid=sp["grid"], stats_visits=sp["visits"], gram_rounds=None, gram_last_round=None)
    else:
        sp = gram_plan(B, T)
        r.update(stats_kernel="gram", stats_tiles=sp["tiles"], stats_grid=sp["grid"], stats_visits=sp["visits"], gram_rounds=sp["rounds"],
                 gram_last_round=sp["last_round"])
    if p12:
        rp = rgrad_plan(B, Cin, F, T, C)
        r.update(rgrad_kernel=rp["kernel"], rgrad_cause=rp["cause"], rgrad_tiles=rp["tiles"], rgrad_grid=rp["grid"], rgrad_grid_y=rp["grid_y"],
                 rgrad_visits=rp["visits"], rgrad_last_waves=rp["last_waves"])
    else:
        r.update(rgrad_kernel=None, rgrad_cause=None, rgrad_tiles=None, rgrad_grid=None, rgrad_grid_y=None, rgrad_visits=None, rgrad_last_waves=None)
    return r


# ───────────────────────── who writes a pooled output element ─────────────────────────
def locate(c, b, tp):
    """pooled row tp of sequence b -> the tile, workgroup and visit of conv1_fused_k (every mode; conv1_rgrad_k walks the same
    tiles) and, for the (1,2) pool, of conv1_rgrad_mfma_k"""
    B, Cin, F, T, C = c["shape"]
    pt = c["pool"][1]
    fp = fused_plan(B, T)
    tile = b * fp["tblocks"] + (tp * pt) // TT
    w = dict(tile=tile, wg=tile % fp["grid"], visit=tile // fp["grid"], visits=fp["visits"])
    if c["pool"] == (1, 2):
        tb = cdiv(T, RM_GT)
        t8 = b * tb + (tp * 2) // RM_GT
        g8 = min(B * tb, fp["grid"])
        w.update(tile8=t8, wg8=t8 % g8, visit8=t8 // g8, wave8=tp % (RM_GT // 2))
    return w


def worst(c, err, what):
    """err [B][T'][F'][C] (torch, >= 0; NaN counts as worst) -> a line naming the worst element and the workgroup that wrote it"""
    import torch
    e = torch.nan_to_num(err.double(), nan=float("inf"))
    i = int(e.argmax())
    b, tp, f, ch = (int(v) for v in torch.unravel_index(torch.tensor(i), e.shape))
    w = locate(c, b, tp)
    return (f"{c['name']} {what}: {int((e > 0).sum())} of {e.numel()} elements off; worst {float(e.flatten()[i]):.3e} at (b, t', f', c) = ({b}, {tp}, {f}, {ch}): "
            f"4-row tile {w['tile']} = visit {w['visit']} (of {w['visits']}) of workgroup {w['wg']}")


# ───────────────────────── inputs and the float64 reference ─────────────────────────
def inputs(name, zero_gamma=False):
    """x [B][Cin][F][T] N(0.5, 1) (NOT standardised: the closed form of the weight gradient subtracts moment terms), w, bias, gamma in
    [0.5, 1.5) with one negative channel (2), beta; zero_gamma: channel 1 has gamma = 0 and beta = 0.4.  float32 torch, CPU."""
    import torch
    B, Cin, F, T, C = case(name)["shape"]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = torch.randn(B, Cin, F, T, generator=gen) + 0.5
    w = torch.randn(C, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5
    bias = torch.randn(C, generator=gen) * 0.3
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    gamma[2] = -0.8
    if zero_gamma:
        gamma[1], beta[1] = 0.0, 0.4
    return dict(x=x, w=w, bias=bias, gamma=gamma, beta=beta)


def dout_of(name):
    import torch
    c = case(name)
    B, Cin, F, T, C = c["shape"]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()) ^ 0x5EED)
    return torch.randn(B, T // c["pool"][1], F // c["pool"][0], C, generator=gen) * 0.1


def taps(x):
    """the 9 Cin shifted inputs of every position in the kernels' order k = (kh * 3 + kw) * Cin + ci (kh: mel, kw: time), zero
    outside the image -> float64 [B][9 Cin][F][T]"""
    import torch.nn.functional as Fn
    B, Cin, F, T = x.shape
    v = Fn.unfold(x.double(), 3, padding=1).view(B, Cin, 9, F, T)      # unfold: channel-major, then the kernel position
    return v.permute(0, 2, 1, 3, 4).reshape(B, 9 * Cin, F, T)


def pack_moments(S1, G):
    """S1 [NK], G [NK][NK] -> the packed vector of gram_out: S1, then the upper triangle row by row"""
    import torch
    nk = S1.numel()
    iu = torch.triu_indices(nk, nk)
    return torch.cat([S1, G[iu[0], iu[1]]])


def ref_moments(x):
    """-> (moments, sum of |terms| per entry), packed, float64"""
    import torch
    v = taps(x).permute(1, 0, 2, 3).reshape(9 * x.shape[1], -1)
    a = v.abs()
    return pack_moments(v.sum(1), v @ v.T), pack_moments(a.sum(1), a @ a.T)


def tie(z0, z1):
    """the near-ties the decision tests leave out"""
    return (z0 - z1).abs() < 1e-4 * (z0.abs() + z1.abs() + 1)


TIE_CAP = 1e-3


@functools.lru_cache(maxsize=None)
def ref_forward(name, zero_gamma=False):
    """conv -> BatchNorm(train) -> ReLU -> MaxPool in torch float64 -> dict: mean / var / second moment of the conv output per channel,
    pooled [B][T'][F'][C] (channels-last, no dropout), and the decisions: for the (1,2) pool bit = z1 > z0 and near = tie(z0, z1); for
    the other pools the routing code (0: gate closed, 1 + df * pt + dt of the first maximum) and near = the first two of the window,
    or the maximum and the gate's 0, within the tie bound.  Computed once per row and left unchanged."""
    import torch
    import torch.nn.functional as Fn
    c = case(name)
    pf, pt = c["pool"]
    d = inputs(name, zero_gamma)
    with torch.no_grad():
        y = Fn.conv2d(d["x"].double(), d["w"].double(), d["bias"].double(), padding=1)
        mean, var, q = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False), (y * y).mean((0, 2, 3))
        sc = d["gamma"].double() / torch.sqrt(var + EPS)
        z = (y - mean.view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + d["beta"].double().view(1, -1, 1, 1)
        del y
        cl = lambda t: t.permute(0, 3, 2, 1).contiguous()
        r = dict(mean=mean, var=var, q=q, pooled=cl(Fn.max_pool2d(torch.relu(z), (pf, pt))))
        if (pf, pt) == (1, 2):
            z0, z1 = z[..., 0::2], z[..., 1::2]
            r.update(bit=cl(z1 > z0), near=cl(tie(z0, z1)))
        else:
            B, C, F, T = z.shape
            win = z.view(B, C, F // pf, pf, T // pt, pt).permute(0, 1, 2, 4, 3, 5).reshape(B, C, F // pf, T // pt, pf * pt)     # w = df * pt + dt
            top = win.topk(2, dim=-1).values
            best, second = top[..., 0], top[..., 1]
            arg = (win == best.unsqueeze(-1)).to(torch.uint8).argmax(-1)                       # the first maximum
            code = torch.where(best > 0, arg + 1, torch.zeros_like(arg)).to(torch.uint8)
            r.update(code=cl(code), near=cl(tie(best, second) | tie(best, torch.zeros_like(best))))
    return r
