"""numpy float64 restatements of the small streaming and reduction passes of the fit step (csrc/bnpool.hip, csrc/misc.hip and
the dropout hash of csrc/common.h), the inputs the tests feed them and the table of shapes.  No torch, no device: the module
is pinned by tests/test_cpu_small_passes_ref.py against float64 autograd and torch.optim.Adam, and
tests/test_gpu_small_passes.py holds every kernel against it.

Every function takes the fp32 arrays the kernel is given and computes in float64 from them, with the formulas written as the
kernels define them (z = y*scale + shift, first maximum in window order w = df*pt + dt, gate = max > 0, floor pooling)."""
import functools
import math

import numpy as np

U = 2.0 ** -24                      # unit roundoff of fp32: one rounding moves a value by at most U times its magnitude
TINY = 2.0 ** -126                  # smallest normal fp32: below it a result may be flushed or lose bits
GOLD = 0x9E3779B97F4A7C15           # salt multiplier of the device step state
M64 = (1 << 64) - 1


def bound(k, magnitude):
    """k roundings of relative size U on `magnitude`: gamma_k = kU / (1 - kU) (no first-order truncation), plus one denormal"""
    return (k * U / (1.0 - k * U)) * np.asarray(magnitude, np.float64) + TINY


# ───────────────────────── dropout hash ─────────────────────────
def fmix32(h):
    h = np.asarray(h, np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def salted_seed(seed, salt):
    """the seed a kernel uses when it is handed the device step state {salt, step}: seed + salt * GOLD mod 2^64"""
    return (int(seed) + int(salt) * GOLD) & M64


def uniform(seed, idx):
    """sed_uniform: 24 bits in [0, 1) from (seed, logical channels-last index), exact in float64"""
    seed = int(seed) & M64
    idx = np.asarray(idx, np.uint64)
    lo = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (idx >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = fmix32(lo ^ np.uint32(seed & 0xFFFFFFFF))
        h = fmix32(h + np.uint32(seed >> 32) + hi * np.uint32(0x9E3779B1))
    return (h >> np.uint32(8)).astype(np.float64) / 16777216.0


def keep_mask(seed, idx, p, salt=None):
    """sed_drop_mult's decision: True where the element is kept (uniform >= p, compared in fp32 as the kernel does)"""
    if salt is not None:
        seed = salted_seed(seed, salt)
    return uniform(seed, idx) >= float(np.float32(p))


def keep_for(shape, seed, p, salt=None):
    """keep mask of a channels-last pooled tensor [B,Tp,Fp,C] (all True at p == 0: the kernels skip the hash)"""
    if p <= 0:
        return np.ones(shape, bool)
    return keep_mask(seed, np.arange(int(np.prod(shape)), dtype=np.uint64), p, salt).reshape(shape)


# ───────────────────────── BatchNorm / ReLU / pool / dropout block ─────────────────────────
def _windows(a, pf, pt):
    """[B,T,F,C] -> [B,Tp,Fp,pf*pt,C], window element w = df*pt + dt; ragged tails dropped"""
    B, T, F, C = a.shape
    Tp, Fp = T // pt, F // pf
    a = a[:, :Tp * pt, :Fp * pf].reshape(B, Tp, pt, Fp, pf, C)
    return a.transpose(0, 1, 3, 4, 2, 5).reshape(B, Tp, Fp, pf * pt, C)


def _unwindows(w, pf, pt):
    """inverse of _windows on the covered region: [B,Tp,Fp,pf*pt,C] -> [B,Tp*pt,Fp*pf,C]"""
    B, Tp, Fp, _, C = w.shape
    return w.reshape(B, Tp, Fp, pf, pt, C).transpose(0, 1, 4, 2, 3, 5).reshape(B, Tp * pt, Fp * pf, C)


def _mult(keep, p):
    return np.asarray(keep, np.float64) / (1.0 - float(np.float32(p)))


def bn_block_fwd(y, scale, shift, pf, pt, keep=None, p=0.0):
    """-> dict(out [B,Tp,Fp,C] = relu(max_w z) * keep / (1 - p), route (0 = gate closed, 1 + w), mag = |y*scale| + |shift| of
    the winner over (1 - p): what one rounding of the output is relative to)"""
    y = np.asarray(y, np.float64)
    sc, sh = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
    yw = _windows(y, pf, pt)
    z = yw * sc + sh
    arg = np.argmax(z, axis=3)                                        # numpy keeps the first maximum, like the kernels
    zmax = np.take_along_axis(z, arg[:, :, :, None, :], 3)[:, :, :, 0, :]
    ywin = np.take_along_axis(yw, arg[:, :, :, None, :], 3)[:, :, :, 0, :]
    gate = zmax > 0.0
    m = _mult(np.ones(zmax.shape, bool) if keep is None else keep, p)
    return {"out": np.where(gate, zmax, 0.0) * m, "route": np.where(gate, 1 + arg, 0).astype(np.uint8), "arg": arg, "gate": gate,
            "mag": (np.abs(ywin * sc) + np.abs(sh)) * m}


def bn_block_bwd(y, dout, scale, shift, mean, rstd, pf, pt, keep, N, p=0.0, sums=None):
    """backward of the block for dout [B,Tp,Fp,C] (channels-last).  -> dict:
    sum_g, sum_gx [C] and the sums of their absolute terms (mag_g; mag_gx with |y| + |mean| for the centred value);
    dy [B,T,F,C] = scale (g_at_the_winner - sum_g/N - xhat sum_gx/N) for `sums` (default: its own), tails with the statistics
    terms only, mag_dy its absolute operands; sum_dy [C]; route."""
    y = np.asarray(y, np.float64)
    B, T, F, C = y.shape
    Tp, Fp = T // pt, F // pf
    sc, mu, rs = (np.asarray(a, np.float64) for a in (scale, mean, rstd))
    fwd = bn_block_fwd(y, scale, shift, pf, pt)
    g = np.asarray(dout, np.float64) * _mult(keep, p) * fwd["gate"]
    xhat = (y - mu) * rs
    axh = (np.abs(y) + np.abs(mu)) * rs
    pick = fwd["arg"][:, :, :, None, :]
    bx = np.take_along_axis(_windows(xhat, pf, pt), pick, 3)[:, :, :, 0, :]
    abx = np.take_along_axis(_windows(axh, pf, pt), pick, 3)[:, :, :, 0, :]
    res = {"sum_g": g.sum((0, 1, 2)), "sum_gx": (g * bx).sum((0, 1, 2)), "mag_g": np.abs(g).sum((0, 1, 2)),
           "mag_gx": (np.abs(g) * abx).sum((0, 1, 2)), "route": fwd["route"]}
    sg, sgx = (res["sum_g"], res["sum_gx"]) if sums is None else (np.asarray(s, np.float64) for s in sums)
    onehot = np.arange(pf * pt)[None, None, None, :, None] == pick
    gfull = np.zeros_like(y)
    gfull[:, :Tp * pt, :Fp * pf] = _unwindows(np.where(onehot, g[:, :, :, None, :], 0.0), pf, pt)
    res["dy"] = sc * (gfull - sg / N - xhat * sgx / N)
    res["mag_dy"] = np.abs(sc) * (np.abs(gfull) + np.abs(sg) / N + axh * np.abs(sgx) / N)
    res["sum_dy"] = res["dy"].sum((0, 1, 2))
    return res


def near_ties(y, scale, shift, pf, pt, channels=None):
    """windows whose decision lacks margin: |z_max| or the gap between the two largest z below 1e-4 (1 + |z_max|)"""
    z = _windows(np.asarray(y, np.float64), pf, pt) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    arg = np.argmax(z, axis=3)
    top = np.take_along_axis(z, arg[:, :, :, None, :], 3)[:, :, :, 0, :]
    thr = 1e-4 * (1.0 + np.abs(top))
    bad = np.abs(top) < thr
    if pf * pt > 1:
        second = np.partition(z, -2, axis=3)[:, :, :, -2, :]
        bad |= (top - second) < thr
    if channels is not None:
        bad &= np.asarray(channels, bool)
    return bad, arg


def repair_near_ties(y, scale, shift, pf, pt, channels=None):
    """-> (y with 2^-4 added to the winner of every window that lacks margin (towards a larger z: subtracted where scale < 0),
    repeated until none remain; the share of windows that were touched).  channels: a [C] mask of the channels to look at."""
    y = np.array(y, np.float32)
    B, T, F, C = y.shape
    Tp, Fp = T // pt, F // pf
    step = np.where(np.asarray(scale, np.float64) < 0, -0.0625, 0.0625).astype(np.float32)
    touched = np.zeros((B, Tp, Fp, C), bool)
    for _ in range(16):
        bad, arg = near_ties(y, scale, shift, pf, pt, channels)
        if not bad.any():
            n = touched.size if channels is None else B * Tp * Fp * int(np.count_nonzero(channels))
            return y, touched.sum() / max(n, 1)
        touched |= bad
        onehot = (np.arange(pf * pt)[None, None, None, :, None] == arg[:, :, :, None, :]) & bad[:, :, :, None, :]
        add = np.zeros_like(y)
        add[:, :Tp * pt, :Fp * pf] = _unwindows(onehot * step, pf, pt)
        y = y + add
    raise AssertionError("repair_near_ties did not converge")


def bn_stats(y, gamma, beta, eps=1e-5):
    """training statistics of y [.., C] in float64, rounded ONCE to fp32: mean, rstd, scale = gamma rstd, shift = beta - mean scale"""
    flat = np.asarray(y, np.float64).reshape(-1, y.shape[-1])
    m = flat.mean(0)
    var = (flat * flat).mean(0) - m * m
    r = 1.0 / np.sqrt(np.maximum(var, 0.0) + eps)
    sc = np.asarray(gamma, np.float64) * r
    f = np.float32
    return m.astype(f), r.astype(f), sc.astype(f), (np.asarray(beta, np.float64) - m * sc).astype(f)


def slow_channels(gamma, beta):
    """channels the pooled identity cannot serve (xhat from the conv output): gamma == 0 with beta > 0, or 64 |gamma| < |beta|"""
    gm, bt = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    return np.where(gm == 0, bt > 0, np.abs(gm) * np.float32(64) < np.abs(bt))


def pooled_sums(pooled, dout, gamma, beta, y, mean, rstd, scale, shift, pf, pt, p):
    """the identity sed_bn_bwd_reduce_pooled uses, from the pooled output q and its gradient (both [B,Tp,C,Fp]): the gradient
    passes where q > 0, g = dout / (1 - p), xhat = (q (1 - p) - beta) / gamma; slow channels take xhat of the window's first
    maximum from the conv output.  -> dict(sum_g, sum_gx, mag_g, mag_gx) per channel"""
    q = np.asarray(pooled, np.float64).transpose(0, 1, 3, 2)          # channels-last [B,Tp,Fp,C]
    d = np.asarray(dout, np.float64).transpose(0, 1, 3, 2)
    gm, bt = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    keepf = 1.0 - float(np.float32(p))
    g = np.where(q > 0, d, 0.0) / keepf
    slow = slow_channels(gamma, beta)
    safe = np.where((gm == 0) | slow, 1.0, gm)
    live = (gm != 0) & ~slow
    xh = np.where(live, (q * keepf - bt) / safe, 0.0)
    axh = np.where(live, (np.abs(q) * keepf + np.abs(bt)) / np.abs(safe), 0.0)
    if slow.any():
        yd = np.asarray(y, np.float64)[..., slow]
        mu, rs = np.asarray(mean, np.float64)[slow], np.asarray(rstd, np.float64)[slow]
        yw = _windows(yd, pf, pt)
        z = yw * np.asarray(scale, np.float64)[slow] + np.asarray(shift, np.float64)[slow]
        yb = np.take_along_axis(yw, np.argmax(z, axis=3)[:, :, :, None, :], 3)[:, :, :, 0, :]
        xh[..., slow] = (yb - mu) * rs
        axh[..., slow] = (np.abs(yb) + np.abs(mu)) * rs
    return {"sum_g": g.sum((0, 1, 2)), "sum_gx": (g * xh).sum((0, 1, 2)), "mag_g": np.abs(g).sum((0, 1, 2)),
            "mag_gx": (np.abs(g) * axh).sum((0, 1, 2))}


def bn_finalize(A, Q, count, gamma, beta, rmean, rvar, momentum, eps):
    """training BatchNorm of every channel from its sums A = sum y, Q = sum y^2 (float64 throughout; momentum and eps are the
    fp32 values the kernel is passed)"""
    A, Q = np.asarray(A, np.float64), np.asarray(Q, np.float64)
    mom, eps = float(np.float32(momentum)), float(np.float32(eps))
    m = A / count
    var = np.maximum(Q / count - m * m, 0.0)
    r = 1.0 / np.sqrt(var + eps)
    sc = np.asarray(gamma, np.float64) * r
    unb = var * count / (count - 1.0) if count > 1 else var
    return {"mean": m, "var": var, "rstd": r, "scale": sc, "shift": np.asarray(beta, np.float64) - m * sc, "unb": unb,
            "rmean": (1.0 - mom) * np.asarray(rmean, np.float64) + mom * m, "rvar": (1.0 - mom) * np.asarray(rvar, np.float64) + mom * unb}


# ───────────────────────── optimiser, norm, losses ─────────────────────────
def adam_step(p, g, m, v, lr, b1, b2, eps, wd, t, grad_scale=1.0):
    """one Adam step with coupled L2 decay, a scale on the gradient and the bias corrections of step t -> (p, m, v).  The
    scalars are the fp32 values the kernel is passed."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (float(np.float32(a)) for a in (lr, b1, b2, eps, wd, grad_scale))
    gi = g * gs + wd * p
    m = b1 * m + (1.0 - b1) * gi
    v = b2 * v + (1.0 - b2) * gi * gi
    bc1, bc2 = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
    return p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps)), m, v


def norm_and_clip(g, max_norm):
    """-> (l2 norm, clip coefficient min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0)"""
    g = np.asarray(g, np.float64)
    nrm = math.sqrt(float((g * g).sum()))
    mx = float(np.float32(max_norm))
    return nrm, (min(1.0, mx / (nrm + float(np.float32(1e-6)))) if mx > 0 else 1.0)


def sigmoid(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_with_logits(x, t, mean=True):
    """-> (loss, d loss / d x, probabilities)"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    s = 1.0 / x.size if mean else 1.0
    l = np.maximum(x, 0.0) - x * t + np.log1p(np.exp(-np.abs(x)))
    p = sigmoid(x)
    return float(l.sum() * s), (p - t) * s, p


def focal_loss(x, t, alpha, gamma, mean=True):
    """the focal loss as misc.hip spells it: pos = (t == 1), pt = p or 1 - p, l = -alpha (1 - pt)^gamma log(pt + 1e-12)
    -> (loss, d loss / d x, probabilities)"""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    alpha, gamma, e12 = float(np.float32(alpha)), float(np.float32(gamma)), float(np.float32(1e-12))
    s = 1.0 / x.size if mean else 1.0
    p = sigmoid(x)
    pos = t == 1.0
    pt = np.where(pos, p, 1.0 - p)
    om = 1.0 - pt
    lg = np.log(pt + e12)
    pw = om ** gamma
    dpw = gamma * om ** (gamma - 1.0) if gamma != 0 else 0.0
    dl_dpt = -alpha * (-dpw * lg + pw / (pt + e12))
    dpt_dx = np.where(pos, p * (1.0 - p), -p * (1.0 - p))
    return float((-alpha * pw * lg).sum() * s), dl_dpt * dpt_dx * s, p


# ───────────────────────── the shapes of the GPU table and their inputs ─────────────────────────
# (B, T, F, C, pf, pt)
B1_FWD_CL = [(1, 1700, 40, 128, 1, 1)]                               # 2 176 000 float4 > 8192 blocks x 256
B2_FWD_TCF = [(3, 2901, 9, 8, 2, 2)]                                 # 4350 rows > 4096, both axes ragged
B3_BWD = [(5, 1027, 8, 16, 1, 2), (3, 1201, 9, 12, 2, 3)]            # 2565 rows (P12, ragged T), 1200 rows (generic, both tails)
B4_CHANNELS = [(2, 5, 6, c, 1, 2) for c in (4, 12, 100, 516, 1024)] + [(2, 5, 7, c, 2, 1) for c in (4, 12, 100, 516, 1024)]
B5_SEED_DEV = [(2, 9, 9, 12, 2, 2)]
B6_POOLED = [(3, 4, 8, 128 * k - 4, 1, 2) for k in range(1, 9)] + [(3, 4, 8, 1500, 1, 2), (3, 4, 8, 2000, 1, 2), (3, 800, 8, 636, 1, 2)]
BLOCK_SHAPES = B1_FWD_CL + B2_FWD_TCF + B3_BWD + B4_CHANNELS + B5_SEED_DEV
REPAIR_CAP = 1e-3                                                    # at most 0.1 % of the windows may need the repair


def pooled_special_channels(C):
    """B6: the channel of every per-thread slot (c = 128 j + 5 at 256 threads, 512 j + 5 at 1024) and its kind, cycling
    0: gamma = 0, beta > 0;  1: gamma = 0, beta < 0;  2: |gamma| = 1e-5;  3: a small gamma < 0"""
    stride = 128 if C * 2 <= 2048 else 512
    return [(c, j % 4) for j, c in enumerate(range(5, C, stride))]


@functools.lru_cache(maxsize=2)
def block_inputs(shape, pooled_kinds=False):
    """inputs of a B case: y = randn 1.5 + 0.3 through repair_near_ties, gamma, beta, and the float64 statistics of y rounded
    once to fp32.  -> dict(y, gamma, beta, mean, rstd, scale, shift, share, N).  pooled_kinds (B6): the special channels of
    pooled_special_channels are planted, and their y sits on a 2^-2 grid plus 2^-4 w, so that a window's elements differ by
    at least 2^-4 there (a gamma of 1e-5 leaves z gaps far below the repair's threshold; this keeps them above an fp32 ulp
    of z)."""
    B, T, F, C, pf, pt = shape
    for draw in range(8):                      # a few hundred windows: one near-tie is already more than the cap -> next draw
        d = _draw_block(shape, pooled_kinds, draw)
        if d["share"] <= REPAIR_CAP:
            return d
    raise AssertionError(f"no draw of {shape} within the repair cap")


def _draw_block(shape, pooled_kinds, draw):
    B, T, F, C, pf, pt = shape
    rng = np.random.default_rng(list(shape) + [int(pooled_kinds), draw])
    f = np.float32
    y = (rng.standard_normal((B, T, F, C), dtype=f) * f(1.5) + f(0.3))
    gamma = (rng.random(C) + 0.5).astype(f)
    beta = (rng.standard_normal(C) * 0.3).astype(f)
    look = None
    if pooled_kinds:
        look = np.ones(C, bool)
        w = (np.arange(F)[None, :] % pf) * pt + (np.arange(T)[:, None] % pt)          # [T,F] window element of a position
        for c, kind in pooled_special_channels(C):
            gamma[c], beta[c] = [(0.0, 0.5), (0.0, -0.2), (1e-5, 0.6), (-1e-3, 0.5)][kind]
            y[..., c] = np.round(y[..., c] * 4) / 4 + (w * 0.0625).astype(f)
            look[c] = False
        gamma[20] = -0.7
    mean, rstd, scale, shift = bn_stats(y, gamma, beta)
    y, share = repair_near_ties(y, scale, shift, pf, pt, look)
    return {"y": y, "gamma": gamma, "beta": beta, "mean": mean, "rstd": rstd, "scale": scale, "shift": shift,
            "share": share, "N": B * T * F}
