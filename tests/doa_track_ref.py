"""Direction tracks restated in numpy on top of tests/doa_ref.py.  TEST INFRASTRUCTURE.

An event located on the frames [f0, f0 + nf) is cut into blocks of W chunks of 32 frames:

    nch = ceil(nf / 32),  T0 = ceil(nch / W),  nl = nf - 32 W (T0 - 1)
    T   = T0 - 1 where T0 > 1 and nl < 16 W (the short tail joins the block before it), else T0;   nf = 0: T = 0
    block b = frames [f0 + 32 W b, f0 + 32 W (b + 1)), the last block up to f0 + nf

``block_maps`` is doa_ref's srp of every block alone, in float64 (or, ``f32=True``, the float32 yardstick: every sum in float32
in the order of the definition).  With a neighbour table (off [D + 1], idx [nnz]: row d lists the directions the path may come
to d from) the track is the best path through the maps,

    s_0 = m_0,   s_b[d] = m_b[d] + max_j s_{b-1}[idx[off[d] + j]],   the path ends at the first maximum of s_{T-1}

``path_f32`` restates that in float32 in the kernel's order — one add per cell, the first maximum in ascending j and in
ascending d — and is exactly reproducible; ``path_f64`` is the same recurrence in float64.  ``scene`` makes the moving source of
the tests.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402

CHUNK = 32


# ───────────── the block rule, stated again ─────────────
def blocks(nf, W):
    """-> [(first frame counted from f0, frames), ...] of an event located on nf frames"""
    if nf <= 0:
        return []
    nch = (nf + CHUNK - 1) // CHUNK
    T0 = (nch + W - 1) // W
    nl = nf - CHUNK * W * (T0 - 1)
    T = T0 - 1 if (T0 > 1 and nl < 16 * W) else T0
    out = [(CHUNK * W * b, CHUNK * W) for b in range(T)]
    out[-1] = (CHUNK * W * (T - 1), nf - CHUNK * W * (T - 1))
    return out


def max_blocks(max_frames, W):
    return -(-(-(-max_frames // CHUNK)) // W)


# ───────────── block maps ─────────────
def block_maps(Pk, f0, nf, W, J, max_lag, Q, f32=False):
    """Pk [frames, P, 1025] (doa_ref.whitened; whitened_f32 with ``f32=True``) -> (maps [T, D], raw [T], power [T])"""
    P, F = Pk.shape[1], max_lag * Q
    maps, raw, power = [], [], []
    for first, n in blocks(nf, W):
        a = f0 + first
        if f32:
            S = Pk[a].copy()
            for f in range(a + 1, a + n):
                S = S + Pk[f]
            fine = doa_ref.fine_curves_f32(S, max_lag, Q)
        else:
            fine = doa_ref.fine_curves(Pk[a:a + n].sum(0), max_lag, Q)
        m = doa_ref._steer(fine, J, F)
        d, pw = doa_ref.pick(m, P, n)
        maps.append(m); raw.append(d); power.append(pw)
    D = J.shape[0]
    return (np.stack(maps) if maps else np.zeros((0, D), np.float32 if f32 else np.float64)), np.array(raw, np.int64), np.array(power)


# ───────────── the path ─────────────
def _path(maps, off, idx, real):
    maps = np.asarray(maps, dtype=real)
    T, D = maps.shape
    off, idx = np.asarray(off, np.int64), np.clip(np.asarray(idx, np.int64), 0, D - 1)
    assert off.shape == (D + 1,) and (np.diff(off) >= 1).all() and off[-1] == idx.shape[0]
    pos = np.arange(idx.shape[0])
    counts = np.diff(off)
    s = maps[0].copy()
    back = np.zeros((T, D), np.int64)
    for b in range(1, T):
        vals = s[idx]
        best = np.maximum.reduceat(vals, off[:-1])
        first = np.minimum.reduceat(np.where(vals == np.repeat(best, counts), pos, idx.shape[0]), off[:-1])    # ascending j: the first maximum
        back[b] = idx[first]
        s = (maps[b] + best).astype(real)                                           # one add per cell
    d = int(np.argmax(s))                                                           # the first maximum in ascending d
    out = np.zeros(T, np.int64)
    for b in range(T - 1, -1, -1):
        out[b] = d
        d = back[b, d]
    return out


def path_f32(maps, off, idx):
    """the kernel's recurrence in its own precision and order -> the path's directions [T]"""
    return _path(maps, off, idx, np.float32)


def path_f64(maps, off, idx):
    return _path(maps, off, idx, np.float64)


def track_dir(maps, raw, off=None, idx=None, f32=True):
    """trk_dir of one event from its maps [T, D] and raw directions [T]: the path where a table is given, -1 where raw is -1"""
    raw = np.asarray(raw, np.int64)
    if off is None or len(raw) == 0:
        return raw.copy()
    p = (path_f32 if f32 else path_f64)(maps, off, idx)
    return np.where(raw < 0, -1, p)


def neighbours(units, max_step_deg):
    """brute force, one row at a time -> (off, idx)"""
    u = np.asarray(units, np.float64)
    off, idx = [0], []
    for d in range(u.shape[0]):
        ang = np.arccos(np.clip(u @ u[d], -1.0, 1.0))
        row = [int(k) for k in np.nonzero(ang <= math.radians(max_step_deg) + 1e-9)[0]]
        if d not in row:
            row = sorted(row + [d])
        idx += row
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32)


# ───────────── the scene: a source that moves, and a louder one for the length of one block ─────────────
SCENE_BLOCKS, SCENE_STEP_DEG, SCENE_START_DEG, SCENE_OTHER_DEG, SCENE_OTHER_DB, SCENE_OTHER_BLOCK = 8, 10.0, 20.0, 120.0, 10.0, 4


def scene_truth():
    """the source's azimuth in every block, radians"""
    return np.radians(SCENE_START_DEG + SCENE_STEP_DEG * np.arange(SCENE_BLOCKS))


def scene(positions, sr, hop=1024, seed=500):
    """[8 * 32 * hop, C] float32: block b (32 frames) holds a far-field source at azimuth 20 + 10 b degrees in the array's plane;
    in block 4 a second source 120 degrees further round is 10 dB stronger.  The event is the frames [0, 256)."""
    n = CHUNK * hop
    parts = []
    for b, az in enumerate(scene_truth()):
        x = doa_ref.far_field(n, positions, doa_ref.unit(az), sr, seed=seed + b).astype(np.float64)
        if b == SCENE_OTHER_BLOCK:
            g = 10.0 ** (SCENE_OTHER_DB / 20.0)
            x = x + g * doa_ref.far_field(n, positions, doa_ref.unit(az + math.radians(SCENE_OTHER_DEG)), sr, seed=seed + 100, noise=0.0)
        parts.append(x)
    return np.concatenate(parts).astype(np.float32)
