"""Contrast SRP-PHAT restated in numpy on top of tests/doa_ref.py, doa_track_ref.py and mvdr_quiet_ref.py's activity.
TEST INFRASTRUCTURE.

The rule is integer and reads the event table and the settings alone.  With H = tf hop and L = n // H + 1 output frames:

    mask[t]          DESIGN 5w's activity of the whole table: bit cls of every row for onset <= t < min(offset, L)
    candidate q      of an event of class k with a = onset tf: feature frame g = a - G - 1 - q, q = 0 .. S-1, exists when g >= 0,
                     eligible when bit k of mask[t] is clear for t = max(g hop - 1024, 0) // H .. min(ceil((g hop + 1024) / H), L) - 1
    background       the first Nb eligible candidates in ascending q, nb of them; nb < M: none.  bg_sel lists them in summation
                     order (descending q: ascending time), -1 behind them

    Sb = sum of Pk_g over the selected frames (chunks of 32 consecutive list entries, each added in ascending order, the chunk
         partials in ascending order, as S's are),  w = float32(weight nf / nb),  S' = S - w Sb
    fine, srp, dir, doa_power = srp[dir] / (P nf) follow from S' by doa_ref's text; a track block b of n_b frames is contrasted
    with the same Sb and w_b = float32(weight n_b / nb).

``f32=True`` is the float32 yardstick: the same definition with ``torch.fft`` spectra and float32 sums in the order above.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import doa_track_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402

from sed_crnn_amd.localize import event_frames  # noqa: E402

CHUNK = 32
HALF = 1024          # half a frame of 2048 samples

activity = mvdr_quiet_ref.activity


# ───────────── the selection ─────────────
def eligible(mask, a, k, n, tf, hop, G, S):
    """-> the eligible candidates q of an event of class k whose first feature frame is a, ascending"""
    H = tf * hop
    L = n // H + 1
    out = []
    for q in range(S):
        g = a - G - 1 - q
        if g < 0:
            break
        t0, t1 = max(g * hop - HALF, 0) // H, min(-(-(g * hop + HALF) // H), L)
        if not any(int(mask[t]) >> k & 1 for t in range(t0, t1)):
            out.append(q)
    return out


def select(mask, onset, k, nf, n, tf, hop, Nb, G, S, M, n_classes):
    """-> (nb, sel [Nb]) of an event located on nf frames"""
    sel = np.full(Nb, -1, np.int32)
    if nf <= 0 or not 0 <= k < n_classes:
        return 0, sel
    qs = eligible(mask, onset * tf, k, n, tf, hop, G, S)[:Nb]
    if len(qs) < M:
        return 0, sel
    sel[:len(qs)] = qs[::-1]
    return len(qs), sel


def frames_of(rows, cls, n, tf, hop, max_frames, ct, n_classes):
    """rows [(onset, offset, peak_frame)] and cls of ONE recording of n samples, ct a sed.Contrast -> (bg_frames [E], bg_sel [E, Nb])"""
    mask = activity(rows, cls, n, tf * hop, n_classes)
    bg, sel = np.zeros(len(rows), np.int32), np.full((len(rows), ct.frames), -1, np.int32)
    for e, ((on, off, pk), k) in enumerate(zip(rows, cls)):
        f0, f1 = event_frames(on, off, pk, tf, 1 + n // hop, max_frames)
        bg[e], sel[e] = select(mask, on, k, f1 - f0, n, tf, hop, ct.frames, ct.guard, ct.search, ct.min_frames, n_classes)
    return bg, sel


# ───────────── the sums ─────────────
def chunk_sum(Pk, frames):
    """sum of Pk[f] over the list ``frames`` in Pk's own precision: chunks of 32 consecutive entries, each added in ascending
    order, the partials in ascending order"""
    total = None
    for c0 in range(0, len(frames), CHUNK):
        part = Pk[frames[c0]].copy()
        for f in frames[c0 + 1:c0 + CHUNK]:
            part = part + Pk[f]
        total = part if total is None else total + part
    return total


def contrasted(S, Sb, weight, n, nb):
    """S' = S - w Sb with w = float32(weight n / nb), in S's own precision"""
    w = np.float32(float(weight) * n / nb)
    return S - (w if S.dtype == np.complex64 else float(w)) * Sb


def _fine(S, max_lag, Q):
    """doa_ref's fine curves in S's own precision.  (At Q = 1 bin 1024 is the transform's own Nyquist bin and counts once:
    doa_ref.fine_curves_f32 halves it for every Q, which at Q = 1 would put 0.5 Re S[1024] / 2048 into the yardstick's error.)"""
    if S.dtype != np.complex64:
        return doa_ref.fine_curves(S, max_lag, Q)
    if Q > 1:
        return doa_ref.fine_curves_f32(S, max_lag, Q)
    import torch
    full = torch.fft.irfft(torch.from_numpy(np.ascontiguousarray(S)), n=doa_ref.NFFT, dim=-1)
    return torch.cat([full[..., doa_ref.NFFT - max_lag:], full[..., :max_lag + 1]], dim=-1).numpy()


def event_doa(Pk, rows, cls, n, tf, hop, J, max_lag, Q, max_frames, ct, n_classes, f32=False):
    """Pk [frames, P, 1025] of ONE recording of n samples (``doa_ref.whitened``; ``whitened_f32`` with ``f32=True``) -> dict(srp
    [E, D], dir [E], doa_power [E], loc_frames [E], bg_frames [E], bg_sel [E, Nb], ranges)"""
    P, F, E, D = Pk.shape[1], max_lag * Q, len(rows), J.shape[0]
    bg, sel = frames_of(rows, cls, n, tf, hop, max_frames, ct, n_classes)
    real = np.float32 if f32 else np.float64
    out = dict(srp=np.zeros((E, D), real), dir=np.full(E, -1, np.int64), doa_power=np.zeros(E), loc_frames=np.zeros(E, np.int32),
               bg_frames=bg, bg_sel=sel, ranges=[])
    for e, (on, off, pk) in enumerate(rows):
        f0, f1 = event_frames(on, off, pk, tf, Pk.shape[0], max_frames)
        out["ranges"].append((f0, f1))
        out["loc_frames"][e] = f1 - f0
        if f1 == f0:
            continue
        S = chunk_sum(Pk, list(range(f0, f1)))
        if bg[e]:
            g0 = on * tf - ct.guard - 1
            S = contrasted(S, chunk_sum(Pk, [g0 - int(q) for q in sel[e, :bg[e]]]), ct.weight, f1 - f0, int(bg[e]))
        out["srp"][e] = doa_ref._steer(_fine(S, max_lag, Q), J, F)
        out["dir"][e], out["doa_power"][e] = doa_ref.pick(out["srp"][e], P, f1 - f0)
    return out


def block_maps(Pk, f0, nf, W, J, max_lag, Q, onset, tf, ct, nb, sel):
    """the contrasted block maps of one event (``doa_track_ref.block_maps`` with every block's S replaced by S_b - w_b Sb) ->
    (maps [T, D], raw [T], power [T]); nb = 0: the plain ones"""
    P, F = Pk.shape[1], max_lag * Q
    Sb = chunk_sum(Pk, [onset * tf - ct.guard - 1 - int(q) for q in sel[:nb]]) if nb else None
    maps, raw, power = [], [], []
    for first, n in doa_track_ref.blocks(nf, W):
        S = chunk_sum(Pk, list(range(f0 + first, f0 + first + n)))
        if nb:
            S = contrasted(S, Sb, ct.weight, n, nb)
        m = doa_ref._steer(_fine(S, max_lag, Q), J, F)
        d, pw = doa_ref.pick(m, P, n)
        maps.append(m); raw.append(d); power.append(pw)
    real = np.float32 if Pk.dtype == np.complex64 else np.float64
    return (np.stack(maps) if maps else np.zeros((0, J.shape[0]), real)), np.array(raw, np.int64), np.array(power)


# ───────────── the scene: a target over a louder source of another class ─────────────
SR, HOP, EDGE, RING, Q = 44100, 1024, 0.06, 72, 8
TARGET = (24, 36)                                    # the target's frames
PAIRS_DEG = ((22.0, 92.0), (63.0, 203.0), (131.0, 291.0), (247.0, 87.0), (312.0, 152.0), (172.0, 12.0))   # (target, interferer): 70..160 apart
N_FRAMES = 48


def scene_parts(target_deg, other_deg, other_db, seed, positions=None, target=TARGET):
    """-> (target, interferer, noise), each [n, C] float64 at 44.1 kHz on a 6 cm tetrahedron; the scene is their sum: a white
    far-field target in the frames ``target`` = [24, 36) (its samples [24 hop, 36 hop)), a white far-field interferer
    ``other_db`` dB above it through the whole recording (None: none), and sensor noise 30 dB below the target"""
    r = doa_ref.tetrahedron(EDGE) if positions is None else positions
    n = N_FRAMES * HOP
    xs, xi = np.zeros((n, r.shape[0])), np.zeros((n, r.shape[0]))
    a, b = target[0] * HOP, target[1] * HOP
    xs[a:b] = doa_ref.far_field(b - a, r, doa_ref.unit(math.radians(target_deg)), SR, seed, noise=0.0).astype(np.float64)
    if other_db is not None:
        xi = 10.0 ** (other_db / 20.0) * doa_ref.far_field(n, r, doa_ref.unit(math.radians(other_deg)), SR, seed + 1, noise=0.0).astype(np.float64)
    xn = 10.0 ** (-30.0 / 20.0) * 0.3 * np.random.default_rng(seed + 2).standard_normal(xs.shape)
    return xs, xi, xn


def scene(target_deg, other_deg, other_db, seed, positions=None, target=TARGET):
    """[n, C] float32: the sum of ``scene_parts``"""
    return sum(scene_parts(target_deg, other_deg, other_db, seed, positions, target)).astype(np.float32)


def ring_units(n=RING):
    az = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(az), np.sin(az), np.zeros(n)], 1)
