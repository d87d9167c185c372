"""Per-event direction of arrival by SRP-PHAT over a grid, restated in numpy float64.  TEST INFRASTRUCTURE.

Built on tests/spatial_ref.py and tests/tdoa_ref.py: with Pk_f the whitened cross spectrum of frame f and pair p = (i, j), i < j
in lexicographic order, as spatial_ref.gcc_phat defines it (thresholds, real DC and Nyquist bins), an event located on the
frames [f0, f1) (sed_crnn_amd.localize.event_frames) has, for the oversampling factor Q and F = max_lag Q,

    S[k]      = sum_{f = f0}^{f1 - 1} Pk_f[k]
    fine_p[j] = (1/2048) (S[0] + Re S[1024] cos(pi j / Q) + 2 sum_{k=1..1023} Re(S[k] e^{+2 pi i k j / (2048 Q)})),   |j| <= F
    tau[d, p] = sr (r_j - r_i) . u_d / c,     J[d, p] = round_half_even(Q tau[d, p]),     max_lag = max_p ceil(sr |r_j - r_i| / c)
    srp[d]    = sum_p fine_p[J[d, p]]
    dir       = the first maximum of srp in ascending d;   doa_power = srp[dir] / (P (f1 - f0))

and dir = -1, doa_power = 0 where the event has no frames or every srp value is 0.  ``fine`` at Q = 1 is tdoa_ref's ``acc``
without its two outermost lags.  ``yardstick`` evaluates the same sums in float32 (torch.fft on the CPU, as
spatial_ref.gcc_phat_f32 does).  ``far_field`` makes the test signals.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_ref  # noqa: E402
from sed_crnn_amd.localize import event_frames  # noqa: E402

NFFT = spatial_ref.NFFT
C_SOUND = 343.0


# ───────────── geometry, stated again ─────────────
def unit(az, el=0.0):
    return np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])


def tetrahedron(edge):
    """4 microphones at the corners of a regular tetrahedron with edges of ``edge`` metres, centred on the origin"""
    v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return v * (edge / (2.0 * math.sqrt(2.0)))


def square(side):
    """4 microphones at the corners of a square with sides of ``side`` metres in the z = 0 plane"""
    h = side / 2.0
    return np.array([[h, h, 0.0], [-h, h, 0.0], [-h, -h, 0.0], [h, -h, 0.0]])


def line(C, spacing):
    """C microphones ``spacing`` metres apart on a slanted line (every pair has its own spacing)"""
    return np.arange(C)[:, None] * (spacing * np.array([[0.8, 0.5, math.sqrt(1.0 - 0.64 - 0.25)]]))


def steering(positions, units, sr, Q, c=C_SOUND):
    """-> (tau float64 [D, P], J int64 [D, P], max_lag)"""
    r, u = np.asarray(positions, np.float64), np.asarray(units, np.float64)
    base = np.stack([r[j] - r[i] for i, j in spatial_ref.pairs(len(r))])
    tau = sr * (u @ base.T) / c
    max_lag = max(int(math.ceil(sr * float(np.linalg.norm(b)) / c)) for b in base)
    return tau, np.rint(tau * Q).astype(np.int64), max_lag


def angle_between(u, v):
    return float(np.arccos(np.clip(np.dot(u, v), -1.0, 1.0)))


def covering_radius(units, samples=20000, seed=0, in_plane=False):
    """the largest angle from a direction to its nearest grid direction, over ``samples`` random directions (of the sphere, or of
    the z = 0 circle): a lower estimate of the grid's covering radius that is tight for these grids"""
    rng = np.random.default_rng(seed)
    if in_plane:
        a = rng.uniform(0.0, 2.0 * np.pi, samples)
        v = np.stack([np.cos(a), np.sin(a), np.zeros(samples)], 1)
    else:
        v = rng.standard_normal((samples, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
    return float(np.arccos(np.clip((v @ np.asarray(units).T).max(1), -1.0, 1.0)).max())


# ───────────── test signals ─────────────
def far_field(n, positions, u, sr, seed, noise=0.2, c=C_SOUND):
    """[n, C] float32: a white burst from the far-field direction ``u`` (a unit vector from the array to the source): channel c
    is the burst delayed by -sr r_c . u / c samples (a phase ramp in a float64 FFT, zero-padded so that nothing wraps), plus
    ``noise`` x independent white noise"""
    rng = np.random.default_rng(seed)
    r = np.asarray(positions, np.float64)
    delay = -sr * (r @ np.asarray(u, np.float64)) / c
    guard = int(math.ceil(np.abs(delay).max())) + 8
    m = n + 2 * guard
    X = np.fft.rfft(rng.standard_normal(m))
    f = np.arange(X.size) / m
    x = np.stack([np.fft.irfft(X * np.exp(-2j * np.pi * f * d), n=m)[guard: guard + n] + noise * rng.standard_normal(n) for d in delay], 1)
    return (0.3 * x).astype(np.float32)


# ───────────── the definition ─────────────
def whitened(x, hop=1024, pad_mode="constant"):
    """x [N, C] -> Pk complex128 [frames, P, 1025]"""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[1]
    spec = [np.fft.rfft(spatial_ref.frames_of(x[:, c], hop, pad_mode).astype(np.float64), axis=1) for c in range(C)]
    out = []
    for i, j in spatial_ref.pairs(C):
        G = spec[i] * np.conj(spec[j])
        m2 = G.real ** 2 + G.imag ** 2
        ok = m2 >= spatial_ref.M2_MIN
        Pk = np.where(ok, G / np.sqrt(np.where(ok, m2, 1.0)), 0.0)
        Pk[:, 0] = Pk[:, 0].real
        Pk[:, -1] = Pk[:, -1].real
        out.append(Pk)
    return np.stack(out, 1)


def whitened_f32(x, hop=1024, pad_mode="constant"):
    """the same in float32 (torch.fft on the CPU) -> complex64 [frames, P, 1025]"""
    import torch
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[1]
    spec = [torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(spatial_ref.frames_of(x[:, c], hop, pad_mode))), dim=1) for c in range(C)]
    out = []
    for i, j in spatial_ref.pairs(C):
        G = spec[i] * torch.conj(spec[j])
        m2 = G.real ** 2 + G.imag ** 2
        ok = m2 >= spatial_ref.M2_MIN
        Pk = torch.where(ok, G / torch.sqrt(torch.where(ok, m2, torch.ones_like(m2))), torch.zeros_like(G)).numpy().copy()
        Pk[:, 0] = Pk[:, 0].real
        Pk[:, -1] = Pk[:, -1].real
        out.append(Pk)
    return np.stack(out, 1)


def fine_curves(S, max_lag, Q):
    """S [..., 1025] complex128 -> fine [..., 2 F + 1] float64, lag j / Q at column j + F"""
    F = max_lag * Q
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    j = np.arange(-F, F + 1, dtype=np.float64)
    ang = 2.0 * np.pi * k[:, None] * j[None, :] / (NFFT * Q)
    wt = np.full(NFFT // 2 + 1, 2.0)
    wt[0] = wt[-1] = 1.0
    return ((S.real * wt) @ np.cos(ang) - (S.imag * wt) @ np.sin(ang)) / NFFT


def fine_curves_f32(S, max_lag, Q):
    """S [..., 1025] complex64 -> the same columns in float32: Q x the inverse real transform of 2048 Q points (whose bin 1024,
    now an interior bin, counts twice: it is halved first)"""
    import torch
    F = max_lag * Q
    S = np.array(S, dtype=np.complex64)
    S[..., -1] *= np.float32(0.5)
    full = torch.fft.irfft(torch.from_numpy(S), n=NFFT * Q, dim=-1) * np.float32(Q)
    return torch.cat([full[..., NFFT * Q - F:], full[..., :F + 1]], dim=-1).numpy()


def _steer(fine, J, F):
    """fine [P, 2 F + 1], J [D, P] -> srp [D], added in ascending p in fine's own precision"""
    srp = fine[0, J[:, 0] + F].copy()
    for p in range(1, fine.shape[0]):
        srp = srp + fine[p, J[:, p] + F]
    return srp


def pick(srp, P, n_frames):
    """-> (dir, doa_power)"""
    if n_frames == 0 or not np.any(srp):
        return -1, 0.0
    d = int(np.argmax(srp))                                           # the first maximum
    return d, float(srp[d]) / (P * n_frames)


def event_doa(Pk, events, time_factor, J, max_lag, Q, max_frames=256, f32=False):
    """Pk [frames, P, 1025] of ONE recording (``whitened``; ``whitened_f32`` with ``f32=True``: the yardstick, every sum in
    float32 in the order of the definition) and events [(onset, offset, peak_frame), ...] -> dict(srp [E, D], fine [E, P, 2F+1],
    dir [E], doa_power [E], loc_frames [E], ranges)"""
    n_feat, P = Pk.shape[:2]
    E, D, F = len(events), J.shape[0], max_lag * Q
    real = np.float32 if f32 else np.float64
    out = dict(srp=np.zeros((E, D), real), fine=np.zeros((E, P, 2 * F + 1), real), dir=np.full(E, -1, np.int64),
               doa_power=np.zeros(E), loc_frames=np.zeros(E, np.int32), ranges=[])
    for e, (on, off, pk) in enumerate(events):
        f0, f1 = event_frames(on, off, pk, time_factor, n_feat, max_frames)
        out["ranges"].append((f0, f1))
        out["loc_frames"][e] = f1 - f0
        if f1 == f0:
            continue
        if f32:
            S = Pk[f0].copy()
            for f in range(f0 + 1, f1):
                S = S + Pk[f]
            fine = fine_curves_f32(S, max_lag, Q)
        else:
            fine = fine_curves(Pk[f0:f1].sum(0), max_lag, Q)
        out["fine"][e] = fine
        out["srp"][e] = _steer(fine, J, F)
        out["dir"][e], out["doa_power"][e] = pick(out["srp"][e], P, f1 - f0)
    return out
