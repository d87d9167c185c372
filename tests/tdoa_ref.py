"""Per-event TDOA from accumulated GCC-PHAT, restated in numpy float64.  TEST INFRASTRUCTURE.

Built on tests/spatial_ref.py: with Pk_f the whitened cross spectrum of frame f and pair p as spatial_ref.gcc_phat defines it
(thresholds, real DC and Nyquist bins, pairs in lexicographic order) and cc_f[tau] its inverse transform at lag tau, an event
located on the frames [f0, f1) (sed_crnn_amd.localize.event_frames — the rule is stated there, once) has

    S[k]     = sum_{f = f0}^{f1 - 1} Pk_f[k]
    acc[tau] = (1/2048) (S[0] + (-1)^tau S[1024] + 2 sum_{k=1..1023} Re(S[k] e^{+2 pi i k tau / 2048}))  =  sum_f cc_f[tau]

(the inverse transform is linear: in exact arithmetic, and in float64 to ~1e-16, the two sides are the same number) for
tau = -(max_lag+1) .. max_lag+1.  t* = the first maximum of acc over |tau| <= max_lag in ascending order; with
l, m, r = acc[t*-1], acc[t*], acc[t*+1] and den = l - 2m + r:  lag = t* + 0.5 (l - r) / den if den < 0 else t*;
strength = m / (f1 - f0).  Where acc is 0 at every searched lag (digital silence), t* = 0: lag 0, strength 0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spatial_ref  # noqa: E402
from sed_crnn_amd.localize import event_frames  # noqa: E402


def broadband(n, delays, seed, noise=0.5):
    """[n, C] float32: a white source that reaches channel c with delay delays[c] (|d| <= 32 samples), plus ``noise`` x independent
    white noise per channel (the _broadband recipe of tests/test_gpu_spatial.py): every bin of every channel carries energy"""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal(n + 64)
    x = np.stack([src[32 - d: 32 - d + n] + noise * rng.standard_normal(n) for d in delays], 1)
    return (0.3 * x).astype(np.float32)


def frame_curves(x, hop=1024, max_lag=24, pad_mode="constant"):
    """x [N, C] -> (cc [frames, P, 2*max_lag + 3] float64: cc_f[tau] of every frame and pair at tau = -(max_lag+1) .. max_lag+1,
    the number of bins the definition zeroed)"""
    C = np.asarray(x).shape[1]
    P, L = C * (C - 1) // 2, 2 * (max_lag + 2)                        # gcc_phat gives tau = -(max_lag+2) .. max_lag+1: drop the first
    cc, zeroed = spatial_ref.gcc_phat(x, hop=hop, n_lags=L, pad_mode=pad_mode)
    return cc.reshape(cc.shape[0], P, L)[:, :, 1:], zeroed


def frame_curves_f32(x, hop=1024, max_lag=24, pad_mode="constant"):
    """the same rows from spatial_ref.gcc_phat_f32 (float32, torch.fft on the CPU): what the yardstick sums"""
    C = np.asarray(x).shape[1]
    P, L = C * (C - 1) // 2, 2 * (max_lag + 2)
    cc = spatial_ref.gcc_phat_f32(x, hop=hop, n_lags=L, pad_mode=pad_mode)
    return cc.reshape(cc.shape[0], P, L)[:, :, 1:]


def narrow(curves, max_lag):
    """curves [..., 2*M + 3] made for a larger max_lag M -> the columns of ``max_lag``"""
    M = (curves.shape[-1] - 3) // 2
    return curves[..., M - max_lag: M + max_lag + 3]


def peak(acc, n_frames):
    """acc [2*max_lag + 3] (any float type; computed in float64) -> (lag, strength, t*, second / m): the last one is the largest
    value among the searched lags more than one lag away from t*, relative to the peak value (0 when there is no such lag, inf when the peak is not positive)"""
    acc = np.asarray(acc, dtype=np.float64)
    max_lag = (acc.size - 3) // 2
    c = max_lag + 1
    seg = acc[1:-1]                                                    # |tau| <= max_lag
    t = int(np.argmax(seg)) - max_lag if seg.any() else 0             # argmax returns the first maximum
    l, m, r = acc[c + t - 1], acc[c + t], acc[c + t + 1]
    den = l - 2.0 * m + r
    lag = t + 0.5 * (l - r) / den if den < 0 else float(t)
    far = np.abs(np.arange(-max_lag, max_lag + 1) - t) > 1
    second = 0.0 if not far.any() else float(seg[far].max()) / m if m > 0 else np.inf     # no positive peak: anything may win
    return lag, (m / n_frames if n_frames else 0.0), t, second


def event_tdoa(curves, events, time_factor, max_frames=256):
    """curves [frames, P, W] of ONE recording (``frame_curves``) and events [(onset, offset, peak_frame), ...] ->
    dict(acc [E, P, W], lag [E, P], strength [E, P], t [E, P], second [E, P], loc_frames [E], ranges [(f0, f1), ...])"""
    n_feat, P, W = curves.shape
    E = len(events)
    out = dict(acc=np.zeros((E, P, W)), lag=np.zeros((E, P)), strength=np.zeros((E, P)), t=np.zeros((E, P), np.int64),
               second=np.zeros((E, P)), loc_frames=np.zeros(E, np.int32), ranges=[])
    for e, (on, off, pk) in enumerate(events):
        f0, f1 = event_frames(on, off, pk, time_factor, n_feat, max_frames)
        out["ranges"].append((f0, f1))
        out["loc_frames"][e] = f1 - f0
        if f1 == f0:
            continue
        out["acc"][e] = curves[f0:f1].sum(0)
        for p in range(P):
            out["lag"][e, p], out["strength"][e, p], out["t"][e, p], out["second"][e, p] = peak(out["acc"][e, p], f1 - f0)
    return out


def yardstick_acc(curves32, ranges):
    """float32 rows summed in float32 in frame order -> [E, P, W] float32 (zeros for an event without frames)"""
    curves32 = np.asarray(curves32, dtype=np.float32)
    out = np.zeros((len(ranges),) + curves32.shape[1:], np.float32)
    for e, (f0, f1) in enumerate(ranges):
        for f in range(f0, f1):
            out[e] = out[e] + curves32[f]
    return out
