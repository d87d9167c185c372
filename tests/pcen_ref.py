"""PCEN (per-channel energy normalisation) as librosa.pcen composes it with max_size = 1, on this project's log-mel
values: float64 with scipy.signal.lfilter / lfilter_zi (the reference), and the same definition evaluated step by step in
float32 numpy (the yardstick a float32 kernel is measured with).  librosa itself is not needed.

    E[t] = scale * exp(x[t]);   T = time_constant * sr / hop;   b = (sqrt(1 + 4 T^2) - 1) / (2 T^2)
    M    = lfilter([b], [1, b - 1], E, zi = lfilter_zi(...) * E[0])      -> M[0] = E[0]
    pcen = (E * (eps + M)^-gain + bias)^power - bias^power;   out = (pcen - mu) * inv_sigma with a scaler
"""
import numpy as np
from scipy import signal

DEFAULTS = dict(gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, scale=1.0)


def smoothing(time_constant=0.4, sr=44100, hop=1024):
    t = time_constant * sr / hop
    return (np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t)


def smooth(E, b):
    """float64 [T, W] energies -> the smoother M, librosa's way: the filter starts in the steady state of a constant E[0]"""
    E = np.asarray(E, np.float64)
    zi = signal.lfilter_zi([b], [1.0, b - 1.0])
    M, _ = signal.lfilter([b], [1.0, b - 1.0], E, zi=zi.reshape(1, 1) * E[0:1], axis=0)
    return M


def pcen(logmel, b, gain=0.98, bias=2.0, power=0.5, eps=1e-6, scale=1.0, mu=None, inv_sigma=None, **_):
    """logmel [T, W] (float32 values, natural log; -inf = digital silence) -> float64 [T, W]"""
    x = np.asarray(logmel, np.float64)
    if x.shape[0] == 0:
        return x.copy()
    E = scale * np.exp(x)
    M = smooth(E, b)
    out = (E * (eps + M) ** (-gain) + bias) ** power - bias ** power
    if mu is not None:
        out = (out - np.asarray(mu, np.float64)) * np.asarray(inv_sigma, np.float64)
    return out


def pcen_f32(logmel, b, gain=0.98, bias=2.0, power=0.5, eps=1e-6, scale=1.0, mu=None, inv_sigma=None, **_):
    """the same definition with every operation in float32: the recurrence one frame after the other"""
    f = np.float32
    x = np.asarray(logmel, f)
    if x.shape[0] == 0:
        return x.copy()
    E = f(scale) * np.exp(x)
    a, bf = f(1.0 - b), f(b)
    M = np.empty_like(E)
    M[0] = E[0]
    for t in range(1, E.shape[0]):
        M[t] = a * M[t - 1] + bf * E[t]
    out = (E * (f(eps) + M) ** f(-gain) + f(bias)) ** f(power) - f(bias) ** f(power)
    if mu is not None:
        out = (out - np.asarray(mu, f)) * np.asarray(inv_sigma, f)
    assert out.dtype == f
    return out
