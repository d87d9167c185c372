"""numpy restatement of the resampler's definition, independent of sed_crnn_amd/resample.py.

L/M = sr_out/sr_in reduced, scale = min(1, L/M), fc = rolloff*scale, half = ceil(zeros/scale/rolloff), K = 2*half;
h[p][k] = fc sinc(fc t) I0(beta sqrt(1 - (t/half)^2)) / I0(beta) with t = p/L - (k - half + 1);
y[m] = sum_k h[p][k] x[i_c - half + 1 + k], u = m M, i_c = u div L, p = u mod L, x = 0 outside [0, N), ceil(N L / M) outputs.
"""
import math

import numpy as np


def design(sr_in, sr_out=44100, zeros=24, rolloff=0.92, beta=10.0):
    """-> (L, M, half, h float64 [L, 2*half])"""
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    scale = min(1.0, L / M)
    fc = rolloff * scale
    half = int(math.ceil(zeros / scale / rolloff))
    p = np.arange(L, dtype=np.float64)[:, None] / L
    k = np.arange(2 * half, dtype=np.float64)[None, :]
    t = p - (k - half + 1)
    w = np.i0(beta * np.sqrt(np.clip(1.0 - (t / half) ** 2, 0.0, None))) / np.i0(beta)
    return L, M, half, fc * np.sinc(fc * t) * w


def n_out(n_in, L, M):
    return -(-int(n_in) * L // M)


def _gather(x, L, M, half):
    """-> (samples [n_out, K] with the zero padding resolved, phase [n_out])"""
    N = len(x)
    m = np.arange(n_out(N, L, M), dtype=np.int64)
    u = m * M
    ic, ph = u // L, u % L
    xp = np.concatenate([np.zeros(half, x.dtype), x, np.zeros(half + 1, x.dtype)])
    idx = ic[:, None] + 1 + np.arange(2 * half, dtype=np.int64)[None, :]      # (i_c - half + 1 + k) + half
    return xp[idx], ph


def resample64(x, sr_in, sr_out=44100, **kw):
    """the definition in float64, float64 table"""
    L, M, half, h = design(sr_in, sr_out, **kw)
    xs, ph = _gather(np.asarray(x, np.float64), L, M, half)
    return (xs * h[ph]).sum(1)


def resample32(x, sr_in, sr_out=44100, **kw):
    """float32 variant: the table rounded to float32, float32 products, summed in float32 in tap order k = 0 .. K-1"""
    L, M, half, h = design(sr_in, sr_out, **kw)
    xs, ph = _gather(np.asarray(x, np.float32), L, M, half)
    hs = h.astype(np.float32)[ph]
    acc = np.zeros(xs.shape[0], np.float32)
    for k in range(2 * half):
        acc = (acc + hs[:, k] * xs[:, k]).astype(np.float32)
    return acc


def prototype_fir(sr_in, sr_out=44100, **kw):
    """the same prototype laid out as ONE FIR at the rate sr_in * L: g[j + half L] for j = -half L .. half L, where tap
    (p, k) sits at j = p + (half - 1 - k) L (the output's time minus the sample's, in units of 1/L input samples)"""
    L, M, half, h = design(sr_in, sr_out, **kw)
    g = np.zeros(2 * half * L + 1)
    p = np.arange(L)[:, None]
    k = np.arange(2 * half)[None, :]
    g[(p + (half - 1 - k) * L + half * L).ravel()] = h.ravel()
    return L, M, half, g
