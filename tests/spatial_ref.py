"""GCC-PHAT spatial features, restated in numpy float64.  TEST INFRASTRUCTURE.

For a recording x [N, C] (C >= 2), frame f of channel c is framed, padded and windowed as the log-mel front end does it
(n_fft 2048, centred, periodic Hann in float32, the product taken in float32); its spectrum is X_c[k], k = 0..1024.  The
P = C(C-1)/2 pairs (i, j), i < j, come in lexicographic order, and for pair p

    G[k]    = X_i[k] conj X_j[k]
    m2      = Re(G)^2 + Im(G)^2
    Pk[k]   = G[k] / sqrt(m2)  if m2 >= 1e-30 else 0
    cc[tau] = (1/2048) (Pk[0] + (-1)^tau Pk[1024] + 2 sum_{k=1..1023} Re(Pk[k] e^{+2 pi i k tau / 2048})),  tau = -L/2 .. L/2-1

sits in columns [p*L, (p+1)*L) of the result, cc[tau] in column tau + L/2.
"""
import numpy as np

NFFT = 2048
M2_MIN = 1e-30


def hann_periodic(n=NFFT):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)


def pairs(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def frames_of(y, hop, pad_mode="constant"):
    """windowed frames [1 + N//hop, 2048] float32 of one channel"""
    y = np.asarray(y, dtype=np.float32)
    if pad_mode == "reflect" and y.size < 2:
        pad_mode = "constant"                                      # a single sample has nothing to reflect: zeros
    yp = np.pad(y, NFFT // 2, mode=pad_mode) if (pad_mode == "constant" or y.size > NFFT // 2) else _reflect_pad(y)
    n_frames = 1 + y.size // hop
    idx = np.arange(NFFT)[None, :] + hop * np.arange(n_frames)[:, None]
    return yp[idx] * hann_periodic()[None, :]


def _reflect_pad(y):
    """numpy 'reflect' for a signal shorter than the pad: index n -> the reflection with period 2 (N - 1)"""
    n = np.arange(-NFFT // 2, y.size + NFFT // 2)
    period = 2 * (y.size - 1)
    r = np.mod(n, period)
    r = np.where(r >= y.size, period - r, r)
    return y[r]


def gcc_phat(x, hop=1024, n_lags=40, pad_mode="constant"):
    """x [N, C] -> (cc [frames, P*n_lags] float64, number of bins that fell under the m2 threshold)"""
    x = np.asarray(x, dtype=np.float32)
    C, L = x.shape[1], int(n_lags)
    spec = [np.fft.rfft(frames_of(x[:, c], hop, pad_mode).astype(np.float64), axis=1) for c in range(C)]
    k = np.arange(NFFT // 2 + 1, dtype=np.float64)
    tau = np.arange(-L // 2, L // 2, dtype=np.float64)
    ang = 2.0 * np.pi * k[:, None] * tau[None, :] / NFFT            # [1025, L]
    wt = np.full(NFFT // 2 + 1, 2.0)
    wt[0] = wt[-1] = 1.0
    out, zeroed = [], 0
    for i, j in pairs(C):
        G = spec[i] * np.conj(spec[j])
        m2 = G.real ** 2 + G.imag ** 2
        ok = m2 >= M2_MIN
        zeroed += int((~ok).sum())
        Pk = np.where(ok, G / np.sqrt(np.where(ok, m2, 1.0)), 0.0)
        Pk[:, 0] = Pk[:, 0].real                                    # the DC and Nyquist bins of a real signal are real
        Pk[:, -1] = Pk[:, -1].real
        cc = ((Pk.real * wt) @ np.cos(ang) - (Pk.imag * wt) @ np.sin(ang)) / NFFT
        out.append(cc)
    return np.concatenate(out, axis=1), zeroed


def gcc_phat_f32(x, hop=1024, n_lags=40, pad_mode="constant"):
    """the same definition evaluated in float32 with torch.fft on the CPU: the yardstick for a float32 implementation"""
    import torch
    x = np.asarray(x, dtype=np.float32)
    C, L = x.shape[1], int(n_lags)
    spec = [torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames_of(x[:, c], hop, pad_mode))), dim=1) for c in range(C)]
    out = []
    for i, j in pairs(C):
        G = spec[i] * torch.conj(spec[j])
        m2 = G.real ** 2 + G.imag ** 2
        ok = m2 >= M2_MIN
        Pk = torch.where(ok, G / torch.sqrt(torch.where(ok, m2, torch.ones_like(m2))), torch.zeros_like(G))
        full = torch.fft.irfft(Pk, n=NFFT, dim=1)                   # cc[tau] at index tau mod 2048
        out.append(torch.cat([full[:, NFFT - L // 2:], full[:, :L // 2]], dim=1))
    return torch.cat(out, dim=1).numpy()
