"""Per-event audio by an adaptive (MVDR) beam, restated in numpy float64.  TEST INFRASTRUCTURE.

The events, their samples [s0, s1) and audio_len / audio_start are the delay-and-sum beam's (tests/beam_ref.py, ``spans``).  The
transform grid is the event's own: N = 2048, B = 1024, len = s1 - s0, J = ceil(len / B); frame j = 0..J holds
x_c[s0 + (j - 1) B + m], m = 0..2047, with EVERY sample outside [s0, s1) read as 0.  Window (analysis and synthesis):
w[m] = sqrt(0.5 - 0.5 cos(2 pi m / 2048)), so that w[m]^2 + w[m + B]^2 = 1.  With X_{c,j} the half spectrum (k = 0..1024) of the
windowed frame j of channel c and tau_c = steering_delays[dir][c] (float64 samples, not rounded):

    R[k]  = sum_{j=0..J} X_j[k] X_j[k]^H                          (C x C, ascending j)
    d_c   = exp(+2 pi i k tau_c / 2048);   lambda = loading trace(R[k]) / C
    v     = (R[k] + lambda I)^-1 d;   w[k] = v / (d^H v);   trace(R[k]) not > 0:  w[k] = d / C
    Y_j[k] = sum_c conj(w_c[k]) X_{c,j}[k]                        (ascending c; the imaginary parts of Y[0] and Y[1024] are dropped)
    v_j   = irfft(Y_j);   output sample i = j B + m < len:  w[m + B] v_j[m + B] + w[m] v_{j+1}[m]

``beamform`` evaluates this in float64 with the float64 window — the definition — or, with ``f32=True``, the way the kernel does
its arithmetic: the window rounded once to float32, the transforms in float32 (torch.fft on the CPU), R accumulated in complex64
in ascending j, the solve in float64, w rounded once to complex64, the combine in complex64 in ascending c, the inverse transform
and the two products and the add of the overlap in float32: the yardstick.  ``event`` does one event and can pass further signals
through the weights it made (the beam is linear once its weights are fixed): how the output SIR of ``scene`` is measured.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402

N, B = 2048, 1024
C_SOUND = beam_ref.C_SOUND


def window(f32=False):
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N))
    return w.astype(np.float32) if f32 else w


def steering(tau_row):
    """d [1025, C] complex128: d_c[k] = exp(+2 pi i k tau_c / 2048)"""
    k = np.arange(B + 1, dtype=np.float64)[:, None]
    return np.exp(2j * np.pi * k * np.asarray(tau_row, np.float64)[None, :] / N)


def weights(R, tau_row, loading):
    """R [1025, C, C] complex (Hermitian) -> w [1025, C] complex128, solved in float64"""
    R = np.asarray(R, np.complex128)
    C = R.shape[1]
    d = steering(tau_row)
    trace = np.einsum("kcc->k", R).real
    ok = trace > 0
    lam = loading * np.where(ok, trace, 0.0) / C
    A = np.where(ok[:, None, None], R + lam[:, None, None] * np.eye(C), np.eye(C))
    v = np.linalg.solve(A, d[:, :, None])[:, :, 0]
    w = v / np.einsum("kc,kc->k", d.conj(), v)[:, None]
    return np.where(ok[:, None], w, d / C)


def frames(seg, f32=False):
    """seg [len, C]: the event's own samples -> X [J + 1, C, 1025]: the spectra of its frames (zero outside the event)"""
    length, C = seg.shape
    J = -(-length // B)
    pad = np.zeros(((J + 2) * B, C), np.float32 if f32 else np.float64)
    pad[B:B + length] = seg
    fr = np.stack([pad[j * B: j * B + N] for j in range(J + 1)])            # [J + 1, N, C]; frame j starts at sample (j - 1) B
    fr = fr * window(f32)[None, :, None]
    if f32:
        import torch
        return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr.transpose(0, 2, 1))), dim=-1).numpy()
    return np.fft.rfft(fr.transpose(0, 2, 1), axis=-1)


def covariance(X):
    """X [J + 1, C, 1025] -> R [1025, C, C] in X's precision, frame after frame"""
    R = np.zeros((X.shape[2], X.shape[1], X.shape[1]), X.dtype)
    for j in range(X.shape[0]):
        R = R + np.einsum("ck,dk->kcd", X[j], X[j].conj()).astype(X.dtype)
    return R


def apply(X, w, length, f32=False):
    """the frames X combined with w [1025, C], transformed back and overlap-added -> y [length]"""
    cplx, real = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    wc = w.astype(cplx).conj()
    Y = np.zeros((X.shape[0], X.shape[2]), cplx)
    for c in range(X.shape[1]):
        Y = Y + (wc[None, :, c] * X[:, c, :]).astype(cplx)
    Y[:, 0] = Y[:, 0].real
    Y[:, B] = Y[:, B].real
    if f32:
        import torch
        v = torch.fft.irfft(torch.from_numpy(Y), n=N, dim=-1).numpy()
    else:
        v = np.fft.irfft(Y, n=N, axis=-1)
    v = (v * window(f32)[None, :]).astype(real)
    J = X.shape[0] - 1
    return (v[:J, B:] + v[1:, :B]).reshape(-1)[:length]


def event(x, s0, length, tau_row, loading, f32=False, through=()):
    """x [n, C], the event's samples [s0, s0 + length) -> (y [length], [the signals of ``through`` — each [n, C] — under the same weights])"""
    seg = np.asarray(x)[s0:s0 + length]
    X = frames(seg.astype(np.float32) if f32 else seg.astype(np.float64), f32)
    w = weights(covariance(X), tau_row, loading)
    rest = [apply(frames(np.asarray(t)[s0:s0 + length].astype(np.float32 if f32 else np.float64), f32), w, length, f32) for t in through]
    return apply(X, w, length, f32), rest


def beamform(x, events, dirs, loc_frames, time_factor, hop, max_frames, tau, loading, f32=False):
    """-> dict(audio [total], audio_start [E], audio_len [E]) of ONE recording x [n, C]; tau float64 [D, C]"""
    s0, lens, starts = beam_ref.spans(events, dirs, loc_frames, time_factor, x.shape[0], hop, max_frames)
    parts = [event(x, int(s0[e]), int(lens[e]), tau[dirs[e]], loading, f32)[0] for e in range(len(events)) if lens[e] > 0]
    audio = np.concatenate(parts) if parts else np.zeros(0, np.float32 if f32 else np.float64)
    return dict(audio=audio, audio_start=starts, audio_len=lens.astype(np.int32), s0=s0)


# ───────────── the two-source scene ─────────────
TARGET, INTERFERER = (2.2, 0.4), (-0.7, -0.2)


def scene(n, positions, sr, seed=11, band=0.8, interferer_db=10.0, noise_db=-30.0):
    """-> (target, interferer, noise), each [n, C] float32, the mix is their sum: a source at (az 2.2, el 0.4) band-limited to
    ``band`` x Nyquist, a second far-field source at (az -0.7, el -0.2) ``interferer_db`` stronger, and independent sensor noise
    ``noise_db`` relative to the target"""
    import doa_ref
    xs, _ = beam_ref.source(n, positions, doa_ref.unit(*TARGET), sr, seed, band=band)
    xi, _ = beam_ref.source(n, positions, doa_ref.unit(*INTERFERER), sr, seed + 1, band=band)
    xi = (xi * np.float32(10.0 ** (interferer_db / 20.0))).astype(np.float32)
    rms = math.sqrt(float(np.mean(xs.astype(np.float64) ** 2)))
    xn = (rms * 10.0 ** (noise_db / 20.0) * np.random.default_rng(seed + 2).standard_normal(xs.shape)).astype(np.float32)
    return xs, xi, xn


def db(num, den):
    return 10.0 * math.log10(float(np.mean(np.asarray(num, np.float64) ** 2)) / float(np.mean(np.asarray(den, np.float64) ** 2)))
