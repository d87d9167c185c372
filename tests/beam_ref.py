"""Per-event audio by a steered delay-and-sum beam, restated in numpy float64.  TEST INFRASTRUCTURE.

Settings: Q = oversample, H = half_width, beta.  The filter ``taps`` float32 [Q, 2H] is resample.design_taps(Q, H, 1.0, beta) in
float64 — h[p][k] = sinc(t) I0(beta sqrt(1 - (t/H)^2)) / I0(beta), t = p/Q - (k - H + 1) — with row 0 replaced by the unit impulse
(1 at column H - 1), every other row divided by its float64 sum, rounded once to float32; row p evaluates a channel at m + p/Q:

    x(m + p/Q) = sum_{k=0}^{2H-1} taps[p][k] x[m + k - H + 1]

Delays: microphones r_c with centroid rbar, grid direction u_d: tau[d][c] = sr (r_c - rbar) . u_d / c_sound — channel c hears
s[n + tau] — and M[d][c] = round_half_even(tau[d][c] Q).

An event is extracted iff dir >= 0; it was located on the frames [f0, f0 + loc_frames) (f0 from localize.event_frames with
n_feat = 1 + n // hop); its samples are [s0, s1) = [f0 hop, min((f0 + loc_frames) hop, n)), audio_len = max(0, s1 - s0) and
audio_start the exclusive prefix sum of audio_len in event order.  Output sample i (n = s0 + i):

    q_c = -M[dir][c];  i_c = floor(q_c / Q);  p_c = q_c - Q i_c
    a_c = sum_k taps[p_c][k] x_c[n + i_c + k - H + 1]          (k ascending)
    y   = (((0 + a_0) + a_1) + ... + a_{C-1}) * float32(1 / C)

with samples outside [0, n_r) read as 0.  ``beamform`` evaluates this in float64 — with the float32 taps and the integer M, as the
kernel has them — or, with ``f32=True``, in float32 in the same order (products and sums rounded one by one): the yardstick.
``source`` makes the test signals: doa_ref.far_field's phase ramps about the centroid, with an optional band limit.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402,F401
from sed_crnn_amd.localize import event_frames  # noqa: E402
from sed_crnn_amd.resample import design_taps  # noqa: E402

C_SOUND = doa_ref.C_SOUND


def taps(Q, H, beta):
    """-> (float32 [Q, 2H], the float64 table before rounding)"""
    t = design_taps(Q, H, 1.0, beta).astype(np.float64)
    t[0, :] = 0.0
    t[0, H - 1] = 1.0
    for p in range(1, Q):
        t[p] = t[p] / t[p].sum()
    return t.astype(np.float32), t


def delays(positions, units, sr, Q, c=C_SOUND):
    """-> (tau float64 [D, C], M int64 [D, C])"""
    r, u = np.asarray(positions, np.float64), np.asarray(units, np.float64).reshape(-1, 3)
    tau = sr * ((r - r.mean(0)) @ u.T).T / c
    return tau, np.rint(tau * Q).astype(np.int64)


def spans(events, dirs, loc_frames, time_factor, n, hop, max_frames):
    """events [(onset, offset, peak_frame), ...] of ONE recording of n samples -> (s0 [E], audio_len [E], audio_start [E])"""
    s0s, lens = [], []
    for (on, off, pk), d, lf in zip(events, dirs, loc_frames):
        s0 = ln = 0
        if d >= 0:
            f0, _ = event_frames(on, off, pk, time_factor, 1 + n // hop, max_frames)
            s0 = f0 * hop
            ln = max(0, min((f0 + int(lf)) * hop, n) - s0)
        s0s.append(s0)
        lens.append(ln)
    lens = np.asarray(lens, np.int64)
    return np.asarray(s0s, np.int64), lens, np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)


def steer(x, s0, length, m_row, tap32, Q, f32=False):
    """x [n, C] float32, the event's samples [s0, s0 + length), m_row = M[dir] -> y [length]"""
    real = np.float32 if f32 else np.float64
    n, C = x.shape
    H = tap32.shape[1] // 2
    y = np.zeros(length, real)
    for c in range(C):
        q = -int(m_row[c])
        ic = q // Q                                                       # python's // is the floor
        row = tap32[q - Q * ic].astype(real)
        first = s0 + ic - H + 1                                           # x_c[first + j + k] is what output j needs at tap k
        idx = first + np.arange(length + 2 * H - 1)
        ok = (idx >= 0) & (idx < n)
        seg = np.where(ok, x[np.clip(idx, 0, n - 1), c], np.float32(0)).astype(real)
        a = np.zeros(length, real)
        for k in range(2 * H):
            a = a + row[k] * seg[k:k + length]
        y = y + a
    return y * real(np.float32(1.0 / C))


def beamform(x, events, dirs, loc_frames, time_factor, hop, max_frames, M, tap32, Q, f32=False):
    """-> dict(audio [total], audio_start [E], audio_len [E]) of ONE recording x [n, C]"""
    s0, lens, starts = spans(events, dirs, loc_frames, time_factor, x.shape[0], hop, max_frames)
    parts = [steer(x, int(s0[e]), int(lens[e]), M[dirs[e]], tap32, Q, f32) for e in range(len(events)) if lens[e] > 0]
    audio = np.concatenate(parts) if parts else np.zeros(0, np.float32 if f32 else np.float64)
    return dict(audio=audio, audio_start=starts, audio_len=lens.astype(np.int32), s0=s0)


def source(n, positions, u, sr, seed, band=None, noise=0.0, c=C_SOUND):
    """-> (x [n, C] float32, s [n] float64): a white source, band-limited to ``band`` x Nyquist when given, from the far-field
    direction ``u``, as every microphone hears it — channel c is s[n + tau_c], tau_c = sr (r_c - rbar) . u / c, a phase ramp in a
    float64 FFT that is zero-padded so that nothing wraps (doa_ref.far_field's method, about the centroid) — plus ``noise`` x
    independent white noise per channel; s is the source at the centroid in the scale of x (x = s + noise where every tau is 0)"""
    rng = np.random.default_rng(seed)
    r = np.asarray(positions, np.float64)
    tau = sr * ((r - r.mean(0)) @ np.asarray(u, np.float64)) / c
    guard = int(math.ceil(np.abs(tau).max())) + 8
    m = n + 2 * guard
    X = np.fft.rfft(rng.standard_normal(m))
    f = np.arange(X.size) / m
    if band is not None:
        X[f > 0.5 * band] = 0.0
    s = np.fft.irfft(X, n=m)[guard: guard + n]
    x = np.stack([np.fft.irfft(X * np.exp(2j * np.pi * f * t), n=m)[guard: guard + n] + noise * rng.standard_normal(n) for t in tau], 1)
    return (0.3 * x).astype(np.float32), 0.3 * s


def line_along(u, offsets_m):
    """microphones on the line through the origin along the unit vector ``u``, at the given distances in metres"""
    return np.asarray(offsets_m, np.float64)[:, None] * np.asarray(u, np.float64)[None, :]


# ───────────── the edge rows of both test files: a recording of 40 hops (41 feature frames), max_frames = 12, time_factor = 1 ─────────────
EDGE_FRAMES, EDGE_MAX_FRAMES = 40, 12
# (onset, offset, peak_frame), recording, located?
EDGE_ROWS = [((3, 4, 3), 0, True),          # one frame
             ((10, 15, 12), 0, True),       # 5 frames: crosses a tile of any size up to 4096 samples
             ((2, 35, 20), 0, True),        # 33 frames, more than max_frames: the 12 around the peak, [14, 26)
             ((0, 3, 1), 0, True),          # at frame 0: the filter reads before sample 0
             ((38, 41, 39), 0, True),       # ends on the last frame: clipped at n, the filter reads beyond it
             ((50, 60, 55), 0, False),      # beyond the recording
             ((5, 12, 8), 7, False),        # names a recording that does not exist
             ((22, 23, 22), 0, False),      # digital silence: located on one frame, no direction
             ((5, 12, 8), 0, True), ((30, 50, 31), 0, True), ((0, 1, 0), 0, True), ((40, 41, 40), 0, True), ((8, 40, 39), 0, True)]
