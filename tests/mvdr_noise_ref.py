"""The MVDR beam with its covariance taken from before the onset, restated in numpy float64.  TEST INFRASTRUCTURE.

Everything is tests/mvdr_ref.py's — the events, their samples [s0, s1), audio_len / audio_start, the grid N = 2048,
B = 1024, the window, the steering vector, the weights' formula and the apply step — except WHICH frames make the covariance,
with the settings Kn = noise_blocks >= 1 and G = noise_guard >= 0:

    an extracted event uses the noise covariance  iff  s0 >= (G + Kn + 1) B                  (all or nothing)
    noise frame q = 0..Kn-1 holds x_c[s0 - (G + Kn + 1 - q) B + m], m = 0..2047, read from the RECORDING (they lie before the
    event: the "outside [s0, s1) reads as 0" rule is not theirs); together they cover [s0 - (G + Kn + 1) B, s0 - G B)
    Rn[k] = sum_q X_q[k] X_q[k]^H        ascending q; chunks of 32 frames, added in ascending chunk order
    w[k]  = mvdr_ref.weights(Rn, tau, loading)[k]      (lambda = loading trace(Rn) / C; trace not > 0: d / C)

and every other event (s0 < (G + Kn + 1) B, or Kn = 0) is mvdr_ref.event's, exactly.  ``f32=True`` is the yardstick, as in
mvdr_ref: the window rounded once, the transforms and Rn in float32 / complex64, the solve in float64.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import mvdr_ref  # noqa: E402

N, B = mvdr_ref.N, mvdr_ref.B
CHUNK = 32


def uses_noise(s0, noise_blocks, noise_guard):
    return noise_blocks >= 1 and s0 >= (noise_guard + noise_blocks + 1) * B


def noise_spectra(x, s0, noise_blocks, noise_guard, f32=False):
    """x [n, C], the recording -> X [Kn, C, 1025]: the spectra of the Kn windowed frames that end G blocks before s0"""
    first = s0 - (noise_guard + noise_blocks + 1) * B
    assert first >= 0 and first + (noise_blocks + 1) * B == s0 - noise_guard * B <= x.shape[0]      # the last frame ends at s0 - G B
    real = np.float32 if f32 else np.float64
    fr = np.stack([np.asarray(x)[first + q * B: first + q * B + N].astype(real) for q in range(noise_blocks)])      # [Kn, N, C]
    fr = fr * mvdr_ref.window(f32)[None, :, None]
    if f32:
        import torch
        return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr.transpose(0, 2, 1))), dim=-1).numpy()
    return np.fft.rfft(fr.transpose(0, 2, 1), axis=-1)


def covariance(X):
    """X [Kn, C, 1025] -> Rn [1025, C, C] in X's precision: every chunk of 32 frames frame after frame, the chunks in order"""
    R = None
    for c0 in range(0, X.shape[0], CHUNK):
        part = mvdr_ref.covariance(X[c0:c0 + CHUNK])
        R = part if R is None else (R + part).astype(X.dtype)
    return R


def event(x, s0, length, tau_row, loading, noise_blocks, noise_guard, f32=False, through=()):
    """x [n, C], the event's samples [s0, s0 + length) -> (y [length], [the signals of ``through`` under the same weights],
    noise_frames: Kn where the weights came from the noise covariance, 0 where the event fell back to mvdr_ref.event)"""
    if not uses_noise(s0, noise_blocks, noise_guard):
        return mvdr_ref.event(x, s0, length, tau_row, loading, f32, through) + (0,)
    real = np.float32 if f32 else np.float64
    w = mvdr_ref.weights(covariance(noise_spectra(x, s0, noise_blocks, noise_guard, f32)), tau_row, loading)
    out = [mvdr_ref.apply(mvdr_ref.frames(np.asarray(t)[s0:s0 + length].astype(real), f32), w, length, f32) for t in (x,) + tuple(through)]
    return out[0], out[1:], noise_blocks


def beamform(x, events, dirs, loc_frames, time_factor, hop, max_frames, tau, loading, noise_blocks, noise_guard, f32=False):
    """mvdr_ref.beamform with the noise covariance -> its dict and ``noise_frames`` int32 [E]"""
    s0, lens, starts = beam_ref.spans(events, dirs, loc_frames, time_factor, x.shape[0], hop, max_frames)
    parts, used = [], np.zeros(len(events), np.int32)
    for e in range(len(events)):
        if lens[e] > 0:
            y, _, used[e] = event(x, int(s0[e]), int(lens[e]), tau[dirs[e]], loading, noise_blocks, noise_guard, f32)
            parts.append(y)
    audio = np.concatenate(parts) if parts else np.zeros(0, np.float32 if f32 else np.float64)
    return dict(audio=audio, audio_start=starts, audio_len=lens.astype(np.int32), s0=s0, noise_frames=used)


# ───────────── the scene of DESIGN 5u: self-cancellation under a steering error ─────────────
SR = 44100
SCENE_BLOCKS, EVENT = 40, (20, 32)                  # a recording of 40 blocks, the target sounds in blocks [20, 32) only


def onset_scene(spacing):
    """-> (positions, target, interferer, noise): mvdr_ref.scene on a tetrahedron of ``spacing`` metres at 44.1 kHz with the
    target zeroed outside the event — before the onset there are the interferer and the sensor noise alone"""
    import doa_ref
    pos = doa_ref.tetrahedron(spacing)
    xs, xi, xn = mvdr_ref.scene(SCENE_BLOCKS * B, pos, SR)
    xs = xs.copy()
    xs[:EVENT[0] * B] = 0.0
    xs[EVENT[1] * B:] = 0.0
    return pos, xs, xi, xn


def steered(positions, azimuth_error=0.0):
    """tau [C] towards the target with ``azimuth_error`` radians added to its azimuth"""
    import doa_ref
    az, el = mvdr_ref.TARGET
    tau, _ = beam_ref.delays(positions, doa_ref.unit(az + azimuth_error, el)[None, :], SR, 1)
    return tau[0]


def measure(spacing, azimuth_error, noise_blocks=8, noise_guard=1, loading=1e-2, blocks=EVENT[1] - EVENT[0]):
    """-> {"own" | "pre": (target level out / in, dB; output SIR, dB)} of the event's first ``blocks`` blocks"""
    pos, xs, xi, xn = onset_scene(spacing)
    tau = steered(pos, azimuth_error)
    s0, length = EVENT[0] * B, blocks * B
    out = {}
    for name, kn in (("own", 0), ("pre", noise_blocks)):
        _, (ys, yi, yn), used = event(xs + xi + xn, s0, length, tau, loading, kn, noise_guard, through=(xs, xi, xn))
        assert used == kn
        out[name] = (mvdr_ref.db(ys, xs[s0:s0 + length, 0]), mvdr_ref.db(ys, yi))
    return out
