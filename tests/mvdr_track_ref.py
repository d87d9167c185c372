"""The MVDR beam steered along the event's direction track, restated in numpy float64.  TEST INFRASTRUCTURE.

Everything is tests/mvdr_ref.py's, mvdr_noise_ref.py's (5u) and mvdr_quiet_ref.py's (5w) — the events, their samples
[s0, s1), the grid N = 2048, B = 1024, the window, WHICH frames make the covariance, the weights' formula, the inverse transform and
the overlap-add — except WHERE the weights of frame j are steered.  THE RULE (integer), with len = s1 - s0, J = ceil(len / B), the
frames j = 0..J, T = trk_len clamped to [0, Tm], W = block_chunks, hop the hop of the located frames:

    b_j = min((j B // hop) // (32 W), T - 1)
    d_j = trk_dir[b_j]  where T > 0 and 0 <= trk_dir[b_j] < D,   else dir
    w_b = mvdr_ref.weights(R, tau[d_b], loading)   for every block b < max(T, 1): ONE covariance R (or Rn) an event
    Y_j = sum_c conj(w_{b_j,c}) X_{c,j}            ascending c

(the centre of frame j is sample j B of the event, which lies in located frame j B // hop; frame J and the short tail that
localize.track_blocks joins to the last block take block T - 1).  A silent block (-1), a row outside [0, D) and an event without
a track keep ``dir``.  ``f32=True`` is the yardstick, as in mvdr_ref.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402
import mvdr_ref  # noqa: E402

N, B = mvdr_ref.N, mvdr_ref.B
CHUNK = 32


def frame_blocks(length, hop, W, T):
    """THE RULE, a loop: -> [J + 1] the track block of every frame (T = 0: block 0, the weights steered at ``dir``)"""
    J = -(-length // B)
    out = []
    for j in range(J + 1):
        located = (j * B) // hop
        out.append(max(min(located // (CHUNK * W), T - 1), 0))
    return out


def block_dirs(dirs_per_block, fallback_dir, D):
    """-> the direction of every block b < max(T, 1); ``dirs_per_block``: the T rows of trk_dir that are read"""
    T = len(dirs_per_block)
    if T == 0:
        return [int(fallback_dir)]
    return [int(d) if 0 <= int(d) < D else int(fallback_dir) for d in dirs_per_block]


def apply(X, w_frames, length, f32=False):
    """mvdr_ref.apply with a weight set per frame: X [J + 1, C, 1025], w_frames [J + 1, 1025, C] -> y [length]"""
    cplx, real = (np.complex64, np.float32) if f32 else (np.complex128, np.float64)
    wc = w_frames.astype(cplx).conj()
    Y = np.zeros((X.shape[0], X.shape[2]), cplx)
    for c in range(X.shape[1]):
        Y = Y + (wc[:, :, c] * X[:, c, :]).astype(cplx)
    Y[:, 0] = Y[:, 0].real
    Y[:, B] = Y[:, B].real
    if f32:
        import torch
        v = torch.fft.irfft(torch.from_numpy(Y), n=N, dim=-1).numpy()
    else:
        v = np.fft.irfft(Y, n=N, axis=-1)
    v = (v * mvdr_ref.window(f32)[None, :]).astype(real)
    J = X.shape[0] - 1
    return (v[:J, B:] + v[1:, :B]).reshape(-1)[:length]


def event(x, s0, length, tau, dirs_per_block, fallback_dir, W, hop, loading, noise_blocks=0, noise_guard=1, qs=None, f32=False,
          through=()):
    """x [n, C], the event's samples [s0, s0 + length), tau float64 [D, C], ``dirs_per_block`` the event's trk_dir[:T] (T already
    clamped to Tm), ``fallback_dir`` its dir.  The covariance: the own frames; with ``noise_blocks`` >= 1 mvdr_noise_ref's (where
    its rule allows it); with ``qs`` — a non-empty list of candidates in summation order — mvdr_quiet_ref's.
    -> (y [length], [the signals of ``through`` — each [n, C] — under the same weights])"""
    real = np.float32 if f32 else np.float64
    tau = np.asarray(tau, np.float64)
    X = mvdr_ref.frames(np.asarray(x)[s0:s0 + length].astype(real), f32)
    if qs is not None and len(qs):
        R = mvdr_quiet_ref.covariance(x, s0, noise_guard, qs, f32)
    elif qs is None and mvdr_noise_ref.uses_noise(s0, noise_blocks, noise_guard):
        R = mvdr_noise_ref.covariance(mvdr_noise_ref.noise_spectra(x, s0, noise_blocks, noise_guard, f32))
    else:
        R = mvdr_ref.covariance(X)
    dirs = block_dirs(dirs_per_block, fallback_dir, tau.shape[0])
    made = {d: mvdr_ref.weights(R, tau[d], loading) for d in sorted(set(dirs))}
    b = frame_blocks(length, hop, W, len(dirs_per_block))
    w = np.stack([made[dirs[bj]] for bj in b])                                # [J + 1, 1025, C]
    rest = [apply(mvdr_ref.frames(np.asarray(t)[s0:s0 + length].astype(real), f32), w, length, f32) for t in through]
    return apply(X, w, length, f32), rest


def beamform(x, events, dirs, loc_frames, trk_len, trk_dir, W, time_factor, hop, max_frames, tau, loading, noise_blocks=0, noise_guard=1,
             quiet=None, f32=False):
    """-> dict(audio [total], audio_start [E], audio_len [E]) of ONE recording x [n, C]; trk_len [E], trk_dir [E, Tm]; ``quiet``: None
    or (noise_frames [E], noise_sel [E, Kn]) as mvdr_quiet_ref.frames_of returns them"""
    s0, lens, starts = beam_ref.spans(events, dirs, loc_frames, time_factor, x.shape[0], hop, max_frames)
    trk_dir = np.asarray(trk_dir).reshape(len(events), -1)
    parts = []
    for e in range(len(events)):
        if lens[e] > 0:
            T = min(max(int(trk_len[e]), 0), trk_dir.shape[1])
            qs = None if quiet is None else list(quiet[1][e][:quiet[0][e]])
            parts.append(event(x, int(s0[e]), int(lens[e]), tau, list(trk_dir[e][:T]), dirs[e], W, hop, loading, noise_blocks, noise_guard,
                               qs, f32)[0])
    audio = np.concatenate(parts) if parts else np.zeros(0, np.float32 if f32 else np.float64)
    return dict(audio=audio, audio_start=starts, audio_len=lens.astype(np.int32), s0=s0)


# ───────────── the scene of DESIGN 5y: a source that moves while it sounds ─────────────
SR, HOP = 44100, 1024
LEAD, BLOCKS, BLOCK_FRAMES = 16, 8, 32              # 16 blocks of 1024 samples of lead-in, then 8 track blocks of 32 frames
AZ0, AZ_STEP = 20.0, 10.0                           # block b: azimuth 20 + 10 b degrees, elevation 0
ONE_DIR_AZ = 30.0                                   # "one dir": what DESIGN 5x's scene gives for the whole event


def azimuth(b, step=AZ_STEP):
    return math.radians(AZ0 + step * b)


def moving_scene(spacing, step=AZ_STEP):
    """-> (positions, target [n, C], interferer, noise, centroid [n]): in block b a far-field source at azimuth 20 + ``step`` b
    degrees (beam_ref.source, seed 700 + b, band 0.8), silent during the lead-in; a static second source over the whole recording
    at mvdr_ref.INTERFERER (seed 12), 10 dB stronger; sensor noise at -30 dB of the target (default_rng(13)).  ``centroid`` is the
    target's waveform at the centroid of the array, the level reference"""
    import doa_ref
    pos = doa_ref.tetrahedron(spacing)
    n, m = (LEAD + BLOCKS * BLOCK_FRAMES) * B, BLOCK_FRAMES * B
    xs, s = np.zeros((n, 4), np.float32), np.zeros(n)
    for b in range(BLOCKS):
        xb, sb = beam_ref.source(m, pos, doa_ref.unit(azimuth(b, step)), SR, 700 + b, band=0.8)
        xs[LEAD * B + b * m: LEAD * B + (b + 1) * m] = xb
        s[LEAD * B + b * m: LEAD * B + (b + 1) * m] = sb
    xi, _ = beam_ref.source(n, pos, doa_ref.unit(*mvdr_ref.INTERFERER), SR, 12, band=0.8)
    xi = (xi * np.float32(10.0 ** (10.0 / 20.0))).astype(np.float32)
    rms = math.sqrt(float(np.mean(xs[LEAD * B:].astype(np.float64) ** 2)))
    xn = (rms * 10.0 ** (-30.0 / 20.0) * np.random.default_rng(13).standard_normal(xs.shape)).astype(np.float32)
    return pos, xs, xi, xn, s


def scene_tau(positions, step=AZ_STEP):
    """tau float64 [BLOCKS + 1, C]: rows 0..7 the true azimuth of every block, row 8 the one direction of 30 degrees"""
    import doa_ref
    units = np.stack([doa_ref.unit(azimuth(b, step)) for b in range(BLOCKS)] + [doa_ref.unit(math.radians(ONE_DIR_AZ))])
    return beam_ref.delays(positions, units, SR, 1)[0]


def measure(spacing, noise_blocks=0, noise_guard=1, loading=1e-2, step=AZ_STEP, f32=False):
    """-> {"one" | "tracked": dict(level, sir: whole event; level_last, sir_last: the last block; error: the target as the beam
    passes it against the source at the centroid, whole event)}, all in dB"""
    pos, xs, xi, xn, s = moving_scene(spacing, step)
    tau = scene_tau(pos, step)
    s0, length = LEAD * B, BLOCKS * BLOCK_FRAMES * B
    last = slice(length - BLOCK_FRAMES * B, length)
    ref = s[s0:s0 + length]
    out = {}
    for name, track in (("one", []), ("tracked", list(range(BLOCKS)))):
        y, (ys, yi, yn) = event(xs + xi + xn, s0, length, tau, track, BLOCKS, 1, HOP, loading, noise_blocks, noise_guard, f32=f32,
                                through=(xs, xi, xn))
        out[name] = dict(level=mvdr_ref.db(ys, ref), sir=mvdr_ref.db(ys, yi), level_last=mvdr_ref.db(ys[last], ref[last]),
                         sir_last=mvdr_ref.db(ys[last], yi[last]), error=mvdr_ref.db(ys - ref, ref))
    return out
