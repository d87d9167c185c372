"""The MVDR beam with its noise frames picked where the event's class is silent, restated in numpy.  TEST INFRASTRUCTURE.

Everything is tests/mvdr_noise_ref.py's — the events, their samples [s0, s1), the grid, the window, the chunked
covariance, the weights' formula and the apply step — except WHICH frames make the noise covariance.  B = 1024, H = tf hop,
Kn = noise_blocks >= 1, G = noise_guard, S = noise_search, M = noise_min; all of the rule is integer:

    mask[t], t < L = n // H + 1: bit k is set when some row of the recording's table — located or not — has cls = k and
        onset <= t < offset, both clamped to [0, L]; a row with cls outside [0, n_classes) or onset < 0 marks nothing
    candidate q = 0..S-1 of an extracted event at s0: the 2048 samples from a_q = s0 - (G + 2 + q) B; it exists when a_q >= 0 and is
        eligible when mask[t] & excl == 0 for all t = max(lo, 0) // H .. ceil(hi / H) - 1, [lo, hi) = [s0 - (2 G + 2 + q) B, s0 - q B);
        excl = 1 << cls ("same") or every bit ("any")
    the first Kn eligible candidates in ascending q are selected, n_e of them; the noise covariance is used when the event is
        extracted, 0 <= cls < n_classes and n_e >= M: Rn = sum X X^H over them in ascending time (descending q), chunks of 32
    every other extracted event is mvdr_ref.event's, exactly.

``f32=True`` is the yardstick, as in mvdr_ref.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_ref  # noqa: E402

N, B = mvdr_ref.N, mvdr_ref.B


def activity(rows, cls, n, H, n_classes):
    """rows [(onset, offset, ...)] and cls of ONE recording of n samples -> mask uint32 [n // H + 1]"""
    assert 1 <= n_classes <= 32
    L = n // H + 1
    mask = np.zeros(L, np.uint32)
    for r, k in zip(rows, cls):
        on, off = int(r[0]), int(r[1])
        if on < 0 or not 0 <= k < n_classes:
            continue
        mask[min(on, L):min(max(off, 0), L)] |= np.uint32(1 << k)
    return mask


def eligible(mask, s0, k, H, G, S, exclude="same"):
    """-> the eligible candidates q of an event of class k at s0, ascending"""
    excl = 0xFFFFFFFF if exclude == "any" else 1 << k
    out = []
    for q in range(S):
        if s0 - (G + 2 + q) * B < 0:
            break
        lo, hi = max(s0 - (2 * G + 2 + q) * B, 0), s0 - q * B
        if not any(int(mask[t]) & excl for t in range(lo // H, -(-hi // H))):
            out.append(q)
    return out


def select(mask, s0, k, H, Kn, G, S, M, exclude="same", n_classes=32):
    """-> (n_e, sel [Kn]): the frames used (0: the own frames) and their q in summation order, -1 behind them"""
    sel = np.full(Kn, -1, np.int32)
    if not 0 <= k < n_classes:
        return 0, sel
    qs = eligible(mask, s0, k, H, G, S, exclude)[:Kn]
    if len(qs) < M:
        return 0, sel
    sel[:len(qs)] = qs[::-1]
    return len(qs), sel


def spectra(x, s0, G, qs, f32=False):
    """x [n, C], the recording -> X [len(qs), C, 1025]: the spectra of the windowed frames of 2048 samples from s0 - (G + 2 + q) B,
    q in qs in that order; a sample outside the recording reads as 0 (the rule selects no such frame)"""
    real = np.float32 if f32 else np.float64
    n = x.shape[0]
    fr = []
    for q in qs:
        a = s0 - (G + 2 + int(q)) * B
        f = np.zeros((N, x.shape[1]), real)
        lo, hi = max(a, 0), min(a + N, n)
        if hi > lo:
            f[lo - a:hi - a] = np.asarray(x)[lo:hi]
        fr.append(f)
    fr = np.stack(fr) * mvdr_ref.window(f32)[None, :, None]
    if f32:
        import torch
        return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(fr.transpose(0, 2, 1))), dim=-1).numpy()
    return np.fft.rfft(fr.transpose(0, 2, 1), axis=-1)


def covariance(x, s0, G, qs, f32=False):
    """Rn [1025, C, C] over the frames qs, in that order: mvdr_noise_ref.covariance's chunks of 32"""
    return mvdr_noise_ref.covariance(spectra(x, s0, G, qs, f32))


def event(x, s0, length, tau_row, loading, G, qs, f32=False, through=()):
    """x [n, C], the event's samples [s0, s0 + length), the selected candidates qs in summation order (none: the own frames) ->
    (y [length], [the signals of ``through`` under the same weights])"""
    if len(qs) == 0:
        return mvdr_ref.event(x, s0, length, tau_row, loading, f32, through)
    real = np.float32 if f32 else np.float64
    w = mvdr_ref.weights(covariance(x, s0, G, qs, f32), tau_row, loading)
    out = [mvdr_ref.apply(mvdr_ref.frames(np.asarray(t)[s0:s0 + length].astype(real), f32), w, length, f32) for t in (x,) + tuple(through)]
    return out[0], out[1:]


def frames_of(rows, cls, dirs, loc_frames, time_factor, n, hop, max_frames, Kn, G, S, M, exclude, n_classes):
    """the selection of every event of ONE recording of n samples -> dict(s0, audio_len, audio_start, noise_frames [E], noise_sel [E, Kn])"""
    s0, lens, starts = beam_ref.spans(rows, dirs, loc_frames, time_factor, n, hop, max_frames)
    mask = activity(rows, cls, n, time_factor * hop, n_classes)
    used, sel = np.zeros(len(rows), np.int32), np.full((len(rows), Kn), -1, np.int32)
    for e in range(len(rows)):
        if lens[e] > 0:
            used[e], sel[e] = select(mask, int(s0[e]), int(cls[e]), time_factor * hop, Kn, G, S, M, exclude, n_classes)
    return dict(s0=s0, audio_len=lens.astype(np.int32), audio_start=starts, noise_frames=used, noise_sel=sel)


def beamform(x, rows, cls, dirs, loc_frames, time_factor, hop, max_frames, tau, loading, Kn, G, S, M, exclude, n_classes, f32=False):
    """frames_of and the audio of ONE recording x [n, C]; tau float64 [D, C]"""
    out = frames_of(rows, cls, dirs, loc_frames, time_factor, x.shape[0], hop, max_frames, Kn, G, S, M, exclude, n_classes)
    parts = []
    for e in range(len(rows)):
        if out["audio_len"][e] > 0:
            qs = out["noise_sel"][e][:out["noise_frames"][e]]
            parts.append(event(x, int(out["s0"][e]), int(out["audio_len"][e]), tau[dirs[e]], loading, G, qs, f32)[0])
    out["audio"] = np.concatenate(parts) if parts else np.zeros(0, np.float32 if f32 else np.float64)
    return out


# ───────────── the scene of DESIGN 5w: a source that sounds twice ─────────────
SR = mvdr_noise_ref.SR
SCENE_BLOCKS, BURSTS, EVENT = 48, ((8, 16), (24, 40)), (24, 16)     # the target sounds in two bursts; the event is the second, 16 blocks
TF, HOP = 8, 1024                                                    # an output frame is 8 blocks: the bursts are frames [1, 2) and [3, 5)
ROWS, CLS = [(1, 2, 1), (3, 5, 3)], [0, 0]


def twice_scene(spacing):
    """-> (positions, target, interferer, noise): mvdr_ref.scene on a tetrahedron of ``spacing`` metres at 44.1 kHz with the target
    zeroed outside its two bursts"""
    import doa_ref
    pos = doa_ref.tetrahedron(spacing)
    xs, xi, xn = mvdr_ref.scene(SCENE_BLOCKS * B, pos, SR)
    keep = np.zeros(SCENE_BLOCKS * B, bool)
    for a, b in BURSTS:
        keep[a * B:b * B] = True
    xs = xs.copy()
    xs[~keep] = 0.0
    return pos, xs, xi, xn


def scene_selection(Kn=8, G=1, S=32, M=1, exclude="same", rows=ROWS, cls=CLS):
    """-> (eligible q, selected q in summation order) of the second burst under the class tracks ROWS"""
    mask = activity(rows, cls, SCENE_BLOCKS * B, TF * HOP, 2)
    s0 = EVENT[0] * B
    n_e, sel = select(mask, s0, 0, TF * HOP, Kn, G, S, M, exclude, 2)
    return eligible(mask, s0, 0, TF * HOP, G, S, exclude), sel[:n_e].tolist()


def measure(spacing, azimuth_error, Kn=8, G=1, loading=1e-2, f32=False):
    """-> {"fixed" | "quiet" | "own": (target level out / in, dB; output SIR, dB)} of the second burst"""
    pos, xs, xi, xn = twice_scene(spacing)
    tau = mvdr_noise_ref.steered(pos, azimuth_error)
    s0, length = EVENT[0] * B, EVENT[1] * B
    mix = xs + xi + xn
    qs = {"fixed": list(range(Kn - 1, -1, -1)), "quiet": scene_selection(Kn, G)[1], "own": []}
    out = {}
    for name, q in qs.items():
        _, (ys, yi, yn) = event(mix, s0, length, tau, loading, G, q, f32, through=(xs, xi, xn))
        out[name] = (mvdr_ref.db(ys, xs[s0:s0 + length, 0]), mvdr_ref.db(ys, yi))
    return out
