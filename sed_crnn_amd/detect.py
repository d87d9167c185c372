"""Whole-recording event detection: windowed eval forward -> one probability track -> (class, start s, end s, peak) events.

Frame arithmetic.  ``tf = model.time_factor`` (product of the time pools), ``L = seq_len`` (default
``data.SEQ_LEN_IN`` = 64, what the nets are trained on) and ``hop`` are in input (feature) frames; ``L % tf == 0`` and
``hop % tf == 0`` are required.  A recording of ``N`` feature frames has ``N_out = N // tf`` output frames (the ragged tail is
dropped, like the pooling does); output frame ``j`` covers input frames ``[tf*j, tf*(j+1))`` and lasts ``tf*hop_length/sr``
seconds (0.186 s at the reference settings).  Windows start at ``0, hop, 2*hop, ...`` while ``start + L <= N``, plus one window
at ``((N-L)//tf)*tf`` when the last regular one stops short, so every output frame is covered
(``((N-L)//tf)*tf + L == tf*N_out``).  ``N < L``: the recording runs as ONE sequence of ``tf*N_out`` frames (the net takes any
T); ``N < tf`` is refused.

The path on the GPU: ``feature.mbe`` (fused scaler) -> per chunk of at most ``max_batch`` windows, ``sed_window_batch``
(one gather into a max_batch-window buffer) and the model's eval forward on one workspace -> ``sed_detect_stitch`` (sigmoid, mean / max over the
covering windows) -> ``sed_detect_events`` (median filter, double threshold, gap merge, minimum length, peaks).  The host
reads one int — the event count — and nothing else.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import feature
from ._lib import SedHipError, TuneSetting, check, lib, ptr, stream_ptr
from .data import SEQ_LEN_IN
from .events import event_beamform, event_doa, event_mvdr, event_tdoa
from .model import HipCRNN

_EVENT_KEYS = ("cls", "onset", "offset", "peak", "peak_frame")
_TDOA_KEYS = ("lag", "strength", "loc_frames")          # added to the events of a localising detector
_DOA_KEYS = ("dir", "doa_power")                        # ... and, with localize=DOA(...), a direction per event
_TRACK_KEYS = ("trk_len", "trk_raw", "trk_dir", "trk_power")   # ... and, with DOA(..., track=DirectionTrack(...)), a direction per block (5x)
_BEAM_KEYS = ("audio_start", "audio_len")               # ... and, with extract=DelaySum(...), its place in result.audio
_NOISE_KEYS = ("noise_frames",)                         # ... and, with extract=MVDR(noise_blocks >= 1), the pre-onset frames its weights used (5u)
_QUIET_KEYS = ("noise_sel",)                            # ... and, with noise_select="quiet", which candidates they are (5w; offline only)
_CONTRAST_KEYS = ("bg_frames", "bg_sel")                # ... and, with DOA(..., contrast=Contrast(...)), the background frames of its map (5z)


def _doa_angles(events, grid, k):
    """[E_k, 3] host float64: azimuth, elevation (radians) and power of the events of class ``k`` (None: all); NaN rows where
    an event was not located (``dir`` = -1)"""
    d = events["dir"].cpu().numpy().astype(np.int64)
    out = np.full((d.shape[0], 3), np.nan)
    ok = d >= 0
    out[ok, 0], out[ok, 1] = grid.azimuth[d[ok]], grid.elevation[d[ok]]
    out[ok, 2] = events["doa_power"].cpu().numpy().astype(np.float64)[ok]
    return out if k is None else out[events["cls"].cpu().numpy() == int(k)]


def _doa_track(result, e):
    """[T_e, 4] host float64 of event ``e``: per block its centre time in seconds, the azimuth and elevation (radians) of the track
    and the block's power; NaN angles where a block is silent; no rows for an event that was not located"""
    from .localize import event_frames, track_blocks
    if "trk_len" not in result.events or result.grid is None or result.track is None:
        raise ValueError("this result holds no direction tracks: detect with EventDetector(..., localize=sed.DOA(..., "
                         "track=sed.DirectionTrack(...))) or pass it through det.localize(result, waveform, ...)")
    ev = result.events
    E = int(ev["trk_len"].numel())
    if not -E <= int(e) < E:
        raise IndexError(f"event {e} of {E}")
    e = int(e) % E
    trk, max_frames, tf, hop = result.track
    T = int(ev["trk_len"][e])
    out = np.full((T, 4), np.nan)
    if T == 0:
        return out
    # (a detector's events end within their recording: the frames of localize.event_frames do not depend on its length)
    f0, _ = event_frames(int(ev["onset"][e]), int(ev["offset"][e]), int(ev["peak_frame"][e]), tf, 0x7fffffff, max_frames)
    T_rule, first, n = track_blocks(int(ev["loc_frames"][e]), trk.block_chunks)
    assert T_rule == T
    out[:, 0] = (f0 + first + (n - 1) / 2.0) * hop / float(result.sr)
    d = ev["trk_dir"][e, :T].cpu().numpy().astype(np.int64)
    ok = d >= 0
    out[ok, 1], out[ok, 2] = result.grid.azimuth[d[ok]], result.grid.elevation[d[ok]]
    out[:, 3] = ev["trk_power"][e, :T].cpu().numpy().astype(np.float64)
    return out


def _is_per_class(v):
    """a decoder argument given per class: a list, a tuple, an ndarray or a tensor with at least one axis"""
    return isinstance(v, (list, tuple)) or (isinstance(v, (np.ndarray, torch.Tensor)) and v.ndim >= 1)


def _class_settings(K, threshold, low, median, min_gap, min_len):
    """The five decoder arguments, each a scalar or a length-K sequence -> (class-wise?, K dicts of scalars).  Scalars
    broadcast; ``low=None`` means low_k = threshold_k.  ValueError names the class and the argument."""
    given = dict(threshold=threshold, low=low, median=median, min_gap=min_gap, min_len=min_len)
    classwise = any(_is_per_class(v) for v in given.values())
    cols = {}
    for name, v in given.items():
        if _is_per_class(v):
            v = v.detach().cpu().tolist() if isinstance(v, torch.Tensor) else np.asarray(v).tolist()
            if len(v) != K or any(_is_per_class(x) for x in v):
                raise ValueError(f"{name} has {len(v)} entries, the net has {K} classes (give a scalar or one value per class, "
                                 f"as a list, tuple, ndarray or 1-D tensor)")
            cols[name] = v
        else:
            cols[name] = [v] * K
    rows = []
    for k in range(K):
        who = f"class {k}: " if classwise else ""
        hi = float(cols["threshold"][k])
        lo_k = cols["low"][k]
        lo = hi if lo_k is None else float(lo_k)
        if not lo <= hi:
            raise ValueError(f"{who}low={lo_k} must not exceed threshold={cols['threshold'][k]}")
        m, gap, ml = cols["median"][k], cols["min_gap"][k], cols["min_len"][k]
        for name, x in (("median", m), ("min_gap", gap), ("min_len", ml)):
            if classwise and int(x) != x:
                raise ValueError(f"{who}{name} must be an integer, got {x}")
        if not (1 <= int(m) <= 31 and int(m) % 2 == 1):
            raise ValueError(f"{who}median must be odd, 1..31, got {m}")
        if classwise and int(gap) < 0:
            raise ValueError(f"{who}min_gap must be >= 0, got {gap}")
        if classwise and int(ml) < 1:
            raise ValueError(f"{who}min_len must be >= 1, got {ml}")
        rows.append(dict(threshold=hi, low=lo, median=int(m), min_gap=int(gap), min_len=int(ml)))
    return classwise, rows


def _event_tensors(keys, cap, device):
    """event buffers for ``cap`` events: one device tensor per key (``peak`` float32, every other int32), rows of one allocation"""
    buf = torch.empty(len(keys), cap, dtype=torch.int32, device=device)
    return {k: buf[i].view(torch.float32) if k == "peak" else buf[i] for i, k in enumerate(keys)}


def _intervals(events, frame_seconds, k):
    """[(start_s, end_s, peak), ...] of class ``k`` among ``events``, on the host (seconds = frame * tf * hop_length / sr)"""
    ev = {n: events[n].cpu().numpy() for n in ("cls", "onset", "offset", "peak")}
    sel = ev["cls"] == int(k)
    fs = frame_seconds
    return [(int(a) * fs, int(b) * fs, float(p)) for a, b, p in zip(ev["onset"][sel], ev["offset"][sel], ev["peak"][sel])]


def _timed(marks, name, fn):
    """run ``fn``; with a list ``marks``, between two hip events that go to it as (name, start, end), for per-phase timing"""
    if marks is None:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    marks.append((name, a, b))
    return out


def _window_jobs(logits, groups, tf, K):
    """``_forward_windows`` jobs for ``groups`` = [(win_len, window starts), ...] (empty ones are skipped) whose logits fill the
    flat buffer ``logits`` back to back: the starts go to the device as int32, every group gets its [n, win_len // tf, K] view"""
    jobs, at = [], 0
    for Lw, starts in groups:
        n, wo = len(starts), Lw // tf
        if n == 0:
            continue
        st = torch.from_numpy(np.asarray(starts, dtype=np.int32)).to(logits.device, non_blocking=True)
        jobs.append((st, Lw, logits[at:at + n * wo * K].view(n, wo, K)))
        at += n * wo * K
    return jobs


@dataclass(frozen=True)
class WindowPlan:
    """The window grid of one recording (input frames unless named ``*_out``)."""
    n_frames: int          # N feature frames
    n_out: int             # N // tf output frames
    win_len: int           # input frames per window (L, or tf*n_out for a recording shorter than L)
    starts: tuple          # window starts (input frames)
    tf: int

    @property
    def n_win(self):
        return len(self.starts)

    @property
    def win_out(self):
        return self.win_len // self.tf

    @property
    def hop_out(self):
        return (self.starts[1] - self.starts[0]) // self.tf if self.n_win > 1 else self.win_out

    @property
    def last_start_out(self):
        return self.starts[-1] // self.tf


def plan_windows(n_frames, tf, seq_len=SEQ_LEN_IN, hop=None, trim=0):
    """The window grid of a recording of ``n_frames`` feature frames (module docstring); raises ValueError on a bad
    ``seq_len`` / ``hop`` / ``trim`` or a recording shorter than one output frame."""
    N, tf, L = int(n_frames), int(tf), int(seq_len)
    hop = L // 2 if hop is None else int(hop)
    if tf < 1 or L < tf or L % tf:
        raise ValueError(f"seq_len={L} must be a positive multiple of the time factor {tf}")
    if hop < tf or hop % tf or hop > L:
        raise ValueError(f"hop={hop} must be a positive multiple of the time factor {tf}, at most seq_len={L}")
    if int(trim) < 0:
        raise ValueError(f"trim must be >= 0, got {trim}")
    if N < tf:
        raise ValueError(f"a recording of {N} frames is shorter than one output frame ({tf} input frames)")
    n_out = N // tf
    if N < L:
        return WindowPlan(N, n_out, tf * n_out, (0,), tf)
    starts = list(range(0, N - L + 1, hop))
    last = ((N - L) // tf) * tf
    if starts[-1] != last:
        starts.append(last)
    plan = WindowPlan(N, n_out, L, tuple(starts), tf)
    if plan.n_win > 1 and plan.hop_out + 2 * int(trim) > plan.win_out:
        raise ValueError(f"trim={trim} leaves output frames uncovered: windows of {plan.win_out} output frames every "
                         f"{plan.hop_out} keep {plan.win_out - 2 * int(trim)} interior frames each")
    return plan


@dataclass(frozen=True)
class BatchPlan:
    """The windows of R recordings whose features are packed back to back (``plan_batch``).  Logits go to one flat buffer:
    first every window of ``seq_len`` frames in (recording, window) order, then the recordings shorter than ``seq_len``
    grouped by their window length (``groups``, in increasing length; a recording's windows are contiguous either way)."""
    plans: tuple           # WindowPlan of every recording
    row_off: tuple         # [R+1] first feature row of every recording in the packed features
    out_off: tuple         # [R+1] first output frame of every recording in the packed track
    full_starts: tuple     # absolute starts (packed rows) of every window of seq_len frames, (recording, window) order
    groups: tuple          # ((win_len, (absolute start, ...)), ...): one window per short recording, by window length
    logit_off: tuple       # [R] first logit (float index) of every recording in the flat buffer
    n_logits: int          # floats in the flat buffer

    def stitch_table(self):
        """[R][6] int64 {first logit, n_win, win_out, hop_out, last_start_out, n_out}: sed_detect_stitch_batch's table"""
        return np.array([[o, p.n_win, p.win_out, p.hop_out, p.last_start_out, p.n_out] for o, p in zip(self.logit_off, self.plans)],
                        dtype=np.int64).reshape(-1, 6)


def plan_batch(n_frames, tf, K, seq_len=SEQ_LEN_IN, hop=None, trim=0):
    """``plan_windows`` for every recording of a packed batch (``n_frames`` = feature frames per recording, ``K`` classes) ->
    BatchPlan.  ValueError names the first recording that cannot be planned (N < tf), before anything runs."""
    plans, row_off = [], [0]
    for i, N in enumerate(n_frames):
        try:
            plans.append(plan_windows(N, tf, seq_len, hop, trim))
        except ValueError as e:
            raise ValueError(f"recording {i}: {e}") from None
        row_off.append(row_off[-1] + int(N))
    if row_off[-1] >= 2 ** 31:
        raise ValueError(f"{row_off[-1]} feature frames in one batch: sed_window_batch takes int32 starts (at most 2^31 - 1)")
    out_off = [0]
    for p in plans:
        out_off.append(out_off[-1] + p.n_out)
    L = int(seq_len)
    full, logit_off, short = [], [None] * len(plans), {}
    for r, p in enumerate(plans):
        if p.win_len == L and p.n_frames >= L:
            logit_off[r] = len(full) * (L // tf) * K
            full.extend(row_off[r] + s for s in p.starts)
        else:
            short.setdefault(p.win_len, []).append(r)
    at = len(full) * (L // tf) * K
    groups = []
    for Lw in sorted(short):
        rs = short[Lw]
        for i, r in enumerate(rs):
            logit_off[r] = at + i * (Lw // tf) * K
        groups.append((Lw, tuple(row_off[r] for r in rs)))
        at += len(rs) * (Lw // tf) * K
    return BatchPlan(tuple(plans), tuple(row_off), tuple(out_off), tuple(full), tuple(groups), tuple(logit_off), at)


class DetectionResult:
    """``probs`` [n_out, K] device track; ``events`` dict of device tensors (``cls``, ``onset``, ``offset``, ``peak_frame``
    int32 output frames, offset exclusive; ``peak`` float32), sorted by (class, onset); ``frame_seconds`` = tf*hop_length/sr."""

    def __init__(self, probs, events, frame_seconds, plan, sr=None, grid=None, audio=None, track=None):
        self.probs, self.events, self.frame_seconds, self.plan = probs, events, frame_seconds, plan
        # (DirectionTrack, max_frames, time_factor, hop_length): set on results located with DOA(..., track=...) settings (5x)
        self.track = track
        self.sr = sr                            # the detector's rate: set on located results (lags are in samples at that rate)
        self.grid = grid                        # the DirectionGrid that ``dir`` indexes: set on results located with DOA settings
        # the packed beamformed audio that ``audio_start`` / ``audio_len`` index: set by a detector with extract=; a
        # ``res[i]`` view of a batch shares the batch's buffer
        self.audio = audio

    def __len__(self):
        return int(self.events["cls"].numel())

    def intervals(self, k=0):
        """[(start_s, end_s, peak), ...] of class ``k`` on the host (seconds = frame * tf * hop_length / sr)."""
        return _intervals(self.events, self.frame_seconds, k)

    def tdoa(self, k=None):
        """time differences of arrival in seconds, a host array [E_k, P] (events of class ``k``; None: all events, in event
        order), one column per microphone pair (i, j), i < j in lexicographic order; channel j hearing the sound ``d`` seconds
        after channel i gives ``-d``.  Only on the result of a localising detector (``EventDetector(..., localize=TDOA())``)."""
        if "lag" not in self.events or self.sr is None:
            raise ValueError("this result holds no lags: detect with EventDetector(..., localize=sed.TDOA(...)) or pass it through "
                             "det.localize(result, waveform, ...)")
        lag = self.events["lag"].cpu().numpy().astype(np.float64) / float(self.sr)
        return lag if k is None else lag[self.events["cls"].cpu().numpy() == int(k)]

    def doa(self, k=None):
        """directions of arrival, a host array [E_k, 3] (events of class ``k``; None: all events, in event order): azimuth and
        elevation in radians (``u = (cos el cos az, cos el sin az, sin el)`` points from the array to the source) and the
        steered response power per pair and frame, in [-1, 1]; NaN where an event was not located.  Only on the result of a
        detector with ``localize=DOA(...)``."""
        if "dir" not in self.events or self.grid is None:
            raise ValueError("this result holds no directions: detect with EventDetector(..., localize=sed.DOA(...)) or pass it "
                             "through det.localize(result, waveform, ...)")
        return _doa_angles(self.events, self.grid, k)

    def doa_track(self, e):
        """the direction track of event ``e``, a host array [T_e, 4]: per block of the event's located frames
        (``localize.track_blocks``) its centre time in seconds, the azimuth and elevation in radians of ``trk_dir`` and the
        block's steered response power per pair and frame; a silent block has NaN angles, an event that was not located no
        rows.  Only on the result of a detector with ``localize=DOA(..., track=DirectionTrack(...))``."""
        return _doa_track(self, e)

    def event_audio(self, e):
        """the beamformed audio of event ``e``: a float32 device slice of ``audio`` at the detector's rate, empty
        where the event was not located.  Only on the result of a detector with ``extract=sed.DelaySum(...)``; the host reads
        the event's two integers."""
        return _event_audio(self, e)

    @property
    def noise_frames(self):
        """int32 [E] on the device: the pre-onset frames every event's MVDR weights were made from — ``noise_blocks``, or 0 for
        an event that fell back to its own frames or was not extracted.  Only on the result of a detector with
        ``extract=sed.MVDR(noise_blocks >= 1)``: otherwise AttributeError."""
        return _noise_frames(self)

    @property
    def bg_frames(self):
        """int32 [E] on the device: the background frames every event's contrasted map was made with — up to ``Contrast.frames``, or
        0 for an event whose map is the plain one.  Only on the result of a detector with
        ``localize=sed.DOA(..., contrast=sed.Contrast(...))``: otherwise AttributeError."""
        return _bg_frames(self)


def _noise_frames(result):
    if "noise_frames" not in result.events:
        raise AttributeError("this result holds no noise_frames: detect with EventDetector(..., localize=sed.DOA(...), "
                             "extract=sed.MVDR(noise_blocks=...))")
    return result.events["noise_frames"]


def _bg_frames(result):
    if "bg_frames" not in result.events:
        raise AttributeError("this result holds no bg_frames: detect with EventDetector(..., localize=sed.DOA(..., "
                             "contrast=sed.Contrast(...)))")
    return result.events["bg_frames"]


def _event_audio(result, e):
    if result.audio is None or "audio_start" not in result.events:
        raise ValueError("this result holds no audio: detect with EventDetector(..., localize=sed.DOA(...), extract=sed.DelaySum(...)) "
                         "or pass it through det.localize(result, waveform, ...)")
    E = int(result.events["audio_start"].numel())
    if not -E <= int(e) < E:
        raise IndexError(f"event {e} of {E}")
    start, n = int(result.events["audio_start"][int(e)]), int(result.events["audio_len"][int(e)])
    return result.audio[start:start + n]


class BatchDetectionResult:
    """R recordings detected together.  ``len()`` = R; ``res[i]`` = a DetectionResult view of recording i (its slice of the
    track and of the events, without ``rec``; frames local to the recording).  Packed: ``probs`` [sum n_out, K] device track,
    ``events`` dict of device tensors with ``rec`` (sorted by recording, class, onset), and the host lists ``out_offsets``
    [R+1] (recording i = rows [out_offsets[i], out_offsets[i+1])) and ``event_offsets`` [R+1]."""

    def __init__(self, probs, events, frame_seconds, plans, out_offsets, event_offsets, sr=None, grid=None, audio=None, track=None):
        self.probs, self.events, self.frame_seconds, self.plans = probs, events, frame_seconds, tuple(plans)
        self.out_offsets, self.event_offsets = list(out_offsets), list(event_offsets)
        self.sr, self.grid, self.audio, self.track = sr, grid, audio, track          # as in DetectionResult

    def __len__(self):
        return len(self.plans)

    def __getitem__(self, i):
        R = len(self.plans)
        if not -R <= int(i) < R:
            raise IndexError(f"recording {i} of {R}")
        i = int(i) % R
        o0, o1 = self.out_offsets[i], self.out_offsets[i + 1]
        e0, e1 = self.event_offsets[i], self.event_offsets[i + 1]
        keys = _EVENT_KEYS + tuple(k for k in _TDOA_KEYS + _DOA_KEYS + _TRACK_KEYS + _BEAM_KEYS + _NOISE_KEYS + _QUIET_KEYS + _CONTRAST_KEYS if k in self.events)
        return DetectionResult(self.probs[o0:o1], {k: self.events[k][e0:e1] for k in keys}, self.frame_seconds, self.plans[i], self.sr,
                               self.grid, self.audio, self.track)

    def doa_track(self, e):
        """the direction track of event ``e`` of the packed table (``DetectionResult.doa_track``)"""
        return _doa_track(self, e)

    def event_audio(self, e):
        """the beamformed audio of event ``e`` of the packed table (``DetectionResult.event_audio``)"""
        return _event_audio(self, e)

    @property
    def noise_frames(self):
        """int32 [E] on the device: the pre-onset frames every event's MVDR weights were made from — ``noise_blocks``, or 0 for
        an event that fell back to its own frames or was not extracted.  Only on the result of a detector with
        ``extract=sed.MVDR(noise_blocks >= 1)``: otherwise AttributeError."""
        return _noise_frames(self)

    @property
    def bg_frames(self):
        """int32 [E] on the device: the background frames every event's contrasted map was made with — up to ``Contrast.frames``, or
        0 for an event whose map is the plain one.  Only on the result of a detector with
        ``localize=sed.DOA(..., contrast=sed.Contrast(...))``: otherwise AttributeError."""
        return _bg_frames(self)

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    @property
    def n_events(self):
        return self.event_offsets[-1]


class EventDetector:
    """Detect events in whole recordings with a trained net in ``eval()`` mode (see the module docstring).

    ``combine`` "mean" | "max" over overlapping windows; ``trim`` output frames dropped at interior window edges;
    ``threshold`` (hi) / ``low`` (lo, default = threshold): runs of p' > lo kept when max p' > hi; ``median`` odd filter width
    in output frames (1 = off); ``min_gap`` merge events separated by at most that many frames; ``min_len`` drop shorter
    events.  Each of these five is a scalar or a sequence of K = ``model.dense[-1]`` values, one per class (list, tuple,
    ndarray or 1-D tensor): with any sequence the detector is CLASS-WISE (``det.classwise``; scalars broadcast, ``low=None``
    means low_k = threshold_k) and every decode — single, batched, streamed — runs class k with its own five values
    (DESIGN 5l).  ``mean`` / ``std``: the float64 [C*F] scaler of ``data.standard_scaler_fit`` (one entry per feature column: [F] for a
    1-channel net), fused into the log-mel front end.  ``spatial="gcc_phat"``: the net reads spatial features — C
    mel images and one GCC-PHAT image per microphone pair, ``model.in_channels = C + C(C-1)/2`` for C = 2..8 audio channels —
    and every waveform entry point (``det(wave, sr=, channels=C)``, ``detect_many``, ``stream``) takes ``[N, C]`` PCM and makes
    them on the device; ``mean`` / ``std`` are ``in_channels * n_mels`` wide.  ``compress=sed.PCEN(...)``: the net
    was trained on PCEN features — every waveform entry point (``det(...)``, ``detect_many``, ``stream``) makes the mel columns
    with ``feature.mbe(..., compress=)`` and ``mean`` / ``std`` are the scaler of such features; ``from_features*`` and
    ``push_features`` take finished features and apply nothing.  ``localize=sed.TDOA(max_lag, max_frames)``: for a
    net that reads at least 2 audio channels, ``det(wave, sr=, channels=C)`` and ``detect_many`` keep the resampled planar PCM
    until the decode is done and return events that also hold ``lag`` [E, P] (samples at the detector's rate, one column per
    microphone pair; ``result.tdoa()`` in seconds), ``strength`` [E, P] and ``loc_frames`` [E] (``events.event_tdoa``);
    ``from_features*`` has no audio and returns un-located events, which ``det.localize(result, waveform, ...)`` locates.
    ``localize=sed.DOA(positions, grid, ...)`` for a known array: the same three keys, with ``max_lag`` taken from the
    array's aperture, and ``dir`` [E] (a row of ``grid``, -1: not located) and ``doa_power`` [E] (``events.event_doa``;
    ``result.doa()`` in radians); with ``sed.DOA(..., track=sed.DirectionTrack(block_chunks, max_step_deg))`` also a direction
    per block of the event's located frames, ``trk_len`` [E], ``trk_raw``, ``trk_dir`` and ``trk_power`` [E, Tm] (``result.doa_track(e)``).
    With ``sed.DOA(..., contrast=sed.Contrast(...))`` (offline only) the directions are made after the share of the sources
    that sound before the onset is removed — an event over a louder source of another class gets its own direction — the class
    count is the model's, and the events also hold ``bg_frames`` [E] (``result.bg_frames``) and ``bg_sel`` [E, frames].  ``extract=sed.DelaySum(...)``(needs ``localize=sed.DOA(...)``): every located event
    also comes with its audio, the array pointed at ``dir`` by a delay-and-sum beam (``events.event_beamform`` on the PCM that
    is kept anyway): ``audio_start`` / ``audio_len`` [E] in the events, the packed float32 buffer ``result.audio`` and
    ``result.event_audio(e)``; ``from_features*`` returns events without audio, ``det.localize`` adds it, ``det.stream`` of such a
    detector takes ``history_frames=`` and ``emit_audio=True`` and emits the same audio on live feeds.
    ``extract=sed.MVDR(loading)`` instead: the same events, samples and results through an adaptive beam that
    suppresses what else the event's frames contain (``events.event_mvdr``; live feeds: ``events.event_mvdr_ring``).  With
    ``sed.MVDR(noise_blocks=Kn)``, ``Kn >= 1``, the weights come from the Kn frames before the onset where the
    recording has them, and the events and ``result.noise_frames`` also hold ``noise_frames``.  With
    ``sed.MVDR(noise_blocks=Kn, noise_select="quiet")`` the Kn frames are the nearest before the onset in which the
    detector's own events of that class are silent — the class count is the model's — and the events also hold ``noise_sel``
    [E, Kn]; offline only: ``stream(..., emit_audio=True)`` of such a detector raises NotImplementedError."""

    def __init__(self, model, seq_len=SEQ_LEN_IN, hop=None, combine="mean", trim=0, threshold=0.5, low=None, median=1,
                 min_gap=0, min_len=1, mean=None, std=None, sr=feature.SR, hop_length=feature.HOP, max_batch=1024, spatial=None,
                 compress=None, localize=None, extract=None):
        if not isinstance(model, HipCRNN):
            raise TypeError(f"EventDetector needs a sed_crnn_amd net, got {type(model).__name__}")
        feature._check_compress(compress)
        self.compress = compress                # PCEN instead of the log on the mel columns of every waveform entry point
        # spatial features: the net reads C mel images and one GCC-PHAT image per microphone pair of C audio channels
        self.spatial, self.audio_channels = spatial, model.in_channels
        if spatial is not None:
            if spatial not in feature.SPATIAL:
                raise ValueError(f"spatial must be None or 'gcc_phat', got {spatial!r}")
            self.audio_channels = feature.audio_channels_of(model.in_channels)
            if self.audio_channels is None:
                raise ValueError(f"spatial={spatial!r} needs a net with in_channels = C + C(C-1)/2 for C = 2..{feature.GCC_MAX_CHANNELS} audio "
                                 f"channels ({', '.join(str(feature.spatial_channels(c)) for c in range(2, feature.GCC_MAX_CHANNELS + 1))}), "
                                 f"the net has in_channels={model.in_channels}")
            if model.n_mels % 2:
                raise ValueError(f"spatial={spatial!r} writes n_mels lags per pair and needs an even count, the net has n_mels={model.n_mels}")
        from .localize import DOA, MVDR, TDOA, DelaySum
        if extract is not None and not isinstance(extract, (DelaySum, MVDR)):
            raise TypeError(f"extract must be None, a DelaySum(...) or an MVDR(...) settings object, got {type(extract).__name__}")
        if extract is not None and not isinstance(localize, DOA):
            raise ValueError(f"extract={type(extract).__name__}(...) points the array at every event's direction and needs "
                             f"localize=sed.DOA(positions, grid), got localize={localize!r}")
        if getattr(extract, "follow_track", False) and localize.track is None:
            raise ValueError("extract=sed.MVDR(follow_track=True) steers the beam along every event's direction track and needs "
                             "localize=sed.DOA(positions, grid, track=sed.DirectionTrack(...))")
        self.extract_settings = extract         # per-event audio: a delay-and-sum or an MVDR beam (5s), or None
        if localize is not None and not isinstance(localize, (TDOA, DOA)):
            raise TypeError(f"localize must be None, a TDOA(...) or a DOA(...) settings object, got {type(localize).__name__}")
        if localize is not None and not 2 <= self.audio_channels <= feature.GCC_MAX_CHANNELS:
            raise ValueError(f"localize= needs a net that reads 2 to {feature.GCC_MAX_CHANNELS} audio channels (one time difference per "
                             f"microphone pair), this one reads {self.audio_channels}")
        if isinstance(localize, DOA):
            if localize.channels != self.audio_channels:
                raise ValueError(f"localize=DOA(...) holds {localize.channels} microphone positions, the net reads {self.audio_channels} "
                                 f"audio channels")
            localize.plan(sr)                                # (an aperture of more than 127 samples at this rate is refused here)
        # per-event TDOA or DOA (5q) settings of the waveform entry points, or None; ``localize_tdoa``: the TDOA
        # settings either of them means
        self.localize_settings = localize
        self.localize_tdoa = localize.tdoa(sr) if isinstance(localize, DOA) else localize
        if combine not in ("mean", "max"):
            raise ValueError(f"combine must be 'mean' or 'max', got {combine!r}")
        K = model.dense[-1]
        if K > 32:
            raise ValueError(f"event decoding handles up to 32 classes, the net has {K}")
        classwise, rows = _class_settings(K, threshold, low, median, min_gap, min_len)
        if any(r["min_gap"] < 0 or r["min_len"] < 1 for r in rows) or int(max_batch) < 1:
            raise ValueError("need min_gap >= 0, min_len >= 1 and max_batch >= 1")
        if (mean is None) != (std is None):
            raise ValueError("give both mean and std (data.standard_scaler_fit) or neither")
        self.model = model
        self.seq_len, self.hop = int(seq_len), (int(seq_len) // 2 if hop is None else int(hop))
        self.combine, self.trim = combine, int(trim)
        self._combine_id = ("mean", "max").index(combine)                  # as the stitch entries take it
        # scalars, or (class-wise) lists of K: a detector given any per-class argument decodes with the class-wise entries
        self.classwise, self._classes, self._ctab = classwise, rows, None
        col = (lambda n: [r[n] for r in rows]) if classwise else (lambda n: rows[0][n])
        self.hi, self.lo = col("threshold"), col("low")
        self.median, self.min_gap, self.min_len = col("median"), col("min_gap"), col("min_len")
        self.median_max = max(r["median"] for r in rows)                   # what a stream's state is sized with
        self.mean = None if mean is None else torch.as_tensor(mean, dtype=torch.float64)      # numpy or device tensors
        self.std = None if std is None else torch.as_tensor(std, dtype=torch.float64)
        if self.mean is not None and model.in_channels > 1:
            CF = model.in_channels * model.n_mels
            if (self.mean.numel() != CF or self.std.numel() != CF) and spatial is not None:
                raise ValueError(f"spatial={spatial!r}: a net with in_channels={model.in_channels} ({self.audio_channels} audio channels) and "
                                 f"{model.n_mels} mel bands needs mean / std of width (C+P)*n_mels = {model.in_channels}*{model.n_mels} = "
                                 f"{CF}, got {self.mean.numel()} / {self.std.numel()}")
            if self.mean.numel() != CF or self.std.numel() != CF:
                raise ValueError(f"a {model.in_channels}-channel net with {model.n_mels} mel bands needs mean / std of width "
                                 f"{model.in_channels}*{model.n_mels} = {CF} (data.standard_scaler_fit on [N, C*F] features), got "
                                 f"{self.mean.numel()} / {self.std.numel()}")
        self.sr, self.hop_length, self.max_batch = int(sr), int(hop_length), int(max_batch)
        plan_windows(4 * self.seq_len, model.time_factor, self.seq_len, self.hop, self.trim)     # validate the grid now
        self.max_events = 256                   # grows to the largest count seen
        self._zlab = None                       # zero label column for sed_window_batch (it requires one)
        self._dws = None
        self._bws = None                        # the batch entries' workspace
        self._tune_cache = {}                   # the sweep's workspace

    @property
    def frame_seconds(self):
        return self.model.time_factor * self.hop_length / self.sr

    def _check_model(self):
        """before any launch: the kernels take raw device pointers, so a model left on the CPU must never reach them"""
        if self.model.training:
            raise RuntimeError("EventDetector needs model.eval(): a training-mode forward would update the running statistics")
        arena = self.model.flat_parameters()
        if arena is None or not arena.is_cuda:
            raise SedHipError("sed_crnn_amd: move the module to the GPU first (model.to('cuda')); there is no CPU fallback")

    def stream(self, n_streams, keep_probs=False, **kw):
        """a ``stream.StreamDetector`` for ``n_streams`` live feeds with this detector's settings; ``input_sr`` /
        ``input_channels``: what ``push`` receives.  A localising detector streams with ``history_frames="min"`` or a
        number of feature frames: the audio every feed keeps for its emitted events; without it, NotImplementedError.  A detector with
        ``extract=`` streams with ``emit_audio=True``: every located event comes with its audio, the offline call's
        bit for bit (``StreamEvents.audio`` / ``event_audio``), for one more blocking 8-byte read and one device allocation per
        step that emits events; without ``emit_audio=True`` it raises NotImplementedError, and ``emit_audio=True`` on a detector
        without ``extract=`` ValueError."""
        from .stream import StreamDetector
        return StreamDetector(self.model, n_streams, keep_probs=keep_probs, _det=self, **kw)

    # ── scoring and tuning the decoder (tune.py) ──
    def decoder_settings(self):
        """this detector's decoder values, as ``with_decoder`` (and, for scalars, ``DecoderGrid``) takes them: scalars, or lists
        of K when the detector is class-wise"""
        g = (lambda v: list(v)) if self.classwise else (lambda v: v)
        return dict(threshold=g(self.hi), low=g(self.lo), median=g(self.median), min_gap=g(self.min_gap), min_len=g(self.min_len))

    def class_settings(self):
        """K dicts of scalars (``threshold``, ``low``, ``median``, ``min_gap``, ``min_len``): what class k is decoded with; on a
        scalar detector K copies of its one setting"""
        return [dict(r) for r in self._classes]

    def _class_table(self, K):
        """the K rows as the class-wise entries take them (a host array of sed_decoder_setting)"""
        if K != len(self._classes):
            raise ValueError(f"the track has {K} classes, the detector has settings for {len(self._classes)}")
        if self._ctab is None:
            self._ctab = (TuneSetting * K)(*[TuneSetting(r["median"], r["low"], r["threshold"], r["min_gap"], r["min_len"])
                                             for r in self._classes])
        return C.cast(self._ctab, C.c_void_p)

    def with_decoder(self, **settings):
        """A new detector that shares the model, the scaler and the window grid and has the decoder values (``threshold``,
        ``low``, ``median``, ``min_gap``, ``min_len``) replaced, each a scalar or one value per class (any sequence makes the
        new detector class-wise).  ``threshold`` without ``low`` means low = threshold."""
        extra = set(settings) - {"threshold", "low", "median", "min_gap", "min_len"}
        if extra:
            raise TypeError(f"with_decoder takes decoder settings only, got {sorted(extra)}")
        kw = self.decoder_settings()
        if "threshold" in settings and settings.get("low") is None:
            kw["low"] = None
        kw.update(settings)
        return EventDetector(self.model, seq_len=self.seq_len, hop=self.hop, combine=self.combine, trim=self.trim, mean=self.mean,
                             std=self.std, sr=self.sr, hop_length=self.hop_length, max_batch=self.max_batch, spatial=self.spatial,
                             compress=self.compress, localize=self.localize_settings, extract=self.extract_settings, **kw)

    def sweep(self, track, ref, grid, collar=1, offset_collar=None, offset_percent=None, block=None, max_workspace_bytes=1 << 30):
        """Score every decoder setting of ``grid`` (a ``DecoderGrid``) on a track against ``ref`` (a ``ReferenceEvents``) on
        the device -> ``SweepResult`` (``tune.sweep``).  ``track``: a BatchDetectionResult, a DetectionResult or
        ``(probs, out_offsets)``; ``collar`` in output frames (0..31); onset-only scoring unless ``offset_collar`` /
        ``offset_percent`` is given; ``block`` output frames per segment, default ``round(1 / frame_seconds)``."""
        from . import tune
        block = max(1, int(round(1.0 / self.frame_seconds))) if block is None else block
        return tune.sweep(track, ref, grid, collar, offset_collar, offset_percent, block, max_workspace_bytes, self._tune_cache)

    def score(self, result, ref, collar=1, offset_collar=None, offset_percent=None, block=None):
        """the sweep with G = 1 and this detector's own decoder setting: how good are ``result``'s events against ``ref``.  A
        class-wise detector sweeps its distinct class settings (at most K) and takes class k's counts from class k's setting, on
        the device: ``counts`` is still [1, K, 6] and ``grid[0]`` the detector's ``decoder_settings()``."""
        from .tune import DecoderGrid, SweepResult
        if not self.classwise:
            return self.sweep(result, ref, DecoderGrid.from_settings([self.decoder_settings()]), collar, offset_collar,
                              offset_percent, block)
        distinct = []
        for r in self._classes:
            if r not in distinct:
                distinct.append(r)
        res = self.sweep(result, ref, DecoderGrid.from_settings(distinct), collar, offset_collar, offset_percent, block)
        dev = res.counts.device
        g = torch.tensor([distinct.index(r) for r in self._classes], device=dev)
        row = res.counts[g, torch.arange(len(self._classes), device=dev)].unsqueeze(0).contiguous()
        return SweepResult(row, [self.decoder_settings()], res.collar, res.block, res.n_slices, res.n_tracks, res.workspace_bytes)

    def psds(self, track, ref, thresholds=50, criteria=None, grid=None, max_workspace_bytes=1 << 30):
        """The polyphonic sound detection score of a track against ``ref`` over a sweep of thresholds, on the device ->
        ``PSDSResult`` (``tune.psds_sweep``): no threshold has to be picked to compare two nets, front ends or
        decoders.  ``thresholds``: an int n for ``np.linspace(0.01, 0.99, n)``, or a sequence; each value is one setting with
        this detector's median, min_gap and min_len and lo = hi = the value.  An explicit ``grid`` (a ``DecoderGrid``) overrides
        ``thresholds``; a class-wise detector needs one, it has no single median to sweep around.  ``criteria``: a
        ``PSDSCriteria``, default ``PSDSCriteria.scenario1()``.  Rates are per hour of ``frame_seconds``."""
        from . import tune
        if grid is None:
            if self.classwise:
                raise ValueError("a class-wise detector has no single median to sweep thresholds around: give an explicit grid")
            values = np.linspace(0.01, 0.99, thresholds) if isinstance(thresholds, (int, np.integer)) else list(thresholds)
            grid = tune.DecoderGrid.from_settings([dict(threshold=float(v), median=self.median, min_gap=self.min_gap, min_len=self.min_len)
                                                   for v in values])
        criteria = tune.PSDSCriteria.scenario1() if criteria is None else criteria
        return tune.psds_sweep(track, ref, grid, criteria, self.frame_seconds, max_workspace_bytes, self._tune_cache)

    # ── the whole path ──
    def __call__(self, waveform, sr=None, channels=1):
        """mono PCM (1-D tensor / ndarray) -> DetectionResult.  The log-mel front end is ``feature.mbe(..., mean, std)``.
        ``sr`` / ``channels``: the waveform is at that rate (default: the detector's), int16 or float, ``[N, channels]``
        interleaved, and is converted, downmixed and resampled to the detector's rate on the device first; event
        times need no change, they are in seconds at the detector's rate.  A net with ``in_channels = C > 1`` takes
        ``[N, C]`` interleaved PCM with ``channels=C``: the channels are kept, each resampled and turned into its own feature
        columns; nothing is mixed down and a mono signal is not duplicated."""
        if self.model.in_channels != 1:
            self._check_channels(channels)
            self._check_model()
            dev = self.model.flat_parameters().device
            with torch.no_grad():
                if self.localize_settings is not None:       # the same front end, whose planar PCM is kept until the events are decoded
                    mel, _, pcm, clips = feature.mbe_many([waveform], sr=self.sr, hop=self.hop_length, n_mels=self.model.n_mels,
                                                          mean=self.mean, std=self.std, input_sr=sr, channels=channels, keep_channels=True,
                                                          device=dev, spatial=self.spatial, compress=self.compress, return_pcm=True)
                    return self._located(self.from_features(mel), pcm, clips)
                mel = feature.mbe(waveform, sr=self.sr, hop=self.hop_length, n_mels=self.model.n_mels, mean=self.mean, std=self.std,
                                  input_sr=sr, channels=channels, keep_channels=True, device=dev, spatial=self.spatial,
                                  compress=self.compress)
            return self.from_features(mel)
        self._check_model()
        if feature._needs_front_end(waveform, sr, self.sr, channels):
            from .resample import resample
            waveform = resample(waveform, self.sr if sr is None else sr, self.sr, channels, self.model.flat_parameters().device)
        y = torch.as_tensor(waveform)
        if y.dim() != 1:
            raise ValueError(f"expected a mono 1-D waveform, got shape {tuple(y.shape)}")
        dev = self.model.flat_parameters().device
        with torch.no_grad():
            mel = feature.mbe(y.to(dev, torch.float32), sr=self.sr, hop=self.hop_length, n_mels=self.model.n_mels,
                              mean=self.mean, std=self.std, compress=self.compress)
        return self.from_features(mel)

    def _check_channels(self, channels):
        """a multichannel net takes exactly its own channel count: no mix-down, no duplication of a mono signal"""
        C_in = self.audio_channels
        if self.spatial is not None and int(channels) != C_in:
            raise ValueError(f"spatial={self.spatial!r}: a net with in_channels={self.model.in_channels} reads {C_in} audio channels "
                             f"({C_in} mel images + {C_in * (C_in - 1) // 2} microphone pairs) and takes [N, {C_in}] interleaved PCM "
                             f"with channels={C_in}, got channels={int(channels)}")
        if int(channels) != C_in:
            raise ValueError(f"a {C_in}-channel net takes [N, {C_in}] interleaved PCM with channels={C_in}, got channels={int(channels)}: "
                             f"there is no mix-down to fewer channels and no duplication of a mono signal (scaled features go "
                             f"through from_features)")

    # ── where the events came from ──
    def _located(self, result, pcm, clips):
        """``result``, MODIFIED IN PLACE and returned, with ``lag``, ``strength`` and ``loc_frames`` added to its events (a new dict)
        and ``sr`` set: ``events.event_tdoa`` on the planar PCM at the detector's rate that the events were detected in"""
        t = self.localize_settings
        with torch.no_grad():
            if self.locates_directions:
                contrast = dict(n_classes=self.model.dense[-1]) if t.contrast is not None else {}   # the class count is the model's
                loc = event_doa(pcm, clips, self.audio_channels, result.events, self.model.time_factor, t, sr=self.sr,
                                        hop=self.hop_length, **contrast)
                result.grid, result.track = t.grid, self._track_info()
            else:
                loc = event_tdoa(pcm, clips, self.audio_channels, result.events, self.model.time_factor, max_lag=t.max_lag,
                                         max_frames=t.max_frames, hop=self.hop_length)
            if self.extract_settings is not None:            # the audio of the located events, from the same PCM
                from .localize import MVDR
                entry = event_mvdr if isinstance(self.extract_settings, MVDR) else event_beamform
                quiet = dict(n_classes=self.model.dense[-1]) if getattr(self.extract_settings, "quiet", False) else {}
                beam = entry(pcm, clips, self.audio_channels, {**result.events, **loc}, self.model.time_factor, t,
                             self.extract_settings, sr=self.sr, hop=self.hop_length, **quiet)
                result.audio = beam.pop("audio")
                loc.update(beam)
        result.events = {**{k: v for k, v in result.events.items() if k not in _TDOA_KEYS + _DOA_KEYS + _TRACK_KEYS + _BEAM_KEYS + _NOISE_KEYS + _QUIET_KEYS + _CONTRAST_KEYS}, **loc}
        result.sr = self.sr
        return result

    @property
    def locates_directions(self):
        """whether the localisation settings are ``DOA(...)``: the events also hold ``dir`` and ``doa_power``"""
        from .localize import DOA
        return isinstance(self.localize_settings, DOA)

    def _track_info(self):
        """what ``doa_track`` of a result needs beside its events: (DirectionTrack, max_frames, time_factor, hop_length), or None"""
        t = self.localize_settings
        if not self.locates_directions or t.track is None:
            return None
        return (t.track, t.max_frames, self.model.time_factor, self.hop_length)

    def localize(self, result, waveforms, sr=None, channels=None):
        """Locate events that were detected without their audio at hand (``from_features*``): ``result`` — a DetectionResult with
        the ``[N, C]`` waveform it came from, or a BatchDetectionResult with the list of them — gets ``lag``, ``strength`` and
        ``loc_frames`` (class docstring): the object that was passed in is modified (its ``events`` becomes a new dict with the
        three keys, its ``sr`` is set) and returned.  ``sr`` / ``channels``: as in ``__call__``; the audio is resampled to
        the detector's rate exactly as the waveform entry points do it, so the result equals theirs bit for bit.  Needs a
        detector made with ``localize=sed.TDOA(...)``."""
        if self.localize_settings is None:
            raise ValueError("this detector has no localisation settings: make it with EventDetector(..., localize=sed.TDOA(...))")
        channels = self.audio_channels if channels is None else channels
        self._check_channels(channels)
        self._check_model()
        batch = isinstance(result, BatchDetectionResult)
        if not batch and not isinstance(result, DetectionResult):
            raise TypeError(f"localize takes a DetectionResult or a BatchDetectionResult, got {type(result).__name__}")
        waves = list(waveforms) if batch else [waveforms]
        if len(waves) != (len(result) if batch else 1):
            raise ValueError(f"the result holds {len(result)} recordings, {len(waves)} waveforms were given")
        if not waves:
            result.events = {**result.events, **self._no_lags()}
            result.sr = self.sr
            if self.extract_settings is not None:
                result.audio = torch.empty(0, device=self.model.flat_parameters().device)
            result.grid = self.localize_settings.grid if self.locates_directions else None
            result.track = self._track_info()
            return result
        from .resample import resample_many
        pcm, clips = resample_many(waves, self.sr if sr is None else sr, self.sr, channels, self.model.flat_parameters().device,
                                   keep_channels=True)
        plans = result.plans if batch else (result.plan,)
        for i, p in enumerate(plans):
            n_feat = 1 + clips[i * int(channels)][1] // self.hop_length
            if n_feat != p.n_frames:
                raise ValueError(f"recording {i}: the waveform makes {n_feat} feature frames, the result was detected in {p.n_frames}")
        return self._located(result, pcm, clips)

    def from_features(self, mel):
        """Scaled features [N, C*F] (the .npz cache layout; channel c = columns [c*F, (c+1)*F)) -> DetectionResult.  There is no
        audio here: the events of a localising detector come back un-located (``det.localize`` adds the lags)."""
        self._check_model()
        with torch.no_grad():
            mel, plan = self._prepare(mel)
            logits = self.window_logits(mel, plan)
            probs = self.stitch(logits, plan)
            events = self.decode(probs)
        return DetectionResult(probs, events, self.frame_seconds, plan)

    # ── phases (public so that tools can time them one by one) ──
    def _prepare(self, mel):
        self._check_model()
        m = self.model
        dev = m.flat_parameters().device
        mel = torch.as_tensor(mel)
        CF = m.in_channels * m.n_mels
        if mel.dim() != 2 or mel.shape[1] != CF:
            raise ValueError(f"expected features [N, {CF}] (C*F = {m.in_channels}*{m.n_mels}), got {tuple(mel.shape)}")
        mel = mel.to(dev, torch.float32).contiguous()
        return mel, plan_windows(mel.shape[0], m.time_factor, self.seq_len, self.hop, self.trim)

    def window_logits(self, mel, plan, marks=None):
        """Every window of the plan through the eval forward -> logits [n_win, win_out, K] (``_forward_windows``).
        ``marks`` (optional list): receives ("gather" | "forward", start, end) hip event pairs around every launch, for
        per-phase timing."""
        m = self.model
        self._check_model()
        logits = torch.empty(plan.n_win, plan.win_out, m.dense[-1], device=mel.device)
        self._forward_windows(mel, _window_jobs(logits.view(-1), [(plan.win_len, plan.starts)], m.time_factor, m.dense[-1]), marks)
        return logits

    def _forward_windows(self, mel, jobs, marks=None):
        """The chunked eval forward of both paths.  ``jobs`` = [(starts, win_len, out), ...]: int32 device window starts
        (rows of ``mel``), their length, and the logits [n, win_len // tf, K] they go to.  Chunks of at most max_batch windows:
        each is gathered by one sed_window_batch launch into ONE reused buffer (memory is bounded by max_batch, not by the
        input's length) and run on ONE workspace, that of the largest need among the jobs' shapes, checked with
        sed_net_workspace_bytes for every other shape (the eval forward of a batch equals that of its chunks bit for bit)."""
        m, N = self.model, mel.shape[0]
        dev = mel.device
        if self._zlab is None or self._zlab.numel() < N or self._zlab.device != dev:
            self._zlab = torch.zeros(max(N, 1 << 16), device=dev)
        CF = m.in_channels * m.n_mels
        shapes = [(min(self.max_batch, starts.numel()), Lw) for starts, Lw, _ in jobs]
        xbuf = torch.empty(max(b * Lw for b, Lw in shapes) * CF, device=dev)
        y = torch.empty(max(b for b, _ in shapes), device=dev)        # the pooled zero labels: pool = Lw -> one per window
        P, _ = m._param_structs()
        cfgs = [m._cfg(b, Lw, training=False) for b, Lw in shapes]
        need = [lib().sed_net_workspace_bytes(C.byref(c), 0) for c in cfgs] if len(cfgs) > 1 else [0]
        ws = m._workspace(cfgs[max(range(len(cfgs)), key=need.__getitem__)], False)
        cap = ws.numel() * 4

        for (starts, Lw, logits), (bmax, _), cfg in zip(jobs, shapes, cfgs):
            nw = starts.numel()
            x = xbuf[:bmax * CF * Lw].view(bmax, m.in_channels, m.n_mels, Lw)
            m._check_input(x[:1])
            for b0 in range(0, nw, bmax):
                b = min(bmax, nw - b0)
                if b != cfg.B:
                    cfg = m._cfg(b, Lw, training=False)
                    if lib().sed_net_workspace_bytes(C.byref(cfg), 0) > cap:
                        check(-1, "sed_net_workspace_bytes (a smaller chunk needs a larger workspace)")
                _timed(marks, "gather", lambda: check(lib().sed_window_batch(
                    ptr(mel), ptr(self._zlab), N, m.in_channels, m.n_mels, 1, ptr(starts[b0:b0 + b]), None, None, 0, 0, 0,
                    ptr(x), ptr(y), b, Lw, Lw, stream_ptr()), "sed_window_batch"))
                _timed(marks, "forward", lambda: check(lib().sed_net_forward(
                    C.byref(cfg), C.byref(P), ptr(x), ptr(logits[b0:b0 + b]), ptr(ws), 0, 0, None, stream_ptr()),
                    "sed_net_forward"))

    def stitch(self, logits, plan):
        """window logits -> probs [n_out, K] (sigmoid, then mean / max over the covering windows)."""
        K = logits.shape[2]
        probs = torch.empty(plan.n_out, K, device=logits.device)
        check(lib().sed_detect_stitch(ptr(logits), plan.n_win, plan.win_out, K, plan.hop_out, plan.last_start_out,
                                      plan.n_out, self._combine_id, self.trim, ptr(probs), stream_ptr()),
              "sed_detect_stitch")
        return probs

    def decode(self, probs):
        """probs [n_out, K] -> events (dict of device tensors).  Reads the event count (one int) from the device; when it
        exceeds the buffers, they grow and only the decode kernels run again."""
        n_out, K = probs.shape
        probs = probs.contiguous()
        dev = probs.device
        need = lib().sed_detect_workspace_bytes(n_out, K, self.max_events)
        if need == 0:
            check(-1, "sed_detect_workspace_bytes")
        if self._dws is None or self._dws.numel() < need or self._dws.device != dev:
            self._dws = torch.empty(need, dtype=torch.uint8, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        if self.classwise:
            table = self._class_table(K)
            return self._decode_growing(_EVENT_KEYS, count, lambda cap, out: check(lib().sed_detect_events_classwise(
                ptr(probs), n_out, K, table, cap, ptr(self._dws), self._dws.numel(), *(ptr(out[n]) for n in _EVENT_KEYS), ptr(count),
                stream_ptr()), "sed_detect_events_classwise"))[0]
        return self._decode_growing(_EVENT_KEYS, count, lambda cap, out: check(lib().sed_detect_events(
            ptr(probs), n_out, K, self.median, self.lo, self.hi, self.min_gap, self.min_len, cap, ptr(self._dws), self._dws.numel(),
            *(ptr(out[n]) for n in _EVENT_KEYS), ptr(count), stream_ptr()), "sed_detect_events"))[0]

    def _decode_growing(self, keys, counts, launch):
        """``launch(cap, out)`` decodes into event buffers of ``cap`` events and leaves its counts, the last one the total, in the
        device tensor ``counts``: reading them is the one read.  When the total exceeds ``cap`` the buffers grow to it and the
        decode runs again.  -> (events cut to the total, the counts as a host list)"""
        while True:
            cap = self.max_events
            out = _event_tensors(keys, cap, counts.device)
            launch(cap, out)
            offs = counts.cpu().tolist()
            if offs[-1] <= cap:
                return {k: v[:offs[-1]] for k, v in out.items()}, offs
            self.max_events = offs[-1]

    # ── batches: many recordings in one pass ──
    def detect_many(self, waveforms, sr=None, channels=1):
        """A list of mono PCM clips (1-D, host or device, any lengths) -> BatchDetectionResult.  One log-mel launch for all
        (``feature.mbe_many``, fused scaler), then ``from_features_many``'s path.  A clip shorter than one output frame
        raises ValueError naming its index before anything runs.  ``sr`` (one rate, or one per clip) / ``channels``: as in
        ``__call__``; the clips of one rate are resampled in one launch, straight into the buffer the log-mel launch reads.
        A net with ``in_channels = C > 1`` takes ``[N, C]`` clips with ``channels=C``: one launch per (rate, format) group writes
        the planar channels of its clips, one ``sed_logmel_multi`` launch turns all of them into ``[sum N, C*F]``.

        Memory, per input frame (hop_length samples): the packed PCM (4*hop_length B), the packed features (4*n_mels B),
        the flat logits (4*K*seq_len/hop/tf B: every frame is in seq_len/hop windows) and the track (4*K/tf B); the window
        buffer is bounded by max_batch windows, the decoder's bit tracks take 2 bits per output frame and class."""
        m = self.model
        waves = list(waveforms)
        multi = m.in_channels != 1                                         # [N, C] clips, channels kept
        if multi:
            self._check_channels(channels)
        front = multi or sr is not None and np.ndim(sr) > 0 or any(feature._needs_front_end(w, sr, self.sr, channels) for w in waves)
        if front:
            from .resample import _rates, as_pcm, plan_for
            waves = [as_pcm(w, channels, f"recording {i}") for i, w in enumerate(waves)]
            rates = _rates(self.sr if sr is None else sr, len(waves))
            lengths = [plan_for(r, self.sr).n_out(w.shape[0]) for r, w in zip(rates, waves)]
        n_frames = []
        for i, w in enumerate(waves):
            shape = tuple(w.shape) if hasattr(w, "shape") else (len(w),)
            if front:
                shape = (lengths[i],)
            if len(shape) != 1:
                raise ValueError(f"recording {i}: expected a mono 1-D waveform, got shape {shape}")
            n_frames.append(1 + shape[0] // self.hop_length)
        bp = plan_batch(n_frames, m.time_factor, m.dense[-1], self.seq_len, self.hop, self.trim)
        self._check_model()
        if not waves:
            return self._empty_batch()
        dev = m.flat_parameters().device
        with torch.no_grad():
            mel, _, *kept = feature.mbe_many(waves, sr=self.sr, hop=self.hop_length, n_mels=m.n_mels, mean=self.mean, std=self.std,
                                             device=dev, compress=self.compress, **(dict(input_sr=rates, channels=channels) if front else {}),
                                             **(dict(keep_channels=True, spatial=self.spatial) if multi else {}),
                                             **(dict(return_pcm=True) if self.localize_settings is not None else {}))
            res = self._detect_packed(mel, bp)
            return self._located(res, *kept) if self.localize_settings is not None else res

    def from_features_many(self, mels):
        """A list of scaled features [N_r, C*F] (any channel count, host or device) -> BatchDetectionResult (un-located, as
        ``from_features``).  The features are packed back to back; every window of every recording goes through the chunked eval forward, then ONE stitch
        launch and ONE decode; the host reads the R+1 event offsets once at the end (see ``detect_many`` for the memory)."""
        m = self.model
        CF = m.in_channels * m.n_mels
        mels = [torch.as_tensor(x) for x in mels]
        for i, x in enumerate(mels):
            if x.dim() != 2 or x.shape[1] != CF:
                raise ValueError(f"recording {i}: expected features [N, {CF}] (C*F = {m.in_channels}*{m.n_mels}), "
                                 f"got {tuple(x.shape)}")
        bp = plan_batch([x.shape[0] for x in mels], m.time_factor, m.dense[-1], self.seq_len, self.hop, self.trim)
        self._check_model()
        if not mels:
            return self._empty_batch()
        dev = m.flat_parameters().device
        with torch.no_grad():
            return self._detect_packed(feature.cat_to_device(mels, dev).contiguous(), bp)

    def _empty_batch(self):
        m = self.model
        dev = m.flat_parameters().device
        ev = _event_tensors(("rec",) + _EVENT_KEYS, 0, dev)
        if self.localize_settings is not None:
            ev.update(self._no_lags())
        return BatchDetectionResult(torch.empty(0, m.dense[-1], device=dev), ev, self.frame_seconds, (), [0], [0],
                                    self.sr if self.localize_settings is not None else None,
                                    self.localize_settings.grid if self.locates_directions else None,
                                    torch.empty(0, device=dev) if self.extract_settings is not None else None, self._track_info())

    def _no_lags(self):
        """the localisation columns of an empty event table"""
        dev, P = self.model.flat_parameters().device, self.audio_channels * (self.audio_channels - 1) // 2
        out = {"lag": torch.empty(0, P, device=dev), "strength": torch.empty(0, P, device=dev),
               "loc_frames": torch.empty(0, dtype=torch.int32, device=dev)}
        if self.locates_directions:
            out.update(dir=torch.empty(0, dtype=torch.int32, device=dev), doa_power=torch.empty(0, device=dev))
            if self.localize_settings.track is not None:
                Tm = self.localize_settings.track.max_blocks(self.localize_settings.max_frames)
                out.update(trk_len=torch.empty(0, dtype=torch.int32, device=dev), trk_raw=torch.empty(0, Tm, dtype=torch.int32, device=dev),
                           trk_dir=torch.empty(0, Tm, dtype=torch.int32, device=dev), trk_power=torch.empty(0, Tm, device=dev))
            if self.localize_settings.contrast is not None:
                out.update(bg_frames=torch.empty(0, dtype=torch.int32, device=dev),
                           bg_sel=torch.empty(0, self.localize_settings.contrast.frames, dtype=torch.int32, device=dev))
        if self.extract_settings is not None:
            out.update(audio_start=torch.empty(0, dtype=torch.int64, device=dev), audio_len=torch.empty(0, dtype=torch.int32, device=dev))
        if getattr(self.extract_settings, "noise_blocks", 0):
            out.update(noise_frames=torch.empty(0, dtype=torch.int32, device=dev))
        if getattr(self.extract_settings, "quiet", False):
            out.update(noise_sel=torch.empty(0, self.extract_settings.noise_blocks, dtype=torch.int32, device=dev))
        return out

    def _detect_packed(self, mel, bp):
        logits = self.window_logits_many(mel, bp)
        probs = self.stitch_many(logits, bp)
        events, ev_off = self.decode_many(probs, bp)
        return BatchDetectionResult(probs, events, self.frame_seconds, bp.plans, bp.out_off, ev_off)

    def window_logits_many(self, mel, bp, marks=None):
        """Packed features [sum N_r, C*F] and their BatchPlan -> the flat logits buffer [bp.n_logits]: all full windows in
        chunks of at most max_batch (one sed_window_batch gather each, absolute starts), then every group of short
        recordings, all on one workspace (``_forward_windows``).  ``marks`` as in ``window_logits``."""
        self._check_model()
        m = self.model
        logits = torch.empty(bp.n_logits, device=mel.device)
        self._forward_windows(mel, _window_jobs(logits, ((self.seq_len, bp.full_starts),) + bp.groups, m.time_factor, m.dense[-1]),
                              marks)
        return logits

    def _batch_workspace(self, n_total, K, R):
        need = lib().sed_detect_batch_workspace_bytes(n_total, K, R, self.max_events)
        if need == 0:
            check(-1, "sed_detect_batch_workspace_bytes")
        if self._bws is None or self._bws.numel() < need or self._bws.device != self.model.flat_parameters().device:
            self._bws = torch.empty(need, dtype=torch.uint8, device=self.model.flat_parameters().device)
        return self._bws

    def stitch_many(self, logits, bp):
        """flat logits -> packed track [sum n_out, K] in ONE launch (sed_detect_stitch_batch); recording r's rows equal
        ``stitch`` of its own logits bit for bit."""
        K, R, n = self.model.dense[-1], len(bp.plans), bp.out_off[-1]
        table = bp.stitch_table()
        ws = self._batch_workspace(n, K, R)
        probs = torch.empty(n, K, device=logits.device)
        check(lib().sed_detect_stitch_batch(ptr(logits), logits.numel(), C.c_void_p(table.ctypes.data), R, K,
                                            self._combine_id, self.trim, ptr(probs), n, ptr(ws), ws.numel(),
                                            stream_ptr()), "sed_detect_stitch_batch")
        return probs

    def decode_many(self, probs, bp):
        """packed track -> (events with ``rec``, event offsets [R+1] host list).  The R+1 offsets are the one read of the
        batch; when the total exceeds the buffers, they grow and only the decode runs again.  Of ``bp`` only ``plans`` (its
        length, R) and ``out_off`` [R+1] are used: ``plan_batch([tf * n for n in n_out], tf, K)`` decodes a track that did
        not come from this detector's forward."""
        n_total, K = probs.shape
        R = len(bp.plans)
        n_out = np.ascontiguousarray(np.diff(np.asarray(bp.out_off, dtype=np.int64)))
        ws = self._batch_workspace(n_total, K, R)
        dev = probs.device
        ev_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
        keys = ("rec",) + _EVENT_KEYS
        if self.classwise:
            table = self._class_table(K)
            return self._decode_growing(keys, ev_off, lambda cap, out: check(lib().sed_detect_events_batch_classwise(
                ptr(probs), C.c_void_p(n_out.ctypes.data), R, K, table, cap, ptr(ws), ws.numel(), *(ptr(out[n]) for n in keys),
                ptr(ev_off), stream_ptr()), "sed_detect_events_batch_classwise"))
        return self._decode_growing(keys, ev_off, lambda cap, out: check(lib().sed_detect_events_batch(
            ptr(probs), C.c_void_p(n_out.ctypes.data), R, K, self.median, self.lo, self.hi, self.min_gap, self.min_len, cap, ptr(ws),
            ws.numel(), *(ptr(out[n]) for n in keys), ptr(ev_off), stream_ptr()), "sed_detect_events_batch"))


def detect_events_many(model, xs, input_sr=None, channels=1, **kw):
    """One shot over a list: ``EventDetector(model, **kw)`` on mono waveforms (all 1-D: ``detect_many``) or on scaled features
    [N_r, C*F] (``from_features_many``) -> BatchDetectionResult.  With ``input_sr`` or ``channels`` > 1 the list holds
    waveforms at that rate (``detect_many(xs, sr=input_sr, channels=channels)``; ``sr=`` stays the detector's own rate)."""
    det = EventDetector(model, **kw)
    xs = list(xs)
    if input_sr is not None or int(channels) != 1:
        return det.detect_many(xs, sr=input_sr, channels=channels)
    if xs and all(torch.as_tensor(x).dim() == 1 for x in xs):
        return det.detect_many(xs)
    return det.from_features_many(xs)


def detect_events(model, x, input_sr=None, channels=1, **kw):
    """One shot: ``EventDetector(model, **kw)`` on a mono waveform (1-D) or on scaled features [N, C*F] (2-D).  With
    ``input_sr`` or ``channels`` > 1, ``x`` is a waveform at that rate (``det(x, sr=input_sr, channels=channels)``)."""
    det = EventDetector(model, **kw)
    if input_sr is not None or int(channels) != 1:
        return det(x, sr=input_sr, channels=channels)
    return det(x) if torch.as_tensor(x).dim() == 1 else det.from_features(x)
