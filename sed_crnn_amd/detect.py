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

import torch

from . import feature
from ._lib import SedHipError, check, lib, ptr, stream_ptr
from .data import SEQ_LEN_IN
from .model import HipCRNN

_EVENT_KEYS = ("cls", "onset", "offset", "peak", "peak_frame")


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


class DetectionResult:
    """``probs`` [n_out, K] device track; ``events`` dict of device tensors (``cls``, ``onset``, ``offset``, ``peak_frame``
    int32 output frames, offset exclusive; ``peak`` float32), sorted by (class, onset); ``frame_seconds`` = tf*hop_length/sr."""

    def __init__(self, probs, events, frame_seconds, plan):
        self.probs, self.events, self.frame_seconds, self.plan = probs, events, frame_seconds, plan

    def __len__(self):
        return int(self.events["cls"].numel())

    def intervals(self, k=0):
        """[(start_s, end_s, peak), ...] of class ``k`` on the host (seconds = frame * tf * hop_length / sr)."""
        ev = {n: self.events[n].cpu().numpy() for n in ("cls", "onset", "offset", "peak")}
        sel = ev["cls"] == int(k)
        fs = self.frame_seconds
        return [(int(a) * fs, int(b) * fs, float(p)) for a, b, p in zip(ev["onset"][sel], ev["offset"][sel], ev["peak"][sel])]


class EventDetector:
    """Detect events in whole recordings with a trained net in ``eval()`` mode (see the module docstring).

    ``combine`` "mean" | "max" over overlapping windows; ``trim`` output frames dropped at interior window edges;
    ``threshold`` (hi) / ``low`` (lo, default = threshold): runs of p' > lo kept when max p' > hi; ``median`` odd filter width
    in output frames (1 = off); ``min_gap`` merge events separated by at most that many frames; ``min_len`` drop shorter
    events; ``mean`` / ``std``: the float64 [F] scaler of ``data.standard_scaler_fit``, fused into the log-mel front end."""

    def __init__(self, model, seq_len=SEQ_LEN_IN, hop=None, combine="mean", trim=0, threshold=0.5, low=None, median=1,
                 min_gap=0, min_len=1, mean=None, std=None, sr=feature.SR, hop_length=feature.HOP, max_batch=1024):
        if not isinstance(model, HipCRNN):
            raise TypeError(f"EventDetector needs a sed_crnn_amd net, got {type(model).__name__}")
        if combine not in ("mean", "max"):
            raise ValueError(f"combine must be 'mean' or 'max', got {combine!r}")
        lo = float(threshold if low is None else low)
        if not lo <= float(threshold):
            raise ValueError(f"low={low} must not exceed threshold={threshold}")
        if not (1 <= int(median) <= 31 and int(median) % 2 == 1):
            raise ValueError(f"median must be odd, 1..31, got {median}")
        if int(min_gap) < 0 or int(min_len) < 1 or int(max_batch) < 1:
            raise ValueError("need min_gap >= 0, min_len >= 1 and max_batch >= 1")
        if model.dense[-1] > 32:
            raise ValueError(f"event decoding handles up to 32 classes, the net has {model.dense[-1]}")
        if (mean is None) != (std is None):
            raise ValueError("give both mean and std (data.standard_scaler_fit) or neither")
        self.model = model
        self.seq_len, self.hop = int(seq_len), (int(seq_len) // 2 if hop is None else int(hop))
        self.combine, self.trim = combine, int(trim)
        self.hi, self.lo = float(threshold), lo
        self.median, self.min_gap, self.min_len = int(median), int(min_gap), int(min_len)
        self.mean = None if mean is None else torch.as_tensor(mean, dtype=torch.float64)      # numpy or device tensors
        self.std = None if std is None else torch.as_tensor(std, dtype=torch.float64)
        self.sr, self.hop_length, self.max_batch = int(sr), int(hop_length), int(max_batch)
        plan_windows(4 * self.seq_len, model.time_factor, self.seq_len, self.hop, self.trim)     # validate the grid now
        self.max_events = 256                   # grows to the largest count seen
        self._zlab = None                       # zero label column for sed_window_batch (it requires one)
        self._dws = None

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

    # ── the whole path ──
    def __call__(self, waveform):
        """mono PCM (1-D tensor / ndarray) -> DetectionResult.  The log-mel front end is ``feature.mbe(..., mean, std)``."""
        self._check_model()
        if self.model.in_channels != 1:
            raise ValueError(f"a mono waveform feeds a 1-channel net; this one has {self.model.in_channels} (use from_features)")
        y = torch.as_tensor(waveform)
        if y.dim() != 1:
            raise ValueError(f"expected a mono 1-D waveform, got shape {tuple(y.shape)}")
        dev = self.model.flat_parameters().device
        with torch.no_grad():
            mel = feature.mbe(y.to(dev, torch.float32), sr=self.sr, hop=self.hop_length, n_mels=self.model.n_mels,
                              mean=self.mean, std=self.std)
        return self.from_features(mel)

    def from_features(self, mel):
        """Scaled features [N, C*F] (the .npz cache layout; channel c = columns [c*F, (c+1)*F)) -> DetectionResult."""
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
        """Every window of the plan through the eval forward -> logits [n_win, win_out, K].  Chunks of at most max_batch
        windows: each is gathered by one sed_window_batch launch into a buffer of max_batch windows (memory is bounded by
        max_batch, not by the recording's length) and run on ONE workspace, the largest chunk's (the eval forward of a batch
        equals that of its chunks bit for bit).  ``marks`` (optional list): receives ("gather" | "forward", start, end)
        hip event pairs around every launch, for per-phase timing."""
        m, N = self.model, plan.n_frames
        self._check_model()
        dev = mel.device
        if self._zlab is None or self._zlab.numel() < N or self._zlab.device != dev:
            self._zlab = torch.zeros(max(N, 1 << 16), device=dev)
        Lw, nw = plan.win_len, plan.n_win
        bmax = min(self.max_batch, nw)
        starts = torch.tensor(plan.starts, dtype=torch.int32).to(dev, non_blocking=True)
        x = torch.empty(bmax, m.in_channels, m.n_mels, Lw, device=dev)
        y = torch.empty(bmax, device=dev)                      # the pooled zero labels: pool = Lw -> one per window
        m._check_input(x[:1])
        logits = torch.empty(nw, plan.win_out, m.dense[-1], device=dev)
        P, _ = m._param_structs()
        cfg = m._cfg(bmax, Lw, training=False)
        ws = m._workspace(cfg, False)
        cap = ws.numel() * 4

        def mark(name, fn):
            if marks is None:
                return fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            marks.append((name, a, b))

        for b0 in range(0, nw, bmax):
            b = min(bmax, nw - b0)
            if b != cfg.B:
                cfg = m._cfg(b, Lw, training=False)
                if lib().sed_net_workspace_bytes(C.byref(cfg), 0) > cap:
                    check(-1, "sed_net_workspace_bytes (a smaller chunk needs a larger workspace)")
            mark("gather", lambda: check(lib().sed_window_batch(
                ptr(mel), ptr(self._zlab), N, m.in_channels, m.n_mels, 1, ptr(starts[b0:b0 + b]), None, None, 0, 0, 0,
                ptr(x), ptr(y), b, Lw, Lw, stream_ptr()), "sed_window_batch"))
            mark("forward", lambda: check(lib().sed_net_forward(
                C.byref(cfg), C.byref(P), ptr(x), ptr(logits[b0:b0 + b]), ptr(ws), 0, 0, None, stream_ptr()), "sed_net_forward"))
        return logits

    def stitch(self, logits, plan):
        """window logits -> probs [n_out, K] (sigmoid, then mean / max over the covering windows)."""
        K = logits.shape[2]
        probs = torch.empty(plan.n_out, K, device=logits.device)
        check(lib().sed_detect_stitch(ptr(logits), plan.n_win, plan.win_out, K, plan.hop_out, plan.last_start_out,
                                      plan.n_out, {"mean": 0, "max": 1}[self.combine], self.trim, ptr(probs), stream_ptr()),
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
        while True:
            cap = self.max_events
            out = {n: torch.empty(cap, dtype=torch.float32 if n == "peak" else torch.int32, device=dev) for n in _EVENT_KEYS}
            check(lib().sed_detect_events(ptr(probs), n_out, K, self.median, self.lo, self.hi, self.min_gap, self.min_len,
                                          cap, ptr(self._dws), self._dws.numel(), *(ptr(out[n]) for n in _EVENT_KEYS),
                                          ptr(count), stream_ptr()), "sed_detect_events")
            n = int(count.item())
            if n <= cap:
                return {k: v[:n] for k, v in out.items()}
            self.max_events = n


def detect_events(model, x, **kw):
    """One shot: ``EventDetector(model, **kw)`` on a mono waveform (1-D) or on scaled features [N, C*F] (2-D)."""
    det = EventDetector(model, **kw)
    return det(x) if torch.as_tensor(x).dim() == 1 else det.from_features(x)
