"""Score detected events against annotations and tune the event decoder on the device.

All positions are OUTPUT frames local to a recording, offsets exclusive, exactly as ``DetectionResult.events`` has them.

Reference events: per (recording r, class k) a list of ``[onset, offset)`` that is sorted and pairwise disjoint (touching is
fine: ``onset[j] >= offset[j-1]``), with ``offset > onset >= 0`` and ``offset <= n_out[r]``.  System events of a setting: what
``sed_detect_events_batch`` produces for ``(median, lo, hi, min_gap, min_len)`` on the same packed track.

Event-based matching, per (r, k): the system events in order, each matched to the first not-yet-matched reference event ``j``
with ``|onset - ref.onset[j]| <= collar`` and, unless scoring is onset-only, ``|offset - ref.offset[j]| <= tol[j]`` where
``tol[j] = max(offset_collar, floor(offset_percent * (ref.offset[j] - ref.onset[j])))`` (float64 on the host, then int).
Segment-based counts, per (r, k): blocks of ``block`` output frames from the recording's frame 0, ``ceil(n_out / block)`` of
them (the partial last block is kept, blocks never straddle recordings); a block is active on a side when one of that side's
events covers one of its frames.

``counts`` [G, K, 6] int64 = (ev_tp, n_sys, n_ref, seg_tp, seg_sys, seg_ref) summed over recordings: integers, so exact and
repeatable.  The sweep is one ``sed_tune_sweep`` call per slice of the grid: no event is written, nothing is read back.

The polyphonic sound detection score (the last section of this module) judges the same system events by how much of
them intersects the reference instead of by a collar, over a sweep of thresholds: ``psds_sweep`` is one ``sed_psds_sweep``
call per slice, ``PSDSResult`` the float64 score on its integer counts."""
import ctypes as C
import itertools

import numpy as np
import torch

from ._lib import SedHipError, TuneSetting, check, lib, ptr, stream_ptr
from .metrics import eps

COUNT_NAMES = ("ev_tp", "n_sys", "n_ref", "seg_tp", "seg_sys", "seg_ref")
_SETTING_KEYS = ("threshold", "low", "median", "min_gap", "min_len")


# ───────────────────────── reference events ─────────────────────────
class ReferenceEvents:
    """Annotated events of R recordings with K classes: the host copy (``off`` [R*K + 1] CSR over (r, k), ``onset`` /
    ``offset`` int32) and, on demand, the packed device form ``sed_tune_sweep`` reads.  Build one with ``from_labels``,
    ``from_labels_out``, ``from_intervals`` or ``from_events``; every constructor validates (module docstring) and a
    ValueError names the first offending (recording, class, event)."""

    def __init__(self, per_rk, n_out, K):
        """``per_rk[r][k]`` = list of (onset, offset) in the order given; ``n_out`` [R] output frames per recording"""
        K = int(K)
        n_out = [int(n) for n in n_out]
        if not 1 <= K <= 32:
            raise ValueError(f"K={K} classes: event scoring handles 1..32 classes")
        if len(per_rk) != len(n_out):
            raise ValueError(f"{len(per_rk)} recordings of events but {len(n_out)} lengths")
        off, on_, off_ = [0], [], []
        for r, rec in enumerate(per_rk):
            if n_out[r] < 1:
                raise ValueError(f"recording {r} has {n_out[r]} output frames")
            if len(rec) != K:
                raise ValueError(f"recording {r}: events of {len(rec)} classes, expected {K}")
            for k, evs in enumerate(rec):
                last = 0
                for j, (a, b) in enumerate(evs):
                    a, b = int(a), int(b)
                    where = f"recording {r}, class {k}, event {j}"
                    if a < 0 or b <= a:
                        raise ValueError(f"{where}: [{a}, {b}) is not an interval with offset > onset >= 0")
                    if b > n_out[r]:
                        raise ValueError(f"{where}: [{a}, {b}) ends past the recording's {n_out[r]} output frames")
                    if j and a < last:
                        raise ValueError(f"{where}: [{a}, {b}) overlaps or precedes the previous event, which ends at {last} "
                                         "(events must be sorted and disjoint)")
                    last = b
                    on_.append(a)
                    off_.append(b)
                off.append(len(on_))
        self.R, self.K, self.n_out = len(n_out), K, tuple(n_out)
        self.off = np.asarray(off, np.int32)
        self.onset = np.asarray(on_, np.int32)
        self.offset = np.asarray(off_, np.int32)
        self._dev = {}

    def __len__(self):
        return int(self.onset.size)

    def events(self, r, k):
        """[(onset, offset), ...] of recording r, class k (host)"""
        a, b = self.off[r * self.K + k], self.off[r * self.K + k + 1]
        return list(zip(self.onset[a:b].tolist(), self.offset[a:b].tolist()))

    def select(self, recordings):
        """the reference of the listed recordings, in that order"""
        return ReferenceEvents([[self.events(r, k) for k in range(self.K)] for r in recordings],
                               [self.n_out[r] for r in recordings], self.K)

    def tolerances(self, offset_collar=None, offset_percent=None):
        """``ref_tol`` int32 [n_ref]: -1 everywhere for onset-only scoring (both None), otherwise
        max(offset_collar, floor(offset_percent * length)) in float64, then int"""
        if offset_collar is None and offset_percent is None:
            return np.full(self.onset.size, -1, np.int32)
        oc = 0 if offset_collar is None else int(offset_collar)
        pc = 0.0 if offset_percent is None else float(offset_percent)
        if oc < 0 or not pc >= 0.0:
            raise ValueError(f"offset_collar={offset_collar} and offset_percent={offset_percent} must not be negative")
        length = (self.offset.astype(np.int64) - self.onset).astype(np.float64)
        tol = np.maximum(np.int64(oc), np.floor(np.float64(pc) * length).astype(np.int64))
        return np.minimum(tol, 2 ** 31 - 1).astype(np.int32)

    def device(self, dev):
        """(ref_off, ref_onset, ref_offset) int32 tensors on ``dev`` (cached; never empty: the entry takes no NULL)"""
        key = str(dev)
        if key not in self._dev:
            pad = lambda a: torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, np.int32))).to(dev)  # noqa: E731
            self._dev[key] = (pad(self.off), pad(self.onset), pad(self.offset))
        return self._dev[key]

    def device_tolerances(self, dev, offset_collar=None, offset_percent=None, tol=None):
        """``tolerances(...)`` as an int32 tensor on ``dev``, cached per (device, offset_collar, offset_percent)"""
        key = (str(dev), offset_collar, offset_percent)
        if key not in self._dev:
            tol = self.tolerances(offset_collar, offset_percent) if tol is None else tol
            self._dev[key] = torch.from_numpy(tol if tol.size else np.zeros(1, np.int32)).to(dev)
        return self._dev[key]

    # ── constructors ──
    @classmethod
    def from_events(cls, events, n_out, K):
        """``events[r]`` = iterable of (class, onset, offset) in output frames.  Events keep their given order within a class:
        unsorted or overlapping ones are refused, not repaired."""
        per = []
        for r, evs in enumerate(events):
            rec = [[] for _ in range(int(K))]
            for j, (k, a, b) in enumerate(evs):
                if not 0 <= int(k) < int(K):
                    raise ValueError(f"recording {r}, event {j}: class {k} outside 0..{int(K) - 1}")
                rec[int(k)].append((a, b))
            per.append(rec)
        return cls(per, n_out, K)

    @classmethod
    def from_result(cls, result):
        """the detected events of a ``BatchDetectionResult`` / ``DetectionResult`` as a reference (one host read)"""
        probs, out_off = _track(result)
        batch = hasattr(result, "event_offsets")
        ev = {n: result.events[n].cpu().numpy() for n in (("rec",) if batch else ()) + ("cls", "onset", "offset")}
        rec = ev["rec"] if batch else np.zeros(ev["cls"].size, np.int64)
        R = len(out_off) - 1
        per = [[] for _ in range(R)]
        for r, k, a, b in zip(rec, ev["cls"], ev["onset"], ev["offset"]):
            per[int(r)].append((int(k), int(a), int(b)))
        return cls.from_events(per, np.diff(out_off), probs.shape[1])

    @classmethod
    def from_labels_out(cls, labels):
        """a list of [n_out_r, K] 0/1 labels at OUTPUT frame rate: every run of non-zero frames of a class is one event"""
        per, n_out, K = [], [], None
        for r, lab in enumerate(labels):
            lab = np.asarray(lab.cpu() if hasattr(lab, "cpu") else lab)
            if lab.ndim != 2 or (K is not None and lab.shape[1] != K):
                raise ValueError(f"recording {r}: expected labels [n_out, {K if K is not None else 'K'}], got {lab.shape}")
            K = lab.shape[1]
            on = np.zeros((lab.shape[0] + 2, K), np.int8)
            on[1:-1] = lab != 0
            d = np.diff(on, axis=0)
            per.append([list(zip(np.flatnonzero(d[:, k] == 1).tolist(), np.flatnonzero(d[:, k] == -1).tolist()))
                        for k in range(K)])
            n_out.append(lab.shape[0])
        if K is None:
            raise ValueError("no recordings")
        return cls(per, n_out, K)

    @classmethod
    def from_labels(cls, labels, tf):
        """a list of [N_r, K] 0/1 labels at FEATURE frame rate and the net's time factor: the max over each group of ``tf``
        frames (the ragged tail is dropped, like the pooling does), then ``from_labels_out``"""
        tf = int(tf)
        if tf < 1:
            raise ValueError(f"tf={tf} must be >= 1")
        pooled = []
        for r, lab in enumerate(labels):
            lab = np.asarray(lab.cpu() if hasattr(lab, "cpu") else lab)
            if lab.ndim != 2:
                raise ValueError(f"recording {r}: expected labels [N, K], got {lab.shape}")
            n = lab.shape[0] // tf
            if n < 1:
                raise ValueError(f"recording {r}: {lab.shape[0]} frames are shorter than one output frame ({tf} input frames)")
            pooled.append((lab[:n * tf] != 0).reshape(n, tf, lab.shape[1]).max(1))
        return cls.from_labels_out(pooled)

    @classmethod
    def from_intervals(cls, intervals, frame_seconds, n_out, K=None):
        """``intervals[r]`` = [(class, start_s, end_s), ...] in seconds; ``frame_seconds`` per output frame
        (``EventDetector.frame_seconds``).  onset = floor(start / frame_seconds), offset = ceil(end / frame_seconds) clipped to
        ``n_out[r]``; touching or overlapping intervals of one class are merged.  ``K`` defaults to the largest class + 1."""
        fs = float(frame_seconds)
        if not fs > 0:
            raise ValueError(f"frame_seconds={frame_seconds} must be positive")
        intervals = [list(x) for x in intervals]
        if K is None:
            K = 1 + max((int(k) for rec in intervals for k, _, _ in rec), default=0)
        if len(intervals) != len(n_out):
            raise ValueError(f"{len(intervals)} recordings of intervals but {len(n_out)} lengths")
        per = []
        for r, rec in enumerate(intervals):
            by_k = [[] for _ in range(int(K))]
            for j, (k, s, e) in enumerate(rec):
                if not 0 <= int(k) < int(K):
                    raise ValueError(f"recording {r}, interval {j}: class {k} outside 0..{int(K) - 1}")
                a, b = int(np.floor(np.float64(s) / fs)), min(int(np.ceil(np.float64(e) / fs)), int(n_out[r]))
                by_k[int(k)].append((a, b))
            merged = []
            for evs in by_k:
                out = []
                for a, b in sorted(evs):
                    if out and a <= out[-1][1]:
                        out[-1] = (out[-1][0], max(out[-1][1], b))
                    else:
                        out.append((a, b))
                merged.append(out)
            per.append(merged)
        return cls(per, n_out, K)


# ───────────────────────── the grid of decoder settings ─────────────────────────
class DecoderGrid:
    """Decoder settings to sweep.  The Cartesian product in a FIXED order — ``threshold`` slowest, then ``low``, ``median``,
    ``min_gap``, ``min_len`` fastest — with the combinations ``low > threshold`` dropped; ``low=None`` means lo = hi.
    ``len(grid)`` settings; ``grid[g]`` is a dict usable as ``EventDetector`` keyword arguments (and ``with_decoder``)."""

    def __init__(self, threshold, low=None, median=(1,), min_gap=(0,), min_len=(1,)):
        lows = [None] if low is None else list(low)
        sets = []
        for hi, lo, m, gap, ml in itertools.product(list(threshold), lows, list(median), list(min_gap), list(min_len)):
            lo = hi if lo is None else lo
            if float(lo) > float(hi):
                continue
            sets.append(dict(threshold=float(hi), low=float(lo), median=int(m), min_gap=int(gap), min_len=int(ml)))
        self._init(sets)

    def _init(self, sets):
        for g, s in enumerate(sets):
            if not (1 <= s["median"] <= 31 and s["median"] % 2 == 1):
                raise ValueError(f"setting {g}: median must be odd, 1..31, got {s['median']}")
            if s["min_gap"] < 0 or s["min_len"] < 1:
                raise ValueError(f"setting {g}: need min_gap >= 0 and min_len >= 1, got {s['min_gap']}, {s['min_len']}")
            if not s["low"] <= s["threshold"]:
                raise ValueError(f"setting {g}: low={s['low']} must not exceed threshold={s['threshold']}")
        self.settings = tuple(sets)

    @classmethod
    def from_settings(cls, settings):
        """an explicit list of dicts (keys ``threshold``, and optionally ``low`` (None = threshold), ``median``, ``min_gap``,
        ``min_len`` with EventDetector's defaults), kept in the given order"""
        sets = []
        for g, s in enumerate(settings):
            extra = set(s) - set(_SETTING_KEYS)
            if extra or "threshold" not in s:
                raise ValueError(f"setting {g}: keys must be 'threshold' and any of {_SETTING_KEYS[1:]}, got {sorted(s)}")
            hi = float(s["threshold"])
            lo = s.get("low")
            sets.append(dict(threshold=hi, low=hi if lo is None else float(lo), median=int(s.get("median", 1)),
                             min_gap=int(s.get("min_gap", 0)), min_len=int(s.get("min_len", 1))))
        grid = cls.__new__(cls)
        grid._init(sets)
        return grid

    def __len__(self):
        return len(self.settings)

    def __getitem__(self, g):
        return dict(self.settings[g])

    def __iter__(self):
        return (dict(s) for s in self.settings)

    @staticmethod
    def track_keys(s):
        """the bit tracks a setting reads: (median, float32 threshold value) of lo and of hi"""
        return (s["median"], float(np.float32(s["low"]))), (s["median"], float(np.float32(s["threshold"])))

    def n_tracks(self, g0=0, g1=None):
        """distinct bit tracks of settings [g0, g1): what the workspace of a slice grows with"""
        return len({t for s in self.settings[g0:g1] for t in self.track_keys(s)})


# ───────────────────────── the result ─────────────────────────
def _f1(tp, nref, nsys):
    tp, nref, nsys = (np.asarray(x, np.float64) for x in (tp, nref, nsys))
    prec, rec = tp / (nsys + eps), tp / (nref + eps)
    return 2 * prec * rec / (prec + rec + eps)


class SweepResult:
    """``counts`` [G, K, 6] int64 on the device (COUNT_NAMES); ``table()`` is the one host read (cached).  The scores are the
    float64 formulas and ``eps`` of ``metrics.py`` on those integers: each gives (class-wise [G, K], micro [G])."""

    def __init__(self, counts, grid, collar, block, n_slices=1, n_tracks=0, workspace_bytes=0):
        self.counts, self.grid, self.collar, self.block = counts, grid, collar, block
        self.n_slices, self.n_tracks, self.workspace_bytes = n_slices, n_tracks, workspace_bytes
        self._table = None

    def __len__(self):
        return len(self.grid)

    def table(self):
        if self._table is None:
            self._table = self.counts.cpu().numpy()
        return self._table

    def f1_event(self):
        t = self.table()
        s = t.sum(1)
        return _f1(t[..., 0], t[..., 2], t[..., 1]), _f1(s[:, 0], s[:, 2], s[:, 1])

    def f1_segment(self):
        t = self.table()
        s = t.sum(1)
        return _f1(t[..., 3], t[..., 5], t[..., 4]), _f1(s[:, 3], s[:, 5], s[:, 4])

    def er_segment(self):
        """class-wise (FN_k + FP_k) / seg_ref_k and its micro sum (no zero-reference guard, like metrics.py)"""
        t = self.table().astype(np.float64)
        err = (t[..., 5] - t[..., 3]) + (t[..., 4] - t[..., 3])
        with np.errstate(divide="ignore", invalid="ignore"):
            return err / t[..., 5], err.sum(1) / t[..., 5].sum(1)

    def best(self, metric="f1_event", average="micro"):
        """(g, settings dict, score) of the best setting: highest F1 / lowest ER, ties broken by the lowest g.
        ``average`` "micro" (from the class-summed counts) or "macro" (mean of the class-wise values)."""
        if metric not in ("f1_event", "f1_segment", "er_segment"):
            raise ValueError(f"metric must be 'f1_event', 'f1_segment' or 'er_segment', got {metric!r}")
        if average not in ("micro", "macro"):
            raise ValueError(f"average must be 'micro' or 'macro', got {average!r}")
        if len(self.grid) == 0:
            raise ValueError("an empty grid has no best setting")
        cw, micro = getattr(self, metric)()
        v = micro if average == "micro" else cw.mean(1)
        if metric == "er_segment":
            g = int(np.argmin(np.where(np.isnan(v), np.inf, v)))
        else:
            g = int(np.argmax(v))
        return g, self.grid[g], float(v[g])


    def best_per_class(self, metric="f1_event"):
        """(g [K] int array, settings dict of K-lists, scores [K]): for every class the setting with its highest class-wise
        F1 / lowest class-wise ER, ties broken by the lowest g.  A NaN ER (a class without reference) counts as +inf, so such a
        class takes g = 0.  The dict is what ``EventDetector.with_decoder`` takes to build the class-wise detector."""
        if metric not in ("f1_event", "f1_segment", "er_segment"):
            raise ValueError(f"metric must be 'f1_event', 'f1_segment' or 'er_segment', got {metric!r}")
        if len(self.grid) == 0:
            raise ValueError("an empty grid has no best setting")
        cw, _ = getattr(self, metric)()
        if metric == "er_segment":
            g = np.argmin(np.where(np.isnan(cw), np.inf, cw), axis=0)
        else:
            g = np.argmax(cw, axis=0)
        sets = [self.grid[int(i)] for i in g]
        return g, {n: [s[n] for s in sets] for n in _SETTING_KEYS}, cw[g, np.arange(cw.shape[1])]


# ───────────────────────── the sweep ─────────────────────────
def _track(track):
    """BatchDetectionResult | DetectionResult | (probs, out_offsets) -> (probs [n_total, K], out_offsets list [R+1])"""
    if hasattr(track, "out_offsets"):
        return track.probs, list(track.out_offsets)
    if hasattr(track, "probs"):
        return track.probs, [0, int(track.probs.shape[0])]
    probs, out_off = track
    return probs, [int(o) for o in out_off]


# what sweep and psds_sweep share: the checks of their three arguments, the device requirement, the slicing of the grid by
# workspace, the workspace itself and the settings as the entries take them
def _checked_types(track, ref, grid):
    """-> (probs, out_off) of ``_track`` once ref, grid and the track have the right types"""
    probs, out_off = _track(track)
    if not isinstance(ref, ReferenceEvents):
        raise TypeError(f"ref must be a ReferenceEvents, got {type(ref).__name__}")
    if not isinstance(grid, DecoderGrid):
        raise TypeError(f"grid must be a DecoderGrid, got {type(grid).__name__}")
    if not (torch.is_tensor(probs) and probs.dim() == 2):
        raise ValueError("the track must be a [n_total, K] tensor of probabilities")
    return probs, out_off


def _checked_sizes(probs, out_off, ref):
    """-> (n_out int64 [R], R, K) once the reference fits the track recording by recording"""
    n_out = np.ascontiguousarray(np.diff(np.asarray(out_off, dtype=np.int64)))
    R, K = n_out.size, int(probs.shape[1])
    if out_off[0] != 0 or out_off[-1] != probs.shape[0]:
        raise ValueError(f"out_offsets run from {out_off[0]} to {out_off[-1]}, the track has {probs.shape[0]} rows")
    if ref.R != R or ref.K != K:
        raise ValueError(f"the reference has {ref.R} recordings of {ref.K} classes, the track {R} of {K}")
    for r in range(R):
        if ref.n_out[r] != int(n_out[r]):
            raise ValueError(f"recording {r}: the reference was built for {ref.n_out[r]} output frames, the track has {int(n_out[r])}")
    return n_out, R, K


def _on_gpu(probs):
    if not probs.is_cuda:
        raise SedHipError("sed_crnn_amd: the track must be on the GPU; there is no CPU fallback")
    return probs.contiguous().float()


def _grid_slices(grid, n_total, K, R, max_workspace_bytes, bytes_fn, fn_name):
    """consecutive slices [(g0, g1, workspace bytes, bit tracks)] of the grid that fit the budget; ``bytes_fn(n_total, K, R,
    n_tracks, G)`` is the entry's size query"""
    G = len(grid)
    slices, g0 = [], 0
    while g0 < G:
        rest = grid.n_tracks(g0, G)                                   # the usual case: everything that is left fits, one query
        b = bytes_fn(n_total, K, R, rest, G - g0)
        if 0 < b <= max_workspace_bytes and (G - g0) * K * R < 2 ** 31:
            slices.append((g0, G, b, rest))
            break
        keys, g1, need = set(), g0, 0
        while g1 < G:
            k2 = keys.union(grid.track_keys(grid.settings[g1]))
            b = bytes_fn(n_total, K, R, len(k2), g1 + 1 - g0)
            if b == 0 and g1 == g0:
                raise ValueError(f"{fn_name} refuses {n_total} output frames of {K} classes in {R} recordings")
            if b == 0 or b > max_workspace_bytes or (g1 + 1 - g0) * K * R >= 2 ** 31:
                break
            keys, need, g1 = k2, b, g1 + 1
        if g1 == g0:
            raise ValueError(f"max_workspace_bytes={max_workspace_bytes} does not hold a single setting "
                             f"({bytes_fn(n_total, K, R, len(k2), 1)} bytes)")
        slices.append((g0, g1, need, len(keys)))
        g0 = g1
    return slices


def _workspace(slices, cache, dev):
    """-> (uint8 tensor that holds the largest slice, its size); ``cache``: a dict that keeps it between calls"""
    need = max(s[2] for s in slices)
    cache = {} if cache is None else cache
    ws = cache.get("ws")
    if ws is None or ws.numel() < need or ws.device != dev:
        ws = cache["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
    return ws, need


def _settings_array(grid, a, b):
    return (TuneSetting * (b - a))(*[TuneSetting(s["median"], s["low"], s["threshold"], s["min_gap"], s["min_len"])
                                     for s in grid.settings[a:b]])


def sweep(track, ref, grid, collar=1, offset_collar=None, offset_percent=None, block=1, max_workspace_bytes=1 << 30, cache=None):
    """Score every setting of ``grid`` on a packed track against ``ref`` (module docstring) -> SweepResult.  The grid is split
    into consecutive slices whose workspace (it grows with the number of distinct bit tracks) fits ``max_workspace_bytes``; each
    slice writes its own rows of ``counts``, so the result does not depend on the split.  ``cache``: a dict that keeps the
    workspace between calls."""
    probs, out_off = _checked_types(track, ref, grid)
    if not 0 <= int(collar) <= 31:
        raise ValueError(f"collar must be in 0..31 output frames, got {collar}")
    if int(block) < 1:
        raise ValueError(f"block must be >= 1 output frame, got {block}")
    n_out, R, K = _checked_sizes(probs, out_off, ref)
    tol = ref.tolerances(offset_collar, offset_percent)
    probs = _on_gpu(probs)
    dev = probs.device
    G = len(grid)
    counts = torch.zeros(G, K, 6, dtype=torch.int64, device=dev)
    if G == 0 or R == 0:
        return SweepResult(counts, grid, int(collar), int(block), 0)
    L = lib()
    slices = _grid_slices(grid, int(probs.shape[0]), K, R, max_workspace_bytes, L.sed_tune_workspace_bytes, "sed_tune_workspace_bytes")
    ws, need = _workspace(slices, cache, dev)
    d_off, d_on, d_offs = ref.device(dev)
    d_tol = ref.device_tolerances(dev, offset_collar, offset_percent, tol)
    for a, b, _, _ in slices:
        check(L.sed_tune_sweep(ptr(probs), C.c_void_p(n_out.ctypes.data), R, K, C.cast(_settings_array(grid, a, b), C.c_void_p), b - a,
                               ptr(d_off), ptr(d_on), ptr(d_offs), ptr(d_tol), int(collar), int(block), ptr(ws), ws.numel(),
                               ptr(counts[a:b]), stream_ptr()),
              "sed_tune_sweep")
    return SweepResult(counts, grid, int(collar), int(block), len(slices), max(s[3] for s in slices), need)


def tune_decoder(det, track, ref, grid, metric="f1_event", average="micro", per_class=False, **kw):
    """One shot: ``det.sweep(track, ref, grid, **kw)``, then the detector with the best setting -> (detector, SweepResult).
    ``per_class=True``: every class gets the setting that is best for it (``SweepResult.best_per_class(metric)``) and the
    detector returned is class-wise; ``average`` is then ignored, there is nothing to average."""
    res = det.sweep(track, ref, grid, **kw)
    if per_class:
        return det.with_decoder(**res.best_per_class(metric)[1]), res
    _, best, _ = res.best(metric, average)
    return det.with_decoder(**best), res


# ───────────────────────── PSDS: intersection criteria, threshold-free score ─────────────────────────
PSDS_COUNT_NAMES = ("tp", "n_ref", "n_sys", "fp")


def _milli(value, name, lowest=1):
    """a criterion in 0..1 as integer thousandths; ValueError unless it is a multiple of 0.001 (to within 1e-9) in range"""
    v = float(value)
    if not np.isfinite(v):
        raise ValueError(f"{name}={value} must be a number in {lowest / 1000:g}..1")
    m = int(round(v * 1000.0))
    if not abs(v - m / 1000.0) <= 1e-9:
        raise ValueError(f"{name}={value} must be a multiple of 0.001")
    if not lowest <= m <= 1000:
        raise ValueError(f"{name}={value} must be in {lowest / 1000:g}..1")
    return m


class PSDSCriteria:
    """The intersection criteria and the weights of the polyphonic sound detection score (module section above).
    ``dtc`` / ``gtc`` / ``cttc``: fractions in (0, 1], multiples of 0.001 (the device compares integers in thousandths);
    ``cttc=None``: no cross triggers.  ``alpha_ct`` weighs the cross-trigger rate in the effective false-positive rate,
    ``alpha_st`` the standard deviation across classes; ``e_max`` is the largest effective FPR (per hour) of the area."""

    def __init__(self, dtc=0.7, gtc=0.7, cttc=None, alpha_ct=0.0, alpha_st=1.0, e_max=100.0):
        self.dtc_milli, self.gtc_milli = _milli(dtc, "dtc"), _milli(gtc, "gtc")
        self.cttc_milli = 0 if cttc is None else _milli(cttc, "cttc")
        self.dtc, self.gtc, self.cttc = self.dtc_milli / 1000.0, self.gtc_milli / 1000.0, None if cttc is None else self.cttc_milli / 1000.0
        self.alpha_ct, self.alpha_st, self.e_max = float(alpha_ct), float(alpha_st), float(e_max)
        if not self.alpha_ct >= 0.0 or not self.alpha_st >= 0.0:
            raise ValueError(f"alpha_ct={alpha_ct} and alpha_st={alpha_st} must not be negative")
        if self.alpha_ct > 0.0 and cttc is None:
            raise ValueError(f"alpha_ct={alpha_ct} needs a cross-trigger criterion: give cttc")
        if not (self.e_max > 0.0 and np.isfinite(self.e_max)):
            raise ValueError(f"e_max={e_max} must be positive and finite")

    @classmethod
    def scenario1(cls):
        """DCASE scenario 1: react fast, localise precisely (dtc = gtc = 0.7, no cross triggers, alpha_st = 1, e_max = 100)"""
        return cls(0.7, 0.7, None, 0.0, 1.0, 100.0)

    @classmethod
    def scenario2(cls):
        """DCASE scenario 2: do not confuse classes (dtc = gtc = 0.1, cttc = 0.3, alpha_ct = 0.5, alpha_st = 1, e_max = 100)"""
        return cls(0.1, 0.1, 0.3, 0.5, 1.0, 100.0)

    def __repr__(self):
        return (f"PSDSCriteria(dtc={self.dtc}, gtc={self.gtc}, cttc={self.cttc}, alpha_ct={self.alpha_ct}, alpha_st={self.alpha_st}, "
                f"e_max={self.e_max})")


class PSDSResult:
    """``counts`` [G, K, 4] int64 (PSDS_COUNT_NAMES) and ``ct`` [G, K, K] int64 (row k, column c: cross triggers of detections of
    class k on the reference of class c; zeros without a cross-trigger criterion) on the device; ``table()`` is the one host
    read (cached).  ``total_seconds`` = T, ``class_seconds`` [K] = T_c.  Everything else is float64 on those integers."""

    def __init__(self, counts, ct, grid, criteria, total_seconds, class_seconds, n_slices=1, n_tracks=0, workspace_bytes=0):
        self.counts, self.ct, self.grid, self.criteria = counts, ct, grid, criteria
        self.total_seconds, self.class_seconds = float(total_seconds), np.asarray(class_seconds, np.float64)
        self.n_slices, self.n_tracks, self.workspace_bytes = n_slices, n_tracks, workspace_bytes
        self._table = None

    def __len__(self):
        return len(self.grid)

    def table(self):
        """(counts, ct) as numpy arrays"""
        if self._table is None:
            self._table = (self.counts.cpu().numpy(), self.ct.cpu().numpy())
        return self._table

    def rates(self):
        """(TPR [G, K], FPR [G, K], CTR [G, K, K], eFPR [G, K]): TPR = tp / n_ref (NaN for a class without reference), FPR and
        CTR per hour, eFPR = FPR + alpha_ct · the mean of CTR over the other classes that have reference time"""
        counts, ct = self.table()
        c = counts.astype(np.float64)
        K = c.shape[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            tpr = c[..., 0] / c[..., 1]
            fpr = c[..., 3] / (self.total_seconds / 3600.0)
            ctr = ct.astype(np.float64) / (self.class_seconds / 3600.0)[None, None, :]
        efpr = fpr.copy()
        if self.criteria.cttc_milli and self.criteria.alpha_ct > 0.0:
            for k in range(K):
                others = [c2 for c2 in range(K) if c2 != k and self.class_seconds[c2] > 0.0]
                if others:
                    efpr[:, k] = fpr[:, k] + self.criteria.alpha_ct * ctr[:, k, others].mean(1)
        return tpr, fpr, ctr, efpr

    def kept_classes(self):
        """the classes with a reference event: the ones the score averages over"""
        counts, _ = self.table()
        if counts.shape[0] == 0:
            raise ValueError("an empty grid has no PSDS")
        kept = np.flatnonzero(counts[0, :, 1] > 0)
        if kept.size == 0:
            raise ValueError("no class has a reference event: the PSDS is undefined")
        return kept

    def roc(self, k):
        """class k's ROC as a step function: (e, tpr) with e the sorted distinct eFPR[:, k] and tpr[i] = max TPR[g, k] over the
        settings with eFPR[g, k] <= e[i]"""
        tpr, _, _, efpr = self.rates()
        e = np.unique(efpr[:, k])
        return e, np.array([tpr[efpr[:, k] <= x, k].max() for x in e], np.float64)

    def _steps(self, e, k):
        ek, tk = self.roc(k)
        i = np.searchsorted(ek, e, side="right") - 1
        return np.where(i >= 0, tk[np.maximum(i, 0)], 0.0)

    def curve(self):
        """(e, mean, std, eTPR): the e axis = the sorted distinct eFPR values <= e_max of the kept classes, then e_max; across
        the kept classes the mean and population std of tpr_k(e), and eTPR = mean − alpha_st · std"""
        kept = self.kept_classes()
        efpr = self.rates()[3][:, kept]
        e = np.unique(efpr[efpr <= self.criteria.e_max])
        e = np.concatenate([e, [self.criteria.e_max]])
        per = np.stack([self._steps(e, int(k)) for k in kept])
        mean, std = per.mean(0), per.std(0)
        return e, mean, std, mean - self.criteria.alpha_st * std

    def psds(self):
        """the area under eTPR over [0, e_max], left-constant, 0 before the first point, divided by e_max"""
        e, _, _, etpr = self.curve()
        return float(np.sum(etpr[:-1] * np.diff(e)) / self.criteria.e_max)

    def per_class_auc(self):
        """[K]: the same area under every class's own tpr_k(e) (NaN for a class without reference)"""
        kept = self.kept_classes()
        e = self.curve()[0]
        out = np.full(self.table()[0].shape[1], np.nan)
        for k in kept:
            out[k] = np.sum(self._steps(e, int(k))[:-1] * np.diff(e)) / self.criteria.e_max
        return out


def psds_sweep(track, ref, grid, criteria, frame_seconds, max_workspace_bytes=1 << 30, cache=None):
    """The PSDS counts of every setting of ``grid`` on a packed track against ``ref`` -> PSDSResult: one ``sed_psds_sweep`` call
    per slice of the grid (sliced by workspace exactly like ``sweep``), no event written, nothing read back.  ``track``, ``ref``
    and ``grid`` as in ``sweep``; ``criteria`` a PSDSCriteria; ``frame_seconds`` per output frame turns frames into the hours
    of the rates."""
    probs, out_off = _checked_types(track, ref, grid)
    if not isinstance(criteria, PSDSCriteria):
        raise TypeError(f"criteria must be a PSDSCriteria, got {type(criteria).__name__}")
    fs = float(frame_seconds)
    if not fs > 0:
        raise ValueError(f"frame_seconds={frame_seconds} must be positive")
    n_out, R, K = _checked_sizes(probs, out_off, ref)
    probs = _on_gpu(probs)
    dev = probs.device
    G = len(grid)
    cls_of = np.repeat(np.arange(R * K), np.diff(ref.off)) % K       # the class of every reference event
    class_seconds = np.bincount(cls_of, weights=ref.offset.astype(np.float64) - ref.onset, minlength=K) * fs
    counts = torch.zeros(G, K, 4, dtype=torch.int64, device=dev)
    ct = torch.zeros(G, K, K, dtype=torch.int64, device=dev)
    total = float(n_out.sum()) * fs
    if G == 0 or R == 0:
        return PSDSResult(counts, ct, grid, criteria, total, class_seconds, 0)
    L = lib()
    slices = _grid_slices(grid, int(probs.shape[0]), K, R, max_workspace_bytes, L.sed_psds_workspace_bytes, "sed_psds_workspace_bytes")
    ws, need = _workspace(slices, cache, dev)
    d_off, d_on, d_offs = ref.device(dev)
    for a, b, _, _ in slices:
        check(L.sed_psds_sweep(ptr(probs), C.c_void_p(n_out.ctypes.data), R, K, C.cast(_settings_array(grid, a, b), C.c_void_p), b - a,
                               ptr(d_off), ptr(d_on), ptr(d_offs), criteria.dtc_milli, criteria.gtc_milli, criteria.cttc_milli,
                               ptr(ws), ws.numel(), ptr(counts[a:b]), ptr(ct[a:b]) if criteria.cttc_milli else None, stream_ptr()),
              "sed_psds_sweep")
    return PSDSResult(counts, ct, grid, criteria, total, class_seconds, len(slices), max(s[3] for s in slices), need)
