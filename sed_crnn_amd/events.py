"""device entries over an event table: where every detected event came from (``event_tdoa``, ``event_doa``) and its audio with the
array pointed at it (``event_beamform``, ``event_mvdr``), on planar PCM and, with ``_ring``, on the PCM rings of live feeds that
``ring_write`` fills.  ``feature`` re-exports the public names.

Every function is: check the arguments, describe where the samples are (``_Source``), run.  The TDOA / DOA entries share
``_locate``, the two beams ``_extract``; the C entry of a call comes from ``_ENTRY``."""
import ctypes as C
import functools
import typing

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr
from .feature import GCC_MAX_CHANNELS, HOP, NB_MEL, NFFT, SR, _LM_OFF_ENT, _clip_table, _tables, build_tables, slaney_mel_basis

# (what is computed, on rings) -> the C entry; its workspace function is the name + "_workspace_bytes"
_ENTRY = {("tdoa", False): "sed_event_tdoa", ("tdoa", True): "sed_event_tdoa_ring",
          ("doa", False): "sed_event_doa", ("doa", True): "sed_event_doa_ring",
          ("doa_track", False): "sed_event_doa_track", ("doa_track", True): "sed_event_doa_track_ring",
          ("doa_contrast", False): "sed_event_doa_contrast", ("doa_track_contrast", False): "sed_event_doa_track_contrast",
          ("spans", False): "sed_event_beam_spans", ("spans", True): "sed_event_beam_spans_ring",
          ("delay_sum", False): "sed_event_beamform", ("delay_sum", True): "sed_event_beamform_ring",
          ("mvdr", False): "sed_event_mvdr", ("mvdr", True): "sed_event_mvdr_ring",
          ("mvdr_noise", False): "sed_event_mvdr_noise", ("mvdr_noise", True): "sed_event_mvdr_noise_ring",
          ("mvdr_quiet", False): "sed_event_mvdr_quiet",
          ("mvdr_track", False): "sed_event_mvdr_track", ("mvdr_track", True): "sed_event_mvdr_track_ring",
          ("mvdr_quiet_track", False): "sed_event_mvdr_quiet_track"}
_LOCATED = ("onset", "offset", "peak_frame", "dir", "loc_frames")


class _Source(typing.NamedTuple):
    """where the samples of a call are.  Holds the tensor and the host table that its C arguments point into."""
    x: torch.Tensor              # the planar PCM; ring: the rings
    table: np.ndarray            # int64: (first sample, samples) per recording and channel; ring: the samples every feed has received
    R: int
    nc: int
    ring: bool
    extent: int                  # what bounds an event's frames: the longest recording's samples; ring: cap
    spans_head: list             # the leading C arguments of the spans call, which reads no samples
    head: list                   # ... of every other call


def _pad_code(pad_mode):
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    return {"constant": 0, "reflect": 1}[pad_mode]


def _need_pcm(who, pcm):
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dim() == 1):
        raise RuntimeError(f"sed_crnn_amd.feature.{who} needs a 1-D CUDA(HIP) PCM buffer; there is no CPU fallback")


def _need_ring(who, ring):
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dim() == 1 and ring.dtype == torch.float32 and ring.is_contiguous()):
        raise RuntimeError(f"sed_crnn_amd.feature.{who} needs a contiguous 1-D float32 CUDA(HIP) ring buffer; there is no CPU fallback")


def _beam_sizes(who, channels, time_factor, hop):
    nc, tf, hop = int(channels), int(time_factor), int(hop)
    if not 2 <= nc <= GCC_MAX_CHANNELS or tf < 1 or hop < 1:
        raise ValueError(f"{who} needs 2 to {GCC_MAX_CHANNELS} audio channels, time_factor >= 1 and hop >= 1, got channels={nc}, "
                         f"time_factor={tf}, hop={hop}")
    return nc, tf, hop


def _linear_source(pcm, clips, nc, align_16=False):
    """R >= 1 recordings of ``nc`` planar channels in the buffer ``pcm`` (``clips`` as ``mbe_planar`` takes them); ``align_16``: the
    kernel loads 16 bytes at a time, a view into a larger buffer that starts elsewhere is copied"""
    table = _clip_table(clips, nc, pcm.numel(), at_least_one=True)
    pcm = pcm.contiguous().float()
    if align_16 and pcm.data_ptr() % 16:
        pcm = pcm.clone()
    R = table.shape[0] // nc
    spans_head = [pcm.numel(), C.c_void_p(table.ctypes.data), R, nc]
    return _Source(pcm, table, R, nc, False, int(table[:, 1].max()), spans_head, [ptr(pcm)] + spans_head)


def _ring_source(ring, cap, n, nc, need_16_byte=False):
    """the rings of R live feeds of ``nc`` channels as ``ring_write`` fills them; ``n`` [R] host ints: the samples every feed has
    received"""
    n = np.ascontiguousarray(np.asarray(n, dtype=np.int64).reshape(-1))
    R = n.shape[0]
    if R < 1 or (n < 0).any():
        raise ValueError(f"n must hold one sample count >= 0 per feed, got {n.tolist()[:8]}")
    if cap < NFFT or cap % 4 or R * nc * cap > ring.numel() or (need_16_byte and ring.data_ptr() % 16):
        raise ValueError(f"{R} feeds of {nc} rings of cap={cap} samples (a multiple of 4, at least {NFFT}, 16-byte aligned) do not fit the "
                         f"ring buffer of {ring.numel()} samples" if need_16_byte else
                         f"{R} feeds of {nc} rings of cap={cap} samples (a multiple of 4, at least {NFFT}) do not fit the ring buffer of "
                         f"{ring.numel()} samples")
    spans_head = [C.c_void_p(n.ctypes.data), R, nc]
    return _Source(ring, n, R, nc, True, cap, spans_head, [ptr(ring), ring.numel(), cap] + spans_head)


def _event_cols(events, R, rec_key, keys, dev):
    """the columns ``keys`` of ``events`` as contiguous int32 tensors on ``dev``, equally long, and with more than one recording
    the column ``rec_key`` that names an event's -> ({key: tensor}, the recording under "rec"; E)"""
    col = {}
    for k in keys + ((rec_key,) if R > 1 else ()):
        if k not in events:
            raise ValueError(f"events has no {k!r}" + (f" ({R} recordings need one)" if k == rec_key else
                                                       " (the events must be located: feature.event_doa)" if k in ("dir", "loc_frames") else ""))
        col["rec" if k == rec_key else k] = events[k].to(dev, torch.int32).contiguous()
    E = col["onset"].numel()
    if any(v.dim() != 1 or v.numel() != E for v in col.values()):
        raise ValueError("the event columns must be 1-D and equally long")
    return col, E


def _cols(src, events, keys):
    """``_event_cols`` for a source: the recording of an event is its ``rec`` column; on rings ``stream`` will do"""
    rec_key = "stream" if src.ring and "stream" in events and "rec" not in events else "rec"
    return _event_cols(events, src.R, rec_key, keys, src.x.device)


def _col_ptrs(col, keys):
    return [ptr(col.get("rec"))] + [ptr(col[k]) for k in keys]


# ───────────────────────── where an event came from: TDOA and DOA ─────────────────────────
def _doa_plan(doa, nc, sr):
    """checks the settings of a DOA call (a ``localize.DOA`` for ``nc`` channels) -> its max_lag at rate ``sr``"""
    from .localize import DOA
    if not isinstance(doa, DOA):
        raise TypeError(f"event_doa takes the settings as a sed.DOA(...) object, got {type(doa).__name__}")
    if doa.channels != nc:
        raise ValueError(f"the DOA settings hold {doa.channels} microphone positions, the audio has {nc} channels")
    return doa.plan(sr)[0]


def _doa_io(doa, sr, E, dev, out, return_map):
    """the steering tables of ``doa`` at rate ``sr`` on ``dev`` (uploaded once per device and rate) and, added to ``out``, the
    outputs a DOA call adds -> [J, D, Q, trig, dir, doa_power, srp or None] as the C entries take them (None without events)"""
    _, J, trig = doa.plan(sr)
    out["dir"] = torch.empty(E, dtype=torch.int32, device=dev)
    out["doa_power"] = torch.empty(E, device=dev)
    if return_map:
        out["srp"] = torch.empty(E, J.shape[0], device=dev)
    if E == 0:
        return None
    key = (dev.index or 0, float(sr))
    if key not in doa._device:
        doa._device[key] = (torch.from_numpy(J).to(dev), torch.from_numpy(trig).to(dev))
    Jd, td = doa._device[key]
    return [ptr(Jd), J.shape[0], doa.oversample, ptr(td), ptr(out["dir"]), ptr(out["doa_power"]), ptr(out.get("srp"))]


def _track_io(doa, E, dev, out, return_map):
    """the outputs a track call adds, added to ``out``, and the neighbour table of ``doa`` on ``dev`` (uploaded once per
    device and step) -> [block_chunks, nbr_off, nbr_idx, trk_len, trk_raw, trk_dir, trk_power, trk_map or None] (None without events)"""
    trk = doa.track
    Tm, D = trk.max_blocks(doa.max_frames), len(doa.grid)
    out["trk_len"] = torch.empty(E, dtype=torch.int32, device=dev)
    out["trk_raw"] = torch.empty(E, Tm, dtype=torch.int32, device=dev)
    out["trk_dir"] = torch.empty(E, Tm, dtype=torch.int32, device=dev)
    out["trk_power"] = torch.empty(E, Tm, device=dev)
    if return_map:
        out["trk_map"] = torch.empty(E, Tm, D, device=dev)
    if E == 0:
        return None
    nbr = [None, None]
    if trk.max_step_deg is not None:
        key = (dev.index or 0, trk.max_step_deg)
        if key not in doa._neighbours_device:
            doa._neighbours_device[key] = tuple(torch.from_numpy(a).to(dev) for a in doa.neighbours())
        nbr = doa._neighbours_device[key]
    return [trk.block_chunks, ptr(nbr[0]), ptr(nbr[1]), ptr(out["trk_len"]), ptr(out["trk_raw"]), ptr(out["trk_dir"]), ptr(out["trk_power"]),
            ptr(out.get("trk_map"))]


def _n_classes(who, settings, n_classes, most):
    """the class count of a call that reads the activity mask, checked; ``settings``: what asks for it"""
    if n_classes is None:
        raise ValueError(f"{who} with {settings} needs n_classes, the number of classes the events' cls column counts in")
    if isinstance(n_classes, bool) or int(n_classes) != n_classes or not 1 <= int(n_classes) <= most:
        raise ValueError(f"{who}: n_classes must be an integer in [1, {most}] (an activity word has {most} bits), got {n_classes!r}")
    return int(n_classes)


def _contrast_classes(who, n_classes):
    from .localize import CONTRAST_MAX_CLASSES
    return _n_classes(who, "sed.DOA(..., contrast=sed.Contrast(...))", n_classes, CONTRAST_MAX_CLASSES)


def _mask_frames(table, nc, tf, hop):
    """the words of the activity mask of a clip table: ``n_r // (tf hop) + 1`` output frames per recording"""
    return int((table[::nc, 1] // (tf * hop) + 1).sum())


def _frames_only(who, clips, nc, events, keys):
    """the selection-only entries' prologue: the event columns must be on the GPU, the clip table is checked without a PCM buffer
    -> (the device, the table, R, the columns ``keys`` and ``cls``, E, the PCM extent the C entry takes)"""
    dev = events["onset"].device if isinstance(events.get("onset"), torch.Tensor) else None
    if dev is None or dev.type != "cuda":
        raise RuntimeError(f"sed_crnn_amd.feature.{who} needs the event columns as CUDA(HIP) tensors; there is no CPU fallback")
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    table = _clip_table(clips, nc, int((table[:, 0] + table[:, 1]).max()) if table.size else 0, at_least_one=True)
    R = table.shape[0] // nc
    col, E = _event_cols(events, R, "rec", keys + ("cls",), dev)
    return dev, table, R, col, E, int((table[:, 0] + table[:, 1]).max())


def _locate(src, events, tf, hop, max_lag, max_frames, settings, return_curve, max_workspace_bytes, doa, n_classes=None):
    """what the four TDOA / DOA functions do once their arguments are checked.  ``settings``: what the C entry takes between ``hop``
    and its outputs; ``doa``: None, or (the ``localize.DOA``, the rate of the PCM, return_map) for the same launches and one more
    per slice; with ``doa.contrast`` (linear only) the entry takes the ``cls`` column behind ``rec``, the
    class count and the six settings behind ``settings`` and ``bg_frames`` / ``bg_sel`` behind its outputs"""
    R, nc, dev = src.R, src.nc, src.x.device
    ct = getattr(doa[0], "contrast", None) if doa is not None else None
    classes = _contrast_classes("event_doa", n_classes) if ct is not None else None
    col, E = _cols(src, events, _LOCATED[:3] + (("cls",) if ct is not None else ()))
    P, W = nc * (nc - 1) // 2, 2 * max_lag + 3
    out = {"lag": torch.empty(E, P, device=dev), "strength": torch.empty(E, P, device=dev),
           "loc_frames": torch.empty(E, dtype=torch.int32, device=dev)}
    if return_curve:
        out["acc"] = torch.empty(E, P, W, device=dev)
    extra = _doa_io(doa[0], doa[1], E, dev, out, doa[2]) if doa is not None else []
    track = doa is not None and getattr(doa[0], "track", None) is not None          # a direction per block too
    if track:
        extra = (extra or []) + (_track_io(doa[0], E, dev, out, doa[2]) or [])
    if ct is not None:
        out["bg_frames"] = torch.zeros(E, dtype=torch.int32, device=dev)
        out["bg_sel"] = torch.full((E, ct.frames), -1, dtype=torch.int32, device=dev)
        extra = (extra or []) + [ptr(out["bg_frames"]), ptr(out["bg_sel"])]
        settings = list(settings) + [classes, ct.frames, ct.search, ct.guard, ct.min_frames, ct.weight]
    if E == 0:
        return out
    tables = _tables(dev.index or 0, SR, NFFT, NB_MEL)                # the window and the twiddles; the mel plan is not read
    kind = "tdoa" if doa is None else ("doa_track" if track else "doa") + ("_contrast" if ct is not None else "")
    sizes = _ENTRY[kind if track or ct is not None else "tdoa", src.ring] + "_workspace_bytes"   # (the steering launch reads the partials in place)
    more = [len(doa[0].grid), doa[0].track.block_chunks, int(doa[0].track.max_step_deg is not None)] if track else []
    if ct is not None:                                                # the mask lies behind the table, once per call
        more += [_mask_frames(src.table, nc, tf, hop), ct.frames]
    need_one = getattr(lib(), sizes)(R, nc, 1, src.extent, hop, max_frames, *more)
    need_all = getattr(lib(), sizes)(R, nc, E, src.extent, hop, max_frames, *more)
    if need_one == 0:
        raise ValueError(f"sed_event_tdoa_ring_workspace_bytes refuses R={R}, channels={nc}, cap={src.extent}, hop={hop}, max_frames={max_frames}"
                         if src.ring else
                         f"sed_event_tdoa_workspace_bytes refuses R={R}, channels={nc}, hop={hop}, max_frames={max_frames}")
    ws = torch.empty(min(need_all, max(need_one, int(max_workspace_bytes))), dtype=torch.uint8, device=dev)
    name = _ENTRY[kind, src.ring]
    cols = _col_ptrs(col, _LOCATED[:3])
    if ct is not None:
        cols = cols[:1] + [ptr(col["cls"])] + cols[1:]
    check(getattr(lib(), name)(*src.head, ptr(tables), tables.numel() * 4, *cols, E, tf, hop, *settings,
                               ptr(out["lag"]), ptr(out["strength"]), ptr(out["loc_frames"]), ptr(out.get("acc")), *extra, ptr(ws),
                               ws.numel(), stream_ptr()), name)
    return out


def _tdoa_linear(pcm, clips, channels, events, time_factor, max_lag, max_frames, hop, pad_mode, return_curve, max_workspace_bytes, doa,
                 n_classes=None):
    """``event_tdoa`` (``doa`` None) and ``event_doa``"""
    from .localize import MAX_LAG_LIMIT
    _need_pcm("event_tdoa", pcm)
    pad = _pad_code(pad_mode)
    nc, tf, max_lag, max_frames, hop = int(channels), int(time_factor), int(max_lag), int(max_frames), int(hop)
    if doa is not None:
        max_lag = _doa_plan(doa[0], nc, doa[1])
    if not 2 <= nc <= GCC_MAX_CHANNELS:
        raise ValueError(f"event_tdoa needs 2 to {GCC_MAX_CHANNELS} audio channels (one estimate per microphone pair), got channels={nc}")
    if not 1 <= max_lag <= MAX_LAG_LIMIT or max_frames < 1 or tf < 1 or hop < 1:
        raise ValueError(f"event_tdoa needs 1 <= max_lag <= {MAX_LAG_LIMIT}, max_frames >= 1, time_factor >= 1 and hop >= 1, got "
                         f"max_lag={max_lag}, max_frames={max_frames}, time_factor={tf}, hop={hop}")
    src = _linear_source(pcm, clips, nc)
    return _locate(src, events, tf, hop, max_lag, max_frames, [pad, max_lag, max_frames], return_curve, max_workspace_bytes, doa, n_classes)


def _tdoa_ring(ring, cap, n, channels, events, time_factor, max_lag, max_frames, hop, lat_frames, history_frames, return_curve,
               max_workspace_bytes, doa):
    """``event_tdoa_ring`` (``doa`` None) and ``event_doa_ring``"""
    from .localize import MAX_LAG_LIMIT
    _need_ring("event_tdoa_ring", ring)
    nc, tf, max_lag, max_frames, hop, cap = int(channels), int(time_factor), int(max_lag), int(max_frames), int(hop), int(cap)
    lat, hist = int(lat_frames), int(history_frames)
    if doa is not None:
        max_lag = _doa_plan(doa[0], nc, doa[1])
    if not 2 <= nc <= GCC_MAX_CHANNELS:
        raise ValueError(f"event_tdoa_ring needs 2 to {GCC_MAX_CHANNELS} audio channels (one estimate per microphone pair), got channels={nc}")
    if not 1 <= max_lag <= MAX_LAG_LIMIT or max_frames < 1 or tf < 1 or hop < 1 or lat < 0 or hist < 1:
        raise ValueError(f"event_tdoa_ring needs 1 <= max_lag <= {MAX_LAG_LIMIT}, max_frames >= 1, time_factor >= 1, hop >= 1, lat_frames >= 0 "
                         f"and history_frames >= 1, got max_lag={max_lag}, max_frames={max_frames}, time_factor={tf}, hop={hop}, "
                         f"lat_frames={lat}, history_frames={hist}")
    src = _ring_source(ring, cap, n, nc)
    return _locate(src, events, tf, hop, max_lag, max_frames, [max_lag, max_frames, lat, hist], return_curve, max_workspace_bytes, doa)


def event_tdoa(pcm, clips, channels, events, time_factor, max_lag=24, max_frames=256, hop=HOP, pad_mode="constant",
               return_curve=False, max_workspace_bytes=128 << 20):
    """Per-event time difference of arrival (``sed_event_tdoa``).  ``pcm`` / ``clips`` / ``channels``: R recordings of
    2..8 planar channels in one float32 CUDA buffer, as ``mbe_planar`` takes them.  ``events``: a dict of int32 device tensors
    ``onset``, ``offset`` (exclusive), ``peak_frame`` in output frames of ``time_factor`` feature frames, as the decoders return
    them, with ``rec`` when R > 1.  For every event and microphone pair p = (i, j), i < j in lexicographic order, the GCC-PHAT of
    the event's frames (``localize.event_frames``: all of them up to ``max_frames``, else ``max_frames`` around the peak) is
    accumulated and searched over ``|tau| <= max_lag`` -> a dict of device tensors: ``lag`` float32 [E, P] in samples at the
    PCM's rate (channel j = channel i delayed by d samples gives -d; seconds = lag / sr), ``strength`` float32 [E, P] in [-1, 1]
    (the accumulated correlation at the peak per frame), ``loc_frames`` int32 [E] (0: the event names no recording or lies
    beyond its end; its lag and strength are 0), and with ``return_curve=True`` ``acc`` float32 [E, P, 2*max_lag + 3], the
    accumulated correlation at lags -(max_lag+1) .. max_lag+1.  The partial sums of at most ``max_workspace_bytes`` worth of
    events are held at a time; the slicing changes no bit, and neither do the other events, the batch or the clip's place in
    the buffer.  The host reads nothing back.  The cost is per located frame (every event transforms its own frames: 21 ns per
    frame at 4 channels on an MI355X): for an event table that covers its recordings more than about five times over — many
    long, heavily overlapping events — ``mbe_planar(..., spatial="gcc_phat")`` with ``n_mels = 2 * (max_lag + 2)`` followed by sums
    of the GCC columns over each event's rows is the cheaper route."""
    return _tdoa_linear(pcm, clips, channels, events, time_factor, max_lag, max_frames, hop, pad_mode, return_curve, max_workspace_bytes,
                        None)


def event_doa(pcm, clips, channels, events, time_factor, doa, sr=SR, hop=HOP, pad_mode="constant", return_curve=False,
              return_map=False, max_workspace_bytes=128 << 20, n_classes=None):
    """Per-event direction of arrival for a known array (``sed_event_doa``): ``event_tdoa`` with ``max_lag`` and
    ``max_frames`` taken from ``doa`` (a ``sed.DOA(positions, grid, ...)``; ``sr``: the rate of the PCM), and for every event
    the direction of ``doa.grid`` with the largest steered response power, summed over all microphone pairs at lags of
    ``1 / doa.oversample`` sample.  Returns the dict of ``event_tdoa`` — the same bits — with ``dir`` int32 [E] (a row of the
    grid; -1: the event has no frames, or digital silence) and ``doa_power`` float32 [E] (the response per pair and frame at
    that direction, in [-1, 1]; 0 where ``dir`` is -1); ``return_map=True`` adds ``srp`` float32 [E, D], the response at every
    direction (secondary peaks are other sources or reflections).  One more launch per slice; the host reads nothing back.

    With ``doa.track`` set (a ``sed.DirectionTrack(block_chunks, max_step_deg)``; ``sed_event_doa_track``) every key
    above keeps its bits and the dict gains a direction per block of ``32 * block_chunks`` located frames
    (``localize.track_blocks``), ``Tm = ceil(ceil(max_frames / 32) / block_chunks)`` columns an event: ``trk_len`` int32 [E], the
    blocks T of the event; ``trk_raw`` int32 [E, Tm], the maximum of every block's own map (-1: a silent block, and behind T);
    ``trk_dir`` int32 [E, Tm], the best path through the block maps that turns by at most ``max_step_deg`` a block (-1 where
    ``trk_raw`` is; ``trk_raw`` itself without ``max_step_deg``); ``trk_power`` float32 [E, Tm], the block's response at
    ``trk_raw`` per pair and frame; and with ``return_map=True`` ``trk_map`` float32 [E, Tm, D].  No frame is transformed twice:
    the blocks are steered from the chunk sums the event's own direction is made from.

    With ``doa.contrast`` set (a ``sed.Contrast(frames, search, guard, min_frames, weight)``; ``sed_event_doa_contrast`` /
    ``sed_event_doa_track_contrast``) the events must also hold ``cls`` and ``n_classes`` in 1..32 — what ``cls`` counts
    in — is required.  ``lag``, ``strength``, ``loc_frames`` and ``acc`` keep their bits; ``dir``, ``doa_power``, ``srp`` and every
    ``trk_`` key are made from ``S' = S - weight (nf / nb) Sb``, with ``Sb`` the summed whitened cross spectrum of the nb frames
    before the onset that ``localize.Contrast`` describes: an event that sounds over a louder source of another class gets its
    own direction, not that source's.  The dict gains ``bg_frames`` int32 [E], nb (0: fewer than ``min_frames`` were found and
    every key of the event is the plain one, bit for bit), and ``bg_sel`` int32 [E, frames], the candidates q in summation order,
    -1 behind them (``event_contrast_frames`` returns the two alone).  Every row of the table marks activity, located or not, and
    the activity is made once from the whole table, whatever the slicing.  An event's outputs then depend on its own samples and
    those of its background frames alone."""
    return _tdoa_linear(pcm, clips, channels, events, time_factor, 24, getattr(doa, "max_frames", 256), hop, pad_mode, return_curve,
                        max_workspace_bytes, (doa, sr, return_map), n_classes)


def event_contrast_frames(clips, channels, events, time_factor, doa, n_classes, hop=HOP):
    """Which frames before its onset ``event_doa`` with ``doa = sed.DOA(..., contrast=sed.Contrast(...))`` makes every event's background
    spectrum from (``sed_event_contrast_frames``): the activity and the selection alone, no sample is read.  ``clips`` /
    ``channels`` as ``event_doa`` takes them (the lengths of the recordings are all that is used); ``events``: the table with
    ``cls`` — every row marks activity, located or not; ``n_classes`` in 1..32: what ``cls`` counts in.  Returns device tensors
    ``{"bg_frames": int32 [E], "bg_sel": int32 [E, frames]}``: the number of frames used (0: the event's map is the plain one) and
    their candidates q — candidate q is feature frame ``onset * tf - guard - 1 - q`` — in summation order, -1 behind them.  Integer
    throughout and a function of the table and the settings alone; the host reads nothing back."""
    from .localize import DOA
    nc, tf, hop = _beam_sizes("event_contrast_frames", channels, time_factor, hop)
    if not isinstance(doa, DOA) or doa.contrast is None:
        raise TypeError("event_contrast_frames takes the settings as a sed.DOA(..., contrast=sed.Contrast(...)) object")
    if doa.channels != nc:
        raise ValueError(f"the DOA settings hold {doa.channels} microphone positions, the audio has {nc} channels")
    ct, classes = doa.contrast, _contrast_classes("event_contrast_frames", n_classes)
    dev, table, R, col, E, extent = _frames_only("event_contrast_frames", clips, nc, events, _LOCATED[:3])
    out = {"bg_frames": torch.zeros(E, dtype=torch.int32, device=dev), "bg_sel": torch.full((E, ct.frames), -1, dtype=torch.int32, device=dev)}
    if E == 0:
        return out
    frames = _mask_frames(table, nc, tf, hop)
    need = lib().sed_event_contrast_frames_workspace_bytes(R, nc, frames, ct.frames)
    if need == 0:
        raise ValueError(f"sed_event_contrast_frames_workspace_bytes refuses R={R}, channels={nc}, {frames} output frames, frames={ct.frames}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    cols = _col_ptrs(col, _LOCATED[:3])
    check(lib().sed_event_contrast_frames(extent, C.c_void_p(table.ctypes.data), R, nc, cols[0], ptr(col["cls"]),
                                          *cols[1:], E, tf, hop, doa.max_frames, classes, ct.frames, ct.search, ct.guard, ct.min_frames,
                                          ptr(out["bg_frames"]), ptr(out["bg_sel"]), ptr(ws), ws.numel(), stream_ptr()),
          "sed_event_contrast_frames")
    return out


def event_tdoa_ring(ring, cap, n, channels, events, time_factor, max_lag=24, max_frames=256, hop=HOP, lat_frames=0,
                    history_frames=0x7fffffff, return_curve=False, max_workspace_bytes=128 << 20):
    """``event_tdoa`` on the PCM rings of live feeds (``sed_event_tdoa_ring``).  ``ring`` / ``cap`` as ``ring_write``
    fills them: feed r's ``channels`` lanes are the rings ``r*channels + c``; ``n`` [R] host ints: the samples feed r has
    received.  ``events`` as ``event_tdoa`` takes them; the feed of an event is its ``rec`` — or ``stream`` — column (needed
    when R > 1).  An event is located on ``localize.event_frames`` with ``n_feat = 1 + n // hop`` unless
    ``offset*tf + lat_frames - f0 > history_frames`` (``localize.stream_locates``: the stream's rule) or its first sample has
    left the ring (``max(0, f0*hop - 1024) < n - cap``): then ``loc_frames = 0``, ``lag = 0``, ``strength = 0`` and nothing is
    read.  Samples before the start of the feed and beyond ``n`` read as 0 (constant padding).  A located event gets, bit for
    bit, what ``event_tdoa`` gives on the feed's samples ``[0, n)`` laid out linearly, wherever the ring wraps.  Returns the
    dict ``event_tdoa`` returns; the host reads nothing back."""
    return _tdoa_ring(ring, cap, n, channels, events, time_factor, max_lag, max_frames, hop, lat_frames, history_frames, return_curve,
                      max_workspace_bytes, None)


def event_doa_ring(ring, cap, n, channels, events, time_factor, doa, sr=SR, hop=HOP, lat_frames=0, history_frames=0x7fffffff,
                   return_curve=False, return_map=False, max_workspace_bytes=128 << 20):
    """``event_doa`` on the PCM rings of live feeds (``sed_event_doa_ring``): the arguments and rules of
    ``event_tdoa_ring``, the outputs of ``event_doa``; an event the stream's rule or the ring's depth refuses has ``dir = -1``
    and ``doa_power = 0``.  A located event gets, bit for bit, what ``event_doa`` gives on the feed's samples laid out linearly.
    A ``doa`` with ``contrast=`` has no ring form yet: NotImplementedError."""
    if getattr(doa, "contrast", None) is not None:
        raise NotImplementedError("event_doa_ring: sed.DOA(..., contrast=...) has no ring form yet (it needs search + guard more feature "
                                  "frames of ring and a per-feed activity ring); locate on the recording (event_doa)")
    return _tdoa_ring(ring, cap, n, channels, events, time_factor, 24, getattr(doa, "max_frames", 256), hop, lat_frames, history_frames,
                      return_curve, max_workspace_bytes, (doa, sr, return_map))


def ring_write(ring, cap, src, table, workspace=None):
    """A round's new samples into the PCM rings of live feeds (``sed_stream_ring_write``).  ``ring``: float32 CUDA
    buffer of ``lanes * cap`` samples, lane l (feed s, channel c: ``s*C + c``) keeps its last ``cap`` samples, sample i of the
    lane at ``ring[l*cap + i % cap]``; ``src``: the new samples, packed (float32 CUDA, or None when every count is 0);
    ``table`` [lanes, 3] host ints ``{first sample in src, count <= cap, absolute index of the first sample}``.  One launch;
    the host reads nothing back.  -> the workspace, for the next call."""
    _need_ring("ring_write", ring)
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int64).reshape(-1, 3))
    lanes, cap = table.shape[0], int(cap)
    if lanes < 1 or cap < 4 or cap % 4 or lanes * cap > ring.numel():
        raise ValueError(f"{lanes} lanes of cap={cap} samples (a multiple of 4) do not fit the ring buffer of {ring.numel()} samples")
    if (table[:, 1] < 0).any() or (table[:, 1] > cap).any():
        raise ValueError(f"a lane takes 0 to cap={cap} new samples per call, got {int(table[:, 1].min())} .. {int(table[:, 1].max())}")
    if src is not None:
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.float32):
            raise RuntimeError("sed_crnn_amd.feature.ring_write needs the new samples as a float32 CUDA(HIP) tensor")
        src = src.contiguous().view(-1)
    need = lib().sed_stream_ring_write_workspace_bytes(lanes)
    if need == 0:
        raise ValueError(f"sed_stream_ring_write takes 1..65535 lanes, got {lanes}")
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=ring.device)
    check(lib().sed_stream_ring_write(ptr(ring), ring.numel(), lanes, cap, ptr(src), src.numel() if src is not None else 0,
                                      C.c_void_p(table.ctypes.data), ptr(workspace), workspace.numel(), stream_ptr()),
          "sed_stream_ring_write")
    return workspace


# ───────────────────────── a located event's audio: delay-and-sum and MVDR ─────────────────────────
_BEAM_TAPS = {}              # (device, DelaySum) -> the filter on the device


def _beam_empty(dev):
    return {"audio": torch.empty(0, device=dev), "audio_start": torch.empty(0, dtype=torch.int64, device=dev),
            "audio_len": torch.empty(0, dtype=torch.int32, device=dev)}


def _mvdr_empty(dev, mvdr):
    out = _beam_empty(dev)
    if mvdr.noise_blocks:
        out["noise_frames"] = torch.empty(0, dtype=torch.int32, device=dev)
    if mvdr.quiet:
        out["noise_sel"] = torch.empty(0, mvdr.noise_blocks, dtype=torch.int32, device=dev)
    return out


@functools.lru_cache(maxsize=8)
def _mvdr_tables(device_index):
    """the 2048-point tables with the MVDR beam's window (``localize.mvdr_window``): the header, window and twiddle sections of a
    ``build_tables`` blob — the mel plan behind them is not read and not kept — cached per device"""
    from .localize import mvdr_window
    blob = build_tables(mvdr_window(), slaney_mel_basis(SR, NFFT, NB_MEL), torch.device("cuda", device_index))
    return blob[:_LM_OFF_ENT].clone()


def _extract(src, kind, col, E, tf, hop, max_frames, D, settings, ws_bytes, Kn=0, track=()):
    """the two calls behind the four beam functions: the spans, ONE blocking read of the total (8 bytes) to size ``audio``, the
    beam ``kind``.  ``settings``: what the beam's C entry takes between ``max_frames`` and the spans; ``mvdr_noise``
    adds ``noise_frames`` int32 [E] to the dict, ``mvdr_quiet`` (``Kn``: its noise_blocks) that and ``noise_sel`` int32
    [E, Kn], and its C entry takes the ``cls`` column behind ``rec``; the track forms are ``mvdr_noise`` and ``mvdr_quiet``
    with ``track`` — block_chunks, Tm and the two columns — behind their outputs, and ``noise_frames`` in the dict only with Kn >= 1"""
    dev = src.x.device
    out = {"audio_start": torch.empty(E, dtype=torch.int64, device=dev), "audio_len": torch.empty(E, dtype=torch.int32, device=dev)}
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cols = _col_ptrs(col, _LOCATED)
    spans, name = _ENTRY["spans", src.ring], _ENTRY[kind, src.ring]
    check(getattr(lib(), spans)(*src.spans_head, *cols, E, tf, hop, max_frames, D, ptr(out["audio_len"]), ptr(out["audio_start"]), ptr(total),
                                ptr(ws), ws.numel(), stream_ptr()), spans)
    n_total = int(total.item())                                       # the one blocking read
    out["audio"] = torch.empty(n_total, device=dev)
    noise = []
    if kind in ("mvdr_noise", "mvdr_quiet", "mvdr_track", "mvdr_quiet_track"):
        frames = torch.zeros(E, dtype=torch.int32, device=dev)        # (a call that extracts nothing launches nothing)
        noise = [ptr(frames)]
        if Kn or kind != "mvdr_track":                                # (the own-frames track form returns the dict of sed_event_mvdr)
            out["noise_frames"] = frames
    if kind in ("mvdr_quiet", "mvdr_quiet_track"):
        out["noise_sel"] = torch.full((E, Kn), -1, dtype=torch.int32, device=dev)
        noise.append(ptr(out["noise_sel"]))
        cols = cols[:1] + [ptr(col["cls"])] + cols[1:]
    check(getattr(lib(), name)(*src.head, *cols, E, tf, hop, max_frames, *settings, ptr(out["audio_len"]), ptr(out["audio_start"]),
                               ptr(out["audio"]), n_total, *noise, *track, ptr(ws), ws.numel(), stream_ptr()), name)
    return out


def _table_bytes(src):
    """the workspace bytes of the recording table alone: all that the spans and the delay-and-sum beam need"""
    return lib().sed_event_beam_ring_workspace_bytes(src.R) if src.ring else lib().sed_event_beam_workspace_bytes(src.R, src.nc)


def _beamform(who, src, events, tf, hop, doa, beam, sr):
    """``event_beamform`` / ``event_beamform_ring`` on their source; M and the taps are uploaded once per device, rate and filter"""
    from .localize import DelaySum
    _doa_plan(doa, src.nc, sr)
    if not isinstance(beam, DelaySum):
        raise TypeError(f"{who} takes the beam settings as a sed.DelaySum(...) object, got {type(beam).__name__}")
    dev = src.x.device
    col, E = _cols(src, events, _LOCATED)
    key = (dev.index or 0, float(sr), beam.oversample)
    if key not in doa._beam_device:
        doa._beam_device[key] = torch.from_numpy(doa.delays(sr, beam.oversample)).to(dev)
    tkey = (dev.index or 0, beam)
    if tkey not in _BEAM_TAPS:
        _BEAM_TAPS[tkey] = torch.from_numpy(beam.taps.copy()).to(dev)                # (the cached table is read-only)
    if E == 0:
        return _beam_empty(dev)
    M = doa._beam_device[key]
    return _extract(src, "delay_sum", col, E, tf, hop, doa.max_frames, M.shape[0],
                    [ptr(M), M.shape[0], beam.oversample, beam.half_width, ptr(_BEAM_TAPS[tkey])], _table_bytes(src))


def _quiet_settings(who, mvdr, n_classes):
    """the quiet settings as the C entries take them behind noise_guard -> [n_classes, S, M, exclude_any]"""
    from .localize import MVDR_MAX_CLASSES
    return [_n_classes(who, "sed.MVDR(noise_select='quiet')", n_classes, MVDR_MAX_CLASSES), mvdr.noise_search, mvdr.noise_min,
            int(mvdr.noise_exclude == "any")]


def _mvdr(who, src, events, tf, hop, doa, mvdr, sr, max_workspace_bytes, n_classes=None):
    """``event_mvdr`` / ``event_mvdr_ring`` on their source; with ``mvdr.noise_blocks >= 1`` the entry's noise form,
    with ``mvdr.quiet`` its quiet form"""
    from .localize import MVDR
    _doa_plan(doa, src.nc, sr)
    if not isinstance(mvdr, MVDR):
        raise TypeError(f"{who} takes the beam settings as a sed.MVDR(...) object, got {type(mvdr).__name__}")
    R, nc, dev, max_frames = src.R, src.nc, src.x.device, doa.max_frames
    quiet = _quiet_settings(who, mvdr, n_classes) if mvdr.quiet else []
    follow = mvdr.follow_track
    if follow and (doa.track is None or "trk_len" not in events or "trk_dir" not in events):
        raise ValueError(f"{who} with sed.MVDR(follow_track=True) steers along the direction track: it needs sed.DOA(..., track="
                         f"sed.DirectionTrack(...)) and the events' trk_len and trk_dir columns as event_doa returns them with track=")
    col, E = _cols(src, events, _LOCATED + (("cls",) if mvdr.quiet else ()))
    track = []
    if follow:                                                                   #  W, Tm and the two columns
        Tm = doa.track.max_blocks(max_frames)
        tlen, tdir = events["trk_len"].to(dev, torch.int32).contiguous(), events["trk_dir"].to(dev, torch.int32).contiguous()
        if tlen.shape != (E,) or tdir.shape != (E, Tm):
            raise ValueError(f"{who}: trk_len must be [E] = [{E}] and trk_dir [E, Tm] = [{E}, {Tm}] (track= of the same sed.DOA), got "
                             f"{tuple(tlen.shape)} and {tuple(tdir.shape)}")
        track = [doa.track.block_chunks, Tm, ptr(tlen), ptr(tdir)]
    if E == 0:
        return _mvdr_empty(dev, mvdr)
    Kn = mvdr.noise_blocks
    kind = "mvdr" if not Kn else "mvdr_quiet" if mvdr.quiet else "mvdr_noise"
    noise = [Kn, mvdr.noise_guard] + quiet if Kn else []                         # what the entry takes behind loading
    if follow:                                                                   # the track entries take noise_blocks = 0 too
        kind = "mvdr_quiet_track" if mvdr.quiet else "mvdr_track"
        noise = [Kn, mvdr.noise_guard] + quiet
    name = _ENTRY[kind, src.ring] + "_workspace_bytes"
    if mvdr.quiet:                                                               # the mask lies behind the table, once per call
        frames = _mask_frames(src.table, nc, tf, hop)
        need_tab = lib().sed_event_quiet_frames_workspace_bytes(R, nc, frames, Kn)
        need_one = getattr(lib(), name)(R, nc, max_frames, hop, Kn, frames, *track[1:2])     # the table, the mask and one event
    else:
        need_tab = _table_bytes(src)
        need_one = getattr(lib(), name)(R, nc, max_frames, hop, *noise[:1], *track[1:2])     # the recording table and one event
    if need_one == 0 or need_tab == 0:
        raise ValueError(f"{name} refuses R={R}, channels={nc}, max_frames={max_frames}, hop={hop}")
    key = (dev.index or 0, float(sr))
    if key not in doa._steering_device:
        doa._steering_device[key] = torch.from_numpy(doa.steering(sr)).to(dev)
    tau = doa._steering_device[key]
    tables = _mvdr_tables(dev.index or 0)
    ws_bytes = min(need_tab + E * (need_one - need_tab), max(need_one, int(max_workspace_bytes)))
    return _extract(src, kind, col, E, tf, hop, max_frames, tau.shape[0],
                    [ptr(tau), tau.shape[0], mvdr.loading, *noise, ptr(tables), tables.numel() * 4], ws_bytes, Kn, track)


def event_quiet_frames(clips, channels, events, time_factor, doa, mvdr, n_classes, hop=HOP):
    """Which pre-onset frames ``event_mvdr`` with ``mvdr = sed.MVDR(..., noise_select="quiet")`` makes every event's noise
    covariance from (``sed_event_quiet_frames``): the activity and the selection alone, no sample is read.  ``clips`` /
    ``channels`` as ``event_mvdr`` takes them (the lengths of the recordings are all that is used); ``events``: the located table
    with ``cls`` — every row marks activity, located or not; ``n_classes`` in 1..32: what ``cls`` counts in.  Returns device tensors
    ``{"noise_frames": int32 [E], "noise_sel": int32 [E, Kn]}``: the number of frames used (0: the event keeps its own frames)
    and their candidates q — frame q is the 2048 samples from ``s0 - (G + 2 + q) 1024`` — in summation order, -1 behind them.
    Integer throughout and a function of the table and the settings alone; the host reads nothing back."""
    from .localize import MVDR
    nc, tf, hop = _beam_sizes("event_quiet_frames", channels, time_factor, hop)
    if not isinstance(mvdr, MVDR) or not mvdr.quiet:
        raise TypeError("event_quiet_frames takes the beam settings as a sed.MVDR(..., noise_select='quiet') object")
    _doa_plan(doa, nc, SR)
    quiet = _quiet_settings("event_quiet_frames", mvdr, n_classes)
    dev, table, R, col, E, extent = _frames_only("event_quiet_frames", clips, nc, events, _LOCATED)
    Kn = mvdr.noise_blocks
    out = {"noise_frames": torch.zeros(E, dtype=torch.int32, device=dev), "noise_sel": torch.full((E, Kn), -1, dtype=torch.int32, device=dev)}
    if E == 0:
        return out
    frames = _mask_frames(table, nc, tf, hop)
    need = lib().sed_event_quiet_frames_workspace_bytes(R, nc, frames, Kn)
    if need == 0:
        raise ValueError(f"sed_event_quiet_frames_workspace_bytes refuses R={R}, channels={nc}, {frames} output frames, noise_blocks={Kn}")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    cols = _col_ptrs(col, _LOCATED)
    check(lib().sed_event_quiet_frames(extent, C.c_void_p(table.ctypes.data), R, nc, cols[0], ptr(col["cls"]),
                                       *cols[1:], E, tf, hop, doa.max_frames, doa.grid.unit_vectors.shape[0], quiet[0], Kn, mvdr.noise_guard,
                                       *quiet[1:], ptr(out["noise_frames"]), ptr(out["noise_sel"]), ptr(ws), ws.numel(), stream_ptr()),
          "sed_event_quiet_frames")
    return out


def event_beamform(pcm, clips, channels, events, time_factor, doa, beam, sr=SR, hop=HOP):
    """The audio of every located event with the array pointed at it (``sed_event_beam_spans`` + ``sed_event_beamform``, DESIGN
    5r): a steered delay-and-sum beam.  ``pcm`` / ``clips`` / ``channels`` / ``events`` / ``time_factor`` as ``event_doa`` takes
    them; the events must also hold ``dir`` and ``loc_frames`` as ``event_doa`` (with the same ``doa``, a ``sed.DOA``) returns
    them; ``beam``: a ``sed.DelaySum(oversample, half_width, beta)``; ``sr``: the rate of the PCM.  An event with ``dir >= 0``
    is extracted: its samples are ``localize.event_samples`` — the frames it was located on — and every output sample is the
    mean over the channels of the channel evaluated ``doa.delays(sr, Q)[dir][c] / Q`` samples earlier, through the 2H-tap filter
    ``beam.taps`` (samples outside the recording read as 0).  Returns device tensors ``{"audio": float32 [total], "audio_start":
    int64 [E], "audio_len": int32 [E]}``: event e is ``audio[audio_start[e] : audio_start[e] + audio_len[e]]``, the events packed
    in event order; events that are not extracted have length 0.  The host does ONE blocking read, the 8 bytes of the total,
    to size ``audio``; nothing else is read back.  ``E == 0`` returns empty tensors without a launch.  Every sample depends on
    its event's own samples alone: the batch, the order of the table, the other events and the clip's place in the buffer
    change no bit."""
    _need_pcm("event_beamform", pcm)
    nc, tf, hop = _beam_sizes("event_beamform", channels, time_factor, hop)
    return _beamform("event_beamform", _linear_source(pcm, clips, nc, align_16=True), events, tf, hop, doa, beam, sr)


def event_beamform_ring(ring, cap, n, channels, events, time_factor, doa, beam, sr=SR, hop=HOP):
    """``event_beamform`` on the PCM rings of live feeds (``sed_event_beam_spans_ring`` + ``sed_event_beamform_ring``):
    ``ring`` / ``cap`` / ``n`` as ``event_doa_ring`` takes them, the events with the ``dir`` and ``loc_frames`` it returned (an
    event the stream's rule or the ring's depth refused has ``dir = -1`` and length 0 here); the feed of an event is its
    ``rec`` — or ``stream`` — column.  An extracted event gets, bit for bit, what ``event_beamform`` gives on the feed's samples
    ``[0, n)`` laid out linearly, wherever the ring wraps.  Returns what ``event_beamform`` returns, with the same single
    8-byte read."""
    _need_ring("event_beamform_ring", ring)
    nc, tf, hop = _beam_sizes("event_beamform_ring", channels, time_factor, hop)
    return _beamform("event_beamform_ring", _ring_source(ring, int(cap), n, nc, need_16_byte=True), events, tf, hop, doa, beam, sr)


def event_mvdr(pcm, clips, channels, events, time_factor, doa, mvdr, sr=SR, hop=HOP, max_workspace_bytes=128 << 20, n_classes=None):
    """The audio of every located event through an adaptive beam (``sed_event_beam_spans`` + ``sed_event_mvdr``):
    the arguments, the events that are extracted, their samples and the returned dict — ``audio`` float32 [total],
    ``audio_start`` int64 [E], ``audio_len`` int32 [E] — are ``event_beamform``'s; ``mvdr``: a ``sed.MVDR(loading)``.  On the
    event's own grid of 2048-sample frames every 1024 samples (sqrt-Hann window; every sample outside the event read as 0) the
    spatial covariance of every frequency bin is summed over the event's frames, the weights
    ``w = (R + loading trace(R)/C I)^-1 d / (d^H (R + ...)^-1 d)`` for the steering vector ``d`` of ``doa.steering(sr)[dir]`` are
    solved in float64 on the device, and the frames are combined, transformed back and overlap-added.  A source in the
    event's direction passes unchanged; whatever else the event's frames contain — a second source, above all — is suppressed
    as far as ``loading`` and the number of frames allow (DESIGN 5s has figures).  The covariance partials of at most
    ``max_workspace_bytes`` worth of events are held at a time; the slicing changes no bit, and neither do the other events,
    the batch, the clip's place in the buffer or the samples outside the event.  The host does ONE blocking read, the 8 bytes
    of the total; ``E == 0`` returns empty tensors without a launch.

    ``sed.MVDR(loading, noise_blocks=Kn, noise_guard=G)`` with ``Kn >= 1`` (``sed_event_mvdr_noise``): an event with
    ``s0 >= (G + Kn + 1) 1024`` gets its weights from the covariance of the Kn frames before its onset, the samples
    ``[s0 - (G + Kn + 1) 1024, s0 - G 1024)`` of its recording, which do not hold the target: a steering error no longer makes
    the beam cancel it.  Every other event gets what ``Kn = 0`` gives, bit for bit.  The dict gains ``noise_frames`` int32 [E]:
    Kn where the noise covariance was used, else 0.  An event's audio then depends on those samples and its own alone.

    ``sed.MVDR(..., noise_blocks=Kn, noise_select="quiet")`` (``sed_event_mvdr_quiet``): the Kn frames are the nearest
    of ``noise_search`` candidates before the onset in which no event of the table with the same class (``noise_exclude="any"``:
    any class) is active; the events must also hold ``cls``, and ``n_classes`` in 1..32 — what ``cls`` counts in — is required.
    Every row of the table marks activity, located or not, and the activity is made once from the whole table, whatever the
    slicing.  The dict gains ``noise_frames`` int32 [E], the number of frames used (0: fewer than ``noise_min`` were found and
    the event keeps its own frames, bit for bit what ``Kn = 0`` gives), and ``noise_sel`` int32 [E, Kn], their candidates q
    in summation order, -1 behind them (``event_quiet_frames`` returns the two alone).  An event whose Kn nearest candidates
    are all eligible gets the audio of ``noise_select="fixed"``, bit for bit.

    ``sed.MVDR(..., follow_track=True)`` (``sed_event_mvdr_track`` / ``sed_event_mvdr_quiet_track``): ``doa`` must have
    ``track=`` and the events the ``trk_len`` / ``trk_dir`` columns ``event_doa`` then returns (else ValueError).  The samples, the
    covariance of the settings above and the returned dict are unchanged; frame j of an event is combined with the weights of
    track block ``localize.mvdr_frame_blocks(...)[j]``, steered at that block's ``trk_dir`` — ``dir`` for a silent block, a row
    outside the grid and an event with ``trk_len = 0`` — one weight set per block from the event's one covariance.  A track
    whose every used row equals ``dir`` gives the audio of ``follow_track=False``, bit for bit."""
    _need_pcm("event_mvdr", pcm)
    nc, tf, hop = _beam_sizes("event_mvdr", channels, time_factor, hop)
    return _mvdr("event_mvdr", _linear_source(pcm, clips, nc), events, tf, hop, doa, mvdr, sr, max_workspace_bytes, n_classes)


def event_mvdr_ring(ring, cap, n, channels, events, time_factor, doa, mvdr, sr=SR, hop=HOP, max_workspace_bytes=128 << 20):
    """``event_mvdr`` on the PCM rings of live feeds (``sed_event_beam_spans_ring`` + ``sed_event_mvdr_ring``): ``ring`` /
    ``cap`` / ``n`` / ``events`` as ``event_beamform_ring`` takes them (an event the stream's rule or the ring's depth refused
    has ``dir = -1`` and length 0 here; the feed of an event is its ``rec`` — or ``stream`` — column), ``mvdr`` and
    ``max_workspace_bytes`` as ``event_mvdr``.  An extracted event gets, bit for bit, what ``event_mvdr`` gives on the feed's
    samples ``[0, n)`` laid out linearly, wherever the ring wraps and whatever the slicing; a sample the ring no longer holds
    reads as 0.  Returns what ``event_mvdr`` returns, with the same single 8-byte read; ``E == 0`` returns empty tensors without
    a launch.  ``sed.MVDR(..., follow_track=True)`` (``sed_event_mvdr_track_ring``) as in ``event_mvdr``, with the
    ``trk_len`` / ``trk_dir`` of ``event_doa_ring``."""
    if getattr(mvdr, "quiet", False):
        raise NotImplementedError("event_mvdr_ring: sed.MVDR(noise_select='quiet') has no ring form yet; extract on the recording (event_mvdr)")
    _need_ring("event_mvdr_ring", ring)
    nc, tf, hop = _beam_sizes("event_mvdr_ring", channels, time_factor, hop)
    return _mvdr("event_mvdr_ring", _ring_source(ring, int(cap), n, nc), events, tf, hop, doa, mvdr, sr, max_workspace_bytes)
