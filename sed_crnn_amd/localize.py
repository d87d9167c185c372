"""Where a detected event came from: the host side of per-event TDOA (the kernels are csrc/tdoa.hip, the device
entry ``feature.event_tdoa``).

``event_frames`` is the rule that picks the feature frames an event is located on — the kernels apply the same rule on the
device.  ``stream_latency_frames``, ``stream_ring_samples`` and ``stream_locates`` are the arithmetic of a localising live
stream: how late an event is emitted, how many samples a lane keeps, and which events are located.  ``TDOA`` holds
the two settings of ``EventDetector(..., localize=TDOA(...))``.  ``max_lag_for`` and ``tdoa_to_azimuth`` are the far-field
geometry of ONE microphone pair; combining pairs into a direction for a given array is left to the caller.
"""
import dataclasses
import math

import numpy as np

MAX_LAG_LIMIT = 127        # tdoa.hip: TD_MAX_LAG
SPEED_OF_SOUND = 343.0     # m/s in air at 20 degrees C


def event_frames(onset, offset, peak_frame, time_factor, n_feat, max_frames=256):
    """The feature frames ``[f0, f1)`` that an event (``onset``, ``offset`` exclusive, ``peak_frame``: output frames of
    ``time_factor`` feature frames each) of a recording with ``n_feat`` feature frames is located on.  With ``a = onset*tf`` and
    ``b = min(offset*tf, n_feat)``: ``[a, b)`` when it has at most ``max_frames`` frames; otherwise the ``max_frames`` frames
    centred on the peak, ``f0 = clamp(peak_frame*tf + tf//2 - max_frames//2, a, b - max_frames)``.  An empty event (``b <= a``,
    which no decoder emits) is located on the single frame ``a``.  An event that lies wholly outside its recording (``onset < 0``
    or ``a >= n_feat``) has no frames: ``(0, 0)``."""
    tf, n_feat, max_frames = int(time_factor), int(n_feat), int(max_frames)
    if tf < 1 or n_feat < 1 or max_frames < 1:
        raise ValueError(f"event_frames needs time_factor >= 1, n_feat >= 1 and max_frames >= 1, got {tf}, {n_feat}, {max_frames}")
    a, b = int(onset) * tf, min(int(offset) * tf, n_feat)
    if int(onset) < 0 or a >= n_feat:
        return 0, 0
    if b <= a:
        return a, a + 1
    if b - a <= max_frames:
        return a, b
    c = int(peak_frame) * tf + tf // 2 - max_frames // 2
    f0 = min(max(c, a), b - max_frames)
    return f0, f0 + max_frames


# ── live feeds: how long an emitted event's audio must be kept ──
def stream_latency_frames(time_factor, seq_len, median_max, min_gap_max):
    """``lat``: the step of a stream that emits the event ``[a, b)`` runs with fewer than ``b*tf + lat + step_frames`` final
    feature frames, ``lat = (max_k min_gap_k + median_max // 2 + seq_len // tf + 1) * tf`` (more than ``b + min_gap`` decided
    frames need ``b + min_gap + 1 + median // 2 + seq_len // tf`` output frames)"""
    tf = int(time_factor)
    if tf < 1 or int(seq_len) < tf or int(median_max) < 1 or int(min_gap_max) < 0:
        raise ValueError(f"stream_latency_frames needs time_factor >= 1, seq_len >= time_factor, median_max >= 1 and min_gap_max >= 0, "
                         f"got {time_factor}, {seq_len}, {median_max}, {min_gap_max}")
    return (int(min_gap_max) + int(median_max) // 2 + int(seq_len) // tf + 1) * tf


def stream_ring_samples(history_frames, step_frames, hop_length, n_fft=2048):
    """``cap``: samples per lane of a stream's PCM ring, ``roundup4((history_frames + step_frames) * hop_length + n_fft)``: enough
    for every event that ``stream_locates`` accepts, in any chunking (DESIGN 5p has the proof)"""
    if int(history_frames) < 1 or int(step_frames) < 1 or int(hop_length) < 1:
        raise ValueError(f"stream_ring_samples needs history_frames, step_frames and hop_length >= 1, got {history_frames}, "
                         f"{step_frames}, {hop_length}")
    return ((int(history_frames) + int(step_frames)) * int(hop_length) + int(n_fft) + 3) & ~3


def stream_locates(onset, offset, peak_frame, time_factor, n_feat, max_frames, lat, history_frames):
    """whether a stream with ``history_frames`` of audio locates this event: it has frames ``[f0, f1) = event_frames(...)`` and
    ``offset*tf + lat - f0 <= history_frames``.  The rule reads the event and the settings only, never the chunking; an event
    it refuses comes back with ``loc_frames = 0``, ``lag = 0`` and ``strength = 0``."""
    f0, f1 = event_frames(onset, offset, peak_frame, time_factor, n_feat, max_frames)
    return f1 > f0 and int(offset) * int(time_factor) + int(lat) - f0 <= int(history_frames)


@dataclasses.dataclass(frozen=True)
class TDOA:
    """Settings of per-event localisation (``EventDetector(model, ..., localize=TDOA(...))``).  ``max_lag``: the
    largest time difference that is searched, in samples at the detector's rate (``max_lag_for(spacing, sr)`` for a pair
    ``spacing`` metres apart), 1..127.  ``max_frames``: an event longer than this many feature frames is located on the
    ``max_frames`` frames around its peak."""
    max_lag: int = 24
    max_frames: int = 256

    def __post_init__(self):
        for name in ("max_lag", "max_frames"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"TDOA: {name} must be an integer, got {v!r}")
            object.__setattr__(self, name, int(v))
        if not 1 <= self.max_lag <= MAX_LAG_LIMIT:
            raise ValueError(f"TDOA: max_lag must be in 1..{MAX_LAG_LIMIT} samples, got {self.max_lag}")
        if self.max_frames < 1:
            raise ValueError(f"TDOA: max_frames must be >= 1, got {self.max_frames}")


def max_lag_for(spacing_m, sr, c=SPEED_OF_SOUND):
    """the largest lag, in samples at rate ``sr``, that a far-field source can produce between two microphones ``spacing_m``
    metres apart: ``ceil(spacing * sr / c)``"""
    if not spacing_m > 0 or not sr > 0 or not c > 0:
        raise ValueError(f"max_lag_for needs spacing_m > 0, sr > 0 and c > 0, got {spacing_m}, {sr}, {c}")
    return int(math.ceil(float(spacing_m) * float(sr) / float(c)))


def tdoa_to_azimuth(tdoa_seconds, spacing_m, c=SPEED_OF_SOUND):
    """far-field angle of arrival of one microphone pair, in radians from broadside: ``asin(clip(c * tdoa / spacing, -1, 1))``
    (0 for a source equally far from both, +-pi/2 along the pair's axis; a time difference larger than the spacing allows is
    clipped).  Host arrays or scalars."""
    if not spacing_m > 0 or not c > 0:
        raise ValueError(f"tdoa_to_azimuth needs spacing_m > 0 and c > 0, got {spacing_m}, {c}")
    return np.arcsin(np.clip(np.asarray(tdoa_seconds, dtype=np.float64) * (float(c) / float(spacing_m)), -1.0, 1.0))
