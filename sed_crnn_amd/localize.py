"""Where a detected event came from: the host side of per-event TDOA (the kernels are csrc/tdoa.hip, the device
entry ``events.event_tdoa``).

``event_frames`` is the rule that picks the feature frames an event is located on — the kernels apply the same rule on the
device.  ``stream_latency_frames``, ``stream_ring_samples`` and ``stream_locates`` are the arithmetic of a localising live
stream: how late an event is emitted, how many samples a lane keeps, and which events are located.  ``TDOA`` holds
the two settings of ``EventDetector(..., localize=TDOA(...))``.  ``max_lag_for`` and ``tdoa_to_azimuth`` are the far-field
geometry of ONE microphone pair.  ``DirectionGrid``, ``steering_lags`` and ``DOA`` are the host side of per-event direction of
arrival for a known array (the kernel is csrc/doa.hip, the device entry ``events.event_doa``): the directions that
are searched, the time difference every direction means for every microphone pair, and the settings of
``EventDetector(..., localize=DOA(positions, grid))``.  ``DelaySum``, ``beam_taps``, ``steering_delays`` and ``event_samples`` are
the host side of per-event audio extraction by a steered delay-and-sum beam (the kernels are csrc/beam.hip, the device
entry ``events.event_beamform``): the settings of ``EventDetector(..., localize=DOA(...), extract=DelaySum())``, the
fractional-delay filter, the delay every direction means for every microphone, and the samples an event's audio consists of.
``MVDR`` and ``mvdr_window`` are the host side of the adaptive beam that extracts the same events (the kernels are
csrc/mvdr.hip, the device entry ``events.event_mvdr``).  ``DirectionTrack``, ``track_blocks`` and ``track_neighbours`` are the host side
of direction tracks (the kernels are csrc/doatrack.hip): the settings of ``DOA(..., track=DirectionTrack(...))``, the
blocks an event's located frames are cut into, and the directions a smoothed track may step between.  ``Contrast`` holds the settings
of contrast SRP-PHAT (the kernels are csrc/contrast.hip): ``DOA(..., contrast=Contrast(...))`` locates an event that sounds
over a louder source of another class.
"""
import dataclasses
import functools
import math
import typing

import numpy as np

MAX_LAG_LIMIT = 127        # tdoa.hip: TD_MAX_LAG
SPEED_OF_SOUND = 343.0     # m/s in air at 20 degrees C
MAX_CHANNELS = 8           # tdoa.hip: TD_MAX_CH
MAX_DIRECTIONS = 16384     # doa.hip: DOA_MAX_DIRS
OVERSAMPLE_CHOICES = (1, 2, 4, 8, 16)


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


def stream_noise_frames(hop_length, noise_blocks, noise_guard=1):
    """``nf``: the feature frames before an event's first that hold the samples its pre-onset noise covariance reads,
    ``ceil((noise_guard + noise_blocks + 1) * 1024 / hop_length)``; 0 with ``noise_blocks = 0``"""
    Kn, G, hop = int(noise_blocks), int(noise_guard), int(hop_length)
    if hop < 1 or Kn < 0 or G < 0:
        raise ValueError(f"stream_noise_frames needs hop_length >= 1, noise_blocks >= 0 and noise_guard >= 0, got {hop}, {Kn}, {G}")
    return -(-(G + Kn + 1) * 1024 // hop) if Kn else 0


def stream_extracts(onset, offset, peak_frame, time_factor, n_feat, max_frames, lat, history_frames, hop_length, noise_blocks=0,
                    noise_guard=1):
    """whether a stream with ``history_frames`` of audio emits this event's audio: ``stream_locates`` it, and —
    where its weights come from the frames before its onset, ``f0 * hop_length >= (noise_guard + noise_blocks + 1) * 1024`` with
    ``noise_blocks >= 1`` — the ring still holds those too: ``offset*tf + lat - f0 + nf <= history_frames``,
    ``nf = stream_noise_frames(...)``.  An event near the feed's start, which falls back to its own frames, needs no more than
    ``stream_locates`` asks.  The rule reads the event and the settings only; an event it refuses keeps its ``dir`` and comes
    with ``audio_len = 0``.  (Whether the event is located at all — ``dir >= 0`` — is for the caller to know.)"""
    if not stream_locates(onset, offset, peak_frame, time_factor, n_feat, max_frames, lat, history_frames):
        return False
    f0, _ = event_frames(onset, offset, peak_frame, time_factor, n_feat, max_frames)
    Kn, G = int(noise_blocks), int(noise_guard)
    if Kn < 1 or f0 * int(hop_length) < (G + Kn + 1) * 1024:
        return True
    return int(offset) * int(time_factor) + int(lat) - f0 + stream_noise_frames(hop_length, Kn, G) <= int(history_frames)


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


# ── direction of arrival for a known array ──
class DirectionGrid:
    """The directions a ``DOA`` searches: ``unit_vectors`` [D, 3], each pointing from the array towards a source,
    ``u = (cos el cos az, cos el sin az, sin el)``; 1 <= D <= 16384.  ``.azimuth`` (in (-pi, pi]) and ``.elevation`` [D] are the
    angles of the rows in radians.  ``ring`` and ``sphere`` build the two usual grids."""

    def __init__(self, unit_vectors):
        u = np.array(unit_vectors, dtype=np.float64)
        if u.ndim != 2 or u.shape[1] != 3 or not 1 <= u.shape[0] <= MAX_DIRECTIONS:
            raise ValueError(f"DirectionGrid: unit_vectors must be [D, 3] with 1 <= D <= {MAX_DIRECTIONS}, got shape {u.shape}")
        if not np.isfinite(u).all():
            raise ValueError("DirectionGrid: unit_vectors must be finite")
        norm = np.sqrt((u * u).sum(1))
        if np.abs(norm - 1.0).max() > 1e-6:
            raise ValueError(f"DirectionGrid: every row must have unit norm (within 1e-6), got norms {norm.min():.6g} .. {norm.max():.6g}")
        u.setflags(write=False)
        self.unit_vectors = u
        self.azimuth = np.arctan2(u[:, 1], u[:, 0])
        self.elevation = np.arcsin(np.clip(u[:, 2], -1.0, 1.0))

    def __len__(self):
        return self.unit_vectors.shape[0]

    @classmethod
    def ring(cls, n_az, elevation=0.0):
        """``n_az`` directions at one elevation (radians), azimuth ``2 pi i / n_az``: what a planar array can tell apart"""
        n_az, el = int(n_az), float(elevation)
        if not 1 <= n_az <= MAX_DIRECTIONS or not abs(el) <= math.pi / 2:
            raise ValueError(f"DirectionGrid.ring needs 1 <= n_az <= {MAX_DIRECTIONS} and |elevation| <= pi/2, got {n_az}, {elevation}")
        az = 2.0 * math.pi * np.arange(n_az) / n_az
        return cls(np.stack([math.cos(el) * np.cos(az), math.cos(el) * np.sin(az), np.full(n_az, math.sin(el))], 1))

    @classmethod
    def sphere(cls, n):
        """``n`` directions spread evenly over the whole sphere: the Fibonacci lattice ``z_i = 1 - (2 i + 1) / n``,
        ``az_i = i pi (3 - sqrt 5)``"""
        n = int(n)
        if not 1 <= n <= MAX_DIRECTIONS:
            raise ValueError(f"DirectionGrid.sphere needs 1 <= n <= {MAX_DIRECTIONS}, got {n}")
        i = np.arange(n)
        z = 1.0 - (2.0 * i + 1.0) / n
        az = i * (math.pi * (3.0 - math.sqrt(5.0)))
        rho = np.sqrt(np.maximum(0.0, 1.0 - z * z))
        return cls(np.stack([rho * np.cos(az), rho * np.sin(az), z], 1))


def _positions(positions, who):
    r = np.array(positions, dtype=np.float64)
    if r.ndim != 2 or r.shape[1] != 3 or not 2 <= r.shape[0] <= MAX_CHANNELS:
        raise ValueError(f"{who}: positions must be [C, 3] metres with 2 <= C <= {MAX_CHANNELS} microphones, got shape {r.shape}")
    if not np.isfinite(r).all():
        raise ValueError(f"{who}: positions must be finite")
    return r


def _pairs(C):
    return [(i, j) for i in range(C) for j in range(i + 1, C)]


def steering_lags(positions, grid, sr, c=SPEED_OF_SOUND):
    """``tau`` float64 [D, P]: the lag, in samples at rate ``sr`` and in the sign of ``event_tdoa`` (channel j delayed by n
    samples gives -n), that a far-field source in direction ``grid.unit_vectors[d]`` produces in the pair p = (i, j), i < j in
    lexicographic order, of microphones at ``positions`` [C, 3] (metres): ``sr (r_j - r_i) . u_d / c``"""
    r = _positions(positions, "steering_lags")
    if not isinstance(grid, DirectionGrid):
        raise TypeError(f"steering_lags: grid must be a DirectionGrid, got {type(grid).__name__}")
    if not float(sr) > 0 or not float(c) > 0 or not math.isfinite(float(sr)) or not math.isfinite(float(c)):
        raise ValueError(f"steering_lags needs sr > 0 and c > 0, got {sr}, {c}")
    base = np.stack([r[j] - r[i] for i, j in _pairs(r.shape[0])])                  # [P, 3]
    return float(sr) * (grid.unit_vectors @ base.T) / float(c)


def trig_table(oversample):
    """float32 [512 Q + 1, 2]: ``(cos, sin)(2 pi k / (2048 Q))``, the quarter wave doa.hip unfolds; float64 values rounded once,
    by the expression that makes the pairing twiddles of the log-mel tables (at Q = 1 the same values)"""
    n = 2048 * int(oversample)
    two_pi = 6.283185307179586476925286766559
    a = [two_pi * float(k) / float(n) for k in range(n // 4 + 1)]
    return np.array([[math.cos(x), math.sin(x)] for x in a], dtype=np.float64).astype(np.float32)


# ── direction tracks ──
TRACK_CHUNK = 32               # tdoa.hip: TD_CHUNK, the located frames of one chunk partial
TRACK_MAX_BLOCK_CHUNKS = 64    # doatrack.hip: TRK_MAX_W
TRACK_MAX_BLOCKS = 256         # doatrack.hip: TRK_MAX_BLOCKS


@dataclasses.dataclass(frozen=True)
class DirectionTrack:
    """Settings of a direction track (``sed.DOA(positions, grid, ..., track=DirectionTrack(...))``): every located
    event also gets a direction per block of ``block_chunks`` = W chunks of 32 located frames (``track_blocks``), for a source
    that moves while it sounds.  ``max_step_deg``: None — every block's direction is the maximum of its own map — or a finite
    angle in (0, 180]: the directions are the best path through the block maps that turns by at most this much from one block to
    the next (``track_neighbours``), which does not jump to a reflection for the length of one block."""
    block_chunks: int = 1
    max_step_deg: typing.Optional[float] = None

    def __post_init__(self):
        w = self.block_chunks
        if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= int(w) <= TRACK_MAX_BLOCK_CHUNKS:
            raise ValueError(f"DirectionTrack: block_chunks must be an integer in [1, {TRACK_MAX_BLOCK_CHUNKS}], got {w!r}")
        object.__setattr__(self, "block_chunks", int(w))
        s = self.max_step_deg
        if s is not None:
            if isinstance(s, bool) or not isinstance(s, (int, float, np.floating, np.integer)) or not math.isfinite(float(s)) \
                    or not 0.0 < float(s) <= 180.0:
                raise ValueError(f"DirectionTrack: max_step_deg must be None or a finite angle in (0, 180] degrees, got {s!r}")
            object.__setattr__(self, "max_step_deg", float(s))

    def max_blocks(self, max_frames):
        """``Tm``: the most blocks an event located on up to ``max_frames`` frames has, ``ceil(ceil(max_frames / 32) / W)``"""
        return -(-(-(-int(max_frames) // TRACK_CHUNK)) // self.block_chunks)


def track_blocks(nf, block_chunks):
    """The blocks of an event located on ``nf`` frames, with W = ``block_chunks`` (doatrack.hip applies the same rule)
    -> ``(T, first_frame [T], n_frames [T])``, the frames counted from the event's first.  ``nch = ceil(nf / 32)``,
    ``T0 = ceil(nch / W)``, ``nl = nf - 32 W (T0 - 1)``; a last block of fewer than ``16 W`` frames joins the block before it
    (``T = T0 - 1`` where ``T0 > 1`` and ``nl < 16 W``).  ``nf = 0`` has no blocks."""
    nf, W = int(nf), int(block_chunks)
    if nf < 0 or not 1 <= W <= TRACK_MAX_BLOCK_CHUNKS:
        raise ValueError(f"track_blocks needs nf >= 0 and 1 <= block_chunks <= {TRACK_MAX_BLOCK_CHUNKS}, got {nf}, {block_chunks}")
    if nf == 0:
        return 0, np.zeros(0, np.int64), np.zeros(0, np.int64)
    step = TRACK_CHUNK * W
    nch = -(-nf // TRACK_CHUNK)
    T0 = -(-nch // W)
    T = T0 - 1 if T0 > 1 and nf - step * (T0 - 1) < step // 2 else T0
    first = step * np.arange(T, dtype=np.int64)
    n = np.full(T, step, np.int64)
    n[-1] = nf - first[-1]
    return T, first, n


def track_neighbours(grid, max_step_deg):
    """The directions a path may come to direction d from -> ``(off int32 [D + 1], idx int32 [nnz])``: row d,
    ``idx[off[d]:off[d + 1]]``, lists in ascending order every d' with ``arccos(clip(u_d . u_d', -1, 1)) <=
    radians(max_step_deg) + 1e-9`` in float64; it always contains d."""
    if not isinstance(grid, DirectionGrid):
        raise TypeError(f"track_neighbours: grid must be a DirectionGrid, got {type(grid).__name__}")
    s = max_step_deg
    if isinstance(s, bool) or not isinstance(s, (int, float, np.floating, np.integer)) or not math.isfinite(float(s)) or not 0.0 < float(s) <= 180.0:
        raise ValueError(f"track_neighbours: max_step_deg must be a finite angle in (0, 180] degrees, got {s!r}")
    u, bound = grid.unit_vectors, math.radians(float(s)) + 1e-9
    D = u.shape[0]
    off, rows = np.zeros(D + 1, np.int64), []
    for d0 in range(0, D, 1024):                                  # (1024 rows of the D x D angles at a time)
        near = np.arccos(np.clip(u[d0:d0 + 1024] @ u.T, -1.0, 1.0)) <= bound
        near[np.arange(near.shape[0]), d0 + np.arange(near.shape[0])] = True
        r, c = np.nonzero(near)                                   # row-major: ascending within a row
        rows.append(c)
        off[d0 + 1:d0 + 1 + near.shape[0]] = np.bincount(r, minlength=near.shape[0])
    off = np.cumsum(off)
    assert off[-1] < 2 ** 31
    return off.astype(np.int32), np.ascontiguousarray(np.concatenate(rows).astype(np.int32))


# ── contrast SRP-PHAT ──
CONTRAST_MAX_FRAMES = 256      # contrast.hip: CT_MAX_FRAMES
CONTRAST_MAX_SEARCH = 4096     #               CT_MAX_SEARCH
CONTRAST_MAX_GUARD = 64        #               CT_MAX_GUARD
CONTRAST_MAX_CLASSES = 32      #               CT_MAX_CLASSES, the bits of an activity word
CONTRAST_MAX_WEIGHT = 4.0      #               CT_MAX_WEIGHT


@dataclasses.dataclass(frozen=True)
class Contrast:
    """Settings of contrast SRP-PHAT (``sed.DOA(positions, grid, ..., contrast=Contrast(...))``): the direction of an event
    that sounds over a louder source of another class.  PHAT whitening gives every frequency bin to whichever source is loudest
    in it, so the plain map of such an event peaks at the louder source.  In feature frames before the onset in which the
    event's own class is silent that source sounds and the event does not: their summed whitened cross spectrum ``Sb``, scaled
    to the event's frames, is subtracted from the event's ``S`` before the map is steered, ``S' = S - weight (nf / nb) Sb``.
    The bins the other source wins cancel, the bins the event wins stay.

    Candidate q = 0 .. ``search`` - 1 is feature frame ``onset * tf - guard - 1 - q``; it is eligible when no row of the event
    table with the event's class is active in an output frame its 2048 samples touch (other classes never block a candidate:
    they are what is subtracted).  The ``frames`` nearest eligible candidates make ``Sb``, as long as there are at least
    ``min_frames`` of them — else the event's map is the plain one, bit for bit.  ``frames`` in [1, 256], ``search`` in
    [``frames``, 4096], ``guard`` in [0, 64], ``min_frames`` in [1, ``frames``], ``weight`` finite in (0, 4].  ``bg_frames`` in the
    results is the number of frames used and ``bg_sel`` [E, frames] lists their q in summation order (-1 behind them).  The
    events need ``cls`` and the calls the number of classes.  Offline only."""
    frames: int = 32
    search: int = 256
    guard: int = 2
    min_frames: int = 8
    weight: float = 1.0

    def __post_init__(self):
        for name, least, most in (("frames", 1, CONTRAST_MAX_FRAMES), ("search", 1, CONTRAST_MAX_SEARCH), ("guard", 0, CONTRAST_MAX_GUARD),
                                  ("min_frames", 1, CONTRAST_MAX_FRAMES)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not least <= int(v) <= most:
                raise ValueError(f"Contrast: {name} must be an integer in [{least}, {most}], got {v!r}")
            object.__setattr__(self, name, int(v))
        if self.search < self.frames:
            raise ValueError(f"Contrast: search must be at least frames = {self.frames}, got {self.search}")
        if self.min_frames > self.frames:
            raise ValueError(f"Contrast: min_frames must be at most frames = {self.frames}, got {self.min_frames}")
        w = self.weight
        if isinstance(w, bool) or not isinstance(w, (int, float, np.floating, np.integer)) or not math.isfinite(float(w)) \
                or not 0.0 < float(w) <= CONTRAST_MAX_WEIGHT:
            raise ValueError(f"Contrast: weight must be a finite number in (0, {CONTRAST_MAX_WEIGHT:g}], got {w!r}")
        object.__setattr__(self, "weight", float(w))


class DOA:
    """Settings of per-event direction of arrival (``EventDetector(model, ..., localize=DOA(positions, grid))``):
    steered response power (SRP-PHAT) over ``grid`` for the microphones at ``positions`` [C, 3] (metres, in the order of the
    audio channels).  ``oversample`` Q in {1, 2, 4, 8, 16}: the correlation of every pair is evaluated at lags of 1/Q sample,
    exactly.  ``max_frames`` as in ``TDOA``; ``max_lag`` follows from the array: ``max_lag_for`` of its largest spacing at the
    detector's rate, which must not exceed 127 samples.  ``c``: the speed of sound in m/s.  A detector with these settings
    also returns everything a ``TDOA(max_lag, max_frames)`` detector returns.  ``track``: None, or a ``DirectionTrack``: every
    event also gets a direction per block of its located frames.  ``contrast``: None, or a ``Contrast``: the map of
    every event — and of every block — is made after the share of the sources that sound before its onset is removed."""

    def __init__(self, positions, grid, max_frames=256, oversample=8, c=SPEED_OF_SOUND, track=None, contrast=None):
        r = _positions(positions, "DOA")
        if not isinstance(grid, DirectionGrid):
            raise TypeError(f"DOA: grid must be a DirectionGrid, got {type(grid).__name__}")
        for name, v in (("max_frames", max_frames), ("oversample", oversample)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"DOA: {name} must be an integer, got {v!r}")
        if int(max_frames) < 1:
            raise ValueError(f"DOA: max_frames must be >= 1, got {max_frames}")
        if int(oversample) not in OVERSAMPLE_CHOICES:
            raise ValueError(f"DOA: oversample must be one of {OVERSAMPLE_CHOICES}, got {oversample}")
        if not (isinstance(c, (int, float, np.floating, np.integer)) and math.isfinite(float(c)) and float(c) > 0):
            raise ValueError(f"DOA: the speed of sound c must be a positive number, got {c!r}")
        dist = np.array([np.linalg.norm(r[j] - r[i]) for i, j in _pairs(r.shape[0])])
        if dist.min() <= 0.0:
            i, j = _pairs(r.shape[0])[int(dist.argmin())]
            raise ValueError(f"DOA: microphones {i} and {j} are at the same position")
        if track is not None:
            if not isinstance(track, DirectionTrack):
                raise TypeError(f"DOA: track must be None or a DirectionTrack(...), got {type(track).__name__}")
            if track.max_blocks(max_frames) > TRACK_MAX_BLOCKS:
                raise ValueError(f"DOA: max_frames={max_frames} in blocks of {track.block_chunks} chunks is {track.max_blocks(max_frames)} "
                                 f"blocks an event, more than {TRACK_MAX_BLOCKS}; use a larger block_chunks")
            self._neighbours, self._neighbours_device = {}, {}   # per max_step_deg: track_neighbours of the grid; per device: its copy
        self.track = track
        if contrast is not None and not isinstance(contrast, Contrast):
            raise TypeError(f"DOA: contrast must be None or a Contrast(...), got {type(contrast).__name__}")
        self.contrast = contrast
        r.setflags(write=False)
        self.positions, self.grid = r, grid
        self.max_frames, self.oversample, self.c = int(max_frames), int(oversample), float(c)
        self.aperture = float(dist.max())
        self._plans, self._device = {}, {}                   # per rate: (max_lag, J, table); per (device, rate): their device copies
        self._delays, self._beam_device = {}, {}             # per (rate, Q): M of steering_delays; per (device, rate, Q): its device copy
        self._steering, self._steering_device = {}, {}       # per rate: steering_delays in float64; per (device, rate): its device copy

    @property
    def channels(self):
        return self.positions.shape[0]

    def max_lag(self, sr):
        """``max_lag_for`` of the largest spacing at rate ``sr``; more than 127 samples is refused"""
        ml = max_lag_for(self.aperture, sr, self.c)
        if ml > MAX_LAG_LIMIT:
            raise ValueError(f"DOA: an aperture of {self.aperture:.4g} m is {ml} samples at {sr} Hz (c = {self.c:g} m/s): more than the "
                             f"{MAX_LAG_LIMIT} that are searched; use a smaller array or a lower rate")
        return ml

    def plan(self, sr):
        """-> (max_lag, J int32 [D, P], trig float32 [512 Q + 1, 2]) at rate ``sr``: ``J = round_half_even(tau Q)``, every
        ``|J| <= max_lag Q`` by construction"""
        key = float(sr)
        if key not in self._plans:
            ml = self.max_lag(sr)
            J = np.rint(steering_lags(self.positions, self.grid, sr, self.c) * self.oversample).astype(np.int32)
            assert np.abs(J).max() <= ml * self.oversample
            self._plans[key] = (ml, np.ascontiguousarray(J), trig_table(self.oversample))
        return self._plans[key]

    def delays(self, sr, oversample):
        """``M`` int32 [D, C] at rate ``sr``: ``round_half_even(steering_delays * oversample)``, the delay of every microphone
        for every direction in 1/oversample samples; every ``|M| <= max_lag * oversample`` by construction"""
        key = (float(sr), int(oversample))
        if key not in self._delays:
            ml = self.max_lag(sr)
            M = np.rint(steering_delays(self.positions, self.grid, sr, self.c) * int(oversample)).astype(np.int32)
            assert np.abs(M).max() <= ml * int(oversample)
            self._delays[key] = np.ascontiguousarray(M)
        return self._delays[key]

    def steering(self, sr):
        """``steering_delays`` of the array at rate ``sr``: float64 [D, C] in samples, not rounded, cached per rate"""
        key = float(sr)
        if key not in self._steering:
            self.max_lag(sr)
            self._steering[key] = np.ascontiguousarray(steering_delays(self.positions, self.grid, sr, self.c))
        return self._steering[key]

    def tdoa(self, sr):
        """the ``TDOA`` settings whose outputs a detector with these settings also returns"""
        return TDOA(self.max_lag(sr), self.max_frames)

    def neighbours(self):
        """``track_neighbours`` of the grid for the track's ``max_step_deg``, cached; None without smoothing"""
        if self.track is None or self.track.max_step_deg is None:
            return None
        key = self.track.max_step_deg
        if key not in self._neighbours:
            self._neighbours[key] = track_neighbours(self.grid, key)
        return self._neighbours[key]

    def __repr__(self):
        return (f"DOA({self.channels} microphones, aperture {self.aperture:.4g} m, {len(self.grid)} directions, max_frames={self.max_frames}, "
                f"oversample={self.oversample}, c={self.c:g}" + (f", track={self.track!r}" if self.track is not None else "") +
                (f", contrast={self.contrast!r}" if self.contrast is not None else "") + ")")


# ── the audio of a located event: a steered delay-and-sum beam ──
BEAM_OVERSAMPLE_CHOICES = (1, 2, 4, 8, 16, 32, 64)
BEAM_MAX_HALF_WIDTH = 32   # beam.hip: BM_MAX_H


@dataclasses.dataclass(frozen=True)
class DelaySum:
    """Settings of per-event audio extraction (``EventDetector(model, ..., localize=DOA(...), extract=DelaySum(...))``):
    every located event's samples with the array pointed at the event's direction, each channel shifted by its delay and the
    channels averaged.  ``oversample`` Q in {1, 2, 4, 8, 16, 32, 64}: delays are applied in steps of 1/Q sample.
    ``half_width`` H in 1..32: the fractional-delay filter has 2H taps.  ``beta >= 0``: its Kaiser window."""
    oversample: int = 16
    half_width: int = 16
    beta: float = 10.0

    def __post_init__(self):
        for name in ("oversample", "half_width"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"DelaySum: {name} must be an integer, got {v!r}")
            object.__setattr__(self, name, int(v))
        if self.oversample not in BEAM_OVERSAMPLE_CHOICES:
            raise ValueError(f"DelaySum: oversample must be one of {BEAM_OVERSAMPLE_CHOICES}, got {self.oversample}")
        if not 1 <= self.half_width <= BEAM_MAX_HALF_WIDTH:
            raise ValueError(f"DelaySum: half_width must be in 1..{BEAM_MAX_HALF_WIDTH}, got {self.half_width}")
        b = self.beta
        if isinstance(b, bool) or not isinstance(b, (int, float, np.floating, np.integer)) or not math.isfinite(float(b)) or float(b) < 0:
            raise ValueError(f"DelaySum: beta must be a finite number >= 0, got {b!r}")
        object.__setattr__(self, "beta", float(b))

    @property
    def taps(self):
        """``beam_taps`` of these settings: float32 [Q, 2H], read-only"""
        return beam_taps(self.oversample, self.half_width, self.beta)


@functools.lru_cache(maxsize=32)
def beam_taps(oversample, half_width, beta):
    """float32 [Q, 2H]: row p evaluates a channel at ``m + p/Q``, ``x(m + p/Q) = sum_k taps[p][k] x[m + k - H + 1]``.
    ``resample.design_taps(Q, H, 1.0, beta)`` in float64 (a Kaiser-windowed sinc); row 0 is replaced by the exact unit impulse
    (1 at column H - 1), every other row is divided by its float64 sum (unit gain at DC), and the table is rounded once."""
    from .resample import design_taps
    Q, H = int(oversample), int(half_width)
    t = design_taps(Q, H, 1.0, float(beta))
    t[0] = 0.0
    t[0, H - 1] = 1.0
    t[1:] /= t[1:].sum(1, keepdims=True)
    t = np.ascontiguousarray(t.astype(np.float32))
    t.setflags(write=False)
    return t


MVDR_BLOCK = 1024               # mvdr.hip: MV_B, the hop of an event's own transform grid
MVDR_MAX_NOISE_BLOCKS = 256     # mvdr.hip: MV_MAX_NOISE
MVDR_MAX_NOISE_GUARD = 64       # mvdr.hip: MV_MAX_GUARD
MVDR_MAX_NOISE_SEARCH = 1024    # mvdr.hip: MV_MAX_SEARCH
MVDR_MAX_CLASSES = 32           # mvdr.hip: MV_MAX_CLASSES, the bits of an activity word


@dataclasses.dataclass(frozen=True)
class MVDR:
    """Settings of per-event audio extraction by an adaptive beam (``EventDetector(model, ..., localize=DOA(...), extract=MVDR(...))``;
    DESIGN 5s): the events and samples of ``DelaySum``, but per frequency bin the channel weights that pass the event's direction
    unchanged and let through the least of everything else the event's own frames contain (minimum variance distortionless
    response).  ``loading`` in [1e-6, 1e6]: ``loading * trace(R) / C`` is added to the diagonal of every bin's covariance R before
    the solve; small values adapt hard (and need more frames than microphones to estimate R), large ones approach the plain
    average of the steered channels.

    ``noise_blocks`` Kn in 0..256 and ``noise_guard`` G in 0..64, in blocks of 1024 samples: with ``Kn >= 1`` the
    covariance is not the event's own — which holds the target, so that any steering error makes the beam cancel part of it —
    but that of the Kn frames of 2048 samples before the onset, ``[s0 - (G + Kn + 1) 1024, s0 - G 1024)`` of the recording.  An
    event that starts earlier than ``(G + Kn + 1) 1024`` samples into its recording keeps its own covariance, wholly;
    ``noise_frames`` in the results says which events used which (Kn or 0).  ``Kn = 0``: the own frames, for every event.  On
    live feeds the ring keeps ``stream_noise_frames`` more feature frames.

    ``noise_select="quiet"`` (needs ``Kn >= 1``) picks the Kn frames by the detector's own class tracks instead of
    taking one fixed stretch: candidate q = 0.. ``noise_search`` - 1 is the 2048 samples from ``s0 - (G + 2 + q) 1024``; it is
    eligible when no event of the table with the event's class (``noise_exclude="same"``; ``"any"``: with any class) is active
    in an output frame that the candidate, widened by G blocks on either side, touches; the Kn nearest eligible candidates make
    the covariance, as long as there are at least ``noise_min`` of them — else the event keeps its own frames.  A repeated
    source, an event longer than ``max_frames`` and an event near the start of its recording then still get a covariance
    without the target in it.  ``noise_search = 0`` means ``min(1024, 4 Kn)`` and is stored resolved; ``noise_frames`` in the
    results is the number of frames used and ``noise_sel`` [E, Kn] lists their q in summation order (-1 behind them).  An
    event whose Kn nearest candidates are all eligible gets the audio of ``noise_select="fixed"``, bit for bit.  Offline only.

    ``follow_track=True`` (needs ``DOA(..., track=DirectionTrack(...))``): the beam follows a source that moves while it
    sounds.  The samples, the covariance and the transform grid stay what they are; frame j of an event is combined with weights
    steered at the direction of the track block it lies in (``mvdr_frame_blocks``; ``trk_dir`` of the events), one weight set per
    block from the event's one covariance, and the sqrt-Hann overlap-add cross-fades from one block's beam to the next.  A silent
    block and an event without a track keep ``dir``.  Offline, in batches and on live feeds; ``False``: every bit as before."""
    loading: float = 1e-2
    noise_blocks: int = 0
    noise_guard: int = 1
    noise_select: str = "fixed"
    noise_search: int = 0
    noise_min: int = 1
    noise_exclude: str = "same"
    follow_track: bool = False

    def __post_init__(self):
        if not isinstance(self.follow_track, (bool, np.bool_)):
            raise ValueError(f"MVDR: follow_track must be a bool, got {self.follow_track!r}")
        object.__setattr__(self, "follow_track", bool(self.follow_track))
        v = self.loading
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 1e-6 <= float(v) <= 1e6:
            raise ValueError(f"MVDR: loading must be a number in [1e-6, 1e6], got {v!r}")
        object.__setattr__(self, "loading", float(v))
        for name, most in (("noise_blocks", MVDR_MAX_NOISE_BLOCKS), ("noise_guard", MVDR_MAX_NOISE_GUARD)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= most:
                raise ValueError(f"MVDR: {name} must be an integer in [0, {most}], got {v!r}")
            object.__setattr__(self, name, int(v))
        for name, allowed in (("noise_select", ("fixed", "quiet")), ("noise_exclude", ("same", "any"))):
            if getattr(self, name) not in allowed:
                raise ValueError(f"MVDR: {name} must be one of {allowed}, got {getattr(self, name)!r}")
        for name, least, most in (("noise_search", 0, MVDR_MAX_NOISE_SEARCH), ("noise_min", 1, MVDR_MAX_NOISE_BLOCKS)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not least <= int(v) <= most:
                raise ValueError(f"MVDR: {name} must be an integer in [{least}, {most}], got {v!r}")
            object.__setattr__(self, name, int(v))
        if self.quiet:
            Kn = self.noise_blocks
            if Kn < 1:
                raise ValueError("MVDR: noise_select='quiet' selects among pre-onset frames and needs noise_blocks >= 1")
            if self.noise_search == 0:
                object.__setattr__(self, "noise_search", min(MVDR_MAX_NOISE_SEARCH, 4 * Kn))
            if self.noise_search < Kn:
                raise ValueError(f"MVDR: noise_search must be 0 or at least noise_blocks = {Kn}, got {self.noise_search}")
            if self.noise_min > Kn:
                raise ValueError(f"MVDR: noise_min must be at most noise_blocks = {Kn}, got {self.noise_min}")

    @property
    def quiet(self):
        """whether the noise frames are picked by the class tracks (``noise_select="quiet"``)"""
        return self.noise_select == "quiet"

    @property
    def noise_lead_blocks(self):
        """``G + Kn + 1``: an event uses the noise covariance iff it starts at least this many blocks of 1024 samples into its
        recording; 0 with ``noise_blocks = 0``"""
        return self.noise_guard + self.noise_blocks + 1 if self.noise_blocks else 0


def mvdr_frame_blocks(length, hop_length, block_chunks, n_blocks):
    """The track block every frame of an MVDR beam with ``follow_track=True`` takes its weights from (mvdr.hip applies
    the same rule) -> int64 [J + 1], ``J = ceil(length / 1024)``: an event of ``length`` samples has the frames j = 0..J, the
    centre of frame j is sample ``j * 1024`` of the event, which lies in located frame ``j * 1024 // hop_length`` and that in block
    ``(j * 1024 // hop_length) // (32 * block_chunks)`` of the track; frame J and the short tail that ``track_blocks`` joins to the
    last block take block ``T - 1``, T = ``n_blocks``.  ``n_blocks = 0`` — an event without a track — is a row of zeros: the one
    weight set steered at ``dir``."""
    length, hop, W, T = int(length), int(hop_length), int(block_chunks), int(n_blocks)
    if length < 0 or hop < 1 or not 1 <= W <= TRACK_MAX_BLOCK_CHUNKS or not 0 <= T <= TRACK_MAX_BLOCKS:
        raise ValueError(f"mvdr_frame_blocks needs length >= 0, hop_length >= 1, 1 <= block_chunks <= {TRACK_MAX_BLOCK_CHUNKS} and "
                         f"0 <= n_blocks <= {TRACK_MAX_BLOCKS}, got {length}, {hop_length}, {block_chunks}, {n_blocks}")
    j = np.arange(-(-length // MVDR_BLOCK) + 1, dtype=np.int64)
    return np.minimum((j * MVDR_BLOCK // hop) // (TRACK_CHUNK * W), max(T - 1, 0))


@functools.lru_cache(maxsize=1)
def mvdr_window():
    """float32 [2048]: ``sqrt(0.5 - 0.5 cos(2 pi m / 2048))`` in float64, rounded once; analysis and synthesis window of the MVDR
    beam (``w[m]^2 + w[m + 1024]^2 = 1``), read-only"""
    m = np.arange(2048, dtype=np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * m / 2048.0)).astype(np.float32)
    w.setflags(write=False)
    return w


def steering_delays(positions, grid, sr, c=SPEED_OF_SOUND):
    """``tau`` float64 [D, C]: channel c hears a far-field source in direction ``grid.unit_vectors[d]`` as ``s[n + tau[d][c]]``,
    ``tau = sr (r_c - rbar) . u_d / c`` in samples at rate ``sr``, ``rbar`` the centroid of the microphones (the delays of a
    direction sum to 0); ``tau[d][j] - tau[d][i]`` is ``steering_lags`` of the pair (i, j)"""
    r = _positions(positions, "steering_delays")
    if not isinstance(grid, DirectionGrid):
        raise TypeError(f"steering_delays: grid must be a DirectionGrid, got {type(grid).__name__}")
    if not float(sr) > 0 or not float(c) > 0 or not math.isfinite(float(sr)) or not math.isfinite(float(c)):
        raise ValueError(f"steering_delays needs sr > 0 and c > 0, got {sr}, {c}")
    return float(sr) * (grid.unit_vectors @ (r - r.mean(0)).T) / float(c)


def event_samples(onset, offset, peak_frame, time_factor, n, hop, max_frames, direction, loc_frames):
    """The samples ``[s0, s1)`` of a recording of ``n`` samples that the audio of an event consists of (the kernels of
    beam.hip apply the same rule).  An event is extracted iff ``direction >= 0`` (``dir`` of ``events.event_doa``); it was then
    located on the frames ``[f0, f0 + loc_frames)`` with ``f0`` from ``event_frames`` (``n_feat = 1 + n // hop``;
    ``loc_frames`` is read as at most that range), and ``[s0, s1) = [f0 * hop, min((f0 + loc_frames) * hop, n))``.  An event
    that is not extracted — unlocated, beyond its recording, digital silence, refused by a stream's ring rule — and one whose
    frames start at or beyond sample ``n`` have no samples: ``(0, 0)``.  These are the samples the audio consists of; an
    ``MVDR`` beam with ``noise_blocks = Kn >= 1`` also READS ``[s0 - (G + Kn + 1) 1024, s0 - G 1024)`` of the recording for the
    weights of an event with ``s0 >= (G + Kn + 1) 1024``, which adds no sample to its audio."""
    n, hop = int(n), int(hop)
    if n < 0 or hop < 1:
        raise ValueError(f"event_samples needs n >= 0 and hop >= 1, got {n}, {hop}")
    if int(direction) < 0:
        return 0, 0
    f0, f1 = event_frames(onset, offset, peak_frame, time_factor, 1 + n // hop, max_frames)
    nf = min(max(int(loc_frames), 0), f1 - f0)
    s0, s1 = f0 * hop, min((f0 + nf) * hop, n)
    return (s0, s1) if s1 > s0 else (0, 0)
