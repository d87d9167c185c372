"""Live streams: stateful incremental event detection for S feeds at once.

A stream gives exactly what the offline path gives on the concatenation of everything it received — ``det(wave)`` /
``det.from_features(mel)`` — whatever the chunking.  That is possible because every quantity has a rule for when it is FINAL:

* feature frame f (centre f*hop_length) is final once its ``n_fft`` samples are there: ``f*hop_length + n_fft/2 <= n``, that is
  ``f < n // hop_length`` at the reference settings; the right-padded frames up to ``n // hop_length`` come at ``flush``;
* with ``N`` final feature frames, ``n_out = N // tf`` and ``win_out = seq_len // tf``: track frame j is final iff
  ``j < n_out - win_out`` (every window that covers it is complete, exists in the offline grid and keeps its right ``trim``);
* filtered frame g is decided once track frame ``g + median // 2`` is final;
* a pending event [a, b) is emitted in the first step in which more than ``b + min_gap`` frames are decided and no run that
  began at or before ``b + min_gap`` is still open.

A class-wise detector (``EventDetector(..., median=[...])``) streams with ONE frontier per feed:

* filtered frame g of EVERY class is decided once track frame ``g + R`` is final, ``R = max_k median_k // 2``: the state and the
  schedule are sized with the widest median, and class k's filter (width ``median_k <= 2R + 1``) reads final frames only;
* a pending event [a, b) of class k is emitted in the first step in which more than ``b + min_gap_k`` frames are decided and no
  run of class k that began at or before ``b + min_gap_k`` is still open.

A class with a narrow filter therefore becomes final ``R - median_k // 2`` output frames later than it strictly could: the
price of per-feed state of constant size and a step that stays one kernel sequence.  Over a feed's life the events are exactly
the offline class-wise decode of the whole track.

``flush`` ends streams: the offline grid's last window (end-aligned, or one short sequence) runs, everything left is emitted and
the streams restart at frame 0.  Between calls everything lives on the device, in buffers whose size depends on ``seq_len``,
``hop``, ``median``, ``max_new_windows`` and S only; a long push is split into steps of at most ``max_new_windows`` windows per
stream.  The host keeps the counters of all streams as arrays, so a push costs no Python per stream beyond reading its list of
pieces.  There is no CPU fallback.

A net with ``in_channels = C > 1`` takes ``[n, C]`` interleaved pieces: the resampling stage is then always on (the
one-tap copy filter at the detector's own rate) and emits C planar lanes per feed; lane ``s*C + c`` has its own resampler
carry and its own log-mel PCM carry on the device, while the host counters stay per feed (the channels of a feed advance in
lockstep), and a round's features come out of ``sed_logmel_multi`` as ``[rows, C*F]``, which is what the feature rows hold.
A spatial detector (``EventDetector(..., spatial="gcc_phat")``) keeps the same C lanes per feed and calls
``sed_logmel_gcc`` instead: ``[rows, (C+P)*F]`` with one GCC-PHAT block per microphone pair, and no further state.
A detector with ``compress=PCEN(...)`` adds one ``sed_pcen`` call per round over the new rows of all feeds, with
the feed's feature-frame counter as the absolute frame index; the smoother's state, two floats per feed and mel column, stays
on the device and is simply ignored when a feed's counter is back at 0 (``flush`` / ``reset`` need nothing more).
A detector with ``localize=sed.TDOA(...)`` streams when given ``history_frames``: every lane then also keeps its
last ``cap`` samples in a ring on the device (``sed_stream_ring_write``, one launch per round), and a step that emits events
locates them from the rings in one ``sed_event_tdoa_ring`` call — an event ``[a, b)`` with frames from ``f0`` iff ``b*tf + lat - f0
<= history_frames`` (``localize.stream_locates``), with the bits of the offline call; ``flush`` / ``reset`` need no ring work either.
With ``localize=sed.DOA(...)`` that call is ``sed_event_doa_ring`` and the events also carry ``dir`` and ``doa_power``
(``StreamEvents.doa()``); an event the rule refuses has ``dir = -1``.  With ``sed.DOA(..., track=sed.DirectionTrack(...))`` (DESIGN
5x) the call is ``sed_event_doa_track_ring`` and the events also carry a direction per block (``StreamEvents.doa_track(e)``); no new
state is kept, and an event the rule refuses has ``trk_len = 0``.
With ``extract=sed.DelaySum(...)`` or ``sed.MVDR(...)`` and ``emit_audio=True`` a step that emitted events makes one
more call on the same rings, ``events.event_beamform_ring`` or ``events.event_mvdr_ring``: the events carry ``audio_start`` and
``audio_len`` (and, with ``sed.MVDR(noise_blocks >= 1)``, ``noise_frames``: DESIGN 5u) and the call's ``StreamEvents.audio`` holds
every located event's audio, the offline call's bit for bit.  Nothing
of it persists between calls: the steps of one push hand their buffers to ``merge_step_audio``.
"""
import ctypes as C

import numpy as np
import torch

from . import feature
from ._lib import SedHipError, check, lib, ptr, stream_ptr
from .detect import (_BEAM_KEYS, _DOA_KEYS, _NOISE_KEYS, _TDOA_KEYS, _TRACK_KEYS, EventDetector, _doa_angles, _doa_track, _event_audio, _event_tensors, _intervals,
                     _noise_frames, _timed, _window_jobs, plan_windows)
from .events import _beam_empty, _mvdr_empty, event_beamform_ring, event_doa_ring, event_mvdr_ring, event_tdoa_ring, ring_write

_KEYS = ("stream", "cls", "onset", "offset", "peak", "peak_frame")


def _excl(x):
    """exclusive prefix sums"""
    return np.cumsum(x) - x


def merge_step_audio(parts):
    """The extracted audio of several steps of one call as one table.  ``parts``: per step, in step order,
    ``(audio float32 [n_i], audio_start int64 [E_i], audio_len int32 [E_i])`` — tensors on one device, host or GPU — where the
    slices of a step are disjoint and cover its ``audio``.  -> ``(audio, audio_start, audio_len)``: the buffers back to back and
    every step's ``audio_start`` moved by the samples of the steps before it, so the slices stay disjoint and cover the joined
    buffer; lengths, zero ones included, are unchanged.  The host knows every ``n_i`` already: nothing is read back."""
    base = _excl(np.asarray([int(p[0].numel()) for p in parts], np.int64))
    return (torch.cat([p[0] for p in parts]), torch.cat([p[1] + int(b) for p, b in zip(parts, base)]),
            torch.cat([p[2] for p in parts]))


class StreamSchedules:
    """The host arithmetic of n streams as int64 arrays (input frames unless named ``*_out``): which windows are due after
    every advance, and how many output frames are final / decided.  Per stream, over the advances up to the one that ends it,
    the windows are exactly ``plan_windows(N, ...).starts``, each once (``StreamSchedule`` is the one-stream view)."""

    def __init__(self, tf, seq_len, hop, trim=0, median=1, n=1):
        plan_windows(4 * int(seq_len), tf, seq_len, hop, trim)            # the detector's own checks and messages
        self.tf, self.L, self.trim = int(tf), int(seq_len), int(trim)
        self.hop = self.L // 2 if hop is None else int(hop)
        self.win_out, self.hop_out, self.r = self.L // self.tf, self.hop // self.tf, int(median) // 2
        self.N = np.zeros(int(n), np.int64)            # final feature frames received
        self.n_win = np.zeros(int(n), np.int64)        # regular windows scheduled so far

    def reset(self, which):
        self.N[which] = 0
        self.n_win[which] = 0

    @property
    def n_out(self):
        return self.N // self.tf

    @property
    def final_frames(self):
        """output frames of the track that are final"""
        return np.maximum(0, self.n_out - self.win_out)

    @property
    def decided(self):
        """filtered frames that are decided (G)"""
        return np.maximum(0, self.final_frames - self.r)

    def keep_from(self):
        """the first feature frame that a window still to come (regular, or the one that ends the stream) can need"""
        return np.where(self.N < self.L, 0, np.minimum(self.n_win * self.hop, ((self.N - self.L) // self.tf) * self.tf))

    def advance(self, rows, end=None):
        """``rows`` [n] more final feature frames; the streams in the mask ``end`` end after them -> (index of the first new
        window, regular windows that completed, start of the window that ends the stream or -1, length of the new windows)"""
        first = self.n_win.copy()
        self.N = self.N + rows
        N, L = self.N, self.L
        self.n_win = np.where(N >= L, (N - L) // self.hop + 1, 0)
        extra, win_len = np.full(N.shape, -1, np.int64), np.full(N.shape, L, np.int64)
        if end is not None and end.any():
            last = ((N - L) // self.tf) * self.tf                           # the end-aligned window, unless the grid ends there
            need = end & (N >= L) & ((self.n_win - 1) * self.hop != last)
            extra[need] = last[need]
            short = end & (N < L)                                           # one sequence of tf * n_out frames
            extra[short] = 0
            win_len[short] = (N // self.tf * self.tf)[short]
        return first, self.n_win - first, extra, win_len


class StreamSchedule:
    """``StreamSchedules`` for one stream, in plain ints.  Over the advances plus ``finish`` the windows are exactly
    ``plan_windows(N, ...).starts``, each once."""

    def __init__(self, tf, seq_len, hop, trim=0, median=1):
        self._v = StreamSchedules(tf, seq_len, hop, trim, median, 1)
        self.tf, self.L, self.hop, self.trim = self._v.tf, self._v.L, self._v.hop, self._v.trim
        self.win_out, self.hop_out = self._v.win_out, self._v.hop_out

    def reset(self):
        self._v.reset(0)

    N = property(lambda self: int(self._v.N[0]))
    n_win = property(lambda self: int(self._v.n_win[0]))
    n_out = property(lambda self: int(self._v.n_out[0]))
    final_frames = property(lambda self: int(self._v.final_frames[0]))
    decided = property(lambda self: int(self._v.decided[0]))

    def keep_from(self):
        return int(self._v.keep_from()[0])

    def advance(self, n_frames):
        """``n_frames`` more final feature frames -> the starts of the regular windows that completed"""
        first, n, _, _ = self._v.advance(np.array([int(n_frames)], np.int64))
        return [w * self.hop for w in range(int(first[0]), int(first[0] + n[0]))]

    def finish(self):
        """the stream ends at N frames -> (starts still to run, their length, the offline WindowPlan); ValueError with
        ``plan_windows``' message when it is shorter than one output frame"""
        plan = plan_windows(self.N, self.tf, self.L, self.hop, self.trim)
        _, _, extra, win_len = self._v.advance(np.zeros(1, np.int64), np.ones(1, bool))
        return ([int(extra[0])] if extra[0] >= 0 else []), int(win_len[0]), plan


class StreamEvents:
    """What one ``push`` / ``push_features`` / ``flush`` made final.  ``events``: dict of device tensors ``stream``, ``cls``,
    ``onset``, ``offset`` (exclusive), ``peak_frame`` (int32 output frames from the start of the stream) and ``peak`` (float32),
    sorted by (stream, class, onset); ``event_offsets`` [S+1] host list (stream s = events [event_offsets[s],
    event_offsets[s+1])); ``final_frames`` [S] host list: output frames of each stream that are final after this call; with
    ``keep_probs``, ``probs`` [sum, K] = the newly final track rows, packed by stream, and ``prob_offsets`` [S+1].  From a stream
    with ``emit_audio=True`` the events also hold ``audio_start`` (int64) and ``audio_len`` (int32), and ``audio`` is
    the call's one packed float32 device buffer: event e is ``audio[audio_start[e] : audio_start[e] + audio_len[e]]``
    (``event_audio(e)``), length 0 where the event was not located.  The slices of one StreamEvents are disjoint and cover
    ``audio`` exactly; after a call that took several steps ``audio_start`` is NOT monotone in event order (the events are sorted
    by stream and class, the buffer is in step order)."""

    def __init__(self, events, event_offsets, final_frames, frame_seconds, probs=None, prob_offsets=None, sr=None, grid=None,
                 audio=None, track=None):
        self.events, self.event_offsets, self.final_frames = events, list(event_offsets), list(final_frames)
        self.frame_seconds, self.probs, self.prob_offsets = frame_seconds, probs, prob_offsets
        self.sr = sr                            # the detector's rate: set by a localising stream (lags are in samples at that rate)
        self.grid = grid                        # the DirectionGrid that ``dir`` indexes: set by a stream with DOA settings
        self.audio = audio                      # the packed extracted audio of this call: set by a stream with emit_audio=True
        self.track = track                      # as in DetectionResult: set by a stream with DOA(..., track=...) settings

    def __len__(self):
        return self.event_offsets[-1]

    def intervals(self, stream, k=0):
        """[(start_s, end_s, peak), ...] of class ``k`` of one stream, on the host"""
        e0, e1 = self.event_offsets[int(stream)], self.event_offsets[int(stream) + 1]
        return _intervals({n: v[e0:e1] for n, v in self.events.items()}, self.frame_seconds, k)

    def tdoa(self, stream=None):
        """time differences of arrival in seconds, a host array [E, P] (the events of one stream; None: all events, in event
        order), one column per microphone pair, as ``DetectionResult.tdoa``; an event that was not located (``loc_frames``
        0) has 0.  Only on what a localising stream returns (``det.stream(S, history_frames=...)``)."""
        if "lag" not in self.events or self.sr is None:
            raise ValueError("these events hold no lags: make the stream from EventDetector(..., localize=sed.TDOA(...)) with "
                             "det.stream(S, history_frames=...)")
        lag = self.events["lag"].cpu().numpy().astype(np.float64) / float(self.sr)
        return lag if stream is None else lag[self.event_offsets[int(stream)]:self.event_offsets[int(stream) + 1]]

    def doa(self, stream=None):
        """directions of arrival, a host array [E, 3] (the events of one stream; None: all events, in event order): azimuth,
        elevation (radians) and power, as ``DetectionResult.doa``; NaN where an event was not located.  Only on what a stream
        with ``localize=sed.DOA(...)`` returns."""
        if "dir" not in self.events or self.grid is None:
            raise ValueError("these events hold no directions: make the stream from EventDetector(..., localize=sed.DOA(...)) with "
                             "det.stream(S, history_frames=...)")
        out = _doa_angles(self.events, self.grid, None)
        return out if stream is None else out[self.event_offsets[int(stream)]:self.event_offsets[int(stream) + 1]]

    def doa_track(self, e):
        """the direction track of event ``e`` (in event order), a host array [T_e, 4] as ``DetectionResult.doa_track``: the times
        count from the start of the event's feed; an event the stream's history rule refused has no rows.  Only on what a
        stream with ``localize=sed.DOA(..., track=sed.DirectionTrack(...))`` returns."""
        return _doa_track(self, e)

    def event_audio(self, e):
        """the extracted audio of event ``e`` of this call (``DetectionResult.event_audio``): a float32 device slice of ``audio``
        at the detector's rate, empty where the event was not located.  Only on what a stream with ``emit_audio=True`` returns
        (DESIGN 5t); the host reads the event's two integers."""
        return _event_audio(self, e)

    @property
    def noise_frames(self):
        """int32 [E] on the device, as ``DetectionResult.noise_frames``: only on what a stream with
        ``emit_audio=True`` of a detector with ``extract=sed.MVDR(noise_blocks >= 1)`` returns, otherwise AttributeError"""
        return _noise_frames(self)


class StreamDetector:
    """``EventDetector`` for audio that is still arriving, S streams at once (module docstring).  The keyword arguments are
    ``EventDetector``'s, checked the same way; ``max_new_windows``: windows per stream and step (longer pushes are split).
    ``history_frames`` (a detector with ``localize=``): every lane also keeps its last samples in a ring, and an
    emitted event ``[a, b)`` whose frames ``[f0, f1)`` (``localize.event_frames``) satisfy ``b*tf + lat - f0 <= history_frames``
    (``localize.stream_locates``) comes with the ``lag``, ``strength`` and ``loc_frames`` of the offline call, bit for bit; the
    others with zeros.  ``"min"`` = ``max_frames + lat``, the least that is accepted: every event of at most ``max_frames``
    feature frames is located.  The ring costs ``4 * C * localize.stream_ring_samples(...)`` bytes per feed.
    ``emit_audio=True`` (a detector with ``extract=sed.DelaySum(...)`` or ``sed.MVDR(...)``, which does not stream without it;
    DESIGN 5t): a step that emits events also extracts their audio from the rings, ``events.event_beamform_ring`` or
    ``events.event_mvdr_ring`` — every located event's audio is the offline call's, bit for bit, in any chunking; an event the
    rule above refuses has ``dir = -1`` and length 0 (``StreamEvents.audio`` / ``event_audio``).  With
    ``extract=sed.MVDR(noise_blocks=Kn)``, ``Kn >= 1``, ``history_frames="min"`` is ``max_frames + lat + nf``,
    ``nf = localize.stream_noise_frames(...)`` feature frames more, and a located event whose weights come from the frames
    before its onset gets its audio iff ``b*tf + lat - f0 + nf <= history_frames`` (``localize.stream_extracts``): otherwise it
    keeps its ``dir`` and has length 0; the events also hold ``noise_frames``.  It costs one more blocking
    8-byte read and one device allocation per step that emits events; ``state_bytes`` does not change."""

    def __init__(self, model, n_streams, keep_probs=False, max_new_windows=4, _det=None, input_sr=None, input_channels=None,
                 history_frames=None, emit_audio=False, **kw):
        self.det = _det if _det is not None else EventDetector(model, **kw)
        det, m = self.det, self.det.model
        self.emit_audio = bool(emit_audio)
        if getattr(det.localize_settings, "contrast", None) is not None:
            raise NotImplementedError("sed.DOA(..., contrast=sed.Contrast(...)) is offline only so far; live feeds are a follow-up: the rule "
                                      "already reads only feature frames before the onset and only the event's own class, which is final "
                                      "when the event is emitted, but it needs search + guard more feature frames of ring and a per-feed "
                                      "activity ring (DESIGN 5z); make the stream from a detector without contrast=")
        if det.extract_settings is not None and not self.emit_audio:
            raise NotImplementedError("live feeds extract audio only when asked to: a detector with extract=sed.DelaySum(...) or "
                                      "sed.MVDR(...) streams with emit_audio=True (and history_frames=), which costs one more "
                                      "blocking read and one device allocation per step (DESIGN 5t); pass emit_audio=True, or make "
                                      "the stream from a detector without extract=")
        if self.emit_audio and getattr(det.extract_settings, "quiet", False):
            raise NotImplementedError("sed.MVDR(noise_select='quiet') is offline only so far; live feeds are a follow-up: with "
                                      "noise_exclude='same' every earlier event of the class is final when an event is emitted, so "
                                      "it needs only noise_search more blocks of ring; with 'any' it also needs the other classes' "
                                      "open events.  Stream with noise_select='fixed', or extract offline (DESIGN 5w)")
        if self.emit_audio and det.extract_settings is None:
            raise ValueError("emit_audio=True needs a detector that extracts audio: EventDetector(..., localize=sed.DOA(...), "
                             "extract=sed.DelaySum(...) or sed.MVDR(...))")
        if det.localize_settings is not None and history_frames is None:
            raise NotImplementedError("live feeds are not localised: when a stream's event becomes final the PCM of its frames is "
                                      "gone (DESIGN 5o); make the StreamDetector without localize=, or give it history_frames= "
                                      "(\"min\" or a number of feature frames) to keep the audio in a ring (DESIGN 5p)")
        if det.localize_settings is None and history_frames is not None:
            raise ValueError("history_frames is the audio a localising stream keeps: the detector has no localize=sed.TDOA(...)")
        S = int(n_streams)
        if not 1 <= S <= 65535 or not 1 <= int(max_new_windows) <= 1024:
            raise ValueError(f"need 1 <= n_streams <= 65535 and 1 <= max_new_windows <= 1024, got {n_streams}, {max_new_windows}")
        # planar lanes per feed: lane s*C + c; a spatial detector's net reads C + C(C-1)/2 images of C audio channels
        self.C = det.audio_channels
        input_channels = self.C if input_channels is None else int(input_channels)
        if self.C > 1 and input_channels != self.C:
            raise ValueError(f"a {self.C}-channel net takes [n, {self.C}] interleaved pieces: input_channels must be {self.C}, got "
                             f"{input_channels} (there is no mix-down to fewer channels and no duplication of a mono signal)")
        if S * self.C > 65535:
            raise ValueError(f"{S} feeds of {self.C} channels are {S * self.C} lanes: sed_stream_append takes at most 65535")
        self.S, self.keep_probs, self.max_new = S, bool(keep_probs), int(max_new_windows)
        self.K, self.CF = m.dense[-1], m.in_channels * m.n_mels
        self.PW = self.C * m.n_mels                                        # mel columns = PCEN chains per feed (with det.compress)
        tf = m.time_factor
        self.sched = StreamSchedules(tf, det.seq_len, det.hop, det.trim, det.median_max, S)     # class-wise: the widest median
        self.win_out, self.hop_out = self.sched.win_out, self.sched.hop_out
        self.step_frames = self.max_new * det.hop                          # feature frames per stream and step
        self.FC = det.seq_len + tf + self.step_frames                      # rows per half of a stream's feature region
        h = det.hop_length
        self.q = -(-(feature.NFFT // 2) // h)                              # frames whose left half reaches before their hop
        if self.q + 1 > self.step_frames:
            raise ValueError(f"hop_length={h} is too small: the {self.q + 1} frames of a flush exceed one step of {self.step_frames}")
        self.CC = (self.q + 1) * h + feature.NFFT // 2                     # samples per half of a stream's PCM carry (an upper bound)
        # the PCM ring of a localising stream: lat, the history and the samples per lane
        self.lat = self.history_frames = None
        self.noise_frames = 0
        self.cap, self._ring, self._rws_ring = 0, None, None
        self._ev_keys = _KEYS
        if history_frames is not None:
            from .localize import stream_latency_frames, stream_noise_frames, stream_ring_samples
            rows = det.class_settings()
            if any(r["low"] < r["threshold"] for r in rows):
                raise ValueError("a localising stream needs low == threshold in every class: below the threshold a run that began "
                                 "within min_gap of a pending event holds that event back for as long as the run lasts, longer than "
                                 "any ring keeps its audio (DESIGN 5p)")
            self.lat = stream_latency_frames(tf, det.seq_len, det.median_max, max(r["min_gap"] for r in rows))
            least = det.localize_settings.max_frames + self.lat
            # the frames before an event's first that its pre-onset noise covariance reads: "min" keeps them too
            mv = det.extract_settings if self.emit_audio else None
            self.noise_frames = stream_noise_frames(h, mv.noise_blocks, mv.noise_guard) if getattr(mv, "noise_blocks", 0) else 0
            if not (history_frames == "min" or (isinstance(history_frames, (int, np.integer)) and not isinstance(history_frames, bool))):
                raise ValueError(f"history_frames must be \"min\" or an integer number of feature frames, got {history_frames!r}")
            self.history_frames = least + self.noise_frames if isinstance(history_frames, str) else int(history_frames)
            if not least <= self.history_frames <= 0x7fffffff:
                raise ValueError(f"history_frames={self.history_frames} is less than the minimum max_frames + lat = "
                                 f"{det.localize_settings.max_frames} + {self.lat} = {least} feature frames (\"min\")")
            self.cap = stream_ring_samples(self.history_frames, self.step_frames, h, feature.NFFT)
            self._ev_keys = _KEYS + _TDOA_KEYS + (_DOA_KEYS if det.locates_directions else ()) + \
                            (_TRACK_KEYS if det._track_info() is not None else ()) + (_BEAM_KEYS if self.emit_audio else ()) + \
                            (_NOISE_KEYS if self.noise_frames else ())
        self._dims = (S, self.K, self.win_out, self.hop_out, det.median_max, self.max_new)
        self._core_bytes = lib().sed_stream_state_bytes(*self._dims)
        if self._core_bytes == 0:
            check(-1, "sed_stream_state_bytes")
        self._state = self._feat = self._pcm = None                        # allocated by the first call that runs
        self._aws = self._sws = self._lm = None
        self._pcen_state = self._pws = self._pc_scaler = None
        z = lambda: np.zeros(S, np.int64)                                   # noqa: E731
        self._n, self._fdone = z(), z()                                    # samples received, feature frames made from them
        self._cbase, self._clen, self._cpar = z(), z(), z()                # the PCM carry: first sample, length, which half
        self._fbase, self._frows, self._fpar = z(), z(), z()               # the feature rows held: first frame, count, which half
        self._ar = np.arange(S, dtype=np.int64)
        self._none = np.zeros(S, bool)
        self.marks = None                                                  # a list here receives (phase, start, end) hip events
        # the resampling stage in front of push: None when push receives mono float PCM at the detector's rate
        self.input_sr = det.sr if input_sr is None else int(input_sr)
        self.input_channels = int(input_channels)
        self._rs = None
        if self.input_sr != det.sr or self.input_channels != 1:
            from .resample import plan_for
            if not 1 <= self.input_channels <= 64:
                raise ValueError(f"input_channels must be 1..64, got {input_channels}")
            plan = plan_for(self.input_sr, det.sr)
            self._rs = plan
            self._rCR = 2 if plan.identity else plan.carry                 # carry samples per half (the copy filter has half = 1)
            self._rn, self._rm, self._rpar = z(), z(), z()                 # input samples received, outputs emitted, carry half
            self._rcarry = self._rws = None
        self.keep_pcm = False                                              # True: pcm_log[s] collects the resampled pieces of feed s
        self.pcm_log = [[] for _ in range(S)]

    # ── sizes ──
    @property
    def state_bytes(self):
        """device bytes held between calls: the step's rings and decoder states, the feature rows, per lane the PCM carry
        and the resampler's carry, with ``compress`` the PCEN smoother's two floats per feed and mel column and, with
        ``history_frames``, the PCM ring of every lane"""
        pcen = 8 * self.S * self.PW if self.det.compress is not None else 0                 # (C_k, loc) per chain
        return self._core_bytes + pcen + 4 * self.S * self.C * self.cap + 4 * self.S * 2 * (self.FC * self.CF + self.C * (self.CC + (self._rCR if self._rs is not None else 0)))

    @property
    def frame_seconds(self):
        return self.det.frame_seconds

    def _reset_host(self, which):
        self.sched.reset(which)
        for x in (self._n, self._fdone, self._cbase, self._clen, self._cpar, self._fbase, self._frows, self._fpar):
            x[which] = 0

    def _ready(self):
        """before any launch: the model's checks, then the device buffers (once)"""
        self.det._check_model()
        if self._state is None:
            dev = self.det.model.flat_parameters().device
            S = self.S
            self._state = torch.empty(self._core_bytes, dtype=torch.uint8, device=dev)
            self._feat = torch.empty(S * 2 * self.FC, self.CF, device=dev)
            self._pcm = torch.empty(S * self.C * 2 * self.CC, device=dev)
            self._aws = torch.empty(lib().sed_stream_append_workspace_bytes(S * self.C), dtype=torch.uint8, device=dev)
            if self.det.compress is not None:
                self._pcen_state = torch.zeros(S, self.PW, 2, device=dev)
            if self.cap:                                                   # (read only where the feed's counter says it was written)
                self._ring = torch.empty(S * self.C * self.cap, device=dev)
            check(lib().sed_stream_init(ptr(self._state), self._state.numel(), *self._dims, stream_ptr()), "sed_stream_init")
        return self._state.device

    # ── log-mel of a round: carry + new samples as one clip per stream ──
    def _logmel_round(self, fresh, takes, end):
        """``fresh``: the round's new samples packed (device, or None; lane by lane: feed s, channel c at lane s*C + c),
        ``takes`` [S] how many belong to each lane of a stream; the streams in the mask ``end`` also get their right-padded
        frames.  -> (features [rows, C*n_mels] or None, first row [S], rows [S])"""
        det, h, S, CC, NC = self.det, self.det.hop_length, self.S, self.CC, self.C
        dev = self._state.device
        takes, half = np.asarray(takes, np.int64), feature.NFFT // 2
        keep, done = self._clen, self._fdone
        n = self._n + takes
        # frames that need no right padding: f*h + n_fft/2 <= n; a stream that ends gets all 1 + n // h of them
        upto = np.where(end, np.where(n > 0, 1 + n // h, 0), np.where(n >= half, (n - half) // h + 1, 0))
        act = (takes > 0) | (upto != done)
        # the carry [cbase, n_prev) and the new samples are one clip; the next carry starts q frames before frame `upto`
        a_new = np.where(end, n, np.maximum(0, upto - self.q) * h)
        total = np.where(act, keep + takes, 0)
        # per lane: the C lanes of a feed move the same counts, each in its own region of the carry and of `work`
        lane = (lambda a: a) if NC == 1 else (lambda a: np.repeat(a, NC))
        total_l, takes_l, cpar_l = lane(total), lane(takes), lane(self._cpar)
        work_at = _excl((total_l + 3) & ~3)                                 # clips start 16-byte aligned (the fast load path)
        base = np.arange(S * NC, dtype=np.int64) * (2 * CC)
        table = np.stack([base + cpar_l * CC, lane(keep), _excl(takes_l), takes_l, work_at, base + (1 - cpar_l) * CC, lane(n - a_new)], 1)
        table[~lane(act)] = 0                                               # sed_stream_append: zeros = nothing moves
        clip = act & (upto > done)
        clip_rows = np.where(clip, 1 + total // h, 0)
        row0 = np.where(clip, _excl(clip_rows) + done - self._cbase // h, 0)
        rows = np.where(clip, upto - done, 0)
        n_rows, n_work = int(clip_rows.sum()), int(((total_l + 3) & ~3).sum())
        if self._ring is not None and takes.any():                         # the new samples also go to the rings, from sample _n on
            self._rws_ring = ring_write(self._ring, self.cap, fresh, np.stack([_excl(takes_l), takes_l, lane(self._n)], 1),
                                                self._rws_ring)
        self._n, self._fdone = n, upto
        self._cbase, self._clen = np.where(act, a_new, self._cbase), np.where(act, n - a_new, self._clen)
        self._cpar = np.where(act, 1 - self._cpar, self._cpar)
        work = torch.empty(max(n_work, 1), device=dev) if n_rows else None
        if act.any():
            table = np.ascontiguousarray(table)
            check(lib().sed_stream_append(ptr(self._pcm), self._pcm.numel(), 2 * CC, ptr(fresh), int(takes_l.sum()), ptr(work),
                                          work.numel() if work is not None else 0, C.c_void_p(table.ctypes.data), S * NC, ptr(self._aws),
                                          self._aws.numel(), stream_ptr()), "sed_stream_append")
        if not n_rows:
            return None, row0, rows
        if self._lm is None:
            m = det.model
            tables = feature._tables(dev.index or 0, det.sr, feature.NFFT, m.n_mels)
            mean, inv = feature._scaler(det.mean, det.std, dev)
            if det.compress is not None:                                    # the mel columns leave the front end unscaled
                (mean, inv), self._pc_scaler = (feature._mel_identity(mean, inv, self.PW) if det.spatial
                                                else ((None, None), (mean, inv)))
            need = (lib().sed_logmel_batch_workspace_bytes(S) if NC == 1 else lib().sed_logmel_gcc_workspace_bytes(S, NC) if det.spatial
                    else lib().sed_logmel_multi_workspace_bytes(S, NC))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._lm = (tables, mean, inv, ws)
        tables, mean, inv, ws = self._lm
        ct = np.ascontiguousarray(np.stack([work_at[lane(clip)], total_l[lane(clip)]], 1))
        out = torch.empty(n_rows, self.CF, device=dev)
        if det.spatial:                                                     # the C lanes of a feed -> C mel blocks and one GCC-PHAT block per
            _timed(self.marks, "logmel", lambda: check(lib().sed_logmel_gcc(   # pair: a frame's GCC needs that frame's samples only
                ptr(work), work.numel(), C.c_void_p(ct.ctypes.data), ct.shape[0] // NC, NC, ptr(tables), tables.numel() * 4, ptr(mean),
                ptr(inv), ptr(out), n_rows, feature.NFFT, h, det.model.n_mels, det.model.n_mels, 0, ptr(ws), ws.numel(), stream_ptr()),
                "sed_logmel_gcc"))
            return self._pcen_round(out, row0, rows, done), row0, rows
        if NC > 1:                                                          # the C lanes of a feed -> its rows' C column blocks
            _timed(self.marks, "logmel", lambda: check(lib().sed_logmel_multi(
                ptr(work), work.numel(), C.c_void_p(ct.ctypes.data), ct.shape[0] // NC, NC, ptr(tables), tables.numel() * 4, ptr(mean),
                ptr(inv), ptr(out), n_rows, feature.NFFT, h, det.model.n_mels, 0, ptr(ws), ws.numel(), stream_ptr()), "sed_logmel_multi"))
            return self._pcen_round(out, row0, rows, done), row0, rows
        _timed(self.marks, "logmel", lambda: check(lib().sed_logmel_batch(
            ptr(work), work.numel(), C.c_void_p(ct.ctypes.data), ct.shape[0], ptr(tables), tables.numel() * 4, ptr(mean), ptr(inv),
            ptr(out), n_rows, feature.NFFT, h, det.model.n_mels, 0, ptr(ws), ws.numel(), stream_ptr()), "sed_logmel_batch"))
        return self._pcen_round(out, row0, rows, done), row0, rows

    def _pcen_round(self, out, row0, rows, done):
        """with ``compress``: PCEN, in place, of the mel columns of the round's NEW rows — feed s owns ``rows[s]`` rows from
        ``row0[s]``, the first of them its feature frame ``done[s]`` — in one ``sed_pcen`` call over all feeds.  The smoother's
        state (S x C*n_mels chains) stays on the device; a feed whose counter is back at 0 starts afresh without a reset."""
        det = self.det
        if det.compress is None:
            return out
        recs = np.stack([row0, rows, np.where(rows > 0, done, 0)], 1)
        def run():
            self._pws = feature._pcen_launch(out, det.compress, det.compress.smoothing(det.sr, det.hop_length), recs, 0, self.PW,
                                             *self._pc_scaler, self._pcen_state, self._pws)
        _timed(self.marks, "logmel", run)
        return out

    # ── one step: new feature rows in, events out ──
    def _step(self, fresh, row0, rows, end):
        """``fresh`` [*, CF] device rows, stream s takes ``rows[s]`` of them from ``row0[s]`` (at most step_frames); the streams
        in the mask ``end`` end after them.  -> (events dict, event offsets [S+1], probs or None, prob counts [S], final [S], the
        events' packed audio or None)"""
        det, S, K, CF, FC, sc = self.det, self.S, self.K, self.CF, self.FC, self.sched
        dev = self._state.device
        tf, L, ar = det.model.time_factor, det.seq_len, self._ar
        rows, row0 = np.asarray(rows, np.int64), np.asarray(row0, np.int64)
        # 1. the feature rows: keep what a later window can need, append the new rows (into the stream's other half)
        act = rows > 0
        if act.any():
            k0 = sc.keep_from()
            keep = self._fbase + self._frows - k0
            base = ar * (2 * FC * CF)
            at = np.stack([base + (self._fpar * FC + (k0 - self._fbase)) * CF, keep * CF, row0 * CF, rows * CF, np.zeros(S, np.int64),
                           base + (1 - self._fpar) * FC * CF, (keep + rows) * CF], 1)
            at[~act] = 0
            at = np.ascontiguousarray(at)
            self._fbase, self._frows = np.where(act, k0, self._fbase), np.where(act, keep + rows, self._frows)
            self._fpar = np.where(act, 1 - self._fpar, self._fpar)
            check(lib().sed_stream_append(ptr(self._feat), self._feat.numel(), 2 * FC * CF, ptr(fresh), fresh.numel(), None, 0,
                                          C.c_void_p(at.ctypes.data), S, ptr(self._aws), self._aws.numel(), stream_ptr()),
                  "sed_stream_append")
        # 2. the windows that are due, and the step's table
        prev_out, prev_F, prev_G = sc.n_out, sc.final_frames, sc.decided
        w0, n_reg, extra, win_len = sc.advance(rows, end)
        now_out = sc.n_out
        now_F, now_G = np.where(end, now_out, sc.final_frames), np.where(end, now_out, sc.decided)
        row_base = ar * (2 * FC) + self._fpar * FC - self._fbase           # + a frame of the stream = its row in the feature state
        short = win_len != L                                                # streams that end below seq_len: one window each
        cf = n_reg + ((extra >= 0) & ~short)                                # windows of seq_len frames per stream
        first = _excl(cf)
        n_full = int(cf.sum())
        idx = np.repeat(ar, cf)
        within = np.arange(n_full, dtype=np.int64) - np.repeat(first, cf)
        full = row_base[idx] + np.where(within < n_reg[idx], (w0[idx] + within) * sc.hop, extra[idx])
        logit_off = first * (self.win_out * K)
        n_logits, groups = n_full * self.win_out * K, []
        for Lw in np.unique(win_len[short]).tolist():                       # grouped by length, like the offline batch
            ss = np.nonzero(short & (win_len == Lw))[0]
            logit_off[ss] = n_logits + np.arange(len(ss)) * ((Lw // tf) * K)
            groups.append((Lw, row_base[ss]))
            n_logits += len(ss) * (Lw // tf) * K
        prob_n, dg = now_F - prev_F, now_G - prev_G
        dg_max, cap, n_probs = int(dg.max()), int((K * (dg // 2 + 2)).sum()), int(prob_n.sum())
        table = np.ascontiguousarray(np.stack([cf + short, logit_off, w0, prev_out, now_out, end.astype(np.int64), win_len // tf,
                                               _excl(prob_n)], 1))
        # 3. gather + forward, chunked exactly like the offline detector
        logits = torch.empty(max(n_logits, 1), device=dev)
        jobs = _window_jobs(logits, [(L, full)] + groups, tf, K)
        if jobs:
            with torch.no_grad():
                det._forward_windows(self._feat, jobs, self.marks)
        # 4. the step
        need = lib().sed_stream_step_workspace_bytes(S, K, dg_max)
        if self._sws is None or self._sws.numel() < need:
            self._sws = torch.empty(need, dtype=torch.uint8, device=dev)
        ev = _event_tensors(_KEYS, max(cap, 1), dev)
        ev_off = torch.empty(S + 1, dtype=torch.int32, device=dev)
        probs = torch.empty(n_probs, K, device=dev) if self.keep_probs else None
        give = probs is not None and n_probs > 0
        rest = (ptr(logits) if n_logits else None, n_logits, C.c_void_p(table.ctypes.data), dg_max, ptr(probs) if give else None,
                n_probs if give else 0, cap, *(ptr(ev[k]) for k in _KEYS), ptr(ev_off), ptr(self._sws), self._sws.numel(), stream_ptr())
        if det.classwise:
            _timed(self.marks, "step", lambda: check(lib().sed_stream_step_classwise(
                ptr(self._state), self._state.numel(), *self._dims, det._combine_id, det.trim, det._class_table(K), *rest),
                "sed_stream_step_classwise"))
        else:
            _timed(self.marks, "step", lambda: check(lib().sed_stream_step(
                ptr(self._state), self._state.numel(), *self._dims, det._combine_id, det.trim, det.lo, det.hi,
                det.min_gap, det.min_len, *rest), "sed_stream_step"))
        offs = ev_off.cpu().tolist()                                        # the one blocking read of a step
        if offs[-1] > cap:
            raise SedHipError(f"sed_stream_step emitted {offs[-1]} events, more than the bound {cap}")
        events = {k: v[:offs[-1]] for k, v in ev.items()}
        audio = None
        if self._ring is not None:
            events.update(self._locate(events, end))
            if self.emit_audio:
                audio = self._extract(events, offs[-1])
        if end.any():
            self._reset_host(end)
        return events, offs, probs, prob_n, now_F, audio

    def _locate(self, events, end):
        """the step's events on the rings, with the samples received so far (before a feed that ends is reset): one
        ``event_tdoa_ring`` call"""
        det, t, h = self.det, self.det.localize_tdoa, self.det.hop_length
        # every frame of an emitted event is final: its samples were received, so nothing is read beyond them — except in a feed
        # that ends, whose count is final and whose last frames are right-padded with zeros as offline
        live = ~end & (self._fdone > 0)
        if (live & ((self._fdone - 1) * h + feature.NFFT // 2 > self._n)).any() or (self.sched.N > self._fdone).any():
            raise SedHipError("a stream holds final feature frames whose samples it has not received")
        if det.locates_directions:                                          # the same call with the steering launch
            return _timed(self.marks, "locate", lambda: event_doa_ring(
                self._ring, self.cap, self._n, self.C, events, det.model.time_factor, det.localize_settings, sr=det.sr, hop=h,
                lat_frames=self.lat, history_frames=self.history_frames))
        return _timed(self.marks, "locate", lambda: event_tdoa_ring(
            self._ring, self.cap, self._n, self.C, events, det.model.time_factor, max_lag=t.max_lag, max_frames=t.max_frames, hop=h,
            lat_frames=self.lat, history_frames=self.history_frames))

    def _extract(self, events, E):
        """the audio of the step's located events from the rings, with the samples received so far, through the detector's
        beam: one ``event_beamform_ring`` / ``event_mvdr_ring`` call when the step emitted events.  ``events`` gains
        ``audio_start`` and ``audio_len``; -> the packed buffer"""
        from .localize import MVDR
        det, dev = self.det, self._state.device
        if E == 0:                                                          # no launch, no read
            events.update({k: v for k, v in self._no_audio(dev).items() if k != "audio"})
            return torch.empty(0, device=dev)
        entry = event_mvdr_ring if isinstance(det.extract_settings, MVDR) else event_beamform_ring
        given = events
        if self.noise_frames:
            given = {**events, "dir": self._dir_with_noise_history(events)}
        beam = _timed(self.marks, "extract", lambda: entry(self._ring, self.cap, self._n, self.C, given, det.model.time_factor,
                                                           det.localize_settings, det.extract_settings, sr=det.sr, hop=det.hop_length))
        audio = beam.pop("audio")
        events.update(beam)
        return audio

    def _no_audio(self, dev):
        """the extraction columns of an empty event table"""
        if self.noise_frames:
            return _mvdr_empty(dev, self.det.extract_settings)
        return _beam_empty(dev)

    def _dir_with_noise_history(self, events):
        """``dir`` for the extraction alone, by device tensor ops (no host read): -1 where the event's weights come from the
        frames before its onset (``f0 * hop >= (G + Kn + 1) 1024``) and the ring need not hold them any more,
        ``offset*tf + lat - f0 + nf > history_frames`` (``localize.stream_extracts``).  ``f0`` is ``event_frames``'
        with the frames the feed has now — an emitted event's frames are final, so it is the offline call's."""
        det, dev = self.det, events["dir"].device
        tf, h, mf, mv = det.model.time_factor, det.hop_length, det.localize_settings.max_frames, det.extract_settings
        n_feat = torch.from_numpy(1 + self._n // h).to(dev)[events["stream"].long()]
        a, off = events["onset"].long() * tf, events["offset"].long() * tf
        b = torch.minimum(off, n_feat)
        c = events["peak_frame"].long() * tf + tf // 2 - mf // 2
        f0 = torch.where(b - a > mf, torch.minimum(torch.maximum(c, a), b - mf), a)
        uses = f0 * h >= (mv.noise_guard + mv.noise_blocks + 1) * 1024
        refused = uses & (off + self.lat - f0 + self.noise_frames > self.history_frames)
        return torch.where(refused, torch.full_like(events["dir"], -1), events["dir"])

    # ── rounds: a push of any size as steps of bounded size ──
    def _run(self, rounds):
        """``rounds``: an iterator of (fresh, row0, rows, end mask) steps -> one StreamEvents for all of them"""
        S, K = self.S, self.K
        dev = self._state.device
        parts = []
        final = self.sched.final_frames
        for fresh, row0, rows, end in rounds:
            if not rows.any() and not end.any():
                continue
            parts.append(self._step(fresh, row0, rows, end))
            final = parts[-1][4]
        final = final.tolist()
        if not parts:
            ev = self._no_events(dev)
            probs = torch.empty(0, K, device=dev) if self.keep_probs else None
            return self._events(ev, [0] * (S + 1), final, probs, [0] * (S + 1) if self.keep_probs else None,
                                torch.empty(0, device=dev) if self.emit_audio else None)
        if len(parts) == 1:
            ev, offs, probs, prob_n, _, audio = parts[0]
            poffs = np.concatenate([[0], np.cumsum(prob_n)]).tolist() if self.keep_probs else None
            return self._events(ev, offs, final, probs, poffs, audio)
        # several steps: a stream's events (and rows) of step 1, then of step 2, ...: one stable sort by (stream, class)
        ev = {k: torch.cat([p[0][k] for p in parts]) for k in self._ev_keys}
        audio = None
        if self.emit_audio:                                                 # the steps' buffers back to back, in step order
            audio, ev["audio_start"], ev["audio_len"] = merge_step_audio([(p[5], p[0]["audio_start"], p[0]["audio_len"]) for p in parts])
        order = torch.sort(ev["stream"].long() * K + ev["cls"].long(), stable=True).indices
        ev = {k: v[order] for k, v in ev.items()}
        counts = np.sum([np.diff(p[1]) for p in parts], axis=0)
        offs = np.concatenate([[0], np.cumsum(counts)]).tolist()
        probs = poffs = None
        if self.keep_probs:
            owner = np.concatenate([np.repeat(self._ar, p[3]) for p in parts])     # the stream of every row, steps in order
            idx = np.argsort(owner, kind="stable")                          # by stream, steps in order within a stream
            allp = torch.cat([p[2] for p in parts])
            probs = allp[torch.from_numpy(idx).to(dev)]
            poffs = np.concatenate([[0], np.cumsum(np.sum([p[3] for p in parts], axis=0))]).tolist()
        return self._events(ev, offs, final, probs, poffs, audio)

    def _no_events(self, dev):
        ev = _event_tensors(_KEYS, 0, dev)
        if self._ring is not None:
            P = self.C * (self.C - 1) // 2
            ev.update(lag=torch.empty(0, P, device=dev), strength=torch.empty(0, P, device=dev),
                      loc_frames=torch.empty(0, dtype=torch.int32, device=dev))
            if self.det.locates_directions:
                ev.update(dir=torch.empty(0, dtype=torch.int32, device=dev), doa_power=torch.empty(0, device=dev))
                ev.update({k: v for k, v in self.det._no_lags().items() if k in _TRACK_KEYS})
            if self.emit_audio:
                ev.update({k: v for k, v in self._no_audio(dev).items() if k != "audio"})
        return ev

    def _events(self, ev, offs, final, probs, poffs, audio=None):
        return StreamEvents(ev, offs, final, self.frame_seconds, probs, poffs, self.det.sr if self.cap else None,
                            self.det.localize_settings.grid if self.cap and self.det.locates_directions else None, audio,
                            self.det._track_info() if self.cap else None)

    def _pieces(self, xs, what, check_one, axis=0):
        xs = list(xs)
        if len(xs) != self.S:
            raise ValueError(f"expected {self.S} {what} (one per stream, None = nothing new), got {len(xs)}")
        pieces, lens = [], np.zeros(self.S, np.int64)
        for s, x in enumerate(xs):
            if x is not None:
                x = check_one(s, x)
                lens[s] = x.shape[axis]
            pieces.append(x)
        return pieces, lens

    def _pack(self, pieces, lens, done, takes, dev, planar=False):
        """the round's share of every piece, back to back on the device (``feature.cat_to_device``); planar [C, n] pieces go
        lane by lane (channel 0's share, then channel 1's, ...)"""
        if planar:
            return feature.cat_to_device([pieces[s][:, done[s]:done[s] + takes[s]].reshape(-1) for s in np.nonzero(takes)[0]], dev)
        return feature.cat_to_device([pieces[s] if takes[s] == lens[s] else pieces[s][done[s]:done[s] + takes[s]]
                                      for s in np.nonzero(takes)[0]], dev)

    # ── the resampling stage: pieces at the input rate -> mono float32 pieces at the detector's rate ──
    def _resample_round(self, pieces, lens, end):
        """``pieces``: per feed a tensor of ``lens[s]`` sample frames (int16 or float32, all one dtype) or None; the feeds in
        the mask ``end`` end: everything up to ceil(n L / M) comes out, zeros to their right.  One launch: the outputs that
        became final, per feed as a view of one packed device buffer (None = none), and the feeds' next carry.  The host
        keeps the int64 counters and reads nothing back.  A multichannel net: one row per lane (feed, channel), each keeping
        its channel of the feed's frames and its own carry; a feed's outputs are then a planar [C, n] view."""
        from .resample import _device_taps, build_rows, launch, pack_pcm, with_channels
        plan, S, CR, NC = self._rs, self.S, self._rCR, self.C
        dev = self._state.device
        if self._rcarry is None:
            self._rcarry = torch.zeros(S * NC * 2 * CR, device=dev)
        taps, L, M, half = _device_taps(plan.sr_in, plan.sr_out, dev.index or 0)
        n_new = self._rn + lens
        if plan.identity:
            done = np.where(end, n_new, np.maximum(0, n_new - 1))          # the copy filter reads x[m + 1] (times zero)
        else:
            done = np.where(end, plan.n_out_array(n_new), plan.n_final_array(n_new))
        act = (lens > 0) | (done > self._rm)
        idx = np.nonzero(act)[0]
        if idx.size == 0:
            return [None] * S
        n_hist = np.minimum(CR, self._rn)
        live = [pieces[s] for s in idx if lens[s] > 0]
        x = pack_pcm(live, dev) if live else None
        is16 = bool(live) and live[0].dtype == torch.int16
        lane = (lambda a: a) if NC == 1 else (lambda a: np.repeat(a, NC))   # the C lanes of a feed share its counters
        base = (lane(idx) * NC + np.tile(np.arange(NC), idx.size)) * (2 * CR)
        rows, _, n_outbuf = build_rows(lane(lens[idx]), lane(self._rn[idx]), lane(self._rm[idx]), lane((done - self._rm)[idx]),
                                       lane(n_hist[idx]), base + lane((self._rpar * CR + CR - n_hist)[idx]),
                                       np.where(lane(end[idx]), -1, base + lane(((1 - self._rpar) * CR)[idx])))
        if NC > 1:                                                          # ... and read the same frames, each its own channel
            rows[:, 0] = lane(_excl(lens[idx]))
            rows = with_channels(rows, np.tile(np.arange(NC), idx.size))
        out = torch.empty(max(n_outbuf, 1), device=dev)
        self._rws = _timed(self.marks, "resample", lambda: launch(x, int(is16), self.input_channels, self._rcarry, taps, L, M, half,
                                                                  rows, out, self._rws))
        res = [None] * S
        for r, s in enumerate(idx.tolist()):
            n_r, at = int(rows[r * NC, 4]), int(rows[r * NC, 5])
            if n_r:
                res[s] = out[at:at + n_r] if NC == 1 else out.as_strided((NC, n_r), ((n_r + 3) & ~3, 1), at)
                if self.keep_pcm:
                    self.pcm_log[s].append(res[s])
        moved = act & ~end
        self._rpar = np.where(moved, 1 - self._rpar, self._rpar)
        self._rn, self._rm = np.where(act, n_new, self._rn), np.where(act, done, self._rm)
        self._rn[end], self._rm[end], self._rpar[end] = 0, 0, 0
        return res

    def push(self, chunks):
        """a list of S mono PCM pieces (1-D, host or device, any length >= 0; None = nothing new) -> StreamEvents.  With
        ``input_sr`` / ``input_channels`` the pieces are at that rate, int16 or float (one dtype per push), ``[n, channels]``
        interleaved, and pass through the resampling stage first.  A net with C > 1 input channels takes ``[n, C]`` pieces and
        keeps the channels (module docstring)."""
        if self._rs is not None:
            from .resample import as_pcm

            def one(s, c):
                try:
                    return as_pcm(c, self.input_channels, f"stream {s}")
                except ValueError as e:
                    if self.C == 1:
                        raise
                    raise ValueError(f"{e}: a {self.C}-channel net takes [n, {self.C}] interleaved PCM pieces (for scaled "
                                     f"features use push_features)") from None
            pieces, lens = self._pieces(chunks, "waveform pieces", one)
            if len({p.dtype for p in pieces if p is not None}) > 1:
                raise ValueError("the pieces of one push must share a sample format (all int16 or all floating point)")
            self._ready()
            chunks = self._resample_round(pieces, lens, self._none)
        return self._push_mono(chunks)

    def _push_mono(self, chunks):
        """``push`` at the detector's own rate: mono pieces, or (a multichannel net) the resampling stage's planar [C, n] pieces"""
        planar = self.C > 1

        def one(s, c):
            c = c if isinstance(c, torch.Tensor) else torch.as_tensor(np.asarray(c))
            if planar:
                if c.dim() != 2 or c.shape[0] != self.C:
                    raise ValueError(f"stream {s}: expected planar PCM [{self.C}, n], got shape {tuple(c.shape)}")
            elif c.dim() != 1:
                raise ValueError(f"stream {s}: expected a mono 1-D waveform, got shape {tuple(c.shape)}")
            return c
        pieces, lens = self._pieces(chunks, "waveform pieces", one, axis=1 if planar else 0)
        dev = self._ready()
        per_round = (self.step_frames - 1) * self.det.hop_length

        def rounds():
            done = np.zeros(self.S, np.int64)
            while True:
                takes = np.minimum(per_round, lens - done)
                if not takes.any():
                    return
                fresh = self._pack(pieces, lens, done, takes, dev, planar)
                done = done + takes
                mel, row0, rows = self._logmel_round(fresh, takes, self._none)
                yield mel, row0, rows, self._none
        return self._run(rounds())

    def push_features(self, mels):
        """a list of S scaled feature pieces [n_s, C*F] (any channel count, host or device; None = nothing new) -> StreamEvents"""
        if self.cap:
            raise ValueError("a localising stream (history_frames=) takes audio: features carry no samples to locate an event on; "
                             "use push, or a stream without history_frames")
        def one(s, x):
            x = torch.as_tensor(x)
            if x.dim() != 2 or x.shape[1] != self.CF:
                m = self.det.model
                raise ValueError(f"stream {s}: expected features [N, {self.CF}] (in_channels*n_mels = {m.in_channels}*{m.n_mels}), got {tuple(x.shape)}")
            return x
        pieces, lens = self._pieces(mels, "feature pieces", one)
        dev = self._ready()

        def rounds():
            done = np.zeros(self.S, np.int64)
            while True:
                rows = np.minimum(self.step_frames, lens - done)
                if not rows.any():
                    return
                fresh = self._pack(pieces, lens, done, rows, dev).contiguous()
                done = done + rows
                yield fresh, _excl(rows), rows, self._none
        return self._run(rounds())

    def flush(self, streams=None):
        """end these streams (default: all): their right-padded log-mel frames and the offline grid's last window run, what
        is left is emitted, and they restart at frame 0.  A stream that received nothing is left alone; one shorter than one
        output frame raises ValueError (``plan_windows``' message) before anything runs."""
        which = range(self.S) if streams is None else [int(s) for s in streams]
        for s in which:
            if not 0 <= s < self.S:
                raise ValueError(f"stream {s} of {self.S}")
        h, sc = self.det.hop_length, self.sched
        held = np.zeros(self.S, np.int64)                                   # samples the resampling stage still owes
        if self._rs is not None:
            held = (self._rn if self._rs.identity else self._rs.n_out_array(self._rn)) - self._rm
        end = np.zeros(self.S, bool)
        for s in sorted(set(which)):
            n = int(self._n[s] + held[s])
            N = int(sc.N[s]) + (int(1 + n // h - self._fdone[s]) if n else 0)
            if N == 0:
                continue
            try:
                plan_windows(N, sc.tf, sc.L, sc.hop, sc.trim)
            except ValueError as e:
                raise ValueError(f"stream {s}: {e}") from None
            end[s] = True
        self._ready()
        first = None
        if (held[end] > 0).any():                                           # what the resampler holds comes out first (zeros to its right)
            first = self._push_mono(self._resample_round([None] * self.S, np.zeros(self.S, np.int64), end & (held > 0)))

        def rounds():
            if not end.any():
                return
            zero = np.zeros(self.S, np.int64)
            if (self._n[end] > 0).any():
                mel, row0, rows = self._logmel_round(None, zero, end)
            else:
                mel, row0, rows = None, zero, zero
            yield mel, row0, rows, end
        last = self._run(rounds())
        return last if first is None else self._joined(first, last)

    def _joined(self, a, b):
        """two StreamEvents of one call as one: per stream a's events (and rows), then b's"""
        K, dev = self.K, self._state.device
        ev = {k: torch.cat([a.events[k], b.events[k]]) for k in self._ev_keys}
        audio = None
        if self.emit_audio:
            audio, ev["audio_start"], ev["audio_len"] = merge_step_audio([(x.audio, x.events["audio_start"], x.events["audio_len"])
                                                                          for x in (a, b)])
        order = torch.sort(ev["stream"].long() * K + ev["cls"].long(), stable=True).indices
        ev = {k: v[order] for k, v in ev.items()}
        offs = (np.asarray(a.event_offsets) + np.asarray(b.event_offsets)).tolist()
        probs = poffs = None
        if self.keep_probs:
            na, nb = np.diff(a.prob_offsets), np.diff(b.prob_offsets)
            owner = np.concatenate([np.repeat(self._ar, na), np.repeat(self._ar, nb)])
            idx = np.argsort(owner, kind="stable")
            probs = torch.cat([a.probs, b.probs])[torch.from_numpy(idx).to(dev)]
            poffs = np.concatenate([[0], np.cumsum(na + nb)]).tolist()
        return self._events(ev, offs, b.final_frames, probs, poffs, audio)

    def reset(self, streams=None):
        """drop these streams (default: all) where they stand: nothing is emitted, they restart at frame 0"""
        which = np.arange(self.S) if streams is None else np.asarray([int(s) for s in streams], np.int64).reshape(-1)
        if which.size and not ((which >= 0) & (which < self.S)).all():
            raise ValueError(f"streams {which.tolist()} of {self.S}")
        self._ready()
        if which.size:
            ids = (C.c_int * which.size)(*which.tolist())
            check(lib().sed_stream_reset(ptr(self._state), self._state.numel(), *self._dims, ids, which.size, stream_ptr()),
                  "sed_stream_reset")
            self._reset_host(which)
            if self._rs is not None:
                self._rn[which], self._rm[which], self._rpar[which] = 0, 0, 0

    def active(self):
        """[(stream, cls, onset), ...] of the events that are open right now: a run that is known to be kept and has not closed
        (with the onset of the pending event it will merge with, if there is one)"""
        self._ready()
        n = self.S * self.K
        d = self._state[self._core_bytes - 64 * n:].view(torch.int32).view(n, 16).cpu().numpy()
        out = []
        gaps = [r["min_gap"] for r in self.det.class_settings()]          # class k merges across its own min_gap
        for i in np.nonzero((d[:, 0] != 0) & (d[:, 2] != 0))[0]:
            merge = d[i, 5] != 0 and d[i, 1] - d[i, 7] <= gaps[int(i) % self.K]
            out.append((int(i) // self.K, int(i) % self.K, int(d[i, 6] if merge else d[i, 1])))
        return out
