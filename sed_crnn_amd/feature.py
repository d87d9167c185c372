"""Log-mel front end on the GPU: ``_mbe`` of reference feature.py:55-59 as one HIP kernel.

``mbe(y)`` = log(mel_basis @ |STFT(y, n_fft=2048, hop=1024)|^2).T with librosa's defaults (periodic Hann,
center=True, Slaney mel scale and area normalisation, fmin 0, fmax sr/2).  librosa changed its STFT
edge padding from 'reflect' to 'constant' in 0.10, so ``pad_mode`` is explicit.  The constant tables
(window, FFT twiddles, mel basis) are computed once on the host in float64 and cached per device.
feature.py:127-129's StandardScaler can be fused in through ``mean``/``std``.
"""
import dataclasses
import functools

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr

SR, NFFT, HOP, NB_MEL = 44_100, 2048, 1024, 40        # reference feature.py:29-32
_LM_OFF_ENT = 8 + 2048 + 2048 + 1028                  # logmel.hip: header, window, inter-pass twiddles, pairing twiddles


def slaney_mel_basis(sr=SR, n_fft=NFFT, n_mels=NB_MEL):
    """librosa.filters.mel(sr, n_fft, n_mels) with its defaults (htk=False, norm='slaney')."""
    f_sp, brk = 200.0 / 3.0, 1000.0
    brk_mel, step = brk / f_sp, np.log(6.4) / 27.0

    def to_mel(f):
        return np.where(f >= brk, brk_mel + np.log(np.maximum(f, brk) / brk) / step, f / f_sp)

    def to_hz(m):
        return np.where(m >= brk_mel, brk * np.exp(step * (m - brk_mel)), f_sp * m)
    edges = to_hz(np.linspace(to_mel(np.float64(0.0)), to_mel(np.float64(sr / 2.0)), n_mels + 2))
    bins = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sr / n_fft)
    lo, ce, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    tri = np.minimum((bins[None, :] - lo) / (ce - lo), (hi - bins[None, :]) / (hi - ce))
    tri = np.maximum(tri, 0.0) * (2.0 / (hi - lo))
    return tri.astype(np.float32)


def hann_periodic(n_fft=NFFT):
    """scipy.signal.get_window('hann', n_fft, fftbins=True) = librosa's default STFT window, float32"""
    n = np.arange(n_fft, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)).astype(np.float32)


def build_tables(window, melfb, device):
    """the kernel's constant blob (window, FFT twiddles, sparse mel plan) for an arbitrary window [n_fft] and filterbank
    [n_mels, n_fft//2+1] (host arrays): built on the host by the library, then copied to ``device``"""
    import ctypes as C
    window = np.ascontiguousarray(window, dtype=np.float32)
    fb = np.ascontiguousarray(melfb, dtype=np.float32)
    n_fft, n_mels = window.shape[0], fb.shape[0]
    if fb.shape != (n_mels, n_fft // 2 + 1):
        raise ValueError(f"filterbank must be [n_mels, {n_fft // 2 + 1}], got {fb.shape}")
    hp = lambda a: C.c_void_p(a.ctypes.data)                                   # noqa: E731  host pointers
    nbytes = lib().sed_logmel_tables_bytes(hp(fb), n_fft, n_mels)
    if nbytes == 0:
        raise ValueError(f"sed_logmel cannot plan this filterbank (n_fft must be {NFFT}, n_mels <= 128, and at most 8192 "
                         f"non-zero weights so that the plan fits LDS beside the FFT scratch; large plans run with fewer waves per CU); got n_fft={n_fft}, n_mels={n_mels}, "
                         f"{int(np.count_nonzero(fb))} non-zeros")
    blob = np.zeros(nbytes // 4, dtype=np.uint32)
    check(lib().sed_logmel_build_tables(hp(window), hp(fb), n_fft, n_mels, hp(blob), nbytes), "sed_logmel_build_tables")
    return torch.from_numpy(blob.view(np.int32)).to(device)


@functools.lru_cache(maxsize=8)
def _tables(device_index, sr, n_fft, n_mels):
    """librosa's defaults (periodic Hann, Slaney bank), cached per (device, configuration)"""
    return build_tables(hann_periodic(n_fft), slaney_mel_basis(sr, n_fft, n_mels), torch.device("cuda", device_index))


_VALIDATED = {}          # (data_ptr, numel, version counter) of a caller's table blob -> its mel count


def _validated_mels(tables):
    """The library cannot read device memory to validate a caller's blob, and the kernel trusts its header: check it here —
    ONCE per blob (keyed by address, size and torch's in-place version counter), not per clip: the check is a blocking
    device-to-host copy (round-3 advisor)."""
    key = (tables.data_ptr(), tables.numel(), tables._version)
    n = _VALIDATED.get(key)
    if n is None:
        hdr = [int(v) & 0xFFFFFFFF for v in tables[:8].cpu().tolist()] if tables.numel() >= 8 else []
        ok = (len(hdr) == 8 and hdr[0] == 0x4C4D3332 and hdr[4] == tables.numel() and 1 <= hdr[1] <= 128 and
              ((hdr[5] == 0 and _LM_OFF_ENT + hdr[2] * 64 + hdr[1] <= hdr[4]) or
               (hdr[5] == 1 and hdr[2] == 33 and _LM_OFF_ENT + 33 * 32 * 4 + hdr[1] * 4 <= hdr[4])))
        if not ok:
            raise ValueError("tables is not a blob written by feature.build_tables / sed_logmel_build_tables (bad header)")
        if len(_VALIDATED) >= 64:
            _VALIDATED.clear()
        n = _VALIDATED[key] = hdr[1]
    return n


def _scaler(mean, std, device):
    """the StandardScaler as the kernels take it: float32 (mean, 1/std), the reciprocal taken in float64; (None, None) without one"""
    if mean is None:
        return None, None
    return mean.to(device).float().contiguous(), (1.0 / std.to(device).double()).float().contiguous()


def cat_to_device(pieces, device):
    """float32 ``torch.cat`` of the pieces on ``device``: host pieces are joined on the host and travel in ONE copy; with a device
    piece among them, each is moved and they are joined on the device"""
    if all(not p.is_cuda for p in pieces):
        return torch.cat([p.to(torch.float32) for p in pieces]).to(device)
    return torch.cat([p.to(device, torch.float32) for p in pieces])


def _needs_front_end(w, input_sr, sr, channels):
    """does this input go through resample.py first: another rate, interleaved channels or int16 samples"""
    from .resample import is_plain
    return (input_sr is not None and int(input_sr) != int(sr)) or not is_plain(w, channels)


SPATIAL = ("gcc_phat",)
GCC_MAX_CHANNELS = 8      # gcc.hip: GC_MAX_CH


def spatial_channels(channels):
    """input channels of a net that reads the spatial features of ``channels`` audio channels: the C mel images and one
    GCC-PHAT image per microphone pair, C + C(C-1)/2 (2 -> 3, 3 -> 6, 4 -> 10)"""
    c = int(channels)
    return c + c * (c - 1) // 2


def audio_channels_of(in_channels):
    """the audio channel count C in 2..8 with ``spatial_channels(C) == in_channels``, or None"""
    return next((c for c in range(2, GCC_MAX_CHANNELS + 1) if spatial_channels(c) == int(in_channels)), None)


def _check_spatial(spatial, keep_channels, channels, n_mels=None):
    if spatial is None:
        return
    if spatial not in SPATIAL:
        raise ValueError(f"spatial must be None or 'gcc_phat', got {spatial!r}")
    if not keep_channels:
        raise ValueError("spatial='gcc_phat' needs keep_channels=True: the cross-correlations are taken between the channels "
                         "that a mix-down would remove")
    if not 2 <= int(channels) <= GCC_MAX_CHANNELS:
        raise ValueError(f"spatial='gcc_phat' needs 2 to {GCC_MAX_CHANNELS} audio channels (one image per microphone pair), got "
                         f"channels={int(channels)}")
    if n_mels is not None and n_mels % 2:
        raise ValueError(f"spatial='gcc_phat' writes n_lags = n_mels lags per pair and needs an even count, got n_mels={n_mels}")


PCEN_BLOCK = 64          # pcen.hip: PC_L, the frames per block of the smoother (aligned to the absolute frame index)


@dataclasses.dataclass(frozen=True)
class PCEN:
    """Per-channel energy normalisation (librosa.pcen's definition with max_size = 1) of the mel energies
    ``E = scale * exp(log-mel)``: ``M[t] = (1 - b) M[t-1] + b E[t]``, ``M[0] = E[0]``;
    ``pcen = (E (eps + M)^-gain + bias)^power - bias^power``.  ``time_constant`` in seconds sets b (``smoothing``).
    ``compress=PCEN(...)`` on ``feature.mbe*`` and on ``EventDetector`` replaces the log compression by it."""
    gain: float = 0.98
    bias: float = 2.0
    power: float = 0.5
    time_constant: float = 0.4
    eps: float = 1e-6
    scale: float = 1.0

    def __post_init__(self):
        for name in ("gain", "bias", "power", "time_constant", "eps", "scale"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"PCEN: {name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not self.gain > 0 or not self.power > 0 or not self.eps > 0 or not self.time_constant > 0 or not self.scale > 0:
            raise ValueError(f"PCEN needs gain > 0, power > 0, eps > 0, time_constant > 0 and scale > 0, got gain={self.gain}, "
                             f"power={self.power}, eps={self.eps}, time_constant={self.time_constant}, scale={self.scale}")
        if self.bias < 0:
            raise ValueError(f"PCEN needs bias >= 0, got {self.bias}")

    def smoothing(self, sr=SR, hop=HOP):
        """b of the smoother for frames ``hop`` samples apart at rate ``sr`` (librosa's: T = time_constant * sr / hop frames,
        b = (sqrt(1 + 4 T^2) - 1) / (2 T^2)); 0.056389 for the defaults"""
        if not sr > 0 or not hop > 0:
            raise ValueError(f"PCEN.smoothing needs sr > 0 and hop > 0, got {sr}, {hop}")
        t = self.time_constant * float(sr) / float(hop)
        return float((np.sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t))


def _check_compress(compress):
    if compress is not None and not isinstance(compress, PCEN):
        raise TypeError(f"compress must be None or a PCEN(...) settings object, got {type(compress).__name__}")


def _pcen_launch(x, settings, b, recs, col0, width, mean32, inv32, state, ws=None):
    """``sed_pcen`` in place on the columns [col0, col0 + width) of the device matrix ``x``; ``recs`` [R, 3] int64 host rows
    (first row, n rows, absolute index of the first frame); ``mean32`` / ``inv32``: ``_scaler``'s pair, ``width`` wide, or None"""
    import ctypes as C
    recs = np.ascontiguousarray(np.asarray(recs, dtype=np.int64).reshape(-1, 3))
    R = recs.shape[0]
    need = lib().sed_pcen_workspace_bytes(x.shape[0], R, width)
    if need == 0:
        raise ValueError(f"sed_pcen takes fewer than 2^31 rows, at most 2^24 recordings and 1..65536 columns, got {x.shape[0]} rows, "
                         f"{R} recordings, {width} columns")
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(lib().sed_pcen(ptr(x), x.shape[0], x.stride(0), col0, width, C.c_void_p(recs.ctypes.data), R, ptr(state), b,
                         settings.gain, settings.bias, settings.power, settings.eps, settings.scale, ptr(mean32), ptr(inv32),
                         ptr(ws), ws.numel(), stream_ptr()), "sed_pcen")
    return ws


def _rows_table(rows, n, start=None):
    """row offsets [R+1] (what ``mbe_many`` returns; None: one recording of all n rows) and absolute start indices -> recs [R, 3]"""
    off = np.asarray([0, n] if rows is None else rows, dtype=np.int64).reshape(-1)
    if off.size < 1 or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > n:
        raise ValueError(f"rows must be non-decreasing row offsets inside the {n} rows of the features, got {off.tolist()}")
    R = off.size - 1
    t0 = np.zeros(R, np.int64) if start is None else np.asarray(start, dtype=np.int64).reshape(-1)
    if t0.size != R or (t0 < 0).any():
        raise ValueError(f"start must hold one absolute frame index >= 0 per recording ({R}), got {t0.tolist()}")
    return np.stack([off[:-1], np.diff(off), t0], 1)


def pcen(logmel, settings=PCEN(), sr=SR, hop=HOP, rows=None, mean=None, std=None, columns=None, state=None, start=None):
    """PCEN of log-mel features that are already on the device (``mbe`` / ``mbe_many`` without a scaler, or stored features):
    ``logmel`` [N, width] float32 CUDA -> a new tensor of the same shape (``sed_pcen``).  ``rows``: the row offsets
    [R+1] that ``mbe_many`` returns — every recording starts its own smoother; default: one recording.  ``mean`` / ``std``:
    the StandardScaler (fitted on PCEN features) of the processed columns, fused in.  ``columns`` = (first, count): only those
    columns are processed (each its own chain), the others are copied — ``(0, C*n_mels)`` for spatial features, whose GCC
    columns stay as they are.  ``state`` / ``start``: for features that arrive in pieces — ``start`` holds the absolute frame
    index of every recording's first row and ``state`` a float32 CUDA tensor ``[R, count, 2]`` that is read where start > 0 and
    updated; pieces of any sizes give bit for bit the rows of one call."""
    _check_compress(settings)
    if settings is None:
        raise TypeError("pcen needs a PCEN(...) settings object")
    if not (isinstance(logmel, torch.Tensor) and logmel.is_cuda and logmel.dim() == 2):
        raise RuntimeError("sed_crnn_amd.feature.pcen needs a 2-D CUDA(HIP) tensor; there is no CPU fallback")
    if (mean is None) != (std is None):
        raise ValueError("give both mean and std or neither")
    n, width = logmel.shape
    col0, cnt = (0, width) if columns is None else (int(columns[0]), int(columns[1]))
    if col0 < 0 or cnt < 1 or col0 + cnt > width:
        raise ValueError(f"columns = (first, count) must lie inside the {width} feature columns, got {(col0, cnt)}")
    if mean is not None and (mean.numel() != cnt or std.numel() != cnt):
        raise ValueError(f"mean / std must have one entry per processed column ({cnt}), got {mean.numel()} / {std.numel()}")
    recs = _rows_table(rows, n, start)
    if state is not None and not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.float32 and
                                  state.is_contiguous() and state.numel() == recs.shape[0] * cnt * 2):
        raise ValueError(f"state must be a contiguous float32 CUDA tensor [R, count, 2] = [{recs.shape[0]}, {cnt}, 2]")
    if state is None and (recs[:, 2] > 0).any():
        raise ValueError("a recording that continues (start > 0) needs the state of the call before it")
    out = logmel.float().clone(memory_format=torch.contiguous_format)
    if n == 0:
        return out
    m32, i32 = _scaler(mean, std, out.device)
    _pcen_launch(out, settings, settings.smoothing(sr, hop), recs, col0, cnt, m32, i32, state)
    return out


def _mel_identity(m32, i32, n_cols):
    """the scaler a spatial log-mel launch gets when PCEN follows: identity on the first ``n_cols`` (mel) columns, whose real
    entries go to the PCEN launch (returned second)"""
    if m32 is None:
        return (None, None), (None, None)
    g_m, g_i = m32.clone(), i32.clone()
    g_m[:n_cols] = 0.0
    g_i[:n_cols] = 1.0
    return (g_m, g_i), (m32[:n_cols].contiguous(), i32[:n_cols].contiguous())


def mbe(y, sr=SR, n_fft=NFFT, hop=HOP, n_mels=NB_MEL, pad_mode="constant", mean=None, std=None, tables=None, input_sr=None,
        channels=1, keep_channels=False, device=None, spatial=None, compress=None):
    """y: mono float32 PCM CUDA tensor [N] -> [1 + N//hop, n_mels] log-mel energies (natural log, no eps).
    ``tables`` = build_tables(window, melfb, device) replaces librosa's default window / filterbank.
    ``input_sr`` / ``channels``: y is at that rate (default: ``sr``), int16 or float, ``[N, channels]`` interleaved when
    channels > 1 (host or device), and is converted, downmixed and resampled to ``sr`` on the device first (resample.py).
    ``keep_channels=True``: the channels are kept, not mixed -> ``[1 + N'//hop, channels*n_mels]``, channel c in columns
    ``[c*n_mels, (c+1)*n_mels)`` (the layout the nets read), each bit for bit ``mbe(y[:, c])``; ``mean`` / ``std`` are then
    ``channels*n_mels`` wide.  ``device``: where a host clip that goes through resample.py is put.
    ``spatial="gcc_phat"`` (with ``keep_channels=True``, 2..8 channels): one GCC-PHAT image per microphone pair
    behind the mel images -> ``[.., (C+P)*n_mels]``, P = C(C-1)/2; ``mean`` / ``std`` are then that wide.
    ``compress=PCEN(...)``: the mel columns hold PCEN instead of the log — the front end as before without the
    scaler on them, then ``sed_pcen`` with it, bit for bit ``pcen(mbe(y), compress, ...)``; every mel column (of every kept
    channel) is its own chain, GCC columns are what they are without ``compress``; ``mean`` / ``std`` keep their width."""
    _check_spatial(spatial, keep_channels, channels)
    _check_compress(compress)
    if keep_channels:
        return mbe_many([y], sr=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, pad_mode=pad_mode, mean=mean, std=std, tables=tables,
                        device=device, input_sr=input_sr, channels=channels, keep_channels=True, spatial=spatial, compress=compress)[0]
    if _needs_front_end(y, input_sr, sr, channels):
        from .resample import resample
        y = resample(y, sr if input_sr is None else input_sr, sr, channels, device)
    if not (isinstance(y, torch.Tensor) and y.is_cuda):
        raise RuntimeError("sed_crnn_amd.feature.mbe needs a CUDA(HIP) tensor; there is no CPU fallback")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    y = y.contiguous().float()
    if tables is None:
        tables = _tables(y.device.index or 0, sr, n_fft, n_mels)
    else:
        n_mels = _validated_mels(tables)
    frames = 1 + y.numel() // hop
    out = torch.empty(frames, n_mels, device=y.device)
    mean, inv = _scaler(mean, std, y.device)
    if compress is not None:
        if mean is not None and (mean.numel() != n_mels or inv.numel() != n_mels):
            raise ValueError(f"mean / std must have n_mels = {n_mels} entries, got {mean.numel()} / {inv.numel()}")
        check(lib().sed_logmel(ptr(y), y.numel(), ptr(tables), tables.numel() * 4, None, None, ptr(out), n_fft, hop,
                               n_mels, {"constant": 0, "reflect": 1}[pad_mode], stream_ptr()), "sed_logmel")
        _pcen_launch(out, compress, compress.smoothing(sr, hop), [(0, frames, 0)], 0, n_mels, mean, inv, None)
        return out
    check(lib().sed_logmel(ptr(y), y.numel(), ptr(tables), tables.numel() * 4, ptr(mean), ptr(inv), ptr(out), n_fft, hop,
                           n_mels, {"constant": 0, "reflect": 1}[pad_mode], stream_ptr()), "sed_logmel")
    return out


def mbe_packed(pcm, clips, sr=SR, n_fft=NFFT, hop=HOP, n_mels=NB_MEL, pad_mode="constant", mean=None, std=None, tables=None,
               compress=None):
    """R clips that lie in ONE mono float32 CUDA buffer ``pcm``, ``clips`` = [(first sample, n_samples >= 1), ...] -> (features
    [sum_r (1 + n_r//hop), n_mels] in clip order, row offsets [R+1] as a host list), in one launch (``sed_logmel_batch``).
    Each clip's rows are bit for bit ``mbe(clip)`` with the same options (its own centre padding at its own ends).
    ``compress=PCEN(...)``: as in ``mbe`` — one ``sed_pcen`` call over all clips, every clip its own smoother."""
    import ctypes as C
    _check_compress(compress)
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dim() == 1):
        raise RuntimeError("sed_crnn_amd.feature.mbe_packed needs a 1-D CUDA(HIP) PCM buffer; there is no CPU fallback")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    R = table.shape[0]
    for i, (o, n) in enumerate(table.tolist()):
        if n < 1 or o < 0 or o + n > pcm.numel():
            raise ValueError(f"clip {i} (first sample {o}, {n} samples) is empty or not inside the buffer of {pcm.numel()} samples")
    if R == 0:
        return torch.empty(0, n_mels, device=pcm.device), [0]
    rows = np.concatenate([[0], np.cumsum(1 + table[:, 1] // hop)]).tolist()
    if tables is None:
        tables = _tables(pcm.device.index or 0, sr, n_fft, n_mels)
    else:
        n_mels = _validated_mels(tables)
    out = torch.empty(rows[-1], n_mels, device=pcm.device)
    if rows[-1] >= 2 ** 31:
        raise ValueError(f"{rows[-1]} feature frames in one batch: at most 2^31 - 1")
    pcm = pcm.contiguous().float()
    mean, inv = _scaler(mean, std, pcm.device)
    ws = torch.empty(lib().sed_logmel_batch_workspace_bytes(R), dtype=torch.uint8, device=pcm.device)
    if compress is not None and mean is not None and (mean.numel() != n_mels or inv.numel() != n_mels):
        raise ValueError(f"mean / std must have n_mels = {n_mels} entries, got {mean.numel()} / {inv.numel()}")
    lm_mean, lm_inv = (None, None) if compress is not None else (mean, inv)
    check(lib().sed_logmel_batch(ptr(pcm), pcm.numel(), C.c_void_p(table.ctypes.data), R, ptr(tables), tables.numel() * 4,
                                 ptr(lm_mean), ptr(lm_inv), ptr(out), rows[-1], n_fft, hop, n_mels,
                                 {"constant": 0, "reflect": 1}[pad_mode], ptr(ws), ws.numel(), stream_ptr()), "sed_logmel_batch")
    if compress is not None:
        _pcen_launch(out, compress, compress.smoothing(sr, hop), _rows_table(rows, rows[-1]), 0, n_mels, mean, inv, None)
    return out, rows


def mbe_planar(pcm, clips, channels, sr=SR, n_fft=NFFT, hop=HOP, n_mels=NB_MEL, pad_mode="constant", mean=None, std=None,
               tables=None, spatial=None, compress=None):
    """The multichannel twin of ``mbe_packed``: R recordings of ``channels`` planar channels each, all in ONE mono float32 CUDA
    buffer ``pcm``; ``clips`` = [(first sample, n_samples >= 1), ...] has ``R * channels`` entries, recording r, channel c at
    ``r * channels + c`` (what ``resample_many(..., keep_channels=True)`` returns), the channels of a recording equally long
    -> (features [sum_r (1 + n_r//hop), channels*n_mels], row offsets [R+1] as a host list), in one launch
    (``sed_logmel_multi``).  Columns ``[c*n_mels, (c+1)*n_mels)`` are bit for bit ``mbe`` of channel c with that slice of
    ``mean`` / ``std`` (``channels*n_mels`` wide: ``data.standard_scaler_fit`` on such features).
    ``spatial="gcc_phat"`` (2..8 channels, even ``n_mels``; ``sed_logmel_gcc``): the P = C(C-1)/2 microphone pairs
    (i, j), i < j in lexicographic order, follow as columns ``[(C+p)*n_mels, (C+p+1)*n_mels)``: the GCC-PHAT of the frame at
    lags -n_mels/2 .. n_mels/2 - 1 (channel j = channel i delayed by d samples peaks at column n_mels/2 - d); the mel columns
    are bit for bit those without ``spatial``, and ``mean`` / ``std`` are ``(C+P)*n_mels`` wide.
    ``compress=PCEN(...)``: the ``channels*n_mels`` mel columns, each its own chain, hold PCEN (``sed_pcen`` with their
    part of the scaler, after a front-end launch that leaves them unscaled); GCC columns are bit for bit those without it."""
    import ctypes as C
    _check_spatial(spatial, True, channels)
    _check_compress(compress)
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dim() == 1):
        raise RuntimeError("sed_crnn_amd.feature.mbe_planar needs a 1-D CUDA(HIP) PCM buffer; there is no CPU fallback")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    nc = int(channels)
    if not 1 <= nc <= 64:
        raise ValueError(f"channels must be 1..64, got {channels}")
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    if table.shape[0] % nc:
        raise ValueError(f"{table.shape[0]} clips are not a whole number of recordings of {nc} channels")
    R = table.shape[0] // nc
    for i, (o, n) in enumerate(table.tolist()):
        if n < 1 or o < 0 or o + n > pcm.numel():
            raise ValueError(f"recording {i // nc}, channel {i % nc} (first sample {o}, {n} samples) is empty or not inside the "
                             f"buffer of {pcm.numel()} samples")
        if n != table[i - i % nc, 1]:
            raise ValueError(f"recording {i // nc}: channel {i % nc} has {n} samples, channel 0 has {int(table[i - i % nc, 1])}")
    if tables is None:
        tables = _tables(pcm.device.index or 0, sr, n_fft, n_mels)
    else:
        n_mels = _validated_mels(tables)
    _check_spatial(spatial, True, nc, n_mels)
    width = (spatial_channels(nc) if spatial else nc) * n_mels
    if R == 0:
        return torch.empty(0, width, device=pcm.device), [0]
    rows = np.concatenate([[0], np.cumsum(1 + table[::nc, 1] // hop)]).tolist()
    if rows[-1] >= 2 ** 31:
        raise ValueError(f"{rows[-1]} feature frames in one batch: at most 2^31 - 1")
    if mean is not None and (mean.numel() != width or std.numel() != width):
        if spatial:
            raise ValueError(f"mean / std must have (C+P)*n_mels = ({nc}+{nc * (nc - 1) // 2})*{n_mels} = {width} entries with "
                             f"spatial={spatial!r} (the {nc} mel images, then one GCC image per microphone pair), got "
                             f"{mean.numel()} / {std.numel()}")
        raise ValueError(f"mean / std must have {nc}*{n_mels} = {nc * n_mels} entries (channel c, band m at c*{n_mels} + m), got "
                         f"{mean.numel()} / {std.numel()}")
    out = torch.empty(rows[-1], width, device=pcm.device)
    pcm = pcm.contiguous().float()
    mean, inv = _scaler(mean, std, pcm.device)
    if compress is not None:                                     # the mel columns leave the front end unscaled; PCEN scales them
        (mean, inv), pc_scaler = _mel_identity(mean, inv, nc * n_mels) if spatial else ((None, None), (mean, inv))
    if spatial:
        ws = torch.empty(lib().sed_logmel_gcc_workspace_bytes(R, nc), dtype=torch.uint8, device=pcm.device)
        check(lib().sed_logmel_gcc(ptr(pcm), pcm.numel(), C.c_void_p(table.ctypes.data), R, nc, ptr(tables), tables.numel() * 4,
                                   ptr(mean), ptr(inv), ptr(out), rows[-1], n_fft, hop, n_mels, n_mels,
                                   {"constant": 0, "reflect": 1}[pad_mode], ptr(ws), ws.numel(), stream_ptr()), "sed_logmel_gcc")
        if compress is not None:
            _pcen_launch(out, compress, compress.smoothing(sr, hop), _rows_table(rows, rows[-1]), 0, nc * n_mels, *pc_scaler, None)
        return out, rows
    ws = torch.empty(lib().sed_logmel_multi_workspace_bytes(R, nc), dtype=torch.uint8, device=pcm.device)
    check(lib().sed_logmel_multi(ptr(pcm), pcm.numel(), C.c_void_p(table.ctypes.data), R, nc, ptr(tables), tables.numel() * 4,
                                 ptr(mean), ptr(inv), ptr(out), rows[-1], n_fft, hop, n_mels,
                                 {"constant": 0, "reflect": 1}[pad_mode], ptr(ws), ws.numel(), stream_ptr()), "sed_logmel_multi")
    if compress is not None:
        _pcen_launch(out, compress, compress.smoothing(sr, hop), _rows_table(rows, rows[-1]), 0, nc * n_mels, *pc_scaler, None)
    return out, rows


def _tdoa_io(events, R, rec_key, nc, max_lag, return_curve, dev):
    """the event columns of ``event_tdoa`` / ``event_tdoa_ring`` as contiguous int32 device tensors (``rec_key`` names the
    recording column, needed when R > 1) and the empty outputs -> (columns with the recording under "rec", E, outputs)"""
    col = {}
    for k in ("onset", "offset", "peak_frame") + ((rec_key,) if R > 1 else ()):
        if k not in events:
            raise ValueError(f"events has no {k!r}" + (f" ({R} recordings need one)" if k == rec_key else ""))
        col["rec" if k == rec_key else k] = events[k].to(dev, torch.int32).contiguous()
    E = col["onset"].numel()
    if any(v.dim() != 1 or v.numel() != E for v in col.values()):
        raise ValueError("the event columns must be 1-D and equally long")
    P, W = nc * (nc - 1) // 2, 2 * max_lag + 3
    out = {"lag": torch.empty(E, P, device=dev), "strength": torch.empty(E, P, device=dev),
           "loc_frames": torch.empty(E, dtype=torch.int32, device=dev)}
    if return_curve:
        out["acc"] = torch.empty(E, P, W, device=dev)
    return col, E, out


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


def event_doa(pcm, clips, channels, events, time_factor, doa, sr=SR, hop=HOP, pad_mode="constant", return_curve=False,
              return_map=False, max_workspace_bytes=128 << 20):
    """Per-event direction of arrival for a known array (``sed_event_doa``): ``event_tdoa`` with ``max_lag`` and
    ``max_frames`` taken from ``doa`` (a ``sed.DOA(positions, grid, ...)``; ``sr``: the rate of the PCM), and for every event
    the direction of ``doa.grid`` with the largest steered response power, summed over all microphone pairs at lags of
    ``1 / doa.oversample`` sample.  Returns the dict of ``event_tdoa`` — the same bits — with ``dir`` int32 [E] (a row of the
    grid; -1: the event has no frames, or digital silence) and ``doa_power`` float32 [E] (the response per pair and frame at
    that direction, in [-1, 1]; 0 where ``dir`` is -1); ``return_map=True`` adds ``srp`` float32 [E, D], the response at every
    direction (secondary peaks are other sources or reflections).  One more launch per slice; the host reads nothing back."""
    return event_tdoa(pcm, clips, channels, events, time_factor, max_frames=getattr(doa, "max_frames", 256),
                      hop=hop, pad_mode=pad_mode, return_curve=return_curve, max_workspace_bytes=max_workspace_bytes,
                      _doa=(doa, sr, return_map))


def event_doa_ring(ring, cap, n, channels, events, time_factor, doa, sr=SR, hop=HOP, lat_frames=0, history_frames=0x7fffffff,
                   return_curve=False, return_map=False, max_workspace_bytes=128 << 20):
    """``event_doa`` on the PCM rings of live feeds (``sed_event_doa_ring``): the arguments and rules of
    ``event_tdoa_ring``, the outputs of ``event_doa``; an event the stream's rule or the ring's depth refuses has ``dir = -1``
    and ``doa_power = 0``.  A located event gets, bit for bit, what ``event_doa`` gives on the feed's samples laid out linearly."""
    return event_tdoa_ring(ring, cap, n, channels, events, time_factor, max_frames=getattr(doa, "max_frames", 256),
                           hop=hop, lat_frames=lat_frames, history_frames=history_frames, return_curve=return_curve,
                           max_workspace_bytes=max_workspace_bytes, _doa=(doa, sr, return_map))


def event_tdoa(pcm, clips, channels, events, time_factor, max_lag=24, max_frames=256, hop=HOP, pad_mode="constant",
               return_curve=False, max_workspace_bytes=128 << 20, _doa=None):
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
    import ctypes as C
    from .localize import MAX_LAG_LIMIT
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dim() == 1):
        raise RuntimeError("sed_crnn_amd.feature.event_tdoa needs a 1-D CUDA(HIP) PCM buffer; there is no CPU fallback")
    if pad_mode not in ("constant", "reflect"):
        raise ValueError(f"pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
    nc, tf, max_lag, max_frames, hop = int(channels), int(time_factor), int(max_lag), int(max_frames), int(hop)
    if _doa is not None:                                              # (doa, sr, return_map) of event_doa: its max_lag
        max_lag = _doa_plan(_doa[0], nc, _doa[1])
    if not 2 <= nc <= GCC_MAX_CHANNELS:
        raise ValueError(f"event_tdoa needs 2 to {GCC_MAX_CHANNELS} audio channels (one estimate per microphone pair), got channels={nc}")
    if not 1 <= max_lag <= MAX_LAG_LIMIT or max_frames < 1 or tf < 1 or hop < 1:
        raise ValueError(f"event_tdoa needs 1 <= max_lag <= {MAX_LAG_LIMIT}, max_frames >= 1, time_factor >= 1 and hop >= 1, got "
                         f"max_lag={max_lag}, max_frames={max_frames}, time_factor={tf}, hop={hop}")
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    if table.shape[0] == 0 or table.shape[0] % nc:
        raise ValueError(f"{table.shape[0]} clips are not a whole number (>= 1) of recordings of {nc} channels")
    R = table.shape[0] // nc
    for i, (o, n) in enumerate(table.tolist()):
        if n < 1 or o < 0 or o + n > pcm.numel():
            raise ValueError(f"recording {i // nc}, channel {i % nc} (first sample {o}, {n} samples) is empty or not inside the "
                             f"buffer of {pcm.numel()} samples")
        if n != table[i - i % nc, 1]:
            raise ValueError(f"recording {i // nc}: channel {i % nc} has {n} samples, channel 0 has {int(table[i - i % nc, 1])}")
    dev = pcm.device
    col, E, out = _tdoa_io(events, R, "rec", nc, max_lag, return_curve, dev)
    extra = _doa_io(_doa[0], _doa[1], E, dev, out, _doa[2]) if _doa is not None else None
    if E == 0:
        return out
    pcm = pcm.contiguous().float()
    tables = _tables(dev.index or 0, SR, NFFT, NB_MEL)                # the window and the twiddles; the mel plan is not read
    longest = int(table[:, 1].max())
    need_one = lib().sed_event_tdoa_workspace_bytes(R, nc, 1, longest, hop, max_frames)
    need_all = lib().sed_event_tdoa_workspace_bytes(R, nc, E, longest, hop, max_frames)
    if need_one == 0:
        raise ValueError(f"sed_event_tdoa_workspace_bytes refuses R={R}, channels={nc}, hop={hop}, max_frames={max_frames}")
    ws = torch.empty(min(need_all, max(need_one, int(max_workspace_bytes))), dtype=torch.uint8, device=dev)
    args = [ptr(pcm), pcm.numel(), C.c_void_p(table.ctypes.data), R, nc, ptr(tables), tables.numel() * 4, ptr(col.get("rec")),
            ptr(col["onset"]), ptr(col["offset"]), ptr(col["peak_frame"]), E, tf, hop, {"constant": 0, "reflect": 1}[pad_mode], max_lag,
            max_frames, ptr(out["lag"]), ptr(out["strength"]), ptr(out["loc_frames"]), ptr(out.get("acc"))]
    if _doa is None:
        check(lib().sed_event_tdoa(*args, ptr(ws), ws.numel(), stream_ptr()), "sed_event_tdoa")
    else:                                                             # the same launches and one more
        check(lib().sed_event_doa(*args, *extra, ptr(ws), ws.numel(), stream_ptr()), "sed_event_doa")
    return out


def ring_write(ring, cap, src, table, workspace=None):
    """A round's new samples into the PCM rings of live feeds (``sed_stream_ring_write``).  ``ring``: float32 CUDA
    buffer of ``lanes * cap`` samples, lane l (feed s, channel c: ``s*C + c``) keeps its last ``cap`` samples, sample i of the
    lane at ``ring[l*cap + i % cap]``; ``src``: the new samples, packed (float32 CUDA, or None when every count is 0);
    ``table`` [lanes, 3] host ints ``{first sample in src, count <= cap, absolute index of the first sample}``.  One launch;
    the host reads nothing back.  -> the workspace, for the next call."""
    import ctypes as C
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dim() == 1 and ring.dtype == torch.float32 and ring.is_contiguous()):
        raise RuntimeError("sed_crnn_amd.feature.ring_write needs a contiguous 1-D float32 CUDA(HIP) ring buffer; there is no CPU fallback")
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


def event_tdoa_ring(ring, cap, n, channels, events, time_factor, max_lag=24, max_frames=256, hop=HOP, lat_frames=0,
                    history_frames=0x7fffffff, return_curve=False, max_workspace_bytes=128 << 20, _doa=None):
    """``event_tdoa`` on the PCM rings of live feeds (``sed_event_tdoa_ring``).  ``ring`` / ``cap`` as ``ring_write``
    fills them: feed r's ``channels`` lanes are the rings ``r*channels + c``; ``n`` [R] host ints: the samples feed r has
    received.  ``events`` as ``event_tdoa`` takes them; the feed of an event is its ``rec`` — or ``stream`` — column (needed
    when R > 1).  An event is located on ``localize.event_frames`` with ``n_feat = 1 + n // hop`` unless
    ``offset*tf + lat_frames - f0 > history_frames`` (``localize.stream_locates``: the stream's rule) or its first sample has
    left the ring (``max(0, f0*hop - 1024) < n - cap``): then ``loc_frames = 0``, ``lag = 0``, ``strength = 0`` and nothing is
    read.  Samples before the start of the feed and beyond ``n`` read as 0 (constant padding).  A located event gets, bit for
    bit, what ``event_tdoa`` gives on the feed's samples ``[0, n)`` laid out linearly, wherever the ring wraps.  Returns the
    dict ``event_tdoa`` returns; the host reads nothing back."""
    import ctypes as C
    from .localize import MAX_LAG_LIMIT
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dim() == 1 and ring.dtype == torch.float32 and ring.is_contiguous()):
        raise RuntimeError("sed_crnn_amd.feature.event_tdoa_ring needs a contiguous 1-D float32 CUDA(HIP) ring buffer; there is no CPU fallback")
    nc, tf, max_lag, max_frames, hop, cap = int(channels), int(time_factor), int(max_lag), int(max_frames), int(hop), int(cap)
    lat, hist = int(lat_frames), int(history_frames)
    if _doa is not None:                                              # (doa, sr, return_map) of event_doa_ring: its max_lag
        max_lag = _doa_plan(_doa[0], nc, _doa[1])
    if not 2 <= nc <= GCC_MAX_CHANNELS:
        raise ValueError(f"event_tdoa_ring needs 2 to {GCC_MAX_CHANNELS} audio channels (one estimate per microphone pair), got channels={nc}")
    if not 1 <= max_lag <= MAX_LAG_LIMIT or max_frames < 1 or tf < 1 or hop < 1 or lat < 0 or hist < 1:
        raise ValueError(f"event_tdoa_ring needs 1 <= max_lag <= {MAX_LAG_LIMIT}, max_frames >= 1, time_factor >= 1, hop >= 1, lat_frames >= 0 "
                         f"and history_frames >= 1, got max_lag={max_lag}, max_frames={max_frames}, time_factor={tf}, hop={hop}, "
                         f"lat_frames={lat}, history_frames={hist}")
    n = np.ascontiguousarray(np.asarray(n, dtype=np.int64).reshape(-1))
    R = n.shape[0]
    if R < 1 or (n < 0).any():
        raise ValueError(f"n must hold one sample count >= 0 per feed, got {n.tolist()[:8]}")
    if cap < NFFT or cap % 4 or R * nc * cap > ring.numel():
        raise ValueError(f"{R} feeds of {nc} rings of cap={cap} samples (a multiple of 4, at least {NFFT}) do not fit the ring buffer of "
                         f"{ring.numel()} samples")
    dev = ring.device
    rec_key = "stream" if "stream" in events and "rec" not in events else "rec"
    col, E, out = _tdoa_io(events, R, rec_key, nc, max_lag, return_curve, dev)
    extra = _doa_io(_doa[0], _doa[1], E, dev, out, _doa[2]) if _doa is not None else None
    if E == 0:
        return out
    tables = _tables(dev.index or 0, SR, NFFT, NB_MEL)                # the window and the twiddles; the mel plan is not read
    need_one = lib().sed_event_tdoa_ring_workspace_bytes(R, nc, 1, cap, hop, max_frames)
    need_all = lib().sed_event_tdoa_ring_workspace_bytes(R, nc, E, cap, hop, max_frames)
    if need_one == 0:
        raise ValueError(f"sed_event_tdoa_ring_workspace_bytes refuses R={R}, channels={nc}, cap={cap}, hop={hop}, max_frames={max_frames}")
    ws = torch.empty(min(need_all, max(need_one, int(max_workspace_bytes))), dtype=torch.uint8, device=dev)
    args = [ptr(ring), ring.numel(), cap, C.c_void_p(n.ctypes.data), R, nc, ptr(tables), tables.numel() * 4, ptr(col.get("rec")),
            ptr(col["onset"]), ptr(col["offset"]), ptr(col["peak_frame"]), E, tf, hop, max_lag, max_frames, lat, hist, ptr(out["lag"]),
            ptr(out["strength"]), ptr(out["loc_frames"]), ptr(out.get("acc"))]
    if _doa is None:
        check(lib().sed_event_tdoa_ring(*args, ptr(ws), ws.numel(), stream_ptr()), "sed_event_tdoa_ring")
    else:
        check(lib().sed_event_doa_ring(*args, *extra, ptr(ws), ws.numel(), stream_ptr()), "sed_event_doa_ring")
    return out


def _located_cols(events, R, rec_key, dev):
    """the columns of located events as the C entries of both beams take them (``rec_key`` names the recording column, needed
    when R > 1) -> ([rec, onset, offset, peak_frame, dir, loc_frames] as pointers to contiguous int32 device tensors, E)"""
    col = {}
    for k in ("onset", "offset", "peak_frame", "dir", "loc_frames") + ((rec_key,) if R > 1 else ()):
        if k not in events:
            raise ValueError(f"events has no {k!r}" + (f" ({R} recordings need one)" if k == rec_key else
                                                       " (the events must be located: feature.event_doa)" if k in ("dir", "loc_frames") else ""))
        col["rec" if k == rec_key else k] = events[k].to(dev, torch.int32).contiguous()
    E = col["onset"].numel()
    if any(v.dim() != 1 or v.numel() != E for v in col.values()):
        raise ValueError("the event columns must be 1-D and equally long")
    cols = [ptr(col.get("rec")), ptr(col["onset"]), ptr(col["offset"]), ptr(col["peak_frame"]), ptr(col["dir"]), ptr(col["loc_frames"])]
    return _Kept(cols, col), E


class _Kept(list):
    """a list of pointers that keeps the tensors they point into alive"""

    def __init__(self, items, owner):
        super().__init__(items)
        self.owner = owner


def _beam_io(who, events, R, rec_key, nc, doa, beam, sr, dev):
    """checks the settings of a beam call and gathers what both entries pass on -> (event columns as the C entries take them, E,
    [max_frames, M, D, Q, H, taps] with M and the taps on ``dev``: uploaded once per device, rate and filter)"""
    from .localize import DelaySum
    _doa_plan(doa, nc, sr)
    if not isinstance(beam, DelaySum):
        raise TypeError(f"{who} takes the beam settings as a sed.DelaySum(...) object, got {type(beam).__name__}")
    cols, E = _located_cols(events, R, rec_key, dev)
    key = (dev.index or 0, float(sr), beam.oversample)
    if key not in doa._beam_device:
        doa._beam_device[key] = torch.from_numpy(doa.delays(sr, beam.oversample)).to(dev)
    tkey = (dev.index or 0, beam)
    if tkey not in _BEAM_TAPS:
        _BEAM_TAPS[tkey] = torch.from_numpy(beam.taps.copy()).to(dev)                # (the cached table is read-only)
    M = doa._beam_device[key]
    return cols, E, [doa.max_frames, ptr(M), M.shape[0], beam.oversample, beam.half_width, ptr(_BEAM_TAPS[tkey])]


_BEAM_TAPS = {}              # (device, DelaySum) -> the filter on the device


def _beam_empty(dev):
    return {"audio": torch.empty(0, device=dev), "audio_start": torch.empty(0, dtype=torch.int64, device=dev),
            "audio_len": torch.empty(0, dtype=torch.int32, device=dev)}


def _beam_run(names, head, cols, E, tf, hop, plan, need, dev):
    """the two calls of a beam entry: the spans, ONE blocking read of the total (8 bytes) to size ``audio``, the beam"""
    max_frames, M, D, Q, H, taps = plan
    out = {"audio_start": torch.empty(E, dtype=torch.int64, device=dev), "audio_len": torch.empty(E, dtype=torch.int32, device=dev)}
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    check(getattr(lib(), names[0])(*head[1], *cols, E, tf, hop, max_frames, D, ptr(out["audio_len"]), ptr(out["audio_start"]), ptr(total),
                                   ptr(ws), ws.numel(), stream_ptr()), names[0])
    n_total = int(total.item())
    out["audio"] = torch.empty(n_total, device=dev)
    check(getattr(lib(), names[1])(*head[0], *head[1], *cols, E, tf, hop, max_frames, M, D, Q, H, taps, ptr(out["audio_len"]),
                                   ptr(out["audio_start"]), ptr(out["audio"]), n_total, ptr(ws), ws.numel(), stream_ptr()), names[1])
    return out


def _planar_recordings(who, pcm, clips, channels, time_factor, hop):
    """checks the PCM buffer and the clip table of ``event_beamform`` / ``event_mvdr`` -> (channels, time_factor, hop, the table as
    int64 [R * channels, 2], R)"""
    if not (isinstance(pcm, torch.Tensor) and pcm.is_cuda and pcm.dim() == 1):
        raise RuntimeError(f"sed_crnn_amd.feature.{who} needs a 1-D CUDA(HIP) PCM buffer; there is no CPU fallback")
    nc, tf, hop = int(channels), int(time_factor), int(hop)
    if not 2 <= nc <= GCC_MAX_CHANNELS or tf < 1 or hop < 1:
        raise ValueError(f"{who} needs 2 to {GCC_MAX_CHANNELS} audio channels, time_factor >= 1 and hop >= 1, got channels={nc}, "
                         f"time_factor={tf}, hop={hop}")
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    if table.shape[0] == 0 or table.shape[0] % nc:
        raise ValueError(f"{table.shape[0]} clips are not a whole number (>= 1) of recordings of {nc} channels")
    for i, (o, n) in enumerate(table.tolist()):
        if n < 1 or o < 0 or o + n > pcm.numel():
            raise ValueError(f"recording {i // nc}, channel {i % nc} (first sample {o}, {n} samples) is empty or not inside the "
                             f"buffer of {pcm.numel()} samples")
        if n != table[i - i % nc, 1]:
            raise ValueError(f"recording {i // nc}: channel {i % nc} has {n} samples, channel 0 has {int(table[i - i % nc, 1])}")
    return nc, tf, hop, table, table.shape[0] // nc


@functools.lru_cache(maxsize=8)
def _mvdr_tables(device_index):
    """the 2048-point tables with the MVDR beam's window (``localize.mvdr_window``): the header, window and twiddle sections of a
    ``build_tables`` blob — the mel plan behind them is not read and not kept — cached per device"""
    from .localize import mvdr_window
    blob = build_tables(mvdr_window(), slaney_mel_basis(SR, NFFT, NB_MEL), torch.device("cuda", device_index))
    return blob[:_LM_OFF_ENT].clone()


def event_mvdr(pcm, clips, channels, events, time_factor, doa, mvdr, sr=SR, hop=HOP, max_workspace_bytes=128 << 20):
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
    Kn where the noise covariance was used, else 0.  An event's audio then depends on those samples and its own alone."""
    import ctypes as C
    from .localize import MVDR
    nc, tf, hop, table, R = _planar_recordings("event_mvdr", pcm, clips, channels, time_factor, hop)
    _doa_plan(doa, nc, sr)
    if not isinstance(mvdr, MVDR):
        raise TypeError(f"event_mvdr takes the beam settings as a sed.MVDR(...) object, got {type(mvdr).__name__}")
    dev = pcm.device
    cols, E = _located_cols(events, R, "rec", dev)
    if E == 0:
        return _mvdr_empty(dev, mvdr)
    pcm = pcm.contiguous().float()
    need_one = _mvdr_workspace("sed_event_mvdr", R, nc, doa.max_frames, hop, mvdr)
    head = ([ptr(pcm)], [pcm.numel(), C.c_void_p(table.ctypes.data), R, nc])
    return _mvdr_run(("sed_event_beam_spans", "sed_event_mvdr"), head, cols, E, tf, hop, doa, mvdr, sr,
                     lib().sed_event_beam_workspace_bytes(R, nc), need_one, max_workspace_bytes, dev)


def _mvdr_empty(dev, mvdr):
    out = _beam_empty(dev)
    if mvdr.noise_blocks:
        out["noise_frames"] = torch.empty(0, dtype=torch.int32, device=dev)
    return out


def _mvdr_workspace(entry, R, nc, max_frames, hop, mvdr):
    """the workspace bytes of the recording table and one event of ``entry`` (``sed_event_mvdr`` / ``sed_event_mvdr_ring``), or of
    its noise form where ``mvdr.noise_blocks >= 1``"""
    if mvdr.noise_blocks:
        name, args = entry.replace("sed_event_mvdr", "sed_event_mvdr_noise") + "_workspace_bytes", (R, nc, max_frames, hop, mvdr.noise_blocks)
    else:
        name, args = entry + "_workspace_bytes", (R, nc, max_frames, hop)
    need_one = getattr(lib(), name)(*args)
    if need_one == 0:
        raise ValueError(f"{name} refuses R={R}, channels={nc}, max_frames={max_frames}, hop={hop}")
    return need_one


def _mvdr_run(names, head, cols, E, tf, hop, doa, mvdr, sr, need_tab, need_one, max_workspace_bytes, dev):
    """the two calls of an MVDR entry, linear or ring: the spans, ONE blocking read of the total (8 bytes) to size ``audio``, the
    beam; ``need_tab`` / ``need_one``: the workspace bytes of the recording table alone and with one event.  With
    ``mvdr.noise_blocks >= 1`` the beam is the entry's noise form and the dict gains ``noise_frames`` int32 [E]"""
    key = (dev.index or 0, float(sr))
    if key not in doa._steering_device:
        doa._steering_device[key] = torch.from_numpy(doa.steering(sr)).to(dev)
    tau = doa._steering_device[key]
    tables = _mvdr_tables(dev.index or 0)
    out = {"audio_start": torch.empty(E, dtype=torch.int64, device=dev), "audio_len": torch.empty(E, dtype=torch.int32, device=dev)}
    total = torch.empty(1, dtype=torch.int64, device=dev)
    per_event = need_one - need_tab
    ws = torch.empty(min(need_tab + E * per_event, max(need_one, int(max_workspace_bytes))), dtype=torch.uint8, device=dev)
    check(getattr(lib(), names[0])(*head[1], *cols, E, tf, hop, doa.max_frames, tau.shape[0], ptr(out["audio_len"]),
                                   ptr(out["audio_start"]), ptr(total), ptr(ws), ws.numel(), stream_ptr()), names[0])
    n_total = int(total.item())                                       # the one blocking read
    out["audio"] = torch.empty(n_total, device=dev)
    if mvdr.noise_blocks:
        name = names[1].replace("sed_event_mvdr", "sed_event_mvdr_noise")
        out["noise_frames"] = torch.zeros(E, dtype=torch.int32, device=dev)      # (a call that extracts nothing launches nothing)
        check(getattr(lib(), name)(*head[0], *head[1], *cols, E, tf, hop, doa.max_frames, ptr(tau), tau.shape[0], mvdr.loading,
                                   mvdr.noise_blocks, mvdr.noise_guard, ptr(tables), tables.numel() * 4, ptr(out["audio_len"]),
                                   ptr(out["audio_start"]), ptr(out["audio"]), n_total, ptr(out["noise_frames"]), ptr(ws), ws.numel(),
                                   stream_ptr()), name)
        return out
    check(getattr(lib(), names[1])(*head[0], *head[1], *cols, E, tf, hop, doa.max_frames, ptr(tau), tau.shape[0], mvdr.loading,
                                   ptr(tables), tables.numel() * 4, ptr(out["audio_len"]), ptr(out["audio_start"]), ptr(out["audio"]),
                                   n_total, ptr(ws), ws.numel(), stream_ptr()), names[1])
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
    import ctypes as C
    nc, tf, hop, table, R = _planar_recordings("event_beamform", pcm, clips, channels, time_factor, hop)
    dev = pcm.device
    cols, E, plan = _beam_io("event_beamform", events, R, "rec", nc, doa, beam, sr, dev)
    if E == 0:
        return _beam_empty(dev)
    pcm = pcm.contiguous().float()
    if pcm.data_ptr() % 16:                                           # (a view into a larger buffer: the kernel loads 16 bytes at a time)
        pcm = pcm.clone()
    head = ([ptr(pcm)], [pcm.numel(), C.c_void_p(table.ctypes.data), R, nc])
    return _beam_run(("sed_event_beam_spans", "sed_event_beamform"), head, cols, E, tf, hop, plan,
                     lib().sed_event_beam_workspace_bytes(R, nc), dev)


def event_beamform_ring(ring, cap, n, channels, events, time_factor, doa, beam, sr=SR, hop=HOP):
    """``event_beamform`` on the PCM rings of live feeds (``sed_event_beam_spans_ring`` + ``sed_event_beamform_ring``):
    ``ring`` / ``cap`` / ``n`` as ``event_doa_ring`` takes them, the events with the ``dir`` and ``loc_frames`` it returned (an
    event the stream's rule or the ring's depth refused has ``dir = -1`` and length 0 here); the feed of an event is its
    ``rec`` — or ``stream`` — column.  An extracted event gets, bit for bit, what ``event_beamform`` gives on the feed's samples
    ``[0, n)`` laid out linearly, wherever the ring wraps.  Returns what ``event_beamform`` returns, with the same single
    8-byte read."""
    import ctypes as C
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dim() == 1 and ring.dtype == torch.float32 and ring.is_contiguous()):
        raise RuntimeError("sed_crnn_amd.feature.event_beamform_ring needs a contiguous 1-D float32 CUDA(HIP) ring buffer; there is no CPU fallback")
    nc, tf, hop, cap = int(channels), int(time_factor), int(hop), int(cap)
    if not 2 <= nc <= GCC_MAX_CHANNELS or tf < 1 or hop < 1:
        raise ValueError(f"event_beamform_ring needs 2 to {GCC_MAX_CHANNELS} audio channels, time_factor >= 1 and hop >= 1, got "
                         f"channels={nc}, time_factor={tf}, hop={hop}")
    n = np.ascontiguousarray(np.asarray(n, dtype=np.int64).reshape(-1))
    R = n.shape[0]
    if R < 1 or (n < 0).any():
        raise ValueError(f"n must hold one sample count >= 0 per feed, got {n.tolist()[:8]}")
    if cap < NFFT or cap % 4 or R * nc * cap > ring.numel() or ring.data_ptr() % 16:
        raise ValueError(f"{R} feeds of {nc} rings of cap={cap} samples (a multiple of 4, at least {NFFT}, 16-byte aligned) do not fit the "
                         f"ring buffer of {ring.numel()} samples")
    dev = ring.device
    rec_key = "stream" if "stream" in events and "rec" not in events else "rec"
    cols, E, plan = _beam_io("event_beamform_ring", events, R, rec_key, nc, doa, beam, sr, dev)
    if E == 0:
        return _beam_empty(dev)
    head = ([ptr(ring), ring.numel(), cap], [C.c_void_p(n.ctypes.data), R, nc])
    return _beam_run(("sed_event_beam_spans_ring", "sed_event_beamform_ring"), head, cols, E, tf, hop, plan,
                     lib().sed_event_beam_ring_workspace_bytes(R), dev)


def event_mvdr_ring(ring, cap, n, channels, events, time_factor, doa, mvdr, sr=SR, hop=HOP, max_workspace_bytes=128 << 20):
    """``event_mvdr`` on the PCM rings of live feeds (``sed_event_beam_spans_ring`` + ``sed_event_mvdr_ring``): ``ring`` /
    ``cap`` / ``n`` / ``events`` as ``event_beamform_ring`` takes them (an event the stream's rule or the ring's depth refused
    has ``dir = -1`` and length 0 here; the feed of an event is its ``rec`` — or ``stream`` — column), ``mvdr`` and
    ``max_workspace_bytes`` as ``event_mvdr``.  An extracted event gets, bit for bit, what ``event_mvdr`` gives on the feed's
    samples ``[0, n)`` laid out linearly, wherever the ring wraps and whatever the slicing; a sample the ring no longer holds
    reads as 0.  Returns what ``event_mvdr`` returns, with the same single 8-byte read; ``E == 0`` returns empty tensors without
    a launch."""
    import ctypes as C
    from .localize import MVDR
    if not (isinstance(ring, torch.Tensor) and ring.is_cuda and ring.dim() == 1 and ring.dtype == torch.float32 and ring.is_contiguous()):
        raise RuntimeError("sed_crnn_amd.feature.event_mvdr_ring needs a contiguous 1-D float32 CUDA(HIP) ring buffer; there is no CPU fallback")
    nc, tf, hop, cap = int(channels), int(time_factor), int(hop), int(cap)
    if not 2 <= nc <= GCC_MAX_CHANNELS or tf < 1 or hop < 1:
        raise ValueError(f"event_mvdr_ring needs 2 to {GCC_MAX_CHANNELS} audio channels, time_factor >= 1 and hop >= 1, got "
                         f"channels={nc}, time_factor={tf}, hop={hop}")
    n = np.ascontiguousarray(np.asarray(n, dtype=np.int64).reshape(-1))
    R = n.shape[0]
    if R < 1 or (n < 0).any():
        raise ValueError(f"n must hold one sample count >= 0 per feed, got {n.tolist()[:8]}")
    if cap < NFFT or cap % 4 or R * nc * cap > ring.numel():
        raise ValueError(f"{R} feeds of {nc} rings of cap={cap} samples (a multiple of 4, at least {NFFT}) do not fit the ring buffer of "
                         f"{ring.numel()} samples")
    _doa_plan(doa, nc, sr)
    if not isinstance(mvdr, MVDR):
        raise TypeError(f"event_mvdr_ring takes the beam settings as a sed.MVDR(...) object, got {type(mvdr).__name__}")
    dev = ring.device
    rec_key = "stream" if "stream" in events and "rec" not in events else "rec"
    cols, E = _located_cols(events, R, rec_key, dev)
    if E == 0:
        return _mvdr_empty(dev, mvdr)
    need_one = _mvdr_workspace("sed_event_mvdr_ring", R, nc, doa.max_frames, hop, mvdr)
    head = ([ptr(ring), ring.numel(), cap], [C.c_void_p(n.ctypes.data), R, nc])
    return _mvdr_run(("sed_event_beam_spans_ring", "sed_event_mvdr_ring"), head, cols, E, tf, hop, doa, mvdr, sr,
                     lib().sed_event_beam_ring_workspace_bytes(R), need_one, max_workspace_bytes, dev)


def pack_clips(waves, device):
    """a list of 1-D clips (host arrays or tensors, any device) -> (one float32 buffer on ``device``, [(first sample, n), ...]);
    every clip starts on a 16-byte boundary.  Host clips travel in one copy, device clips are joined by one torch.cat."""
    clips, pieces, at = [], [], 0
    on_host = all(not (isinstance(w, torch.Tensor) and w.is_cuda) for w in waves)
    for i, w in enumerate(waves):
        w = w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w))
        if w.dim() != 1:
            raise ValueError(f"clip {i}: expected a mono 1-D waveform, got shape {tuple(w.shape)}")
        n = w.numel()
        clips.append((at, n))
        pad = -n % 4
        pieces.append(w.float() if on_host else w.to(device, torch.float32))
        if pad:
            pieces.append(torch.zeros(pad, dtype=torch.float32, device="cpu" if on_host else device))
        at += n + pad
    if not pieces:
        return torch.empty(0, device=device), clips
    buf = torch.cat(pieces)
    return (buf.to(device) if on_host else buf), clips


def mbe_many(waves, sr=SR, n_fft=NFFT, hop=HOP, n_mels=NB_MEL, pad_mode="constant", mean=None, std=None, tables=None,
             device=None, input_sr=None, channels=1, keep_channels=False, spatial=None, compress=None, return_pcm=False):
    """``mbe`` of every clip in a list of 1-D clips (host or device; ``device`` defaults to the first CUDA clip's, else
    cuda:current) in one launch -> (features [sum_r (1 + n_r//hop), n_mels] in clip order, row offsets [R+1] host list).
    Bit for bit ``torch.cat([mbe(w) for w in waves])``.  ``input_sr`` (one rate, or one per clip) / ``channels``: as in
    ``mbe``; the clips are resampled straight into the packed buffer the log-mel launch reads (``resample.resample_many``).
    ``keep_channels=True``: every clip is ``[N, channels]`` and its channels are kept -> features ``[.., channels*n_mels]``
    (``mbe_planar``; the resampler writes the planar channels of every clip straight into the buffer that launch reads).
    ``spatial="gcc_phat"``: as in ``mbe_planar`` — bit for bit the per-recording calls.  ``compress=PCEN(...)``: as in ``mbe``;
    one ``sed_pcen`` call for all clips, bit for bit the per-clip calls.  ``return_pcm=True`` (with ``keep_channels=True``): also
    the resampled planar PCM the features were made from -> (features, row offsets, pcm, clips), what ``event_tdoa`` reads."""
    _check_spatial(spatial, keep_channels, channels)
    _check_compress(compress)
    if return_pcm and not keep_channels:
        raise ValueError("return_pcm=True needs keep_channels=True: it returns the planar channels of every recording")
    waves = list(waves)
    if device is None:
        device = next((w.device for w in waves if isinstance(w, torch.Tensor) and w.is_cuda), None)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    if keep_channels:
        from .resample import resample_many
        for i, w in enumerate(waves):
            if len(w) < 1:
                raise ValueError(f"clip {i} is empty")
        pcm, clips = resample_many(waves, sr if input_sr is None else input_sr, sr, channels, device, keep_channels=True)
        out = mbe_planar(pcm, clips, channels, sr=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, pad_mode=pad_mode, mean=mean, std=std,
                         tables=tables, spatial=spatial, compress=compress)
        return out + (pcm, clips) if return_pcm else out
    if input_sr is not None and np.ndim(input_sr) > 0 or any(_needs_front_end(w, input_sr, sr, channels) for w in waves):
        from .resample import resample_many
        pcm, clips = resample_many(waves, sr if input_sr is None else input_sr, sr, channels, device)
    else:
        pcm, clips = pack_clips(waves, device)
    for i, (_, n) in enumerate(clips):
        if n < 1:
            raise ValueError(f"clip {i} is empty")
    return mbe_packed(pcm, clips, sr=sr, n_fft=n_fft, hop=hop, n_mels=n_mels, pad_mode=pad_mode, mean=mean, std=std,
                      tables=tables, compress=compress)


# ───────────────────────── feature.py's on-disk formats ─────────────────────────
def rasterize_hits(n_frames, hits, sr=SR, hop=HOP):
    """Frame labels of one recording from its hit intervals in seconds (feature.py:89-93): frames
    [floor(start*sr/hop), ceil(end*sr/hop)) are 1.  -> float32 [n_frames, 1]"""
    lbl = np.zeros((n_frames, 1), dtype=np.float32)
    for start, end in hits:
        s = int(np.floor(start * sr / hop))
        e = int(np.ceil(end * sr / hop))
        lbl[s:e, 0] = 1.0
    return lbl


def save_video_npz(path, mbe_frames, labels):
    """per-recording cache `{base}_mon.npz` (feature.py:72,95): positional arr_0 = features [n, n_mels], arr_1 = labels [n, 1]"""
    np.savez(path, np.asarray(mbe_frames, dtype=np.float32), np.asarray(labels, dtype=np.float32))


def load_video_npz(path):
    with np.load(path, allow_pickle=False) as d:
        if "arr_0" not in d.files or "arr_1" not in d.files:
            raise ValueError(f"{path}: not a per-recording cache (feature.py:95 saves two positional arrays)")
        mbe_frames, labels = d["arr_0"], d["arr_1"]
    if mbe_frames.shape[0] != labels.shape[0]:
        raise ValueError(f"{path}: {mbe_frames.shape[0]} feature frames but {labels.shape[0]} label frames")
    return mbe_frames, labels


def build_fold_packs(per_video, cache_dir, device="cuda"):
    """feature.py:114-132 on the device: for every fold f the recordings of fold f are the test split and all others the
    train split (concatenated in dict order), a StandardScaler is fitted on the train split and applied to both
    (`data.standard_scaler_fit` / `standard_scaler_transform`: sklearn's rules, float64 statistics), and the pack is saved
    as `mbe_mon_fold{f+1}.npz` with the positional arrays X_train, Y_train, X_test, Y_test that sed.py:119-123 reads.
    ``per_video``: {name: (features [n, F] host or device, labels [n, 1], fold_id)}.  Returns the written paths."""
    import os
    from .data import standard_scaler_fit, standard_scaler_transform
    folds = max(v[2] for v in per_video.values()) + 1
    dev = torch.device(device)
    as_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(dev).float()   # noqa: E731
    feats = {k: (as_dev(v[0]), np.asarray(v[1].cpu() if isinstance(v[1], torch.Tensor) else v[1], dtype=np.float32), v[2])
             for k, v in per_video.items()}
    os.makedirs(cache_dir, exist_ok=True)
    paths = []
    for f in range(folds):
        test = [v for v in feats.values() if v[2] == f]
        train = [v for v in feats.values() if v[2] != f]
        if not test or not train:
            raise ValueError(f"fold {f} has {len(test)} test and {len(train)} train recordings")
        x_train, x_test = torch.cat([v[0] for v in train]), torch.cat([v[0] for v in test])
        mean, scale = standard_scaler_fit(x_train)
        x_train = standard_scaler_transform(x_train, mean, scale, out=x_train)
        x_test = standard_scaler_transform(x_test, mean, scale, out=x_test)
        path = os.path.join(cache_dir, f"mbe_mon_fold{f + 1}.npz")
        np.savez(path, x_train.cpu().numpy(), np.concatenate([v[1] for v in train]), x_test.cpu().numpy(),
                 np.concatenate([v[1] for v in test]))
        paths.append(path)
    return paths
