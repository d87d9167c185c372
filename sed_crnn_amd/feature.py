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


def _clip_table(clips, nc, n_pcm, at_least_one):
    """checks the clip table of planar recordings of ``nc`` channels in a buffer of ``n_pcm`` samples — every channel inside the
    buffer, the channels of a recording equally long, and with ``at_least_one`` a recording to work on — -> it as contiguous int64
    [R * nc, 2]"""
    table = np.ascontiguousarray(np.asarray(clips, dtype=np.int64).reshape(-1, 2))
    if at_least_one and (table.shape[0] == 0 or table.shape[0] % nc):
        raise ValueError(f"{table.shape[0]} clips are not a whole number (>= 1) of recordings of {nc} channels")
    if table.shape[0] % nc:
        raise ValueError(f"{table.shape[0]} clips are not a whole number of recordings of {nc} channels")
    for i, (o, n) in enumerate(table.tolist()):
        if n < 1 or o < 0 or o + n > n_pcm:
            raise ValueError(f"recording {i // nc}, channel {i % nc} (first sample {o}, {n} samples) is empty or not inside the "
                             f"buffer of {n_pcm} samples")
        if n != table[i - i % nc, 1]:
            raise ValueError(f"recording {i // nc}: channel {i % nc} has {n} samples, channel 0 has {int(table[i - i % nc, 1])}")
    return table


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
    table = _clip_table(clips, nc, pcm.numel(), at_least_one=False)
    R = table.shape[0] // nc
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


# The entries over an event table live in events.py and stay importable from here.  This line stays LAST: events.py imports names
# of this module while it is still being executed (whichever of the two is imported first) and may use what stands above only.
from .events import event_beamform, event_beamform_ring, event_contrast_frames, event_doa, event_doa_ring, event_mvdr, event_mvdr_ring, event_quiet_frames, event_tdoa, event_tdoa_ring, ring_write  # noqa: E402,F401
