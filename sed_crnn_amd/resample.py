"""Audio at any sample rate: polyphase resampling, sample-format conversion and downmix on the GPU.

What the reference leaves to ``ffmpeg -ac 1 -ar 44100`` (feature.py:40-50).  A ``ResamplePlan`` is the filter design, made on
the host in float64: ``L/M = sr_out/sr_in`` reduced, a Kaiser-windowed sinc of ``zeros`` zero crossings per side at the lower
of the two rates, cut off at ``rolloff`` of the lower Nyquist, as a table of ``L`` phases x ``K = 2*half`` taps, rounded once
to float32.  Output ``m`` (absolute index) has ``u = m*M``, ``i_c = u // L``, ``p = u % L`` and

    y[m] = sum_k h[p][k] * x[i_c - half + 1 + k]        (x = 0 outside [0, N); a clip of N samples gives ceil(N*L/M))

summed in fp32 in one fixed order (``csrc/resample.hip``), so that a recording resampled in pieces equals the recording
resampled whole, bit for bit.  int16 input (scaled by 1/32768) and interleaved channels ``[N, C]`` (downmixed as
``(sum_c x_c) * (1/C)``) are converted while they are loaded.  With ``keep_channels=True`` the channels are kept instead of
mixed: one row of the launch per (clip, channel), planar mono clips out, each bit for bit the mono call on that
channel.  There is no CPU fallback.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr
from .feature import SR

TILE_OUT = 1024            # outputs per workgroup tile (resample.hip: RS_TILE)
MAX_TABLE_FLOATS = 26_624  # L * (K + 1): the padded table must stay in LDS beside the input tile (resample.hip: RS_TAPS_MAX)
MAX_TILE_SPAN = 8192       # input samples one tile may read (resample.hip: RS_SPAN_MAX)
ROW = 9                    # int64 per row of sed_resample's host table
ROW_SELECT = 10            # ... of sed_resample_select's: the tenth is the channel the row keeps (-1 = downmix)


class ResamplePlan:
    """The filter and the index arithmetic of ``sr_in -> sr_out`` (module docstring).  ``taps`` [L, K] float32 (None for the
    identity plan ``sr_in == sr_out``, which runs no kernel).  Refuses, with the reason, a ratio whose padded table
    ``L * (K + 1)`` exceeds ``MAX_TABLE_FLOATS`` = 26 624 floats (104 KiB: table and input tile share the 160 KiB LDS; the
    largest table among the common rates is 441 x 54 for 8 / 16 / 32 kHz -> 44.1 kHz) or whose tiles would read more than
    ``MAX_TILE_SPAN`` input samples (``sr_in`` above about 7.5 ``sr_out``)."""

    def __init__(self, sr_in, sr_out=SR, zeros=24, rolloff=0.92, beta=10.0):
        if int(sr_in) != sr_in or int(sr_out) != sr_out or int(sr_in) < 1 or int(sr_out) < 1:
            raise ValueError(f"sample rates must be positive integers, got {sr_in!r} -> {sr_out!r}")
        if int(zeros) < 1 or not 0.0 < float(rolloff) <= 1.0 or float(beta) < 0.0:
            raise ValueError(f"need zeros >= 1, 0 < rolloff <= 1 and beta >= 0, got {zeros}, {rolloff}, {beta}")
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.zeros, self.rolloff, self.beta = int(zeros), float(rolloff), float(beta)
        g = math.gcd(self.sr_in, self.sr_out)
        self.L, self.M = self.sr_out // g, self.sr_in // g
        self.identity = self.L == self.M == 1
        self.scale = min(1.0, self.L / self.M)
        self.fc = self.rolloff * self.scale
        self.half = int(math.ceil(self.zeros / self.scale / self.rolloff))
        self.K = 2 * self.half
        self.carry = 2 * self.half                 # input samples a stream keeps per feed
        self.taps = None
        if self.identity:
            return
        if self.L * (self.K + 1) > MAX_TABLE_FLOATS:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz reduces to L/M = {self.L}/{self.M}: a table of {self.L} phases x "
                             f"{self.K} taps exceeds the {MAX_TABLE_FLOATS} floats that stay in LDS (rates with a large common "
                             f"divisor resample; convert such a feed to a standard rate first)")
        if ((TILE_OUT - 1) * self.M + self.L - 1) // self.L + self.K > MAX_TILE_SPAN:
            raise ValueError(f"{self.sr_in} -> {self.sr_out} Hz: a tile of {TILE_OUT} outputs would read more than {MAX_TILE_SPAN} "
                             f"input samples (input rates above about 7.5 x the output rate are not taken)")
        self.taps = design_taps(self.L, self.half, self.fc, self.beta).astype(np.float32)

    # ── index arithmetic (python ints: exact at any length) ──
    def n_out(self, n_in):
        """outputs of a clip of ``n_in`` samples: ceil(n_in * L / M)"""
        return -(-int(n_in) * self.L // self.M)

    def n_final(self, n_in):
        """outputs that are FINAL once ``n_in`` samples of a feed are there: output m is final when sample i_c + half has
        arrived, i.e. m*M // L <= n_in - 1 - half"""
        q = int(n_in) - self.half
        return 0 if q < 1 else (q * self.L - 1) // self.M + 1

    def n_final_array(self, n_in):
        """``n_final`` of an int64 array"""
        q = np.asarray(n_in, np.int64) - self.half
        return np.where(q < 1, 0, (np.maximum(q, 1) * self.L - 1) // self.M + 1)

    def n_out_array(self, n_in):
        return -(-np.asarray(n_in, np.int64) * self.L // self.M)


def design_taps(L, half, fc, beta):
    """h[p][k] = fc sinc(fc t) I0(beta sqrt(1 - (t/half)^2)) / I0(beta), t = p/L - (k - half + 1): float64 [L, 2*half]"""
    p = np.arange(L, dtype=np.float64)[:, None] / L
    k = np.arange(2 * half, dtype=np.float64)[None, :]
    t = p - (k - half + 1)
    w = np.i0(beta * np.sqrt(np.clip(1.0 - (t / half) ** 2, 0.0, None))) / np.i0(beta)
    return fc * np.sinc(fc * t) * w


@functools.lru_cache(maxsize=32)
def plan_for(sr_in, sr_out=SR):
    return ResamplePlan(sr_in, sr_out)


_COPY_TAPS = np.array([[1.0, 0.0]], np.float32)       # L = M = 1, half = 1: y[m] = 1 * x[m] + 0 * x[m + 1]


@functools.lru_cache(maxsize=64)
def _device_taps(sr_in, sr_out, device_index):
    """(taps on the device, L, M, half) of a plan; the identity plan converts and downmixes through a one-tap copy filter"""
    plan = plan_for(sr_in, sr_out)
    dev = torch.device("cuda", device_index)
    if plan.identity:
        return torch.from_numpy(_COPY_TAPS).to(dev), 1, 1, 1
    return torch.from_numpy(plan.taps).to(dev), plan.L, plan.M, plan.half


def build_rows(n_in, in_base, out_first, n_out, n_hist=None, hist_off=None, carry_dst=None):
    """sed_resample's host table [R][9] from int64 arrays: the clips' frames lie back to back in x, their outputs back to
    back in out with every clip on a 16-byte boundary -> (table, x frames, out samples)"""
    n_in = np.asarray(n_in, np.int64).reshape(-1)
    R = n_in.shape[0]
    col = lambda a, fill: np.full(R, fill, np.int64) if a is None else np.asarray(a, np.int64).reshape(-1)   # noqa: E731
    n_out = col(n_out, 0)
    padded = (n_out + 3) & ~3
    rows = np.stack([np.cumsum(n_in) - n_in, n_in, col(in_base, 0), col(out_first, 0), n_out, np.cumsum(padded) - padded,
                     col(hist_off, 0), col(n_hist, 0), col(carry_dst, -1)], 1)
    return np.ascontiguousarray(rows), int(n_in.sum()), int(padded.sum())


def with_channels(rows, channel):
    """a [R][9] table and the channel every row keeps (int64 [R]; -1 = downmix) -> sed_resample_select's table [R][10]"""
    rows = np.asarray(rows, np.int64).reshape(-1, ROW)
    return np.ascontiguousarray(np.concatenate([rows, np.asarray(channel, np.int64).reshape(-1, 1)], 1))


def build_keep_rows(n_in, n_out, channels):
    """sed_resample_select's table [R*channels][10] for R whole clips whose channels are kept: one row per (clip, channel), the
    rows of a clip all reading its frames, row ``r*channels + c`` keeping channel c; the planar outputs lie back to back,
    every one on a 16-byte boundary -> (table, x frames, out samples)"""
    nc = int(channels)
    n_in = np.asarray(n_in, np.int64).reshape(-1)
    rows, _, out_len = build_rows(np.repeat(n_in, nc), None, None, np.repeat(np.asarray(n_out, np.int64).reshape(-1), nc))
    rows[:, 0] = np.repeat(np.cumsum(n_in) - n_in, nc)
    return with_channels(rows, np.tile(np.arange(nc), n_in.shape[0])), int(n_in.sum()), out_len


def check_rows(rows, x_frames, hist_len, out_len, L, M, half, channels=None):
    """the library's host checks of a table (no GPU call); raises SedHipError with its message.  With ``channels`` the table
    is sed_resample_select's [R][10]."""
    if channels is not None:
        rows = np.ascontiguousarray(rows, np.int64).reshape(-1, ROW_SELECT)
        check(lib().sed_resample_select_check_table(C.c_void_p(rows.ctypes.data), rows.shape[0], int(channels), int(x_frames),
                                                    int(hist_len), int(out_len), int(L), int(M), int(half)),
              "sed_resample_select_check_table")
        return
    rows = np.ascontiguousarray(rows, np.int64).reshape(-1, ROW)
    check(lib().sed_resample_check_table(C.c_void_p(rows.ctypes.data), rows.shape[0], int(x_frames), int(hist_len), int(out_len),
                                         int(L), int(M), int(half)), "sed_resample_check_table")


def launch(x, fmt, channels, hist, taps, L, M, half, rows, out, ws=None):
    """one sed_resample launch on torch's current stream (sed_resample_select when the table is [R][10], ``with_channels``);
    ``ws`` (optional) is a reusable workspace"""
    rows = np.asarray(rows, np.int64)
    select = rows.ndim == 2 and rows.shape[1] == ROW_SELECT
    rows = np.ascontiguousarray(rows).reshape(-1, ROW_SELECT if select else ROW)
    R = rows.shape[0]
    name = "sed_resample_select" if select else "sed_resample"
    need = getattr(lib(), name + "_workspace_bytes")(R)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=out.device)
    check(getattr(lib(), name)(ptr(x), (x.numel() // channels) if x is not None else 0, fmt, channels, ptr(hist),
                               hist.numel() if hist is not None else 0, ptr(taps), taps.numel(), L, M, half,
                               C.c_void_p(rows.ctypes.data), R, ptr(out), out.numel(), ptr(ws), ws.numel(), stream_ptr()), name)
    return ws


# ───────────────────────── input handling ─────────────────────────
def as_pcm(w, channels, what="clip"):
    """one clip / piece as a tensor of int16 or float32, shape [N] (channels == 1) or [N, channels]"""
    w = w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w))
    channels = int(channels)
    if channels < 1 or channels > 64:
        raise ValueError(f"channels must be 1..64, got {channels}")
    if channels == 1 and w.dim() == 2 and w.shape[1] == 1:
        w = w[:, 0]
    if (w.dim() != 1) if channels == 1 else (w.dim() != 2 or w.shape[1] != channels):
        want = "[N]" if channels == 1 else f"[N, {channels}]"
        raise ValueError(f"{what}: expected a waveform of shape {want}, got {tuple(w.shape)}")
    if w.dtype == torch.int16:
        return w
    if not w.dtype.is_floating_point:
        raise ValueError(f"{what}: PCM must be int16 or floating point, got {w.dtype}")
    return w.to(torch.float32)


def is_plain(w, channels):
    """mono float PCM: what every entry point took before there was a resampler"""
    return int(channels) == 1 and not (isinstance(w, torch.Tensor) and w.dtype == torch.int16) and \
        not (isinstance(w, np.ndarray) and w.dtype == np.int16)


def pack_pcm(pieces, device):
    """pieces of one dtype ([N] or [N, C], host or device) -> one flat buffer on ``device``; host pieces travel in one copy"""
    flat = [p.reshape(-1) for p in pieces]
    if len(flat) == 1:
        return flat[0].to(device).contiguous()                          # a device clip is read where it lies
    if all(not p.is_cuda for p in flat):
        return torch.cat(flat).to(device).contiguous()
    return torch.cat([p.to(device) for p in flat]).contiguous()


def _rates(sr_in, R):
    if np.ndim(sr_in) == 0:
        return [int(sr_in)] * R
    rates = [int(r) for r in sr_in]
    if len(rates) != R:
        raise ValueError(f"sr_in: {len(rates)} rates for {R} clips")
    return rates


def resample_many(waves, sr_in, sr_out=SR, channels=1, device=None, keep_channels=False):
    """Every clip of a list (host or device; int16 or float; [N], or [N, channels] interleaved) resampled to ``sr_out`` mono
    float32 -> (one packed buffer on the device, clips [(first sample, n), ...]): what ``feature.mbe_packed`` takes, every clip
    on a 16-byte boundary.  ``sr_in``: one rate, or one per clip; clips of one (rate, sample format) share a launch.  Clip r
    is bit for bit ``resample(waves[r], sr_in[r])``; mono float clips already at ``sr_out`` are copied.
    ``keep_channels=True``: nothing is mixed; R recordings give ``R * channels`` planar clips, recording r, channel c = clip
    ``r * channels + c`` (what ``feature.mbe_planar`` takes), each bit for bit ``resample(waves[r][:, c], sr_in[r])``."""
    waves = list(waves)
    Ck = int(channels) if keep_channels else 1                          # clips per recording
    rates = _rates(sr_in, len(waves))
    if device is None:
        device = next((w.device for w in waves if isinstance(w, torch.Tensor) and w.is_cuda), None)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("sed_crnn_amd.resample needs a CUDA(HIP) device; there is no CPU fallback")
    pcs = [as_pcm(w, channels, f"clip {i}") for i, w in enumerate(waves)]
    plans = [plan_for(r, int(sr_out)) for r in rates]
    n_out = np.repeat(np.array([pl.n_out(p.shape[0]) for pl, p in zip(plans, pcs)], np.int64), Ck)
    padded = (n_out + 3) & ~3
    out_off = np.cumsum(padded) - padded
    out = torch.empty(int(padded.sum()), device=device)
    pad = np.concatenate([np.arange(o + n, o + q) for o, n, q in zip(out_off, n_out, padded)]) if len(waves) else np.zeros(0)
    if pad.size:                                                      # the padding between clips is zero, never garbage
        out[torch.from_numpy(pad.astype(np.int64)).to(device)] = 0.0
    clips = [(int(o), int(n)) for o, n in zip(out_off, n_out)]
    groups = {}
    for i, (pl, p) in enumerate(zip(plans, pcs)):
        if p.shape[0] == 0:
            continue
        if pl.identity and int(channels) == 1 and p.dtype == torch.float32:
            out[clips[i][0]:clips[i][0] + clips[i][1]] = p.to(device)      # the identity: the samples pass through untouched
            continue                                                       # (one channel: clip i is recording i either way)
        groups.setdefault((pl.sr_in, p.dtype == torch.int16), []).append(i)
    for (rate, is16), idx in groups.items():
        taps, L, M, half = _device_taps(rate, int(sr_out), device.index or 0)
        x = pack_pcm([pcs[i] for i in idx], device)
        if keep_channels:                                               # one row per (recording, channel), all reading the same frames
            rows, _, _ = build_keep_rows([pcs[i].shape[0] for i in idx], n_out[np.asarray(idx) * Ck], Ck)
            rows[:, 5] = out_off[(np.asarray(idx)[:, None] * Ck + np.arange(Ck)[None, :]).reshape(-1)]
        else:
            rows, _, _ = build_rows([pcs[i].shape[0] for i in idx], None, None, n_out[idx])
            rows[:, 5] = out_off[idx]
        launch(x, int(is16), int(channels), None, taps, L, M, half, rows, out)
    return out, clips


def resample(y, sr_in, sr_out=SR, channels=1, device=None, keep_channels=False):
    """One clip ([N], or [N, channels] interleaved; int16 or float; host or device) -> mono float32 [ceil(N*sr_out/sr_in)] on
    the device.  ``sr_in == sr_out`` with mono float input is the identity: no kernel runs, the samples come back bit for bit.
    ``keep_channels=True``: planar float32 ``[channels, n_out]`` instead of the downmix, row c bit for bit
    ``resample(y[:, c], sr_in)`` (at ``sr_in == sr_out`` the one-tap copy filter de-interleaves and converts)."""
    p = as_pcm(y, channels)
    if keep_channels:
        out, clips = resample_many([p], sr_in, sr_out, channels, device, keep_channels=True)
        n = clips[0][1]
        return out.as_strided((int(channels), n), ((n + 3) & ~3, 1))       # every channel starts on a 16-byte boundary
    if plan_for(int(sr_in), int(sr_out)).identity and int(channels) == 1 and p.dtype == torch.float32:
        if device is None:
            device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return p.to(device)
    out, clips = resample_many([p], sr_in, sr_out, channels, device)
    return out[:clips[0][1]]
