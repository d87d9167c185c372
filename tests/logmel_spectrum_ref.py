"""The power spectrum of the log-mel kernel, read out bin by bin: stimuli, frame layout, float64 reference, float32 yardstick.
TEST INFRASTRUCTURE shared by test_cpu_logmel_spectrum.py and test_gpu_logmel_spectrum.py.

The read-out.  ``feature.build_tables`` takes any window and any bank; a band with ONE weight of 1.0 at bin k makes the kernel
return ``L = log |X[k]|^2`` of the windowed frame, so ``A = exp(L / 2)`` is the magnitude of one bin.  1025 bins take nine banks
(``readout_banks``): with one-hot bands only the planner picks the two-band plan, with one extra band that shares bins with two
non-adjacent bands it picks the list plan.  ``filler_bank`` mixes 64 one-hot bands with 64 wide bands of random weights, whose
non-zero count decides how many waves per workgroup the launcher picks (``waves_per_workgroup`` restates its arithmetic).

The layout.  One stimulus per frame at hop 2048 (frames do not overlap) with constant padding.  The kernel takes a PAIR of
frames (2p, 2p + 1) through its unguarded loads only when the whole pair lies inside the clip, so stimulus j sits in frame
``LEAD + j`` with LEAD = 2 and two empty frames follow the last one: every stimulus frame is then on the fast path
(``takes_fast_path`` restates the kernel's condition).  The same stimuli at hop 2049 are all on the guarded path.

The rule.  Reference: ``|rfft|`` of float64(x) * float64(window).  Error of a bin: ``|A - A64| / peak`` with peak the frame's
largest reference magnitude.  Yardstick: the same frames through scipy's float32 rfft, float32 power, float32 log and the same
read-out, its error maximised over the WHOLE family (per frame it is degenerate: pocketfft is nearly exact on tones and impulses)
and floored at 2^-23, one float32 ulp of the peak after the log / exp read-out.  Bound: FACTOR = 8 times that, the convention of
test_gpu_spatial.py.  A frame whose windowed samples are all zero must give -inf in every band and is left out of the statistics.
"""
import collections
import functools

import numpy as np
import scipy.fft

NFFT, NB = 2048, 1025
HOP_FAST, HOP_GUARDED = 2048, 2049
LEAD = 2                                            # stimulus j sits in frame LEAD + j
FLOOR = 2.0 ** -23
FACTOR = 8.0
WINDOWS = ("rect", "hann")
FAMILIES = ("impulses", "tones", "noise_1e-3", "noise_1", "noise_1e3")
MUST_BINS = (0, 1, 31, 32, 33, 511, 512, 513, 991, 992, 1023, 1024)
SPECIAL_BINS = (0, 512, 1024)                       # lane 0's self-paired branch (0, 1024) and the single-lane line (512)
SIXTY_DB = 6.0 * np.log(10.0)                       # 60 dB of power, in nepers of the natural log


def window(name):
    from sed_crnn_amd import feature
    return np.ones(NFFT, np.float32) if name == "rect" else feature.hann_periodic(NFFT)


# ───────────── stimuli: [M, 2048] float32, one frame each ─────────────
def impulses():
    return np.eye(NFFT, dtype=np.float32)


def tones(seed=20261021):
    """frame k = 0.5 cos(2 pi k n / 2048 + phi_k), k = 0 .. 1024 (DC .. the alternating sequence), seeded phases"""
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, NB)
    kn = (np.arange(NB)[:, None] * np.arange(NFFT)[None, :]) % NFFT
    return (0.5 * np.cos(2.0 * np.pi * kn / NFFT + phi[:, None])).astype(np.float32)


def noise(amplitude, frames=256, seed=7):
    return (amplitude * np.random.default_rng(seed).standard_normal((frames, NFFT))).astype(np.float32)


def stimuli(family):
    if family == "impulses":
        return impulses()
    if family == "tones":
        return tones()
    return noise(float(family.split("_")[1]))


# ───────────── layout ─────────────
def lay_out(stim, hop):
    """the clip whose frame LEAD + j (centre padding: it starts at sample hop (LEAD + j) - 1024) holds stim[j] and whose other
    samples are zero; two more whole frames follow the last stimulus and the length is a multiple of 4"""
    m = stim.shape[0]
    n = hop * (m + LEAD + 2) + NFFT // 2
    clip = np.zeros(n + (-n) % 4, np.float32)
    at = hop * (np.arange(m) + LEAD) - NFFT // 2
    clip[at[:, None] + np.arange(NFFT)[None, :]] = stim
    return clip


def rows(m):
    return slice(LEAD, LEAD + m)


def frames_of(clip, hop):
    """the reference's framing: centre = True with constant padding, 1 + n // hop frames of 2048 samples"""
    padded = np.pad(np.asarray(clip, np.float32), NFFT // 2)
    count = 1 + clip.shape[0] // hop
    return padded[hop * np.arange(count)[:, None] + np.arange(NFFT)[None, :]]


def takes_fast_path(frame, hop, n_samples):
    """logmel_fft_k's fast_ok for the pair that holds ``frame`` (a clip that starts on an 8-byte boundary)"""
    pair = frame // 2
    first = pair * 2 * hop - NFFT // 2
    return hop % 2 == 0 and first >= 0 and first + hop + NFFT <= n_samples and pair * 2 + 1 < 1 + n_samples // hop


# ───────────── reference and yardstick ─────────────
def spectrum64(frames, win):
    return np.abs(np.fft.rfft(frames.astype(np.float64) * win.astype(np.float64), axis=1))


def power32(frames, win):
    spec = scipy.fft.rfft(frames.astype(np.float32) * win.astype(np.float32), axis=1)
    assert spec.dtype == np.complex64, spec.dtype
    return spec.real * spec.real + spec.imag * spec.imag


def log32(power):
    assert power.dtype == np.float32
    with np.errstate(divide="ignore"):
        return np.log(power)


def amplitude(log_power):
    """A = exp(L / 2) in float64 from a float32 L (-inf -> 0)"""
    return np.exp(0.5 * np.asarray(log_power).astype(np.float64))


Family = collections.namedtuple("Family", "name window_name stim win a64 peak live yard_raw yard")


def family_of(name, window_name, stim):
    """a Family of any frames [M, 2048] float32 (see ``family``)"""
    win = window(window_name)
    a64 = spectrum64(stim, win)
    peak = a64.max(1)
    live = (stim * win != 0).any(1)
    assert ((peak > 0) == live).all()
    safe = np.where(live, peak, 1.0)[:, None]
    yard_raw = float((np.abs(amplitude(log32(power32(stim, win))) - a64) / safe)[live].max())
    for a in (stim, win, a64, peak, live):
        a.setflags(write=False)
    return Family(name, window_name, stim, win, a64, peak, live, yard_raw, max(yard_raw, FLOOR))


@functools.lru_cache(maxsize=None)
def family(name, window_name):
    """stimuli, float64 magnitudes [M, 1025], frame peaks, which frames are not all zero, and the family's yardstick (as measured
    and floored); computed once and shared, read-only"""
    return family_of(name, window_name, stimuli(name))


def errors(log_power, fam, bins=None):
    """|A - A64| / peak of the live frames, [live frames, bins], from log power [M, len(bins)] read out at ``bins`` (default: all
    1025); asserts -inf in every band of an all-zero frame and finite-or-minus-infinity values elsewhere"""
    bins = np.arange(NB) if bins is None else np.asarray(bins)
    log_power = np.asarray(log_power)
    assert log_power.shape == (fam.a64.shape[0], bins.shape[0]), log_power.shape
    assert np.isneginf(log_power[~fam.live]).all(), "an all-zero frame must give -inf in every band"
    got = log_power[fam.live]
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    return np.abs(amplitude(got) - fam.a64[fam.live][:, bins]) / fam.peak[fam.live][:, None]


# ───────────── banks ─────────────
def readout_banks(plan):
    """nine (bank [n_mels, 1025], bins [n_mels]) that read out all 1025 bins between them; bins[m] = -1 marks the one band of a
    "list" bank that is no read-out: it holds the bins of bands 0 and 2, which no two-band plan can express"""
    banks = []
    if plan == "two_band":
        groups = [np.arange(128 * i, 128 * i + 128) for i in range(8)] + [np.array([1024])]
    else:
        groups = [np.arange(127 * i, 127 * i + 127) for i in range(8)] + [np.arange(1016, 1025)]
    for bins in groups:
        extra = plan != "two_band"
        fb = np.zeros((bins.shape[0] + extra, NB), np.float32)
        fb[np.arange(bins.shape[0]), bins] = 1.0
        if extra:
            fb[-1, bins[0]] = fb[-1, bins[2]] = 1.0
            bins = np.concatenate([bins, [-1]])
        banks.append((fb, bins))
    return banks


def filler_bins():
    """the 64 bins the filler banks read out: MUST_BINS and a spread of others"""
    bins = list(MUST_BINS)
    i = 0
    while len(bins) < 64:
        k = (37 * i + 5) % NB
        if k not in bins:
            bins.append(k)
        i += 1
    return np.array(sorted(bins))


def filler_bank(width, seed=11):
    """128 bands: 64 one-hot read-outs at filler_bins(), then 64 bands of ``width`` adjacent bins with weights in [0.1, 1.1) spread
    over the spectrum (neighbours overlap: a list plan of 64 + 64 width non-zeros) -> (bank, bins)"""
    rng = np.random.default_rng(seed + width)
    bins = filler_bins()
    fb = np.zeros((128, NB), np.float32)
    fb[np.arange(64), bins] = 1.0
    for j in range(64):
        at = j * (NB - width) // 63
        fb[64 + j, at:at + width] = rng.random(width).astype(np.float32) + np.float32(0.1)
    return fb, bins


FILLER_WIDTH = {8: 60, 4: 127}                      # waves per workgroup -> filler width (3 904 and 8 192 non-zeros)


def band_reference(a64, fb):
    """sqrt of the band energies of float64 magnitudes [M, 1025] under a bank, float64"""
    return np.sqrt((a64 * a64) @ fb.astype(np.float64).T)


def band_log32(frames, win, fb):
    """the float32 evaluation of log band energies: scipy's float32 rfft, float32 power, float32 bank product, float32 log"""
    return log32(power32(frames, win) @ fb.astype(np.float32).T)


def band_errors(log_bands, fam, fb):
    """``errors`` for the bands of any bank: |A - A64| / peak of the live frames with A64 = band_reference and peak the frame's
    largest reference magnitude among THESE bands (wide bands are not measured against a single bin, nor single bins against them)"""
    want = band_reference(fam.a64, fb)[fam.live]
    log_bands = np.asarray(log_bands)
    assert log_bands.shape == (fam.a64.shape[0], fb.shape[0]), log_bands.shape
    assert np.isneginf(log_bands[~fam.live]).all(), "an all-zero frame must give -inf in every band"
    got = log_bands[fam.live]
    assert not np.isnan(got).any() and not np.isposinf(got).any()
    return np.abs(amplitude(got) - want) / want.max(1)[:, None]


def band_yardstick(fam, fb):
    """the family maximum of band_errors of the float32 evaluation, as measured and floored"""
    raw = float(band_errors(band_log32(fam.stim, fam.win, fb), fam, fb).max())
    return raw, max(raw, FLOOR)


def scale32(log_values, mean32, inv32):
    """the fused scaler as the kernel applies it: (v - mean) * (1 / sigma), every step rounded to float32"""
    assert log_values.dtype == mean32.dtype == inv32.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (log_values - mean32) * inv32


def unscale(values, mean32, inv32):
    """scaled float32 values back to log power, in float64 (exact to 1e-16: it adds nothing to what is measured)"""
    return np.asarray(values).astype(np.float64) / inv32.astype(np.float64) + mean32.astype(np.float64)


def waves_per_workgroup(blob_words, scaler_bytes=2 * 128 * 4):
    """launch_logmel_any's choice: the most of 12, 8, 4, 2 waves whose exchange scratch fits the 160 KiB LDS beside the blob and the
    scaler (2 * 128 floats for the single-clip and packed entries, 2 C n_mels floats for a scaled multichannel call, else 0)"""
    per_wave = 2 * (32 * 33 + 32 + 128) * 4
    room = 160 * 1024 - scaler_bytes
    return next((w for w in (12, 8, 4) if blob_words * 4 + w * per_wave <= room), 2)


# ───────────── the kernel's decomposition in complex64 (stands in for a correct kernel where there is no GPU) ─────────────
def emulate_log_power(frames, win, wrong_pairing_twiddle=None):
    """log |X[k]|^2, k = 0 .. 1024, the way logmel_fft_k computes it, in float32 / complex64: z[n] = x[2n] + i x[2n+1], a 1024-point
    transform as 32 x 32 with W_1024 twiddles between the passes, the pairing pass with W_2048, power, float32 log.
    ``wrong_pairing_twiddle`` = (k, delta) adds delta to the real part of the pairing twiddle that bins k and 1024 - k share
    (what a damaged table entry would do)"""
    f32, c64 = np.float32, np.complex64
    x = frames.astype(f32) * win.astype(f32)
    z = (x[:, 0::2] + 1j * x[:, 1::2]).astype(c64).reshape(-1, 32, 32)              # [frame, n1, r]: z[32 n1 + r]
    a = scipy.fft.fft(z, axis=1)                                                    # [frame, k1, r]
    assert a.dtype == c64
    k1r = (np.arange(32)[:, None] * np.arange(32)[None, :]) % 1024
    a = a * np.exp(-2j * np.pi * k1r / 1024.0).astype(c64)
    big = scipy.fft.fft(a, axis=2).transpose(0, 2, 1).reshape(-1, 1024)             # Z[k1 + 32 k2]
    assert big.dtype == c64
    k = np.arange(NB)
    zk, zm = big[:, k % 1024], np.conj(big[:, (1024 - k) % 1024])
    e, q = zk + zm, (-1j * (zk - zm)).astype(c64)
    pw = np.exp(-2j * np.pi * k / 2048.0).astype(c64)
    if wrong_pairing_twiddle is not None:
        at, delta = wrong_pairing_twiddle
        pw[at] += f32(delta)
        pw[1024 - at] = -np.conj(pw[at])                                            # W^(1024-k) = -conj W^k: one table entry, two bins
    four_x = e + q * pw
    power = f32(0.25) * (four_x.real * four_x.real + four_x.imag * four_x.imag)
    return log32(power.astype(f32))


# ───────────── mel level ─────────────
MelCase = collections.namedtuple("MelCase", "y fb want yard_raw yard")
MEL_FLOOR = 2.0 ** -22                              # FLOOR in the log domain: dL = 2 dA / A


@functools.lru_cache(maxsize=None)
def mel_case(n_mels, frames=48, seed=3):
    """broadband noise whose level steps by 20 dB every 12 frames, librosa's Slaney bank of ``n_mels`` bands under the periodic Hann
    window at hop 1024 -> the clip, the bank, float64 log band energies [frames, n_mels] and the float32 yardstick (family maximum
    of the log-domain error, as measured and floored)"""
    from sed_crnn_amd import feature
    rng = np.random.default_rng(seed + n_mels)
    n = 1024 * (frames - 1) + 517
    gain = 10.0 ** (-(np.arange(n) // (12 * 1024)).astype(np.float64))
    y = (0.3 * gain * rng.standard_normal(n)).astype(np.float32)
    fb = feature.slaney_mel_basis(n_mels=n_mels)
    fr, win = frames_of(y, 1024), window("hann")
    want = np.log((spectrum64(fr, win) ** 2) @ fb.astype(np.float64).T)
    yard_raw = float(np.abs(band_log32(fr, win, fb).astype(np.float64) - want).max())
    for a in (y, fb, want):
        a.setflags(write=False)
    return MelCase(y, fb, want, yard_raw, max(yard_raw, MEL_FLOOR))
