"""What test_gpu_logmel_spectrum.py rests on, checked without a GPU (tests/logmel_spectrum_ref.py): the plans the host-side planner
gives the read-out banks and the waves per workgroup the launcher then picks, the frame layout against the reference's framing and
the kernel's fast-path condition, the float32 yardsticks and their floor, the 60 dB condition on the mel-level inputs — and the
rule itself on a complex64 restatement of the kernel's decomposition: it passes, and fails with one damaged pairing twiddle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_spectrum_ref as R  # noqa: E402


def _blob(fb, window="hann"):
    from sed_crnn_amd import feature
    return feature.build_tables(R.window(window), fb, "cpu").numpy().view(np.uint32)


# ───────────── plans ─────────────
@pytest.mark.parametrize("plan", ["two_band", "list"])
def test_readout_banks_cover_every_bin_and_get_the_plan_they_are_named_for(plan):
    banks = R.readout_banks(plan)
    assert len(banks) == 9
    seen = np.concatenate([bins[bins >= 0] for _, bins in banks])
    assert np.array_equal(np.sort(seen), np.arange(R.NB))                          # every bin once
    for fb, bins in banks:
        read = bins >= 0
        assert (fb[read].sum(1) == 1.0).all() and (np.count_nonzero(fb[read], axis=1) == 1).all()
        assert (fb[np.flatnonzero(read), bins[read]] == 1.0).all()
        blob = _blob(fb)
        assert blob[1] == fb.shape[0] and blob[5] == (1 if plan == "two_band" else 0)
        assert (~read).sum() == (0 if plan == "two_band" else 1)
        assert R.waves_per_workgroup(blob.shape[0]) == 12
    assert (banks[-1][1] == 1024).any()


def test_two_band_plans_store_nothing_after_bin_1024():
    """lane 31 walks bins 1023 .. 1055: its last stored sums end at bin 1024, and the entries of the 31 slots behind it carry zero
    weights and no store, so whatever lies in those slots reaches no band"""
    from sed_crnn_amd import feature
    banks = [fb for fb, _ in R.readout_banks("two_band")] + [feature.slaney_mel_basis(n_mels=40)]       # (64 and 128 Slaney bands get the list plan)
    for fb in banks:
        blob = _blob(fb)
        assert blob[5] == 1 and blob[2] == 33
        ent = blob[feature._LM_OFF_ENT:feature._LM_OFF_ENT + 33 * 32 * 4].reshape(33, 32, 4)      # [bin of the lane, lane, word]
        assert ent[1, 31, 2] < 0x80000000 or not fb[:, 1024].any()              # bin 1024 = lane 31's second: its sums are stored
        assert not ent[2:, 31, :2].any() and (ent[2:, 31, 2] == 0xFFFFFFFF).all()


def test_filler_banks_land_in_the_8_wave_and_4_wave_ranges_and_a_wide_scaler_leaves_2():
    bins = R.filler_bins()
    assert bins.shape == (64,) and np.unique(bins).shape == (64,) and set(R.MUST_BINS) <= set(bins.tolist())
    want = {8: (3904, 96, 248), 4: (8192, 255, 256)}
    for waves, width in R.FILLER_WIDTH.items():
        fb, b = R.filler_bank(width)
        assert np.array_equal(b, bins) and (fb[np.arange(64), bins] == 1.0).all() and (np.count_nonzero(fb[:64], axis=1) == 1).all()
        assert (np.count_nonzero(fb[64:], axis=1) == width).all() and fb[64:].min() >= 0.0
        nnz, above, up_to = want[waves]
        blob = _blob(fb)
        assert np.count_nonzero(fb) == nnz and blob[5] == 0 and above < blob[2] <= up_to, blob[:6]
        assert R.waves_per_workgroup(blob.shape[0]) == waves
    # the 8 192-non-zero blob beside the scaler of a scaled multichannel call: 4 waves up to 37 channels, 2 from 38, and 40 still fit
    words = blob.shape[0]
    assert R.waves_per_workgroup(words, 0) == 4 and R.waves_per_workgroup(words, 2 * 37 * 128 * 4) == 4
    assert R.waves_per_workgroup(words, 2 * 38 * 128 * 4) == 2 and R.waves_per_workgroup(words, 2 * 40 * 128 * 4) == 2
    assert words * 4 + 2 * 2 * (32 * 33 + 160) * 4 + 2 * 40 * 128 * 4 <= 160 * 1024


# ───────────── layout ─────────────
@pytest.mark.parametrize("hop", [R.HOP_FAST, R.HOP_GUARDED])
def test_layout_puts_each_stimulus_in_its_frame(hop):
    rng = np.random.default_rng(hop)
    for m in (1, 2, 7, 256):
        stim = rng.standard_normal((m, R.NFFT)).astype(np.float32)
        clip = R.lay_out(stim, hop)
        assert clip.shape[0] % 4 == 0
        frames = R.frames_of(clip, hop)
        assert frames.shape[0] == 1 + clip.shape[0] // hop >= R.LEAD + m + 2
        assert np.array_equal(frames[R.rows(m)], stim)                             # each stimulus alone in its frame
        assert not frames[:R.LEAD].any() and not frames[R.LEAD + m:].any()         # and nothing of it in any other
        fast = [R.takes_fast_path(f, hop, clip.shape[0]) for f in range(R.LEAD, R.LEAD + m)]
        assert all(fast) if hop == R.HOP_FAST else not any(fast)
    clip = R.lay_out(stim, R.HOP_FAST)
    assert not R.takes_fast_path(0, R.HOP_FAST, clip.shape[0]) and not R.takes_fast_path(1, R.HOP_FAST, clip.shape[0])
    assert not R.takes_fast_path(1 + clip.shape[0] // R.HOP_FAST - 1, R.HOP_FAST, clip.shape[0])


def test_stimuli_are_what_they_are_named():
    imp, ton = R.stimuli("impulses"), R.stimuli("tones")
    assert imp.shape == (2048, 2048) and imp.dtype == np.float32 and (imp.sum(1) == 1).all() and (imp.argmax(1) == np.arange(2048)).all()
    assert ton.shape == (1025, 2048) and ton.dtype == np.float32
    assert (ton[0] == ton[0, 0]).all() and np.array_equal(ton[1024, 0::2], -ton[1024, 1::2])      # DC, the alternating sequence
    a = R.family("tones", "rect").a64
    assert (a.argmax(1) == np.arange(1025)).all()                                  # bin-centred: frame k peaks at bin k
    for amp in ("1e-3", "1", "1e3"):
        x = R.stimuli("noise_" + amp)
        assert x.shape == (256, 2048) and abs(x.std() / float(amp) - 1.0) < 0.01
    assert (~R.family("impulses", "hann").live).sum() == 1 and not R.family("impulses", "hann").live[0]      # hann[0] = 0
    assert R.family("impulses", "rect").live.all()


# ───────────── yardstick, floor and the rule ─────────────
# measured with scipy's pocketfft in float32 (family maxima; they move by some per cent with the noise seed and with the vector
# width pocketfft is built for, so they are held to a factor 1.5)
YARDSTICKS = {("impulses", "rect"): 2.4e-7, ("impulses", "hann"): 7.4e-7, ("tones", "hann"): 2.4e-7, ("noise_1", "hann"): 3.7e-7,
              ("noise_1e-3", "hann"): 2.9e-7, ("noise_1e3", "rect"): 5.9e-7}


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_yardsticks_and_the_rule_on_a_float32_restatement_of_the_kernel(name, window):
    fam = R.family(name, window)
    assert R.FLOOR == 2.0 ** -23 and R.FACTOR == 8.0
    assert 2.0 ** -25 < fam.yard_raw < 1e-6 and fam.yard == max(fam.yard_raw, R.FLOOR)
    if (name, window) in YARDSTICKS:
        assert 1 / 1.5 < fam.yard_raw / YARDSTICKS[name, window] < 1.5, fam.yard_raw
    err = R.errors(R.emulate_log_power(fam.stim, fam.win), fam)
    print(f"{name} {window}: yardstick {fam.yard_raw:.2e}  emulation {err.max():.2e}  ratio {err.max() / fam.yard:.2f}")
    assert err.max() <= R.FACTOR * fam.yard
    # one pairing twiddle off by 1e-4 (bins 300 and 724): three orders above float32 rounding, far below the log-mel tests' 1e-3
    bad = R.errors(R.emulate_log_power(fam.stim, fam.win, wrong_pairing_twiddle=(300, 1e-4)), fam)
    assert bad.max() > R.FACTOR * fam.yard and bad[:, [300, 724]].max() == bad.max()
    rest = np.delete(bad, [300, 724], axis=1)
    assert rest.max() <= R.FACTOR * fam.yard


def test_errors_wants_minus_infinity_for_an_all_zero_frame():
    fam = R.family("impulses", "hann")
    log_power = R.emulate_log_power(fam.stim, fam.win)
    assert np.isneginf(log_power[0]).all()
    log_power[0, 5] = -80.0
    with pytest.raises(AssertionError, match="all-zero frame"):
        R.errors(log_power, fam)


# ───────────── mel level ─────────────
@pytest.mark.parametrize("n_mels", [40, 64, 128])
def test_mel_level_inputs_keep_every_band_within_60_db_of_the_strongest(n_mels):
    case = R.mel_case(n_mels)
    assert case.want.shape == (48, n_mels) and np.isfinite(case.want).all()
    spread = (case.want.max(1) - case.want.min(1)).max()
    print(f"n_mels={n_mels}: weakest band {10 * spread / np.log(10):.1f} dB below the strongest; yardstick {case.yard_raw:.2e}")
    assert spread <= R.SIXTY_DB
    assert case.want.max(1).max() - case.want.max(1).min() > 4 * np.log(10.0)      # the level does step: 60 dB over the clip
    assert 2.0 ** -24 < case.yard_raw < 1e-5 and case.yard == max(case.yard_raw, R.MEL_FLOOR)
