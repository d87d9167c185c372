"""The resampler's design and host planning without a GPU (sed_crnn_amd/resample.py, csrc/resample.hip's host checks): the
product's table against the numpy restatement of tests/resample_ref.py, the design itself against analytic signals and
scipy's polyphase resampler, the index arithmetic, the streaming finality rule and the table validator."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402

RATES = (8000, 11025, 16000, 22050, 32000, 48000, 88200, 96000)
#        sr_in: (L, M, half)
PLANS = {8000: (441, 80, 27), 11025: (4, 1, 27), 16000: (441, 160, 27), 22050: (2, 1, 27), 32000: (441, 320, 27),
         48000: (147, 160, 29), 88200: (1, 2, 53), 96000: (147, 320, 57)}


def test_product_table_is_the_reference_table_rounded_to_float32():
    from sed_crnn_amd.resample import ResamplePlan
    for sr in RATES:
        plan = ResamplePlan(sr)
        L, M, half, h = ref.design(sr)
        assert (plan.L, plan.M, plan.half, plan.K) == (L, M, half, 2 * half) == PLANS[sr] + (2 * PLANS[sr][2],)
        assert plan.taps.dtype == np.float32 and plan.taps.shape == (L, 2 * half)
        assert np.array_equal(plan.taps.view(np.int32), h.astype(np.float32).view(np.int32)), sr
        assert plan.carry == 2 * half
    assert ResamplePlan(48000).taps.size == 147 * 58 and ResamplePlan(16000).taps.size == 441 * 54 == 23_814


@pytest.mark.parametrize("sr", [48000, 16000])
def test_design_reproduces_analytic_sines_and_unit_dc_gain(sr):
    N = sr // 5
    for f in (1000.0, 0.2 * min(sr, 44100)):
        x = np.sin(2 * np.pi * f * np.arange(N) / sr)
        y = ref.resample64(x, sr)
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / 44100)
        err = np.abs(y - want)[2000:-2000].max()
        print(f"{sr} Hz, {f:.0f} Hz sine: float64 reference error {err:.2e}")
        assert len(y) == -(-N * 44100 // sr) and err <= 1e-5
    dc = ref.resample64(np.ones(N), sr)
    assert np.abs(dc[2000:-2000] - 1.0).max() <= 1e-5
    # the float32 variant (rounded table, fp32 sums) stays within float32 rounding of it
    x = np.sin(2 * np.pi * 1000.0 * np.arange(N) / sr)
    assert np.abs(ref.resample32(x, sr) - ref.resample64(x.astype(np.float32), sr)).max() <= 2e-6


def test_design_suppresses_a_tone_above_the_output_nyquist():
    x = np.sin(2 * np.pi * 30000 * np.arange(96000 // 5) / 96000)
    y = ref.resample64(x, 96000)
    assert np.abs(y[2000:-2000]).max() <= 1e-5


@pytest.mark.parametrize("sr", [48000, 16000, 96000, 22050])
def test_reference_indexing_agrees_with_scipy_resample_poly(sr):
    """an independent check of the polyphase indexing: scipy upsamples by L, filters with ONE FIR and keeps every M-th sample"""
    from scipy.signal import resample_poly
    L, M, half, g = ref.prototype_fir(sr)
    rng = np.random.default_rng(sr)
    x = rng.standard_normal(4000)
    got = ref.resample64(x, sr)
    want = resample_poly(x, L, M, window=g / L)            # scipy scales its window by `up`
    n = min(len(got), len(want))
    assert abs(len(got) - len(want)) <= 1
    edge = 2 * half * L // M + 2
    assert np.abs(got[:n] - want[:n])[edge:-edge].max() <= 1e-12


def test_output_counts_and_identity_and_refusals():
    from sed_crnn_amd.resample import MAX_TABLE_FLOATS, ResamplePlan
    for sr in RATES:
        plan = ResamplePlan(sr)
        L, M = plan.L, plan.M
        for N in (1, M - 1, M, M + 1, 10 * M + 3):
            if N < 1:
                continue
            assert plan.n_out(N) == -(-N * L // M) == int(np.ceil(N * L / M)) == len(ref.resample64(np.zeros(N), sr))
        assert plan.n_out(0) == 0 and plan.n_out(2 ** 40) == -(-(2 ** 40) * L // M)
    ident = ResamplePlan(44100)
    assert ident.identity and ident.taps is None and (ident.L, ident.M) == (1, 1) and ident.n_out(12345) == 12345
    with pytest.raises(ValueError, match="exceeds"):
        ResamplePlan(44101)                                 # L = 44 100 phases
    assert 441 * 55 <= MAX_TABLE_FLOATS < 44100 * 49
    with pytest.raises(ValueError, match="input rates above"):
        ResamplePlan(352_800)                             # L/M = 1/8: a tile would read 8 602 samples
    with pytest.raises(ValueError):
        ResamplePlan(0)
    with pytest.raises(ValueError):
        ResamplePlan(48000.5)


@pytest.mark.parametrize("sr", [48000, 16000, 96000])
def test_streaming_finality_partitions_the_outputs_exactly_once(sr):
    """output m is final once sample i_c + half is there; over any chunking, what the pushes declare final plus the flush
    remainder is [0, ceil(N L / M)) exactly once, in order, and the carry of 2*half samples always covers the next output"""
    from sed_crnn_amd.resample import ResamplePlan
    plan = ResamplePlan(sr)
    rng = np.random.default_rng(sr + 1)
    for trial in range(40):
        N = int(rng.integers(1, 5000))
        n, done, got = 0, 0, []
        while n < N:
            n = min(N, n + int(rng.choice([1, 2, plan.M - 1, plan.M, 97, 997, 4000])))
            f = plan.n_final(n)
            assert f == int(plan.n_final_array(np.array([n]))[0]) and done <= f <= plan.n_out(n)
            for m in range(done, f):                        # final: its last tap has arrived; and it was not final before
                assert m * plan.M // plan.L + plan.half <= n - 1
            if f < plan.n_out(n):
                assert f * plan.M // plan.L + plan.half > n - 1
                assert f * plan.M // plan.L - plan.half + 1 >= n - plan.carry       # the carry holds its first tap
            got.append((done, f))
            done = f
        got.append((done, plan.n_out(N)))
        flat = [m for a, b in got for m in range(a, b)]
        assert flat == list(range(plan.n_out(N)))


def _rows(*rows):
    return np.ascontiguousarray(np.array(rows, np.int64).reshape(-1, 9))


def test_table_validator_and_argument_checks():
    from sed_crnn_amd import _lib
    from sed_crnn_amd.resample import ResamplePlan, build_rows, check_rows
    L = _lib.lib()
    assert L.sed_resample_workspace_bytes(0) == 0 and L.sed_resample_workspace_bytes(-3) == 0
    assert L.sed_resample_workspace_bytes(5) == 5 * 80
    plan = ResamplePlan(48000)
    a = (plan.L, plan.M, plan.half)
    rows, x_frames, out_len = build_rows([1000, 1, 77], None, None, [plan.n_out(1000), plan.n_out(1), plan.n_out(77)])
    assert x_frames == 1078 and out_len % 4 == 0 and (rows[:, 5] % 4 == 0).all()
    check_rows(rows, x_frames, 0, out_len, *a)
    #          in_off n_in base m0  n_out out_off hist_off n_hist carry
    good = [0, 100, 0, 0, 92, 0, 0, 0, -1]

    def bad(row, x_frames=100, hist_len=0, out_len=92, plan_args=a):
        with pytest.raises(_lib.SedHipError):
            check_rows(_rows(row), x_frames, hist_len, out_len, *plan_args)
    check_rows(_rows(good), 100, 0, 92, *a)
    bad([1, 100, 0, 0, 92, 0, 0, 0, -1])                    # the clip leaves the buffer
    bad([-1, 10, 0, 0, 0, 0, 0, 0, -1])
    bad([0, -5, 0, 0, 0, 0, 0, 0, -1])                      # negative counts
    bad([0, 100, 0, 0, -1, 0, 0, 0, -1])
    bad([0, 100, -1, 0, 92, 0, 0, 0, -1])
    bad([0, 100, 0, -1, 92, 0, 0, 0, -1])
    bad([0, 100, 0, 0, 93, 0, 0, 0, -1])                    # more outputs than the buffer holds
    bad([0, 100, 0, 0, 80, 2, 0, 0, -1])                    # not on a 16-byte boundary
    bad([0, 100, 0, 0, 92, 0, 0, 5, -1])                    # history it does not have
    bad([0, 100, 500, 0, 92, 0, 0, 5, -1], hist_len=5)      # history that does not reach the first tap (sample 0 - half + 1 .. is before it)
    bad(good, plan_args=(44100, 44101, 27))                 # a plan whose table does not fit
    bad(good, plan_args=(1, 9, 240))                        # a tile that reads too much
    bad(good, plan_args=(0, 1, 1))
    with pytest.raises(_lib.SedHipError):                   # two clips whose outputs overlap
        check_rows(_rows(good, [0, 100, 0, 0, 92, 0, 0, 0, -1]), 100, 0, 92, *a)
    # a stream step: history = the carry, the next carry goes to the other half
    CR = plan.carry
    step = [0, 480, 96_000, plan.n_final(96_000), plan.n_final(96_480) - plan.n_final(96_000), 0, 0, CR, CR]
    check_rows(_rows(step), 480, 2 * CR, 444, *a)
    bad(step[:8] + [CR - 1], x_frames=480, hist_len=2 * CR, out_len=444)        # the carry would overwrite its source
    bad(step[:8] + [CR + 1], x_frames=480, hist_len=2 * CR, out_len=444)        # the carry leaves the buffer
    bad(step[:3] + [step[3] - 3] + step[4:], x_frames=480, hist_len=2 * CR, out_len=444)   # an output older than the carry
    # the launch itself refuses the same things before it touches a GPU
    FAKE = C.c_void_p(0x1000)
    r = _rows([1, 100, 0, 0, 92, 0, 0, 0, -1])
    args = lambda fmt=0, ch=1, taps_len=plan.taps.size, ws=80: (FAKE, 100, fmt, ch, None, 0, FAKE, taps_len, *a,   # noqa: E731
                                                                C.c_void_p(r.ctypes.data), 1, FAKE, 92, FAKE, ws, None)
    assert L.sed_resample(*args()) != 0 and b"not inside the input buffer" in L.sed_last_error_string()
    r[0, 0] = 0
    assert L.sed_resample(*args(fmt=2)) != 0 and b"format" in L.sed_last_error_string()
    assert L.sed_resample(*args(ch=0)) != 0 and b"channels" in L.sed_last_error_string()
    assert L.sed_resample(*args(taps_len=7)) != 0 and b"tap table" in L.sed_last_error_string()
    assert L.sed_resample(*args(ws=8)) != 0 and b"workspace" in L.sed_last_error_string()


def test_python_surface_refuses_bad_input_without_a_gpu():
    import torch
    from sed_crnn_amd.resample import as_pcm, is_plain
    assert as_pcm(np.zeros(5, np.int16), 1).dtype == torch.int16
    assert as_pcm(np.zeros((5, 2), np.float64), 2).dtype == torch.float32
    assert as_pcm(np.zeros((5, 1), np.float32), 1).shape == (5,)
    for w, ch in ((np.zeros((5, 2), np.float32), 1), (np.zeros(5, np.float32), 2), (np.zeros((5, 3), np.int16), 2)):
        with pytest.raises(ValueError, match="expected a waveform"):
            as_pcm(w, ch)
    with pytest.raises(ValueError, match="int16 or floating"):
        as_pcm(np.zeros(5, np.int32), 1)
    assert is_plain(np.zeros(4, np.float32), 1) and not is_plain(np.zeros(4, np.int16), 1) and not is_plain(np.zeros((4, 2)), 2)
