"""Localising live streams without a GPU: the three host functions of localize.py, the ring capacity against a brute
force over StreamSchedules (every event the rule accepts is emitted while its first sample is still in the ring, in any
chunking, and the capacity is no more than one step above what the worst case needs), StreamDetector's history_frames argument
and the host-only argument checks of sed_stream_ring_write and sed_event_tdoa_ring."""
import ctypes as C

import numpy as np
import pytest

NFFT = 2048


# ───────────── 1. the host functions ─────────────
def test_latency_and_ring_size_formulas():
    import sed_crnn_amd as sed
    from sed_crnn_amd.localize import stream_latency_frames, stream_ring_samples
    assert sed.stream_latency_frames is stream_latency_frames and sed.stream_ring_samples is stream_ring_samples
    assert stream_latency_frames(1, 256, 1, 0) == 257                       # (0 + 0 + 256 + 1) * 1
    assert stream_latency_frames(8, 256, 5, 3) == (3 + 2 + 32 + 1) * 8
    assert stream_latency_frames(4, 10, 3, 0) == (0 + 1 + 2 + 1) * 4        # seq_len // tf rounds down
    assert stream_ring_samples(100, 20, 1024) == 120 * 1024 + 2048
    assert stream_ring_samples(7, 3, 441) == (10 * 441 + 2048 + 3) // 4 * 4 == 6460
    assert all(stream_ring_samples(h, 5, 441) % 4 == 0 for h in range(1, 9))
    for bad in ((0, 256, 1, 0), (8, 4, 1, 0), (1, 256, 0, 0), (1, 256, 1, -1)):
        with pytest.raises(ValueError, match="stream_latency_frames"):
            stream_latency_frames(*bad)
    for bad in ((0, 5, 441), (5, 0, 441), (5, 5, 0)):
        with pytest.raises(ValueError, match="stream_ring_samples"):
            stream_ring_samples(*bad)


@pytest.mark.parametrize("event,tf,n_feat,max_frames,lat,hist,want", [
    ((10, 18, 12), 1, 1000, 8, 20, 28, True),                # f0 = 10: 18 + 20 - 10 = 28, equal to history_frames
    ((10, 18, 12), 1, 1000, 8, 20, 27, False),               # ... and one more than it
    ((10, 50, 30), 1, 1000, 8, 20, 44, True),                # longer than max_frames: f0 = 30 - 4 = 26, 50 + 20 - 26 = 44
    ((10, 50, 30), 1, 1000, 8, 20, 43, False),
    ((10, 50, 49), 1, 1000, 8, 20, 28, True),                # peak at the end: f0 = 42, as recent as a short event
    ((10, 50, 10), 1, 1000, 8, 20, 59, False),               # peak at the start: f0 = 10, 50 + 20 - 10 = 60
    ((10, 50, 10), 1, 1000, 8, 20, 60, True),
    ((2, 5, 3), 4, 1000, 256, 40, 52, True),                 # tf = 4: f0 = 8, 20 + 40 - 8 = 52
    ((2, 5, 3), 4, 1000, 256, 40, 51, False),
    ((60, 70, 65), 2, 100, 256, 0, 10 ** 6, False),          # no frames: never located
    ((-1, 3, 0), 2, 100, 256, 0, 10 ** 6, False),
])
def test_stream_locates_is_event_frames_plus_the_inequality(event, tf, n_feat, max_frames, lat, hist, want):
    from sed_crnn_amd.localize import event_frames, stream_locates
    a, b, pk = event
    f0, f1 = event_frames(a, b, pk, tf, n_feat, max_frames)
    assert stream_locates(a, b, pk, tf, n_feat, max_frames, lat, hist) is (f1 > f0 and b * tf + lat - f0 <= hist) is want


def test_stream_locates_against_event_frames_on_random_events():
    from sed_crnn_amd.localize import event_frames, stream_locates
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(2000):
        tf, mf = int(rng.choice([1, 4, 8])), int(rng.choice([1, 5, 8, 64]))
        a = int(rng.integers(-2, 200))
        b = a + int(rng.integers(0, 60))
        pk = int(rng.integers(a, max(a + 1, b)))
        n_feat, lat, hist = int(rng.integers(1, 2000)), int(rng.integers(0, 300)), int(rng.integers(1, 600))
        f0, f1 = event_frames(a, b, pk, tf, n_feat, mf)
        want = f1 > f0 and b * tf + lat - f0 <= hist
        assert stream_locates(a, b, pk, tf, n_feat, mf, lat, hist) == want
        seen.add(want)
    assert seen == {True, False}


# ───────────── 2. the ring capacity ─────────────
def _steps(tf, L, hop_win, median, max_new, h, chunks):
    """what StreamDetector's host arithmetic does with pushes of ``chunks`` samples: [(decided frames, samples received)] after
    every step, and the samples at the end"""
    from sed_crnn_amd.stream import StreamSchedules
    sc = StreamSchedules(tf, L, hop_win, 0, median, 1)
    per_round = (max_new * hop_win - 1) * h                                 # _push_mono: samples per round
    n = N = 0
    log = []
    for c in chunks:
        done = 0
        while done < c:
            take = min(per_round, c - done)
            done += take
            n += take
            upto = (n - NFFT // 2) // h + 1 if n >= NFFT // 2 else 0          # _logmel_round: frames that need no right padding
            if upto > N:
                sc.advance(np.array([upto - N], np.int64))
                N = upto
                assert int(sc.N[0]) == N
                log.append((int(sc.decided[0]), n))
    return log, n


def _chunkings(rng, total, per_round):
    yield [total]                                                           # one push: rounds of per_round samples
    yield [per_round] * (total // per_round) + [total % per_round]
    yield [1024] * (total // 1024) + [total % 1024]
    for _ in range(4):
        out, left = [], total
        while left:
            c = int(min(left, rng.choice([1, 7, 441, 1024, 5000, per_round, per_round + 1, 3 * per_round])))
            out.append(c)
            left -= c
        yield out


@pytest.mark.parametrize("h", [1024, 441])
@pytest.mark.parametrize("tf", [1, 8])
def test_ring_capacity_holds_for_every_located_event_and_is_tight_to_one_step(tf, h):
    """for hypothetical events that the rule accepts: the step that emits [a, b) of a class with min_gap g is the first with
    more than b + g decided frames (else the flush, with every sample received); then n - max(0, f0*h - n_fft/2), the samples
    from the event's first to the newest, must fit the ring.  Events ON the rule's boundary need at least the capacity less one
    step (and a frame): no smaller ring of this form would do."""
    from sed_crnn_amd.localize import event_frames, stream_latency_frames, stream_locates, stream_ring_samples
    rng = np.random.default_rng(tf * 1000 + h)
    L, hop_win, median, max_new, g_max, mf = 16 * tf, 8 * tf, 5, 2, 3, 16
    step_frames = max_new * hop_win
    lat = stream_latency_frames(tf, L, median, g_max)
    for hist in (mf + lat, mf + lat + 5 * tf):
        cap = stream_ring_samples(hist, step_frames, h)
        total = (hist + 12 * step_frames) * h + 333
        n_feat = 1 + total // h
        n_out = n_feat // tf
        worst, boundary = 0, []
        for chunks in _chunkings(rng, total, (step_frames - 1) * h):
            log, n_end = _steps(tf, L, hop_win, median, max_new, h, chunks)
            assert n_end == total
            decided = np.array([d for d, _ in log])
            events = []
            for _ in range(300):
                a = int(rng.integers(0, n_out))
                b = int(min(n_out, a + 1 + rng.integers(0, 3 * mf // tf + 6)))
                events.append((a, b, int(rng.integers(a, b)), int(rng.integers(0, g_max + 1))))
            for a in range(0, n_out - mf // tf, 3):                          # short events on the boundary of the minimum history
                b = a + (hist - lat) // tf
                if b <= n_out:
                    events.append((a, b, a, g_max))
            n_loc = 0
            for a, b, pk, g in events:
                if not stream_locates(a, b, pk, tf, n_feat, mf, lat, hist):
                    continue
                n_loc += 1
                f0, _ = event_frames(a, b, pk, tf, n_feat, mf)
                at = int(np.searchsorted(decided, b + g, side="right"))       # the first step with decided > b + g
                n = log[at][1] if at < len(log) else total
                need = n - max(0, f0 * h - NFFT // 2)
                assert need <= cap, (tf, h, hist, (a, b, pk, g), n, f0, need, cap)
                worst = max(worst, need)
                if g == g_max and b * tf + lat - f0 == hist and f0 * h >= NFFT // 2 and at < len(log):
                    boundary.append(need)
            assert n_loc > 50
        assert len(boundary) > 20
        print(f"tf={tf} h={h} history={hist}: cap {cap}, worst need {worst}, boundary events need {min(boundary)} .. {max(boundary)}")
        assert min(boundary) >= cap - (step_frames + 1) * h - 3 and worst > cap - step_frames * h


# ───────────── 3. the constructor ─────────────
def _net(cin=2):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def test_history_frames_argument():
    import sed_crnn_amd as sed
    from sed_crnn_amd.localize import stream_latency_frames, stream_ring_samples
    t = sed.TDOA(max_lag=12, max_frames=8)
    det = sed.EventDetector(_net(), median=3, min_gap=[2] + [0] * (_net().dense[-1] - 1), localize=t)
    with pytest.raises(NotImplementedError, match="live feeds"):
        det.stream(2)
    with pytest.raises(NotImplementedError, match="history_frames"):
        sed.StreamDetector(_net(), 2, localize=t)
    tf = det.model.time_factor
    lat = stream_latency_frames(tf, det.seq_len, 3, 2)
    assert lat == (2 + 1 + det.seq_len // tf + 1) * tf
    st = det.stream(2, history_frames="min", max_new_windows=1)
    assert (st.lat, st.history_frames) == (lat, 8 + lat)
    assert st.cap == stream_ring_samples(8 + lat, st.step_frames, det.hop_length) and st.cap % 4 == 0
    plain = sed.EventDetector(_net(), median=3, min_gap=[2] + [0] * (_net().dense[-1] - 1)).stream(2, max_new_windows=1)
    assert st.state_bytes == plain.state_bytes + 4 * 2 * 2 * st.cap and plain.cap == 0
    more = det.stream(3, history_frames=np.int64(8 + lat + 100))
    assert more.history_frames == 8 + lat + 100 and more.cap == stream_ring_samples(8 + lat + 100, more.step_frames, det.hop_length)
    assert det.stream(1, history_frames=8 + lat).history_frames == 8 + lat
    with pytest.raises(ValueError, match=f"minimum max_frames \\+ lat = 8 \\+ {lat} = {8 + lat}"):
        det.stream(2, history_frames=8 + lat - 1)
    for bad in ("max", 10.5, True):
        with pytest.raises(ValueError, match="history_frames must be"):
            det.stream(2, history_frames=bad)
    with pytest.raises(ValueError, match="no localize"):
        sed.EventDetector(_net()).stream(2, history_frames="min")
    with pytest.raises(ValueError, match="no localize"):
        sed.StreamDetector(_net(), 2, history_frames=300)
    # below the threshold a run can hold a pending event back without bound: no ring covers that
    with pytest.raises(ValueError, match="low == threshold"):
        sed.EventDetector(_net(), threshold=0.5, low=0.3, localize=t).stream(2, history_frames="min")
    # the defaults of the issue: about 1.9 MB per lane
    big = sed.EventDetector(_net(), localize=sed.TDOA()).stream(1, history_frames="min")
    assert big.cap == stream_ring_samples(256 + big.lat, 4 * big.det.hop, det.hop_length)
    print(f"defaults: lat {big.lat} frames, ring {big.cap} samples = {4 * big.cap / 1e6:.2f} MB per lane")


def test_stream_events_tdoa_without_lags():
    import sed_crnn_amd as sed
    with pytest.raises(ValueError, match="hold no lags"):
        sed.StreamEvents({"cls": None}, [0, 0], [0], 0.1).tdoa()


# ───────────── 4. the C entries on the host ─────────────
def _err(L):
    return L.sed_last_error_string().decode()


def test_ring_write_checks_its_table_on_the_host():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    assert L.sed_stream_ring_write_workspace_bytes(3) == 3 * 24
    assert L.sed_stream_ring_write_workspace_bytes(0) == 0 and L.sed_stream_ring_write_workspace_bytes(65536) == 0
    FAKE = C.c_void_p(0x1000)

    def call(table, lanes=2, cap=4096, ring=FAKE, ring_len=8192, src=FAKE, src_len=10000, ws=FAKE, ws_bytes=48):
        t = np.ascontiguousarray(np.asarray(table, dtype=np.int64))
        return L.sed_stream_ring_write(ring, ring_len, lanes, cap, src, src_len, C.c_void_p(t.ctypes.data), ws, ws_bytes, None)
    good = [(0, 100, 5000), (100, 100, 5000)]
    assert call(good, ring=None) != 0 and "null pointer" in _err(L)
    assert call(good, ws=None) != 0 and "null pointer" in _err(L)
    assert L.sed_stream_ring_write(FAKE, 8192, 2, 4096, FAKE, 10000, None, FAKE, 48, None) != 0 and "null pointer" in _err(L)
    assert call(good, cap=4098, ring_len=9000) != 0 and "multiple of 4" in _err(L)
    assert call(good, cap=0) != 0 and "bad sizes" in _err(L)
    assert call(good, ring_len=8191) != 0 and "bad sizes" in _err(L)
    assert call(good, lanes=0) != 0 and "bad sizes" in _err(L)
    assert call(good, ws_bytes=47) != 0 and "workspace" in _err(L)
    assert call([(0, 4097, 0), (0, 0, 0)]) != 0 and "the ring holds 4096" in _err(L)        # count > cap: an entry would be written twice
    assert call([(0, -1, 0), (0, 0, 0)]) != 0 and "new samples" in _err(L)
    assert call([(9950, 100, 0), (0, 0, 0)]) != 0 and "leave the buffer" in _err(L)
    assert call([(-1, 100, 0), (0, 0, 0)]) != 0 and "leave the buffer" in _err(L)
    assert call([(0, 100, -1), (0, 0, 0)]) != 0 and "first sample index" in _err(L)
    assert call(good, src=None, src_len=0) != 0 and "leave the buffer" in _err(L)
    assert call([(0, 10, 0), (0, 0, 0)], src=None) != 0 and "null buffer" in _err(L)
    assert call([(0, 0, 0), (0, 0, 77)], src=None, src_len=0) == 0                          # nothing new: nothing is launched


def test_event_tdoa_ring_checks_its_arguments_on_the_host():
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    assert L.sed_event_tdoa_ring_workspace_bytes(1, 2, 0, 8192, 1024, 256) == 16                  # n [1], to 16
    assert L.sed_event_tdoa_ring_workspace_bytes(3, 2, 3, 8192, 1024, 256) == 32 + 3 * 1 * 1 * row  # at most 9 frames: one chunk
    assert L.sed_event_tdoa_ring_workspace_bytes(2, 4, 10, 100 * 1024, 1024, 40) == 16 + 10 * 2 * 6 * row
    for bad in ((0, 2, 1, 8192, 1024, 8), (1, 1, 1, 8192, 1024, 8), (1, 9, 1, 8192, 1024, 8), (1, 2, -1, 8192, 1024, 8),
                (1, 2, 1, 2044, 1024, 8), (1, 2, 1, 8194, 1024, 8), (1, 2, 1, 8192, 0, 8), (1, 2, 1, 8192, 1024, 0)):
        assert L.sed_event_tdoa_ring_workspace_bytes(*bad) == 0, bad
    FAKE, blob = C.c_void_p(0x1000), (8 + 2048 + 2048 + 1028) * 4

    def call(n=(5000,), channels=2, ring=FAKE, ring_len=1 << 20, cap=8192, E=1, max_lag=24, max_frames=8, ws=1 << 20, rec=None, tf=1,
             hop=1024, lat=10, hist=20, tables=FAKE, onset=FAKE, wsp=FAKE):
        t = np.asarray(n, dtype=np.int64)
        return L.sed_event_tdoa_ring(ring, ring_len, cap, C.c_void_p(t.ctypes.data), len(n), channels, tables, blob, rec, onset, FAKE,
                                     FAKE, E, tf, hop, max_lag, max_frames, lat, hist, FAKE, FAKE, FAKE, None, wsp, ws, None)
    assert call(channels=1) != 0 and "channels" in _err(L)
    assert call(channels=9) != 0 and "channels" in _err(L)
    assert call(max_lag=0) != 0 and "max_lag" in _err(L)
    assert call(max_lag=128) != 0 and "max_lag" in _err(L)
    assert call(max_frames=0) != 0 and "max_frames" in _err(L)
    assert call(tf=0) != 0 and "bad sizes" in _err(L)
    assert call(lat=-1) != 0 and "lat_frames" in _err(L)
    assert call(hist=0) != 0 and "history_frames" in _err(L)
    assert call(ring=None) != 0 and "null pointer" in _err(L)
    assert call(tables=None) != 0 and "null pointer" in _err(L)
    assert L.sed_event_tdoa_ring(FAKE, 1 << 20, 8192, None, 1, 2, FAKE, blob, None, FAKE, FAKE, FAKE, 1, 1, 1024, 24, 8, 10, 20, FAKE,
                                 FAKE, FAKE, None, FAKE, 1 << 20, None) != 0 and "null pointer" in _err(L)
    assert call(cap=8194) != 0 and "multiple of 4" in _err(L)
    assert call(cap=2044) != 0 and "at least one frame" in _err(L)
    assert call(ring_len=2 * 8192 - 1) != 0 and "leave the buffer" in _err(L)
    assert call(ring=C.c_void_p(0x1004)) != 0 and "16-byte aligned" in _err(L)
    assert call(n=(-1,)) != 0 and "samples received" in _err(L)
    assert call(n=(5000, 6000)) != 0 and "need ev_rec" in _err(L)
    assert call(onset=None) != 0 and "null pointer" in _err(L)
    assert call(wsp=C.c_void_p(0x1008)) != 0 and "workspace must be 16-byte aligned" in _err(L)
    assert call(ws=16 + row - 16) != 0 and "workspace" in _err(L)
    assert call(E=0, ws=0, wsp=None) == 0                                   # no events: nothing is launched, nothing is needed
