"""Contrast SRP-PHAT, the host side: the settings, the C entries' signatures, argument checks and workspace sizes, the
build guard, what the stream, the ring entry and the Python entries refuse, the selection rule as the float64 reference
(tests/contrast_ref.py) applies it to a hand-made table, and the scene the feature was made for: an event that sounds over a
louder source of another class.  No GPU.

Measured with the reference (6 cm tetrahedron at 44.1 kHz, ring of 72 directions, oversample 8, hop 1024, target in frames
[24, 36), a white far-field interferer through the whole recording, Contrast(frames=16, search=64, guard=2, min_frames=8); six
pairs of directions 70 to 160 degrees apart):
    +10 dB   plain dir 1 .. 2 degrees from the interferer, contrasted dir 1 .. 3 degrees from the target, doa_power 0.076 .. 0.115
    +30 dB   plain dir 1 .. 2 degrees from the interferer, contrasted dir 1 .. 3 degrees from the target, doa_power 0.002 .. 0.003
    alone    the two dir are equal, 1 .. 2 degrees from the target
MVDR() of the reference on the event's samples of the first +10 dB scene (input SIR -10.1 dB): output SIR -8.2 dB steered at the
plain dir, +8.0 dB steered at the contrasted dir."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contrast_ref as cr  # noqa: E402
import doa_ref  # noqa: E402
import mvdr_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sed_event_contrast_frames", "sed_event_doa_contrast", "sed_event_doa_track_contrast")
KERNELS = ("contrast_select_k", "contrast_accum_k")
ROW = 1026 * 8


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


# ───────────── 1. the settings ─────────────
def test_contrast_validates_its_settings(sed):
    c = sed.Contrast()
    assert (c.frames, c.search, c.guard, c.min_frames, c.weight) == (32, 256, 2, 8, 1.0)
    assert c == sed.Contrast(32, 256, 2, 8, 1.0) and hash(c) == hash(sed.Contrast(weight=1)) and c != sed.Contrast(weight=0.5)
    n = sed.Contrast(frames=np.int64(1), search=np.int32(1), guard=np.int64(0), min_frames=np.int32(1), weight=np.float32(4.0))
    assert all(type(getattr(n, k)) is int for k in ("frames", "search", "guard", "min_frames")) and type(n.weight) is float and n.weight == 4.0
    assert sed.Contrast(256, 4096, 64, 256).search == 4096
    with pytest.raises(Exception):
        c.frames = 8                                                         # frozen
    for bad in (dict(frames=0), dict(frames=257, search=300), dict(frames=True), dict(frames=8.0), dict(search=31), dict(search=4097),
                dict(search=None), dict(guard=-1), dict(guard=65), dict(guard="2"), dict(min_frames=0), dict(min_frames=33),
                dict(frames=4, search=8, min_frames=5), dict(weight=0.0), dict(weight=-1.0), dict(weight=4.5), dict(weight=float("nan")),
                dict(weight=float("inf")), dict(weight=True), dict(weight="1"), dict(weight=None)):
        with pytest.raises(ValueError, match="Contrast: "):
            sed.Contrast(**bad)


def test_doa_takes_contrast_as_its_last_keyword(sed):
    import inspect
    pos, grid = doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(8)
    assert list(inspect.signature(sed.DOA.__init__).parameters)[-2:] == ["track", "contrast"]
    plain = sed.DOA(pos, grid)
    assert plain.contrast is None and "contrast" not in repr(plain)
    d = sed.DOA(pos, grid, contrast=sed.Contrast())
    assert d.contrast == sed.Contrast() and repr(d).endswith(", contrast=Contrast(frames=32, search=256, guard=2, min_frames=8, weight=1.0))")
    both = sed.DOA(pos, grid, track=sed.DirectionTrack(2, 15), contrast=sed.Contrast(8, 16, 0, 1, 2.0))
    assert "track=DirectionTrack(block_chunks=2, max_step_deg=15.0), contrast=Contrast(frames=8, search=16, guard=0, min_frames=1, weight=2.0))" in repr(both)
    with pytest.raises(TypeError, match="contrast must be None or a Contrast"):
        sed.DOA(pos, grid, contrast=dict(frames=8))


# ───────────── 2. the C entries ─────────────
def test_the_header_the_signatures_and_the_exports_agree(sed):
    from sed_crnn_amd import _lib, events, feature
    L, sig = _lib.lib(), _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sedcrnn.h")).read()
    for name in ENTRIES:
        for n in (name, name + "_workspace_bytes"):
            assert n in sig and f" {n}(" in header and hasattr(L, n), n
    i, p, l, d = C.c_int, C.c_void_p, C.c_long, C.c_double
    for old, new, tail in (("sed_event_doa", "sed_event_doa_contrast", 3), ("sed_event_doa_track", "sed_event_doa_track_contrast", 3)):
        (res, args), (nres, nargs) = sig[old], sig[new]
        # ev_cls follows ev_rec (argument 7); the six settings follow max_frames (argument 16); the two outputs precede the workspace
        assert nres == res and nargs == args[:8] + [p] + args[8:17] + [i, i, i, i, i, d] + args[17:-tail] + [p, p] + args[-tail:], new
        assert sig[new + "_workspace_bytes"] == (C.c_size_t, sig[old + "_workspace_bytes"][1] + [l, i])
    assert sig["sed_event_contrast_frames_workspace_bytes"] == (C.c_size_t, [i, i, l, i])
    assert sig["sed_event_contrast_frames"] == (i, [l, p, i, i, p, p, p, p, p, l, i, i, i, i, i, i, i, i, p, p, p, C.c_size_t, p])
    assert re.search(r"int sed_event_doa_contrast\([^;]*const int\* ev_rec, const int\* ev_cls, const int\* ev_onset,[^;]*int max_frames,\s+"
                     r"int n_classes, int frames, int search, int guard, int min_frames, double weight, float\* lag_out,[^;]*float\* srp_out, "
                     r"int\* bg_frames_out, int\* bg_sel_out,\s+void\* workspace, size_t workspace_bytes, void\* stream\);", header)
    assert len(sig["sed_event_doa"][1]) == 31 and len(sig["sed_event_doa_track"][1]) == 39          # the old entries are what they were
    assert events._ENTRY["doa_contrast", False] == "sed_event_doa_contrast" and events._ENTRY["doa_track_contrast", False] == "sed_event_doa_track_contrast"
    assert ("doa_contrast", True) not in events._ENTRY and ("doa_track_contrast", True) not in events._ENTRY
    assert feature.event_contrast_frames is events.event_contrast_frames and sed.Contrast is sed.localize.Contrast
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in integration, name


@pytest.mark.parametrize("frames,slots", [(1, 1), (32, 1), (33, 2), (256, 8)])
def test_workspace_sizes(frames, slots):
    """the recording table, mask_off [R] and the mask of sum L_r words — each rounded to 16 bytes — then per event the chunk slots
    of sed_event_tdoa and ceil(frames / 32) more (and the track's tail); 0 for sizes that are refused"""
    from sed_crnn_amd import _lib
    L = _lib.lib()

    def r16(v):
        return (v + 15) // 16 * 16
    for R, Cn, mf, words in ((1, 2, 12, 1), (3, 4, 256, 3), (3, 8, 40, 1001), (2, 3, 96, 1 << 33)):
        P = Cn * (Cn - 1) // 2
        tab = r16(8 * (R * Cn + R))
        mask = r16(8 * R) + r16(4 * words)
        assert L.sed_event_contrast_frames_workspace_bytes(R, Cn, words, frames) == tab + mask
        own = L.sed_event_doa_workspace_bytes(R, Cn, 1, 100000, 1024, mf) - tab
        assert own == -(-min(mf, 98) // 32) * P * ROW
        for E in (0, 1, 7):
            assert L.sed_event_doa_contrast_workspace_bytes(R, Cn, E, 100000, 1024, mf, words, frames) == tab + mask + E * (own + slots * P * ROW)
            for smooth in (0, 1):
                tail = L.sed_event_doa_track_workspace_bytes(R, Cn, E, 100000, 1024, mf, 24, 2, smooth) - L.sed_event_doa_workspace_bytes(R, Cn, E, 100000, 1024, mf)
                assert (tail > 0) == (smooth == 1 and E > 0)
                assert L.sed_event_doa_track_contrast_workspace_bytes(R, Cn, E, 100000, 1024, mf, 24, 2, smooth, words, frames) == \
                    tab + mask + E * (own + slots * P * ROW) + tail
    for bad in ((0, 2, 1, frames), (1, 1, 1, frames), (1, 9, 1, frames), (2, 2, 1, frames), (1, 2, 0, frames), (1, 2, (1 << 40) + 1, frames),
                (1, 2, 5, 0), (1, 2, 5, 257)):
        assert L.sed_event_contrast_frames_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 2, 1, 5000, 1024, 8, 5, frames), (1, 9, 1, 5000, 1024, 8, 5, frames), (1, 2, -1, 5000, 1024, 8, 5, frames),
                (1, 2, 1, 0, 1024, 8, 5, frames), (1, 2, 1, 5000, 0, 8, 5, frames), (1, 2, 1, 5000, 1024, 0, 5, frames),
                (1, 2, 1, 5000, 1024, 8, 0, frames), (3, 2, 1, 5000, 1024, 8, 2, frames), (1, 2, 1, 5000, 1024, 8, 5, 0), (1, 2, 1, 5000, 1024, 8, 5, 257)):
        assert L.sed_event_doa_contrast_workspace_bytes(*bad) == 0, bad
        assert L.sed_event_doa_track_contrast_workspace_bytes(*bad[:6], 24, 1, 1, *bad[6:]) == 0, bad
    for bad in ((0, 1, 1), (16385, 1, 1), (24, 0, 1), (24, 65, 1)):            # the track's own sizes
        assert L.sed_event_doa_track_contrast_workspace_bytes(1, 2, 1, 5000, 1024, 8, *bad, 5, frames) == 0, bad


def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE = C.c_void_p(0x1000)

    def frames(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, cls=FAKE, on=FAKE, K=10, Nb=8, S=32, G=1, M=1,
               used=FAKE, sel=FAKE, ws=FAKE, ws_bytes=0, R=1, rec=None):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_contrast_frames(20000, C.c_void_p(t.ctypes.data), R, channels, rec, cls, on, FAKE, FAKE, E, tf, hop, max_frames, K, Nb, S, G,
                                           M, used, sel, ws, ws_bytes, None)

    def doa(track=False, clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_lag=8, max_frames=8, cls=FAKE, on=FAKE, K=10, Nb=8,
            S=32, G=1, M=1, weight=1.0, used=FAKE, sel=FAKE, ws=FAKE, ws_bytes=0, pcm=FAKE, tables=FAKE, tables_bytes=5132 * 4, pad=0, steer=FAKE,
            D=24, Q=8, trig=FAKE, dir_=FAKE, lag=FAKE, W=1, tlen=FAKE, R=1, rec=None):
        t = np.asarray(clips, dtype=np.int64)
        head = (pcm, 20000, C.c_void_p(t.ctypes.data), R, channels, tables, tables_bytes, rec, cls, on, FAKE, FAKE, E, tf, hop, pad, max_lag, max_frames,
                K, Nb, S, G, M, weight, lag, FAKE, FAKE, None, steer, D, Q, trig, dir_, FAKE, None)
        if track:
            return L.sed_event_doa_track_contrast(*head, W, None, None, tlen, FAKE, FAKE, FAKE, None, used, sel, ws, ws_bytes, None)
        return L.sed_event_doa_contrast(*head, used, sel, ws, ws_bytes, None)

    def err():
        return L.sed_last_error_string().decode()
    settings = ((dict(Nb=0), "frames must be in [1, 256]"), (dict(Nb=257, S=300), "frames must be"), (dict(S=7), "search must be in [frames = 8, 4096]"),
                (dict(S=4097), "search must be"), (dict(G=-1), "guard must be in [0, 64]"), (dict(G=65), "guard must be"), (dict(M=0), "min_frames"),
                (dict(M=9), "min_frames must be in [1, frames = 8]"), (dict(K=0), "n_classes must be in [1, 32]"), (dict(K=33), "n_classes"),
                (dict(cls=None), "null pointer (ev_cls"), (dict(used=None), "null pointer (ev_cls"), (dict(sel=None), "null pointer (ev_cls"))
    shared = ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(tf=0), "bad sizes"),
              (dict(hop=0), "bad sizes"), (dict(E=-1), "bad sizes"), (dict(on=None), "null pointer"), (dict(R=2, clips=((0, 5000), (8000, 5000)) * 2), "need ev_rec"),
              (dict(clips=((0, 5000), (18000, 5000))), "not inside the PCM buffer"), (dict(clips=((0, 5000), (8000, 4000))), "equal length"))
    tab, mask = 32, 16 + 32                                                  # mask_off [1] and 5000 // 1024 + 1 = 5 words, each rounded to 16 bytes
    assert L.sed_event_contrast_frames_workspace_bytes(1, 2, 5, 8) == tab + mask
    for bad, what in settings + shared + ((dict(ws=None), "16-byte aligned"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"),
                                          (dict(), f"workspace of 0 bytes, {tab + mask} needed"), (dict(ws_bytes=tab + mask - 1), f"{tab + mask} needed")):
        assert frames(**bad) != 0 and what in err() and err().startswith("contrast_frames:"), (bad, err())
    assert frames(E=0) == 0 and frames(E=0, used=None, sel=None, cls=None) == 0                   # nothing is launched
    weights = ((dict(weight=0.0), "weight must be finite and in (0, 4]"), (dict(weight=4.5), "weight"), (dict(weight=float("nan")), "weight"),
               (dict(weight=float("inf")), "weight"), (dict(weight=-1.0), "weight"))
    one = tab + mask + 2 * ROW                                               # one own chunk and one background chunk of one pair
    assert L.sed_event_doa_contrast_workspace_bytes(1, 2, 1, 5000, 1024, 8, 5, 8) == one
    own = ((dict(steer=None), "null pointer (steering lags"), (dict(trig=None), "null pointer (steering lags"), (dict(dir_=None), "null pointer (steering lags"),
           (dict(D=0), "directions"), (dict(D=16385), "directions"), (dict(Q=3), "oversample"), (dict(max_lag=0), "max_lag"), (dict(max_lag=128), "max_lag"),
           (dict(pcm=None), "null pointer"), (dict(tables=None), "null pointer"), (dict(tables_bytes=5128 * 4), "table blob"), (dict(pad=2), "pad_mode"),
           (dict(lag=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"),
           (dict(), f"workspace of 0 bytes, at least {one} needed"), (dict(ws_bytes=one - 1), f"at least {one} needed"),
           (dict(Nb=33, S=33, ws_bytes=one), f"at least {one + ROW} needed"))
    for bad, what in settings + weights + shared + own:
        assert doa(**bad) != 0 and what in err() and err().startswith("doa_contrast:"), (bad, err())
    assert doa(E=0) == 0 and doa(E=0, used=None, sel=None, cls=None) == 0
    for bad, what in settings + weights + shared + own[:-3] + ((dict(W=0), "block_chunks"), (dict(W=65), "block_chunks"), (dict(tlen=None), "null pointer (trk_len_out"),
                                                               (dict(), f"workspace of 0 bytes, at least {one} needed"),
                                                               (dict(ws_bytes=one - 1), f"at least {one} needed")):
        assert doa(True, **bad) != 0 and what in err() and err().startswith("doa_track_contrast:"), (bad, err())
    assert doa(True, E=0) == 0 and doa(True, E=0, used=None, sel=None, cls=None) == 0


def test_build_guards_the_contrast_kernels_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS, SOURCES
    assert "contrast.hip" in SOURCES and set(KERNELS) <= set(NO_SCRATCH_KERNELS["contrast.hip"])
    assert "activity.hip" in SOURCES and "event_activity_k" in NO_SCRATCH_KERNELS["activity.hip"]
    assert NO_SCRATCH_KERNELS["tdoa.hip"] == ("tdoa_accum_k", "tdoa_finish_k") and "doa_steer_k" in NO_SCRATCH_KERNELS["doa.hip"]
    assert "doa_track_steer_k" in NO_SCRATCH_KERNELS["doatrack.hip"]        # (their contrast forms are instantiations: found by substring)
    every = [k for ks in NO_SCRATCH_KERNELS.values() for k in ks]
    for name in KERNELS + ("event_activity_k",):                             # the assembly tests and the guard find kernels by substring
        assert not any(o in name or name in o for o in every if o != name), name
    src = open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "contrast.hip")).read()
    for name in KERNELS:
        assert re.search(r"\b%s\b" % name, src), name
    assert re.search(r"\bevent_activity_k\b", open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "activity.hip")).read())
    assert "atomicOr" in src and not re.search(r"atomic(Add|Max|Min|CAS|Exch|And|Xor)", src)     # no atomics beyond the mask's OR


# ───────────── 3. what is refused ─────────────
def test_the_stream_the_ring_entry_and_the_python_entries_refuse_as_specified(sed):
    import torch
    from sed_crnn_amd import events, feature
    ct = sed.Contrast(8, 16)
    doa = sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(24), contrast=ct)
    plain = sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(24))
    net = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=4, n_mels=40).eval()
    det = sed.EventDetector(net, localize=doa)
    assert det.localize_settings is doa and det.with_decoder(threshold=0.3).localize_settings is doa
    with pytest.raises(NotImplementedError, match="follow-up") as e:
        det.stream(1, history_frames="min")
    assert "search + guard more feature frames of ring" in str(e.value) and "per-feed activity ring" in str(e.value)
    assert sed.EventDetector(net, localize=plain).stream(1, history_frames="min") is not None      # the plain detector streams as before
    with pytest.raises(NotImplementedError, match="no ring form"):
        events.event_doa_ring(None, 4096, [0], 4, {}, 1, doa)
    ev = {k: torch.zeros(1, dtype=torch.int32) for k in ("onset", "offset", "peak_frame", "cls")}
    with pytest.raises(TypeError, match=r"sed.DOA\(..., contrast=sed.Contrast"):
        feature.event_contrast_frames([(0, 5000)] * 4, 4, ev, 1, plain, 3)
    with pytest.raises(ValueError, match="4 microphone positions, the audio has 2 channels"):
        feature.event_contrast_frames([(0, 5000)] * 2, 2, ev, 1, doa, 3)
    for bad in (None, 0, 33, 2.5, True):
        with pytest.raises(ValueError, match="n_classes"):
            feature.event_contrast_frames([(0, 5000)] * 4, 4, ev, 1, doa, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature.event_contrast_frames([(0, 5000)] * 4, 4, ev, 1, doa, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        feature.event_doa(torch.zeros(20000), [(0, 5000)] * 4, 4, ev, 1, doa, n_classes=3)
    res = sed.DetectionResult(None, {"cls": torch.zeros(0)}, 0.1, None)
    with pytest.raises(AttributeError, match="bg_frames"):
        res.bg_frames
    assert sed.DetectionResult(None, {"bg_frames": 5}, 0.1, None).bg_frames == 5


# ───────────── 4. the selection on a hand-made table ─────────────
def test_the_selection_on_a_hand_made_table(sed):
    """one recording of 100 feature frames, time_factor 1, hop 1024 (an output frame is a feature frame; candidate g touches the
    output frames g - 1 and g), n_classes 4"""
    n, tf, hop, mf, K = 100 * 1024, 1, 1024, 12, 4
    ct = sed.Contrast(frames=8, search=20, guard=2, min_frames=1)

    def pick(rows, cls, c=ct):
        return cr.frames_of(rows, cls, n, tf, hop, mf, c, K)
    # an isolated event selects q = 0 .. Nb-1 (in summation order: descending)
    bg, sel = pick([(40, 46, 42)], [0])
    assert bg.tolist() == [8] and sel.tolist() == [[7, 6, 5, 4, 3, 2, 1, 0]]
    # right after a same-class event [30, 36): the frames g = 37 - q that touch it are g = 30 .. 36, q = 1 .. 7, exactly; with guard 2
    # the candidates start at g = 37
    bg, sel = pick([(30, 36, 32), (40, 46, 42)], [0, 0])
    assert bg.tolist() == [8, 8] and sel[1].tolist() == [14, 13, 12, 11, 10, 9, 8, 0]
    assert sel[0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    # ... and with guard 0 the candidates start at g = 39: q = 0, 1, 2 are free, q = 3 .. 9 touch [30, 36)
    assert pick([(30, 36, 32), (40, 46, 42)], [0, 0], sed.Contrast(8, 20, 0, 1))[1][1].tolist() == [14, 13, 12, 11, 10, 2, 1, 0]
    # covered by another class: as if alone; the other class's own selection is its own
    bg, sel = pick([(20, 60, 30), (40, 46, 42)], [1, 0])
    assert bg.tolist() == [8, 8] and sel[1].tolist() == [7, 6, 5, 4, 3, 2, 1, 0] and sel[0].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    # near the start: g = 5 - 2 - 1 - q >= 0 leaves q = 0, 1, 2: 0 < nb < Nb; with M = Nb the fallback, a row of -1
    bg, sel = pick([(5, 9, 6)], [2])
    assert bg.tolist() == [3] and sel.tolist() == [[2, 1, 0, -1, -1, -1, -1, -1]]
    bg, sel = pick([(5, 9, 6)], [2], sed.Contrast(8, 20, 2, 8))
    assert bg.tolist() == [0] and (sel == -1).all()
    # an activity of the class longer than the search: the fallback; an unlocated row (beyond the end) marks nothing and a class the
    # table does not count neither marks nor selects
    bg, sel = pick([(50, 90, 60), (90, 95, 91), (200, 210, 205), (0, 100, 5)], [3, 3, 0, 4])
    assert bg.tolist() == [8, 0, 0, 0] and (sel[1:] == -1).all()
    assert cr.activity([(200, 210, 205), (0, 100, 5), (-3, 5, 0)], [0, 4, 1], n, tf * hop, K).tolist() == [0] * 101
    # time_factor 8: an output frame is 8 feature frames; the event's own row blocks the candidates that reach into it
    bg, sel = cr.frames_of([(5, 6, 5)], [0], n, 8, 1024, mf, sed.Contrast(4, 20, 0, 1), K)
    assert bg.tolist() == [4] and sel.tolist() == [[3, 2, 1, 0]]             # g = 39 touches samples up to 40 * 1024: output frame 4 only


# ───────────── 5. the scene ─────────────
_SCENES = {}


def _located(sed, pair, db):
    """(plain dir, contrasted dir, contrasted doa_power, units) of one scene in float64, computed once"""
    if (pair, db) not in _SCENES:
        tg, ot = cr.PAIRS_DEG[pair]
        x = cr.scene(tg, ot, db, 100 + pair)
        units = cr.ring_units()
        _, J, ml = doa_ref.steering(doa_ref.tetrahedron(cr.EDGE), units, cr.SR, cr.Q)
        assert ml == sed.max_lag_for(cr.EDGE, cr.SR)
        Pk = doa_ref.whitened(x, cr.HOP)
        rows = [(cr.TARGET[0], cr.TARGET[1], 30)]
        ct = sed.Contrast(frames=16, search=64, guard=2, min_frames=8)
        plain = doa_ref.event_doa(Pk, rows, 1, J, ml, cr.Q, 256)
        con = cr.event_doa(Pk, rows, [0], x.shape[0], 1, cr.HOP, J, ml, cr.Q, 256, ct, 1)
        assert con["bg_frames"].tolist() == [16] and con["bg_sel"][0].tolist() == list(range(16))[::-1]
        _SCENES[pair, db] = (int(plain["dir"][0]), int(con["dir"][0]), float(con["doa_power"][0]), units)
    return _SCENES[pair, db]


def _deg(units, d, az_deg):
    return math.degrees(doa_ref.angle_between(units[d], doa_ref.unit(math.radians(az_deg))))


@pytest.mark.parametrize("db", [10.0, 30.0])
@pytest.mark.parametrize("pair", range(6))
def test_over_a_louder_source_the_plain_map_finds_the_interferer_and_the_contrasted_map_the_target(sed, pair, db):
    """5 degrees is twice the ring's covering radius (2.5 degrees)"""
    tg, ot = cr.PAIRS_DEG[pair]
    assert 70.0 <= min(abs(tg - ot), 360.0 - abs(tg - ot)) <= 160.0
    plain, con, power, units = _located(sed, pair, db)
    print(f"{db:+.0f} dB, target {tg}, interferer {ot}: plain dir {_deg(units, plain, ot):.1f} deg from the interferer, contrasted dir "
          f"{_deg(units, con, tg):.1f} deg from the target, doa_power {power:.3f}")
    assert _deg(units, plain, ot) <= 5.0 and _deg(units, con, tg) <= 5.0


@pytest.mark.parametrize("pair", range(6))
def test_for_an_isolated_event_the_two_maps_agree(sed, pair):
    plain, con, power, units = _located(sed, pair, None)
    assert plain == con and _deg(units, con, cr.PAIRS_DEG[pair][0]) <= 5.0


def test_an_mvdr_beam_steered_at_the_contrasted_dir_has_the_higher_sir(sed):
    """the reference's MVDR() beam (tests/mvdr_ref.py, loading 1e-2) on the event's samples of the first +10 dB scene, steered at
    the plain dir and at the contrasted dir: the output SIR (target / interferer under the same weights).
    Measured: steered at the plain dir -8.2 dB (the beam passes the interferer and cancels the target), at the contrasted dir +8.0 dB;
    the input SIR is -10.1 dB."""
    from sed_crnn_amd.localize import steering_delays
    tg, ot = cr.PAIRS_DEG[0]
    plain, con, _, units = _located(sed, 0, 10.0)
    xs, xi, xn = cr.scene_parts(tg, ot, 10.0, 100)
    x = (xs + xi + xn).astype(np.float32)
    tau = steering_delays(doa_ref.tetrahedron(cr.EDGE), sed.DirectionGrid(units), cr.SR)
    s0, length = cr.TARGET[0] * cr.HOP, (cr.TARGET[1] - cr.TARGET[0]) * cr.HOP
    sir = {}
    for name, d in (("plain", plain), ("contrasted", con)):
        _, (ys, yi) = mvdr_ref.event(x, s0, length, tau[d], sed.MVDR().loading, through=(xs, xi))
        sir[name] = mvdr_ref.db(ys, yi)
    print(f"MVDR output SIR: steered at the plain dir {sir['plain']:+.1f} dB, at the contrasted dir {sir['contrasted']:+.1f} dB "
          f"(input {mvdr_ref.db(xs[s0:s0 + length], xi[s0:s0 + length]):+.1f} dB)")
    assert sir["contrasted"] > sir["plain"]
