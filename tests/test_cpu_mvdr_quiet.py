"""The MVDR beam with its noise frames picked where the event's class is silent, the host side: the settings, the C
entries' signatures, argument checks and workspace sizes, the build guard, what the stream and the ring entry refuse, the rule as
the float64 reference (tests/mvdr_quiet_ref.py) applies it to the scene the feature was made for — a source that sounds twice —
and what the reference gains there.  No GPU.

Measured with the reference (tetrahedron at 44.1 kHz, bursts in blocks [8, 16) and [24, 40), the event is the second burst,
Kn = 8, G = 1, loading 1e-2; target level out / in and output SIR in dB: fixed stretch | selected frames | own frames):
    6 cm, 0 rad       -0.00 / 13.17 | -0.00 / 15.64 | -0.00 / 10.98
    6 cm, 0.05 rad    -1.22 / 12.58 | -0.02 / 15.60 | -3.98 /  9.20
    18 cm, 0 rad      -0.00 / 14.68 | -0.00 / 18.89 | -0.01 / 11.62
    18 cm, 0.05 rad   -3.37 / 12.74 | +0.13 / 18.45 | -8.26 /  6.99"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_noise_ref  # noqa: E402
import mvdr_quiet_ref  # noqa: E402
import mvdr_ref  # noqa: E402

B = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sed_event_quiet_frames", "sed_event_mvdr_quiet", "sed_event_quiet_frames_workspace_bytes", "sed_event_mvdr_quiet_workspace_bytes")
KERNELS = ("mvdr_select_k", "mvdr_quiet_own_k", "mvdr_quiet_k", "mvdr_quiet_weights_k")
# the issue's table: (spacing, error) -> (fixed, selected, own), each (target level, SIR)
TABLE = {(0.06, 0.0): ((-0.00, 13.17), (-0.00, 15.64), (-0.00, 10.98)), (0.06, 0.05): ((-1.22, 12.58), (-0.02, 15.60), (-3.98, 9.20)),
         (0.18, 0.0): ((-0.00, 14.68), (-0.00, 18.89), (-0.01, 11.62)), (0.18, 0.05): ((-3.37, 12.74), (0.13, 18.45), (-8.26, 6.99))}


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


# ───────────── 1. the settings ─────────────
def test_mvdr_validates_the_quiet_settings(sed):
    m = sed.MVDR()
    assert (m.noise_select, m.noise_search, m.noise_min, m.noise_exclude) == ("fixed", 0, 1, "same") and not m.quiet
    # what tests/test_cpu_mvdr_noise.py holds of the three older fields still holds
    assert (m.loading, m.noise_blocks, m.noise_guard) == (1e-2, 0, 1) and m == sed.MVDR(1e-2, 0, 1) and hash(m) == hash(sed.MVDR(0.01, 0, 1))
    assert sed.MVDR(0.5) == sed.MVDR(loading=0.5) and sed.MVDR(noise_blocks=8).noise_lead_blocks == 10 and m.noise_lead_blocks == 0
    assert sed.MVDR(noise_blocks=8) == sed.MVDR(1e-2, 8, 1, "fixed", 0, 1, "same") and sed.MVDR(noise_blocks=8).noise_search == 0
    q = sed.MVDR(noise_blocks=8, noise_select="quiet")
    assert q.quiet and q.noise_search == 32 and q.noise_min == 1 and q.noise_exclude == "same" and q != sed.MVDR(noise_blocks=8)
    assert q == sed.MVDR(noise_blocks=8, noise_select="quiet", noise_search=32)                   # stored resolved
    assert sed.MVDR(noise_blocks=256, noise_select="quiet").noise_search == 1024 and sed.MVDR(noise_blocks=1, noise_select="quiet").noise_search == 4
    n = sed.MVDR(noise_blocks=8, noise_select="quiet", noise_search=np.int64(70), noise_min=np.int32(8), noise_exclude="any")
    assert type(n.noise_search) is int and type(n.noise_min) is int and (n.noise_search, n.noise_min, n.noise_exclude) == (70, 8, "any")
    with pytest.raises(Exception):
        q.noise_select = "fixed"                                             # frozen
    for bad in (dict(noise_select="quiet"), dict(noise_blocks=0, noise_select="quiet"), dict(noise_blocks=8, noise_select="quiet", noise_search=7),
                dict(noise_blocks=8, noise_select="quiet", noise_min=9), dict(noise_select="loud"), dict(noise_exclude="none"), dict(noise_select=None),
                dict(noise_search=-1), dict(noise_search=1025), dict(noise_search=True), dict(noise_search=8.0), dict(noise_min=0),
                dict(noise_min=257), dict(noise_min="1"), dict(noise_min=None)):
        with pytest.raises(ValueError, match="MVDR: noise_"):
            sed.MVDR(**bad)


# ───────────── 2. the C entries ─────────────
def test_the_header_the_signatures_and_the_exports_agree():
    from sed_crnn_amd import _lib
    L, sig = _lib.lib(), _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sedcrnn.h")).read()
    for name in NEW:
        assert name in sig and f" {name}(" in header and hasattr(L, name), name
    i, p, l = C.c_int, C.c_void_p, C.c_long
    (res, args), (nres, nargs) = sig["sed_event_mvdr_noise"], sig["sed_event_mvdr_quiet"]
    at = args.index(C.c_double) + 3                                          # behind loading, noise_blocks and noise_guard
    # ev_cls follows ev_rec; n_classes, noise_search, noise_min, exclude_any follow noise_guard; noise_sel_out follows noise_frames_out
    assert nres == res and nargs == args[:6] + [p] + args[6:at] + [i, i, i, i] + args[at:-3] + [p] + args[-3:] and len(nargs) == len(args) + 6
    assert sig["sed_event_mvdr_quiet_workspace_bytes"] == (C.c_size_t, sig["sed_event_mvdr_noise_workspace_bytes"][1] + [l])
    assert sig["sed_event_quiet_frames_workspace_bytes"] == (C.c_size_t, [i, i, l, i])
    spans = sig["sed_event_beam_spans"][1]                                   # the selection reads no sample either: the spans' head and columns
    assert sig["sed_event_quiet_frames"] == (i, spans[:5] + [p] + spans[5:15] + [i] * 6 + [p, p] + spans[-3:])
    assert re.search(r"int sed_event_mvdr_quiet\([^;]*const int\* ev_rec,\s+const int\* ev_cls, [^;]*double loading, int noise_blocks, int noise_guard, "
                     r"int n_classes,\s+int noise_search, int noise_min,\s+int exclude_any, [^;]*int\* noise_frames_out,\s+int\* noise_sel_out, "
                     r"void\* workspace,\s+size_t workspace_bytes, void\* stream\);", header)
    assert len(sig["sed_event_mvdr_noise"][1]) == 30 and len(sig["sed_event_mvdr"][1]) == 27     # the old entries are what they were


@pytest.mark.parametrize("Kn,slots", [(1, 1), (32, 1), (33, 2), (256, 8)])
def test_workspace_sizes(Kn, slots):
    """the recording table, mask_off [R] and the mask of sum L_r words — each rounded to 16 bytes — and for the beam one event's
    rows as sed_event_mvdr_noise counts them"""
    from sed_crnn_amd import _lib
    L = _lib.lib()

    def r16(v):
        return (v + 15) // 16 * 16
    for R, Cn, frames in ((1, 2, 1), (3, 4, 3), (3, 8, 1001), (2, 3, 1 << 33)):
        tab = L.sed_event_beam_workspace_bytes(R, Cn)
        mask = r16(8 * R) + r16(4 * frames)
        assert L.sed_event_quiet_frames_workspace_bytes(R, Cn, frames, Kn) == tab + mask
        per_event = L.sed_event_mvdr_noise_workspace_bytes(R, Cn, 12, 1024, Kn) - tab
        assert per_event == (slots * Cn * (Cn + 1) // 2 + Cn) * 1026 * 8
        assert L.sed_event_mvdr_quiet_workspace_bytes(R, Cn, 12, 1024, Kn, frames) == tab + mask + per_event
    for bad in ((0, 2, 1, Kn), (1, 1, 1, Kn), (1, 9, 1, Kn), (2, 2, 1, Kn), (1, 2, 0, Kn), (1, 2, (1 << 40) + 1, Kn), (1, 2, 5, 0), (1, 2, 5, 257)):
        assert L.sed_event_quiet_frames_workspace_bytes(*bad) == 0, bad
    for bad in ((0, 2, 8, 1024, Kn, 5), (1, 9, 8, 1024, Kn, 5), (1, 2, 0, 1024, Kn, 5), (1, 2, 8, 0, Kn, 5), (1, 2, 8, 1024, 0, 5),
                (1, 2, 8, 1024, 257, 5), (1, 2, 8, 1024, Kn, 0), (3, 2, 8, 1024, Kn, 2)):
        assert L.sed_event_mvdr_quiet_workspace_bytes(*bad) == 0, bad


def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE = C.c_void_p(0x1000)
    row = 1026 * 8

    def beam(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, cls=FAKE, dir_=FAKE, loc=FAKE, tau=FAKE,
             loading=1e-2, Kn=8, G=1, K=10, S=32, M=1, any_=0, tables=FAKE, tables_bytes=5132 * 4, alen=FAKE, audio=FAKE, total=100, used=FAKE,
             sel=FAKE, ws=FAKE, ws_bytes=0, pcm=FAKE):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_mvdr_quiet(pcm, 20000, C.c_void_p(t.ctypes.data), 1, channels, None, cls, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop,
                                      max_frames, tau, D, loading, Kn, G, K, S, M, any_, tables, tables_bytes, alen, FAKE, audio, total, used, sel,
                                      ws, ws_bytes, None)

    def frames(clips=((0, 5000), (8000, 5000)), channels=2, E=1, tf=1, hop=1024, max_frames=8, D=72, cls=FAKE, dir_=FAKE, loc=FAKE, Kn=8, G=1, K=10,
               S=32, M=1, any_=0, used=FAKE, sel=FAKE, ws=FAKE, ws_bytes=0):
        t = np.asarray(clips, dtype=np.int64)
        return L.sed_event_quiet_frames(20000, C.c_void_p(t.ctypes.data), 1, channels, None, cls, FAKE, FAKE, FAKE, dir_, loc, E, tf, hop, max_frames,
                                        D, K, Kn, G, S, M, any_, used, sel, ws, ws_bytes, None)

    def err():
        return L.sed_last_error_string().decode()
    shared = ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(tf=0), "bad sizes"),
              (dict(hop=0), "bad sizes"), (dict(E=-1), "bad sizes"), (dict(D=0), "at least one direction"), (dict(dir_=None), "null pointer"),
              (dict(loc=None), "null pointer"), (dict(clips=((0, 5000), (18000, 5000))), "not inside the PCM buffer"),
              (dict(clips=((0, 5000), (8000, 4000))), "equal length"),
              (dict(Kn=0), "noise_blocks must be in [1, 256]"), (dict(Kn=257, S=300), "noise_blocks"), (dict(G=-1), "noise_guard"), (dict(G=65), "noise_guard"),
              (dict(S=7), "noise_search must be in [noise_blocks = 8, 1024]"), (dict(S=1025), "noise_search"), (dict(M=0), "noise_min"),
              (dict(M=9), "noise_min must be in [1, noise_blocks = 8]"), (dict(K=0), "n_classes must be in [1, 32]"), (dict(K=33), "n_classes"),
              (dict(any_=2), "exclude_any"), (dict(cls=None), "null pointer (ev_cls"), (dict(used=None), "null pointer (ev_cls"),
              (dict(sel=None), "null pointer (ev_cls"), (dict(ws=None), "16-byte aligned"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"))
    mask = 16 + 32                                                           # mask_off [1] and 5000 // 1024 + 1 = 5 words, each rounded to 16 bytes
    assert L.sed_event_quiet_frames_workspace_bytes(1, 2, 5, 8) == 32 + mask
    for bad, what in shared + ((dict(), f"workspace of 0 bytes, {32 + mask} needed"), (dict(ws_bytes=32 + mask - 1), f"{32 + mask} needed")):
        assert frames(**bad) != 0 and what in err() and err().startswith("quiet_frames:"), (bad, err())
    assert frames(E=0) == 0 and frames(E=0, used=None, sel=None, cls=None) == 0                   # nothing is launched
    for bad, what in shared + ((dict(pcm=None), "null pointer (the samples)"), (dict(pcm=C.c_void_p(0x1002)), "4-byte aligned"),
                               (dict(loading=0.0), "loading"), (dict(loading=float("nan")), "loading"), (dict(tau=None), "null pointer (tau"),
                               (dict(alen=None), "null pointer (tau"), (dict(audio=None), "null output buffer"), (dict(total=-1), "a total of -1"),
                               (dict(tables=None), "table blob"), (dict(tables_bytes=5128 * 4), "table blob"),
                               (dict(), "workspace of 0 bytes"), (dict(ws_bytes=32 + mask + 5 * row - 1), f"at least {32 + mask + 5 * row} needed"),
                               (dict(Kn=33, S=33, ws_bytes=32 + mask + 5 * row), f"at least {32 + mask + 8 * row} needed")):
        assert beam(**bad) != 0 and what in err() and err().startswith("mvdr_quiet:"), (bad, err())
    assert beam(E=0) == 0 and beam(total=0, audio=None) == 0 and beam(E=0, used=None, sel=None, cls=None) == 0


def test_build_guards_the_quiet_kernels_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS, SOURCES
    assert set(KERNELS) <= set(NO_SCRATCH_KERNELS["mvdr.hip"])
    assert "activity.hip" in SOURCES and "event_activity_k" in NO_SCRATCH_KERNELS["activity.hip"]
    older = ("mvdr_cov_k", "mvdr_weights_k", "mvdr_apply_k", "mvdr_noise_k", "mvdr_ring_noise_k", "mvdr_ring_cov_k", "mvdr_ring_apply_k")
    assert set(older) <= set(NO_SCRATCH_KERNELS["mvdr.hip"])
    for name in KERNELS + ("event_activity_k",):                             # the assembly tests and the guard find kernels by substring
        assert not any(o in name for o in older), name
    src = open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "mvdr.hip")).read()
    for name in KERNELS:
        assert re.search(r"\b%s\b" % name, src), name
    assert re.search(r"\bevent_activity_k\b", open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "activity.hip")).read())


# ───────────── 3. what is refused ─────────────
def test_the_stream_the_ring_entry_and_the_python_entries_refuse_as_specified(sed):
    import torch
    from sed_crnn_amd import events, feature
    assert feature.event_quiet_frames is events.event_quiet_frames
    doa = sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(12), max_frames=16)
    net = sed.LightningTimePooledCRNN(dropout=0.0, in_channels=4, n_mels=40).eval()
    mv = sed.MVDR(noise_blocks=8, noise_select="quiet")
    det = sed.EventDetector(net, localize=doa, extract=mv)
    assert det.extract_settings is mv and det.with_decoder(threshold=0.3).extract_settings is mv
    with pytest.raises(NotImplementedError, match="follow-up") as e:
        det.stream(1, history_frames="min", emit_audio=True)
    assert "'same'" in str(e.value) and "noise_search more blocks of ring" in str(e.value) and "open events" in str(e.value)
    with pytest.raises(NotImplementedError, match="emit_audio=True"):       # without emit_audio: what every extracting detector is told
        det.stream(1, history_frames="min")
    fixed = sed.EventDetector(net, localize=doa, extract=sed.MVDR(noise_blocks=8))
    assert fixed.stream(1, history_frames="min", emit_audio=True).noise_frames > 0               # the fixed stretch streams as before
    with pytest.raises(NotImplementedError, match="no ring form"):
        events.event_mvdr_ring(None, 4096, [0], 4, {}, 1, doa, mv)
    empty = det._no_lags()
    assert empty["noise_sel"].shape == (0, 8) and empty["noise_sel"].dtype == torch.int32 and "noise_sel" not in fixed._no_lags()
    with pytest.raises(TypeError, match="noise_select='quiet'"):
        events.event_quiet_frames([(0, 5000)] * 4, 4, {}, 1, doa, sed.MVDR(noise_blocks=8), 10)
    for bad in (None, 0, 33, 2.5, True):
        with pytest.raises(ValueError, match="n_classes"):
            events.event_quiet_frames([(0, 5000)] * 4, 4, {}, 1, doa, mv, bad)


# ───────────── 4. the rule, as the reference applies it ─────────────
def test_the_reference_selects_the_frames_of_the_issue():
    """tf = 8, hop = 1024, same-class events at output frames [1, 2) and [3, 5), the event at s0 = 24 B, Kn = 8, G = 1"""
    for S in (19, 22, 32, 70):
        elig, sel = mvdr_quiet_ref.scene_selection(S=S)
        assert elig == [q for q in (0, 1, 2, 3, 4, 16, 17, 18, 19, 20, 21) if q < S], (S, elig)
        assert sel == [18, 17, 16, 4, 3, 2, 1, 0]                            # summation order: ascending time
    assert [21 - q for q in sel] == [3, 4, 5, 17, 18, 19, 20, 21]            # the blocks the frames start at
    # an other-class event over output frame 2 changes nothing under "same" and removes q = 0..4 under "any"
    rows, cls = mvdr_quiet_ref.ROWS + [(2, 3, 2)], mvdr_quiet_ref.CLS + [1]
    assert mvdr_quiet_ref.scene_selection(rows=rows, cls=cls) == (elig[:11], sel)
    elig_any, sel_any = mvdr_quiet_ref.scene_selection(exclude="any", rows=rows, cls=cls)
    assert elig_any == [16, 17, 18, 19, 20, 21] and sel_any == [21, 20, 19, 18, 17, 16]
    assert mvdr_quiet_ref.scene_selection(exclude="any", M=7, rows=rows, cls=cls)[1] == []       # fewer than noise_min: the own frames
    # rows that mark nothing: an unknown class, a negative onset, an empty interval; offsets beyond the end are clamped
    n, H = 48 * B, 8 * B
    m = mvdr_quiet_ref.activity([(1, 2), (0, 9), (-1, 3), (4, 4), (5, 99), (7, 8)], [0, 2, 0, 1, 1, 1], n, H, 2)
    assert m.dtype == np.uint32 and m.tolist() == [0, 1, 0, 0, 0, 2, 2]      # L = 48 // 8 + 1 = 7: frame 7 does not exist


@pytest.mark.parametrize("Kn,G", [(1, 0), (8, 1), (33, 1)])
def test_an_isolated_event_is_the_fixed_stretch_exactly(Kn, G):
    """nothing is active before the event: q = Kn-1 .. 0 are selected, and the audio is mvdr_noise_ref.event's, bit for bit"""
    pos = doa_ref.tetrahedron(0.06)
    x, tau = sum(mvdr_ref.scene(48 * B, pos, mvdr_noise_ref.SR)), mvdr_noise_ref.steered(pos, 0.05)
    s0 = -(-(G + Kn + 1) * B // 1001) * 1001                              # the first frame of hop 1001 with all Kn candidates
    mask = mvdr_quiet_ref.activity([(s0 // 1001, s0 // 1001 + 3)], [4], 48 * B, 1001, 10)
    n_e, sel = mvdr_quiet_ref.select(mask, s0, 4, 1001, Kn, G, 70, Kn, "any", 10)
    assert n_e == Kn and sel.tolist() == list(range(Kn - 1, -1, -1))
    for f32 in (False, True):
        y, _, used = mvdr_noise_ref.event(x, s0, 3 * B, tau, 1e-2, Kn, G, f32)
        assert used == Kn and np.array_equal(mvdr_quiet_ref.event(x, s0, 3 * B, tau, 1e-2, G, sel, f32)[0], y)
        own = mvdr_quiet_ref.event(x, s0, 3 * B, tau, 1e-2, G, [], f32)[0]
        assert np.array_equal(own, mvdr_ref.event(x, s0, 3 * B, tau, 1e-2, f32)[0]) and not np.array_equal(own, y)
    # one block earlier the farthest candidate does not exist: partial use, or the fallback with noise_min = Kn
    n_e, sel = mvdr_quiet_ref.select(mask, (G + Kn + 1) * B - 1, 4, 1001, Kn, G, 70, 1, "same", 10)
    assert n_e == Kn - 1 and sel.tolist() == list(range(Kn - 2, -1, -1)) + [-1]
    assert mvdr_quiet_ref.select(mask, (G + Kn + 1) * B - 1, 4, 1001, Kn, G, 70, Kn, "same", 10)[0] == 0
    assert mvdr_quiet_ref.select(mask, s0, 10, 1001, Kn, G, 70, 1, "same", 10)[0] == 0           # a class the table does not count


@pytest.fixture(scope="module")
def table():
    rows = {k: mvdr_quiet_ref.measure(*k) for k in TABLE}
    print("array, steering error: target level out/in and output SIR (dB), fixed | selected | own")
    for (sp, err), m in rows.items():
        print(f"  {sp * 100:.0f} cm, {err:.2f} rad: " + " | ".join(f"{m[k][0]:+.2f} / {m[k][1]:.2f}" for k in ("fixed", "quiet", "own")))
    return rows


def test_the_reference_reproduces_the_table(table):
    for key, want in TABLE.items():
        for name, w in zip(("fixed", "quiet", "own"), want):
            assert abs(table[key][name][0] - w[0]) <= 0.05 and abs(table[key][name][1] - w[1]) <= 0.05, (key, name, table[key][name], w)
    five = {}                                                                # the five frames at blocks 17 .. 21 alone
    for sp in (0.06, 0.18):
        pos, xs, xi, xn = mvdr_quiet_ref.twice_scene(sp)
        _, (ys, yi, yn) = mvdr_quiet_ref.event(xs + xi + xn, 24 * B, 16 * B, mvdr_noise_ref.steered(pos, 0.05), 1e-2, 1, [4, 3, 2, 1, 0],
                                               through=(xs, xi, xn))
        five[sp] = mvdr_ref.db(ys, yi)
    print(f"five frames: {five[0.06]:.2f} dB, {five[0.18]:.2f} dB")
    assert abs(five[0.06] - 15.57) <= 0.05 and abs(five[0.18] - 18.41) <= 0.05


@pytest.mark.parametrize("spacing,fixed_below,gap", [(0.06, -1.0, 2.5), (0.18, -3.0, 5.0)])
def test_the_selected_frames_keep_the_target_and_the_suppression(table, spacing, fixed_below, gap):
    """0.05 rad of steering error: the fixed stretch holds the end of the earlier burst and the beam cancels part of the target;
    the selected frames have never seen it.  Measured gaps in output SIR: 3.0 dB (6 cm) and 5.7 dB (18 cm)"""
    m = table[(spacing, 0.05)]
    assert abs(m["quiet"][0]) <= 0.25 and m["fixed"][0] < fixed_below
    assert m["quiet"][1] - m["fixed"][1] >= gap
