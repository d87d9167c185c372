"""The MVDR beam steered along the event's direction track, the host side: the setting and what it refuses, the C
entries' argument checks and workspace sizes, the build guard, the frame-to-block rule against a loop, and what the float64
reference (tests/mvdr_track_ref.py) does on the scene the feature was made for: a source that moves by 10 degrees per track block
while a static, stronger second source sounds.  No GPU.

Measured with the reference (tetrahedron at 44.1 kHz, hop 1024, an event of 8 track blocks of 32 frames, loading 1e-2; target level
out / in and output SIR in dB, whole event | last block; "one dir" steers at 30 degrees, "tracked" at every block's own azimuth):
    array, covariance        one dir                         tracked
    6 cm, own frames         -3.79, 8.58 | -8.34, 4.70       -0.02, 12.99 | -0.00, 13.89
    6 cm, 8 pre-onset        -2.24, 10.66 | -3.86, 9.75      -0.02, 13.61 | -0.00, 15.61
    18 cm, own frames        -4.39, 11.92 | -6.85, 10.51     -0.05, 13.18 | -0.00, 17.67
    18 cm, 8 pre-onset       -3.31, 13.98 | -4.24, 14.45     -0.05, 17.30 | -0.00, 20.55
6 cm, own frames: the target as the beam passes it against the source at the centroid, -2.61 dB with one dir, -28.12 dB tracked;
with 3 degrees per block one dir still loses 3.89 dB of the target in the last block, tracked 0.00."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import doa_ref  # noqa: E402
import mvdr_ref  # noqa: E402
import mvdr_track_ref  # noqa: E402

B = 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sed_event_mvdr_track", "sed_event_mvdr_track_ring", "sed_event_mvdr_quiet_track")
NEW_KERNELS = ("mvdr_trk_weights_k", "mvdr_trk_quiet_weights_k", "mvdr_trk_apply_k", "mvdr_trk_ring_apply_k")


@pytest.fixture(scope="module")
def sed():
    import sed_crnn_amd as s
    return s


def _net(cin=4):
    import sed_crnn_amd as sed
    return sed.LightningTimePooledCRNN(dropout=0.0, in_channels=cin, n_mels=40).eval()


def _doa(sed, track=True):
    return sed.DOA(doa_ref.tetrahedron(0.06), sed.DirectionGrid.ring(12), max_frames=96, track=sed.DirectionTrack(1) if track else None)


# ───────────── 1. the setting ─────────────
def test_follow_track_is_a_validated_last_field(sed):
    import dataclasses
    m = sed.MVDR()
    assert m.follow_track is False and m == sed.MVDR(1e-2, 0, 1) and hash(m) == hash(sed.MVDR(1e-2, 0, 1))
    assert [f.name for f in dataclasses.fields(sed.MVDR)][-1] == "follow_track"
    t = sed.MVDR(follow_track=True)
    assert t.follow_track is True and t != m and sed.MVDR(follow_track=np.bool_(True)) == t and type(sed.MVDR(follow_track=np.bool_(True)).follow_track) is bool
    assert sed.MVDR(1e-2, 8, 1, "quiet", 0, 1, "same", True).follow_track is True
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="MVDR: follow_track"):
            sed.MVDR(follow_track=bad)
    with pytest.raises(Exception):
        t.follow_track = False                                               # frozen


def test_the_detector_and_the_functions_need_a_track(sed):
    import torch
    from sed_crnn_amd import feature
    t = sed.MVDR(follow_track=True)
    with pytest.raises(ValueError, match="track="):
        sed.EventDetector(_net(), localize=_doa(sed, track=False), extract=t)
    with pytest.raises(ValueError, match="extract=MVDR"):
        sed.EventDetector(_net(), extract=t)
    det = sed.EventDetector(_net(), localize=_doa(sed), extract=t)
    assert det.extract_settings is t and det.with_decoder(threshold=0.3).extract_settings is t
    plain = sed.EventDetector(_net(), localize=_doa(sed), extract=sed.MVDR())
    st, own = det.stream(3, history_frames="min", emit_audio=True), plain.stream(3, history_frames="min", emit_audio=True)
    assert st.state_bytes == own.state_bytes and st.cap == own.cap and st.history_frames == own.history_frames      # no new state
    if not torch.cuda.is_available():
        return
    # (the checks below need device tensors to get as far as the track's)
    ev = {k: torch.zeros(1, dtype=torch.int32, device="cuda") for k in ("onset", "offset", "peak_frame", "dir", "loc_frames")}
    pcm = torch.zeros(4 * 4096, device="cuda")
    clips = [(c * 4096, 4096) for c in range(4)]
    with pytest.raises(ValueError, match="track="):
        feature.event_mvdr(pcm, clips, 4, ev, 1, _doa(sed), t, sr=44100, hop=1024)                # no columns
    with pytest.raises(ValueError, match="track="):
        feature.event_mvdr(pcm, clips, 4, {**ev, "trk_len": ev["dir"], "trk_dir": ev["dir"][:, None]}, 1, _doa(sed, track=False), t, sr=44100,
                           hop=1024)


# ───────────── 2. the C entries ─────────────
def test_the_header_the_signatures_and_the_exports_agree():
    from sed_crnn_amd import _lib
    L, sig = _lib.lib(), _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "sedcrnn.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        for n in (name, name + "_workspace_bytes"):
            assert n in sig and f" {n}(" in header and hasattr(L, n) and n in doc, n
    i, p = C.c_int, C.c_void_p
    for old, new in (("sed_event_mvdr_noise", "sed_event_mvdr_track"), ("sed_event_mvdr_noise_ring", "sed_event_mvdr_track_ring"),
                     ("sed_event_mvdr_quiet", "sed_event_mvdr_quiet_track")):
        (res, args), (nres, nargs) = sig[old], sig[new]
        assert nres == res and nargs == args[:-3] + [i, i, p, p] + args[-3:]                     # behind the last output, before the workspace
        assert sig[new + "_workspace_bytes"] == (C.c_size_t, sig[old + "_workspace_bytes"][1] + [i])
        assert re.search(r"int %s\([^;]*int\* noise_\w+_out,\s+int block_chunks, int track_slots, const int\* trk_len,\s+const int\* trk_dir,"
                         r"\s+void\* workspace,\s+size_t workspace_bytes, void\* stream\);" % new, header)
    assert len(sig["sed_event_mvdr_noise"][1]) == 30 and len(sig["sed_event_mvdr_quiet"][1]) == 36   # the old entries are what they were


def test_workspace_sizes():
    """per event the chunk slots of the untracked entry and C rows of weights for each of Tm blocks: monotone in track_slots, the
    untracked size at Tm = 1, 0 for refused sizes"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    row = 1026 * 8
    for Cn in (2, 4, 8):
        for Kn in (0, 8, 40):
            base = L.sed_event_mvdr_noise_workspace_bytes(1, Cn, 96, 1024, Kn)
            ring = L.sed_event_mvdr_noise_ring_workspace_bytes(3, Cn, 96, 1024, Kn)
            quiet = L.sed_event_mvdr_quiet_workspace_bytes(1, Cn, 96, 1024, max(Kn, 1), 13)
            last = 0
            for Tm in (1, 2, 3, 96, 256):
                got = L.sed_event_mvdr_track_workspace_bytes(1, Cn, 96, 1024, Kn, Tm)
                assert got == base + (Tm - 1) * Cn * row and got > last
                last = got
                assert L.sed_event_mvdr_track_ring_workspace_bytes(3, Cn, 96, 1024, Kn, Tm) == ring + (Tm - 1) * Cn * row
                assert L.sed_event_mvdr_quiet_track_workspace_bytes(1, Cn, 96, 1024, max(Kn, 1), 13, Tm) == quiet + (Tm - 1) * Cn * row
    for bad in ((0, 2, 8, 1024, 0, 1), (1, 1, 8, 1024, 0, 1), (1, 9, 8, 1024, 0, 1), (1, 2, 0, 1024, 0, 1), (1, 2, 8, 0, 0, 1), (1, 2, 8, 1024, -1, 1),
                (1, 2, 8, 1024, 257, 1), (1, 2, 8, 1024, 0, 0), (1, 2, 8, 1024, 0, 257), (1, 2, 8, 1024, 0, -1)):
        assert L.sed_event_mvdr_track_workspace_bytes(*bad) == 0 and L.sed_event_mvdr_track_ring_workspace_bytes(*bad) == 0, bad
    for bad in ((1, 2, 8, 1024, 0, 5, 1), (1, 2, 8, 1024, 8, 0, 1), (1, 2, 8, 1024, 8, 5, 0), (1, 2, 8, 1024, 8, 5, 257), (1, 9, 8, 1024, 8, 5, 1)):
        assert L.sed_event_mvdr_quiet_track_workspace_bytes(*bad) == 0, bad


def test_c_entries_check_their_arguments_on_the_host():
    """every refusal is made before anything is enqueued: the pointers are never followed (they point nowhere)"""
    from sed_crnn_amd import _lib
    L = _lib.lib()
    FAKE = C.c_void_p(0x1000)
    row = 1026 * 8

    def linear(channels=2, E=1, hop=1024, max_frames=8, D=72, dir_=FAKE, tau=FAKE, loading=1e-2, Kn=0, G=1, tables=FAKE, tables_bytes=5132 * 4,
               alen=FAKE, audio=FAKE, total=100, used=FAKE, W=1, Tm=1, tlen=FAKE, tdir=FAKE, ws=FAKE, ws_bytes=0, pcm=FAKE):
        t = np.asarray(((0, 5000), (8000, 5000)), dtype=np.int64)
        return L.sed_event_mvdr_track(pcm, 20000, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, dir_, FAKE, E, 1, hop,
                                      max_frames, tau, D, loading, Kn, G, tables, tables_bytes, alen, FAKE, audio, total, used, W, Tm, tlen, tdir,
                                      ws, ws_bytes, None)

    def ring(channels=2, E=1, hop=1024, max_frames=8, D=72, loading=1e-2, Kn=0, G=1, tables=FAKE, tb=1 << 16, alen=FAKE, audio=FAKE, total=100,
             used=FAKE, W=1, Tm=1, tlen=FAKE, tdir=FAKE, ws=FAKE, ws_bytes=0, cap=8192, n=9000, ring_=FAKE, tau=FAKE):
        t = np.asarray([n], dtype=np.int64)
        return L.sed_event_mvdr_track_ring(ring_, 1 << 20, cap, C.c_void_p(t.ctypes.data), 1, channels, None, FAKE, FAKE, FAKE, FAKE, FAKE, E, 1,
                                           hop, max_frames, tau, D, loading, Kn, G, tables, tb, alen, FAKE, audio, total, used, W, Tm, tlen, tdir,
                                           ws, ws_bytes, None)

    def quiet(channels=2, E=1, hop=1024, max_frames=8, D=72, loading=1e-2, Kn=8, G=1, K=3, S=32, M=1, any_=0, cls=FAKE, total=100, audio=FAKE,
              used=FAKE, sel=FAKE, W=1, Tm=1, tlen=FAKE, tdir=FAKE, ws=FAKE, ws_bytes=0):
        t = np.asarray(((0, 5000), (8000, 5000)), dtype=np.int64)
        return L.sed_event_mvdr_quiet_track(FAKE, 20000, C.c_void_p(t.ctypes.data), 1, channels, None, cls, FAKE, FAKE, FAKE, FAKE, FAKE, E, 1,
                                            hop, max_frames, FAKE, D, loading, Kn, G, K, S, M, any_, FAKE, 5132 * 4, FAKE, FAKE, audio, total,
                                            used, sel, W, Tm, tlen, tdir, ws, ws_bytes, None)

    def err():
        return L.sed_last_error_string().decode()
    one = 32 + (1 * 3 + 2 * 3) * row                                         # C = 2, one chunk slot, Tm = 3
    for bad, what in ((dict(channels=1), "channels"), (dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(hop=0), "bad sizes"),
                      (dict(E=-1), "bad sizes"), (dict(D=0), "at least one direction"), (dict(dir_=None), "null pointer"),
                      (dict(pcm=None), "null pointer (the samples)"), (dict(loading=0.0), "loading"), (dict(Kn=-1), "noise_blocks"),
                      (dict(Kn=257), "noise_blocks"), (dict(G=65), "noise_guard"), (dict(used=None), "null pointer (noise_frames_out)"),
                      (dict(W=0), "block_chunks must be in [1, 64]"), (dict(W=65), "block_chunks must be in [1, 64]"),
                      (dict(Tm=0), "track_slots must be in [1, 256]"), (dict(Tm=257), "track_slots must be in [1, 256]"),
                      (dict(tlen=None), "null pointer (trk_len or trk_dir)"), (dict(tdir=None), "null pointer (trk_len or trk_dir)"),
                      (dict(tau=None), "null pointer (tau"), (dict(alen=None), "null pointer (tau"), (dict(audio=None), "null output buffer"),
                      (dict(total=-1), "a total of -1"), (dict(tables=None), "table blob"), (dict(tables_bytes=5128 * 4), "table blob"),
                      (dict(ws=None), "16-byte aligned"), (dict(ws=C.c_void_p(0x1008)), "16-byte aligned"), (dict(), "workspace of 0 bytes"),
                      (dict(Tm=3, ws_bytes=one - 1), f"at least {one} needed"),
                      (dict(Tm=3, ws_bytes=32 + 5 * row), f"at least {one} needed")):               # the untracked entry's size is too small
        assert linear(**bad) != 0 and what in err() and err().startswith("mvdr_track:"), (bad, err())
    assert linear(E=0) == 0 and linear(total=0, audio=None) == 0 and linear(E=0, used=None, tlen=None, tdir=None) == 0   # nothing is launched
    for bad, what in ((dict(channels=9), "channels"), (dict(max_frames=0), "max_frames"), (dict(D=0), "at least one direction"),
                      (dict(ring_=None), "null pointer (the rings)"), (dict(cap=100), "a ring holds"), (dict(loading=0.0), "loading"),
                      (dict(Kn=257), "noise_blocks"), (dict(G=65), "noise_guard"), (dict(used=None), "null pointer (noise_frames_out)"),
                      (dict(W=0), "block_chunks"), (dict(W=65), "block_chunks"), (dict(Tm=0), "track_slots"), (dict(Tm=257), "track_slots"),
                      (dict(tlen=None), "null pointer (trk_len or trk_dir)"), (dict(tdir=None), "null pointer (trk_len or trk_dir)"),
                      (dict(total=-1), "a total of -1"), (dict(tau=None), "null pointer"), (dict(audio=None), "null output buffer"),
                      (dict(tables=None), "table blob"), (dict(), "workspace of 0 bytes"),
                      (dict(Tm=3, ws_bytes=L.sed_event_mvdr_track_ring_workspace_bytes(1, 2, 8, 1024, 0, 3) - 1), "needed (one event)")):
        assert ring(**bad) != 0 and what in err() and err().startswith("mvdr_track_ring:"), (bad, err())
    assert ring(E=0) == 0 and ring(total=0, audio=None) == 0
    for bad, what in ((dict(channels=9), "channels"), (dict(Kn=0), "noise_blocks must be in [1, 256]"), (dict(S=4), "noise_search"),
                      (dict(M=9), "noise_min"), (dict(K=33), "n_classes"), (dict(any_=2), "exclude_any"), (dict(cls=None), "null pointer (ev_cls"),
                      (dict(sel=None), "null pointer (ev_cls"), (dict(W=0), "block_chunks"), (dict(Tm=257), "track_slots"),
                      (dict(tlen=None), "null pointer (trk_len or trk_dir)"), (dict(audio=None), "null output buffer"),
                      (dict(ws=None), "16-byte aligned"), (dict(), "workspace of 0 bytes"),
                      (dict(Tm=3, ws_bytes=L.sed_event_mvdr_quiet_track_workspace_bytes(1, 2, 8, 1024, 8, 5, 3) - 1), "needed (one event)")):
        assert quiet(**bad) != 0 and what in err() and err().startswith("mvdr_quiet_track:"), (bad, err())
    assert quiet(E=0) == 0 and quiet(total=0, audio=None) == 0


def test_build_guards_the_tracked_kernels_against_scratch():
    from sed_crnn_amd.build import NO_SCRATCH_KERNELS
    listed = NO_SCRATCH_KERNELS["mvdr.hip"]
    assert set(NEW_KERNELS) <= set(listed) and len(listed) == 15            # (the activity kernel is activity.hip's)
    assert NO_SCRATCH_KERNELS["activity.hip"] == ("event_activity_k",)
    for new in NEW_KERNELS:                                                  # the assembly tests and the guard find kernels by substring
        for old in listed:
            assert old == new or old not in new, (old, new)
    src = open(os.path.join(ROOT, "sed_crnn_amd", "csrc", "mvdr.hip")).read()
    for new in NEW_KERNELS:
        assert re.search(r"__global__[^\n]*void %s\(" % new, src), new
    tracked = src[src.index("struct MvTrack {"):src.index("long mv_chunks(")]
    assert "atomic" not in tracked.replace("no atomics", "")                # plain vector stores only


# ───────────── 3. the rule ─────────────
@pytest.mark.parametrize("hop", [1024, 1001, 441])
@pytest.mark.parametrize("W", [1, 2])
def test_frame_blocks_against_a_loop(sed, hop, W):
    lengths = [0, 1, 1023, 1024, 1025, 31 * hop, 32 * hop, 32 * hop + 1, 33 * hop, 47 * hop, 48 * hop, 64 * hop - 7, 64 * hop, 96 * hop, 97 * hop + 300,
               128 * hop + 5]
    for length in lengths:
        for T in range(5):
            got = sed.mvdr_frame_blocks(length, hop, W, T)
            J = -(-length // B)
            want = []
            for j in range(J + 1):
                centre = j * B                                               # sample j B of the event ...
                located = centre // hop                                      # ... lies in this located frame ...
                block = located // (32 * W)                                  # ... and that in this block of the track
                want.append(0 if T == 0 else min(block, T - 1))
            assert got.dtype == np.int64 and got.tolist() == want == mvdr_track_ref.frame_blocks(length, hop, W, T), (length, T)
            assert (np.diff(got) >= 0).all() and (len(want) == 1 or T == 0 or got.max() <= T - 1)
    assert sed.mvdr_frame_blocks(96 * 1024, 1024, 1, 3).tolist() == [0] * 32 + [1] * 32 + [2] * 33
    for bad in ((-1, 1024, 1, 1), (10, 0, 1, 1), (10, 1024, 0, 1), (10, 1024, 65, 1), (10, 1024, 1, -1), (10, 1024, 1, 257)):
        with pytest.raises(ValueError, match="mvdr_frame_blocks"):
            sed.mvdr_frame_blocks(*bad)


def test_the_rule_agrees_with_track_blocks(sed):
    """a frame whose centre lies in block b of localize.track_blocks takes block b, the joined short tail the last block"""
    for hop in (1024, 1001, 441):
        for W in (1, 2):
            for nf in (1, 33, 47, 48, 96, 100):
                T, first, n = sed.track_blocks(nf, W)
                got = sed.mvdr_frame_blocks(nf * hop, hop, W, T)
                for j, b in enumerate(got[:-1]):                             # (frame J's centre is the event's end)
                    f = j * B // hop
                    assert first[b] <= f < first[b] + n[b], (hop, W, nf, j)
                assert got[-1] == T - 1


# ───────────── 4. the reference ─────────────
def test_a_constant_track_is_the_untracked_reference_exactly():
    pos = doa_ref.tetrahedron(0.06)
    xs, xi, xn = mvdr_ref.scene(80 * B + 300, pos, 44100)
    x = xs + xi + xn
    tau = mvdr_track_ref.scene_tau(pos)
    for f32 in (False, True):
        for s0, length, W, hop, track in ((3 * B, 70 * B + 300, 1, 1024, [2, 2, 2]), (12 * B, 40 * B, 2, 441, [2]), (12 * B, 40 * B, 1, 1001, []),
                                          (5 * B, 33 * B, 1, 1024, [-1, 99])):
            want, (ws,) = mvdr_ref.event(x, s0, length, tau[2], 1e-2, f32, through=(xs,))
            got, (gs,) = mvdr_track_ref.event(x, s0, length, tau, track, 2, W, hop, 1e-2, f32=f32, through=(xs,))
            assert got.dtype == want.dtype and np.array_equal(got, want) and np.array_equal(gs, ws), (f32, s0, track)
    import mvdr_noise_ref
    want, _, used = mvdr_noise_ref.event(x, 12 * B, 40 * B, tau[2], 1e-2, 8, 1)
    got, _ = mvdr_track_ref.event(x, 12 * B, 40 * B, tau, [2, 2], 5, 1, 1024, 1e-2, noise_blocks=8, noise_guard=1)
    assert used == 8 and np.array_equal(got, want)
    moved, _ = mvdr_track_ref.event(x, 12 * B, 40 * B, tau, [2, 4], 2, 1, 1024, 1e-2)
    still, _ = mvdr_ref.event(x, 12 * B, 40 * B, tau[2], 1e-2)
    assert np.array_equal(moved[:31 * B], still[:31 * B]) and not np.array_equal(moved[31 * B:33 * B], still[31 * B:33 * B])   # the cross-fade


def test_the_beam_follows_a_moving_source():
    """the scene in float64 on the 6 cm array with the event's own frames; the bounds are the issue's, about 1.5 dB inside what
    the reference measures (module docstring)"""
    m = mvdr_track_ref.measure(0.06)
    one, trk = m["one"], m["tracked"]
    print({k: {a: round(b, 2) for a, b in v.items()} for k, v in m.items()})
    assert one["level_last"] < -6.0                                          # measured -8.34
    assert trk["level_last"] > -0.5                                          # -0.00
    assert trk["sir"] - one["sir"] >= 3.0                                    # 12.99 against 8.58
    assert trk["error"] < -20.0                                              # -28.12
    assert abs(one["level"] + 3.79) < 0.5 and abs(one["level_last"] + 8.34) < 0.5 and abs(trk["sir"] - 12.91) < 0.5 and abs(one["sir"] - 8.50) < 0.5
