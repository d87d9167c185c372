"""The entries over an event table live in ``sed_crnn_amd.events``; ``sed_crnn_amd.feature`` keeps their names."""
import inspect
import os
import subprocess
import sys

from sed_crnn_amd import events, feature

PUBLIC = ("event_tdoa", "event_tdoa_ring", "event_doa", "event_doa_ring", "event_beamform", "event_beamform_ring", "event_mvdr",
          "event_mvdr_ring", "ring_write")


def test_feature_reexports_the_same_objects():
    for name in PUBLIC:
        assert getattr(feature, name) is getattr(events, name), name


def test_tdoa_signatures_have_no_private_parameter():
    for fn in (events.event_tdoa, events.event_tdoa_ring):
        assert not [p for p in inspect.signature(fn).parameters if p.startswith("_")], fn.__name__


def test_events_imports_first_in_a_fresh_interpreter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", "import sed_crnn_amd.events as e; assert e.event_tdoa.__module__ == 'sed_crnn_amd.events'"],
                       capture_output=True, text=True, cwd=root, timeout=120)
    assert r.returncode == 0, r.stderr
