"""Layout arithmetic of the whole-network plan's per-layer GRU scratch (host only, no GPU): every GRU layer has its own
W_hh^T region ("gru_whh_t", 2 * 3H * H floats: all of them are written by the one packing launch at the head of a training
forward) and, in training, its own bias-gradient partial region ("gru_bias_part": the auxiliary stream reduces layer i's while the
recurrence of layer i-1 writes its own).  The regions lie inside the workspace and overlap neither each other nor the tensors
the recurrences read and write."""
import ctypes as C

import pytest


def _model(H, layers):
    import sed_crnn_amd as sed
    return sed.TimePooledCRNN(conv_channels=8, dropout=0.0, gru_hidden=H, gru_layers=layers)


def _region(cfg, training, name, i):
    import sed_crnn_amd._lib as L
    off, n = C.c_size_t(), C.c_size_t()
    rc = L.lib().sed_net_workspace_region(C.byref(cfg), int(training), name.encode(), i, C.byref(off), C.byref(n))
    assert rc == 0, (name, i, L.lib().sed_last_error_string())
    assert off.value % 256 == 0, f"{name}[{i}] is not on a 256-byte granule"
    return off.value // 4, n.value


@pytest.mark.parametrize("H,layers,B,T", [(8, 2, 3, 40), (32, 3, 4, 64), (128, 2, 128, 256), (128, 4, 300, 64)])
def test_per_layer_gru_regions_are_disjoint_and_inside_the_workspace(H, layers, B, T):
    import sed_crnn_amd._lib as L
    m = _model(H, layers)
    for training in (0, 1):
        cfg = m._cfg(B, T, training=bool(training))
        total = L.lib().sed_net_workspace_bytes(C.byref(cfg), training) // 4
        assert total > 0
        regions = []
        for i in range(layers):
            off, n = _region(cfg, training, "gru_whh_t", i)
            assert n == 2 * 3 * H * H == L.lib().sed_gru_seq_workspace_bytes(H) // 4
            regions.append((f"gru_whh_t[{i}]", off, n))
            for name in ("gi", "gru_out") + (("dgru_out",) if training else ()):
                regions.append((f"{name}[{i}]",) + _region(cfg, training, name, i))
            if training:
                off, n = _region(cfg, training, "gru_bias_part", i)
                assert n == L.lib().sed_gru_seq_bwd_workspace_bytes(B, H) // 4 and n >= 2 * 4 * H
                regions.append((f"gru_bias_part[{i}]", off, n))
        if not training:      # no backward scratch in an inference layout
            off, n = C.c_size_t(), C.c_size_t()
            assert L.lib().sed_net_workspace_region(C.byref(cfg), 0, b"gru_bias_part", 0, C.byref(off), C.byref(n)) < 0
        regions.sort(key=lambda r: r[1])
        for (na, oa, la), (nb, ob, _) in zip(regions, regions[1:]):
            assert oa + la <= ob, f"{na} [{oa}, {oa + la}) overlaps {nb} at {ob} (training={training})"
        name, off, n = regions[-1]
        assert off + n <= total, f"{name} ends at {off + n}, the workspace holds {total} floats"


def test_workspace_grows_by_exactly_the_extra_per_layer_regions():
    """two layers against one: the second layer adds its own gi / gru_out / saved / gradient tensors AND its own packed-W_hh and
    bias-partial regions (one shared region per kind would leave the size of those two unchanged)"""
    import sed_crnn_amd._lib as L
    H, B, T = 32, 4, 64
    g = lambda v: (v + 63) // 64 * 64          # the carver's 256-byte granules, in floats
    M = B * (T // 8)
    size = {}
    for layers in (1, 2):
        cfg = _model(H, layers)._cfg(B, T, training=True)
        size[layers] = L.lib().sed_net_workspace_bytes(C.byref(cfg), 1) // 4
    per_layer = g(M * 6 * H) + g(M * 2 * H) + g(M * 10 * H) + 2 * g(M * 6 * H) + g(M * 2 * H)      # gi, out, saved, dgi, dgh, dgout
    own = g(6 * H * H) + g(L.lib().sed_gru_seq_bwd_workspace_bytes(B, H) // 4)
    grown = size[2] - size[1]
    # (the split-K scratch of the GEMMs is a maximum over the layers and may grow too: bounded, not pinned)
    assert grown >= per_layer + own, (grown, per_layer, own)
