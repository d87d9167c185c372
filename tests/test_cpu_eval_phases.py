"""The phased forward refuses an inference layout it cannot run, on the host and before anything is launched.  In the eval layout
the conv blocks that pool in their epilogue (or run in bf16) keep no conv output — their `conv_out` region is one 64-float granule —
while the phased path writes the whole B*T*F*C tensor there.  No GPU: the refusal is a host-side check, which is the point."""
import ctypes as C

import pytest


def _lib():
    from sed_crnn_amd import _lib
    return _lib


def _cfg2(training):
    import sed_crnn_amd as sed
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
    return m, m._cfg(128, 256, training=training)


def _dummy():
    """a host buffer standing in for a device pointer: the call must return before it touches any of them"""
    buf = (C.c_float * 64)()
    return buf, C.cast(buf, C.c_void_p)


@pytest.mark.parametrize("pb,pe", [(0, 1), (2, 3), (1, 7), (0, 6), (6, 7)])
def test_phased_inference_is_refused_where_a_block_keeps_no_conv_output(pb, pe):
    L = _lib()
    _, cfg = _cfg2(False)
    assert cfg.conv_mode == 0 and cfg.n_conv == 3
    # the layout of this config: blocks 1 and 2 pool in the conv epilogue (no `conv_out` region)
    off, n = C.c_size_t(), C.c_size_t()
    for l in (1, 2):
        assert L.lib().sed_net_workspace_region(C.byref(cfg), 0, b"conv_out", l, C.byref(off), C.byref(n)) < 0
    keep = [_dummy() for _ in range(3)]
    x, logits, ws = (p for _, p in keep)
    rc = L.lib().sed_net_forward_phases(C.byref(cfg), C.byref(L.NetParams()), x, logits, ws, 0, 0, pb, pe, 1.0, None)
    msg = L.lib().sed_last_error_string()
    assert rc < 0 and b"phases" in msg and f"[{pb},{pe})".encode() in msg and b"launch" not in msg, (rc, msg)
    assert all(v == 0.0 for buf, _ in keep for v in buf)


def test_whole_inference_and_phased_training_are_still_accepted():
    L = _lib()
    m, cfg = _cfg2(False)
    n = cfg.n_conv
    assert L.lib().sed_net_workspace_bytes(C.byref(cfg), 0) > 0
    assert m.inference_plan(128, 256) == {"conv": ["f32"] * 3, "proj": "f32"}
    keep = [_dummy() for _ in range(3)]
    x, logits, ws = (p for _, p in keep)
    # the whole range passes the guard: with empty parameters it stops at the next host check, the missing conv parameters
    rc = L.lib().sed_net_forward_phases(C.byref(cfg), C.byref(L.NetParams()), x, logits, ws, 0, 0, 0, 2 * n + 1, 1.0, None)
    msg = L.lib().sed_last_error_string()
    assert rc < 0 and b"missing parameters of conv block 0" in msg, (rc, msg)
    # a training layout has no such block: a partial range reaches the same check
    _, tcfg = _cfg2(True)
    assert L.lib().sed_net_workspace_bytes(C.byref(tcfg), 1) > L.lib().sed_net_workspace_bytes(C.byref(cfg), 0)
    rc = L.lib().sed_net_forward_phases(C.byref(tcfg), C.byref(L.NetParams()), x, logits, ws, 1, 0, 2, 3, 1.0, None)
    msg = L.lib().sed_last_error_string()
    assert rc < 0 and b"missing parameters of conv block 1" in msg, (rc, msg)
    # a bad range is still named as such
    rc = L.lib().sed_net_forward_phases(C.byref(cfg), C.byref(L.NetParams()), x, logits, ws, 0, 0, 3, 3, 1.0, None)
    assert rc < 0 and b"bad phase range" in L.lib().sed_last_error_string()
