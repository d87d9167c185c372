"""The bf16 inference plan without a GPU: the host library's acceptance / refusal of conv_mode 2, the Python setting, and the
CPU emulation the GPU tests measure against (with rounding disabled it must be the float64 reference itself)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_emul as emu  # noqa: E402


def _lib():
    from sed_crnn_amd import _lib
    return _lib


def test_host_accepts_mode_2_for_eval_and_refuses_it_for_training():
    import sed_crnn_amd as sed
    L = _lib()
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
    cfg = m._cfg(128, 256)
    cfg.conv_mode = 2
    ev = L.lib().sed_net_workspace_bytes(C.byref(cfg), 0)
    assert ev > 0
    cfg.conv_mode = 0
    assert ev < L.lib().sed_net_workspace_bytes(C.byref(cfg), 0)          # bf16 weights / activations take half the bytes
    cfg.conv_mode = 2
    assert L.lib().sed_net_workspace_bytes(C.byref(cfg), 1) == 0
    assert b"eval-only" in L.lib().sed_last_error_string()
    rc = L.lib().sed_net_forward_phases(C.byref(cfg), C.byref(L.NetParams()), None, None, None, 0, 0, 0, 1, 1.0, None)
    assert rc < 0 and b"phases" in L.lib().sed_last_error_string()
    cfg.conv_mode = 3
    assert L.lib().sed_net_workspace_bytes(C.byref(cfg), 0) == 0
    assert b"conv_mode" in L.lib().sed_last_error_string()


def test_inference_plan_reports_what_runs_in_bf16():
    import sed_crnn_amd as sed
    m = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, gru_hidden=128)
    assert m.inference_plan(128, 256) == {"conv": ["f32"] * 3, "proj": "f32"}
    m.set_inference_precision("bf16")
    assert m.inference_plan(128, 256) == {"conv": ["f32", "bf16", "bf16"], "proj": "bf16"}
    assert m._cfg(128, 256).conv_mode == 0                                # training keeps its own mode
    assert m._cfg(128, 256, training=False).conv_mode == 2
    m5 = sed.TimePooledCRNN(conv_channels=128, dropout=0.5, in_channels=4, n_mels=128, gru_hidden=256).set_inference_precision("bf16")
    assert m5.inference_plan(2, 512) == {"conv": ["f32", "bf16", "bf16"], "proj": "bf16"}
    lt = sed.LightningTimePooledCRNN().set_inference_precision("bf16")      # 16-channel blocks: nothing qualifies
    assert lt.inference_plan(4, 64) == {"conv": ["f32"] * 3, "proj": "f32"}
    m.set_inference_precision("f32")
    assert m.inference_plan(128, 256) == {"conv": ["f32"] * 3, "proj": "f32"}


def test_set_inference_precision_rejects_unknown_names_and_stays_out_of_the_state_dict():
    import sed_crnn_amd as sed
    from oracle import crnn_ref
    m = sed.TimePooledCRNN(conv_channels=32, dropout=0.0, gru_hidden=32)
    for bad in ("fp16", "bf16x3", "f64", "", None):
        with pytest.raises(ValueError):
            m.set_inference_precision(bad)
    sd0 = m.state_dict()
    m.set_inference_precision("bf16")
    sd1 = m.state_dict()
    assert list(sd0) == list(sd1)
    crnn_ref.SedNetRef(conv_channels=32, dropout=0.0, gru_hidden=32).load_state_dict(sd1)


def test_kernel_level_entries_answer_without_a_gpu():
    L = _lib().lib()
    assert L.sed_conv3x3_bf16_eval_supported(128, 128, 40, 128, 128) == 1
    assert L.sed_conv3x3_bf16_eval_supported(2, 64, 37, 5, 64) == 1
    assert L.sed_conv3x3_bf16_eval_supported(2, 16, 40, 8, 16) == 0      # Cin % 32
    assert L.sed_conv3x3_bf16_eval_supported(2, 128, 40, 8, 96) == 0     # Cout % 64
    assert L.sed_conv3x3_bf16_eval_supported(2, 128, 40, 1, 128) == 0    # no time pair
    rc = L.sed_gemm_bf16_nt(1, 1, None, 1, 64, 4, 64, 48, None)           # K % 32
    assert rc < 0 and b"K % 32" in L.sed_last_error_string()
    rc = L.sed_conv3x3_bf16_bn_relu_pool_eval(None, 0, None, None, None, 1, 128, 40, 8, 128, None)
    assert rc < 0 and b"null pointer" in L.sed_last_error_string()


@pytest.mark.parametrize("which", ["sed", "lightning"])
def test_emulation_without_rounding_is_the_float64_reference(which):
    from oracle import crnn_ref
    torch.manual_seed(0)
    if which == "sed":
        ref = crnn_ref.SedNetRef(conv_channels=32, dropout=0.5, gru_hidden=16)
    else:
        ref = crnn_ref.LightningNetRef()
    ref.load_state_dict(crnn_ref.rs_state_dict(ref, 7))
    ref = ref.double().eval()
    x = torch.randn(3, 1, 40, 27, dtype=torch.float64)
    plan = {"conv": ["f32", "bf16", "bf16"], "proj": "bf16"}
    _, lg = emu.forward(ref, x, plan, rnd=False)
    with torch.no_grad():
        want = ref(x)
    assert (lg - want).abs().max().item() < 1e-12


def test_emulation_rounds_exactly_at_the_three_points():
    """rounding on: the first block (fp32) is untouched, the bf16 blocks move by bf16-sized amounts"""
    from oracle import crnn_ref
    ref = crnn_ref.SedNetRef(conv_channels=32, dropout=0.5, gru_hidden=16)
    ref.load_state_dict(crnn_ref.rs_state_dict(ref, 3))
    ref.eval()
    x = torch.randn(2, 1, 40, 16, dtype=torch.float64)
    plan = {"conv": ["f32", "bf16", "bf16"], "proj": "bf16"}
    p_r, lg_r = emu.forward(ref, x, plan)
    p_e, lg_e = emu.forward(ref, x, plan, rnd=False)
    assert torch.equal(p_r[0], p_e[0])
    d1 = (p_r[1] - p_e[1]).abs().max().item() / p_e[1].abs().max().item()
    assert 1e-5 < d1 < 3e-2
    assert 0 < (lg_r - lg_e).abs().max().item() < 0.1
    assert torch.equal(emu.bf16(torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)), torch.tensor([1.0], dtype=torch.float64))  # ties to even
