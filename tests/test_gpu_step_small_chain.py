"""The small kernels the fit step keeps off its critical chain, at the smallest net the parity tests run (the C = 8 net of
g1_sed_c8.npz, two GRU layers): moving them changes no bit.

 a. one fit step with the auxiliary stream (head weight gradient and GRU bias-gradient reductions issued there) and without it
    (everything on one stream): bit-equal loss, parameters and gradients;
 b. FusedTrainStep(graph=True): the captured step replayed twice against the same launches issued eagerly;
 c. the public sed_gru_seq_fwd, which transposes W_hh for itself, against the plan's route, where the packing launch at the head
    of the forward wrote W_hh^T of every layer: bit-equal outputs at H = 8 and H = 128, B = 3, T' = 5;
 d. sed_net_forward_phases over two phase ranges (the second packs where it stands) against the whole forward."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd
    return sed_crnn_amd


@pytest.fixture(scope="module")
def g1():
    return load_golden("g1_sed_c8.npz")


def _net(sed, d):
    m = sed.TimePooledCRNN(conv_channels=8, dropout=0.0)
    assert len(m.gru_hidden) == 2
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in d.items() if k.startswith("sd.")})
    return m.cuda()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    n = int((a != b).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} words differ"


def _running(m):
    return torch.cat([v.float().flatten() for k, v in m.state_dict().items() if "running" in k])


def test_fit_step_with_and_without_the_auxiliary_stream(sed, g1):
    from sed_crnn_amd.trainer import FusedTrainStep
    x, y = torch.from_numpy(g1["x"]).cuda(), torch.from_numpy(g1["y"]).cuda()
    got = []
    for aux in (True, False):
        m = _net(sed, g1)
        m.overlap_wgrad = aux
        st = FusedTrainStep(m, lr=1e-3)
        loss, probs = st.step(x, y)
        torch.cuda.synchronize()
        got.append((loss.clone(), probs.clone(), m.flat_parameters().clone(), m.flat_grads().clone(), _running(m)))
    assert bool(torch.isfinite(got[0][3]).all()) and float(got[0][3].abs().max()) > 0
    for a, b, what in zip(got[0], got[1], ("loss", "probabilities", "parameters", "gradients", "running statistics")):
        _same(a, b, what)


def test_graph_replays_equal_the_same_steps_issued_eagerly(sed, g1):
    """call 1 of a graph trainer runs eagerly, call 2 captures and replays, call 3 replays: against three eager steps on the
    same device-side step state (the same kernels with the same arguments, so every bit must agree)"""
    from sed_crnn_amd.trainer import FusedTrainStep
    x, y = torch.from_numpy(g1["x"]).cuda(), torch.from_numpy(g1["y"]).cuda().float()
    mg, me = _net(sed, g1), _net(sed, g1)
    sg, se = FusedTrainStep(mg, lr=1e-3, graph=True), FusedTrainStep(me, lr=1e-3, graph=True)
    for k in range(3):
        lg, pg = sg.step(x, y)
        le, pe = se._step_eager(x, y, state=se._state)
        torch.cuda.synchronize()
        _same(lg, le, f"loss of step {k}")
        _same(pg, pe, f"probabilities of step {k}")
        _same(mg.flat_grads(), me.flat_grads(), f"gradients of step {k}")
        _same(mg.flat_parameters(), me.flat_parameters(), f"parameters after step {k}")
    assert isinstance(sg._graphs[(tuple(x.shape), tuple(y.shape))], tuple), "the step was never captured"
    _same(_running(mg), _running(me), "running statistics")


@pytest.mark.parametrize("H", [8, 128])
def test_public_gru_forward_equals_the_plans_prepacked_route(sed, H):
    from sed_crnn_amd import ops
    torch.manual_seed(H)
    m = sed.TimePooledCRNN(conv_channels=8, dropout=0.0, gru_hidden=H).cuda()
    x = torch.randn(3, 1, 40, 40, device="cuda")           # T' = 40 / 8 = 5
    m._run_forward(x, training=True)
    torch.cuda.synchronize()
    for i in range(2):
        gi = m.workspace_view("gi", i).clone().view(3, 5, 2, 3 * H)
        plan = m.workspace_view("gru_out", i).clone().view(3, 5, 2 * H)
        packed = m.workspace_view("gru_whh_t", i).clone().view(2, H, 3 * H)
        lay = [m.gru.layer(i, d) for d in range(2)]
        for d in range(2):
            _same(packed[d], lay[d][1].detach().t().contiguous(), f"layer {i} dir {d}: W_hh^T as the packing launch wrote it")
        out, _ = ops.gru_seq_fwd(gi, [lay[0][1].detach(), lay[1][1].detach()], [lay[0][3].detach(), lay[1][3].detach()], save=False)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(plan).all()) and float(plan.abs().max()) > 0
        _same(out, plan, f"H={H} layer {i}: sed_gru_seq_fwd against the plan's recurrence")


@pytest.mark.parametrize("split", [2, 6])
def test_forward_in_two_phase_ranges_equals_the_whole_forward(sed, g1, split):
    import sed_crnn_amd._lib as L
    m = _net(sed, g1)
    x = torch.from_numpy(g1["x"]).cuda()
    whole = m._run_forward(x, training=True).clone()
    torch.cuda.synchronize()
    names = [("pooled", l) for l in range(3)] + [("gru_out", i) for i in range(2)]
    keep = [m.workspace_view(n, i).clone() for n, i in names]
    cfg, ws, xin = m._last
    P, _ = m._param_structs()
    ws.fill_(float("nan"))
    logits = torch.full_like(whole, float("nan"))
    for pb, pe in ((0, split), (split, 7)):
        L.check(L.lib().sed_net_forward_phases(C.byref(cfg), C.byref(P), L.ptr(xin), L.ptr(logits), L.ptr(ws), 1, m._seed, pb, pe, 1.0,
                                               L.stream_ptr()), "sed_net_forward_phases")
    torch.cuda.synchronize()
    _same(logits, whole, f"logits, phases [0,{split}) + [{split},7)")
    for (n, i), ref in zip(names, keep):
        _same(m.workspace_view(n, i), ref, f"{n}[{i}]")
