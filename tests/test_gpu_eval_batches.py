"""The whole eval forward at the batch sizes the detector and the live streams run it at (chunks of max_batch = 1024 windows),
where the GRU recurrence leaves its one-row batch tile: B = 255 (tile 1), 256, 257 (tile 2, even and ragged), 512, 513 (tile 4
for H < 128, even and ragged) and 1024.  Three nets on 64-frame windows: the Lightning net (H = 16 and 8: register-resident
tiles 1, 2, 4), the 128-channel net with two BiGRU layers of 128 (<128, 1|2>) and a small 4-channel / 128-mel net with H = 256
(the hybrid at B = 255, the streamed <0, 2> above).

The float64 oracle is per sample, so it runs on about 48 sampled rows per batch size: the first and last rows, the rows on
both sides of every multiple of 128 and of the tile thresholds, and a fixed random set.  Asserted per batch size: probabilities
within the 1e-3 of test_cfg2_eval_..., the relative L2 error of the sampled logits within 3x torch-float32's own error against
float64 plus 2e-6 (the form of test_single_step_gradients_are_as_close_to_float64_as_torch_float32), and that a row's logits do
not depend on the batch it ran in (bitwise against the B = 1024 run: at these sizes every batch takes the same GEMM plan)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHES = (255, 256, 257, 512, 513, 1024)
N_ROWS = 48


@pytest.fixture(scope="module")
def sed():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import sed_crnn_amd as s
    return s


def sampled_rows(B, n=N_ROWS):
    """first and last rows, both sides of every multiple of 128 (256 and 512 are the tile thresholds), then a fixed random fill"""
    rows = {0, 1, 2, 3, B - 4, B - 3, B - 2, B - 1}
    for edge in range(128, B + 1, 128):
        rows |= {edge - 2, edge - 1, edge, edge + 1}
    rows = {r for r in rows if 0 <= r < B}
    for r in np.random.default_rng(20).permutation(1024):
        if len(rows) >= n:
            break
        if r < B:
            rows.add(int(r))
    return sorted(rows)


def _build(sed, which):
    from oracle import crnn_ref
    if which == "lightning":
        r, m = crnn_ref.LightningNetRef(dropout=0.0), sed.LightningTimePooledCRNN(dropout=0.0)
        shape = (1, 40)
    elif which == "timepooled128":
        kw = dict(conv_channels=128, dropout=0.0, gru_hidden=128)
        r, m, shape = crnn_ref.SedNetRef(**kw), sed.TimePooledCRNN(**kw), (1, 40)
    else:                                                       # config-5-like, small: 4 channels, 128 mel, BiGRU 2 x 256
        kw = dict(conv_channels=16, dropout=0.0, in_channels=4, n_mels=128, gru_hidden=256)
        r, m, shape = crnn_ref.SedNetRef(**kw), sed.TimePooledCRNN(**kw), (4, 128)
    sd = crnn_ref.rs_state_dict(r, 31)                         # running statistics away from 0 / 1
    r.load_state_dict(sd)
    m.load_state_dict(sd)
    return r.eval(), m.cuda().eval(), shape


@pytest.mark.parametrize("which", ["lightning", "timepooled128", "cfg5_small_h256"])
def test_eval_forward_at_detector_batch_sizes_vs_float64_oracle(sed, which):
    import copy
    r32, m, (cin, mel) = _build(sed, which)
    r64 = copy.deepcopy(r32).double()
    x = torch.randn(max(BATCHES), cin, mel, 64, generator=torch.Generator().manual_seed(7))
    xg = x.cuda()
    rows_of = {B: sampled_rows(B) for B in BATCHES}
    union = sorted(set().union(*rows_of.values()))
    at = {row: i for i, row in enumerate(union)}
    with torch.no_grad():
        l64 = torch.cat([r64(x[union[i:i + 32]].double()) for i in range(0, len(union), 32)])
        l32 = torch.cat([r32(x[union[i:i + 32]]) for i in range(0, len(union), 32)]).double()
        hip = {B: m(xg[:B]).cpu() for B in BATCHES}
    fails = []
    for B in BATCHES:
        rows = rows_of[B]
        assert len(rows) >= N_ROWS and rows[0] == 0 and rows[-1] == B - 1
        idx = [at[row] for row in rows]
        want, t32, got = l64[idx], l32[idx], hip[B][rows].double()
        assert hip[B].shape == (B, 8, l64.shape[2])
        dp = (torch.sigmoid(got) - torch.sigmoid(want)).abs().max().item()
        den = want.norm().item()
        e_h, e_t = (got - want).norm().item() / den, (t32 - want).norm().item() / den
        same = torch.equal(hip[B], hip[max(BATCHES)][:B])
        print(f"eval {which} B={B}: {len(rows)} rows vs float64: max |dp| {dp:.2e}; logit rel L2 hip {e_h:.2e} torch-f32 {e_t:.2e} "
              f"ratio {e_h / (e_t + 1e-300):.2f} bound use {e_h / (3.0 * e_t + 2e-6):.2f}; rows bitwise those of the B=1024 run: {same}")
        if not dp <= 1e-3:
            fails.append(f"B={B}: max |dp| {dp:.3e} > 1e-3")
        if not e_h <= 3.0 * e_t + 2e-6:
            fails.append(f"B={B}: logit rel L2 {e_h:.3e} > 3 * {e_t:.3e} + 2e-6")
        if not same:
            d = (hip[B] - hip[max(BATCHES)][:B]).abs().reshape(B, -1).max(1).values
            fails.append(f"B={B}: {int((d > 0).sum())} rows differ from the B=1024 run (first {d.nonzero().flatten()[:6].tolist()}, max {d.max().item():.2e})")
    assert not fails, which + ":\n  " + "\n  ".join(fails)


def test_sampled_rows_sit_on_the_tile_boundaries():
    for B in BATCHES:
        rows = sampled_rows(B)
        assert N_ROWS <= len(rows) <= N_ROWS + 24 and {0, B - 1} <= set(rows)
        for edge in (128, 256, 512, 1024):
            if edge < B:
                assert {edge - 1, edge} <= set(rows)
