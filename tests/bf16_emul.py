"""CPU float64 restatement of the eval forward of SedNetRef / LightningNetRef that rounds to bf16 (round to nearest even)
exactly where the bf16 inference plan does, and nowhere else:
  1. the BatchNorm-folded conv weights of a bf16 block (s = gamma / sqrt(var + eps) and w * s in fp32, then bf16),
  2. the input of a bf16 block,
  3. both operands of the GRU layer-0 input projection (when the plan runs it in bf16).
Everything else (fold of the fp32 blocks, bias, ReLU, pool, recurrences, head) is float64.  Used by the bf16 tests only."""
import torch
import torch.nn.functional as F

from oracle import crnn_ref


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def folded(conv, bn, rnd):
    """(w', b') of one block: rnd -> w' in fp32 then bf16 (rule 1); else float64 throughout.  b' is float64 either way."""
    w, b = conv.weight.detach(), conv.bias.detach()
    g, be, rm, rv, eps = bn.weight.detach(), bn.bias.detach(), bn.running_mean.detach(), bn.running_var.detach(), bn.eps
    if rnd:
        s32 = g.float() / torch.sqrt(rv.float() + eps)
        wf = bf16(w.float() * s32.view(-1, 1, 1, 1))
    else:
        wf = w.double() * (g.double() / torch.sqrt(rv.double() + eps)).view(-1, 1, 1, 1)
    s = g.double() / torch.sqrt(rv.double() + eps)
    bf = (b.double() - rm.double()) * s + be.double()
    return wf, bf


def blocks(model):
    bl, _, _ = crnn_ref._blocks(model)
    return bl


def block(model, l, x, bf, rnd=True):
    """block l on x [B,C,F,T] (float64): relu(pool(conv(x; w') + b')); bf: the block runs bf16 (x and w' rounded)"""
    conv, bn, (pf, pt) = blocks(model)[l]
    w, b = folded(conv, bn, bf and rnd)
    if bf and rnd:
        x = bf16(x)
    return torch.relu(F.max_pool2d(F.conv2d(x.double(), w, b, padding=1), (pf, pt)))


def block_floor(model, l, x, bf):
    """K 2^-23 (|w'| * |x| + |b'|) pooled like the output (an upper bound over the pooling window): the fp32 accumulation floor.
    One fp32 ulp (2^-23) per addition rather than half of one: the matrix cores' internal sums are not bound to round to nearest
    (one element of config 5 measured at 1.03x the 2^-24 form)."""
    conv, bn, (pf, pt) = blocks(model)[l]
    w, b = folded(conv, bn, bf)
    if bf:
        x = bf16(x)
    K = 9 * w.shape[1]
    a = F.conv2d(x.float().abs(), w.float().abs(), b.float().abs(), padding=1)
    return (K * 2.0 ** -23) * F.max_pool2d(a, (pf, pt)).double()


def gru_layers(model):
    if hasattr(model, "gru"):
        g = model.gru
        return [[tuple(getattr(g, f"{n}_l{i}{sfx}").detach().double() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                 for sfx in ("", "_reverse")] for i in range(g.num_layers)]
    out = []
    for g in (model.gru1, model.gru2):
        out.append([tuple(getattr(g, f"{n}_l0{sfx}").detach().double() for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                    for sfx in ("", "_reverse")])
    return out


def _recur(gi, whh, bhh, reverse):
    B, T, H3 = gi.shape
    H = H3 // 3
    h = torch.zeros(B, H, dtype=torch.float64)
    out = torch.empty(B, T, H, dtype=torch.float64)
    steps = range(T - 1, -1, -1) if reverse else range(T)
    for t in steps:
        gh = h @ whh.t() + bhh
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        out[:, t] = h
    return out


def head(model, pooled, proj_bf, rnd=True):
    """GRU stack + dense head on the last block's output pooled [B,C,F',T'] (float64); proj_bf: layer 0's projection in bf16"""
    b, c, f, t = pooled.shape
    x = pooled.double().permute(0, 3, 1, 2).reshape(b, t, c * f)
    for i, dirs in enumerate(gru_layers(model)):
        outs = []
        for d, (wih, whh, bih, bhh) in enumerate(dirs):
            if i == 0 and proj_bf and rnd:
                gi = bf16(x) @ bf16(wih.float()).t() + bih
            else:
                gi = x @ wih.t() + bih
            outs.append(_recur(gi, whh, bhh, d == 1))
        x = torch.cat(outs, -1)
    if hasattr(model, "fc"):
        return x @ model.fc.weight.detach().double().t() + model.fc.bias.detach().double()
    y = torch.relu(x @ model.d1.weight.detach().double().t() + model.d1.bias.detach().double())
    return y @ model.d2.weight.detach().double().t() + model.d2.bias.detach().double()


def forward(model, x, plan, rnd=True):
    """the whole eval forward; plan = model.inference_plan() of the HIP model ({"conv": [...], "proj": ...}).
    Returns (pooled outputs per block [B,C,F,T] float64, logits float64)."""
    pooled = []
    h = x.double()
    for l in range(len(blocks(model))):
        h = block(model, l, h, plan["conv"][l] == "bf16", rnd)
        pooled.append(h)
    return pooled, head(model, h, plan["proj"] == "bf16", rnd)


def bf16_ulp(v):
    """one bf16 ulp of |v| (8 significant bits); the smallest normal's ulp at 0"""
    a = v.abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 7)
