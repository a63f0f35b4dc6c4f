"""GPU: every dropout-ON kernel against a float64 CPU reference that applies the kernel's OWN keep-mask.

The masks are counter-based (csrc/common.h pdf_uniform: a hash of host seed, device step counter and element index), so with the seed pinned a
probe on zeros and ones reads back the exact mask a site uses (tests/util.py probe_*), and the reference multiplies by mask / (1 - p) where the
reference network applies nn.Dropout.  That makes dropout-on parity as strict as dropout-off parity without restating the hash: the mask on
the wrong operand, a 1 / (1 - p) in the wrong place, a forward and a backward kernel that disagree on the index expression, or an index that
repeats across hands / samples / heads / rows all fail here.

  part 2  the recovered masks behave like Bernoulli(1 - p) masks (keep-rate, pairwise independence, determinism);
  part 3  F.dropout, F.dropout_add, F.layer_norm_fused, F.attention: values and all gradients against float64;
  part 4  a whole DualGraphLayer in train mode (unfused chain and the fused level in both arithmetic modes) against oracle.pdfnet_cpu in
          float64 with the twelve masks of the level queued into its nn.Dropout sites.

Tolerances of part 3 are the ones the dropout-off assertions of the same op use in tests/test_ops_gpu.py (absolute and relative part of its
`close`), divided by (1 - p): kept values and their gradients are scaled by 1 / (1 - p) and nothing else about the arithmetic changes.

`python -m tests.test_dropout_gpu MASKS.pt [SEEDS]` re-measures the CPU-side constants of part 4 (TAU, INPUT_SEED); it needs the GPU only while
MASKS.pt does not exist yet."""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from tests.util import (pinned_seeds, probe_attention_mask, probe_dropout_add_mask, probe_dropout_mask, probe_ln_fused_mask, recorded_seeds)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pdfnet_amd import functional as F
    return F


def dev(t):
    return t.cuda()


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uni(*shape, seed=0):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def close(a, b, atol, rtol=1e-5, what="", p=0.0):
    """tests/test_ops_gpu.py `close` with both parts of the bound divided by (1 - p)."""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs().max().item()
    lim = (atol + rtol * b.abs().max().item()) / (1 - p)
    print("%s: max err %.3e (limit %.3e, max|ref| %.3e)" % (what, err, lim, b.abs().max().item()))
    assert err <= lim, "%s: max err %.3e > %.3e (max|ref|=%.3e)" % (what, err, lim, b.abs().max().item())


# ----------------------------------------------------------------------------------------------
# part 2: the recovered masks behave like dropout masks
SEED_A, SEED_B = 0x1D2C3B4A59687706, 0x0123456789ABCDEF          # fixed: the checks are deterministic
EW_SHAPE = (2, 3, 63, 256)                                        # [hand, sample, V, Fd]
ATT = dict(nb=6, V=63, Fd=256, heads=4)                           # 2 hands x 3 samples stacked


def _keep_rate(m, p, what):
    n = m.numel()
    rate, sd = m.float().mean().item(), math.sqrt(p * (1 - p) / n)
    print("%s: kept %.5f of %d (expected %.2f, 5 sigma = %.5f)" % (what, rate, n, 1 - p, 5 * sd))
    assert abs(rate - (1 - p)) <= 5 * sd, (what, rate, 1 - p, sd)


def _independent(a, b, p, what):
    """Two independent Bernoulli(1 - p) masks agree in a fraction (1 - p)^2 + p^2.  Every pairing below is made of DISJOINT pairs of
    slices, so the agreement indicators are independent and the binomial deviation is exact."""
    assert a.shape == b.shape and a.numel() > 0
    n = a.numel()
    exp = (1 - p) ** 2 + p ** 2
    got, sd = (a == b).float().mean().item(), math.sqrt(exp * (1 - exp) / n)
    print("%s: agree in %.5f of %d (expected %.5f, 5 sigma = %.5f)" % (what, got, n, exp, 5 * sd))
    assert abs(got - exp) <= 5 * sd, (what, got, exp, sd)


def _probe(F, kind, p, seed, step=0):
    if kind == "dropout":
        return probe_dropout_mask(F, EW_SHAPE, p, seed, step)
    if kind == "dropout_add":
        return probe_dropout_add_mask(F, EW_SHAPE, p, seed, step)
    if kind == "ln_fused":
        return probe_ln_fused_mask(F, EW_SHAPE, p, seed, step)
    return probe_attention_mask(F, ATT["nb"], ATT["V"], ATT["Fd"], ATT["heads"], p, seed, step, kv_shift={"attn": 0, "attn_shift": 3}[kind])


@pytest.mark.parametrize("p", [0.05, 0.3])
@pytest.mark.parametrize("kind", ["dropout", "dropout_add", "ln_fused", "attn", "attn_shift"])
def test_recovered_masks_behave_like_dropout_masks(F, kind, p):
    dev0 = torch.device('cuda', torch.cuda.current_device())
    state0, step0 = F._seed_state[0], int(F.step_counter(dev0).item())
    m = _probe(F, kind, p, SEED_A)
    again = _probe(F, kind, p, SEED_A)
    other_seed = _probe(F, kind, p, SEED_B)
    other_step = _probe(F, kind, p, SEED_A, step=1)
    assert F._seed_state[0] == state0 and int(F.step_counter(dev0).item()) == step0, "the probes must leave the seed state and the step counter alone"
    assert torch.equal(m, again), "same seed, same step: the same mask"
    for name, t in (("seed A", m), ("seed B", other_seed), ("seed A, step 1", other_step)):
        _keep_rate(t, p, "%s p %.2f %s" % (kind, p, name))
    _independent(m, other_seed, p, "%s p %.2f: two seeds" % (kind, p))
    _independent(m, other_step, p, "%s p %.2f: step 0 / step 1" % (kind, p))
    if kind.startswith("attn"):                                   # [2 * 3 stacked samples, head, query, key]
        _independent(m[:3], m[3:], p, "%s p %.2f: hand 0 / hand 1" % (kind, p))
        _independent(m[0::2], m[1::2], p, "%s p %.2f: sample b / b + 1" % (kind, p))
        _independent(m[:, 0::2], m[:, 1::2], p, "%s p %.2f: head h / h + 1" % (kind, p))
        _independent(m[:, :, 0:62:2], m[:, :, 1:63:2], p, "%s p %.2f: query row i / i + 1" % (kind, p))
    else:                                                         # [hand, sample, V, Fd]
        _independent(m[0], m[1], p, "%s p %.2f: hand 0 / hand 1" % (kind, p))
        _independent(m[:, 0], m[:, 1], p, "%s p %.2f: sample 0 / 1" % (kind, p))
        _independent(m[:, 1], m[:, 2], p, "%s p %.2f: sample 1 / 2" % (kind, p))


# ----------------------------------------------------------------------------------------------
# part 3: op-level parity with the recovered mask
@pytest.mark.parametrize("p", [0.05, 0.3])
@pytest.mark.parametrize("n", [2 * 3 * 63 * 256, 1000003])       # the second: odd, and more than one pass of the grid
def test_dropout_and_dropout_add_against_float64_with_their_own_masks(F, n, p):
    """Inputs are uniform in (-1, 1), so |y| <= 1 + 1 / (1 - p) < 2.5: half an ulp there is 1.2e-7 and the fp32 rounding of the scale
    1 / (1 - p) adds 1e-7 relative, which leaves the issue's absolute 1e-6 well above rounding (at a normal tail of 5 / 0.7 it would not be)."""
    x, res, dy = uni(n, seed=1), uni(n, seed=2), uni(n, seed=3)
    # F.dropout
    m = probe_dropout_mask(F, (n,), p, SEED_A).double()
    xd = dev(x).requires_grad_()
    with pinned_seeds(F, [SEED_A]) as pin:
        y = F.dropout(xd, p, True)
        y.backward(dev(dy))
    assert pin.drawn == 1
    close(y, x.double() * m / (1 - p), 1e-6, rtol=0, what="dropout n %d p %.2f y" % (n, p))
    close(xd.grad, dy.double() * m / (1 - p), 1e-6, rtol=0, what="dropout n %d p %.2f dx" % (n, p))
    # F.dropout_add
    m = probe_dropout_add_mask(F, (n,), p, SEED_B).double()
    xd, rd = dev(x).requires_grad_(), dev(res).requires_grad_()
    with pinned_seeds(F, [SEED_B]) as pin:
        y = F.dropout_add(xd, rd, p, True)
        y.backward(dev(dy))
    assert pin.drawn == 1
    close(y, res.double() + x.double() * m / (1 - p), 1e-6, rtol=0, what="dropout_add n %d p %.2f y" % (n, p))
    close(xd.grad, dy.double() * m / (1 - p), 1e-6, rtol=0, what="dropout_add n %d p %.2f dx" % (n, p))
    assert torch.equal(rd.grad.cpu(), dy), "dropout_add: the residual's gradient is dy itself"


RELU_MARGIN = 1e-5


@pytest.mark.parametrize("p", [0.05, 0.3])
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("V,Fd", [(63, 256), (252, 64), (63, 96)])
def test_layer_norm_fused_with_dropout_against_float64_with_its_own_mask(F, V, Fd, act, p):
    """z = x + add * m / (1 - p), y_i = act(LN(z_i; gamma_i, beta_i)), loss = sum(z gz) + sum(y gy): z, y, dx, dadd, both dgamma, both dbeta."""
    shape = (2, 3, V, Fd)
    relu = act == "relu"
    x, a = rnd(*shape, seed=7), rnd(*shape, seed=8)
    gs = [rnd(Fd, seed=9 + i) for i in range(2)]
    be = [rnd(Fd, seed=11 + i) for i in range(2)]
    gz, gy = rnd(*shape, seed=13), rnd(*shape, seed=14)
    m = probe_ln_fused_mask(F, shape, p, SEED_A).double()

    def reference(x):
        xr, ar = x.double().requires_grad_(), a.double().requires_grad_()
        gr = [t.double().requires_grad_() for t in gs]
        er = [t.double().requires_grad_() for t in be]
        zr = xr + ar * m / (1 - p)
        pre = torch.stack([TF.layer_norm(zr[i], (Fd,), gr[i], er[i], 1e-6) for i in range(2)])
        return xr, ar, gr, er, zr, pre
    if relu:
        # no float64 pre-activation within RELU_MARGIN of zero: the offending inputs are nudged (found in the float64 reference alone), none excluded
        for it in range(20):
            with torch.no_grad():
                bad = reference(x)[5].abs() < RELU_MARGIN
            if not bad.any():
                break
            x = x + bad.float() * 1e-3 * (it + 1)
    xr, ar, gr, er, zr, pre = reference(x)
    if relu:
        assert float(pre.detach().abs().min()) >= RELU_MARGIN, "a ReLU pre-activation of the reference is within %.0e of zero" % RELU_MARGIN
    yr = TF.relu(pre) if relu else pre
    ((zr * gz.double()).sum() + (yr * gy.double()).sum()).backward()

    xd, ad = dev(x).requires_grad_(), dev(a).requires_grad_()
    gd = [dev(t).requires_grad_() for t in gs]
    ed = [dev(t).requires_grad_() for t in be]
    with pinned_seeds(F, [SEED_A]) as pin:
        zd, yd = F.layer_norm_fused(xd, gd[0], ed[0], 1e-6, F.ACT_RELU if relu else F.ACT_NONE, add=ad, p=p, training=True, gamma1=gd[1], beta1=ed[1])
        ((zd * dev(gz)).sum() + (yd * dev(gy)).sum()).backward()
        F.join_wgrad()
    assert pin.drawn == 1
    tag = "ln_fused V %d Fd %d %s p %.2f " % (V, Fd, act, p)
    close(zd, zr, 1e-6, what=tag + "z", p=p)
    close(yd, yr, 2e-5, what=tag + "y", p=p)
    close(xd.grad, xr.grad, 5e-5, what=tag + "dx", p=p)
    close(ad.grad, ar.grad, 5e-5, what=tag + "dadd", p=p)
    for i in range(2):
        close(gd[i].grad, gr[i].grad, 2e-4, rtol=2e-5, what=tag + "dgamma%d" % i, p=p)
        close(ed[i].grad, er[i].grad, 2e-4, rtol=2e-5, what=tag + "dbeta%d" % i, p=p)


# (stacked samples, V, Fd, heads, kv_shift)
ATTN_CASES = [
    (2, 63, 256, 4, 0),       # dh 64: the plain family, 16 lanes per row
    (2, 126, 128, 4, 0),      # dh 32: the *_keys family
    (2, 252, 64, 4, 0),       # dh 16: the *_keys family
    (2, 63, 16, 4, 0),        # dh 4
    (2, 300, 64, 4, 0),       # dh 16, two lanes per row; V outside 63 / 126 / 252: the last query tile is ragged.  (The *_keys backward would need
                              # 65.3 KB of LDS here: forward and backward take the plain family, csrc/graph.hip attn_keys_split)
    (1, 520, 16, 4, 0),       # dh 4, one lane per row: the plain family at a small head size
    (4, 63, 256, 4, 2),       # [2, B = 2, 63, 256] with kv_shift = B: sample b attends to the keys / values of sample (b + B) % 2B
    (4, 252, 64, 4, 2),
]


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("nb,V,Fd,heads,shift", ATTN_CASES)
def test_attention_with_dropout_against_the_float64_oracle_with_its_own_mask(F, nb, V, Fd, heads, shift, p):
    from oracle import pdfnet_cpu as O
    q, k, v, gy = (rnd(nb, V, Fd, seed=3 + i) for i in range(4))
    if p > 0:
        m = probe_attention_mask(F, nb, V, Fd, heads, p, SEED_A, kv_shift=shift).double()      # indexed by the QUERY's stacked sample
        _keep_rate(m.bool(), p, "attention mask %s" % ((nb, V, Fd, heads, shift),))            # (a probe that read nothing would show here)
    qr, kr, vr = (t.double().requires_grad_() for t in (q, k, v))
    if shift:
        B = shift
        drop = [(lambda a, s=s: a * m[s] / (1 - p)) if p > 0 else (lambda a: a) for s in (slice(0, B), slice(B, 2 * B))]
        ref = torch.cat((O.mha(qr[:B], kr[B:], vr[B:], heads, drop[0]), O.mha(qr[B:], kr[:B], vr[:B], heads, drop[1])))
    else:
        ref = O.mha(qr, kr, vr, heads, (lambda a: a * m / (1 - p)) if p > 0 else (lambda a: a))
    ref.backward(gy.double())
    qd, kd, vd = (dev(t).requires_grad_() for t in (q, k, v))
    with pinned_seeds(F, [SEED_A]) as pin:
        out = F.attention(qd, kd, vd, heads, p, True, shift)
        out.backward(dev(gy))
    assert pin.drawn == (1 if p > 0 else 0)
    tag = "attn %s p %.1f " % ((nb, V, Fd, heads, shift), p)
    close(out, ref, 2e-5, what=tag + "out", p=p)
    for name, u, w in (("dq", qd, qr), ("dk", kd, kr), ("dv", vd, vr)):
        close(u.grad, w.grad, 5e-5, rtol=2e-5, what=tag + name, p=p)


# ----------------------------------------------------------------------------------------------
# part 4: a whole DualGraphLayer with dropout on, against the float64 oracle
LAYER_B = 2
LAYER_CASES = [(0, 0.3), (1, 0.3), (2, 0.3), (2, 0.05)]
# TAU[level]: 8 x the largest |float32 - float64| of any ReLU pre-activation of the oracle layer (the norm2 outputs, the norm3 outputs that feed
# the inter-block ReLU, the fc1 outputs of the four MLP blocks) on the CPU, with the masks of the case, over input seeds 0..7; rounded upwards
# to two digits.  Measured largest differences: level 0 4.285e-06, level 1 3.476e-06, level 2 3.100e-06 (p = 0.3 and p = 0.05 alike).
TAU = {0: 3.6e-05, 1: 2.9e-05, 2: 2.6e-05}
# INPUT_SEED[(level, p)] = (seed of the input generator, the samples of the float64 reference that have a ReLU pre-activation with |z| < TAU).
# With ~0.6 M pre-activations per case and this TAU an input has 5 to 30 such elements, so no seed leaves none (searched from 0 on the
# CPU: every seed before the chosen one has them in BOTH samples); the seed is the first at which they all sit in ONE of the B = 2 samples.
# That sample's output gradient is zeroed for both hands, in the reference and in the GPU runs; the other sample and every parameter gradient
# stay on the bars.  Elements within TAU at the chosen seed: level 0 10, level 1 4, level 2 6 (p = 0.3), 8 (p = 0.05).
INPUT_SEED = {(0, 0.3): (19088, [1]), (1, 0.3): (464, [1]), (2, 0.3): (36, [0]), (2, 0.05): (533, [0])}


@pytest.fixture(params=["x3", "native"])
def mesh_arithmetic(request):
    """As in tests/test_meshdec_gpu.py: the fused levels' linear products as x3 arithmetic (the shipped default) and on the native fp32 MFMA."""
    from pdfnet_amd import functional as F
    F.set_x3(7 if request.param == "x3" else 3)
    assert F.mesh_x3() == (request.param == "x3")
    yield request.param
    F.set_x3(None)


class _MaskedDropout(nn.Module):
    """Stands where the oracle has an nn.Dropout: multiplies by the next queued keep-mask / (1 - p)."""

    def __init__(self, p, masks):
        super().__init__()
        self.p, self.queue = p, list(masks)

    def forward(self, a):
        assert self.queue, "an nn.Dropout of the oracle is called more often than the product draws masks for it"
        m = self.queue.pop(0)
        assert m.shape == a.shape, (tuple(m.shape), tuple(a.shape))
        return a * m.to(a.dtype) / (1 - self.p)


class _Unreached(nn.Module):
    def forward(self, a):
        raise AssertionError("an nn.Dropout of the oracle that the layer's forward should not reach was called")


def _dims(level):
    from oracle import synth
    return synth.DUALGRAPH_DIMS[level]


def _product_layer(level, p):
    from oracle import synth
    from pdfnet_amd.networks import intaghand_decoder as D
    V, cin, cout = _dims(level)
    gc = D.load_graph_constants()
    layer = D.DualGraphLayer(V, cin, cout, gc['ell_left'][level], gc['ell_right'][level], 4, [12, 24, 48][level], 256, (256, 128, 64)[level], 4, p)
    layer.load_state_dict(synth.det_state_dict(layer.state_dict(), salt=level + 1))
    return layer.cuda().train()


def _oracle_layer(level, p, masks, dtype):
    """oracle.pdfnet_cpu.DualGraphLayer in train mode with the twelve masks of one forward (the order the product draws them: four GCN
    blocks; self-attention probabilities, fc(a), MLP hidden, MLP output; the same four for the cross-hand attention) queued into its
    nn.Dropout sites.  Hand 0 feeds the left modules, hand 1 the right ones; the shared InterAttn.dropout1 / dropout2 are called twice, left
    queries (stacked samples 0..B-1) first.  -> (layer, [the _MaskedDropout modules], [hooked ReLU pre-activations, filled by a forward])."""
    from oracle import pdfnet_cpu as O
    from oracle import synth
    V, cin, cout = _dims(level)
    B = LAYER_B
    g = O.load_graph_constants()
    layer = O.DualGraphLayer(V, cin, cout, g['L_left'][level], g['L_right'][level], 4, [12, 24, 48][level], 256, 6, (256, 128, 64)[level], 4, p)
    layer.load_state_dict(synth.det_state_dict(layer.state_dict(), salt=level + 1))
    layer = layer.to(dtype).train()
    assert len(masks) == 12
    at = layer.attn
    sites = {}
    for i in range(4):
        sites[layer.graph_left.GCN_blocks[i], 'dropout'] = [masks[i][0]]
        sites[layer.graph_right.GCN_blocks[i], 'dropout'] = [masks[i][1]]
    for hand, sa in enumerate((at.L_self_attn_layer, at.R_self_attn_layer)):
        sites[sa, 'dropout1'] = [masks[4][hand * B:(hand + 1) * B]]
        sites[sa, 'dropout2'] = [masks[5][hand]]
        sites[sa.ff, 'dropout1'] = [masks[6][hand]]
        sites[sa.ff, 'dropout2'] = [masks[7][hand]]
    sites[at, 'dropout1'] = [masks[8][:B], masks[8][B:]]
    sites[at, 'dropout2'] = [masks[9][0], masks[9][1]]
    for hand, ff in enumerate((at.ffL, at.ffR)):
        sites[ff, 'dropout1'] = [masks[10][hand]]
        sites[ff, 'dropout2'] = [masks[11][hand]]
    queued = []
    for (mod, name), ms in sites.items():
        assert isinstance(getattr(mod, name), nn.Dropout)
        setattr(mod, name, _MaskedDropout(p, ms))
        queued.append(getattr(mod, name))
    for mod in list(layer.modules()):
        for name, child in list(mod.named_children()):
            if isinstance(child, nn.Dropout):
                setattr(mod, name, _Unreached())
    pre = []
    relu_inputs = [at.L_self_attn_layer.ff.fc1, at.R_self_attn_layer.ff.fc1, at.ffL.fc1, at.ffR.fc1]
    for graph in (layer.graph_left, layer.graph_right):
        for i, blk in enumerate(graph.GCN_blocks):
            relu_inputs.append(blk.norm2)
            if i != 3:
                relu_inputs.append(blk.norm3)
    for mod in relu_inputs:
        mod.register_forward_hook(lambda _m, _i, o: pre.append(o.detach()))
    return layer, queued, pre


def _oracle_run(level, p, masks, x, gy, dtype, tau=None, backward=True):
    """One forward (+ backward) of the oracle layer.  With `tau`: the samples that have a ReLU pre-activation with |z| < tau are found (from
    this run alone) and their output gradient is zeroed for both hands before the backward."""
    layer, queued, pre = _oracle_layer(level, p, masks, dtype)
    xr = x.to(dtype).clone().requires_grad_(backward)
    with torch.set_grad_enabled(backward):
        Lf, Rf = layer(xr[0], xr[1])
        out = torch.stack((Lf, Rf))
    assert all(not m.queue for m in queued), "the oracle did not consume every queued mask"
    assert len(pre) == 4 + 2 * 7
    res = dict(out=out.detach(), pre=pre, near=[])
    if tau is not None:
        near = torch.zeros(LAYER_B, dtype=torch.bool)
        for t in pre:
            near |= (t.abs() < tau).flatten(1).any(1)
        res['near'] = [int(b) for b in near.nonzero().flatten()]
    if backward:
        gy = gy.to(dtype).clone()
        for b in res['near']:
            gy[:, b] = 0
        out.backward(gy)
        res['dx'] = xr.grad
        res['grads'] = {n: q.grad for n, q in layer.named_parameters() if q.grad is not None}
    return res


def _layer_inputs(level, seed):
    V, cin, cout = _dims(level)
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(2, LAYER_B, V, cin, generator=g), torch.randn(2, LAYER_B, V, cout, generator=g)


def _forward(layer, x, fused):
    from pdfnet_amd import functional as F
    F.MESH_FUSED = fused
    try:
        if fused:
            assert F.mesh_level_ok(layer, x + layer.position_embeddings.weight), "the fused kernels must take the level"
        return layer(x)
    finally:
        F.MESH_FUSED = True


def _site_seeds_and_masks(F, level, p):
    """The twelve seeds one train forward of the level draws (recorded in a dry run of the unfused chain) and each site's keep-mask, probed at
    the site's own shape with the site's own seed."""
    V, cin, cout = _dims(level)
    B = LAYER_B
    layer = _product_layer(level, p)
    state = F._seed_state[0]
    F.manual_seed(4200 + level)
    try:
        with torch.no_grad(), recorded_seeds(F) as seeds:
            _forward(layer, dev(_layer_inputs(level, 0)[0]), fused=False)
        torch.cuda.synchronize()
    finally:
        F._seed_state[0] = state
    assert len(seeds) == 12 and len(set(seeds)) == 12, seeds
    shape = (2, B, V, cout)
    masks = [probe_ln_fused_mask(F, shape, p, s) for s in seeds[:4]]
    for s_att, s_z, s_t, s_x, shift in (tuple(seeds[4:8]) + (0,), tuple(seeds[8:12]) + (B,)):
        masks += [probe_attention_mask(F, 2 * B, V, cout, 4, p, s_att, kv_shift=shift), probe_ln_fused_mask(F, shape, p, s_z),
                  probe_dropout_mask(F, shape, p, s_t), probe_dropout_add_mask(F, shape, p, s_x)]
    return layer, seeds, masks


_CASES = {}


def _case(F, level, p):
    """Seeds, masks and the float64 reference of one (level, p): computed once, shared by the product paths, left unchanged."""
    if (level, p) not in _CASES:
        layer, seeds, masks = _site_seeds_and_masks(F, level, p)
        x, gy = _layer_inputs(level, INPUT_SEED[level, p][0])
        ref = _oracle_run(level, p, masks, x, gy, torch.float64, tau=TAU[level])
        _CASES[level, p] = (layer, seeds, masks, x, gy, ref)
    return _CASES[level, p]


@pytest.mark.parametrize("path", ["unfused", "fused"])
@pytest.mark.parametrize("level,p", LAYER_CASES)
def test_dualgraph_layer_with_dropout_equals_the_float64_oracle(F, mesh_arithmetic, level, p, path):
    """out, dx and every parameter gradient (whole tensors) of one DualGraphLayer in train mode, dropout p, on the bars of
    tests/test_dualgraph_golden_gpu.py::test_fused_level_train_forward_and_gradients_equal_the_reference_layer."""
    layer, seeds, masks, x, gy, ref = _case(F, level, p)
    # ReLU sign flips are handled from the reference alone: at the chosen input seed at most one of the B samples has a float64 pre-activation
    # within TAU of zero, and that sample's output gradient is zeroed (both hands, reference and GPU runs alike)
    near = ref['near']
    assert len(near) <= 1, "more than one sample has a ReLU pre-activation within TAU of zero: %s" % near
    assert near == INPUT_SEED[level, p][1], (near, INPUT_SEED[level, p])
    gy = gy.clone()
    for b in near:
        gy[:, b] = 0
    layer.zero_grad(set_to_none=True)
    xd = dev(x).requires_grad_()
    with pinned_seeds(F, seeds) as pin:
        out = _forward(layer, xd, fused=path == "fused")
        assert pin.drawn == 12, "the %s path drew %d seeds, not the 12 of the level" % (path, pin.drawn)
        out.backward(dev(gy))
        F.join_wgrad()
        torch.cuda.synchronize()
    tag = "level %d p %.2f %s/%s" % (level, p, path, mesh_arithmetic)
    ro, rdx = ref['out'], ref['dx']
    e_out = float((out.detach().cpu().double() - ro).abs().max())
    e_dx, top = float((xd.grad.cpu().double() - rdx).abs().max()), float(rdx.abs().max())
    print("%s: out max |diff| %.2e (max |ref| %.2f); dx max |diff| %.2e of max %.2e = %.1e; %d zeroed sample(s)"
          % (tag, e_out, float(ro.abs().max()), e_dx, top, e_dx / top, len(near)))
    mine = {n: q.grad.detach().cpu().double() for n, q in layer.named_parameters() if q.grad is not None}
    assert set(mine) == set(ref['grads']), set(mine) ^ set(ref['grads'])
    worst, bad = [], []
    for n, rg in ref['grads'].items():
        if n.endswith("w_ks.bias"):                           # zero in exact arithmetic (softmax is shift-invariant): rounding noise on both sides
            lim = 1e-4 * float(mine[n[:-4] + "weight"].abs().max()) + 1e-7
            if not float(mine[n].abs().max()) <= lim:
                bad.append((n, float(mine[n].abs().max()), lim))
            continue
        e_norm = abs(float(mine[n].norm()) / float(rg.norm()) - 1)
        e_el = float((mine[n] - rg).abs().max()) / (float(rg.abs().max()) + 1e-30)
        worst.append((max(e_norm, e_el), n))
        if not (e_norm <= 1e-3 and e_el <= 2e-3):
            bad.append((n, e_norm, e_el))
    worst.sort(reverse=True)
    print("%s: %d parameter gradients against the float64 oracle; worst %s" % (tag, len(mine), ["%s %.1e" % (n, e) for e, n in worst[:3]]))
    assert e_out <= 2e-5 * max(1.0, float(ro.abs().max())), e_out
    assert e_dx <= 2e-4 * top, (e_dx, top)
    assert not bad, bad


# ----------------------------------------------------------------------------------------------
def _measure(mask_file, n_seeds):
    """Re-measures TAU and INPUT_SEED.  The GPU is needed once, for the masks of the four cases (kept in `mask_file`, so that the search
    itself can run anywhere); everything else is the CPU oracle."""
    import os
    if not os.path.exists(mask_file):
        from pdfnet_amd import functional as F
        torch.save({c: _site_seeds_and_masks(F, *c)[2] for c in LAYER_CASES}, mask_file)
        print("masks of %s written to %s" % (LAYER_CASES, mask_file), flush=True)
    if n_seeds <= 0:
        return
    all_masks = torch.load(mask_file)
    tau = {}
    for level, p in LAYER_CASES:
        worst = 0.0
        for seed in range(8):
            x, gy = _layer_inputs(level, seed)
            r64 = _oracle_run(level, p, all_masks[level, p], x, gy, torch.float64, backward=False)
            r32 = _oracle_run(level, p, all_masks[level, p], x, gy, torch.float32, backward=False)
            worst = max(worst, max(float((a.double() - b).abs().max()) for a, b in zip(r32['pre'], r64['pre'])))
        print("level %d p %.2f: largest |float32 - float64| of a ReLU pre-activation over input seeds 0..7 = %.3e" % (level, p, worst), flush=True)
        tau[level] = max(tau.get(level, 0.0), float("%.1e" % (8 * worst * 1.05)))        # (rounded to two digits, upwards)
    print("TAU = %s" % tau, flush=True)
    for level, p in LAYER_CASES:
        for seed in range(n_seeds):
            x, gy = _layer_inputs(level, seed)
            r = _oracle_run(level, p, all_masks[level, p], x, gy, torch.float64, tau=tau[level], backward=False)
            if len(r['near']) <= 1:                           # (a seed with no such element at all would be taken here too)
                n_near = sum(int((t.abs() < tau[level]).sum()) for t in r['pre'])
                print("level %d p %.2f: input seed %d: %d element(s) within tau, all in sample(s) %s" % (level, p, seed, n_near, r['near']), flush=True)
                break
        else:
            print("level %d p %.2f: no seed below %d has its elements within tau in one sample" % (level, p, n_seeds), flush=True)


if __name__ == "__main__":
    import sys
    _measure(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 20000)
