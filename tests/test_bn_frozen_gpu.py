"""BatchNorm backward with FROZEN statistics (eval mode under autograd): pdf_bn_eval_bwd / pdf_bn_relu_maxk_eval_bwd through
F.batch_norm / F.bn_relu_max_over_k and called directly, against torch autograd in float64 on the CPU; then the whole model in
.eval() and in .train() with layers.freeze_batchnorm against the float64 oracle's gradients.

The float64 references take their ReLU mask (and the arg-max of the pooled form) from the HIP forward's own output, so no element
is excluded and a pre-activation within rounding of zero cannot decide a comparison; the forward itself is held to 2e-5."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.util import make_opt, ROOT

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pdfnet_amd import functional as F
    return F


def close(a, b, atol, rtol=1e-5, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    print("%-40s max err %.3e (limit %.3e)" % (what, err, lim))
    assert err <= lim, "%s: max err %.3e > %.3e (max|ref|=%.3e)" % (what, err, lim, b.abs().max().item())


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _params(C, seed=2):
    """gamma with one exactly-zero and some negative channels, running_var in [0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::5] *= -1.0
    gamma[1] = 0.0
    return gamma, rnd(C, seed=seed + 1) * 0.5, rnd(C, seed=seed + 2), torch.rand(C, generator=g) * 0.999 + 0.5


def _cuda_like(x):
    return x.cuda().contiguous(memory_format=torch.channels_last) if x.dim() == 4 else x.cuda()


# (4, 64, 7, 7): float4 kernels, R = 196 rows = several row chunks; (3, 6, 5, 5): C % 4 != 0, the scalar pair; (20000, 64): 313 chunks of 64 rows,
# the row rule of the chunk count
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(4, 64, 7, 7), (3, 6, 5, 5), (20000, 64)])
def test_batch_norm_eval_backward(F, shape, relu, res):
    C = shape[1]
    x = rnd(*shape, seed=1) * 2 + 0.5
    r = rnd(*shape, seed=5) if res else None
    gamma, beta, rm, rv = _params(C)
    gy = rnd(*shape, seed=4)

    def hip_inputs(params_grad=True):
        xd = _cuda_like(x).requires_grad_()
        gd, bd = gamma.cuda().requires_grad_(params_grad), beta.cuda().requires_grad_(params_grad)
        rd = _cuda_like(r).requires_grad_() if res else None
        return xd, gd, bd, rd

    xd, gd, bd, rd = hip_inputs()
    rmd, rvd = rm.cuda(), rv.cuda()
    out = F.batch_norm(xd, gd, bd, rmd, rvd, False, 0.1, EPS, relu, rd)
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    # ---- float64 reference; the ReLU mask is the HIP forward's
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    r64 = r.double().requires_grad_() if res else None
    pre = TF.batch_norm(x64, rm.double(), rv.double(), g64, b64, False, 0.1, EPS)
    if res:
        pre = pre + r64
    close(out, TF.relu(pre) if relu else pre, 2e-5, what="bn eval fwd")
    ref = pre * (out.detach().cpu() > 0).double() if relu else pre
    ref.backward(gy.double())
    # ---- the backward, twice: bit-identical
    ins = (xd, gd, bd) + ((rd,) if res else ())
    gyd = _cuda_like(gy)
    g1 = torch.autograd.grad(out, ins, gyd, retain_graph=True)
    g2 = torch.autograd.grad(out, ins, gyd, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    close(g1[0], x64.grad, 5e-5, rtol=5e-5, what="bn eval dx")
    close(g1[1], g64.grad, 2e-4, rtol=5e-5, what="bn eval dgamma")
    close(g1[2], b64.grad, 2e-4, rtol=5e-5, what="bn eval dbeta")
    assert float(g64.grad[1].abs()) > 1e-3                    # the gamma == 0 channel has a real dgamma
    if res:
        close(g1[3], r64.grad, 1e-6, what="bn eval dres")
    # ---- direct accumulation into the trainer's gradient buffers (_main_grad): pre-fill + the returned gradient, to the bit
    gd._pdf_main_grad = bd._pdf_main_grad = True
    gd.grad, bd.grad = torch.full_like(g1[1], 0.75), torch.full_like(g1[2], -1.5)
    pg, pb = gd.grad.clone(), bd.grad.clone()
    got = torch.autograd.grad(out, ins, gyd, retain_graph=True, allow_unused=True)
    assert got[1] is None and got[2] is None and torch.equal(got[0], g1[0])
    assert torch.equal(gd.grad, pg + g1[1]) and torch.equal(bd.grad, pb + g1[2])
    # ---- frozen affine parameters: same dx, no parameter gradient
    xf, gf, bf, rf = hip_inputs(params_grad=False)
    outf = F.batch_norm(xf, gf, bf, rmd, rvd, False, 0.1, EPS, relu, rf)
    assert torch.equal(outf, out)
    outf.backward(gyd)
    assert torch.equal(xf.grad, g1[0]) and gf.grad is None and bf.grad is None
    if res:
        assert torch.equal(rf.grad, g1[3])
    # ---- only the parameters want a gradient (dx == NULL inside): the same sums
    xn, gn, bn_, rn = hip_inputs()
    xn.requires_grad_(False)
    if res:
        rn.requires_grad_(False)
    F.batch_norm(xn, gn, bn_, rmd, rvd, False, 0.1, EPS, relu, rn).backward(gyd)
    assert xn.grad is None and torch.equal(gn.grad, g1[1]) and torch.equal(bn_.grad, g1[2])


def test_running_statistics_updated_between_forward_and_backward_are_reported(F):
    x = rnd(64, 8, seed=1).cuda().requires_grad_()
    gamma, beta, rm, rv = (t.cuda() for t in _params(8))
    out = F.batch_norm(x, gamma.requires_grad_(), beta.requires_grad_(), rm, rv, False, 0.1, EPS, True)
    rm.mul_(0.9)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


# the C entry point on channel slices of wider tensors (ldx, lddy, lddx > C): 64 of 80 columns at a 16-byte aligned offset -> float4 kernels;
# 6 of 11 columns at offset 3 -> scalar kernels
@pytest.mark.parametrize("C,W,off,R", [(64, 80, 8, 333), (6, 11, 3, 333)])
@pytest.mark.parametrize("relu", [0, 1])
def test_entry_point_on_channel_slices(F, C, W, off, R, relu):
    from pdfnet_amd import hip
    L = hip.lib()
    gamma, beta, rm, rv = _params(C)
    scale = gamma / torch.sqrt(rv + EPS)
    shift = beta - rm * scale
    dyw, xw, yw = rnd(R, W, seed=1), rnd(R, W, seed=2) * 2 + 0.5, rnd(R, W, seed=3)
    sl = slice(off, off + C)
    g64 = dyw[:, sl].double() * ((yw[:, sl] > 0).double() if relu else 1.0)
    xh64 = (xw[:, sl].double() - rm.double()) / torch.sqrt(rv.double() + EPS)
    dx64, dbeta64, dgamma64 = g64 * scale.double(), g64.sum(0), (g64 * xh64).sum(0)
    d = lambda t: t.cuda()
    dyd, xd, yd, rmd, rvd, scd, shd = d(dyw), d(xw), d(yw), d(rm), d(rv), d(scale), d(shift)
    ws = torch.empty(L.pdf_bn_workspace_floats(C, R), device='cuda')
    at = lambda t: hip.ptr_at(t, off)
    SENT = 7.0

    def run(want_dx, want_dres, want_sums, accumulate=0):
        dxw, drw = torch.full((R, W), SENT, device='cuda'), torch.full((R, W), SENT, device='cuda')
        dg, db = torch.full((C,), 2.0, device='cuda'), torch.full((C,), -3.0, device='cuda')
        L.pdf_bn_eval_bwd(at(dyd), W, at(yd) if relu else None, W, relu, at(xd), W, hip.ptr(rmd), hip.ptr(rvd), EPS, hip.ptr(scd), hip.ptr(shd), C, R,
                          at(dxw) if want_dx else None, W, at(drw) if want_dres else None, W,
                          hip.ptr(dg) if want_sums else None, hip.ptr(db) if want_sums else None, accumulate, hip.ptr(ws), hip.stream())
        torch.cuda.synchronize()
        for name, t, want, ref in (("dx", dxw, want_dx, dx64), ("dres", drw, want_dres, g64)):
            t = t.cpu()
            outside = torch.cat((t[:, :off], t[:, off + C:]), 1)
            assert bool((outside == SENT).all()), name + ": a column outside the slice was written"
            if want:
                close(t[:, sl], ref, 5e-5 if name == "dx" else 1e-6, rtol=5e-5 if name == "dx" else 0.0, what="slice " + name)
            else:
                assert bool((t == SENT).all()), name + " was written though NULL was passed"
        if want_sums:
            base_g, base_b = (2.0, -3.0) if accumulate else (0.0, 0.0)
            close(dg, dgamma64 + base_g, 2e-4, rtol=5e-5, what="slice dgamma")
            close(db, dbeta64 + base_b, 2e-4, rtol=5e-5, what="slice dbeta")
        else:
            assert bool((dg == 2.0).all()) and bool((db == -3.0).all())
        return dxw, dg, db

    full = run(True, True, True)
    sums_only = run(False, False, True)                      # dx == NULL
    dx_only = run(True, False, False)                        # both sum pointers NULL
    assert torch.equal(full[1], sums_only[1]) and torch.equal(full[2], sums_only[2]) and torch.equal(full[0], dx_only[0])
    run(True, True, True, accumulate=1)


@pytest.mark.parametrize("R,K,C", [(96, 64, 128), (300, 64, 256), (7, 5, 8)])
def test_bn_relu_max_over_k_eval_backward(F, R, K, C):
    from pdfnet_amd import hip
    x = rnd(R * K, C, seed=1) * 1.5 + 0.3
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(C, generator=g) + 0.5, rnd(C, seed=2) * 0.5
    gamma[::7] *= -1.0                                       # negative scales: the max then sits on the smallest input
    rm, rv = rnd(C, seed=3), torch.rand(C, generator=g) * 0.999 + 0.5
    gy = rnd(R, C, seed=4)
    xd, gd, bd = x.cuda().requires_grad_(), gamma.cuda().requires_grad_(), beta.cuda().requires_grad_()
    rmd, rvd = rm.cuda(), rv.cuda()
    out = F.bn_relu_max_over_k(xd, gd, bd, rmd, rvd, K, False, 0.1, EPS)
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)
    # the arg-max the forward took: the same entry point called directly
    L = hip.lib()
    o2, arg = torch.empty(R, C, device='cuda'), torch.empty(R, C, dtype=torch.int32, device='cuda')
    tmp = [torch.empty(C, device='cuda') for _ in range(4)]
    ws = torch.empty(L.pdf_bn_workspace_floats(C, R * K), device='cuda')
    L.pdf_bn_relu_maxk_fwd(hip.ptr(xd), C, C, R, K, hip.ptr(gd), hip.ptr(bd), hip.ptr(rmd), hip.ptr(rvd), 0.1, EPS, 0, hip.ptr(o2), C, hip.ptr(arg),
                           *[hip.ptr(t) for t in tmp], hip.ptr(ws), hip.stream())
    assert torch.equal(o2, out.detach())
    arg = arg.cpu().long()
    assert int(arg.min()) >= 0 and int(arg.max()) < K
    # ---- float64: the value, then the gradients with (out > 0, arg) fixed
    x64, g64, b64 = (t.double().requires_grad_() for t in (x, gamma, beta))
    z = TF.batch_norm(x64, rm.double(), rv.double(), g64, b64, False, 0.1, EPS).view(R, K, C)
    close(out, TF.relu(z).max(1)[0], 2e-5, what="maxk eval fwd")
    ref = torch.gather(z, 1, arg.unsqueeze(1)).squeeze(1) * (out.detach().cpu() > 0).double()
    ref.backward(gy.double())
    gyd = gy.cuda()
    g1 = torch.autograd.grad(out, (xd, gd, bd), gyd, retain_graph=True)
    g2 = torch.autograd.grad(out, (xd, gd, bd), gyd, retain_graph=True)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    close(g1[0], x64.grad, 5e-5, rtol=5e-5, what="maxk eval dx")
    close(g1[1], g64.grad, 2e-4, rtol=5e-5, what="maxk eval dgamma")
    close(g1[2], b64.grad, 2e-4, rtol=5e-5, what="maxk eval dbeta")
    # direct accumulation and frozen parameters, as for the plain form
    gd._pdf_main_grad = bd._pdf_main_grad = True
    gd.grad, bd.grad = torch.full_like(g1[1], 0.75), torch.full_like(g1[2], -1.5)
    got = torch.autograd.grad(out, (xd, gd, bd), gyd, retain_graph=True, allow_unused=True)
    assert got[1] is None and got[2] is None and torch.equal(got[0], g1[0])
    assert torch.equal(gd.grad, 0.75 + g1[1]) and torch.equal(bd.grad, -1.5 + g1[2])
    xf = x.cuda().requires_grad_()
    F.bn_relu_max_over_k(xf, gamma.cuda(), beta.cuda(), rmd, rvd, K, False, 0.1, EPS).backward(gyd)
    assert torch.equal(xf.grad, g1[0])


# ----------------------------------------------------------------------------------------------
def _compare_gradients(m, go, what):
    """The fixed bars of tests/test_full_gradient_gpu.py: norm within 1.5e-3 (5e-3 for the 3-channel SFT layer on the raw cloud, see
    there) and cosine >= 0.9999 for every parameter the float64 oracle has a gradient for; none or an exact zero for every other.
    That test's escape for a bias in front of a training-mode BatchNorm is NOT taken over: with frozen statistics those gradients are
    real and meet the fixed bars.  What remains are the nine key biases of the attention blocks (`*.w_ks.bias`): a key bias shifts
    every logit of a query by the same amount, softmax does not see it, and the gradient is zero in exact arithmetic in any mode
    (float64: ~3e-13) -- a cosine against it compares rounding noise.  They are held to what an exact zero allows: float64 norm
    <= 1e-6 and float32 norm <= 1e-2 of the norm of the same layer's weight gradient (the bar that test sets for exact zeros)."""
    bad, checked, none_o, zeros, worst = [], 0, 0, 0, (0.0, 1.0)
    for n, p in m.named_parameters():
        g64 = go[n].grad
        if g64 is None:
            none_o += 1
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, (what, n)
            continue
        assert p.grad is not None, (what, n)
        g = p.grad.detach().cpu().double()
        na, nb = float(g64.norm()), float(g.norm())
        cos = float((g64 * g).sum()) / (na * nb + 1e-300)
        tol = 5e-3 if 'pointnet_plus.sft0' in n else 1.5e-3
        if 'pointnet_plus.sft0' not in n and not n.endswith('.w_ks.bias'):
            worst = (max(worst[0], abs(na - nb) / (na + 1e-300)), min(worst[1], cos))
        if abs(na - nb) <= tol * na + 1e-12 and cos >= 0.9999:
            checked += 1
        elif n.endswith('.w_ks.bias') and na <= 1e-6 * float(go[n[:-4] + 'weight'].grad.norm()) and nb <= 1e-2 * float(go[n[:-4] + 'weight'].grad.norm()):
            checked += 1
            zeros += 1
        else:
            bad.append((n, tuple(g.shape), na, nb, cos))
    print("%s: %d gradients checked, %d without one; worst norm error %.3e, worst cosine %.7f" % (what, checked, none_o, worst[0], worst[1]))
    assert not bad, what + "\n" + "\n".join("%s %s |g64|=%.4e |g32|=%.4e cos=%.6f" % b for b in bad[:20])
    assert none_o == 324 and checked == len(go) - 324            # tests/golden/params_without_grad.txt
    assert zeros <= 9


def test_whole_model_gradients_with_frozen_batchnorm_against_the_fp64_oracle(F):
    """Weights, batch and loss of tests/test_full_gradient_gpu.py with oracle and HIP model in .eval(); then the same step in .train() with
    layers.freeze_batchnorm (dropout off), and once more through the opt-in fused set-abstraction mode, whose frozen levels must take
    the per-layer path.  The running statistics must not move by a bit."""
    from oracle import loss_cpu as LC
    from oracle import pdfnet_cpu as O
    from oracle import synth
    from pdfnet_amd.networks import layers
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 256, 2
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    batch = synthetic_train_batch(B, R, seed=41, consts=consts)
    m = load_model_intag(opt)
    sd = synth.det_state_dict(m.state_dict())
    # ---- oracle, float64, eval mode
    torch.set_num_threads(max(1, (os.cpu_count() or 2) // 2))
    o = O.load_model_cpu(opt)
    o.load_state_dict(sd)
    o.double().eval()
    bd = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in batch.items()}
    z = np.load(os.path.join(ROOT, "pdfnet_amd", "data", "gcn_core.npz"))
    result, params, hand, other = o(bd['input'], bd['choose'], bd['cloud'], bd['depth'], bd['ind'], bd['K_new'], bd['valid'])
    for h in ('left', 'right'):
        other['converter_' + h] = LC.Converter(z['graph_perm_' + h], z['graph_perm_reverse_' + h])
    loss_o, stats_o = LC.ctdet_loss(opt, consts, result, params, hand, other, bd, 'train', 25)
    extra = lambda oth: oth['ret']['wh'].pow(2).mean() + oth['ret']['params'].pow(2).mean()
    (loss_o.mean() + extra(other)).backward()
    go = dict(o.named_parameters())
    # ---- HIP, float32
    m.load_state_dict(sd)
    m.cuda().eval()
    crit = CtdetLoss(opt, consts).cuda()
    bg = {k: v.cuda() for k, v in batch.items()}
    is_stat = lambda k: k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))
    before = {k: v.clone() for k, v in m.state_dict().items() if is_stat(k)}
    assert len(before) > 150 * 3 // 2

    def step(what):
        m.zero_grad(set_to_none=True)
        res = m(bg['input'], bg['choose'], bg['cloud'], bg['depth'], bg['ind'], bg['K_new'], bg['valid'])
        loss_g, stats_g, _, _ = crit(*res, bg, 'train', 25)
        (loss_g.mean() + extra(res[3])).backward()
        F.join_wgrad()
        torch.cuda.synchronize()
        for k, v in stats_o.items():
            a, b = torch.as_tensor(stats_g[k]).detach().cpu().double().reshape(-1), torch.as_tensor(v).detach().reshape(-1)
            assert torch.allclose(a, b, rtol=2e-4, atol=1e-6), (what, k, a, b)
        _compare_gradients(m, go, what)
        after = m.state_dict()
        for k, v in before.items():
            assert torch.equal(after[k], v), (what, k)

    step("eval")
    m.train()
    layers.freeze_batchnorm(m)
    for mod in m.modules():
        if isinstance(getattr(mod, 'p', None), float):
            mod.p = 0.0
    bns = [b for b in m.modules() if isinstance(b, layers.BatchNorm)]
    assert m.training and len(bns) > 75 and not any(b.training for b in bns)
    step("train, frozen BatchNorm")
    was = F.SA_FUSED
    try:
        F.set_sa_fused(True)
        step("train, frozen BatchNorm, fused set abstraction switched on")
    finally:
        F.set_sa_fused(was)
    assert not any(b.training for b in bns)


def test_trainer_freezes_batchnorm_when_opt_freeze_bn_is_set(F):
    """opt.freeze_bn: the Trainer applies layers.freeze_batchnorm to the model it is given; its train steps (model.train() inside, gradients
    accumulated straight into the flat buffer) then move the parameters and leave every BatchNorm statistic and counter untouched."""
    from pdfnet_amd.networks import layers
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 2
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0, freeze_bn=True)
    consts = synthetic_loss_constants()
    batch = to_device(synthetic_train_batch(B, R, seed=3, consts=consts), dev)
    torch.manual_seed(7)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev), lr=1e-4)
    bns = [b for b in m.modules() if isinstance(b, layers.BatchNorm)]
    assert bns and not any(b.training for b in bns)
    is_stat = lambda k: k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))
    before = {k: v.clone() for k, v in m.state_dict().items() if is_stat(k)}
    p0 = tr.optimizer.flat_p.clone()
    for _ in range(2):
        tr.train_step(batch, 0)
    torch.cuda.synchronize()
    assert m.training and not any(b.training for b in bns)
    after = m.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert bool(torch.isfinite(tr.optimizer.flat_p).all()) and float((tr.optimizer.flat_p - p0).abs().max()) > 1e-5
    # the BatchNorm affine parameters are trained: their gradients arrived in the flat buffer
    assert float(m.encoder.resnet.bn1.weight.grad.abs().max()) > 0 and float(m.encoder.resnet.layer1[0].bn3.bias.grad.abs().max()) > 0
