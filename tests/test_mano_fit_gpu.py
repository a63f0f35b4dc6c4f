"""pdf_mano_fit (csrc/manofit.hip, F.mano_fit, utils.mano_fit_pair, Trainer.evaluation(mano_fit=...)) against the float64 restatement of its
contract in tests/mano_fit_ref.py, on the synthetic MANO constants.  Converged quantities and single-step quantities only: a 20-step fp32
trajectory is never compared with a float64 one.  B <= 4 everywhere; the float64 references are computed once per module."""
import functools

import pytest
import torch

from tests import mano_fit_ref as R
from tests.util import make_opt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEEDS, POSE_STD = (0, 1, 2), (0.2, 0.5, 0.8)
CLEAN_BAR_MM = 1e-3          # one ulp of a coordinate at 0.5 m is 3e-5 mm: about 30 ulp


def dev():
    return torch.device('cuda')


@functools.lru_cache(maxsize=None)
def gpu_consts(side):
    return {k: v.float().to(dev()).contiguous() for k, v in R.consts_of(side).items()}


def params_of(f):
    return torch.cat((f.root, f.pose, f.shape, f.trans), 1)


@functools.lru_cache(maxsize=None)
def targets(side, s, noise=0.0):
    """[3, 778, 3] float32 on the CPU: seeds 0-2 of one pose spread; float64 generation, then rounded (the rounded mesh is the target of both)."""
    return torch.stack([R.case(seed, s, side, noise)[1].float() for seed in SEEDS])


@functools.lru_cache(maxsize=None)
def gpu_clean(side, s):
    from pdfnet_amd import functional as F
    return F.mano_fit(gpu_consts(side), targets(side, s).to(dev()), side=side, iters=20)


def random_state(side, seed=0):
    """A state a tenth of a radian (and 0.1 shape units, 10 cm) off the generating one, rounded to float32 -> (init [61] f32, target [778, 3] f32)"""
    p, t = R.case(seed, 0.5, side)
    g = torch.Generator().manual_seed(11 + seed)
    return (p + 0.1 * torch.randn(R.NP, dtype=torch.float64, generator=g)).float(), t.float()


def random_weight(seed=3):
    g = torch.Generator().manual_seed(seed)
    w = 2 * torch.rand(R.NV, generator=g)
    w[torch.rand(R.NV, generator=g) < 0.1] = 0
    return w


# ---- 1. the system at iters = 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('at', ['start', 'init'])
@pytest.mark.parametrize('side', ['left', 'right'])
def test_system_against_float64(side, at, weighted):
    """A, g and cost0 of one build.  |A_ij - A64_ij| / S_ij with S_ij = sum_k w_k |J_ki| |J_kj|, |g_i - g64_i| / sum_k w_k |J_ki| |r_k| and
    |E - E64| / E64; the bar of each is 8 x the same figure of the restatement run in float32 on the CPU, never below 32 * 2^-24 (a different
    summation order over 2,334 terms).  'start' is the default start, where every rotation is the Rodrigues edge a = 0."""
    from pdfnet_amd import functional as F
    init, t = random_state(side)
    w = random_weight() if weighted else None
    kw = dict(weight=None if w is None else w[None].to(dev()))
    if at == 'init':
        kw['init'] = init[None].to(dev())
    f = F.mano_fit(gpu_consts(side), t[None].to(dev()), side=side, iters=0, return_system=True, **kw)
    p0 = params_of(f)[0].cpu()
    c64, c32 = R.consts_of(side), R.consts_of(side, torch.float32)
    if at == 'init':
        assert torch.equal(p0, init)
    else:
        want = R.start_point(c64, t.double())
        assert float(p0[:58].abs().max()) == 0.0 and float((p0[58:].double() - want[58:]).abs().max()) <= 2 * U
    assert int(f.accepted[0]) == 0 and int(f.rejected[0]) == 0 and float(f.cost[0]) == float(f.cost0[0]) and float(f.lam[0]) == pytest.approx(1e-3, rel=1e-6)
    w64 = None if w is None else w.double()
    J, r, wr, A, g, E = R.system(c64, p0.double(), t.double(), side, weight=w64)
    _, _, _, A32, g32, E32 = R.system(c32, p0, t, side, weight=w)
    eA32, eg32 = R.normalised_errors(J, r, wr, A, g, A32, g32)
    eA, eg = R.normalised_errors(J, r, wr, A, g, f.A[0].cpu(), f.g[0].cpu())
    eE, eE32 = abs(float(f.cost0[0]) - E) / E, abs(E32 - E) / E
    bars = [max(8 * e, 32 * U) for e in (eA32, eg32, eE32)]
    print('%s %s weighted=%s: A %.3g (cpu fp32 %.3g, bar %.3g, ratio %.3f)  g %.3g (%.3g, %.3g, %.3f)  E %.3g (%.3g, %.3g, %.3f)' % (
        side, at, weighted, eA, eA32, bars[0], eA / bars[0], eg, eg32, bars[1], eg / bars[1], eE, eE32, bars[2], eE / bars[2]))
    assert torch.equal(f.A[0], f.A[0].T)
    assert eA <= bars[0] and eg <= bars[1] and eE <= bars[2]


# ---- 2. one step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', ['left', 'right'])
def test_one_step_is_the_solve_of_the_returned_system(side):
    """iters = 1: p - init is the float64 solution of the kernel's own (A, g, lambda_0) -- this pins the Cholesky, not the trajectory.  Bar:
    cond(A + lambda D) * 2^-24 * |delta|, computed here; the rounding of p = init + delta to float32 (2^-24 |p| per entry) is far inside it."""
    from pdfnet_amd import functional as F
    init, t = random_state(side, seed=1)
    f = F.mano_fit(gpu_consts(side), t[None].to(dev()), side=side, iters=1, init=init[None].to(dev()), return_system=True)
    ref = R.fit(R.consts_of(side), t.double(), side, init=init.double(), iters=1)
    assert (int(f.accepted[0]), int(f.rejected[0])) == (ref['accepted'], ref['rejected']) == (1, 0)
    assert float(f.lam[0]) == pytest.approx(1e-3 / 4, rel=1e-6)
    Ad = R.damped(f.A[0].cpu().double(), float(torch.tensor(1e-3, dtype=torch.float32)))
    delta = torch.linalg.solve(Ad, -f.g[0].cpu().double())
    cond = float(torch.linalg.cond(Ad))
    err = float((params_of(f)[0].cpu().double() - init.double() - delta).norm())
    bar = cond * U * float(delta.norm())
    print('%s: |delta| %.4g, cond %.4g, |p - init - delta| %.3g, bar %.3g' % (side, float(delta.norm()), cond, err, bar))
    assert err <= bar
    assert float(f.cost[0]) < float(f.cost0[0])


# ---- 3. convergence on noise-free targets, 5. consistency -------------------------------------------------------
@pytest.mark.parametrize('s', POSE_STD)
@pytest.mark.parametrize('side', ['left', 'right'])
def test_noise_free_targets_converge(side, s):
    f, t = gpu_clean(side, s), targets(side, s)
    for b in range(len(SEEDS)):
        rms = R.rms_mm(f.verts[b].cpu(), t[b])
        print('%s pose std %.1f seed %d: rms %.3g mm, cost0 %.4g, cost %.4g, accepted %d, rejected %d, lambda %.3g' % (
            side, s, SEEDS[b], rms, float(f.cost0[b]), float(f.cost[b]), int(f.accepted[b]), int(f.rejected[b]), float(f.lam[b])))
        assert rms < CLEAN_BAR_MM
        assert float(f.cost[b]) <= float(f.cost0[b])
        assert int(f.accepted[b]) + int(f.rejected[b]) == 20


@pytest.mark.parametrize('side', ['left', 'right'])
def test_returned_mesh_is_the_layer_at_the_returned_parameters(side):
    from pdfnet_amd import functional as F
    f = gpu_clean(side, 0.8)
    v, j = F.mano_lbs(gpu_consts(side), f.root.contiguous(), f.pose.contiguous(), f.shape.contiguous(), f.trans.contiguous(), side=side)
    dv, dj = float((v - f.verts).abs().max()), float((j - f.joints).abs().max())
    print('%s: max |verts - mano_lbs| %.3g m, joints %.3g m' % (side, dv, dj))
    assert dv <= 1e-6 and dj <= 1e-6


# ---- 4. convergence on noisy targets -----------------------------------------------------------------------
@pytest.mark.parametrize('s', POSE_STD)
def test_noisy_targets_reach_the_float64_minimum(s):
    """N(0, 2 mm) per coordinate: E_gpu <= E_float64 (1 + 1e-4), the float64 value being the converged minimum of the restatement."""
    from pdfnet_amd import functional as F
    t = targets('left', s, 0.002)
    f = F.mano_fit(gpu_consts('left'), t.to(dev()), iters=20)
    c64 = R.consts_of('left')
    for b in range(len(SEEDS)):
        ref = R.fit(c64, t[b].double(), 'left')
        E, rms = float(f.cost[b]), R.rms_mm(f.verts[b].cpu(), t[b])
        print('pose std %.1f seed %d: E %.9g, float64 %.9g, ratio - 1 = %.3g, rms %.4f mm' % (s, SEEDS[b], E, ref['cost'], E / ref['cost'] - 1, rms))
        assert E <= ref['cost'] * (1 + 1e-4)
        assert int(f.accepted[b]) + int(f.rejected[b]) == 20


# ---- 6. batch independence, invalid rows -------------------------------------------------------------------
FIELDS = ('root', 'pose', 'shape', 'trans', 'verts', 'joints', 'cost0', 'cost', 'accepted', 'rejected', 'lam', 'A', 'g')


def test_rows_do_not_depend_on_the_batch_and_invalid_rows_stay_put():
    from pdfnet_amd import functional as F
    c = gpu_consts('left')
    t = torch.stack([R.case(seed, s, 'left', 0.001)[1].float() for seed, s in ((0, 0.2), (1, 0.8), (2, 0.5))]).to(dev())
    whole = F.mano_fit(c, t, iters=20, return_system=True)
    again = F.mano_fit(c, t, iters=20, return_system=True)
    for b in range(3):
        alone = F.mano_fit(c, t[b:b + 1], iters=20, return_system=True)
        for k in FIELDS:
            assert torch.equal(getattr(whole, k)[b], getattr(alone, k)[0]), (b, k)
            assert torch.equal(getattr(whole, k), getattr(again, k)), k
    valid = torch.tensor([1.0, 0.0, 1.0], device=dev())
    part = F.mano_fit(c, t, valid=valid, iters=20, return_system=True)
    for k in FIELDS:
        assert torch.equal(getattr(part, k)[[0, 2]], getattr(whole, k)[[0, 2]]), k
    start = R.start_point(R.consts_of('left'), t[1].cpu().double())
    p1 = params_of(part)[1].cpu()
    assert float(p1[:58].abs().max()) == 0.0 and float((p1[58:].double() - start[58:]).abs().max()) <= 2 * U
    assert float(part.cost0[1]) == 0.0 and float(part.cost[1]) == 0.0 and int(part.accepted[1]) == 0 and int(part.rejected[1]) == 0
    assert float(part.A[1].abs().max()) == 0.0 and float(part.g[1].abs().max()) == 0.0
    v, j = F.mano_lbs(c, part.root[1:2].contiguous(), part.pose[1:2].contiguous(), part.shape[1:2].contiguous(), part.trans[1:2].contiguous(), side='left')
    assert float((v[0] - part.verts[1]).abs().max()) <= 1e-6 and float((j[0] - part.joints[1]).abs().max()) <= 1e-6


# ---- 7. weights ------------------------------------------------------------------------------------------
def test_zero_weights_ignore_their_vertices():
    """Zero weight on a random half of the vertices and 5 mm noise only there: the weighted half meets the noise-free bar."""
    from pdfnet_amd import functional as F
    _, t = R.case(2, 0.5)
    g = torch.Generator().manual_seed(5)
    off = torch.randperm(R.NV, generator=g)[:R.NV // 2]
    w = torch.ones(R.NV)
    w[off] = 0
    noisy = t.clone()
    noisy[off] += 0.005 * torch.randn(len(off), 3, dtype=torch.float64, generator=g)
    f = F.mano_fit(gpu_consts('left'), noisy.float()[None].to(dev()), weight=w[None].to(dev()), iters=20)
    keep = w > 0
    v = f.verts[0].cpu()
    rms = R.rms_mm(v[keep], t.float()[keep])
    print('weighted half: rms %.3g mm; unweighted half: %.3g mm' % (rms, R.rms_mm(v[~keep], noisy.float()[~keep])))
    assert rms < CLEAN_BAR_MM
    assert R.rms_mm(v[~keep], noisy.float()[~keep]) > 1.0


# ---- 8. priors -------------------------------------------------------------------------------------------
def test_priors():
    """prior_shape = 1e6 pins the shape while the fit still lowers the cost.  With prior_pose > 0 the returned cost is the restatement's E at the
    returned parameters: a float32 residual coordinate near 0.5 m carries up to ~4 ulp = 1.2e-7 m of rounding (the skinning sum and the
    translation), so |E - E64| <= 2 * 1.2e-7 * sum_k |r_k| + 8 * 2^-24 * E (the second term: the squares and the prior term in float32 inputs)."""
    from pdfnet_amd import functional as F
    _, t = R.case(0, 0.5)
    tg = t.float()[None].to(dev())
    f = F.mano_fit(gpu_consts('left'), tg, iters=20, prior_shape=1e6)
    assert float(f.shape[0].norm()) < 1e-3 and float(f.cost[0]) < float(f.cost0[0])
    assert int(f.accepted[0]) + int(f.rejected[0]) == 20
    c64 = R.consts_of('left')
    for iters in (0, 6):
        f = F.mano_fit(gpu_consts('left'), tg, iters=iters, prior_pose=0.05, init=None if iters else random_state('left')[0][None].to(dev()))
        p = params_of(f)[0].cpu().double()
        E64 = R.energy(c64, p, t.float().double(), 'left', prior_pose=0.05)
        with R.default_dtype(torch.float64):
            r1 = float((R.model(c64, p, 'left')[0] - t.float().double()).abs().sum())
        bar = 2 * 1.2e-7 * r1 + 8 * U * E64
        print('prior_pose, iters %d: E %.9g, float64 %.9g, |difference| %.3g, bar %.3g' % (iters, float(f.cost[0]), E64, abs(float(f.cost[0]) - E64), bar))
        assert abs(float(f.cost[0]) - E64) <= bar
        assert float(f.cost[0]) <= float(f.cost0[0])


# ---- 9. evaluation ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluation_runs():
    """R = 128, B = 2, one batch, random-init model; the ground-truth meshes are F.mano_lbs hands, the right hand of sample 0 is invalid."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    res, B = 128, 2
    opt = make_opt(res, size_train=[res, res], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev())
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev()))
    batch = synthetic_train_batch(B, res, seed=31, consts=consts)
    lbs = {side: gpu_consts(side) for side in ('left', 'right')}
    K = batch['K_new']
    proj = lambda p: (p @ K.transpose(1, 2))[..., :2] / (p @ K.transpose(1, 2))[..., 2:]
    for side in ('left', 'right'):
        p = torch.stack([R.case(10 + b, 0.5, side)[0].float() for b in range(B)]).to(dev())
        v = F.mano_lbs(lbs[side], p[:, :3].contiguous(), p[:, 3:48].contiguous(), p[:, 48:58].contiguous(), p[:, 58:].contiguous(), side=side)[0].cpu()
        j = torch.einsum('jv,bvc->bjc', consts['full_regressor_' + side], v)
        batch['verts_%s_gt' % side], batch['joints_%s_gt' % side] = v, j
        batch['verts2d_%s_gt' % side], batch['lms_%s_gt' % side] = proj(v), proj(j)
    batch['valid'][0, 1] = 0
    loader = [batch]
    return {'plain': tr.evaluation(loader), 'off': tr.evaluation(loader, mano_fit=False), 'on': tr.evaluation(loader, mano_fit=lbs),
            'others': tr.evaluation(loader, aligned=True, interaction=True, two_sided=True),
            'others_on': tr.evaluation(loader, aligned=True, interaction=True, two_sided=True, mano_fit=lbs)}


def test_evaluation_mano_fit_keys():
    from pdfnet_amd.trains.base_trainer import MANO_FIT_KEYS
    runs = evaluation_runs()
    plain = runs['plain']
    assert plain['samples'] == 2 and runs['off'] == plain and list(runs['off']) == list(plain)
    for base, on in ((plain, runs['on']), (runs['others'], runs['others_on'])):
        assert sorted(on) == sorted(list(base) + list(MANO_FIT_KEYS))
        for k, v in base.items():
            assert on[k] == v, k                                  # bit for bit: the floats come from the same sums
        assert on['mano_fit_samples'] == 2
        for k in ('mano_residual', 'mano_residual_gt', 'mano_abs_verts', 'mano_abs_joints'):
            assert k in on and k + '_left' in on and k + '_right' in on
    on = runs['on']
    print({k: on[k] for k in MANO_FIT_KEYS})
    for k in ('mano_residual_gt', 'mano_residual_gt_left', 'mano_residual_gt_right'):
        assert 0.0 <= on[k] < CLEAN_BAR_MM
    assert on['mano_residual'] > on['mano_residual_gt']           # a random-init network's mesh is no hand
    assert on['mano_abs_verts'] > 0 and on['mano_abs_joints'] > 0
    assert runs['on'] == {**plain, **{k: runs['others_on'][k] for k in MANO_FIT_KEYS}}


def test_mano_fit_pair_is_the_two_single_calls():
    from pdfnet_amd import functional as F
    from pdfnet_amd.utils import mano_fit_pair
    lbs = {side: gpu_consts(side) for side in ('left', 'right')}
    v = torch.stack((targets('left', 0.5)[:2], targets('right', 0.5)[:2]), 1).to(dev())      # [2, 2, 778, 3]
    valid = torch.tensor([[1.0, 0.0], [1.0, 1.0]], device=dev())
    pair = mano_fit_pair(lbs, v, valid, iters=3)
    for h, side in enumerate(('left', 'right')):
        one = F.mano_fit(lbs[side], v[:, h], side=side, valid=valid[:, h], iters=3)
        for k in FIELDS[:-2]:
            assert torch.equal(getattr(pair[h], k), getattr(one, k)), (side, k)
    assert float(pair[1].cost[0]) == 0.0 and float(pair[0].cost[0]) > 0.0


# ---- 10. bad arguments -----------------------------------------------------------------------------------
def test_bad_arguments_raise():
    from pdfnet_amd import functional as F
    c = gpu_consts('left')
    t = targets('left', 0.2).to(dev())
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_fit(c, t.cpu())
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_fit(c, t, weight=torch.ones(3, 778))
    for bad in (t[:, :777], t[0], t[..., :2]):
        with pytest.raises(ValueError, match='target'):
            F.mano_fit(c, bad)
    with pytest.raises(ValueError, match='weight'):
        F.mano_fit(c, t, weight=torch.ones(3, 777, device=dev()))
    with pytest.raises(ValueError, match='valid'):
        F.mano_fit(c, t, valid=torch.ones(2, device=dev()))
    with pytest.raises(ValueError, match='init'):
        F.mano_fit(c, t, init=torch.zeros(3, 58, device=dev()))
    with pytest.raises(ValueError, match='iterations'):
        F.mano_fit(c, t, iters=-1)
    with pytest.raises(ValueError, match='priors'):
        F.mano_fit(c, t, prior_pose=-1.0)
    with pytest.raises(ValueError, match='side'):
        F.mano_fit(c, t, side='both')
    with pytest.raises(ValueError, match='J_regressor'):
        F.mano_fit({**c, 'J_regressor': c['J_regressor'][:15]}, t)
    from pdfnet_amd.hip import lib, ptr, stream
    L = lib()
    assert L.pdf_mano_fit_workspace_floats(3) >= 0
    with pytest.raises(RuntimeError, match='code -1'):           # PDF_E_BADARG: a required output is NULL
        L.pdf_mano_fit(ptr(t), None, None, None, ptr(c['v_template']), ptr(c['shapedirs']), ptr(c['posedirs']), ptr(c['J_regressor']),
                       ptr(c['weights']), 3, 1, 20, 0.0, 0.0, None, None, None, None, None, None, None, None, None, stream())
