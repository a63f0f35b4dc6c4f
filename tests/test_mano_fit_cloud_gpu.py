"""pdf_mano_cloud_targets and pdf_mano_fit_cloud on the GPU (csrc/icp.hip, csrc/manofit.hip, F.mano_cloud_targets, F.mano_fit_cloud,
utils.mano_fit_cloud_pair, Trainer.evaluation(cloud_fit=...)) against the float64 restatement in tests/mano_fit_cloud_ref.py.

The targets are compared with the restatement GIVEN the association the same call returns (tri, bary, closest), so no near-tie between two
triangles can flip the comparison; the association itself is pinned by bit-equality with F.cloud_mesh_loss and F.mesh_icp(iters=0), whose
device code the kernel shares.  The loop is compared bit for bit with its own composition out of F.mano_cloud_targets and F.mano_fit, and its
behaviour on the scene of tests/test_mano_fit_cloud_cpu.py with the float64 loop.  B = 3, P = 200, outer <= 4, inner = 3 throughout; the
float64 references are computed once per module."""
import functools

import numpy as np
import pytest
import torch

from tests import mano_fit_cloud_ref as C
from tests import mano_fit_ref as R
from tests.test_cloud_loss_gpu import REGION_CLOSEST, REGION_WEIGHTS
from tests.test_icp_gpu import REGION_QUERIES, TET, TRI, TRIM, TRIM_MARGIN, cu
from tests.test_mano_fit_gpu import gpu_consts
from tests.util import make_opt

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
KEYS = ('target', 'weight', 'rms', 'inliers', 'tri', 'bary', 'closest')
SEEDS = (C.SCENE_SEED, 1, 2)         # rows of the batch; row 1 is invalid
INVALID = 1


def dev():
    return torch.device('cuda')


def run_targets(V, faces, cloud, valid=None, trim=TRIM, anchor=None, alpha=0.0):
    from pdfnet_amd import functional as F
    opt = lambda x: None if x is None else cu(np.asarray(x, np.float32))
    got = F.mano_cloud_targets(cu(np.asarray(V, np.float32)), cu(np.asarray(faces, np.int64)), cu(np.asarray(cloud, np.float32)), opt(valid),
                               trim=trim, anchor=opt(anchor), anchor_weight=alpha, return_fields=True)
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in zip(KEYS, got)}


def check_targets(got, V, faces, cloud, valid, trim, anchor, alpha, label):
    """Every row against the restatement given the kernel's own association.  Per vertex and coordinate, with den = W + alpha:
      S: each contribution w d carries the one fp32 rounding of d = p - q, at most 2^-24 |d| (the product and the sums are double), so
         |S - S64| <= 2^-24 sum w |d|, and the target moves by that over den;
      the final rounding to fp32: 2^-24 |target|;  the double arithmetic (W v + S + alpha a) / den: 1e-14 of the terms' sizes.
    weight = fp32(W + alpha): 2^-24 weight."""
    V, cloud = np.asarray(V, np.float32), np.asarray(cloud, np.float32)
    worst = 0.0
    for b in range(len(V)):
        a = None if anchor is None else np.asarray(anchor[b], np.float32).astype(np.float64)
        ref = C.targets(V[b].astype(np.float64), faces, cloud[b].astype(np.float64), 1 if valid is None else valid[b], trim, a, alpha,
                        fields=(got['tri'][b], got['bary'][b], got['closest'][b]))
        hit = np.isfinite(ref['dist'])
        assert not hit.any() or np.abs(ref['dist'][hit] - trim).min() >= TRIM_MARGIN, (label, b)
        assert got['inliers'][b] == ref['inliers'], (label, b, got['inliers'][b], ref['inliers'])
        den = np.maximum(ref['weight'], 1e-300)[:, None]
        size = np.abs(V[b]).astype(np.float64) + (0 if a is None else np.abs(a)) + ref['absS'] / den
        bar = U * ref['absS'] / den + U * np.abs(ref['target']) * (1 + 1e-6) + 1e-14 * size
        err = np.abs(got['target'][b].astype(np.float64) - ref['target'])
        ratio = float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0        # (a bar of 0: a coordinate that is exactly 0)
        worst = max(worst, ratio)
        assert (err <= bar).all(), (label, b, ratio)
        assert (np.abs(got['weight'][b].astype(np.float64) - ref['weight']) <= U * ref['weight']).all(), (label, b)
        # rms is made of the fp32 |q - p|^2 taken before q = p + (q - p) is rounded: a distance differs from |p - closest| by that rounding
        assert abs(float(got['rms'][b]) - ref['rms']) <= 3 ** 0.5 * U * float(np.abs(cloud[b]).max()) + 4 * U * ref['rms'], (label, b)
        off = ref['W'] == 0
        want = V[b] if (a is None or alpha == 0) else a.astype(np.float32)
        assert np.array_equal(got['target'][b][off], want[off]) and (got['weight'][b][off] == np.float32(alpha if a is not None else 0)).all()
    print('  %s: largest target error / bar %.3f' % (label, worst))
    assert all(np.isfinite(got[k]).all() for k in got)


@functools.lru_cache(maxsize=None)
def batch():
    """-> (verts [3, 778, 3] f32 = M(init) of three scenes computed in float64, faces, cloud [3, 200, 3], valid [3], init [3, 61] f32, anchor [3,
    778, 3] f32: the start meshes moved by 3 mm of seeded noise)."""
    ss = [C.scene(seed) for seed in SEEDS]
    c64 = R.consts_of('left')
    with R.default_dtype(torch.float64):
        verts = np.stack([R.model(c64, s['init'].double(), 'left')[0].numpy() for s in ss]).astype(np.float32)
    valid = np.ones(3, np.float32)
    valid[INVALID] = 0
    g = np.random.default_rng(9)
    anchor = (verts + 0.003 * g.standard_normal(verts.shape)).astype(np.float32)
    return verts, ss[0]['faces'], np.stack([s['cloud'] for s in ss]), valid, torch.stack([s['init'] for s in ss]), anchor


# ---- 1. the targets against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [0.0, 0.5])
def test_targets_against_float64_on_the_template(alpha):
    verts, faces, cloud, valid, _, anchor = batch()
    a = anchor if alpha else None
    got = run_targets(verts, faces, cloud, valid, anchor=a, alpha=alpha)
    check_targets(got, verts, faces, cloud, valid, TRIM, a, alpha, 'template alpha %.1f' % alpha)
    assert got['inliers'][INVALID] == 0 and got['rms'][INVALID] == 0 and (got['tri'][INVALID] == -1).all()
    assert min(got['inliers'][0], got['inliers'][2]) >= 0.9 * C.SCENE_P
    assert abs(float(got['weight'][0].sum()) - alpha * R.NV - got['inliers'][0]) <= 1e-4 * got['inliers'][0]      # sum_v W_v = the inliers


@pytest.mark.parametrize('P', [1, 63, 65])
def test_sizes_on_the_tetrahedron(P):
    V, tris = TET
    g = np.random.default_rng(40 + P)
    pts = np.concatenate((g.uniform(-0.08, 0.08, (2, P, 2)), g.uniform(0.40, 0.56, (2, P, 1))), -1).astype(np.float32)
    Vb = np.stack((V, V + 0.002)).astype(np.float32)
    anchor = Vb + np.float32(0.001)
    for a, alpha in ((None, 0.0), (anchor, 0.25)):
        got = run_targets(Vb, tris, pts, anchor=a, alpha=alpha)
        check_targets(got, Vb, tris, pts, None, TRIM, a, alpha, 'tetrahedron P %d alpha %.2f' % (P, alpha))


# ---- 2. exact checks ----------------------------------------------------------------------------------------
def test_association_is_the_loss_and_the_icp_association_bit_for_bit():
    from pdfnet_amd import functional as F
    verts, faces, cloud, valid, _, _ = batch()
    got = run_targets(verts, faces, cloud, valid)
    pair = lambda x: cu(np.stack((x, x), 1))
    f2 = cu(np.stack((faces, faces)))
    loss = F.cloud_mesh_loss(pair(verts), f2, pair(cloud), pair(valid), trim=TRIM, return_fields=True)
    icp = F.mesh_icp(pair(verts), f2, pair(cloud), pair(valid), iters=0, trim=TRIM, return_fields=True)
    for h in range(2):
        for k, x in (('inliers', loss[1]), ('tri', loss[2]), ('bary', loss[3]), ('closest', loss[4]), ('rms', icp[3]), ('inliers', icp[4]),
                     ('closest', icp[5]), ('tri', icp[6])):
            assert np.array_equal(got[k], x[:, h].cpu().numpy()), (h, k)


def one_triangle(tris, pts, **kw):
    got = run_targets(TRI[None], np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(pts, np.float32)[None], **kw)
    return {k: v[0] for k, v in got.items()}


def test_one_triangle_worked_out_by_hand():
    """n = 3, Fc = 1, 8 points: the seven region queries of tests/test_icp_gpu.py (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc,
    face; 10 to 43.6 mm from the triangle) and one point 10 cm in front of it, beyond the trim of 5 cm.  W = the column sums of the weights
    (2.4, 2.3, 2.3), S = sum w (p - q), target = v + S / W.  Margins as tests/test_cloud_loss_gpu.py derives them: a weight to 1e-5, a closest
    point to 1e-6 m, |p - q| <= 0.0436 m: S to 7 (1e-5 * 0.0436 + 1e-6) = 1e-5 m, W to 7e-5."""
    far = np.array([[0.03, 0.03, 0.40]], np.float32)
    pts = np.concatenate((REGION_QUERIES, far))
    got = one_triangle([0, 1, 2], pts, trim=0.05)
    d = pts[:7].astype(np.float64) - REGION_CLOSEST
    W, S = REGION_WEIGHTS.sum(0), REGION_WEIGHTS.T @ d
    assert np.allclose(W, (2.4, 2.3, 2.3)) and got['inliers'] == 7 and (got['tri'] == 0).all()
    assert np.abs(got['weight'] - W).max() <= 7e-5 and np.abs(got['target'] - (TRI + S / W[:, None])).max() <= 1e-5 / 2.3 + 1e-6
    assert np.abs(got['closest'][:7] - REGION_CLOSEST).max() <= 1e-6 and np.abs(got['bary'][:7] - REGION_WEIGHTS).max() <= 1e-5
    assert abs(float(got['rms']) - np.sqrt((d ** 2).sum(-1).mean())) <= 1e-6
    # the far point has its closest point but is no inlier: without it nothing changes
    assert got['tri'][7] == 0 and np.abs(got['bary'][7] - [0.4, 0.3, 0.3]).max() <= 1e-5
    seven = one_triangle([0, 1, 2], REGION_QUERIES, trim=0.05)
    for k in ('target', 'weight', 'rms', 'inliers'):
        assert np.array_equal(got[k], seven[k]), k
    # a tighter trim: only the face query (10 mm) stays; its weights (0.4, 0.3, 0.3) and d = (0, 0, -0.01) on every corner
    got = one_triangle([0, 1, 2], pts, trim=0.02)
    assert got['inliers'] == 1 and np.abs(got['weight'] - [0.4, 0.3, 0.3]).max() <= 1e-5
    assert np.abs(got['target'] - (TRI + [0, 0, -0.01])).max() <= 2e-6
    # a point with Z = 0 (and one behind the camera) is ignored: the same sums as the remaining points alone, in the same order
    cut = pts.copy()
    cut[1, 2], cut[4] = 0.0, (0.05, -0.02, -0.49)
    live = np.array([1, 0, 1, 1, 0, 1, 1, 1], bool)
    got, rest = one_triangle([0, 1, 2], cut, trim=0.05), one_triangle([0, 1, 2], pts[live], trim=0.05)
    assert np.array_equal(got['tri'], np.where(live, 0, -1)) and (got['closest'][~live] == 0).all() and (got['bary'][~live] == 0).all()
    for k in ('target', 'weight', 'rms', 'inliers'):
        assert np.array_equal(got[k], rest[k]), k
    # the reversed triangle faces away: weight 0, target = v exactly
    got = one_triangle([0, 2, 1], pts, trim=0.05)
    assert (got['tri'] == -1).all() and got['inliers'] == 0 and got['rms'] == 0 and (got['weight'] == 0).all() and np.array_equal(got['target'], TRI)
    a = TRI + np.float32(0.01)
    got = one_triangle([0, 2, 1], pts, trim=0.05, anchor=a[None], alpha=3.0)
    assert (got['weight'] == 3.0).all() and np.array_equal(got['target'], a)


def test_anchor_alone():
    """An all-zero cloud, and valid = 0 with a cloud: target = the anchor exactly, weight = alpha; without an anchor target = v, weight = 0."""
    verts, faces, cloud, valid, _, anchor = batch()
    empty = np.zeros_like(cloud)
    for c, va in ((empty, None), (cloud, np.zeros(3, np.float32))):
        got = run_targets(verts, faces, c, va, anchor=anchor, alpha=1.5)
        assert np.array_equal(got['target'], anchor) and (got['weight'] == 1.5).all()
        assert (got['inliers'] == 0).all() and (got['rms'] == 0).all() and (got['tri'] == -1).all() and (got['bary'] == 0).all() and (got['closest'] == 0).all()
        got = run_targets(verts, faces, c, va)
        assert np.array_equal(got['target'], verts) and (got['weight'] == 0).all()
        got = run_targets(verts, faces, c, va, anchor=anchor, alpha=0.0)
        assert np.array_equal(got['target'], verts) and (got['weight'] == 0).all()


# ---- 3. the loop against its own composition ----------------------------------------------------------------
def fit_cloud(outer, valid=True, anchor=None, alpha=0.0, rows=slice(None), **kw):
    from pdfnet_amd import functional as F
    _, faces, cloud, va, init, _ = batch()
    return F.mano_fit_cloud(gpu_consts('left'), cu(cloud)[rows], cu(faces), init.to(dev())[rows], valid=cu(va)[rows] if valid else None,
                            anchor=None if anchor is None else anchor[rows], anchor_weight=alpha, outer=outer, inner=C.INNER, trim=TRIM, **kw)


@pytest.mark.parametrize('alpha', [0.0, 0.5])
def test_loop_is_its_own_composition(alpha):
    """outer = 0, 1, 2 against F.mano_cloud_targets -> F.mano_fit(target, weight, init, iters = inner) written out by hand: the same kernels
    with the same arguments, so torch.equal."""
    from pdfnet_amd import functional as F
    c = gpu_consts('left')
    _, faces, cloud, va, init, anchor = batch()
    f, cl, va, p, an = cu(faces), cu(cloud), cu(va), init.to(dev()), (cu(anchor) if alpha else None)
    start = F.mano_fit(c, torch.zeros(3, 778, 3, device=dev()), valid=va, init=p, iters=0)
    v, steps = start.verts, []
    for outer in (0, 1, 2):
        got = fit_cloud(outer, anchor=an, alpha=alpha)
        assert got.rms.shape == (outer + 1, 3) and got.inliers.shape == (outer + 1, 3) and got.cost.shape == (outer, 3, 2) and got.info.shape == (outer, 3, 2)
        if outer:
            tg, w, rms, inl = F.mano_cloud_targets(v, f, cl, va, trim=TRIM, anchor=an, anchor_weight=alpha)
            one = F.mano_fit(c, tg, valid=va, weight=w, init=p, iters=C.INNER)
            p, v = torch.cat((one.root, one.pose, one.shape, one.trans), 1), one.verts
            steps.append((rms, inl, one))
        assert torch.equal(got.params, p) and torch.equal(got.verts, v), outer
        assert torch.equal(torch.cat((got.root, got.pose, got.shape, got.trans), 1), got.params)
        last = F.mano_cloud_targets(v, f, cl, va, trim=TRIM, anchor=an, anchor_weight=alpha)
        assert torch.equal(got.rms[outer], last[2]) and torch.equal(got.inliers[outer], last[3])
        for o, (rms, inl, one) in enumerate(steps):
            assert torch.equal(got.rms[o], rms) and torch.equal(got.inliers[o], inl)
            assert torch.equal(got.cost[o], torch.stack((one.cost0, one.cost), 1)) and torch.equal(got.info[o], torch.stack((one.accepted, one.rejected), 1))
        assert torch.equal(got.joints, (steps[-1][2] if steps else start).joints)
        if outer == 0:
            assert torch.equal(got.params, init.to(dev())) and torch.equal(got.verts, start.verts)
        assert torch.equal(got.params[INVALID], init[INVALID].to(dev())) and torch.equal(got.verts[INVALID], start.verts[INVALID])
        assert float(got.rms[:, INVALID].abs().max()) == 0 and int(got.inliers[:, INVALID].abs().max()) == 0
        if outer:
            assert float(got.cost[:, INVALID].abs().max()) == 0 and int(got.info[:, INVALID].abs().max()) == 0
            assert (got.info[:, [0, 2]].sum(-1) == C.INNER).all()


# ---- 4. behaviour on the scene ------------------------------------------------------------------------------
def test_scene_against_the_float64_loop():
    """Row 0 of the batch is the scene of tests/test_mano_fit_cloud_cpu.py; OUTER x INNER = 4 x 3.  The GPU's final rms and its mean
    visible-vertex distance to the generating mesh against the float64 restatement's.  Margin: MULTIPLE = 8 times the deviation that the
    restatement run in float32 on the CPU shows from float64 on this scene (measured here, printed), the multiple the neighbouring MANO-fit
    tests take for a different summation order.  Measured on an MI355X and its host: the float32 CPU run deviates by 7.2e-6 m in the final rms
    and 8.1e-6 m in the visible distance (it accepts other steps than float64 does; on another host the same run accepted nearly the same
    steps and deviated by 4.7e-8 m and 7.4e-8 m, so the margin moves with the host's float32 kernels), the GPU by 6.7e-8 m and 8.5e-8 m: rms
    3.856 -> 1.760 mm against float64's 3.856 -> 1.760 mm.  Independently the final rms is below half the initial one, which the CPU test
    guarantees of the reference."""
    MULTIPLE = 8
    s = C.scene()
    r64, r32 = C.scene_fit(torch.float64), C.scene_fit(torch.float32)
    got = fit_cloud(C.OUTER, rows=slice(0, 1))
    rms = got.rms[:, 0].cpu().double().numpy()
    vis = C.visible_distance(got.verts[0].cpu().numpy(), s)
    v64, v32 = C.visible_distance(r64['verts'].numpy(), s), C.visible_distance(r32['verts'].numpy(), s)
    d_rms, d_vis = abs(r32['rms'][-1] - r64['rms'][-1]), abs(v32 - v64)
    print('rms mm: gpu %s  float64 %s  cpu fp32 %s' % (*(['%.4f' % (1000 * x) for x in y] for y in (rms, r64['rms'], r32['rms'])),))
    print('final rms: |gpu - f64| %.3e m, |cpu fp32 - f64| %.3e m (bar %.3e);  visible distance: gpu %.6f f64 %.6f cpu fp32 %.6f m, '
          '|gpu - f64| %.3e, |cpu fp32 - f64| %.3e (bar %.3e)' % (abs(rms[-1] - r64['rms'][-1]), d_rms, MULTIPLE * d_rms, vis, v64, v32,
                                                                  abs(vis - v64), d_vis, MULTIPLE * d_vis))
    print('inliers gpu %s f64 %s, accepted gpu %s f64 %s' % (got.inliers[:, 0].tolist(), r64['inliers'], got.info[:, 0, 0].tolist(), r64['accepted']))
    assert rms[-1] < 0.5 * rms[0]
    assert abs(rms[-1] - r64['rms'][-1]) <= MULTIPLE * d_rms
    assert abs(vis - v64) <= MULTIPLE * d_vis


# ---- 5. batch independence, determinism, the anchor's hold ---------------------------------------------------
FIELDS = ('params', 'verts', 'joints', 'rms', 'inliers', 'cost', 'info')


def test_rows_alone_and_two_runs_are_bit_identical():
    _, _, _, _, _, anchor = batch()
    an = cu(anchor)
    whole, again = fit_cloud(2, anchor=an, alpha=0.5), fit_cloud(2, anchor=an, alpha=0.5)
    for k in FIELDS:
        assert torch.equal(getattr(whole, k), getattr(again, k)), k
    for b in range(3):
        alone = fit_cloud(2, anchor=an, alpha=0.5, rows=slice(b, b + 1))
        for k in FIELDS:
            x, y = getattr(whole, k), getattr(alone, k)
            assert torch.equal(x[b] if k in FIELDS[:3] else x[:, b], y[0] if k in FIELDS[:3] else y[:, 0]), (b, k)
    free = fit_cloud(2, valid=False, anchor=an, alpha=0.5)                                 # valid = None: every row is fitted
    for k in FIELDS:
        x, y = getattr(whole, k), getattr(free, k)
        assert torch.equal(x[[0, 2]] if k in FIELDS[:3] else x[:, [0, 2]], y[[0, 2]] if k in FIELDS[:3] else y[:, [0, 2]]), k
    assert int(free.inliers[0, INVALID]) > 0 and not torch.equal(free.params[INVALID], whole.params[INVALID])


def test_a_heavy_anchor_holds_the_mesh():
    """anchor = a = M(init), anchor_weight = 1e6: every target t is within eps = trim * W_v / 1e6 of a (W_v <= the largest weight the data
    alone gives; the mesh the targets are made at is a itself, or as close to it as this bound says).  The weights are 1e6 to a part in 1e5,
    and no outer iteration raises its cost, so in the 2-norm over the 778 vertices |M_1 - a| <= |M_1 - t_1| + |t_1 - a| <= 2 sqrt(778) eps
    after the first and |M_2 - a| <= |M_1 - t_2| + |t_2 - a| <= 4 sqrt(778) eps after the second; a vertex moves by no more than that norm,
    plus 4 ulp of a coordinate at 0.5 m (1.2e-7 m)."""
    from pdfnet_amd import functional as F
    verts, faces, cloud, va, init, _ = batch()
    start = fit_cloud(0)
    data = F.mano_cloud_targets(start.verts, cu(faces), cu(cloud), cu(va), trim=TRIM)[1]
    bar = 4 * 778 ** 0.5 * TRIM * float(data.max()) / 1e6 + 1.2e-7
    held, free = fit_cloud(2, anchor=start.verts, alpha=1e6), fit_cloud(2)
    moved = float((held.verts - start.verts).abs().max())
    print('moved %.3e m under the anchor (bar %.3e), %.3e m without' % (moved, bar, float((free.verts - start.verts).abs().max())))
    assert moved <= bar and float((free.verts[0] - start.verts[0]).abs().max()) > 1e-3


# ---- 6. bad arguments ---------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    from pdfnet_amd import functional as F
    from pdfnet_amd.utils import mano_fit_cloud_pair
    c = gpu_consts('left')
    verts, faces, cloud, va, init, anchor = batch()
    v, f, cl, p = cu(verts), cu(faces), cu(cloud), init.to(dev())
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_cloud_targets(v.cpu(), f, cl)
    for kw, what in ((dict(trim=0.0), 'trim'), (dict(trim=float('inf')), 'trim'), (dict(anchor=v, anchor_weight=-1.0), 'anchor_weight'),
                     (dict(anchor=v, anchor_weight=float('nan')), 'anchor_weight'), (dict(anchor=v[:, :777]), 'anchor'), (dict(valid=cu(va)[:2]), 'valid')):
        with pytest.raises(ValueError, match=what):
            F.mano_cloud_targets(v, f, cl, **kw)
    for bad in ((v[0], f, cl), (v, f[None], cl), (v, f, cl[..., :2]), (v[:2], f, cl)):
        with pytest.raises(ValueError, match='verts'):
            F.mano_cloud_targets(*bad)
    big = torch.zeros(1, 1025, 3, device=dev())
    for bad in ((big, f, cl[:1]), (v[:1], torch.zeros(2049, 3, dtype=torch.long, device=dev()), cl[:1]), (v[:1], f, big)):
        with pytest.raises(ValueError, match='1 to 1024'):
            F.mano_cloud_targets(*bad)
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_fit_cloud(c, cl.cpu(), f, p)
    for kw, what in ((dict(outer=-1), 'outer'), (dict(outer=65), 'outer'), (dict(inner=0), 'inner'), (dict(inner=1001), 'inner'), (dict(trim=-1.0), 'trim'),
                     (dict(trim=float('nan')), 'trim'), (dict(prior_pose=-1.0), 'priors'), (dict(side='both'), 'side'), (dict(anchor=v[:, :5]), 'anchor'),
                     (dict(anchor_weight=-0.5), 'anchor_weight'), (dict(valid=cu(va)[:2]), 'valid')):
        with pytest.raises(ValueError, match=what):
            F.mano_fit_cloud(c, cl, f, p, **kw)
    with pytest.raises(ValueError, match='init'):
        F.mano_fit_cloud(c, cl, f, None)
    with pytest.raises(ValueError, match='init'):
        F.mano_fit_cloud(c, cl, f, p[:, :58])
    with pytest.raises(ValueError, match='cloud'):
        F.mano_fit_cloud(c, cl[0], f, p)
    with pytest.raises(ValueError, match='J_regressor'):
        F.mano_fit_cloud({**c, 'J_regressor': c['J_regressor'][:15]}, cl, f, p)
    lbs = {'left': c, 'right': gpu_consts('right')}
    f2, cl2, p2 = torch.stack((f, f)), torch.stack((cl, cl), 1), torch.stack((p, p), 1)
    for bad, what in (((f, cl2, p2), 'faces_pair'), ((f2, cl, p2), 'cloud'), ((f2, cl2, p), 'init_pair'), ((f2, cl2, None), 'init_pair')):
        with pytest.raises(ValueError, match=what):
            mano_fit_cloud_pair(lbs, *bad)
    with pytest.raises(ValueError, match='valid'):
        mano_fit_cloud_pair(lbs, f2, cl2, p2, valid=cu(va))


def test_pair_is_the_two_single_calls():
    from pdfnet_amd import functional as F
    from pdfnet_amd.utils import mano_fit_cloud_pair
    lbs = {side: gpu_consts(side) for side in ('left', 'right')}
    verts, faces, cloud, va, init, anchor = batch()
    fr = C.template_faces('right')
    f2 = torch.stack((cu(faces), cu(fr)))
    cl2, p2, an2 = torch.stack((cu(cloud), cu(cloud[::-1].copy())), 1), torch.stack((init, init.flip(0)), 1).to(dev()), torch.stack((cu(anchor), cu(anchor)), 1)
    valid = torch.tensor([[1.0, 1.0], [0.0, 1.0], [1.0, 0.0]], device=dev())
    pair = mano_fit_cloud_pair(lbs, f2, cl2, p2, valid=valid, anchor=an2, anchor_weight=0.5, outer=2, inner=C.INNER)
    for h, side in enumerate(('left', 'right')):
        one = F.mano_fit_cloud(lbs[side], cl2[:, h], f2[h], p2[:, h], side=side, valid=valid[:, h], anchor=an2[:, h], anchor_weight=0.5, outer=2, inner=C.INNER)
        for k in FIELDS:
            assert torch.equal(getattr(pair[h], k), getattr(one, k)), (side, k)


# ---- 7. evaluation ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluation_runs():
    """The fixture of tests/test_mano_fit_gpu.py::evaluation_runs: R = 128, B = 2, one batch, random-init model, the right hand of sample 0
    invalid; the batch's synthetic clouds are random."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer, cloud_fit_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    res, B = 128, 2
    opt = make_opt(res, size_train=[res, res], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev())
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev()))
    b = synthetic_train_batch(B, res, seed=31, consts=consts)
    b['valid'][0, 1] = 0
    loader = [b]
    lbs = {side: gpu_consts(side) for side in ('left', 'right')}
    runs = {'plain': tr.evaluation(loader), 'off': tr.evaluation(loader, cloud_fit=False), 'on': tr.evaluation(loader, cloud_fit=lbs),
            'others': tr.evaluation(loader, aligned=True, refined=True, mano_fit=lbs),
            'others_on': tr.evaluation(loader, aligned=True, refined=True, mano_fit=lbs, cloud_fit=lbs),
            'interaction': tr.evaluation(loader, interaction=True), 'interaction_on': tr.evaluation(loader, interaction=True, cloud_fit=lbs)}
    with pytest.raises(KeyError, match='cloud'):
        tr.evaluation([{k: v for k, v in b.items() if k != 'cloud'}], cloud_fit=lbs)
    assert m.training
    tr.model_with_loss.eval()
    with torch.no_grad():
        bd = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in b.items()}
        sums = cloud_fit_sums(tr.model_with_loss(bd, 'test', None), bd, tr.model_with_loss.loss.faces_pair, lbs).cpu()
    tr.model_with_loss.train()
    return runs, sums


def test_evaluation_cloud_fit_keys():
    """The plumbing: the flag off changes nothing; the flag on changes no other key, alone or with `aligned`, `refined`, `mano_fit` and with
    `interaction` (whose block is read from the end of the shared buffer); the new keys are finish_cloud_fit of cloud_fit_sums."""
    from pdfnet_amd.trains.base_trainer import CLOUD_FIT_INNER, CLOUD_FIT_KEYS, CLOUD_FIT_OUTER, finish_cloud_fit
    runs, sums = evaluation_runs()
    plain = runs['plain']
    assert plain['samples'] == 2 and runs['off'] == plain and list(runs['off']) == list(plain)
    want = finish_cloud_fit(sums)
    assert list(want) == list(CLOUD_FIT_KEYS) and want['cloud_fit_samples'] == 2
    for base, on in ((plain, runs['on']), (runs['others'], runs['others_on']), (runs['interaction'], runs['interaction_on'])):
        assert sorted(on) == sorted(list(base) + list(CLOUD_FIT_KEYS))
        for k, v in base.items():
            assert on[k] == v, k                                  # bit for bit: the floats come from the same sums
        for k in CLOUD_FIT_KEYS:
            assert np.isfinite(on[k]) and on[k] == want[k], (k, on[k], want[k])
    on = runs['on']
    print({k: on[k] for k in CLOUD_FIT_KEYS})
    assert 0.0 <= on['cloud_fit_inlier_share0'] <= 1.0 and 0.0 <= on['cloud_fit_inlier_share'] <= 1.0
    assert 0.0 <= on['cloud_fit_accepted'] <= CLOUD_FIT_OUTER * CLOUD_FIT_INNER and on['cloud_fit_mpvpe_mm'] > 0 and on['cloud_fit_mpjpe_mm'] > 0
