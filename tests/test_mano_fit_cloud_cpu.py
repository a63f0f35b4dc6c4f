"""The float64 restatement of pdf_mano_cloud_targets / pdf_mano_fit_cloud (tests/mano_fit_cloud_ref.py) checked on its own, the scene the GPU
tests share, and the host side of the feature: the declared symbols, the refusals that return before any launch, the evaluation block.
No GPU.  What is asserted here is what makes the restatement a reference: the targets majorise the fixed-association energy with equality at
the mesh they were made at, and on the scene the loop itself at least halves the cloud residual and keeps the points as inliers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import mano_fit_cloud_ref as C
from tests import mano_fit_ref as R
from tests.test_icp_gpu import TRIM
from tests.util import ROOT


def test_template_faces_are_a_closed_surface_oriented_outwards():
    for side in ('left', 'right'):
        f = C.template_faces(side)
        v = R.consts_of(side)['v_template'].numpy()
        assert f.shape == (2 * R.NV - 4, 3) and f.shape[0] <= 2048 and set(f.ravel().tolist()) == set(range(R.NV))
        edges = {(int(t[k]), int(t[(k + 1) % 3])) for t in f for k in range(3)}
        assert len(edges) == 3 * len(f) and all((b, a) in edges for a, b in edges)        # every edge once in each direction
        assert C.signed_volume(v - v.mean(0), f) > 0
        A, B, Cc = (v[f[:, k]] - v.mean(0) for k in range(3))
        assert ((np.cross(A, B) * Cc).sum(-1) > 0).all()                                   # star-shaped: every face sees the centroid from inside


def test_scene_is_as_described():
    s = C.scene()
    assert s['cloud'].shape == (C.SCENE_P, 3) and s['cloud'].dtype == np.float32 and (s['cloud'][:, 2] > 0).all()
    assert 0.40 < s['gt'][:, 2].mean() < 0.50
    d = s['init'].double() - s['p_true']
    assert abs(float(d[58:].norm()) - 0.01) < 1e-6 and float(d[48:58].abs().max()) < 1e-6 and 0.05 < float(d[:48].std()) < 0.15
    t = C.targets(s['gt'], s['faces'], s['cloud'])
    assert t['inliers'] == C.SCENE_P and t['rms'] < 2.5 * C.SCENE_NOISE                   # the cloud lies on the surface it was sampled on


@pytest.mark.parametrize('anchored', [False, True])
def test_targets_majorise_the_fixed_association_energy(anchored):
    """For meshes M around v (1 mm and 1 cm of noise per coordinate): surrogate(M) >= the energy with the association held, with equality at
    M = v to 1e-12 relative; sum_v W_v is the number of inliers; and the merged (target, weight) is the surrogate plus the anchor term up to
    a constant, to 1e-12 of its size."""
    s = C.scene()
    with R.default_dtype(torch.float64):
        V = R.model(R.consts_of('left'), s['init'].double(), 'left')[0].numpy()
    cloud = s['cloud'].astype(np.float64)
    g = np.random.default_rng(5)
    anchor, alpha = (V + 0.003 * g.standard_normal(V.shape), 0.7) if anchored else (None, 0.0)
    t = C.targets(V, s['faces'], cloud, anchor=anchor, alpha=alpha)
    assert t['inliers'] >= 0.9 * C.SCENE_P and abs(t['W'].sum() - t['inliers']) <= 1e-12 * t['inliers']
    E0 = C.association_energy(V, s['faces'], cloud, t)
    assert abs(E0 - t['rms'] ** 2 * t['inliers']) <= 1e-12 * E0
    assert abs(C.surrogate_energy(V, V, t) - E0) <= 1e-12 * E0
    merged = lambda M: float((t['weight'][:, None] * (M - t['target']) ** 2).sum())
    extra = lambda M: alpha * float(((M - anchor) ** 2).sum()) if anchored else 0.0
    const = C.surrogate_energy(V, V, t) + extra(V) - merged(V)
    for scale in (0.001, 0.01):
        for _ in range(8):
            M = V + scale * g.standard_normal(V.shape)
            true, sur = C.association_energy(M, s['faces'], cloud, t), C.surrogate_energy(M, V, t)
            assert sur >= true * (1 - 1e-12), (scale, sur, true)
            assert abs(merged(M) + const - sur - extra(M)) <= 1e-12 * (sur + extra(M)), scale
    off = t['W'] == 0
    assert off.any() and np.array_equal(t['target'][off], anchor[off] if anchored else V[off]) and (t['weight'][off] == alpha).all()


def test_rows_without_data_get_the_anchor_alone():
    s = C.scene()
    V = s['gt']
    a = V + 0.01
    for kw in (dict(valid=0), dict(cloud=np.zeros_like(s['cloud']))):
        args = dict(V=V, faces=s['faces'], cloud=s['cloud'], anchor=a, alpha=2.0)
        args.update(kw)
        t = C.targets(**args)
        assert t['inliers'] == 0 and t['rms'] == 0.0 and (t['tri'] == -1).all() and (t['weight'] == 2.0).all() and np.array_equal(t['target'], a)
        args.update(anchor=None)
        t = C.targets(**args)
        assert (t['weight'] == 0.0).all() and np.array_equal(t['target'], V)


def test_the_restatement_halves_the_residual_on_the_scene():
    """The two conditions on the scene (the seed is chosen so that they hold): in OUTER x INNER = 4 x 3 steps the float64 loop at least halves
    the root mean square inlier distance, and at least 90 % of the points are inliers at the start and at the end."""
    r = C.scene_fit(torch.float64)
    print('rms %s mm, inliers %s, accepted %s' % (['%.3f' % (1000 * x) for x in r['rms']], r['inliers'], r['accepted']))
    assert len(r['rms']) == C.OUTER + 1 and (C.OUTER, C.INNER) == (4, 3)
    assert r['rms'][-1] <= 0.5 * r['rms'][0]
    assert min(r['inliers'][0], r['inliers'][-1]) >= 0.9 * C.SCENE_P
    s = C.scene()
    with R.default_dtype(torch.float64):
        start = R.model(R.consts_of('left'), s['init'].double(), 'left')[0].numpy()
    assert C.visible_distance(r['verts'].numpy(), s) < C.visible_distance(start, s)


def test_an_invalid_row_stays_at_init():
    s = C.scene()
    r = C.fit_cloud(R.consts_of('left'), s['faces'], s['cloud'], s['init'].double(), valid=0, outer=2, inner=3)
    assert torch.equal(r['p'], s['init'].double()) and r['rms'] == [0.0] * 3 and r['inliers'] == [0] * 3 and r['accepted'] == [0, 0]


def test_header_declares_the_three_symbols_and_they_refuse_before_launching():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_long
    assert protos['pdf_mano_cloud_targets'] == (I, [P, P, P, P, P, Fl, I, I, I, I, Fl, P, P, P, P, P, P, P, P])
    assert protos['pdf_mano_fit_cloud_workspace_floats'] == (Lg, [I, I])
    assert protos['pdf_mano_fit_cloud'] == (I, [P, P, P, P, P, Fl, Fl, I, I, Fl, Fl, P, P, P, P, P, I, I, I, I, P, P, P, P, P, P, P, P, P])
    L = hip.lib()
    for name in ('pdf_mano_cloud_targets', 'pdf_mano_fit_cloud_workspace_floats', 'pdf_mano_fit_cloud'):
        fn = getattr(L.cdll, name)
        assert fn.restype is protos[name][0] and list(fn.argtypes) == protos[name][1]
    c = L.cdll
    assert c.pdf_mano_fit_cloud_workspace_floats(0, 8) == 0
    need = c.pdf_mano_fit_cloud_workspace_floats(3, 8)
    assert need >= 3 * (778 * 3 + 778 + 61) and need == c.pdf_mano_fit_cloud_workspace_floats(3, 0)
    one = ctypes.c_void_p(64)                                          # never dereferenced: every call below returns before a launch

    def targets(B=1, n=778, Fc=1552, P_=200, trim=0.03, alpha=0.0, verts=one, out=one):
        return c.pdf_mano_cloud_targets(verts, one, one, None, None, alpha, B, n, Fc, P_, trim, out, one, one, one, None, None, None, None)
    assert targets(B=0) == 0 and targets(B=-1, n=5000) == 0
    for bad in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P_=0), dict(P_=1025), dict(trim=0.0), dict(trim=-1.0),
                dict(trim=float('inf')), dict(trim=float('nan')), dict(alpha=-1.0), dict(alpha=float('inf')), dict(alpha=float('nan')),
                dict(verts=None), dict(out=None)):
        assert targets(**bad) == -1, bad

    def fit(B=1, Fc=1552, P_=200, outer=2, inner=3, trim=0.03, alpha=0.0, pp=0.0, ps=0.0, init=one, ws=one, cost=one):
        return c.pdf_mano_fit_cloud(one, one, None, init, None, alpha, trim, outer, inner, pp, ps, one, one, one, one, one, B, Fc, P_, 1,
                                    one, one, one, one, one, cost, one, ws, None)
    assert fit(B=0) == 0
    for bad in (dict(outer=-1), dict(outer=65), dict(inner=0), dict(inner=1001), dict(trim=0.0), dict(trim=float('nan')), dict(alpha=-1.0),
                dict(pp=-1.0), dict(ps=float('inf')), dict(Fc=0), dict(Fc=2049), dict(P_=0), dict(P_=1025), dict(init=None), dict(ws=None),
                dict(cost=None)):
        assert fit(**bad) == -1, bad


def test_finish_cloud_fit_on_a_hand_made_accumulator():
    from pdfnet_amd.trains.base_trainer import CLOUD_FIT_KEYS, CLOUD_FIT_SUMS, finish_cloud_fit
    assert finish_cloud_fit(torch.zeros(CLOUD_FIT_SUMS, dtype=torch.float64)) == {'cloud_fit_samples': 0}
    #       n   joints      verts       rms0        rms1        share0    share1    accepted  valid  with inlier 0 / 1
    acc = [4, .020, .030, .010, .012, .008, .006, .003, .002, 1.8, 2.4, 1.9, 2.7, 20, 33, 2, 3, 2, 2, 2, 3]
    out = finish_cloud_fit(torch.tensor(acc, dtype=torch.float64))
    assert list(out) == list(CLOUD_FIT_KEYS)
    want = {'cloud_fit_mpjpe_mm': (10.0 + 10.0) / 2, 'cloud_fit_mpvpe_mm': (5.0 + 4.0) / 2, 'cloud_fit_res0_mm': 14.0 / 4, 'cloud_fit_res_mm': 5.0 / 5,
            'cloud_fit_inlier_share0': 4.2 / 5, 'cloud_fit_inlier_share': 4.6 / 5, 'cloud_fit_accepted': 53 / 5, 'cloud_fit_samples': 4}
    for k in CLOUD_FIT_KEYS:
        assert out[k] == pytest.approx(want[k], rel=1e-12), k
    acc[15], acc[17], acc[19] = 0, 0, 0                                # no valid left hand: the means are the right hand's
    acc[1] = acc[3] = acc[5] = acc[7] = acc[9] = acc[11] = acc[13] = 0
    out = finish_cloud_fit(torch.tensor(acc, dtype=torch.float64))
    assert out['cloud_fit_mpjpe_mm'] == pytest.approx(10.0) and out['cloud_fit_res0_mm'] == pytest.approx(3.0)


def test_write_cloud_fit_scores_format(tmp_path):
    from pdfnet_amd.trains.base_trainer import CLOUD_FIT_KEYS, write_cloud_fit_scores
    ev = {k: 0.5 * (i + 1) for i, k in enumerate(CLOUD_FIT_KEYS)}
    path = str(tmp_path / 'scores.txt')
    write_cloud_fit_scores(path, ev)
    write_cloud_fit_scores(path, ev)                                   # appends
    block = ['eval cloud-fit '] + ['%s: %.2f' % (k, ev[k]) for k in CLOUD_FIT_KEYS]
    assert open(path).read().splitlines() == block + block


def test_python_argument_checks_come_before_the_gpu_is_needed_for_nothing():
    """Without a GPU the functions refuse CPU tensors as their neighbours do."""
    from pdfnet_amd import functional as F
    s = C.scene()
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_cloud_targets(torch.from_numpy(s['gt']).float()[None], torch.from_numpy(s['faces']), torch.from_numpy(s['cloud'])[None])
    with pytest.raises(RuntimeError, match='GPU'):
        F.mano_fit_cloud(R.consts_of('left', torch.float32), torch.from_numpy(s['cloud'])[None], torch.from_numpy(s['faces']), s['init'][None])
