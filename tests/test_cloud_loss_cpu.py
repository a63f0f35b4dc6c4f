"""Host side of the cloud-to-mesh loss: conditions on the float64 restatement of tests/test_cloud_loss_gpu.py (its gradient against central
differences of its own loss, the identities that tie it to the ICP restatement, the seven regions of one triangle by hand), the prototype of
pdf_cloud_mesh_loss in the header and its refusals, and the errors of F.cloud_mesh_loss and of the training term without a GPU or a cloud.

The central differences move ONE coordinate of one vertex by 1e-6 m at a time: the loss is differentiable only where the inlier set and the set
of camera-facing triangles do not change, and the test asserts that they do not at either end of every step before it compares (moving all
vertices at once by 1e-6 m carries a point across the trim in one of the rows)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT

FD_STEP, FD_TOP, FD_BAR = 1e-6, 6, 1e-6                            # metres; vertices per row; of the row's max |grad|.  Measured: <= 1.6e-8


def test_gradient_against_central_differences():
    from tests.test_cloud_loss_gpu import ref_cloud_loss_row
    from tests.test_icp_gpu import TRIM, recovery_rows, ref_facing, template_scene
    verts, _, faces, cloud, valid = template_scene()
    rows = recovery_rows()
    assert len(rows) == 4
    for b, h in rows:
        V = verts[b, h].astype(np.float64)
        base = ref_cloud_loss_row(V, faces[h], cloud[b, h], valid[b, h], TRIM)
        facing = ref_facing(V, faces[h])[0] < 0
        top = np.abs(base['grad']).max()
        assert base['inliers'] > 0 and top > 0
        worst = 0.0
        for i in np.argsort(-np.linalg.norm(base['grad'], axis=-1))[:FD_TOP]:
            for c in range(3):
                ends = []
                for sign in (1.0, -1.0):
                    W = V.copy()
                    W[i, c] += sign * FD_STEP
                    r = ref_cloud_loss_row(W, faces[h], cloud[b, h], valid[b, h], TRIM)
                    assert np.array_equal(r['inlier'], base['inlier']) and np.array_equal(ref_facing(W, faces[h])[0] < 0, facing), (b, h, i, c)
                    ends.append(r['loss'])
                worst = max(worst, abs((ends[0] - ends[1]) / (2 * FD_STEP) - base['grad'][i, c]))
        print("  row (%d, %d): central differences within %.2e of max |grad| = %.3e" % (b, h, worst / top, top))
        assert worst <= FD_BAR * top, (b, h, worst, top)


def test_identities_with_the_icp_restatement():
    from tests.test_cloud_loss_gpu import ref_cloud_loss
    from tests.test_icp_gpu import EMPTY, INVALID, TRIM, template_ref, template_scene
    verts, _, faces, cloud, valid = template_scene()
    r = ref_cloud_loss(verts, faces, cloud, valid, TRIM)
    r0, r1 = template_ref(0, False), template_ref(1, False)
    assert np.array_equal(r['tri'], r0['tri']) and np.array_equal(r['inliers'], r0['inliers'])
    mean = np.zeros((3, 2, 3))
    for b in range(3):
        for h in range(2):
            m = r['inlier'][b, h]
            if m.any():
                mean[b, h] = (cloud[b, h].astype(np.float64)[m] - r['closest'][b, h][m]).mean(0)
    assert np.abs(r['grad'].sum(2) + 2 * mean).max() <= 1e-12                       # the weights of a point sum to 1
    assert np.abs(-0.5 * r['grad'].sum(2) - r1['t']).max() <= 1e-12                 # one translation-only ICP step
    assert np.abs(r['loss'] - r0['rms'] ** 2).max() <= 1e-12
    assert np.abs(r['bary'].sum(-1)[r['tri'] >= 0] - 1).max() <= 1e-12 and (r['bary'] >= 0).all() and (r['bary'] <= 1).all()
    for b, h in (INVALID, EMPTY):
        assert r['loss'][b, h] == 0 and r['inliers'][b, h] == 0 and (r['grad'][b, h] == 0).all() and (r['tri'][b, h] == -1).all()
    # given its own tri the restatement returns itself
    again = ref_cloud_loss(verts, faces, cloud, valid, TRIM, tri=r['tri'])
    assert all(np.array_equal(again[k], r[k]) for k in r)


def test_seven_regions_of_one_triangle_by_hand():
    from tests.test_cloud_loss_gpu import REGION_CLOSEST, REGION_TRIMS, REGION_WEIGHTS, ref_cloud_loss_row
    from tests.test_icp_gpu import REGION_QUERIES, TRI
    p = REGION_QUERIES.astype(np.float64)
    d = np.linalg.norm(p - REGION_CLOSEST, axis=-1)
    for trim, want in REGION_TRIMS:
        r = ref_cloud_loss_row(TRI, np.array([[0, 1, 2]]), REGION_QUERIES, 1, trim)
        m = d < trim
        assert (r['tri'] == 0).all() and r['inliers'] == want == m.sum()
        # 1e-7: the float32 0.1 of TRI is 1.5e-9 off
        assert np.abs(r['bary'] - REGION_WEIGHTS).max() <= 1e-7 and np.abs(r['closest'] - REGION_CLOSEST).max() <= 1e-7
        assert np.array_equal(r['bary'][[0, 1, 3]], REGION_WEIGHTS[[0, 1, 3]])
        assert r['bary'][2, 2] == 0 and r['bary'][4, 1] == 0 and r['bary'][5, 0] == 0
        grad = -(2.0 / max(want, 1)) * np.einsum('jk,jc->kc', REGION_WEIGHTS[m], (p - REGION_CLOSEST)[m])
        assert np.abs(r['grad'] - grad).max() <= 1e-7 and abs(r['loss'] - ((d[m] ** 2).mean() if want else 0.0)) <= 1e-7
    flipped = ref_cloud_loss_row(TRI, np.array([[0, 2, 1]]), REGION_QUERIES, 1, 0.05)
    assert flipped['loss'] == 0 and flipped['inliers'] == 0 and (flipped['grad'] == 0).all() and (flipped['tri'] == -1).all()


def test_input_conditions_of_the_gpu_test():
    """No point of the size cases lies within TRIM_MARGIN of the trim in float64, and the grid's trim rejects something."""
    from tests.test_cloud_loss_gpu import GRID_SEEDS, grid_mesh, ref_cloud_loss
    from tests.test_icp_gpu import TRIM, TRIM_MARGIN, ref_facing
    V, tris = grid_mesh()
    assert V.shape == (1024, 3) and tris.shape == (2048, 3) and (ref_facing(V.astype(np.float64), tris)[0] < 0).sum() == 1922
    assert (tris[1922:, 0] == tris[1922:, 1]).all()
    for P, seed in GRID_SEEDS.items():
        g = np.random.default_rng(seed)
        pts = np.concatenate((g.uniform(-0.1, 0.1, (P, 2)), g.uniform(0.46, 0.54, (P, 1))), -1).astype(np.float32)
        verts, faces, cloud = np.stack((V, V + [0.002, 0, 0.003]))[None].astype(np.float32), np.stack((tris, tris)), np.stack((pts, pts[::-1]))[None]
        r = ref_cloud_loss(verts, faces, cloud, None, TRIM)
        assert (r['tri'] >= 0).all() and np.abs(r['dist'] - TRIM).min() >= TRIM_MARGIN, (P, np.abs(r['dist'] - TRIM).min())
        assert (r['inliers'] > 0).all() and (P == 1 or (r['inliers'] < P).all())


def test_header_declares_cloud_mesh_loss_and_the_library_refuses_without_a_launch():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["pdf_cloud_mesh_loss"] == (I, [P, P, P, P, I, I, I, I, Fl, P, P, P, P, P, P, P])
    c = hip.lib().cdll
    call = lambda B=1, n=778, Fc=1538, P_=1024, trim=0.03: c.pdf_cloud_mesh_loss(None, None, None, None, B, n, Fc, P_, trim, None, None, None, None,
                                                                                 None, None, None)
    assert call(B=0) == 0 and call(B=-1) == 0
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P_=0), dict(P_=1025), dict(trim=0.0), dict(trim=-1.0),
               dict(trim=float('inf')), dict(trim=float('nan')), dict()):                     # the last: no vertices, no outputs
        assert call(**kw) == -1, kw


def test_cloud_mesh_loss_and_the_training_term_need_the_gpu_and_the_cloud():
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.simplified import cloud_term
    v, f, c = torch.zeros(1, 2, 4, 3, requires_grad=True), torch.zeros(2, 4, 3, dtype=torch.long), torch.zeros(1, 2, 4, 3)
    with pytest.raises(RuntimeError):
        F.cloud_mesh_loss(v, f, c)
    with pytest.raises(RuntimeError):
        F.cloud_mesh_loss(v, f, c, valid=torch.ones(1, 2), return_fields=True)
    batch = {'valid': torch.ones(1, 2), 'K_new': torch.eye(3)[None], 'ind': torch.zeros(1, 2, dtype=torch.long)}
    with pytest.raises(KeyError, match="cloud"):
        cloud_term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, f, 128)
