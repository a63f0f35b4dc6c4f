"""Host side of the mesh-to-cloud loss: conditions on the float64 restatement of tests/test_mesh_cloud_loss_gpu.py (its gradient against central
differences of its own loss, the hand-made occlusion cases), the input conditions that the GPU file's comparisons rest on, for every seeded
case there (the ambiguous share under its cap, no matched distance within TRIM_MARGIN of the trim, no two nearest candidates within the band
of the `nn` rule), the arithmetic of finish_two_sided, the prototype of pdf_mesh_cloud_loss in the header with its refusals, and the errors
of F.mesh_cloud_loss and of the training term without a GPU or a cloud."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT

FD_STEP, FD_TOP, FD_BAR = 1e-6, 6, 1e-6                            # metres; vertices per row; of the row's max |grad|.  Measured: <= 2e-10


def rows_of(verts, faces, cloud, valid, trim, margin):
    from tests.test_mesh_cloud_loss_gpu import ref_row
    return {(b, h): ref_row(verts, faces, cloud, valid, b, h, trim, margin) for b in range(verts.shape[0]) for h in range(2)}


def conditions(rows, trim, label):
    """What tests/test_mesh_cloud_loss_gpu.py::check needs of its inputs, whichever way the kernel decides the ambiguous vertices."""
    from tests.test_icp_gpu import TRIM_MARGIN
    from tests.test_mesh_cloud_loss_gpu import AMBIGUOUS_CAP, NN_BAND
    worst = [0.0, np.inf, np.inf]
    for key, r in rows.items():
        share = float((~r['sure_hidden'] & ~r['sure_visible']).mean())
        assert not (r['sure_hidden'] & r['sure_visible']).any() and share <= AMBIGUOUS_CAP, (label, key, share)
        assert not (r['vis'] & r['sure_hidden']).any() and (r['vis'] | ~r['sure_visible']).all(), (label, key)
        may = ~r['sure_hidden'] & np.isfinite(r['d2'])
        if may.any():
            gap = np.abs(np.sqrt(r['d2'][may]) - trim).min()
            tie = (r['second'][may] / np.maximum(r['d2'][may], 1e-300)).min()
            # (2e-8 m: the kernel's match may be NN_BAND farther in squared distance, 0.03 m * 4.8e-7)
            assert gap >= TRIM_MARGIN + 2e-8 and tie > NN_BAND ** 2, (label, key, gap, tie)
            worst = [max(worst[0], share), min(worst[1], gap), min(worst[2], tie)]
    print("  %s: ambiguous share <= %.4f, smallest gap to the trim %.3e m, smallest runner-up / best %.6f" % (label, *worst))


def test_gradient_against_central_differences():
    from tests.test_icp_gpu import TRIM, recovery_rows, template_scene
    from tests.test_mesh_cloud_loss_gpu import MARGIN, ref_row
    verts, _, faces, cloud, valid = template_scene()
    for b, h in recovery_rows():
        base = ref_row(verts, faces, cloud, valid, b, h, TRIM, MARGIN)
        top = np.abs(base['grad']).max()
        assert base['inliers'] > 0 and top > 0
        worst = 0.0
        for i in np.argsort(-np.linalg.norm(base['grad'], axis=-1))[:FD_TOP]:
            for c in range(3):
                ends = []
                for sign in (1.0, -1.0):
                    W = verts.astype(np.float64)
                    W[b, h, i, c] += sign * FD_STEP
                    r = ref_row(W, faces, cloud, valid, b, h, TRIM, MARGIN)
                    assert np.array_equal(r['vis'], base['vis']) and np.array_equal(r['nn'], base['nn']) and np.array_equal(r['inlier'], base['inlier'])
                    ends.append(r['loss'])
                worst = max(worst, abs((ends[0] - ends[1]) / (2 * FD_STEP) - base['grad'][i, c]))
        print("  row (%d, %d): central differences within %.2e of max |grad| = %.3e" % (b, h, worst / top, top))
        assert worst <= FD_BAR * top, (b, h, worst, top)


def test_hand_made_occlusion_cases_in_float64():
    from tests.test_icp_gpu import TET, TRI
    from tests.test_mesh_cloud_loss_gpu import FAR, MARGIN, OCCLUDER, QUAD, TRI_POINTS, TRI_TRIMS, pair, small_facing
    far = (FAR, [0, 1, 2])

    def left(args, valid=None, trim=0.05, margin=MARGIN):
        return rows_of(*args, valid, trim, margin)[(0, 0)]
    p = TRI_POINTS.astype(np.float64)
    d = np.linalg.norm(TRI.astype(np.float64) - p[:3], axis=-1)
    assert np.abs(d - [0.01, 0.02, 0.03]).max() <= 1e-7
    for trim, want in TRI_TRIMS:
        r = left(pair((TRI, [0, 1, 2]), far, TRI_POINTS), trim=trim)
        assert r['vis'].all() and np.array_equal(r['nn'], [0, 1, 2]) and r['inliers'] == want and r['sure_visible'].all()
        m = d < trim
        assert abs(r['loss'] - ((d[m] ** 2).mean() if want else 0.0)) <= 1e-15
        assert np.abs(r['grad'] - np.where(m[:, None], (2.0 / max(want, 1)) * (TRI - p[:3]), 0.0)).max() <= 1e-15
    r = left(pair((TRI, [0, 2, 1]), far, TRI_POINTS))
    assert not r['vis'].any() and r['sure_hidden'].all() and r['loss'] == 0 and (r['nn'] == -1).all()
    both = np.concatenate((TRI, OCCLUDER))
    assert np.array_equal(left(pair((both, [[0, 1, 2], [3, 4, 5]]), far, TRI_POINTS))['vis'], [0, 0, 0, 1, 1, 1])
    assert np.array_equal(left(pair((both, [[0, 1, 2], [3, 5, 4]]), far, TRI_POINTS))['vis'], [1, 1, 1, 0, 0, 0])
    for tris, valid, want in (([0, 1, 2], (1, 1), 0), ([0, 1, 2], (1, 0), 1), ([0, 2, 1], (1, 1), 1)):
        r = left(pair((TRI, [0, 1, 2]), (OCCLUDER, tris), TRI_POINTS), np.array([valid], np.float32))
        assert (r['vis'] == want).all() and (r['sure_visible'] if want else r['sure_hidden']).all()
    for dz, margin, want in ((0.001, 0.002, 1), (0.003, 0.002, 0), (0.001, 0.0, 0), (0.003, 0.0, 0)):
        occ = OCCLUDER.copy()
        occ[:, 2] = 0.5 - dz
        for args in (pair((np.concatenate((TRI, occ)), [[0, 1, 2], [3, 4, 5]]), far, TRI_POINTS), pair((TRI, [0, 1, 2]), (occ, [0, 1, 2]), TRI_POINTS)):
            r = left(args, margin=margin)
            assert (r['vis'][:3] == want).all() and (r['sure_visible'] if want else r['sure_hidden'])[:3].all(), (dz, margin)
    for at in ((0.0625, 0.0625, 0.5), (0.25, 0.25, 0.5), (0.0, 0.0, 0.5), (0.125, 0.125, 0.5)):
        V, tris = small_facing(at)
        for margin in (MARGIN, 0.0):
            same = left(pair((np.concatenate((V, QUAD[0])), np.concatenate((tris, QUAD[1] + 3))), far, TRI_POINTS), margin=margin)
            other = left(pair((V, tris), QUAD, TRI_POINTS), margin=margin)
            assert not same['vis'][0] and not other['vis'][0] and same['vis'][3:7].all(), (at, margin)
            assert not same['sure_hidden'][0] and not same['sure_visible'][0]          # exactly on the edge: neither sure set holds it
        assert left(pair((V, tris), (QUAD[0], QUAD[1][:, ::-1]), TRI_POINTS))['vis'][:3].all()
    r = left(pair(TET, far, TRI_POINTS), trim=0.2, margin=0.0)
    assert r['vis'].all() and r['sure_visible'].all() and r['nn'][0] == 0


def test_input_conditions_of_the_gpu_test():
    from tests.test_icp_gpu import EMPTY, INVALID, TRIM, template_scene
    from tests.test_mesh_cloud_loss_gpu import (GRID_SEEDS, MARGIN, SIZE_SEEDS, SIZE_TRIM, TIGHT_TRIM, grid_case, interacting_pair, size_case)
    for (n, P) in SIZE_SEEDS:
        verts, faces, cloud = size_case(n, P)
        rows = rows_of(verts, faces, cloud, None, SIZE_TRIM, MARGIN)
        conditions(rows, SIZE_TRIM, "n=%d P=%d" % (n, P))
        assert all(not (~r['sure_hidden'] & ~r['sure_visible']).any() for r in rows.values())      # (1 % of 65 vertices is less than one)
        if n > 1:
            assert 0 < rows[(0, 0)]['visible'] < n and rows[(0, 1)]['visible'] == n
    for P in GRID_SEEDS:
        verts, faces, cloud = grid_case(P)
        rows = rows_of(verts, faces, cloud, None, TRIM, MARGIN)
        conditions(rows, TRIM, "grid P=%d" % P)
        assert 0 < rows[(0, 0)]['visible'] < 1024 and rows[(0, 1)]['visible'] == 1024
        assert all(not (~r['sure_hidden'] & ~r['sure_visible']).any() for r in rows.values())
        assert rows[(0, 0)]['inliers'] > 0 and (P == 1 or all(0 < r['inliers'] < r['visible'] for r in rows.values()))
    verts, gt, faces, cloud, valid = template_scene()
    for trim in (TRIM, TIGHT_TRIM):
        rows = rows_of(verts, faces, cloud, valid, trim, MARGIN)
        conditions(rows, trim, "template trim %g" % trim)
        for key, r in rows.items():
            if key in (INVALID, EMPTY):
                assert r['inliers'] == 0 and r['loss'] == 0 and (r['nn'] == -1).all() and (r['visible'] > 0) == (key == EMPTY)
            else:
                share = 1.0 - r['inliers'] / r['visible']
                assert share == 0 if trim == TRIM else 0.05 < share < 0.6, (trim, key, share)
    truth = rows_of(gt.astype(np.float32), faces, cloud, valid, TRIM, MARGIN)
    conditions(truth, TRIM, "template ground truth")
    verts, faces, cloud = interacting_pair()
    rows = rows_of(verts, faces, cloud, None, TRIM, MARGIN)
    conditions(rows, TRIM, "interacting")
    off = np.array([[0, 1]], np.float32)
    solo = rows_of(verts, faces, cloud, off, TRIM, MARGIN)
    conditions(solo, TRIM, "interacting, left hand off")
    by_left = int((solo[(0, 1)]['sure_visible'] & rows[(0, 1)]['sure_hidden']).sum())
    print("  interacting: %d vertices of the right hand are hidden only by the left hand" % by_left)
    assert by_left > 210                                           # (the GPU test asks for 200: at most 1 % of 778 are ambiguous in each run)


def test_finish_two_sided_arithmetic(tmp_path):
    from pdfnet_amd.trains.base_trainer import TWO_SIDED_KEYS, TWO_SIDED_SUMS, finish_two_sided, write_refined_scores, write_two_sided_scores
    assert finish_two_sided(torch.zeros(TWO_SIDED_SUMS, dtype=torch.float64)) == {'two_sided_samples': 0}
    acc = torch.zeros(TWO_SIDED_SUMS, dtype=torch.float64)
    acc[0] = 2                                                     # two samples, no valid hand: every mean is over nothing
    out = finish_two_sided(acc)
    assert list(out) == list(TWO_SIDED_KEYS) and out['two_sided_samples'] == 2 and all(out[k] == 0 for k in TWO_SIDED_KEYS[:-1])
    acc[1:3], acc[13:15] = torch.tensor([0.004, 0.008], dtype=torch.float64), torch.tensor([1.0, 2.0], dtype=torch.float64)          # 12 mm over 3 hands
    acc[3:5], acc[11:13] = torch.tensor([1.0, 1.5], dtype=torch.float64), torch.tensor([2.0, 3.0], dtype=torch.float64)              # 2.5 over 5 valid hands
    acc[5:7], acc[15:17] = torch.tensor([1.5, 1.5], dtype=torch.float64), torch.tensor([2.0, 2.0], dtype=torch.float64)              # 3 over 4 hands with a visible vertex
    acc[7:9], acc[17:19] = torch.tensor([0.001, 0.002], dtype=torch.float64), torch.tensor([1.0, 2.0], dtype=torch.float64)          # 3 mm over 3 hands
    acc[9:11], acc[19:21] = torch.tensor([0.004, 0.006], dtype=torch.float64), torch.tensor([2.0, 3.0], dtype=torch.float64)         # 10 mm over 5 hands
    out = finish_two_sided(acc)
    want = {'mesh_cloud_mm': 4.0, 'gt_mesh_cloud_mm': 1.0, 'cloud_mesh_mm': 2.0, 'chamfer_mm': 3.0, 'visible_share': 0.5, 'covered_share': 0.75,
            'two_sided_samples': 2}
    assert list(out) == list(TWO_SIDED_KEYS) and all(abs(out[k] - want[k]) <= 1e-12 for k in want), out
    path = str(tmp_path / "scores.txt")
    write_refined_scores(path, {'cloud_res_mm': 2.0})
    write_two_sided_scores(path, out)
    lines = open(path).read().splitlines()
    assert lines[:2] == ['eval refined ', 'cloud_res_mm: 2.00'] and lines[2] == 'eval two-sided '
    assert lines[3:] == ['%s: %.2f' % (k, out[k]) for k in TWO_SIDED_KEYS]


def test_header_declares_mesh_cloud_loss_and_the_library_refuses_without_a_launch():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["pdf_mesh_cloud_loss"] == (I, [P, P, P, P, I, I, I, I, Fl, Fl, P, P, P, P, P, P, P])
    c = hip.lib().cdll
    call = lambda B=1, n=778, Fc=1538, P_=1024, trim=0.03, margin=0.002: c.pdf_mesh_cloud_loss(None, None, None, None, B, n, Fc, P_, trim, margin, None,
                                                                                               None, None, None, None, None, None)
    assert call(B=0) == 0 and call(B=-1) == 0
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P_=0), dict(P_=1025), dict(trim=0.0), dict(trim=-1.0),
               dict(trim=float('inf')), dict(trim=float('nan')), dict(margin=-0.001), dict(margin=float('inf')), dict(margin=float('nan')),
               dict()):                                            # the last: no vertices, no outputs
        assert call(**kw) == -1, kw


def test_mesh_cloud_loss_and_the_training_term_need_the_gpu_and_the_cloud():
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.simplified import mesh_cloud_term
    v, f, c = torch.zeros(1, 2, 4, 3, requires_grad=True), torch.zeros(2, 4, 3, dtype=torch.long), torch.zeros(1, 2, 4, 3)
    with pytest.raises(RuntimeError):
        F.mesh_cloud_loss(v, f, c)
    with pytest.raises(RuntimeError):
        F.mesh_cloud_loss(v, f, c, valid=torch.ones(1, 2), return_fields=True)
    batch = {'valid': torch.ones(1, 2), 'K_new': torch.eye(3)[None], 'ind': torch.zeros(1, 2, dtype=torch.long)}
    with pytest.raises(KeyError, match="cloud"):
        mesh_cloud_term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, f, 128)
