"""Host side of the ICP refinement: the float64 restatement's own pieces (Kabsch with the determinant correction, the degenerate step), the two
conditions on the GPU test's inputs, finish_refined on hand-written accumulators, the score writer, the prototype of pdf_mesh_icp in the header
and its refusals.  No GPU.

The input conditions are conditions on the restatement, not measurements of the kernel: (1) no cloud point lies within TRIM_MARGIN of the trim
in any association of any case, so an exact comparison of `inliers` is well-posed; (2) on every recovery case the restatement itself at least
halves the mean vertex error.  A recovery case is a displaced, valid hand with a cloud, refined with the full iters = 8, in either mode: iters = 0
moves nothing and a single step (iters = 1) recovers about a quarter of these displacements, so those two are compared with the restatement
only; the invalid hand and the all-zero cloud are not moved at all."""
import ctypes
import os

import numpy as np
import torch

from tests.util import ROOT


def test_kabsch_returns_a_known_rigid_transform():
    from tests.test_icp_gpu import ref_kabsch, rotation
    g = np.random.default_rng(0)
    q = g.normal(0, 0.05, (40, 3)) + [0.0, 0.0, 0.5]
    R, t = rotation((1, -2, 0.5), 23.0), np.array([0.01, -0.02, 0.03])
    Rk, tk, full = ref_kabsch(q, q @ R.T + t)
    assert full and np.abs(Rk - R).max() <= 1e-12 and np.abs(tk - t).max() <= 1e-12 and abs(np.linalg.det(Rk) - 1) <= 1e-12


def test_kabsch_mirrored_configuration_needs_the_determinant_correction():
    """A planar set and its mirror image: the best orthogonal map is a reflection (det = -1); the proper rotation that Kabsch must return
    instead maps the plane onto itself the other way round."""
    from tests.test_icp_gpu import ref_kabsch
    g = np.random.default_rng(1)
    q = g.normal(0, 0.05, (30, 3))
    p = q * [1.0, 1.0, -1.0]                                       # mirrored in z; the spread in z is the smallest
    q[:, 2] *= 0.1
    p[:, 2] *= 0.1
    U, S, Vt = np.linalg.svd((q - q.mean(0)).T @ (p - p.mean(0)))
    assert np.linalg.det(Vt.T @ U.T) < 0                           # without the correction: a reflection
    R, t, full = ref_kabsch(q, p)
    assert full and abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
    res = np.linalg.norm(q @ R.T + t - p, axis=-1)
    # no rotation does better: compare with the identity and with 2,000 random rotations about the optimum
    best = (res ** 2).sum()
    assert best <= (np.linalg.norm(q - q.mean(0) + p.mean(0) - p, axis=-1) ** 2).sum() + 1e-15
    from tests.test_icp_gpu import rotation
    for _ in range(200):
        Rn = rotation(g.normal(size=3), g.uniform(-5, 5)) @ R
        tn = p.mean(0) - Rn @ q.mean(0)
        assert (np.linalg.norm(q @ Rn.T + tn - p, axis=-1) ** 2).sum() >= best - 1e-15


def test_collinear_cloud_takes_the_translation_only_step():
    from tests.test_icp_gpu import ref_kabsch
    q = np.outer(np.linspace(-1, 1, 9), [0.03, 0.01, 0.02]) + [0.0, 0.0, 0.5]
    p = q + [0.004, -0.002, 0.001]
    R, t, full = ref_kabsch(q, p)
    assert not full and np.array_equal(R, np.eye(3)) and np.abs(t - [0.004, -0.002, 0.001]).max() <= 1e-15
    same = ref_kabsch(q[:1].repeat(5, 0), p[:1].repeat(5, 0))       # rank 0
    assert not same[2] and np.array_equal(same[0], np.eye(3))


def test_input_conditions_of_the_gpu_test():
    from tests.test_icp_gpu import (EMPTY, INVALID, P_TEMPLATE, TRIM, TRIM_MARGIN, mean_vertex_error, recovery_rows, template_ref,
                                    template_scene)
    verts, gt, faces, cloud, valid = template_scene()
    assert valid[INVALID] == 0 and (cloud[EMPTY] == 0).all() and cloud.shape == (3, 2, P_TEMPLATE, 3)
    before = mean_vertex_error(verts, gt)
    assert 0.010 <= before.min() and before.max() <= 0.025
    trimmed = False
    for iters in (0, 1, 8):
        for rigid in (False, True):
            ref = template_ref(iters, rigid)
            assert ref['margin'].min() >= TRIM_MARGIN, (iters, rigid, ref['margin'].min())
            after = mean_vertex_error(ref['out'], gt)
            for b, h in recovery_rows():
                assert ref['steps'][b, h] == iters and 0 < ref['inliers'][b, h]
                trimmed |= ref['inliers'][b, h] < P_TEMPLATE
                if iters == 8:
                    assert after[b, h] <= 0.5 * before[b, h], (rigid, b, h, before[b, h], after[b, h])
            for b, h in (INVALID, EMPTY):
                assert ref['steps'][b, h] == 0 and ref['inliers'][b, h] == 0 and np.array_equal(ref['out'][b, h], verts[b, h].astype(np.float64))
    assert trimmed                                                # the trim rejects something in these clouds
    # the noiseless, undisplaced scene lies on the surface
    v0, _, _, c0, va = template_scene(noise=0.0, displaced=False)
    from tests.test_icp_gpu import ref_icp
    flat = ref_icp(v0, faces, c0, va, 0, TRIM)
    assert flat['rms'].max() <= 1e-7 and flat['inliers'].sum() == 4 * P_TEMPLATE


def test_finish_refined_on_a_hand_made_accumulator():
    from pdfnet_amd.trains.base_trainer import REFINED_KEYS, REFINED_SUMS, finish_refined
    # 5 samples, the left hand valid in 4 and the right in 2; sums (left, right) of: joint error, vertex error (m), residual before, after (m),
    # inlier share, valid samples, samples with an inlier before, after
    acc = torch.tensor([5.0, 0.04, 0.03, 0.06, 0.02, 0.027, 0.013, 0.009, 0.003, 3.2, 1.0, 4.0, 2.0, 3.0, 1.0, 3.0, 1.0], dtype=torch.float64)
    assert acc.numel() == REFINED_SUMS
    out = finish_refined(acc)
    assert list(out) == list(REFINED_KEYS)
    want = {'ref_abs_left_joints': 10.0, 'ref_abs_right_joints': 15.0, 'ref_abs_left_verts': 15.0, 'ref_abs_right_verts': 10.0, 'ref_mpjpe_mm': 12.5,
            'ref_mpvpe_mm': 12.5, 'cloud_res_mm': 10.0, 'ref_cloud_res_mm': 3.0, 'ref_inlier_share': 0.7, 'refined_samples': 5}
    assert set(want) == set(REFINED_KEYS)
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-12, (k, out[k], v)
    assert isinstance(out['refined_samples'], int)
    # a hand that is never valid: its figures are 0 and the means are the other hand's; no inlier at all: residual 0
    acc[[2, 4, 6, 8, 10, 12, 14, 16]] = 0
    acc[[13, 15]] = 0
    out = finish_refined(acc)
    assert out['ref_abs_right_joints'] == 0 and out['ref_mpjpe_mm'] == out['ref_abs_left_joints'] and out['ref_mpvpe_mm'] == out['ref_abs_left_verts']
    assert out['cloud_res_mm'] == 0 and out['ref_cloud_res_mm'] == 0 and abs(out['ref_inlier_share'] - 0.8) <= 1e-12


def test_no_sample_returns_only_the_count():
    from pdfnet_amd.trains.base_trainer import REFINED_SUMS, finish_refined
    assert finish_refined(torch.zeros(REFINED_SUMS, dtype=torch.float64)) == {'refined_samples': 0}


def test_write_refined_scores_appends_its_own_block(tmp_path):
    from pdfnet_amd.trains.base_trainer import REFINED_KEYS, RENDERED_KEYS, write_h2o_scores, write_refined_scores, write_rendered_scores
    ev = {'%s_%s_%s' % (kind, hand, what): 1.0 for kind in ('abs', 'off') for hand in ('left', 'right') for what in ('joints', 'verts')}
    ev.update({k: 0.5 for k in RENDERED_KEYS})
    ev.update({k: 1.23456 * (i + 1) for i, k in enumerate(REFINED_KEYS)})
    ev['refined_samples'] = 7
    path = str(tmp_path / 'H2O-val.txt')
    write_h2o_scores(path, ev)
    write_rendered_scores(path, ev)
    before = open(path).read()
    write_refined_scores(path, ev)
    text = open(path).read()
    assert text.startswith(before)
    assert text[len(before):].splitlines() == ['eval refined '] + ['%s: %.2f' % (k, ev[k]) for k in REFINED_KEYS]
    assert text[len(before):].splitlines()[1] == 'ref_abs_left_joints: 1.23' and text.splitlines()[-1] == 'refined_samples: 7.00'


def test_header_declares_mesh_icp_and_the_library_refuses_without_a_launch():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["pdf_mesh_icp"] == (I, [P, P, P, P, I, I, I, I, I, Fl, I, P, P, P, P, P, P, P, P])
    c = hip.lib().cdll
    call = lambda B=1, n=778, Fc=1538, P_=1024, iters=8, trim=0.03: c.pdf_mesh_icp(None, None, None, None, B, n, Fc, P_, iters, trim, 0, None, None,
                                                                                   None, None, None, None, None, None)
    assert call(B=0) == 0
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P_=0), dict(P_=1025), dict(iters=-1), dict(iters=65), dict(trim=0.0),
               dict(trim=float('inf')), dict(trim=float('nan')), dict()):                     # the last: no vertices, no outputs
        assert call(**kw) == -1, kw


def test_mesh_icp_and_refined_need_the_gpu_and_the_cloud():
    import pytest
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.base_trainer import refined_sums
    v, f, c = torch.zeros(1, 2, 4, 3), torch.zeros(2, 4, 3, dtype=torch.long), torch.zeros(1, 2, 4, 3)
    with pytest.raises(RuntimeError):
        F.mesh_icp(v, f, c)
    z = torch.zeros(1, 2, 21, 3)
    with pytest.raises(KeyError, match="cloud"):
        refined_sums((v, z, v, z, z, z, z, z, z), {'valid': torch.ones(1, 2)}, f)
