"""Host side of the aligned evaluation metrics: the finishing helper of Trainer.evaluation(aligned=True) on hand-made accumulators, the
score writer, and the two prototypes of csrc/metrics.hip in the header.  No GPU."""
import ctypes
import os

import numpy as np
import torch

from tests.util import ROOT


def _acc(pa=(0.0, 0.0, 0.0, 0.0), f=(0.0, 0.0, 0.0, 0.0)):
    return torch.tensor(list(pa) + list(f), dtype=torch.float64)


def test_finish_aligned_on_hand_made_accumulators():
    from pdfnet_amd.trains.base_trainer import ALIGNED_KEYS, PCK_STEPS, finish_aligned
    n = 4
    table = torch.zeros((21, PCK_STEPS), dtype=torch.int64)
    # sums over 4 samples of per-sample means in metres -> mm; F-score sums -> means
    out = finish_aligned(_acc(pa=(0.004, 0.008, 0.012, 0.02), f=(1.0, 2.0, 3.0, 4.0)), table, n)
    assert set(out) == set(ALIGNED_KEYS)
    want = {'pa_left_joints': 1.0, 'pa_right_joints': 2.0, 'pa_left_verts': 3.0, 'pa_right_verts': 5.0, 'pa_mpjpe_mm': 1.5, 'pa_mpvpe_mm': 4.0,
            'f5_left': 0.25, 'f5_right': 0.5, 'f15_left': 0.75, 'f15_right': 1.0, 'f5': 0.375, 'f15': 0.875, 'auc_joints': 0.0}
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-12, (k, out[k], v)
    # AUC: an all-pass table is 1, an all-fail table 0, a step at threshold k of 100 is the trapezoid area behind it
    assert finish_aligned(_acc(), table + 2 * n, n)['auc_joints'] == 1.0
    assert finish_aligned(_acc(), table, n)['auc_joints'] == 0.0
    step = table.clone()
    step[:, 50:] = 2 * n
    assert abs(finish_aligned(_acc(), step, n)['auc_joints'] - 49.5 / 99) <= 1e-12
    half = table.clone()
    half[:10] = 2 * n                                           # 10 of 21 keypoints always pass: the mean is over keypoints
    assert abs(finish_aligned(_acc(), half, n)['auc_joints'] - 10 / 21) <= 1e-12


def test_fscore_of_a_sample_without_matches_is_zero():
    """F = 2pr / (p + r), and 0 when p + r = 0 (calculate_fscore), from the int32 counts the kernel writes."""
    from pdfnet_amd.trains.base_trainer import fscores
    f = fscores(torch.tensor([[[0, 0], [778, 778]], [[389, 778], [0, 778]]], dtype=torch.int32), 778)
    assert f.dtype == torch.float64 and f.tolist() == [[0.0, 1.0], [2 * 0.5 / 1.5, 0.0]]


def test_empty_loader_returns_only_samples():
    from pdfnet_amd.trains.base_trainer import PCK_STEPS, finish_aligned, finish_evaluation
    out = finish_evaluation(torch.zeros(11, dtype=torch.float64))
    out.update(finish_aligned(_acc(), torch.zeros((21, PCK_STEPS), dtype=torch.int64), out['samples']))
    assert out == {'samples': 0}


def test_pck_thresholds_are_numpys_linspace():
    from pdfnet_amd.trains.base_trainer import pck_thresholds
    assert np.array_equal(pck_thresholds(), np.linspace(0.0, 0.05, 100))
    assert np.array_equal(pck_thresholds(torch.device('cpu')).numpy(), np.linspace(0.0, 0.05, 100))


def test_write_aligned_scores_format(tmp_path):
    from pdfnet_amd.trains.base_trainer import ALIGNED_KEYS, write_aligned_scores
    ev = {k: 1.23456 * (i + 1) for i, k in enumerate(ALIGNED_KEYS)}
    path = str(tmp_path / 'scores.txt')
    write_aligned_scores(path, ev)
    write_aligned_scores(path, ev)                              # appends
    block = ['eval aligned '] + ['%s: %.2f' % (k, ev[k]) for k in ALIGNED_KEYS]
    assert open(path).read().splitlines() == block + block


def test_nearest_neighbour_seeds_pass_the_margin_check_at_the_first_draw():
    """The inputs of the exact count comparison on the GPU: with the committed seeds no float64 nearest-neighbour distance lies within 1e-5 m of
    a threshold and every count is strictly between 0 and n, so the GPU test never has to redraw."""
    from tests.test_eval_aligned_gpu import NN_SEEDS, nn_case
    for (rows, n), seed in NN_SEEDS.items():
        assert nn_case(rows, n)[0] == seed, (rows, n)


def test_header_declares_both_metric_entry_points():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I = ctypes.c_void_p, ctypes.c_int
    assert protos["pdf_procrustes_dist"] == (I, [P, P, I, I, P, P, P, P])
    assert protos["pdf_mesh_nn_counts"] == (I, [P, P, I, I, P, I, P, P, P, P])
    # empty problems and refused shapes return before any launch
    c = hip.lib().cdll
    thr = (ctypes.c_float * 2)(0.005, 0.015)
    assert c.pdf_procrustes_dist(None, None, 0, 21, None, None, None, None) == 0
    assert c.pdf_procrustes_dist(None, None, 2, 0, None, None, None, None) == 0
    assert c.pdf_procrustes_dist(None, None, 1, 1025, None, None, None, None) == -1
    assert c.pdf_mesh_nn_counts(None, None, 0, 21, thr, 2, None, None, None, None) == 0
    assert c.pdf_mesh_nn_counts(None, None, 1, 1025, thr, 2, None, None, None, None) == -1
    assert c.pdf_mesh_nn_counts(None, None, 1, 21, thr, 0, None, None, None, None) == -1
    assert c.pdf_mesh_nn_counts(None, None, 1, 21, thr, 5, None, None, None, None) == -1
