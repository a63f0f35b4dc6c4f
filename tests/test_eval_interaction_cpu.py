"""Host side of the inter-hand evaluation metrics: finish_interaction on hand-written accumulators, the score writer, the prototype of
pdf_mesh_penetration in the header and its refusals, and the float64 side of the GPU test's inputs.  No GPU."""
import ctypes
import os

import torch

from tests.util import ROOT


def test_finish_interaction_on_a_hand_made_accumulator():
    from pdfnet_amd.trains.base_trainer import INTERACTION_KEYS, finish_interaction
    # 4 two-handed samples; sums of: MRRPE (m), prediction (share L, share R, depth m, any-inside, gap m), ground truth (the same five)
    acc = torch.tensor([4.0, 0.1, 0.4, 1.2, 0.02, 3.0, 0.008, 0.2, 0.6, 0.004, 1.0, 0.012], dtype=torch.float64)
    out = finish_interaction(acc)
    assert list(out) == list(INTERACTION_KEYS)
    want = {'mrrpe_mm': 25.0, 'pen_ratio_left': 0.1, 'pen_ratio_right': 0.3, 'pen_ratio': 0.2, 'pen_depth_mm': 5.0, 'pen_rate': 0.75,
            'contact_mm': 2.0, 'gt_pen_ratio': 0.1, 'gt_pen_depth_mm': 1.0, 'gt_pen_rate': 0.25, 'gt_contact_mm': 3.0, 'interaction_samples': 4}
    assert set(want) == set(INTERACTION_KEYS)
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-12, (k, out[k], v)
    assert isinstance(out['interaction_samples'], int)


def test_no_two_handed_sample_returns_only_the_count():
    from pdfnet_amd.trains.base_trainer import finish_interaction
    assert finish_interaction(torch.zeros(12, dtype=torch.float64)) == {'interaction_samples': 0}


def test_write_interaction_scores_format(tmp_path):
    from pdfnet_amd.trains.base_trainer import INTERACTION_KEYS, write_interaction_scores
    ev = {k: 1.23456 * (i + 1) for i, k in enumerate(INTERACTION_KEYS)}
    ev['interaction_samples'] = 7
    path = str(tmp_path / 'scores.txt')
    write_interaction_scores(path, ev)
    write_interaction_scores(path, ev)                          # appends
    block = ['eval interaction ', 'mrrpe_mm: 1.23', 'pen_ratio_left: 2.47', 'pen_ratio_right: 3.70', 'pen_ratio: 4.94', 'pen_depth_mm: 6.17',
             'pen_rate: 7.41', 'contact_mm: 8.64', 'gt_pen_ratio: 9.88', 'gt_pen_depth_mm: 11.11', 'gt_pen_rate: 12.35', 'gt_contact_mm: 13.58',
             'interaction_samples: 7.00']
    assert open(path).read().splitlines() == block + block


def test_header_declares_mesh_penetration():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I = ctypes.c_void_p, ctypes.c_int
    assert protos["pdf_mesh_penetration"] == (I, [P, P, I, I, I, P, P, P, P, P, P])
    # an empty batch and refused shapes return before any launch
    c = hip.lib().cdll
    assert c.pdf_mesh_penetration(None, None, 0, 778, 1538, None, None, None, None, None, None) == 0
    assert c.pdf_mesh_penetration(None, None, 1, 1025, 1538, None, None, None, None, None, None) == -1
    assert c.pdf_mesh_penetration(None, None, 1, 778, 2049, None, None, None, None, None, None) == -1
    assert c.pdf_mesh_penetration(None, None, 1, 778, 1538, None, None, None, None, None, None) == -1       # no vertices, no outputs


def test_tetrahedron_inputs_of_the_gpu_test_are_what_its_docstring_says():
    """The float64 side of tests/test_eval_interaction_gpu.py's smallest case: outward faces, one corner of the second solid inside the first."""
    import numpy as np
    from tests.test_eval_interaction_gpu import TET, TET_FACES, ref_penetration, well_conditioned
    verts = np.stack((TET, TET + np.array([0.04, 0.04, -0.04])))[None].astype(np.float32)
    ref = ref_penetration(verts, np.stack((TET_FACES, TET_FACES)))
    assert ref['count'].tolist() == [[0, 1]] and well_conditioned(ref)
    assert np.abs(ref['wind'] - (ref['wind'] > 0.5)).max() < 1e-12
    assert abs(ref['depth'][0, 1] - 0.04 / np.sqrt(3)) < 1e-9     # 40 mm short of the face x + y + z = -50 mm along its normal
