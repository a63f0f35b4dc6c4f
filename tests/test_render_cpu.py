"""Host side of the hand renderer: the prototypes of pdf_render_hands / pdf_render_compare in the header and their refusals,
vertex_face_table against a numpy loop, the float64 side of the GPU test's inputs (how many pixels are ambiguous), finish_rendered and the
score writer.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT


def test_header_declares_the_renderer_and_it_refuses_before_launching():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["pdf_render_hands"] == (I, [P, P, P, P, P, I, P, I, I, I, I, I, I, Fl, I, P, P, P, P, P, P])
    assert protos["pdf_render_compare"] == (I, [P, P, P, P, I, I, I, I, P, P, P])
    c = hip.lib().cdll

    def hands(B=1, n=778, Fc=1538, M=8, H=64, W=64, z=0.01):
        return c.pdf_render_hands(None, None, None, None, None, 0, None, B, n, Fc, M, H, W, z, 0, None, None, None, None, None, None)
    assert hands(B=0) == 0 and hands(B=-3) == 0 and hands(B=0, n=5000) == 0
    for bad in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(H=0), dict(H=2049), dict(W=0), dict(W=2049), dict(M=0), dict(M=33),
                dict(z=0.0), dict(B=65536), dict()):                 # the last: every size fine, but no vertices and no outputs
        assert hands(**bad) == -1, bad

    def compare(B=1, H=64, W=64, Fc=1538):
        return c.pdf_render_compare(None, None, None, None, B, H, W, Fc, None, None, None)
    assert compare(B=0) == 0 and compare(B=0, Fc=0) == 0
    for bad in (dict(Fc=0), dict(Fc=2049), dict(H=0), dict(H=2049), dict(W=0), dict(W=2049), dict()):
        assert compare(**bad) == -1, bad


def test_vertex_face_table_against_a_loop():
    from pdfnet_amd import functional as F
    from tests.test_render_gpu import template
    faces = template()[2]
    table = F.vertex_face_table(torch.from_numpy(faces), 778)
    assert table.dtype == torch.int32 and table.shape[:2] == (2, 778) and 1 <= table.shape[2] <= 32
    table = table.numpy()
    deg = 0
    for h in range(2):
        for v in range(778):
            want = np.nonzero((faces[h] == v).any(1))[0].tolist()
            row = table[h, v]
            assert row[:len(want)].tolist() == want and (row[len(want):] == -1).all()
            deg = max(deg, len(want))
    assert table.shape[2] == deg
    assert F.vertex_face_table(torch.from_numpy(faces)).shape == table.shape          # n from the largest index
    wider = F.vertex_face_table(torch.from_numpy(faces), 800)
    assert wider.shape[1] == 800 and (wider[:, 778:] == -1).all() and np.array_equal(wider[:, :778].numpy(), table)
    tiny = F.vertex_face_table(torch.tensor([[[0, 1, 2], [2, 2, 1]], [[0, 0, 0], [3, 1, 0]]]))
    assert tiny.tolist() == [[[0, -1], [0, 1], [0, 1], [-1, -1]], [[0, 1], [1, -1], [-1, -1], [1, -1]]]
    fan = torch.tensor([[[0, i + 1, i + 2] for i in range(33)]] * 2)
    for bad in (lambda: F.vertex_face_table(fan), lambda: F.vertex_face_table(torch.from_numpy(faces), 700),
                lambda: F.vertex_face_table(torch.from_numpy(faces[0])), lambda: F.vertex_face_table(torch.tensor([[[0, 1, -1]]] * 2))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_ambiguous_pixels_of_the_gpu_cases_are_few(name):
    """The condition on the inputs of tests/test_render_gpu.py: at most 2 % of a case's covered pixels lie within 1e-3 px of an edge or have
    two covering depths within 1e-6 relative; and an fp32 run of the restatement picks the float64 face on every other pixel."""
    from tests.test_render_gpu import ambiguous_share, case_inputs, case_ref, ref_render, template
    ref = case_ref(name)
    share, covered = ambiguous_share(ref)
    print("  case %s: %d covered pixels, %.2f %% ambiguous, %d depth ties" % (name, covered, 100 * share, ref['ties'].sum()))
    assert share <= 0.02 and covered > 1000 and ref['ties'].sum() == 0
    verts, K, size = case_inputs(name)
    low = ref_render(verts, template()[2], K, size, dt=np.float32)
    ok = ~ref['ambiguous']
    assert np.array_equal(low['face'][ok], ref['face'][ok])
    hit = ok & (ref['face'] >= 0)
    assert (np.abs(low['depth'] - ref['depth'])[hit] <= 1e-5 * ref['depth'][hit]).all() and np.abs(low['bary'] - ref['bary'])[ok].max() <= 2e-4


def test_finish_rendered_on_hand_made_accumulators():
    from pdfnet_amd.trains.base_trainer import RENDERED_KEYS, finish_rendered
    # 5 samples; IoU sums (left, right) over 4 and 2 samples; 0.6 m of residual over 300 pixels
    out = finish_rendered(torch.tensor([5.0, 3.0, 0.5, 4.0, 2.0, 0.6, 300.0, 5.0], dtype=torch.float64))
    assert list(out) == list(RENDERED_KEYS)
    want = {'sil_iou_left': 0.75, 'sil_iou_right': 0.25, 'sil_iou': 0.5, 'depth_res_mm': 2.0, 'rendered_samples': 5}
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-12, (k, out[k], v)
    assert isinstance(out['rendered_samples'], int)
    assert finish_rendered(torch.zeros(8, dtype=torch.float64)) == {'rendered_samples': 0}
    # no depth map, and no sample with a visible left hand: those keys are absent, sil_iou is the hand there is
    out = finish_rendered(torch.tensor([2.0, 0.0, 1.5, 0.0, 2.0, 0.0, 0.0, 0.0], dtype=torch.float64))
    assert out == {'sil_iou_right': 0.75, 'sil_iou': 0.75, 'rendered_samples': 2}
    # depth maps, but the prediction covers no measured pixel: the residual is reported as 0
    out = finish_rendered(torch.tensor([2.0, 0.0, 0.0, 2.0, 2.0, 0.0, 0.0, 2.0], dtype=torch.float64))
    assert out == {'sil_iou_left': 0.0, 'sil_iou_right': 0.0, 'sil_iou': 0.0, 'depth_res_mm': 0.0, 'rendered_samples': 2}


def test_write_rendered_scores_format(tmp_path):
    from pdfnet_amd.trains.base_trainer import RENDERED_KEYS, write_rendered_scores
    ev = {k: 0.12345 * (i + 1) for i, k in enumerate(RENDERED_KEYS)}
    ev['rendered_samples'] = 7
    path = str(tmp_path / 'scores.txt')
    write_rendered_scores(path, ev)
    del ev['depth_res_mm']
    write_rendered_scores(path, ev)                               # appends; an absent key has no line
    block = ['eval rendered ', 'sil_iou_left: 0.12', 'sil_iou_right: 0.25', 'sil_iou: 0.37', 'depth_res_mm: 0.49', 'rendered_samples: 7.00']
    assert open(path).read().splitlines() == block + block[:4] + block[5:]


def test_overlay_is_the_demo_formula():
    from pdfnet_amd.render import HandRenderer
    g = torch.Generator().manual_seed(0)
    img, image = torch.rand(2, 5, 7, 3, generator=g), torch.rand(2, 5, 7, 3, generator=g)
    alpha = (torch.rand(2, 5, 7, generator=g) > 0.5).float()
    over = HandRenderer.overlay(img, alpha, image)
    assert torch.equal(over, img * alpha[..., None] + image * (1 - alpha[..., None]))
    assert torch.equal(over[alpha == 1], img[alpha == 1]) and torch.equal(over[alpha == 0], image[alpha == 0])
