"""Host side of the inter-hand penetration loss: conditions on the float64 restatement of tests/test_penetration_loss_gpu.py (its gradient
against central differences of its own loss, the identities that tie it to the penetration metric's restatement, a dented octahedron by hand),
the input conditions of the GPU cases, the prototype of pdf_penetration_loss in the header and its refusals, and the errors of
F.penetration_loss and of the training term without a GPU.

The central differences move ONE coordinate of one vertex by 1e-6 m at a time: the loss is differentiable only where the inside set does not
change, and the test asserts that it does not at either end of every step before it compares."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT

FD_STEP, FD_TOP, FD_BAR = 1e-6, 4, 1e-6                            # metres; vertices per sample; of the sample's max |grad|.  Measured: <= 4e-9


def moved_total(V, W, faces, base, h, i):
    """The restatement's total loss (both rows) and inside sets [2, n] of one sample whose vertices W [2, n, 3] differ from V, the sample `base`
    was computed on, in vertex i of hand h alone -- evaluated incrementally by the restatement's own functions, since a full evaluation
    costs a second: in row h only query i has moved (the other vertices keep their squared distances); in row 1 - h the queries stand
    still and only the triangles at vertex i have moved, so every winding number changes by those triangles' solid angles, new minus old,
    and the closest points of the inside vertices are searched again over the whole moved mesh."""
    from tests.test_cloud_loss_gpu import ref_closest_weights
    from tests.test_eval_interaction_gpu import ref_wind
    from tests.test_penetration_loss_gpu import ref_penetration_row
    n = V.shape[1]
    inside = base['inside'][0].copy()
    d2 = ((V[h] - base['closest'][0, h]) ** 2).sum(-1)
    own = ref_penetration_row(W[h, i:i + 1], W[1 - h], faces[1 - h], with_dist=False)       # (a row of one vertex: its loss is |v - q|^2 / 1)
    inside[h, i], d2[i] = own['inside'][0], own['loss']
    loss_h = d2[inside[h]].sum() / n
    f = np.clip(faces[h], 0, n - 1)
    at = f[(f == i).any(-1)]
    P = V[1 - h]
    wind = base['wind'][0, 1 - h] + ref_wind(P, W[h][at[:, 0]], W[h][at[:, 1]], W[h][at[:, 2]]) - ref_wind(P, V[h][at[:, 0]], V[h][at[:, 1]], V[h][at[:, 2]])
    inside[1 - h] = wind > 0.5
    Q = P[inside[1 - h]]
    q_all, _ = ref_closest_weights(Q[:, None], W[h][f[:, 0]][None], W[h][f[:, 1]][None], W[h][f[:, 2]][None])
    return loss_h + ((Q[:, None] - q_all) ** 2).sum(-1).min(-1).sum() / n, inside


def test_gradient_against_central_differences():
    """d (loss of row (b, 0) + loss of row (b, 1)) / d verts[b] = grad_self + grad_other with the hands swapped, on the two interpenetrating
    template samples, for the 4 vertices of largest gradient of each: vertices that are inside the other hand, and vertices that only receive
    corner gradient from the other hand's inside vertices."""
    from tests.test_eval_interaction_gpu import template_case
    from tests.test_penetration_loss_gpu import ref_penetration_loss, template_reference, total_gradient
    verts, faces, _ = template_case()
    kinds = set()
    for b in (1, 2):
        V = verts[b:b + 1].astype(np.float64)
        base = {k: v[b:b + 1] for k, v in template_reference().items()}
        grad = total_gradient(base)[0]                              # [2, n, 3]
        top = np.abs(grad).max()
        assert (base['count'] > 0).all() and top > 0
        order = np.argsort(-np.linalg.norm(grad, axis=-1).ravel())[:FD_TOP]
        worst = 0.0
        for k, (h, i) in enumerate(zip(*np.unravel_index(order, grad.shape[:2]))):
            kinds.add((bool(base['inside'][0, h, i]), bool((base['grad_other'][0, 1 - h, i] != 0).any())))
            for c in range(3):
                ends = []
                for sign in (1.0, -1.0):
                    W = V.copy()
                    W[0, h, i, c] += sign * FD_STEP
                    loss, inside = moved_total(V[0], W[0], faces, base, h, i)
                    assert np.array_equal(inside, base['inside'][0]), (b, h, i, c)
                    ends.append(loss)
                    if b == 1 and k == 0 and c == 0 and sign > 0:   # the incremental evaluation is the restatement's own total loss
                        full = ref_penetration_loss(W, faces, with_dist=False)
                        assert abs(full['loss'].sum() - loss) <= 1e-17 and np.array_equal(full['inside'][0], inside)
                worst = max(worst, abs((ends[0] - ends[1]) / (2 * FD_STEP) - grad[h, i, c]))
        print("  sample %d: central differences within %.2e of max |grad| = %.3e" % (b, worst / top, top))
        assert worst <= FD_BAR * top, (b, worst, top)
    print("  (inside, receives corner gradient) of the vertices moved: %s" % sorted(kinds))
    assert any(k[1] for k in kinds) and any(k[0] for k in kinds)


def test_identities():
    from tests.test_eval_interaction_gpu import template_case, well_conditioned
    from tests.test_penetration_loss_gpu import ref_penetration_loss, template_reference
    verts, faces, pen = template_case()
    r = template_reference()
    assert well_conditioned(pen)
    assert np.array_equal(r['count'], pen['count']) and np.array_equal(r['wind'], pen['wind']) and r['count'].tolist() == [[0, 0], [121, 131], [180, 80]]
    m = r['inside']
    assert np.abs(r['bary'].sum(-1)[m] - 1).max() <= 1e-12 and (r['bary'] >= 0).all() and (r['bary'] <= 1).all()
    # the corner weights of an inside vertex sum to 1: the term exerts no net force on the pair
    assert np.abs(r['grad_self'].sum(2) + r['grad_other'].sum(2)).max() <= 1e-12
    # the closest point is the surface distance of the metric's restatement
    d = np.linalg.norm(verts.astype(np.float64) - r['closest'], axis=-1)
    assert np.abs(d[m] - pen['dist'][m]).max() <= 1e-12
    assert np.abs(r['loss'] - np.where(m, pen['dist'] ** 2, 0).sum(-1) / 778).max() <= 1e-14
    for k in ('loss', 'grad_self', 'grad_other', 'bary', 'closest'):
        assert (r[k][0] == 0).all(), k                              # the separated sample
    assert (r['tri'][0] == -1).all() and (r['tri'][m] >= 0).all() and (r['tri'][~m] == -1).all()
    # the closest points fall in all three kinds of region
    kinds = [[int(((r['bary'][b, h][m[b, h]] > 0).sum(-1) == k).sum()) for k in (1, 2, 3)] for b in (1, 2) for h in range(2)]
    print("  vertex / edge / face regions per row: %s" % kinds)
    assert kinds == [[1, 15, 105], [1, 23, 107], [8, 41, 131], [0, 12, 68]]
    # a sample with one invalid hand gives zeros and tri = -1
    for valid in ((1, 0), (0, 1), (0, 0)):
        z = ref_penetration_loss(verts[1:2], faces, np.array([valid]))
        assert all((z[k] == 0).all() for k in ('loss', 'count', 'inside', 'bary', 'closest', 'grad_self', 'grad_other')) and (z['tri'] == -1).all()
    on = ref_penetration_loss(verts[1:2], faces, np.array([[1, 1]]), with_dist=False)
    assert all(np.array_equal(on[k], r[k][1:2]) for k in r if k != 'dist')
    # given its own tri the restatement returns itself
    again = ref_penetration_loss(verts[2:], faces, tri=r['tri'][2:], with_dist=False)
    assert all(np.array_equal(again[k], r[k][2:]) for k in r if k != 'dist')


def test_dented_octahedron_by_hand():
    from tests.test_penetration_loss_gpu import (OCT, OCT_BARY, OCT_CLOSEST, OCT_FACES, OCT_INSIDE, OCT_QUERIES, OCT_TRI, octahedron_by_hand,
                                                 octahedron_case, ref_penetration_loss)
    for f in OCT_FACES:                                            # outward: the normal points away from an interior point
        assert np.dot(np.cross(OCT[f[1]] - OCT[f[0]], OCT[f[2]] - OCT[f[0]]), OCT[f].mean(0) - np.array([0, 0, 0.0375])) > 0
    verts, faces = octahedron_case()
    r = ref_penetration_loss(verts, faces)
    row = {k: v[0, 0] for k, v in r.items()}
    assert np.array_equal(row['inside'][:5], OCT_INSIDE) and not row['inside'][5] and r['count'].tolist() == [[3, 0]]
    assert np.abs(row['wind'][:5] - OCT_INSIDE).max() <= 1e-6       # (the float32 corners are up to 2e-9 m off the decimal ones)
    assert np.array_equal(row['tri'][:5], OCT_TRI)                 # the lowest face index among equal distances
    # 1e-8 m, 1e-6: the float32 corners and queries are up to 2e-9 m off the decimal numbers, over 25 mm edges
    assert np.abs(row['closest'][:5] - OCT_CLOSEST).max() <= 1e-8 and np.abs(row['bary'][:5] - OCT_BARY).max() <= 1e-6
    assert np.array_equal(row['bary'][0], [0, 0, 1]) and row['bary'][1, 0] == 0 and (row['bary'][2] > 0.1).all()      # vertex, edge, face
    # the ties are real: the apex is shared by the faces 1, 3, 5, 7, the edge 0-5 by the faces 1 and 7
    from tests.test_cloud_loss_gpu import ref_closest_weights
    V = verts[0, 1].astype(np.float64)
    A, B, C = (V[OCT_FACES[:, k]] for k in range(3))
    q_all, _ = ref_closest_weights(verts[0, 0, :2].astype(np.float64)[:, None], A[None], B[None], C[None])
    d = np.linalg.norm(verts[0, 0, :2].astype(np.float64)[:, None] - q_all, axis=-1)
    assert np.flatnonzero(d[0] <= d[0].min() + 1e-12).tolist() == [1, 3, 5, 7] and np.flatnonzero(d[1] <= d[1].min() + 1e-12).tolist() == [1, 7]
    loss, grad_self, grad_other = octahedron_by_hand()
    assert abs(row['loss'] - loss) <= 1e-10 and np.abs(row['grad_self'] - grad_self).max() <= 1e-8
    assert np.abs(row['grad_other'] - grad_other).max() <= 1e-8 and (row['grad_other'][[2, 3]] == 0).all()
    assert all((r[k][0, 1] == 0).all() for k in ('loss', 'grad_self', 'grad_other', 'inside'))


def test_input_conditions_of_the_gpu_test():
    """The seeded octahedron cases and the padded template case are well conditioned in float64, and hold inside and outside queries."""
    from tests.test_eval_interaction_gpu import template_case, well_conditioned
    from tests.test_penetration_loss_gpu import OCT_TRI, SIZE_SEEDS, caps_case, octahedron_case, overlapping_hands, ref_penetration_loss, tetrahedron_pair
    for n, seed in SIZE_SEEDS.items():
        verts, faces = octahedron_case(n, seed)
        assert verts.shape == (1, 2, n, 3)
        r = ref_penetration_loss(verts, faces)
        print("  octahedron n=%d: inside %s, min |wind - 0.5| %.2e, min dist %.2e m" % (n, r['count'].tolist(), np.abs(r['wind'] - 0.5).min(), r['dist'].min()))
        assert well_conditioned(r) and 10 <= r['count'][0, 0] <= n - 10 and r['count'][0, 1] == 0 and np.array_equal(r['tri'][0, 0, :5], OCT_TRI)
    verts, faces = tetrahedron_pair()
    r = ref_penetration_loss(verts, faces)
    assert well_conditioned(r) and r['count'].tolist() == [[0, 1]]
    i = int(np.argmax(r['inside'][0, 1]))
    assert abs(np.linalg.norm(verts[0, 1, i] - r['closest'][0, 1, i]) - 0.04 / np.sqrt(3.0)) <= 1e-8 and (r['bary'][0, 1, i] > 0.01).all()
    pv, pf = caps_case()
    assert pv.shape == (2, 2, 1024, 3) and pf.shape == (2, 2048, 3)
    pen = template_case()[2]
    rep = np.arange(1024) % 778
    assert well_conditioned({'wind': pen['wind'][1:][..., rep], 'dist': pen['dist'][1:][..., rep]})
    r = ref_penetration_loss(overlapping_hands(), template_case()[1], with_dist=False)      # (the same hands as above, up to the fp32 rounding at z)
    print("  template hands at z = 0.45 m: inside %s, min |wind - 0.5| %.2e" % (r['count'].tolist(), np.abs(r['wind'] - 0.5).min()))
    assert np.abs(r['wind'] - 0.5).min() >= 1e-3 and r['count'].tolist() == [[121, 131], [180, 80], [121, 131]]


def test_header_declares_penetration_loss_and_the_library_refuses_without_a_launch():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I = ctypes.c_void_p, ctypes.c_int
    assert protos["pdf_penetration_loss"] == (I, [P, P, P, I, I, I, P, P, P, P, P, P, P, P, P])
    c = hip.lib().cdll
    call = lambda B=1, n=778, Fc=1538: c.pdf_penetration_loss(None, None, None, B, n, Fc, None, None, None, None, None, None, None, None, None)
    assert call(B=0) == 0 and call(B=-1) == 0
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict()):       # the last: no vertices, no outputs
        assert call(**kw) == -1, kw


def test_penetration_loss_and_the_training_term_need_the_gpu():
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.simplified import cloud_term, mesh_cloud_term, penetration_term
    v, f = torch.zeros(1, 2, 4, 3, requires_grad=True), torch.zeros(2, 4, 3, dtype=torch.long)
    with pytest.raises(RuntimeError):
        F.penetration_loss(v, f)
    with pytest.raises(RuntimeError):
        F.penetration_loss(v, f, valid=torch.ones(1, 2), return_fields=True)
    batch = {'valid': torch.ones(1, 2), 'K_new': torch.eye(3)[None], 'ind': torch.zeros(1, 2, dtype=torch.long)}
    with pytest.raises(RuntimeError):                              # it needs no cloud: it gets as far as the kernel's door
        penetration_term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, f, 128)
    for term in (cloud_term, mesh_cloud_term):                     # the two cloud terms still ask for theirs
        with pytest.raises(KeyError, match="cloud"):
            term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, f, 128)
