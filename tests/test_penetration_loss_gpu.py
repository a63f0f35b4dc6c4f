"""The differentiable inter-hand penetration loss on the GPU (csrc/penetration.hip pdf_penetration_loss, F.penetration_loss, CtdetLoss's
penetration_weight term) against a float64 numpy restatement of the contract in include/pdfnet_hip.h, built from the two restatements the
kernel's cores already have: `ref_wind` (tests/test_eval_interaction_gpu.py: the generalized winding number) decides which vertices of a hand
are inside the other hand, and `ref_closest_weights` (tests/test_cloud_loss_gpu.py: the seven regions with the corner weights) gives their
closest points q = w_a a + w_b b + w_c c on the other hand's surface.  loss = (1/n) sum |v - q|^2; an inside vertex receives (2/n)(v - q) and
corner k of its triangle -(2/n) w_k (v - q) (the envelope theorem); tests/test_penetration_loss_cpu.py checks that against central differences
of the restatement's own loss.

`ref_penetration_loss` evaluates every inside vertex either on its float64 arg-min triangle or, given `tri`, on the triangle the kernel chose:
on the template hands 10 to 40 inside vertices per row are exactly equidistant from two or more triangles (their closest point lies on a shared
edge or vertex); q and the gradients do not depend on the choice, tri and bary do.  The continuous outputs are compared GIVEN the kernel's tri,
after the test has asserted that the chosen triangle is as near as the float64 minimum over all triangles (DISCRETE_BAR).

BARS come from the float64 side of each row, never from the kernel's errors (those are printed; profiles/NOTES.md has them).  With
    D = the largest |v - q| of an inside vertex, m = the inside count, a = the smallest altitude of a matched triangle,
    T = the largest number of inside vertices whose triangle touches one corner,
and q within DISCRETE_BAR = 1e-6 m (tests/test_icp_gpu.py):
    closest 1e-6 m            bary dw = 1e-6 / a (a weight is a ratio of lengths across the triangle)
    loss (m/n) 2 D 1e-6       grad_self (2/n) 1e-6           grad_other (2/n) T (dw D + 1e-6)
Every comparison of `inside` or `count` first asserts on the float64 side `well_conditioned`: |wind - 0.5| >= 1e-3 everywhere and no vertex within
1e-7 m of the other surface.  That is a condition on the inputs: no vertex is excluded."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_cloud_loss_gpu import GRAD_NOISE_BAR, gradient_distance, ref_closest_weights, train_step, trainer_fixture
from tests.test_eval_interaction_gpu import SHIFTS, TET, TET_FACES, hands, ref_row, ref_wind, template_case, well_conditioned
from tests.test_icp_gpu import DISCRETE_BAR, cu

pytestmark = pytest.mark.gpu

KEYS = ('loss', 'count', 'inside', 'tri', 'bary', 'closest')


# ---- float64 restatement -----------------------------------------------------------------------
def ref_penetration_row(P, V, faces, tri=None, with_dist=True):
    """Vertices P [n, 3] of one hand against the other hand's mesh (V [n, 3], faces [F, 3]) in float64 -> dict: loss, count, inside [n] bool,
    tri [n] (-1: not inside), bary, closest [n, 3], grad_self [n, 3] (on P), grad_other [n, 3] (on V), and wind, dist [n] of every vertex
    (dist, which only `well_conditioned` needs, is NaN without with_dist).
    tri: evaluate every inside vertex on that triangle instead of the float64 arg-min (the lowest index among equal distances)."""
    P, V = np.asarray(P, np.float64), np.asarray(V, np.float64)
    n = len(P)
    faces = np.clip(faces, 0, len(V) - 1)
    if with_dist:
        wind, dist = ref_row(P, V, faces)
    else:
        wind, dist = ref_wind(P, V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]), np.full(n, np.nan)
    inside = wind > 0.5
    out = {'loss': 0.0, 'count': int(inside.sum()), 'inside': inside, 'tri': np.full(n, -1, np.int64), 'bary': np.zeros((n, 3)),
           'closest': np.zeros((n, 3)), 'grad_self': np.zeros((n, 3)), 'grad_other': np.zeros_like(V), 'wind': wind, 'dist': dist}
    if not inside.any():
        return out
    A, B, C = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    Q = P[inside]
    if tri is None:
        q_all, _ = ref_closest_weights(Q[:, None], A[None], B[None], C[None])
        t = np.linalg.norm(Q[:, None] - q_all, axis=-1).argmin(-1)
    else:
        t = np.asarray(tri, np.int64)[inside]
        assert (t >= 0).all() and (t < len(faces)).all()
    q, w = ref_closest_weights(Q, A[t], B[t], C[t])
    r = Q - q
    out['tri'][inside], out['bary'][inside], out['closest'][inside] = t, w, q
    out['loss'] = float((r ** 2).sum() / n)
    out['grad_self'][inside] = (2.0 / n) * r
    for c in range(3):
        np.add.at(out['grad_other'], faces[t, c], -(2.0 / n) * w[:, c:c + 1] * r)
    return out


def zero_row(n):
    """A row that is not live (dist = inf: it has no surface to be near)."""
    return {'loss': 0.0, 'count': 0, 'inside': np.zeros(n, bool), 'tri': np.full(n, -1, np.int64), 'bary': np.zeros((n, 3)),
            'closest': np.zeros((n, 3)), 'grad_self': np.zeros((n, 3)), 'grad_other': np.zeros((n, 3)), 'wind': np.zeros(n), 'dist': np.full(n, np.inf)}


def ref_penetration_loss(verts, faces, valid=None, tri=None, with_dist=True):
    """verts [B, 2, n, 3], faces [2, F, 3], valid [B, 2] or None, tri [B, 2, n] or None -> dict of stacked float64 arrays ([B, 2, ...]).  Row
    (b, h) is hand h's vertices against hand 1 - h's mesh; grad_other of row (b, h) is indexed by hand 1 - h's vertices.  A sample that lacks a
    valid hand gives zeros and tri = -1."""
    rows = [[ref_penetration_row(verts[b, h], verts[b, 1 - h], faces[1 - h], None if tri is None else tri[b, h], with_dist)
             if valid is None or (valid[b] != 0).all() else zero_row(verts.shape[2]) for h in range(2)] for b in range(verts.shape[0])]
    return {k: np.array([[r[k] for r in pair] for pair in rows]) for k in rows[0][0]}


@functools.lru_cache(maxsize=None)
def template_reference():
    """The restatement of `template_case()`, computed once and left unchanged; the distances of every vertex are the metric's restatement's."""
    verts, faces, pen = template_case()
    ref = ref_penetration_loss(verts, faces, with_dist=False)
    assert np.array_equal(ref['wind'], pen['wind'])
    ref['dist'] = pen['dist']
    return ref


def total_gradient(ref):
    """d (sum of both rows' losses) / d verts [B, 2, n, 3]: the formula of F.penetration_loss's backward with g = 1."""
    return ref['grad_self'] + ref['grad_other'][:, ::-1]


def bars(ref, verts, faces):
    """The bars of the module docstring, per row -> dict of [B, 2] arrays (a row without an inside vertex: all 0), and D, m, a, T."""
    Bn, _, n, _ = verts.shape
    out = {k: np.zeros((Bn, 2)) for k in ('closest', 'bary', 'loss', 'grad_self', 'grad_other', 'D', 'm', 'a', 'T')}
    for b in range(Bn):
        for h in range(2):
            m = ref['inside'][b, h]
            if not m.any():
                continue
            V, f = verts[b, 1 - h].astype(np.float64), np.clip(faces[1 - h], 0, n - 1)[ref['tri'][b, h][m]]
            D = np.linalg.norm(verts[b, h].astype(np.float64)[m] - ref['closest'][b, h][m], axis=-1).max()
            A, B, C = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
            area2 = np.linalg.norm(np.cross(B - A, C - A), axis=-1)
            longest = np.maximum(np.maximum(np.linalg.norm(B - A, axis=-1), np.linalg.norm(C - A, axis=-1)), np.linalg.norm(C - B, axis=-1))
            assert (area2 > 0).all(), (b, h)                      # no matched triangle is degenerate
            a = (area2 / longest).min()
            T = np.bincount(np.concatenate([np.unique(row) for row in f]), minlength=n).max()      # (a face with a repeated corner counts once)
            dw = DISCRETE_BAR / a
            out['D'][b, h], out['m'][b, h], out['a'][b, h], out['T'][b, h] = D, m.sum(), a, T
            out['closest'][b, h], out['bary'][b, h] = DISCRETE_BAR, dw
            out['loss'][b, h] = m.sum() / n * 2 * D * DISCRETE_BAR
            out['grad_self'][b, h] = 2.0 / n * DISCRETE_BAR
            out['grad_other'][b, h] = 2.0 / n * T * (dw * D + DISCRETE_BAR)
    return out


# ---- running and comparing -----------------------------------------------------------------------
def run(verts, faces, valid=None, g=None):
    """-> the fields of F.penetration_loss as numpy arrays, 'grad' = verts.grad after (loss * g).sum().backward() (g = 1 by default), and the
    kernel's own two gradient tensors 'grad_self', 'grad_other'."""
    from pdfnet_amd import functional as F
    v = cu(verts).requires_grad_()
    got = F.penetration_loss(v, cu(faces), None if valid is None else cu(valid), return_fields=True)
    (got[0] * (torch.ones_like(got[0]) if g is None else cu(g))).sum().backward()
    torch.cuda.synchronize()
    out = {k: x.detach().cpu().numpy() for k, x in zip(KEYS, got)}
    out['grad'] = v.grad.cpu().numpy()
    out['grad_self'], out['grad_other'] = raw_gradients(verts, faces, valid)
    return out


def raw_gradients(verts, faces, valid=None):
    """The kernel's grad_self and grad_other through the C ABI, every other optional output NULL."""
    from pdfnet_amd import hip
    v, f = cu(verts), cu(faces)
    va = None if valid is None else cu(valid)
    Bn, _, n, _ = verts.shape
    loss, count = torch.empty(Bn, 2, device='cuda'), torch.empty(Bn, 2, dtype=torch.int32, device='cuda')
    gs, go = torch.full_like(v, 7.0), torch.full_like(v, 7.0)
    hip.lib().pdf_penetration_loss(v.data_ptr(), f.data_ptr(), None if va is None else va.data_ptr(), Bn, n, faces.shape[1], loss.data_ptr(),
                                   count.data_ptr(), gs.data_ptr(), go.data_ptr(), None, None, None, None, None)
    torch.cuda.synchronize()
    return gs.cpu().numpy(), go.cpu().numpy()


def check_against_the_restatement(got, verts, faces, valid, label, free=None):
    """All fields against the restatement given the kernel's tri, with the derived bars; inside and count exactly (after `well_conditioned`).
    free: the restatement of these inputs on its own arg-min triangles, where the caller has it.
    -> (the restatement given the kernel's tri, the bars)."""
    free = ref_penetration_loss(verts, faces, valid) if free is None else free
    live = np.isfinite(free['dist']).all(-1)
    assert not live.any() or well_conditioned({'wind': free['wind'][live], 'dist': free['dist'][live]}), label
    assert np.array_equal(got['inside'] != 0, free['inside']) and np.array_equal(got['count'], free['count']), (label, got['count'], free['count'])
    assert np.array_equal(got['tri'] >= 0, free['inside']), label
    ref = ref_penetration_loss(verts, faces, valid, tri=got['tri'], with_dist=False)
    bar = bars(ref, verts, faces)
    assert all(np.isfinite(v).all() for v in got.values()), label
    # the chosen triangle is as near as the float64 minimum over all triangles
    m = ref['inside']
    d_given = np.linalg.norm(verts.astype(np.float64) - ref['closest'], axis=-1)
    assert not m.any() or np.abs(d_given[m] - free['dist'][m]).max() <= DISCRETE_BAR, label
    err = {}
    for k, nd in (('loss', 0), ('closest', 2), ('bary', 2), ('grad_self', 2), ('grad_other', 2)):
        e = np.abs(got[k].astype(np.float64) - ref[k])
        err[k] = e.reshape(e.shape[:2] + (-1,)).max(-1) if nd else e
    print("  %s D %s mm, m %s, a %s mm, T %s" % (label, (bar['D'] * 1e3).round(2).tolist(), bar['m'].astype(int).tolist(),
                                                   (bar['a'] * 1e3).round(3).tolist(), bar['T'].astype(int).tolist()))
    for k, e in err.items():
        print("  %s %-10s max err %s bar %s (max |ref| %.3e)" % (label, k, ["%.2e" % x for x in e.ravel()], ["%.2e" % x for x in bar[k].ravel()],
                                                               np.abs(ref[k]).max()))
    for k, e in err.items():
        assert (e <= bar[k]).all(), (label, k, e, bar[k])
    assert (got['bary'] >= 0).all() and (got['bary'] <= 1).all() and (got['bary'][got['tri'] < 0] == 0).all() and (got['closest'][got['tri'] < 0] == 0).all()
    assert (got['grad_self'][~m] == 0).all(), label                # exactly 0 off the inside set
    touched = np.zeros(m.shape, bool)
    n = verts.shape[2]
    for b in range(verts.shape[0]):
        for h in range(2):
            touched[b, h, np.clip(faces[1 - h], 0, n - 1)[got['tri'][b, h][m[b, h]]].ravel()] = True
    assert (got['grad_other'][~touched] == 0).all(), label         # a vertex that no inside vertex's triangle touches: exactly 0
    # autograd with g = 1 is the formula on the kernel's own two tensors
    assert np.array_equal(got['grad'], got['grad_self'] + got['grad_other'][:, ::-1]), label
    return ref, bar


# ---- tetrahedron pair ------------------------------------------------------------------------------
def tetrahedron_pair():
    second = TET + np.array([0.04, 0.04, -0.04])
    return np.stack((TET, second))[None].astype(np.float32), np.stack((TET_FACES, TET_FACES))


def test_tetrahedron_pair():
    """tests/test_eval_interaction_gpu.py::test_tetrahedron_pair's input: B = 1, n = 4, Fc = 4, fewer vertices than a wave.  The second
    tetrahedron's corner (-10, -10, 10) mm is inside the first, in a face region, 40 / sqrt(3) = 23.094 mm from the surface."""
    verts, faces = tetrahedron_pair()
    got = run(verts, faces)
    ref, _ = check_against_the_restatement(got, verts, faces, None, "tetrahedra")
    assert got['count'].tolist() == [[0, 1]]
    for k in ('loss', 'grad_self', 'grad_other', 'bary', 'closest', 'inside'):
        assert (got[k][0, 0] == 0).all(), k
    assert (got['tri'][0, 0] == -1).all()
    i = int(np.argmax(got['inside'][0, 1]))
    d = 0.04 / np.sqrt(3.0)                                        # 23.094 mm
    assert abs(np.linalg.norm(verts[0, 1, i].astype(np.float64) - got['closest'][0, 1, i]) - d) <= DISCRETE_BAR
    assert abs(got['loss'][0, 1] - d * d / 4) <= 1 / 4 * 2 * d * DISCRETE_BAR
    assert (got['bary'][0, 1, i] > 0.01).all() and abs(got['bary'][0, 1, i].sum() - 1) <= 1e-5      # a face region
    others = np.arange(4) != i
    assert (got['grad_self'][0, 1, i] != 0).any() and (got['grad_self'][0, 1, others] == 0).all()
    corners = TET_FACES[got['tri'][0, 1, i]]
    fourth = np.setdiff1d(np.arange(4), corners)
    assert len(fourth) == 1 and (got['grad_other'][0, 1, fourth[0]] == 0).all() and (got['grad_other'][0, 1, corners] != 0).any(-1).all()


# ---- dented octahedron -------------------------------------------------------------------------------
OCT_S = 0.05
OCT = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 0, 0.5]], np.float64) * OCT_S
OCT_FACES = np.array([f for k in range(4) for f in ((k, (k + 1) % 4, 4), ((k + 1) % 4, k, 5))], np.int64)
OCT_QUERIES = np.array([[0, 0, 0.6], [0.2, 0, 0.55], [0.15, 0.15, 0.6], [0, 0, 0.4], [0, 0, 1.2]], np.float64) * OCT_S
OCT_INSIDE = np.array([1, 1, 1, 0, 0], bool)
OCT_TRI = np.array([1, 1, 0, -1, -1])
OCT_BARY = np.array([[0, 0, 1], [0, 0.14, 0.86], [0.55 / 3, 0.55 / 3, 1.9 / 3], [0, 0, 0], [0, 0, 0]])
OCT_CLOSEST = np.array([[0, 0, 0.5], [0.14, 0, 0.43], [0.55 / 3, 0.55 / 3, 1.9 / 3], [0, 0, 0], [0, 0, 0]]) * OCT_S


def octahedron_by_hand(n=6):
    """The hand values of hand 0 = OCT_QUERIES (padded to n with the last, outside, query) against hand 1 = OCT: loss, grad_self [n, 3],
    grad_other [6, 3], from the table of the module's constants by plain arithmetic."""
    r = (OCT_QUERIES - OCT_CLOSEST) * OCT_INSIDE[:, None]
    loss = (r ** 2).sum() / n
    grad_self = np.zeros((n, 3))
    grad_self[:5] = 2.0 / n * r
    grad_other = np.zeros((6, 3))
    # query 0 -> the apex (vertex 5) alone; query 1 -> vertex 0 with 0.14 and the apex with 0.86; query 2 -> vertices 0, 1, 4 of face 0
    grad_other[5] = -2.0 / n * (r[0] + 0.86 * r[1])
    grad_other[0] = -2.0 / n * (0.14 * r[1] + 0.55 / 3 * r[2])
    grad_other[1] = -2.0 / n * (0.55 / 3 * r[2])
    grad_other[4] = -2.0 / n * (1.9 / 3 * r[2])
    return loss, grad_self, grad_other


def octahedron_case(n=6, seed=None):
    """hand 0: the five queries, the last one repeated up to index 5, then (n - 6) seeded queries scattered through the octahedron's bounding
    box; hand 1: the octahedron, its vertices repeated up to n.  Hand 0's own faces are degenerate.  -> (verts [1, 2, n, 3] f32, faces)."""
    q = np.concatenate((OCT_QUERIES, OCT_QUERIES[-1:]))
    if n > 6:
        g = np.random.default_rng(seed)
        q = np.concatenate((q, g.uniform((-0.6, -0.6, 0.3), (0.6, 0.6, 1.0), (n - 6, 3)) * OCT_S))
    mesh = OCT[np.arange(n) % 6]
    return np.stack((q[:n], mesh))[None].astype(np.float32), np.stack((np.zeros_like(OCT_FACES), OCT_FACES))


def test_dented_octahedron_by_hand():
    """A closed, outward-oriented mesh on which an inside point's closest point is a vertex (the dented apex, a four-way tie between the faces
    1, 3, 5, 7), an edge (edge 0-5, a tie between the faces 1 and 7) or a face: the lowest face index wins."""
    verts, faces = octahedron_case()
    got = run(verts, faces)
    ref, bar = check_against_the_restatement(got, verts, faces, None, "octahedron")
    assert got['count'].tolist() == [[3, 0]] and np.array_equal(got['inside'][0, 0, :5] != 0, OCT_INSIDE) and got['inside'][0, 0, 5] == 0
    assert np.array_equal(got['tri'][0, 0, :5], OCT_TRI) and got['tri'][0, 0, 5] == -1
    b = {k: v[0, 0] for k, v in bar.items()}
    assert np.abs(got['closest'][0, 0, :5] - OCT_CLOSEST).max() <= b['closest']
    assert np.abs(got['bary'][0, 0, :5] - OCT_BARY).max() <= b['bary']
    assert np.array_equal(got['bary'][0, 0, 0], [0, 0, 1]) and got['bary'][0, 0, 1, 0] == 0      # one-hot at the apex; the opposite corner of the edge
    loss, grad_self, grad_other = octahedron_by_hand()
    assert abs(got['loss'][0, 0] - loss) <= b['loss']
    assert np.abs(got['grad_self'][0, 0] - grad_self).max() <= b['grad_self']
    assert np.abs(got['grad_other'][0, 0] - grad_other).max() <= b['grad_other']
    assert (got['grad_other'][0, 0, [2, 3]] == 0).all()
    for k in ('loss', 'grad_self', 'grad_other', 'bary', 'closest'):       # the octahedron's vertices against a mesh collapsed to a point
        assert (got[k][0, 1] == 0).all(), k


# ---- template hands --------------------------------------------------------------------------------------
def test_template_hands_against_the_restatement():
    """B = 3, n = 778, Fc = 1538: apart, and two interpenetrating poses."""
    from pdfnet_amd import functional as F
    verts, faces, pen = template_case()
    assert well_conditioned(pen)
    got = run(verts, faces)
    ref, bar = check_against_the_restatement(got, verts, faces, None, "template", free=template_reference())
    assert ref['count'].tolist() == [[0, 0], [121, 131], [180, 80]]
    assert np.array_equal(ref['count'], pen['count'])
    # the same bits as the evaluation metric's rule on the same tensors
    count, _, _, wind, _ = F.mesh_penetration(cu(verts), cu(faces), return_fields=True)
    assert np.array_equal(got['inside'] != 0, (wind > 0.5).cpu().numpy()) and np.array_equal(got['count'], count.cpu().numpy())
    for k in KEYS + ('grad', 'grad_self', 'grad_other'):
        assert ((got[k][0] == -1) if k == 'tri' else (got[k][0] == 0)).all(), k        # the separated sample
    assert (ref['loss'][1:] > 5e-6).all() and (np.abs(ref['grad_self']).max((2, 3))[1:] > 10 * bar['grad_self'][1:]).all()
    assert (np.abs(ref['grad_other']).max((2, 3))[1:] > 10 * bar['grad_other'][1:]).all() and (ref['loss'][1:] > 100 * bar['loss'][1:]).all()


# ---- the loss's inside set is the metric's, bit for bit ------------------------------------------------------
def threshold_case():
    """n = 64, Fc = 4.  Hand 1 is the test tetrahedron, its spare vertices parked on corner 0.  Hand 0's vertices sit on its surface, where
    the side of 0.5 a vertex falls on is decided by rounding alone (a point on a face sees that face under +-2 pi by the sign of a
    determinant that is 0 in exact arithmetic, so its winding number is 0 or 1; on an edge or a corner both arguments of atan2 vanish): the
    4 corners, 2 points on each of the 6 edges and 2 on each of the 4 faces (24), and the first 20 of those moved by +1e-7 m and by -1e-7 m
    along the direction from the centroid (40).  Hand 0's own faces index its first four vertices."""
    on = [TET[i] for i in range(4)]
    on += [(1 - t) * TET[i] + t * TET[j] for i in range(4) for j in range(i + 1, 4) for t in (0.5, 0.3)]
    on += [w[0] * TET[f[0]] + w[1] * TET[f[1]] + w[2] * TET[f[2]] for f in TET_FACES for w in ((1 / 3, 1 / 3, 1 / 3), (0.6, 0.3, 0.1))]
    on = np.array(on)
    out = on[:20] / np.linalg.norm(on[:20], axis=-1, keepdims=True)
    own = np.concatenate((on, on[:20] + 1e-7 * out, on[:20] - 1e-7 * out))
    other = TET[np.concatenate((np.arange(4), np.zeros(60, np.int64)))]
    assert own.shape == other.shape == (64, 3)
    return np.stack((own, other))[None].astype(np.float32), np.stack((TET_FACES, TET_FACES))


def random_case(n=33, Fc=50, seed=7):
    g = np.random.default_rng(seed)
    return g.normal(0.0, 0.05, (2, 2, n, 3)).astype(np.float32), g.integers(0, n, (2, Fc, 3)).astype(np.int64)


@pytest.mark.parametrize("case", [threshold_case, random_case])
def test_inside_is_the_metrics_wind_above_half_with_no_condition_on_the_input(case):
    """Both kernels call one function for a triangle's solid angle (csrc/mesh_geom.h geo_solid_angle) and sum, scale and compare alike, so
    `inside` IS mesh_penetration's wind > 0.5 and count its count, for every vertex of every input: asserted where rounding alone decides the
    side (on the other hand's faces, edges and corners, and 1e-7 m off them) and on a seeded random pair of triangle soups.  Nothing is
    excluded and nothing is compared with float64: the statement is the equality of two kernels' bits."""
    from pdfnet_amd import functional as F
    verts, faces = case()
    with torch.no_grad():
        _, count, inside, _, _, _ = F.penetration_loss(cu(verts), cu(faces), return_fields=True)
        m_count, _, _, wind, _ = F.mesh_penetration(cu(verts), cu(faces), return_fields=True)
    wind, inside = wind.cpu().numpy(), inside.cpu().numpy()
    print("  %s: inside %s of %d, smallest |wind - 0.5| %.3e, vertices with |wind - 0.5| < 1e-6: %d" % (
        case.__name__, count.cpu().numpy().tolist(), verts.shape[2], np.abs(wind - 0.5).min(), (np.abs(wind - 0.5) < 1e-6).sum()))
    assert np.array_equal(inside != 0, wind > 0.5), np.argwhere((inside != 0) != (wind > 0.5))
    assert np.array_equal(count.cpu().numpy(), m_count.cpu().numpy())
    assert np.array_equal(count.cpu().numpy(), (wind > 0.5).sum(-1))


# ---- sizes -------------------------------------------------------------------------------------------------
SIZE_SEEDS = {63: 1, 65: 1}                                        # seeds for which the case is well conditioned (tests/test_penetration_loss_cpu.py)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_sizes_that_are_no_multiple_of_64(n):
    if n == 1:                                                     # one vertex against a mesh of one vertex: nothing can be inside a point
        verts = np.stack((OCT_QUERIES[:1], OCT[5:6]))[None].astype(np.float32)
        faces = np.zeros((2, 3, 3), np.int64)
        got = run(verts, faces)
        check_against_the_restatement(got, verts, faces, None, "n=1")
        assert got['count'].tolist() == [[0, 0]] and (got['loss'] == 0).all() and (got['grad'] == 0).all() and (got['tri'] == -1).all()
        return
    verts, faces = octahedron_case(n, SIZE_SEEDS[n])
    got = run(verts, faces)
    ref, _ = check_against_the_restatement(got, verts, faces, None, "octahedron n=%d" % n)
    assert 10 <= ref['count'][0, 0] <= n - 10 and ref['count'][0, 1] == 0
    assert np.array_equal(got['tri'][0, 0, :5], OCT_TRI)


def caps_case():
    """tests/test_eval_interaction_gpu.py::test_the_caps' padding of the interpenetrating template samples: n = 1024 (vertices repeated) and
    Fc = 2048 (degenerate faces (0, 0, 0) appended: the point vertex 0, which lies on the surface already)."""
    verts, faces, _ = template_case()
    pv = verts[1:, :, np.arange(1024) % 778]
    return pv, np.concatenate((faces, np.zeros((2, 2048 - faces.shape[1], 3), np.int64)), 1)


def test_the_caps():
    verts, faces, pen = template_case()
    pv, pf = caps_case()
    got = run(pv, pf)
    ref, _ = check_against_the_restatement(got, pv, pf, None, "caps")
    rep = np.arange(1024) % 778
    assert np.array_equal(ref['inside'], (pen['wind'][1:] > 0.5)[..., rep])
    assert (got['tri'] < 1538).all()                               # never a padding triangle: a real face holds vertex 0 at a lower index


# ---- invalid hands, determinism, shapes -----------------------------------------------------------------------
def test_invalid_hand():
    verts, faces, _ = template_case()
    v = verts[1:2]
    for valid in ((1, 0), (0, 1), (0, 0)):
        got = run(v, faces, np.array([valid], np.float32))
        for k in KEYS + ('grad', 'grad_self', 'grad_other'):
            assert ((got[k] == -1) if k == 'tri' else (got[k] == 0)).all(), (valid, k)
    on = run(v, faces, np.array([[1, 1]], np.float32))
    plain = run(v, faces)
    assert all(np.array_equal(on[k], plain[k]) for k in plain) and (plain['count'] > 0).all()
    for h in range(2):                                             # H2O marks an absent hand with zeros: finite, nothing inside either way
        z = v.copy()
        z[:, h] = 0
        got = run(z, faces)
        assert all(np.isfinite(x).all() for x in got.values()) and (got['count'] == 0).all() and (got['loss'] == 0).all() and (got['grad'] == 0).all()
    both = run(np.zeros((1, 2, 778, 3), np.float32), faces)
    assert all(np.isfinite(x).all() for x in both.values()) and (both['count'] == 0).all() and (both['loss'] == 0).all()


def test_determinism_rows_alone_optional_outputs_and_leading_dimensions():
    import itertools
    from pdfnet_amd import functional as F, hip
    verts, faces, _ = template_case()
    f = cu(faces)

    def call(sl=slice(None)):
        v = cu(verts)[sl].requires_grad_()
        out = F.penetration_loss(v, f, return_fields=True)
        out[0].sum().backward()
        return tuple(out) + (v.grad,)
    first, second = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(verts.shape[0]):
        assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, call(slice(b, b + 1)))), b
    assert first[0].shape == (3, 2) and first[1].dtype == first[2].dtype == first[3].dtype == torch.int32 and first[2].shape == (3, 2, 778)
    assert first[4].shape == first[5].shape == (3, 2, 778, 3)
    gs, go = (cu(x) for x in raw_gradients(verts, faces))
    # every combination of the optional outputs NULL: the others do not change
    L = hip.lib()
    v = cu(verts)
    full = {'grad_self': gs, 'grad_other': go, 'inside': first[2], 'tri': first[3], 'bary': first[4], 'closest': first[5]}
    for mask in itertools.product((False, True), repeat=6):
        loss, count = torch.empty(3, 2, device='cuda'), torch.empty(3, 2, dtype=torch.int32, device='cuda')
        outs = {k: torch.full_like(t, 7) if on else None for (k, t), on in zip(full.items(), mask)}
        L.pdf_penetration_loss(v.data_ptr(), f.data_ptr(), None, 3, 778, faces.shape[1], loss.data_ptr(), count.data_ptr(),
                               *[None if o is None else o.data_ptr() for o in outs.values()], None)
        torch.cuda.synchronize()
        assert torch.equal(loss, first[0]) and torch.equal(count, first[1]), mask
        assert all(o is None or torch.equal(o, full[k]) for k, o in outs.items()), mask
    assert torch.equal(F.penetration_loss(v, f), first[0])
    lead = F.penetration_loss(torch.stack((v, v.flip(0))).reshape(2, 3, 1, 2, 778, 3), f, return_fields=True)
    assert lead[0].shape == (2, 3, 1, 2) and lead[2].shape == (2, 3, 1, 2, 778) and lead[4].shape == (2, 3, 1, 2, 778, 3)
    for x, y in zip(lead, first):
        assert torch.equal(x[0, :, 0], y) and torch.equal(x[1, :, 0], y.flip(0))


def test_autograd():
    from pdfnet_amd import functional as F
    verts, faces, _ = template_case()
    g = np.array([[0.5, -2.0], [3.0, 0.25], [1.5, 7.0]], np.float32)
    scaled = run(verts, faces, g=g)
    w = g[..., None, None]
    assert np.array_equal(scaled['grad'], w * scaled['grad_self'] + (w * scaled['grad_other'])[:, ::-1])
    assert (scaled['grad'][1:] != 0).any()
    v, f = cu(verts).requires_grad_(), cu(faces)
    out = F.penetration_loss(v, f, return_fields=True)
    assert out[0].requires_grad and not any(x.requires_grad for x in out[1:])
    (first,) = torch.autograd.grad(out[0].sum(), v, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(first.sum(), v)                        # once differentiable
    with torch.no_grad():
        quiet = F.penetration_loss(v, f)
    assert not quiet.requires_grad and torch.equal(quiet, out[0])
    assert torch.equal(F.penetration_loss(v.detach(), f), out[0].detach())      # no gradient asked for: NULL is passed, the same loss


def test_refusals():
    from pdfnet_amd import functional as F, hip
    c = hip.lib().cdll
    v, f = torch.zeros(1, 2, 1025, 3, device='cuda'), torch.zeros(2, 2049, 3, dtype=torch.long, device='cuda')
    outs = [torch.full((2,), 7.0, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'), torch.full((1, 2, 1025, 3), 7.0, device='cuda'),
            torch.full((1, 2, 1025, 3), 7.0, device='cuda'), torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda'),
            torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda'), torch.full((1, 2, 1025, 3), 7.0, device='cuda'),
            torch.full((1, 2, 1025, 3), 7.0, device='cuda')]
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n=4, Fc=4, B=1, null=()):
        o = [None if i in null else P_(x) for i, x in enumerate(outs)]
        return c.pdf_penetration_loss(None if 'v' in null else P_(v), None if 'f' in null else P_(f), None, B, n, Fc, *o, None)
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(null=('v',)), dict(null=('f',)), dict(null=(0,)), dict(null=(1,))):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0 and call(B=-1) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    x, fa = v[:, :, :4], f[:, :4]
    for bad in (lambda: F.penetration_loss(v, fa), lambda: F.penetration_loss(x, f), lambda: F.penetration_loss(x[:, :1], fa),
                lambda: F.penetration_loss(x[..., :2], fa), lambda: F.penetration_loss(x, fa[:1]), lambda: F.penetration_loss(x, fa[..., :2]),
                lambda: F.penetration_loss(x, fa, valid=torch.ones(2, 2, device='cuda'))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        F.penetration_loss(x.cpu(), fa.cpu())


# ---- the training term ---------------------------------------------------------------------------------------
PEN_WEIGHT = 10.0
OVERLAP_VALID = np.array([[1, 1], [1, 1], [1, 0]], np.float32)
ROOT_Z = np.float32(0.4) + np.float32(5.0) / np.float32(100.0)      # what uv_root_3d makes of root = (5, 0, 0), in its own fp32 arithmetic


def overlapping_hands():
    """hands((SHIFTS[1], SHIFTS[2], SHIFTS[1])) moved to z = 0.45 m, as fp32 sums -> [3, 2, 778, 3]."""
    return hands((SHIFTS[1], SHIFTS[2], SHIFTS[1])) + np.array([0, 0, ROOT_Z], np.float32)


def total_bars(ref, verts, faces):
    """The bar of d (sum of both rows' losses) / d verts [B, 2]: hand h collects grad_self of row (b, h) and grad_other of row (b, 1 - h)."""
    bar = bars(ref, verts, faces)
    return bar['grad_self'] + bar['grad_other'][:, ::-1], bar


def test_penetration_term_on_overlapping_hands():
    """`penetration_term` called directly, on inputs whose absolute vertices are the interpenetrating template hands at z = 0.45 m (K with focal
    length 100 and centre 0, ind = 0 and root = (5, 0, 0): uv_root_3d gives (0, 0, 0.45)); sample 2 has an invalid hand."""
    from pdfnet_amd.trains.simplified import penetration_term
    _, faces, _ = template_case()
    K = np.tile(np.array([[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]], np.float32), (3, 1, 1))
    batch = {'valid': cu(OVERLAP_VALID), 'K_new': cu(K), 'ind': torch.zeros(3, 2, dtype=torch.long, device='cuda')}
    vp = cu(hands((SHIFTS[1], SHIFTS[2], SHIFTS[1])).transpose(1, 0, 2, 3)).requires_grad_()
    root = torch.zeros(2, 3, 3, device='cuda')
    root[..., 0] = 5.0
    root.requires_grad_()
    term = penetration_term(vp, root, batch['ind'], batch, cu(faces), 128)
    absolute = overlapping_hands()
    ref = ref_penetration_loss(absolute, faces, OVERLAP_VALID)
    want = 1e6 * ref['loss'].sum(1)
    assert want[0] > 1 and want[1] > 1 and want[2] == 0            # mm^2, float64: not vacuous
    tbar, bar = total_bars(ref, absolute, faces)
    print("  penetration_term %s mm^2, float64 %s" % (term.tolist(), want.tolist()))
    assert term.shape == (3,) and (np.abs(term.detach().cpu().numpy() - want) <= 1e6 * bar['loss'].sum(1) + np.spacing(np.float32(want))).all()
    assert float(term.detach()[2]) == 0.0
    term.sum().backward()
    gv, gr = vp.grad.cpu().numpy().transpose(1, 0, 2, 3), root.grad.cpu().numpy().transpose(1, 0, 2)
    assert np.isfinite(gv).all() and np.isfinite(gr).all() and (gv[2] == 0).all() and (gr[2] == 0).all()
    total = 1e6 * total_gradient(ref)                                # [B, 2, n, 3], mm^2 per metre
    e = np.abs(gv - total).max((2, 3))
    print("  d term / d vp: max err %s bar %s (max %.3e)" % (e.tolist(), (1e6 * tbar).tolist(), np.abs(total).max()))
    assert (e <= 1e6 * tbar * (1 + 1e-6)).all()
    # the root: with root_xy = 0 and the centre at 0, d verts / d root = (dz, dx, dy) = (1 / 100, z / 100 / K00, z / 100 / K11) for every
    # vertex of the hand, so its gradient is the summed vertex gradient (the net force on the hand) in those units; 778 vertex bars add up.
    # The term exerts no net force on the pair: the two hands' cancel.
    force, chain = total.sum(2), np.array([1 / 100, ROOT_Z / 100 / 100, ROOT_Z / 100 / 100])
    want_r = force[..., [2, 0, 1]] * chain
    bar_r = 778 * 1e6 * tbar[..., None] * chain
    print("  d term / d root: %s, float64 %s, bar %s" % (gr[:2].tolist(), want_r[:2].tolist(), bar_r[:2].tolist()))
    assert (force[:2] != 0).any(-1).all()
    assert (np.abs(gr - want_r) <= bar_r * (1 + 1e-6)).all() and (np.abs(gr[:2, 0] + gr[:2, 1]) <= bar_r[:2].sum(1)).all()


@pytest.mark.parametrize("fused", [True, False])
def test_training_term(fused, monkeypatch):
    """penetration_weight absent / 0: the new code is not entered (penetration_term and F.penetration_loss are replaced by functions that
    raise), the loss and every statistic are bit-equal, the statistics' keys come in the same order and the autograd graph of the loss has the
    same nodes in the same order: nothing is computed that was not computed before.  The parameter gradients of two runs of this model are
    not bit-reproducible (float atomics in its backward: tests/test_cloud_loss_gpu.py::test_training_term has the measurements -- two runs
    WITHOUT the field already differ in about half of the gradient tensors), so they are compared as that test compares them: all gradients
    as one vector, within GRAD_NOISE_BAR of its norm, the distance of two identical runs printed beside.
    penetration_weight = w > 0: stats['penetration_loss'] is `penetration_term` evaluated apart, the total grows by w times it, and the
    gradients are those of the w = 0 run plus w times the term's own gradient, to GRAD_NOISE_BAR of the gradient norm.  The random model's
    hands need not intersect, so for this run the absolute vertices the term sees have the VALUES of the interpenetrating template hands at
    z = 0.45 m and the derivatives of the model's own (`_abs_verts` is replaced by template + (own - own.detach())): the float64 restatement
    on those very vertices asserts that the term is > 0, and its gradient reaches every parameter behind verts3d and root."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains import simplified
    R, model, _, batch = trainer_fixture()
    monkeypatch.setattr(F, 'MESH_LOSS_FUSED', fused)
    real = (simplified.penetration_term, F.penetration_loss)

    def never(*a, **k):
        raise AssertionError("the penetration term ran with penetration_weight 0 or absent")
    monkeypatch.setattr(simplified, 'penetration_term', never)
    monkeypatch.setattr(F, 'penetration_loss', never)
    absent, again, zero = train_step(), train_step(), train_step(penetration_weight=0)
    monkeypatch.setattr(simplified, 'penetration_term', real[0])
    monkeypatch.setattr(F, 'penetration_loss', real[1])
    for other in (again, zero):
        assert torch.equal(absent[0], other[0]) and list(absent[1]) == list(other[1]) and 'penetration_loss' not in other[1]
        assert all(torch.equal(torch.as_tensor(absent[1][k]), torch.as_tensor(other[1][k])) for k in absent[1])
        assert absent[5] == other[5] and list(absent[2]) == list(other[2])
    noise, n_noise = gradient_distance(again[2], absent[2])
    off, n_off = gradient_distance(zero[2], absent[2])
    print("  fused=%s gradients of %d parameters: absent vs absent differ in %d tensors, by %.3e of their norm; absent vs 0 in %d, by %.3e"
          % (fused, len(absent[2]), n_noise, noise, n_off, off))
    assert off <= GRAD_NOISE_BAR and noise <= GRAD_NOISE_BAR

    base, real_abs = cu(overlapping_hands()), simplified._abs_verts

    def overlapping(vp, root, ind, b, input_res, down_ratio):
        verts, valid = real_abs(vp, root, ind, b, input_res, down_ratio)
        return base + (verts - verts.detach()), valid              # the template hands' values (x - x = 0 exactly), the model's gradient
    monkeypatch.setattr(simplified, '_abs_verts', overlapping)
    loss, stats, grads, (result, params, hand, other_info), crit, nodes = train_step(penetration_weight=PEN_WEIGHT)
    pl = stats['penetration_loss']
    assert list(stats) == list(zero[1]) + ['penetration_loss'] and pl.shape == (3,) and bool(torch.isfinite(pl).all())
    assert len(nodes) > len(zero[5])
    for k in zero[1]:
        if k != 'loss':
            assert torch.equal(torch.as_tensor(stats[k]), torch.as_tensor(zero[1][k])), k
    vp, root = simplified._pair(result['verts3d']), simplified._pair(params['root'])
    with torch.no_grad():
        direct = simplified.penetration_term(vp, root, batch['ind'], batch, crit.faces_pair, R, 4)
        seen, valid = overlapping(vp, root, batch['ind'], batch, R, 4)
    assert torch.equal(direct, pl.detach()) and torch.equal(stats['loss'], loss)
    ref = ref_penetration_loss(seen.cpu().numpy(), crit.faces_pair.cpu().numpy(), valid.cpu().numpy())
    want = 1e6 * ref['loss'].sum(1)
    print("  fused=%s penetration_loss mm^2 %s, float64 %s, inside %s" % (fused, pl.tolist(), want.tolist(), ref['count'].tolist()))
    assert (want > 1).any() and (pl.detach().cpu().numpy()[want > 1] > 0).all()      # not vacuous
    diff = (loss.double() - zero[0].double() - PEN_WEIGHT * pl.detach().double()).abs().cpu().numpy()
    ulp = np.spacing(np.abs(loss.cpu().numpy()))
    print("  fused=%s loss %s |loss - loss_off - w penetration_loss| %s ulp %s" % (fused, loss.tolist(), diff, ulp))
    assert (diff <= ulp).all()
    # the term's own gradient with respect to the parameters: the term alone, on a forward of its own
    model.zero_grad(set_to_none=True)
    F.manual_seed(5)
    F.step_counter(torch.device('cuda')).zero_()
    res = model(batch['input'], batch['choose'], batch['cloud'], batch.get('depth'), batch['ind'], batch['K_new'], batch['valid'])
    term = simplified.penetration_term(simplified._pair(res[0]['verts3d']), simplified._pair(res[1]['root']), batch['ind'], batch, crit.faces_pair, R, 4)
    assert torch.equal(term.detach(), pl.detach())
    term.sum().backward()
    F.join_wgrad()
    torch.cuda.synchronize()
    own = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    assert list(grads) == list(zero[2]) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    predicted = {k: zero[2][k] + PEN_WEIGHT * own[k] if k in own else zero[2][k] for k in zero[2]}
    dist = gradient_distance(grads, predicted)[0]
    dec = [k for k in grads if k.startswith('decoder.')]
    moved = gradient_distance({k: grads[k] for k in dec}, {k: zero[2][k] for k in dec})[0]
    print("  fused=%s gradients vs (w = 0) + w * (the term's own): %.3e of their norm; the term moves the mesh-decoder gradients by %.3e of theirs"
          % (fused, dist, moved))
    assert dec and moved > GRAD_NOISE_BAR and dist <= GRAD_NOISE_BAR


