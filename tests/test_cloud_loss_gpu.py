"""The differentiable cloud-to-mesh loss on the GPU (csrc/icp.hip pdf_cloud_mesh_loss, F.cloud_mesh_loss, CtdetLoss's cloud_weight term) against a
float64 numpy restatement of the contract in include/pdfnet_hip.h: the association of pdf_mesh_icp with iters = 0, loss = the mean of |p - q|^2
over the inliers, and for every inlier -(2/m) w_k (p - q) on corner k of its triangle, (w_a, w_b, w_c) the weights of the closest point
q = w_a a + w_b b + w_c c (the envelope theorem: q minimises over the triangle, so only its explicit dependence on the corners counts).
tests/test_cloud_loss_cpu.py checks that formula against central differences of the restatement's own loss.

The restatement extends tests/test_icp_gpu.py's: the seven-region function also returns the weights, and ref_cloud_loss evaluates every point
either on its float64 arg-min triangle or, given `tri`, on the triangle the kernel chose.  The discrete outputs (tri, inliers) are pinned by
test_icp_gpu.py's rules and by equality with F.mesh_icp(iters=0), whose association code the kernel shares; the continuous outputs (loss m^2,
grad, bary, and the translation -0.5 sum_vertices grad = mean (p - q), metres) are compared with the restatement GIVEN the kernel's tri, so
that no point and no vertex is excluded and a tie between two triangles cannot break the comparison.  Before that comparison the float64 side
asserts that no |p - q| lies within TRIM_MARGIN of the trim.

BARS: four times the largest difference from the restatement measured on an MI355X over every case of this file (profiles/NOTES.md has the
values per case), which was
    loss 6.13e-11 m^2 (one triangle: half an fp32 ulp of 1.1e-3 m^2)      grad 5.65e-9 (tetrahedron, P = 63)
    bary 8.59e-7 (template hands: 3e-8 m of rounding over 5 mm edges)      translation 2.17e-9 m (template hands)
The test meshes hold no needle-shaped matched triangle: the fp32 weights of such a triangle are ill-conditioned (the quotients vb / (va + vb + vc)
lose the digits that the cancellation in va, vb, vc took), and bars measured here say nothing about them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_icp_gpu import (DISCRETE_BAR, EMPTY, INVALID, REGION_QUERIES, SIZE_SEEDS, TET, TRI, TRIM, TRIM_MARGIN, _dot, check_discrete, cu,
                                ref_associate, ref_closest_pairs, ref_facing, ref_icp, template_ref, template_scene)
from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

BARS = {'loss': 2.46e-10, 'grad': 2.26e-8, 'bary': 3.44e-6, 't': 8.7e-9}
# weights of (a, b, c) for REGION_QUERIES on TRI, in the order of the regions: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face
REGION_WEIGHTS = np.array([[1, 0, 0], [0, 1, 0], [.5, .5, 0], [0, 0, 1], [.5, 0, .5], [0, .5, .5], [.4, .3, .3]])
REGION_CLOSEST = REGION_WEIGHTS @ np.array([[0, 0, 0.5], [0, 0.1, 0.5], [0.1, 0, 0.5]])
REGION_TRIMS = ((0.05, 7), (0.0225, 3), (0.0222, 1), (0.009, 0))          # those of test_one_triangle_seven_regions_and_the_trim
# Margins of the hand values (the float32 0.1, 0.49 of TRI and the queries are up to 3e-8 m off the decimal numbers written here, and the
# kernel rounds in fp32): closest 1e-6 m as everywhere; a weight is a ratio of lengths along a 0.1 m edge, 1e-6 m / 0.1 m = 1e-5; |p - q| is at
# most 0.0436 m, so |p - q|^2 moves by 2 * 0.0436 * 1e-6 = 8.7e-8 m^2; a corner's gradient is a mean over m of 2 w (p - q) summed over the
# points: 2 * (1e-5 * 0.0436 + 1e-6) = 2.9e-6 per point of the mean
HAND_BARS = {'closest': DISCRETE_BAR, 'bary': 1e-5, 'loss': 8.7e-8, 'grad': 2.9e-6}


# ---- float64 restatement -----------------------------------------------------------------------
def ref_closest_weights(P, A, B, C):
    """tests/test_icp_gpu.py::ref_closest_pairs that also returns the weights -> (q [..., 3], w [..., 3]) with q = w_a A + w_b B + w_c C."""
    ab, ac = B - A, C - A
    ap, bp, cp = P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):          # (quotients of regions that are not selected)
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = vb / (va + vb + vc), vc / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    weights = [(one, zero, zero), (zero, one, zero), (1 - t_ab, t_ab, zero), (zero, zero, one), (1 - t_ac, zero, t_ac), (zero, 1 - t_bc, t_bc)]
    wts = np.select([c[..., None] for c in conds], [np.stack(x, -1) for x in weights], np.stack((1 - v - w, v, w), -1))
    q = wts[..., 0:1] * A + wts[..., 1:2] * B + wts[..., 2:3] * C
    assert np.isfinite(q).all() and np.isfinite(wts).all()
    return q, wts


def ref_cloud_loss_row(V, faces, cloud, valid, trim, tri=None):
    """One (sample, hand) of pdf_cloud_mesh_loss in float64 -> dict: loss, inliers, grad [n, 3], bary [P, 3], tri [P], closest [P, 3],
    dist [P] (inf where tri = -1), inlier [P] bool.  tri: evaluate every point on that triangle (-1: none) instead of the float64 arg-min."""
    V, cloud = np.asarray(V, np.float64), np.asarray(cloud, np.float64)
    faces = np.clip(faces, 0, len(V) - 1)
    P = len(cloud)
    out = {'loss': 0.0, 'inliers': 0, 'grad': np.zeros_like(V), 'bary': np.zeros((P, 3)), 'tri': np.full(P, -1, np.int64),
           'closest': np.zeros((P, 3)), 'dist': np.full(P, np.inf), 'inlier': np.zeros(P, bool)}
    if valid == 0 or not (cloud[:, 2] > 0).any():
        return out
    tri = ref_associate(V, faces, cloud, trim)['tri'] if tri is None else np.asarray(tri, np.int64)
    hit = tri >= 0
    if not hit.any():
        return out
    k = faces[tri[hit]]
    q, w = ref_closest_weights(cloud[hit], V[k[:, 0]], V[k[:, 1]], V[k[:, 2]])
    out['tri'][hit], out['closest'][hit], out['bary'][hit], out['dist'][hit] = tri[hit], q, w, np.linalg.norm(cloud[hit] - q, axis=-1)
    m = out['inlier'] = out['dist'] < trim
    n_in = out['inliers'] = int(m.sum())
    if n_in:
        r = cloud[m] - out['closest'][m]
        out['loss'] = float((r ** 2).sum(-1).mean())
        for c in range(3):
            np.add.at(out['grad'], faces[tri[m], c], -(2.0 / n_in) * out['bary'][m, c:c + 1] * r)
    return out


def ref_cloud_loss(V, faces, cloud, valid=None, trim=TRIM, tri=None):
    """V [B, 2, n, 3], faces [2, F, 3], cloud [B, 2, P, 3], valid [B, 2] or None, tri [B, 2, P] or None -> dict of stacked float64 arrays
    ([B, 2, ...]): loss, inliers, grad, bary, and tri, closest, dist, inlier."""
    rows = [[ref_cloud_loss_row(V[b, h], faces[h], cloud[b, h], 1 if valid is None else valid[b, h], trim, None if tri is None else tri[b, h])
             for h in range(2)] for b in range(V.shape[0])]
    return {k: np.array([[r[k] for r in pair] for pair in rows]) for k in rows[0][0]}


# ---- running and comparing -----------------------------------------------------------------------
KEYS = ('loss', 'inliers', 'tri', 'bary', 'closest')


def run(verts, faces, cloud, valid=None, trim=TRIM, g=None):
    """-> the fields of F.cloud_mesh_loss as numpy arrays plus 'grad': verts.grad after (loss * g).sum().backward(), g = 1 by default, so that
    grad is the kernel's own output times exactly 1."""
    from pdfnet_amd import functional as F
    v = cu(verts).requires_grad_()
    got = F.cloud_mesh_loss(v, cu(faces), cu(cloud), None if valid is None else cu(valid), trim=trim, return_fields=True)
    (got[0] * (torch.ones_like(got[0]) if g is None else cu(g))).sum().backward()
    torch.cuda.synchronize()
    out = {k: x.detach().cpu().numpy() for k, x in zip(KEYS, got)}
    out['grad'] = v.grad.cpu().numpy()
    return out


def errors(got, ref):
    return {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in ('loss', 'grad', 'bary')}


def check_against_the_restatement(got, verts, faces, cloud, valid, trim, label):
    """loss, grad, bary against the restatement given the kernel's tri; the discrete outputs must agree with it exactly.  -> the restatement."""
    ref = ref_cloud_loss(verts, faces, cloud, valid, trim, tri=got['tri'])
    hit = np.isfinite(ref['dist'])
    assert not hit.any() or np.abs(ref['dist'][hit] - trim).min() >= TRIM_MARGIN, label
    assert np.array_equal(got['inliers'], ref['inliers']), (label, got['inliers'], ref['inliers'])
    assert all(np.isfinite(got[k]).all() for k in got)
    e = errors(got, ref)
    print("  %s max err: loss %.3e m^2, grad %.3e, bary %.3e (bars %s)" % (label, e['loss'], e['grad'], e['bary'], BARS))
    for k, x in e.items():
        assert x <= BARS[k], (label, k, x, BARS[k])
    assert (got['bary'] >= 0).all() and (got['bary'] <= 1).all() and (got['bary'][got['tri'] < 0] == 0).all()
    touched = np.zeros(got['grad'].shape[:3], bool)
    for b in range(verts.shape[0]):
        for h in range(2):
            touched[b, h, np.clip(faces[h], 0, verts.shape[2] - 1)[got['tri'][b, h][ref['inlier'][b, h]]].ravel()] = True
    assert (got['grad'][~touched] == 0).all(), label               # a vertex that no inlier touches: exactly 0
    return ref


def one_mesh(V, tris, pts, **kw):
    """The same small mesh as both hands of one sample -> the outputs of the left hand."""
    V, tris, pts = np.asarray(V, np.float32), np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(pts, np.float32).reshape(-1, 3)
    args = (np.stack((V, V))[None], np.stack((tris, tris)), np.stack((pts, pts))[None])
    got = run(*args, **kw)
    assert all(np.array_equal(v[0, 0], v[0, 1]) for v in got.values())
    check_against_the_restatement(got, *args, None, kw.get('trim', TRIM), "one mesh")
    return {k: v[0, 0] for k, v in got.items()}


# ---- one triangle ------------------------------------------------------------------------------------
def test_one_triangle_seven_regions_and_the_trim():
    p = REGION_QUERIES.astype(np.float64)
    d = np.linalg.norm(p - REGION_CLOSEST, axis=-1)                 # 30, 37.4, 22.4, 37.4, 22.4, 43.6, 10 mm
    for trim, want in REGION_TRIMS:
        got = one_mesh(TRI, [0, 1, 2], REGION_QUERIES, trim=trim)
        m = d < trim
        assert (got['tri'] == 0).all() and got['inliers'] == want == m.sum(), (trim, got['inliers'])
        assert np.abs(got['closest'] - REGION_CLOSEST).max() <= HAND_BARS['closest']
        assert np.abs(got['bary'] - REGION_WEIGHTS).max() <= HAND_BARS['bary']
        # exactly one-hot in the vertex regions, exactly 0 for the opposite corner in the edge regions
        assert np.array_equal(got['bary'][[0, 1, 3]], REGION_WEIGHTS[[0, 1, 3]].astype(np.float32))
        assert got['bary'][2, 2] == 0 and got['bary'][4, 1] == 0 and got['bary'][5, 0] == 0
        loss = (d[m] ** 2).mean() if want else 0.0
        grad = -(2.0 / max(want, 1)) * np.einsum('jk,jc->kc', REGION_WEIGHTS[m], (p - REGION_CLOSEST)[m])
        assert abs(got['loss'] - loss) <= HAND_BARS['loss'], (trim, got['loss'], loss)
        assert np.abs(got['grad'] - grad).max() <= HAND_BARS['grad'], (trim, got['grad'], grad)
        if not want:
            assert got['loss'] == 0 and (got['grad'] == 0).all()


def test_reversed_winding_gives_no_loss_and_no_gradient():
    got = one_mesh(TRI, [0, 2, 1], REGION_QUERIES, trim=0.05)
    assert (got['tri'] == -1).all() and (got['closest'] == 0).all() and (got['bary'] == 0).all()
    assert got['inliers'] == 0 and got['loss'] == 0 and (got['grad'] == 0).all()


def test_zero_area_triangle_beside_a_good_one_gets_no_gradient():
    # faces 0 and 1 have zero area (collinear corners with edges that are exact multiples; two equal corners) and lie nearer to the queries
    V = np.concatenate((TRI, [[0.0, 0.0, 0.48], [0.0, 0.05, 0.48], [0.0, 0.1, 0.48]])).astype(np.float32)
    got = one_mesh(V, [[3, 4, 5], [3, 3, 5], [0, 1, 2]], REGION_QUERIES, trim=0.05)
    assert (got['tri'] == 2).all() and got['inliers'] == 7 and np.abs(got['closest'] - REGION_CLOSEST).max() <= HAND_BARS['closest']
    assert (got['grad'][3:] == 0).all() and (got['grad'][:3] != 0).any()
    alone = one_mesh(TRI, [0, 1, 2], REGION_QUERIES, trim=0.05)
    assert np.array_equal(got['grad'][:3], alone['grad']) and got['loss'] == alone['loss'] and np.array_equal(got['bary'], alone['bary'])


def test_a_point_with_z_zero_contributes_nothing():
    pts = REGION_QUERIES.copy()
    pts[1, 2], pts[4] = 0.0, (0.05, -0.02, -0.49)
    live = np.array([1, 0, 1, 1, 0, 1, 1], bool)
    got = one_mesh(TRI, [0, 1, 2], pts, trim=0.05)
    assert np.array_equal(got['tri'], np.where(live, 0, -1)) and (got['closest'][~live] == 0).all() and (got['bary'][~live] == 0).all()
    assert got['inliers'] == 5
    # the same five points alone: the same sums in the same order
    five = one_mesh(TRI, [0, 1, 2], REGION_QUERIES[live], trim=0.05)
    assert got['loss'] == five['loss'] and np.array_equal(got['grad'], five['grad'])


# ---- sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, 1024])
def test_sizes_that_are_no_multiple_of_64(P):
    V, tris = TET
    g = np.random.default_rng(SIZE_SEEDS[P])
    pts = np.concatenate((g.uniform(-0.08, 0.08, (P, 2)), g.uniform(0.40, 0.56, (P, 1))), -1).astype(np.float32)
    verts, faces, cloud = np.stack((V, V + [0.01, 0, 0]))[None].astype(np.float32), np.stack((tris, tris)), np.stack((pts, pts[::-1]))[None]
    got = run(verts, faces, cloud, trim=0.02)
    check_discrete(dict(got, out=verts), faces, cloud, 0.02, "P=%d" % P)
    assert (got['tri'] < 3).all() and (got['tri'] >= 0).all()
    assert np.array_equal(got['inliers'], ref_icp(verts, faces, cloud, None, 0, 0.02)['inliers'])
    check_against_the_restatement(got, verts, faces, cloud, None, 0.02, "tetrahedron P=%d" % P)


GRID_SEEDS = {1: 5, 1024: 1054}                                    # seeds for which no point lies within TRIM_MARGIN of the trim (tests/test_cloud_loss_cpu.py)


@functools.lru_cache(maxsize=None)
def grid_mesh():
    """32 x 32 vertices at Z = 0.5 m, 16 cm across: n = 1,024; 31 * 31 * 2 = 1,922 triangles that face the camera, padded to Fc = 2,048 with
    triangles of two equal corners (zero area: never matched).  -> (V [1024, 3] float32, faces [2048, 3])."""
    i, j = np.meshgrid(np.arange(32), np.arange(32), indexing='ij')
    V = np.stack((-0.08 + 0.16 / 31 * j, -0.08 + 0.16 / 31 * i, np.full(i.shape, 0.5)), -1).reshape(-1, 3).astype(np.float32)
    c = (i[:31, :31] * 32 + j[:31, :31]).ravel()
    tris = np.concatenate((np.stack((c, c + 32, c + 1), -1), np.stack((c + 33, c + 1, c + 32), -1)))
    pad = np.stack((np.arange(126), np.arange(126), np.arange(126) + 500), -1)
    return V, np.concatenate((tris, pad)).astype(np.int64)


@pytest.mark.parametrize("P", [1, 1024])
def test_the_largest_mesh(P):
    V, tris = grid_mesh()
    assert V.shape == (1024, 3) and tris.shape == (2048, 3) and (ref_facing(V.astype(np.float64), tris)[0] < 0).sum() == 1922
    g = np.random.default_rng(GRID_SEEDS[P])
    pts = np.concatenate((g.uniform(-0.1, 0.1, (P, 2)), g.uniform(0.46, 0.54, (P, 1))), -1).astype(np.float32)
    verts, faces, cloud = np.stack((V, V + [0.002, 0, 0.003]))[None].astype(np.float32), np.stack((tris, tris)), np.stack((pts, pts[::-1]))[None]
    got = run(verts, faces, cloud, trim=TRIM)
    assert (got['tri'] < 1922).all() and (got['tri'] >= 0).all()     # never a padding triangle (check_discrete's loose set would hold them)
    ref = check_against_the_restatement(got, verts, faces, cloud, None, TRIM, "grid P=%d" % P)
    for h in range(2):                                             # the chosen triangle is as near as the float64 minimum over the facing ones
        strict = ref_associate(verts[0, h], faces[h], cloud[0, h], TRIM)
        assert np.abs(ref['dist'][0, h] - strict['dist']).max() <= DISCRETE_BAR
        assert np.abs(got['closest'][0, h] - ref['closest'][0, h]).max() <= DISCRETE_BAR
    if P == 1024:
        assert (0 < ref['inliers']).all() and (ref['inliers'] < P).all()     # the trim rejects something


# ---- template hands --------------------------------------------------------------------------------------
def test_template_hands_against_the_restatement():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    got = run(verts, faces, cloud, valid)
    icp = F.mesh_icp(cu(verts), cu(faces), cu(cloud), cu(valid), iters=0, trim=TRIM, return_fields=True)
    assert np.array_equal(got['tri'], icp[6].cpu().numpy()) and np.array_equal(got['inliers'], icp[4].cpu().numpy())      # shared association
    ref0 = template_ref(0, False)
    assert np.array_equal(got['inliers'], ref0['inliers'])
    check_discrete(dict(got, out=verts), faces, cloud, TRIM, "template", valid)
    check_against_the_restatement(got, verts, faces, cloud, valid, TRIM, "template")
    # one translation-only ICP step is the mean of p - q over the inliers, and so is -0.5 * the gradient summed over the vertices
    t = -0.5 * got['grad'].astype(np.float64).sum(2)
    et = np.abs(t - template_ref(1, False)['t']).max()
    print("  template translation identity: max err %.3e m (bar %.1e)" % (et, BARS['t']))
    assert et <= BARS['t']
    for b, h in (INVALID, EMPTY):
        assert got['loss'][b, h] == 0 and got['inliers'][b, h] == 0 and (got['grad'][b, h] == 0).all() and (got['tri'][b, h] == -1).all()
        assert (got['bary'][b, h] == 0).all() and (got['closest'][b, h] == 0).all()


def test_determinism_rows_alone_and_optional_outputs():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    f, c, va = cu(faces), cu(cloud), cu(valid)

    def call(sl=slice(None)):
        v = cu(verts)[sl].requires_grad_()
        out = F.cloud_mesh_loss(v, f, c[sl], va[sl], return_fields=True)
        out[0].sum().backward()
        return tuple(out) + (v.grad,)
    first, second = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(verts.shape[0]):
        assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, call(slice(b, b + 1)))), b
    # every optional output NULL: loss and inliers do not change
    L = __import__('pdfnet_amd.hip', fromlist=['lib']).lib()
    v, loss, inl = cu(verts), torch.empty(3, 2, device='cuda'), torch.empty(3, 2, dtype=torch.int32, device='cuda')
    L.pdf_cloud_mesh_loss(v.data_ptr(), f.data_ptr(), c.data_ptr(), va.data_ptr(), 3, 778, faces.shape[1], cloud.shape[2], TRIM, loss.data_ptr(),
                          inl.data_ptr(), None, None, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(loss, first[0]) and torch.equal(inl, first[1])
    assert torch.equal(F.cloud_mesh_loss(v, f, c, va), first[0])


def test_autograd():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    g = np.array([[0.5, -2.0], [3.0, 0.25], [1.5, 7.0]], np.float32)
    unit, scaled = run(verts, faces, cloud, valid), run(verts, faces, cloud, valid, g=g)
    assert np.array_equal(scaled['grad'], g[..., None, None] * unit['grad']) and np.array_equal(scaled['loss'], unit['loss'])
    v, f, c = cu(verts).requires_grad_(), cu(faces), cu(cloud).requires_grad_()
    out = F.cloud_mesh_loss(v, f, c, cu(valid), return_fields=True)
    assert out[0].requires_grad and not any(x.requires_grad for x in out[1:])
    out[0].sum().backward()
    assert v.grad is not None and c.grad is None and f.grad is None
    with torch.no_grad():
        quiet = F.cloud_mesh_loss(v, f, c, cu(valid))
    assert not quiet.requires_grad and torch.equal(quiet, out[0])
    assert np.array_equal(quiet.cpu().numpy(), unit['loss'])


def test_refusals():
    from pdfnet_amd import functional as F, hip
    c = hip.lib().cdll
    v, f, p = torch.zeros(1, 2, 1025, 3, device='cuda'), torch.zeros(2, 2049, 3, dtype=torch.long, device='cuda'), torch.zeros(1, 2, 1025, 3, device='cuda')
    outs = [torch.full((2,), 7.0, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'), torch.full((1, 2, 1025, 3), 7.0, device='cuda'),
            torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda'), torch.full((1, 2, 1025, 3), 7.0, device='cuda'),
            torch.full((1, 2, 1025, 3), 7.0, device='cuda')]
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n=4, Fc=4, P=4, trim=0.03, B=1):
        return c.pdf_cloud_mesh_loss(P_(v), P_(f), P_(p), None, B, n, Fc, P, ctypes.c_float(trim), *[P_(o) for o in outs], None)
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P=0), dict(P=1025), dict(trim=0.0), dict(trim=-1.0),
               dict(trim=float('inf')), dict(trim=float('nan'))):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0 and call(B=-1) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    x, fa, cl = v[:, :, :4], f[:, :4], p[:, :, :4]
    for bad in (lambda: F.cloud_mesh_loss(v, fa, cl), lambda: F.cloud_mesh_loss(x, f, cl), lambda: F.cloud_mesh_loss(x, fa, p),
                lambda: F.cloud_mesh_loss(x, fa, cl, trim=0.0), lambda: F.cloud_mesh_loss(x, fa, cl[0]),
                lambda: F.cloud_mesh_loss(x[:, :1], fa, cl[:, :1]), lambda: F.cloud_mesh_loss(x, fa, cl, valid=torch.ones(2, 2, device='cuda'))):
        with pytest.raises(ValueError):
            bad()


# ---- the training term ---------------------------------------------------------------------------------------
GRAD_NOISE_BAR = 1e-4      # of the norm of all gradients: see test_training_term
CLOUD_TRIM = 10.0          # metres: every live point of the random synthetic cloud is an inlier, so the term is not vacuous


@functools.lru_cache(maxsize=None)
def trainer_fixture():
    """The fixture of tests/test_icp_gpu.py::evaluation_runs: R = 128, B = 3, random-init model (dropout off, so that two steps see the same
    network), one synthetic batch."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    R, B = 128, 3
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(make_opt(R)).cuda()
    for mod in m.modules():
        if isinstance(getattr(mod, 'p', None), float):
            mod.p = 0.0
    m.train()
    return R, m, consts, tree_to(synthetic_train_batch(B, R, seed=21, consts=consts), torch.device('cuda'))


def train_step(**over):
    """One forward + backward of model and CtdetLoss in train mode -> (loss [B], stats, {parameter name: gradient}, the model's outputs, the
    loss module, the autograd graph of the loss as the list of its nodes' type names in depth-first order)."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, m, consts, batch = trainer_fixture()
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0, **over)
    crit = CtdetLoss(opt, consts).cuda()
    m.zero_grad(set_to_none=True)
    F.manual_seed(5)
    F.step_counter(torch.device('cuda')).zero_()
    res = m(batch['input'], batch['choose'], batch['cloud'], batch.get('depth'), batch['ind'], batch['K_new'], batch['valid'])
    loss, stats, _, _ = crit(*res, batch, 'train', 0)
    nodes, seen, stack = [], set(), [loss.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        nodes.append(type(fn).__name__)
        stack.extend(f for f, _ in fn.next_functions)
    loss.sum().backward()
    F.join_wgrad()                                                 # (weight gradients run on side streams)
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    return loss.detach(), stats, grads, res, crit, nodes


def gradient_distance(a, b):
    """|a - b| / |b| over ALL gradient tensors taken as one vector (2-norms), and how many of the tensors differ in some bit."""
    num = sum(float((a[k].double() - b[k].double()).pow(2).sum()) for k in b)
    return (num / sum(float(b[k].double().pow(2).sum()) for k in b)) ** 0.5, sum(not torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize("fused", [True, False])
def test_training_term(fused, monkeypatch):
    """cloud_weight absent / 0: the new code is not entered (cloud_term and F.cloud_mesh_loss are replaced by functions that raise), the loss
    and every statistic are bit-equal, the statistics' keys come in the same order, and the autograd graph of the loss has the same nodes in
    the same order -- nothing is computed that was not computed before.
    The parameter gradients cannot be compared bit for bit: the backward of this model is not bit-reproducible from run to run (float
    atomics in the point scatter, the L2Norm and LayerNorm weight gradients and the face terms: tests/test_bf16_gpu.py
    test_bf16_shadows_in_the_whole_model, tests/test_loss_float64_gpu.py test_forked_dense_terms_equal_the_inline_ones), so two runs with
    cloud_weight ABSENT already differ in about half of the gradient tensors.  All gradients taken as one vector, two such runs were measured
    on an MI355X to differ by 4.2e-9 to 1.8e-6 of its norm (eight pairs; which of the two it is changes from run to run), and the term at
    weight 0.01 moves the mesh-decoder gradients by 1.0e-1 of theirs: GRAD_NOISE_BAR = 1e-4 lies a factor of 50 above the one and a factor of
    1,000 below the other.  absent vs 0 must stay within it, the term on must move the decoder gradients by more; the distance of the
    two identical runs is printed beside them."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains import simplified
    R, _, _, batch = trainer_fixture()
    monkeypatch.setattr(F, 'MESH_LOSS_FUSED', fused)
    real = (simplified.cloud_term, F.cloud_mesh_loss)

    def never(*a, **k):
        raise AssertionError("the cloud term ran with cloud_weight 0 or absent")
    monkeypatch.setattr(simplified, 'cloud_term', never)
    monkeypatch.setattr(F, 'cloud_mesh_loss', never)
    absent, again, zero = train_step(), train_step(), train_step(cloud_weight=0, cloud_trim=CLOUD_TRIM)
    monkeypatch.setattr(simplified, 'cloud_term', real[0])
    monkeypatch.setattr(F, 'cloud_mesh_loss', real[1])
    on = train_step(cloud_weight=0.01, cloud_trim=CLOUD_TRIM)
    for other in (again, zero):
        assert torch.equal(absent[0], other[0]) and list(absent[1]) == list(other[1]) and 'cloud_loss' not in other[1]
        assert all(torch.equal(torch.as_tensor(absent[1][k]), torch.as_tensor(other[1][k])) for k in absent[1])
        assert absent[5] == other[5] and list(absent[2]) == list(other[2])
    noise, n_noise = gradient_distance(again[2], absent[2])
    off, n_off = gradient_distance(zero[2], absent[2])
    print("  fused=%s gradients of %d parameters: absent vs absent differ in %d tensors, by %.3e of their norm; absent vs 0 in %d, by %.3e"
          % (fused, len(absent[2]), n_noise, noise, n_off, off))
    assert off <= GRAD_NOISE_BAR and noise <= GRAD_NOISE_BAR
    loss, stats, grads, (result, params, hand, other_info), crit, nodes = on
    cl = stats['cloud_loss']
    assert list(stats) == list(zero[1]) + ['cloud_loss'] and cl.shape == (3,) and bool(torch.isfinite(cl).all()) and bool((cl > 0).all())
    assert len(nodes) > len(zero[5])
    for k in zero[1]:
        if k != 'loss':
            assert torch.equal(torch.as_tensor(stats[k]), torch.as_tensor(zero[1][k])), k
    with torch.no_grad():
        direct = simplified.cloud_term(simplified._pair(result['verts3d']), simplified._pair(params['root']), batch['ind'], batch, crit.faces_pair,
                                       R, 4, CLOUD_TRIM)
    assert torch.equal(direct, cl.detach()) and torch.equal(stats['loss'], loss)
    diff = (loss.double() - zero[0].double() - 0.01 * cl.detach().double()).abs().cpu().numpy()
    ulp = np.spacing(np.abs(loss.cpu().numpy()))
    print("  fused=%s loss %s cloud_loss mm^2 %s |loss - loss_off - 0.01 cloud_loss| %s ulp %s" % (fused, loss.tolist(), cl.tolist(), diff, ulp))
    assert (diff <= ulp).all()
    assert list(grads) == list(zero[2]) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    dec = [k for k in grads if k.startswith('decoder.')]
    moved = gradient_distance({k: grads[k] for k in dec}, {k: zero[2][k] for k in dec})[0]
    print("  fused=%s the term on moves the mesh-decoder gradients by %.3e of their norm" % (fused, moved))
    assert dec and moved > GRAD_NOISE_BAR
    with pytest.raises(KeyError, match="cloud"):
        crit(result, params, hand, other_info, {k: v for k, v in batch.items() if k != 'cloud'}, 'train', 0)
