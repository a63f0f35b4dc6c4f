"""ICP refinement of the hand meshes against their sensor point clouds on the GPU (csrc/icp.hip pdf_mesh_icp, F.mesh_icp,
Trainer.evaluation(refined=...)) against a float64 numpy restatement of the contract in include/pdfnet_hip.h: association with the camera-facing
surface by the seven regions of the point-to-triangle distance (Ericson, Real-Time Collision Detection 5.1.5), a strict trim, the mean
translation or Kabsch with determinant correction per iteration, the composed (R, t) applied to the original vertices.  No reference program
has this feature, so the contract is all there is to pin to.

Meshes: hand-made triangles, and the template hands of tests/test_eval_interaction_gpu.py::template half a metre from the camera, displaced by
up to 2 cm and 6 degrees, with 1,000 cloud points sampled on the camera-facing surface of the undisplaced mesh plus seeded 1 mm noise, 40 of
them pushed 2 to 8 cm behind the surface so that the trim has something to reject.

Discrete outputs are compared so that rounding cannot break the comparison and without excluding a point: the float64 distance from the point
to the triangle the kernel chose is at most 1e-6 m above the float64 minimum over the triangles that face the camera in float64, and at most
1e-6 m below the minimum over those and the ones within FACING_EPS of the threshold (about which fp32 and float64 may disagree); the chosen
triangle is one of the latter set; `closest` is within 1e-6 m of the float64 closest point of that same triangle; `inliers` equals the
restatement's, which is well-posed because no point lies within TRIM_MARGIN of `trim` in any iteration (tests/test_icp_cpu.py checks that on the
float64 side, as it checks that the restatement itself at least halves the mean vertex error of every recovery case).

Continuous outputs (out_verts, t in metres; R; rms in metres): BARS holds, per (iters, mode), four times the largest difference from the
restatement measured on an MI355X (profiles/NOTES.md has the measured values)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_eval_interaction_gpu import template
from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

TRIM, TRIM_MARGIN, FACING_EPS, DISCRETE_BAR = 0.03, 1e-5, 1e-5, 1e-6
P_TEMPLATE = 1000
# (iters, rigid) -> bars for (out_verts m, R, t m, rms m): 4 x the maximum measured on an MI355X, which was
#   iters 0:             0        0        0        1.39e-10
#   iters 1 translation: 3.01e-8  0        2.17e-9  1.04e-8        iters 1 rigid: 3.38e-8  5.01e-8  3.00e-8  3.09e-10
#   iters 8 translation: 2.83e-8  0        2.29e-9  1.52e-9        iters 8 rigid: 3.08e-8  2.75e-8  6.84e-9  4.83e-10
# (3e-8 is half an fp32 ulp of a coordinate at 0.5 m and 6e-8 that of a rotation entry near 1: the differences are the rounding of the
# outputs, below the 7e-8 m / 1.6e-5 m by which an fp32 numpy run of the restatement differs from float64)
BARS = {(0, False): (0.0, 0.0, 0.0, 5.6e-10), (0, True): (0.0, 0.0, 0.0, 5.6e-10),
        (1, False): (1.2e-7, 0.0, 8.7e-9, 4.2e-8), (1, True): (1.35e-7, 2.0e-7, 1.2e-7, 1.24e-9),
        (8, False): (1.13e-7, 0.0, 9.1e-9, 6.1e-9), (8, True): (1.23e-7, 1.1e-7, 2.7e-8, 1.93e-9)}
# zero displacement: the restatement leaves such a hand at the identity up to the fp32 rounding of its inputs, and the kernel may end anywhere
# within the bars above from the restatement: the largest bar of each quantity
ZERO_BARS = tuple(max(b[k] for b in BARS.values()) for k in range(3))


# ---- float64 restatement -----------------------------------------------------------------------
def _dot(u, v):
    return (u * v).sum(-1)


def ref_closest_pairs(P, A, B, C):
    """Queries and triangle corners of shapes that broadcast to [..., 3] -> [..., 3]: the closest point of the triangle to the query, by
    region: vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face -- the first whose test holds."""
    ab, ac = B - A, C - A
    ap, bp, cp = P - A, P - B, P - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):          # (quotients of regions that are not selected)
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v, w = vb / (va + vb + vc), vc / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    points = [A + 0 * P, B + 0 * P, A + t_ab[..., None] * ab, C + 0 * P, A + t_ac[..., None] * ac, B + t_bc[..., None] * (C - B)]
    face = A + v[..., None] * ab + w[..., None] * ac
    q = np.select([c[..., None] for c in conds], points, face)
    assert np.isfinite(q).all()
    return q


def ref_closest(P, A, B, C):
    """Queries P [m, 3], triangle corners [F, 3] -> [m, F, 3]: every query against every triangle."""
    return ref_closest_pairs(P[:, None], A[None], B[None], C[None])


def ref_facing(V, faces):
    """-> (n . (a + b + c) [F], the same divided by |n| |a + b + c|, 0 where n = 0); a triangle faces the camera when the first is < 0."""
    A, B, C = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    n, m = np.cross(B - A, C - A), A + B + C
    s = _dot(n, m)
    scale = np.linalg.norm(n, axis=-1) * np.linalg.norm(m, axis=-1)
    return s, np.where(scale > 0, s / np.where(scale > 0, scale, 1.0), 0.0)


def ref_associate(V, faces, cloud, trim, keep=None):
    """One association of cloud [P, 3] with the mesh (V [n, 3], faces [F, 3]) in float64 -> dict: tri [P] (-1: no triangle or ignored point),
    closest [P, 3] (0 there), dist [P] (inf there), inlier [P] bool.  keep: the triangles that count (default: those facing the camera)."""
    V, cloud = np.asarray(V, np.float64), np.asarray(cloud, np.float64)
    faces = np.clip(faces, 0, len(V) - 1)
    P = len(cloud)
    out = {'tri': np.full(P, -1, np.int64), 'closest': np.zeros((P, 3)), 'dist': np.full(P, np.inf), 'inlier': np.zeros(P, bool)}
    live = cloud[:, 2] > 0
    idx = np.nonzero(ref_facing(V, faces)[0] < 0 if keep is None else keep)[0]        # ascending: argmin takes the lowest face among equals
    if live.any() and len(idx):
        # Exact pruning: the distance to a triangle's centroid bounds the distance to the triangle from above, that minus the triangle's
        # radius from below; a triangle whose lower bound exceeds the smallest upper bound cannot hold the minimum (nor tie with it).
        pts, (A, B, C) = cloud[live], (V[faces[idx, k]] for k in range(3))
        cen = (A + B + C) / 3.0
        rad = np.maximum(np.maximum(np.linalg.norm(A - cen, axis=-1), np.linalg.norm(B - cen, axis=-1)), np.linalg.norm(C - cen, axis=-1))
        dc = np.linalg.norm(pts[:, None] - cen[None], axis=-1)
        pi, fi = np.nonzero(dc - rad[None] <= dc.min(1)[:, None] * (1 + 1e-12))
        q = ref_closest_pairs(pts[pi], A[fi], B[fi], C[fi])
        d = np.linalg.norm(pts[pi] - q, axis=-1)
        order = np.lexsort((fi, d, pi))                          # per point: the smallest distance first, the lowest face among equals
        sel = order[np.r_[True, pi[order][1:] != pi[order][:-1]]]
        out['tri'][live], out['closest'][live], out['dist'][live] = idx[fi[sel]], q[sel], d[sel]
        out['inlier'] = out['dist'] < trim
    return out


def ref_kabsch(q, p):
    """The rotation with det = +1 and the translation that minimise sum |R q + t - p|^2 -> (R, t, full): full is False, with R = I and
    t = mean p - mean q, when the cross-covariance's second singular value is below 1e-6 of its largest."""
    qm, pm = q.mean(0), p.mean(0)
    H = (q - qm).T @ (p - pm)
    U, S, Vt = np.linalg.svd(H)
    if not S[0] > 0 or S[1] < 1e-6 * S[0]:
        return np.eye(3), pm - qm, False
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, pm - R @ qm, True


def ref_icp_row(verts, faces, cloud, valid, iters, trim, rigid):
    """One (sample, hand) of pdf_mesh_icp in float64 -> dict with out [n, 3], R, t, rms, inliers, tri, closest, and `margin`: the smallest
    | |p - q| - trim | over every association made, `steps`: the updates taken."""
    v0, cloud = np.asarray(verts, np.float64), np.asarray(cloud, np.float64)
    R, t, cur, margin, steps = np.eye(3), np.zeros(3), v0.copy(), np.inf, 0
    if valid == 0 or not (cloud[:, 2] > 0).any():
        return {'out': v0, 'R': R, 't': t, 'rms': 0.0, 'inliers': 0, 'tri': np.full(len(cloud), -1, np.int64), 'closest': np.zeros((len(cloud), 3)),
                'margin': margin, 'steps': 0}
    for it in range(iters + 1):
        a = ref_associate(cur, faces, cloud, trim)
        hit = a['tri'] >= 0
        if hit.any():
            margin = min(margin, np.abs(a['dist'][hit] - trim).min())
        m = a['inlier']
        if it == iters or m.sum() < (3 if rigid else 1):
            break
        p, q = cloud[m], a['closest'][m]
        Rk, tk = ref_kabsch(q, p)[:2] if rigid else (np.eye(3), (p - q).mean(0))
        R, t = Rk @ R, Rk @ t + tk
        cur = v0 @ R.T + t
        steps += 1
    n_in = int(m.sum())
    rms = float(np.sqrt((a['dist'][m] ** 2).mean())) if n_in else 0.0
    return {'out': cur, 'R': R, 't': t, 'rms': rms, 'inliers': n_in, 'tri': a['tri'], 'closest': a['closest'], 'margin': margin, 'steps': steps}


def ref_icp(verts, faces, cloud, valid=None, iters=8, trim=TRIM, rigid=False):
    """verts [B, 2, n, 3], faces [2, F, 3], cloud [B, 2, P, 3], valid [B, 2] or None -> dict of stacked float64 arrays ([B, 2, ...])."""
    rows = [[ref_icp_row(verts[b, h], faces[h], cloud[b, h], 1 if valid is None else valid[b, h], iters, trim, rigid) for h in range(2)]
            for b in range(verts.shape[0])]
    return {k: np.array([[r[k] for r in pair] for pair in rows]) for k in rows[0][0]}


# ---- inputs --------------------------------------------------------------------------------------
def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def sample_cloud(V, faces, P, seed, noise=0.001, outliers=0):
    """P points on the camera-facing triangles of the mesh, area-weighted, plus Gaussian noise of `noise` metres per coordinate; the last
    `outliers` of them pushed 2 to 8 cm away from the camera (background seen past the hand's edge: what the trim is for) -> float32."""
    g = np.random.default_rng(seed)
    f = faces[ref_facing(V, faces)[0] < 0]
    A, B, C = V[f[:, 0]], V[f[:, 1]], V[f[:, 2]]
    area = np.linalg.norm(np.cross(B - A, C - A), axis=-1)
    k = g.choice(len(f), P, p=area / area.sum())
    u, v = g.uniform(size=P), g.uniform(size=P)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    pts = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k])
    pts = pts + g.normal(0.0, noise, pts.shape)
    if outliers:
        pts[P - outliers:, 2] += g.uniform(0.02, 0.08, outliers)
    return pts.astype(np.float32)


CENTRES = ((-0.05, 0.0, 0.5), (0.05, 0.0, 0.5))                   # of the left and the right hand, metres
# per sample and hand: (rotation axis, degrees, translation in metres) of the prediction relative to the surface the cloud was sampled on
DISPLACEMENTS = (
    (((0, 0, 1), 0.0, (0.008, -0.006, 0.015)), ((0, 0, 1), 0.0, (-0.005, 0.004, -0.018))),
    (((1, 2, 0.5), 6.0, (0.006, 0.005, 0.016)), ((-1, 0.5, 2), -4.0, (-0.003, 0.006, 0.010))),
    (((0, 1, 0), 3.0, (0.0, 0.005, 0.010)), ((1, 0, 0), 5.0, (0.006, 0.0, -0.012))),
)
INVALID, EMPTY = (2, 0), (2, 1)                                   # (sample, hand): valid = 0 with a cloud; valid = 1 with the all-zero cloud
SEED, OUTLIERS = 11, 40          # (a seed for which the two input conditions of tests/test_icp_cpu.py hold)


@functools.lru_cache(maxsize=None)
def template_scene(noise=0.001, displaced=True):
    """-> (verts [3, 2, 778, 3] float32: the displaced hands, gt [3, 2, 778, 3] float64: where the clouds were sampled, faces [2, 1538, 3],
    cloud [3, 2, P_TEMPLATE, 3] float32, valid [3, 2] float32)."""
    left, right, faces = template()
    gt = np.stack([np.stack((left.astype(np.float64) + CENTRES[0], right.astype(np.float64) + CENTRES[1])) for _ in DISPLACEMENTS])
    verts, cloud = np.zeros(gt.shape, np.float32), np.zeros(gt.shape[:2] + (P_TEMPLATE, 3), np.float32)
    for b, pair in enumerate(DISPLACEMENTS):
        for h, (axis, deg, shift) in enumerate(pair):
            c = gt[b, h].mean(0)
            moved = (gt[b, h] - c) @ rotation(axis, deg).T + c + np.asarray(shift) if displaced else gt[b, h]
            verts[b, h] = moved.astype(np.float32)
            cloud[b, h] = sample_cloud(gt[b, h], faces[h], P_TEMPLATE, SEED + 10 * b + h, noise, OUTLIERS if noise > 0 else 0)
    valid = np.ones((len(DISPLACEMENTS), 2), np.float32)
    valid[INVALID] = 0
    cloud[EMPTY] = 0
    return verts, gt, faces, cloud, valid


@functools.lru_cache(maxsize=None)
def template_ref(iters, rigid):
    verts, _, faces, cloud, valid = template_scene()
    return ref_icp(verts, faces, cloud, valid, iters, TRIM, bool(rigid and iters))


def recovery_rows():
    return [(b, h) for b in range(len(DISPLACEMENTS)) for h in range(2) if (b, h) not in (INVALID, EMPTY)]


def mean_vertex_error(out, gt):
    return np.linalg.norm(out - gt, axis=-1).mean(-1)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


KEYS = ('out', 'R', 't', 'rms', 'inliers', 'closest', 'tri')


def run(verts, faces, cloud, valid=None, iters=8, trim=TRIM, rigid=False, fields=True):
    from pdfnet_amd import functional as F
    got = F.mesh_icp(cu(verts), cu(faces), cu(cloud), None if valid is None else cu(valid), iters=iters, trim=trim, rigid=rigid, return_fields=fields)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(KEYS, got)}


def check_discrete(got, faces, cloud, trim, label="", valid=None):
    """The rules of the module docstring for tri / closest, on the mesh the kernel returned (got['out'])."""
    worst = [0.0, 0.0, 0.0]
    for b in range(cloud.shape[0]):
        for h in range(2):
            if valid is not None and valid[b, h] == 0:
                assert (got['tri'][b, h] == -1).all() and (got['closest'][b, h] == 0).all()
                continue
            V, pts, tri = got['out'][b, h].astype(np.float64), cloud[b, h].astype(np.float64), got['tri'][b, h]
            f = np.clip(faces[h], 0, len(V) - 1)
            s, sn = ref_facing(V, f)
            strict, loose = ref_associate(V, f, pts, trim), ref_associate(V, f, pts, trim, keep=(s < 0) | (sn < FACING_EPS))
            hit = tri >= 0
            assert np.array_equal(hit, loose['tri'] >= 0) or np.array_equal(hit, strict['tri'] >= 0), (label, b, h)
            assert (got['closest'][b, h][~hit] == 0).all()
            if not hit.any():
                continue
            assert ((s[tri[hit]] < 0) | (sn[tri[hit]] < FACING_EPS)).all(), (label, b, h)
            k = f[tri[hit]]
            q = ref_closest_pairs(pts[hit], V[k[:, 0]], V[k[:, 1]], V[k[:, 2]])
            d = np.linalg.norm(pts[hit] - q, axis=-1)
            over = (d - np.where(np.isfinite(strict['dist'][hit]), strict['dist'][hit], loose['dist'][hit])).max()
            under = (loose['dist'][hit] - d).max()
            qerr = np.abs(got['closest'][b, h][hit] - q).max()
            worst = [max(worst[0], over), max(worst[1], under), max(worst[2], qerr)]
            assert over <= DISCRETE_BAR and under <= DISCRETE_BAR and qerr <= DISCRETE_BAR, (label, b, h, over, under, qerr)
    print("  %s chosen triangle: %.2e m above / %.2e m below the float64 minimum, closest err %.2e m" % (label, *worst))


def check_continuous(got, ref, bars, label=""):
    errs = [np.abs(got[k].astype(np.float64) - ref[k]).max() for k in ('out', 'R', 't', 'rms')]
    print("  %s max err: out_verts %.3e m, R %.3e, t %.3e m, rms %.3e m (bars %s)" % (label, *errs, bars))
    assert all(np.isfinite(got[k]).all() for k in KEYS if k in got)
    for k, e, bar in zip(('out', 'R', 't', 'rms'), errs, bars):
        assert e <= bar, (label, k, e, bar)
    return errs


# ---- association alone, on hand-made meshes -------------------------------------------------------
TRI = np.array([[0.0, 0.0, 0.5], [0.0, 0.1, 0.5], [0.1, 0.0, 0.5]], np.float32)       # a, b, c: faces the camera at the origin
# a query 1 cm in front of the triangle's plane in each of the seven regions, and its closest point
REGION_QUERIES = np.array([[-0.02, -0.02, 0.49], [-0.02, 0.13, 0.49], [-0.02, 0.05, 0.49], [0.13, -0.02, 0.49], [0.05, -0.02, 0.49],
                           [0.08, 0.08, 0.49], [0.03, 0.03, 0.49]], np.float32)
REGION_CLOSEST = np.array([[0, 0, 0.5], [0, 0.1, 0.5], [0, 0.05, 0.5], [0.1, 0, 0.5], [0.05, 0, 0.5], [0.05, 0.05, 0.5], [0.03, 0.03, 0.5]])


def one_mesh(V, tris, pts, **kw):
    """The same small mesh as both hands of one sample -> the outputs of the left hand."""
    V, tris, pts = np.asarray(V, np.float32), np.asarray(tris, np.int64).reshape(-1, 3), np.asarray(pts, np.float32).reshape(-1, 3)
    got = run(np.stack((V, V))[None], np.stack((tris, tris)), np.stack((pts, pts))[None], **kw)
    assert all(np.array_equal(v[0, 0], v[0, 1]) for v in got.values())
    return {k: v[0, 0] for k, v in got.items()}


def test_one_triangle_seven_regions_and_the_trim():
    d = np.linalg.norm(REGION_QUERIES.astype(np.float64) - REGION_CLOSEST, axis=-1)       # 30, 37.4, 22.4, 37.4, 22.4, 43.6, 10 mm
    for trim, want in ((0.05, 7), (0.0225, 3), (0.0222, 1), (0.009, 0)):
        got = one_mesh(TRI, [0, 1, 2], REGION_QUERIES, iters=0, trim=trim)
        assert (got['tri'] == 0).all() and np.abs(got['closest'] - REGION_CLOSEST).max() <= DISCRETE_BAR
        assert got['inliers'] == want == (d < trim).sum(), (trim, got['inliers'])
        m = d < trim
        assert abs(got['rms'] - (np.sqrt((d[m] ** 2).mean()) if m.any() else 0.0)) <= DISCRETE_BAR
        assert np.array_equal(got['out'], TRI) and np.array_equal(got['R'], np.eye(3, dtype=np.float32)) and (got['t'] == 0).all()
    ref = ref_associate(TRI, np.array([[0, 1, 2]]), REGION_QUERIES, 0.05)
    assert np.abs(ref['closest'] - REGION_CLOSEST).max() <= 1e-8          # (the float32 0.1 of TRI is 1.5e-9 off)


def test_reversed_winding_matches_nothing():
    got = one_mesh(TRI, [0, 2, 1], REGION_QUERIES, iters=0, trim=0.05)
    assert (got['tri'] == -1).all() and (got['closest'] == 0).all() and got['inliers'] == 0 and got['rms'] == 0
    got = one_mesh(TRI, [0, 2, 1], REGION_QUERIES, iters=3, trim=0.05, rigid=True)          # nothing to move towards
    assert np.array_equal(got['out'], TRI) and np.array_equal(got['R'], np.eye(3, dtype=np.float32)) and (got['t'] == 0).all()


def test_zero_area_triangle_beside_a_good_one_is_never_matched():
    # faces 0 and 1 have zero area (collinear corners with edges that are exact multiples; two equal corners) and lie nearer to the queries
    V = np.concatenate((TRI, [[0.0, 0.0, 0.48], [0.0, 0.05, 0.48], [0.0, 0.1, 0.48]])).astype(np.float32)
    got = one_mesh(V, [[3, 4, 5], [3, 3, 5], [0, 1, 2]], REGION_QUERIES, iters=0, trim=0.05)
    assert (got['tri'] == 2).all() and np.abs(got['closest'] - REGION_CLOSEST).max() <= DISCRETE_BAR and got['inliers'] == 7


def test_a_point_with_z_zero_is_ignored():
    pts = REGION_QUERIES.copy()
    pts[1, 2], pts[4] = 0.0, (0.05, -0.02, -0.49)
    got = one_mesh(TRI, [0, 1, 2], pts, iters=0, trim=0.05)
    live = np.array([1, 0, 1, 1, 0, 1, 1], bool)
    assert np.array_equal(got['tri'], np.where(live, 0, -1)) and (got['closest'][~live] == 0).all() and got['inliers'] == 5
    assert np.abs(got['closest'][live] - REGION_CLOSEST[live]).max() <= DISCRETE_BAR


def test_collinear_cloud_takes_the_translation_only_step_in_rigid_mode():
    """Eight points on a line 1 cm in front of the triangle's face: the cross-covariance has rank 1, so every rigid iteration falls back to the
    translation and R stays the identity exactly; the triangle moves onto the line."""
    pts = np.array([[0.01 + 0.005 * i, 0.02, 0.49] for i in range(8)], np.float32)
    got = one_mesh(TRI, [0, 1, 2], pts, iters=3, trim=0.05, rigid=True)
    ref = ref_icp(np.stack((TRI, TRI))[None], np.array([[[0, 1, 2]]] * 2), np.stack((pts, pts))[None], None, 3, 0.05, True)
    assert np.array_equal(ref['R'][0, 0], np.eye(3)) and ref['steps'][0, 0] == 3
    assert np.array_equal(got['R'], np.eye(3, dtype=np.float32)) and got['inliers'] == 8
    # 1e-7 m: the fp32 rounding of the coordinates 0.49 and 0.5 (3e-8 each) and of the output
    assert np.abs(got['t'] - ref['t'][0, 0]).max() <= 1e-7 and np.abs(got['t'] - [0, 0, -0.01]).max() <= 1e-7
    assert np.abs(got['out'] - ref['out'][0, 0]).max() <= 1e-7 and got['rms'] <= 1e-7


# n = 4, Fc = 4: a tetrahedron with its apex towards the camera; its three sides face the camera, its base faces away
TET = (np.array([[0.0, 0.0, 0.45], [0.05, 0.0, 0.52], [-0.03, 0.04, 0.52], [-0.03, -0.04, 0.52]]), np.array([[0, 1, 3], [0, 3, 2], [0, 2, 1], [1, 2, 3]]))


SIZE_SEEDS = {1: 1, 63: 63, 65: 65, 1000: 1007, 1024: 1028}         # seeds for which no point lies within TRIM_MARGIN of the trim


@pytest.mark.parametrize("P", [1, 63, 65, 1000, 1024])
def test_sizes_that_are_no_multiple_of_64(P):
    V, tris = TET
    g = np.random.default_rng(SIZE_SEEDS[P])
    pts = np.concatenate((g.uniform(-0.08, 0.08, (P, 2)), g.uniform(0.40, 0.56, (P, 1))), -1).astype(np.float32)
    verts, faces, cloud = np.stack((V, V + [0.01, 0, 0]))[None].astype(np.float32), np.stack((tris, tris)), np.stack((pts, pts[::-1]))[None]
    s = ref_facing(V, tris)[0]
    assert (s[:3] < 0).all() and s[3] > 0                              # the base faces away
    got = run(verts, faces, cloud, iters=0, trim=0.02)
    ref = ref_icp(verts, faces, cloud, None, 0, 0.02)
    assert np.abs(np.abs(np.linalg.norm(cloud[0].astype(np.float64) - ref['closest'], axis=-1) - 0.02)).min() >= TRIM_MARGIN
    check_discrete(got, faces, cloud, 0.02, "P=%d" % P)
    assert np.array_equal(got['inliers'], ref['inliers']) and np.abs(got['rms'] - ref['rms']).max() <= DISCRETE_BAR
    assert (got['tri'] < 3).all() and (got['tri'] >= 0).all()


def test_refusals_leave_the_outputs_alone():
    from pdfnet_amd import functional as F, hip
    c = hip.lib().cdll
    v, f, p = torch.zeros(1, 2, 1025, 3, device='cuda'), torch.zeros(2, 2049, 3, dtype=torch.long, device='cuda'), torch.zeros(1, 2, 1025, 3, device='cuda')
    outs = [torch.full((1, 2, 1025, 3), 7.0, device='cuda'), torch.full((18,), 7.0, device='cuda'), torch.full((6,), 7.0, device='cuda'),
            torch.full((2,), 7.0, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'), torch.full((1, 2, 1025, 3), 7.0, device='cuda'),
            torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda')]
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n=4, Fc=4, P=4, iters=1, trim=0.03, B=1):
        return c.pdf_mesh_icp(P_(v), P_(f), P_(p), None, B, n, Fc, P, iters, ctypes.c_float(trim), 0, *[P_(o) for o in outs], None)
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P=0), dict(P=1025), dict(iters=-1), dict(iters=65), dict(trim=0.0),
               dict(trim=-1.0), dict(trim=float('inf')), dict(trim=float('nan'))):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0 and call(B=-1) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    assert c.pdf_mesh_icp(None, P_(f), P_(p), None, 1, 4, 4, 4, 1, ctypes.c_float(0.03), 0, *[P_(o) for o in outs], None) == -1
    x, fa, cl = v[:, :, :4], f[:, :4], p[:, :, :4]
    for bad in (lambda: F.mesh_icp(v, fa, cl), lambda: F.mesh_icp(x, f, cl), lambda: F.mesh_icp(x, fa, p), lambda: F.mesh_icp(x, fa, cl, iters=65),
                lambda: F.mesh_icp(x, fa, cl, trim=0.0), lambda: F.mesh_icp(x, fa, cl[0]), lambda: F.mesh_icp(x[:, :1], fa, cl[:, :1]),
                lambda: F.mesh_icp(x, fa, cl, valid=torch.ones(2, 2, device='cuda'))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        F.mesh_icp(x.cpu(), fa.cpu(), cl.cpu())


# ---- template hands ---------------------------------------------------------------------------------
@pytest.mark.parametrize("iters,rigid", [(0, False), (0, True), (1, False), (1, True), (8, False), (8, True)])
def test_template_hands_against_the_restatement(iters, rigid):
    verts, gt, faces, cloud, valid = template_scene()
    ref = template_ref(iters, rigid)
    got = run(verts, faces, cloud, valid, iters=iters, rigid=rigid)
    label = "iters=%d %s" % (iters, 'rigid' if rigid else 'translation')
    assert ref['margin'].min() >= TRIM_MARGIN
    print("  %s mean vertex error mm: before %s after (kernel) %s after (float64) %s" % (
        label, np.round(mean_vertex_error(verts, gt) * 1000, 2).tolist(), np.round(mean_vertex_error(got['out'], gt) * 1000, 2).tolist(),
        np.round(mean_vertex_error(ref['out'], gt) * 1000, 2).tolist()))
    check_discrete(got, faces, cloud, TRIM, label, valid)
    assert np.array_equal(got['inliers'], ref['inliers']), (got['inliers'], ref['inliers'])
    check_continuous(got, ref, BARS[(iters, rigid)], label)
    for b, h in (INVALID, EMPTY):
        assert np.array_equal(got['out'][b, h], verts[b, h]) and np.array_equal(got['R'][b, h], np.eye(3, dtype=np.float32))
        assert (got['t'][b, h] == 0).all() and got['rms'][b, h] == 0 and got['inliers'][b, h] == 0 and (got['tri'][b, h] == -1).all()
    if iters == 0:
        assert np.array_equal(got['out'], verts)
    # out = R v + t, in float64 from the kernel's own R and t: their fp32 rounding (6e-8 of a coordinate below 1 m, three terms) and out's
    rv = np.einsum('bhij,bhkj->bhki', got['R'].astype(np.float64), verts.astype(np.float64)) + got['t'].astype(np.float64)[:, :, None]
    assert np.abs(rv - got['out']).max() <= 5e-7


def test_zero_displacement_stays_put():
    verts, gt, faces, cloud, valid = template_scene(noise=0.0, displaced=False)
    for rigid in (False, True):
        got = run(verts, faces, cloud, valid, iters=8, rigid=rigid)
        eR, et = np.abs(got['R'] - np.eye(3)).max(), np.abs(got['t']).max()
        print("  zero displacement %s: |R - I| %.3e, |t| %.3e m, rms %.3e m" % ('rigid' if rigid else 'translation', eR, et, got['rms'].max()))
        assert eR <= (ZERO_BARS[1] if rigid else 0.0) and et <= ZERO_BARS[2] and got['rms'].max() <= 1e-6
        assert np.abs(got['out'] - verts).max() <= ZERO_BARS[0]
        live = np.ones((3, 2), bool)
        live[INVALID] = live[EMPTY] = False
        assert (got['inliers'][live] == P_TEMPLATE).all()


def test_determinism_rows_alone_and_optional_outputs():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    v, f, c, va = cu(verts), cu(faces), cu(cloud), cu(valid)
    for rigid in (False, True):
        first, second = (F.mesh_icp(v, f, c, va, iters=8, rigid=rigid, return_fields=True) for _ in range(2))
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        short = F.mesh_icp(v, f, c, va, iters=8, rigid=rigid)
        assert len(short) == 5 and all(torch.equal(a, b) for a, b in zip(first, short))
        for b in range(verts.shape[0]):
            alone = F.mesh_icp(v[b:b + 1], f, c[b:b + 1], va[b:b + 1], iters=8, rigid=rigid, return_fields=True)
            assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, alone)), b
    # every optional output NULL: rms and inliers do not change
    L = __import__('pdfnet_amd.hip', fromlist=['lib']).lib()
    rms, inl = torch.empty(3, 2, device='cuda'), torch.empty(3, 2, dtype=torch.int32, device='cuda')
    L.pdf_mesh_icp(v.data_ptr(), f.data_ptr(), c.data_ptr(), va.data_ptr(), 3, 778, faces.shape[1], P_TEMPLATE, 8, TRIM, 1, None, None, None,
                   rms.data_ptr(), inl.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(rms, first[3]) and torch.equal(inl, first[4])


# ---- refined_sums and Trainer.evaluation(refined=...) --------------------------------------------------
def test_refined_sums_on_a_hand_made_tuple():
    from pdfnet_amd.trains.base_trainer import REFINE_ITERS, REFINE_TRIM, finish_refined, refined_sums
    verts, gt, faces, cloud, valid = template_scene()
    assert (REFINE_ITERS, REFINE_TRIM) == (8, TRIM)
    g = np.random.default_rng(3)
    jp = (verts[:, :, :21] + g.normal(0, 0.002, (3, 2, 21, 3))).astype(np.float32)        # "joints": 21 points that move with the hand
    jg = gt[:, :, :21].astype(np.float32)
    z = torch.zeros(3, 2, 21, 3, device='cuda')
    tup = (cu(verts), cu(jp), cu(gt.astype(np.float32)), cu(jg), z, z, z, z, z)
    batch = {'cloud': cu(cloud), 'valid': cu(valid)}
    for rigid in (False, True):
        got = refined_sums(tup, batch, cu(faces), rigid)
        assert got.dtype == torch.float64 and got.shape == (17,) and got.is_cuda
        got = got.cpu().numpy()
        r0, r1 = template_ref(0, False), template_ref(8, rigid)
        want = np.zeros(17)
        want[0] = 3
        for b in range(3):
            for h in range(2):
                if valid[b, h] != 1:
                    continue
                jr = jp[b, h].astype(np.float64) @ r1['R'][b, h].T + r1['t'][b, h]
                live = (cloud[b, h, :, 2] > 0).sum()
                terms = (np.linalg.norm(jr - jg[b, h], axis=-1).mean(), np.linalg.norm(r1['out'][b, h] - gt[b, h].astype(np.float32), axis=-1).mean(),
                         r0['rms'][b, h], r1['rms'][b, h], r1['inliers'][b, h] / max(live, 1), 1.0, float(r0['inliers'][b, h] > 0),
                         float(r1['inliers'][b, h] > 0))
                for k, x in enumerate(terms):
                    want[1 + 2 * k + h] += x
        print("  %s got %s\n  want %s" % ('rigid' if rigid else 'translation', got.tolist(), want.tolist()))
        # three samples a sum; per sample 1e-6 m: the bar on out_verts (1.2e-7 m) moves a mean distance by no more than itself, and
        # point_dist_sum adds up to 778 fp32 distances of about 2 cm (a sum near 16, ulp 1e-6, divided by 778 again)
        bar = 3e-6
        assert np.array_equal(got[[0, 11, 12, 13, 14, 15, 16]], want[[0, 11, 12, 13, 14, 15, 16]]) and got[11] == 2 and got[12] == 3 and got[16] == 2
        assert np.abs(got[1:9] - want[1:9]).max() <= bar and np.abs(got[9:11] - want[9:11]).max() <= 1e-12
        out = finish_refined(torch.from_numpy(got))
        assert abs(out['ref_abs_left_verts'] - got[3] / 2 * 1000) <= 1e-9 and abs(out['ref_abs_right_verts'] - got[4] / 3 * 1000) <= 1e-9
        assert out['ref_cloud_res_mm'] < out['cloud_res_mm'] and out['refined_samples'] == 3
    with pytest.raises(KeyError, match="cloud"):
        refined_sums(tup, {'valid': batch['valid']}, cu(faces))


@functools.lru_cache(maxsize=None)
def evaluation_runs():
    """The fixture of tests/test_render_gpu.py::evaluation_runs: R = 128, B = 3, two batches, random-init model."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer, refined_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 3
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev))
    loader = [synthetic_train_batch(B, R, seed=s, consts=consts) for s in (21, 22)]
    runs = {'plain': tr.evaluation(loader), 'off': tr.evaluation(loader, refined=False), 'on': tr.evaluation(loader, refined=True),
            'translation': tr.evaluation(loader, refined='translation'), 'rigid': tr.evaluation(loader, refined='rigid'),
            'others': tr.evaluation(loader, aligned=True, interaction=True, rendered=True),
            'all': tr.evaluation(loader, aligned=True, interaction=True, rendered=True, refined=True),
            'all_rigid': tr.evaluation(loader, aligned=True, interaction=True, rendered=True, refined='rigid'),
            'interaction': tr.evaluation(loader, interaction=True), 'interaction_on': tr.evaluation(loader, interaction=True, refined=True),
            'rendered': tr.evaluation(loader, rendered=True), 'rendered_on': tr.evaluation(loader, rendered=True, refined='rigid'),
            'aligned': tr.evaluation(loader, aligned=True), 'aligned_on': tr.evaluation(loader, aligned=True, refined=True)}
    assert m.training
    with pytest.raises(KeyError, match="cloud"):
        tr.evaluation([{k: v for k, v in b.items() if k != 'cloud'} for b in loader], refined=True)
    with pytest.raises(ValueError):
        tr.evaluation(loader, refined='affine')
    assert m.training
    sums = {rigid: torch.zeros(17, dtype=torch.float64, device=dev) for rigid in (False, True)}
    tr.model_with_loss.eval()
    with torch.no_grad():
        for b in loader:
            bd = tree_to({k: v for k, v in b.items() if torch.is_tensor(v)}, dev)
            tup = tr.model_with_loss(bd, 'test', None)
            for rigid in sums:
                sums[rigid] += refined_sums(tup, bd, tr.model_with_loss.loss.faces_pair, rigid)
    tr.model_with_loss.train()
    return runs, {k: v.cpu() for k, v in sums.items()}


def test_evaluation_refined_keys():
    """The plumbing (the synthetic clouds are random): the flag off changes nothing; the flag on changes no other key, alone or with `aligned`,
    `interaction` (whose block is read from the end of the shared buffer) and `rendered`; the new keys are finish_refined of the summed
    refined_sums; a batch without `cloud` raises KeyError."""
    from pdfnet_amd.trains.base_trainer import REFINED_KEYS, finish_refined
    runs, sums = evaluation_runs()
    plain = runs['plain']
    assert plain['samples'] == 6 and runs['off'] == plain and list(runs['off']) == list(plain)
    assert runs['on'] == runs['translation']
    for base, on, mode in ((plain, runs['on'], False), (plain, runs['rigid'], True), (runs['others'], runs['all'], False),
                           (runs['others'], runs['all_rigid'], True), (runs['interaction'], runs['interaction_on'], False),
                           (runs['rendered'], runs['rendered_on'], True), (runs['aligned'], runs['aligned_on'], False)):
        assert sorted(on) == sorted(list(base) + list(REFINED_KEYS))
        for k, v in base.items():
            assert on[k] == v, k
        want = finish_refined(sums[mode])
        assert list(want) == list(REFINED_KEYS) and want['refined_samples'] == 6
        for k in REFINED_KEYS:
            assert np.isfinite(on[k]) and abs(on[k] - want[k]) <= 1e-12, (k, on[k], want[k])
    for k in REFINED_KEYS:
        print("  %-22s translation %.6g rigid %.6g" % (k, runs['on'][k], runs['rigid'][k]))
    assert 0.0 <= runs['on']['ref_inlier_share'] <= 1.0 and runs['on']['cloud_res_mm'] >= 0
