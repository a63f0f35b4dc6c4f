"""The visibility-aware mesh-to-cloud loss on the GPU (csrc/meshcloud.hip pdf_mesh_cloud_loss, F.mesh_cloud_loss, CtdetLoss's mesh_cloud_weight
term, Trainer.evaluation(two_sided=True)) against a float64 numpy restatement of the contract in include/pdfnet_hip.h: a vertex is visible
when it is a corner of a camera-facing triangle of its hand and the ray from it to the camera meets no camera-facing triangle of either hand
(its own incident ones apart) more than `margin` metres in front of it; a visible vertex is matched to its nearest sensor point; the loss is
the mean of |v - p|^2 over the matches closer than `trim`, with the gradient (2/m)(v - p).  No reference program has this feature, so the
contract is all there is to pin to.

Discrete outputs are checked by rules that rounding cannot break.  The restatement computes visibility twice.  A vertex is SURELY HIDDEN when
no triangle that faces the camera or lies within FACING_EPS of the threshold holds it, or when an occluder that faces the camera by more than
FACING_EPS hides it with every normalised edge value sgn(S) s_k / (|v| |o'| |t'|) >= +EDGE_EPS (o', t' the edge's corners relative to the
vertex) and the margin taken as margin + MARGIN_EPS; it is SURELY VISIBLE when a triangle facing the camera by more than FACING_EPS holds it
and no occluder, facing or within the band, hides it with the edge values >= -EDGE_EPS and the margin taken as margin - MARGIN_EPS.  The
kernel's `vis` must be 0 on the first set and 1 on the second; the rest may be either, and a row fails when more than AMBIGUOUS_CAP of its
vertices are in it.  (A triangle with two equal corner indices -- the padding of the test meshes -- is in no band: its normal is exactly 0 in
fp32 as in float64.)  `nn`: the float64 squared distance of the chosen point is at most (1 + 16 * 2^-24) times the float64 minimum over the
usable points (two fp32 evaluations of a three-term sum of squares).

loss, grad, inliers and visible are compared with the restatement GIVEN the kernel's vis and nn, so that no vertex is excluded and a tie
cannot break the comparison; before that the float64 side asserts that no matched distance lies within TRIM_MARGIN of the trim.  The bars are
derived, not measured: v - p is one fp32 subtraction of a difference below trim, the squares are summed in fp32, the row in double and the
result is rounded once: loss within 8 * 2^-24 * trim^2 (4.3e-10 m^2 at 0.03 m), grad within 8 * 2^-24 * 2 * trim (2.9e-8).  The measured
maxima are printed, and profiles/NOTES.md has them.  tests/test_mesh_cloud_loss_cpu.py checks the input conditions of every seeded case
here in float64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_cloud_loss_gpu import grid_mesh
from tests.test_eval_interaction_gpu import template
from tests.test_icp_gpu import EMPTY, FACING_EPS, INVALID, TET, TRI, TRIM, TRIM_MARGIN, _dot, cu, ref_facing, sample_cloud, template_scene
from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

MARGIN = 0.002
EDGE_EPS, MARGIN_EPS, AMBIGUOUS_CAP = 1e-5, 1e-5, 0.01
NN_BAND = 1.0 + 16.0 * 2.0 ** -24
TIGHT_TRIM = 0.012                                                 # rejects part of the template scene's visible vertices


def loss_bar(trim):
    return 8.0 * 2.0 ** -24 * trim * trim


def grad_bar(trim):
    return 8.0 * 2.0 ** -24 * 2.0 * trim


# ---- float64 restatement -----------------------------------------------------------------------
def _edge(v, O, T, io, it):
    """v [m, 1, 3], O, T [1, F, 3], io, it [F] their vertex indices -> (v . ((o - v) x (t - v)) evaluated from the corner with the lower index to
    the other one and negated when that is T -> O, |o - v| |t - v|), both [m, F]."""
    first = (io <= it)[None, :, None]
    lo, hi = np.where(first, O, T) - v, np.where(first, T, O) - v
    val = _dot(v, np.cross(lo, hi))
    return np.where(first[..., 0], val, -val), np.linalg.norm(lo, axis=-1) * np.linalg.norm(hi, axis=-1)


def ref_hides(V, A, B, C, idx, own, margin):
    """Vertices V [n, 3] against the occluders (A, B, C [F, 3], their vertex indices idx [F, 3], own [F] bool: a triangle of the vertices' own
    hand, which never hides its corners) -> three bool [n, F]: hides by the contract, surely hides, possibly hides (module docstring)."""
    n, F = len(V), len(A)
    out = [np.zeros((n, F), bool) for _ in range(3)]
    if F == 0:
        return out
    for lo in range(0, n, 64):
        v = V[lo:lo + 64, None]
        L = np.linalg.norm(v, axis=-1)
        s, scale = zip(_edge(v, B[None], C[None], idx[:, 1], idx[:, 2]), _edge(v, C[None], A[None], idx[:, 2], idx[:, 0]),
                       _edge(v, A[None], B[None], idx[:, 0], idx[:, 1]))
        det = _dot(A[None] - v, np.cross(B[None] - v, C[None] - v))
        S = s[0] + s[1] + s[2]
        sg, area = np.sign(S), np.abs(S)
        D = -sg * det
        mine = own[None] & (idx[None] == np.arange(lo, lo + v.shape[0])[:, None, None]).any(-1)
        nk = [np.where(L * sc > 0, sg * x / np.where(L * sc > 0, L * sc, 1.0), 0.0) for x, sc in zip(s, scale)]
        between = (S != 0) & (D < area) & ~mine
        for k, (tol, mg) in enumerate(((None, margin), (EDGE_EPS, margin + MARGIN_EPS), (-EDGE_EPS, margin - MARGIN_EPS))):
            inside = (sg * s[0] >= 0) & (sg * s[1] >= 0) & (sg * s[2] >= 0) if tol is None else (nk[0] >= tol) & (nk[1] >= tol) & (nk[2] >= tol)
            out[k][lo:lo + 64] = inside & between & (D * L > mg * area)
    return out


def ref_visibility(V, faces, Vo, faces_o, valid, valid_o, margin):
    """One (sample, hand): its vertices V [n, 3] and faces, the other hand's Vo and faces_o -> dict of bool [n]: vis (the contract in float64),
    sure_hidden, sure_visible."""
    n = len(V)
    if valid == 0:
        return {'vis': np.zeros(n, bool), 'sure_hidden': np.ones(n, bool), 'sure_visible': np.zeros(n, bool)}
    parts, fronts = [], None
    for W, f, own in ((V, faces, True), (Vo, faces_o, False)):
        if not own and valid_o == 0:
            continue
        f = np.clip(f, 0, n - 1)
        s, sn = ref_facing(W, f)
        # (a triangle with two equal corner indices has a normal of exactly 0 in fp32 as in float64: it is in no band)
        proper = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
        exact, sure, loose = s < 0, (s < 0) & (sn < -FACING_EPS), proper & ((s < 0) | (sn < FACING_EPS))
        if own:
            fronts = [np.isin(np.arange(n), f[m].ravel()) for m in (exact, sure, loose)]
        keep = np.nonzero(loose)[0]
        parts.append((W[f[keep, 0]], W[f[keep, 1]], W[f[keep, 2]], f[keep], np.full(len(keep), own), exact[keep], sure[keep]))
    A, B, C, idx, own, exact, sure = (np.concatenate(x) for x in zip(*parts))
    hides, surely, possibly = ref_hides(V, A, B, C, idx, own, margin)
    return {'vis': fronts[0] & ~(hides & exact[None]).any(1), 'sure_hidden': ~fronts[2] | (surely & sure[None]).any(1),
            'sure_visible': fronts[1] & ~possibly.any(1)}


def ref_nearest(V, cloud):
    """-> (nn [n] the usable point at the smallest squared distance, lowest index first, -1 without one; d2 [n] that squared distance, inf; second
    [n] the squared distance of the runner-up, inf)."""
    n = len(V)
    use = np.nonzero(cloud[:, 2] > 0)[0]
    if not len(use):
        return np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    d2 = ((V[:, None] - cloud[use][None]) ** 2).sum(-1)
    k = d2.argmin(1)
    best = d2[np.arange(n), k]
    rest = d2.copy()
    rest[np.arange(n), k] = np.inf
    return use[k], best, rest.min(1)


def ref_given(V, cloud, vis, nn, trim):
    """loss, inliers, visible, grad [n, 3], inlier [n], dist [n] (inf without a match) of one row in float64, given the visible set and the match."""
    V, cloud = np.asarray(V, np.float64), np.asarray(cloud, np.float64)
    vis, nn = np.asarray(vis, bool), np.asarray(nn, np.int64)
    out = {'loss': 0.0, 'inliers': 0, 'visible': int(vis.sum()), 'grad': np.zeros_like(V), 'inlier': np.zeros(len(V), bool), 'dist': np.full(len(V), np.inf)}
    m = vis & (nn >= 0)
    if m.any():
        r = V[m] - cloud[nn[m]]
        out['dist'][m] = np.linalg.norm(r, axis=-1)
        inl = out['inlier'] = out['dist'] < trim
        k = out['inliers'] = int(inl.sum())
        if k:
            out['loss'] = float((out['dist'][inl] ** 2).sum() / k)
            out['grad'][inl] = (2.0 / k) * (V[inl] - cloud[nn[inl]])
    return out


def ref_row(verts, faces, cloud, valid, b, h, trim, margin):
    """Row (b, h) of pdf_mesh_cloud_loss in float64 on its own visibility and match -> ref_visibility's dict plus nn, d2, second, and ref_given's."""
    V, Vo, pts = verts[b, h].astype(np.float64), verts[b, 1 - h].astype(np.float64), cloud[b, h].astype(np.float64)
    va, vo = (1, 1) if valid is None else (valid[b, h], valid[b, 1 - h])
    out = ref_visibility(V, faces[h], Vo, faces[1 - h], va, vo, margin)
    nn, d2, second = ref_nearest(V, pts)
    out.update(nn=np.where(out['vis'], nn, -1), d2=d2, second=second)
    out.update(ref_given(V, pts, out['vis'], out['nn'], trim))
    return out


# ---- running and comparing -----------------------------------------------------------------------
KEYS = ('loss', 'inliers', 'visible', 'vis', 'nn')


def run(verts, faces, cloud, valid=None, trim=TRIM, margin=MARGIN, g=None):
    """-> the fields of F.mesh_cloud_loss as numpy arrays plus 'grad': verts.grad after (loss * g).sum().backward(), g = 1 by default, so that
    grad is the kernel's own output times exactly 1."""
    from pdfnet_amd import functional as F
    v = cu(np.asarray(verts, np.float32)).requires_grad_()
    got = F.mesh_cloud_loss(v, cu(faces), cu(np.asarray(cloud, np.float32)), None if valid is None else cu(valid), trim=trim, margin=margin,
                            return_fields=True)
    (got[0] * (torch.ones_like(got[0]) if g is None else cu(g))).sum().backward()
    torch.cuda.synchronize()
    out = {k: x.detach().cpu().numpy() for k, x in zip(KEYS, got)}
    out['grad'] = v.grad.cpu().numpy()
    return out


WORST = {'loss': 0.0, 'grad': 0.0, 'ambiguous': 0.0, 'nn': 0.0}


def check(got, verts, faces, cloud, valid, trim, margin, label):
    """Every row of `got` by the rules of the module docstring -> the restatement's rows {(b, h): dict}."""
    verts, cloud = np.asarray(verts, np.float32), np.asarray(cloud, np.float32)
    n, refs = verts.shape[2], {}
    assert all(np.isfinite(got[k]).all() for k in got)
    for b in range(verts.shape[0]):
        for h in range(2):
            vis, nn = got['vis'][b, h], got['nn'][b, h]
            r = refs[(b, h)] = ref_row(verts, faces, cloud, valid, b, h, trim, margin)
            assert set(np.unique(vis)) <= {0, 1}
            assert (vis[r['sure_hidden']] == 0).all(), (label, b, h, np.nonzero(r['sure_hidden'] & (vis != 0))[0])
            assert (vis[r['sure_visible']] == 1).all(), (label, b, h, np.nonzero(r['sure_visible'] & (vis != 1))[0])
            share = float((~r['sure_hidden'] & ~r['sure_visible']).mean())
            assert share <= AMBIGUOUS_CAP, (label, b, h, share)
            V, pts = verts[b, h].astype(np.float64), cloud[b, h].astype(np.float64)
            usable = pts[:, 2] > 0
            assert (nn[vis == 0] == -1).all(), (label, b, h)
            ratio = 1.0
            if usable.any():
                m = vis == 1
                assert (nn[m] >= 0).all() and usable[nn[m]].all(), (label, b, h)
                if m.any():
                    ratio = float((((V[m] - pts[nn[m]]) ** 2).sum(-1) / np.maximum(r['d2'][m], 1e-300)).max())
                    assert ratio <= NN_BAND, (label, b, h, ratio)
            else:
                assert (nn == -1).all(), (label, b, h)
            given = ref_given(V, pts, vis, nn, trim)
            hit = np.isfinite(given['dist'])
            assert not hit.any() or np.abs(given['dist'][hit] - trim).min() >= TRIM_MARGIN, (label, b, h)
            assert got['inliers'][b, h] == given['inliers'] and got['visible'][b, h] == given['visible'], (label, b, h, got['inliers'][b, h], given)
            el, eg = abs(float(got['loss'][b, h]) - given['loss']), float(np.abs(got['grad'][b, h] - given['grad']).max())
            assert el <= loss_bar(trim) and eg <= grad_bar(trim), (label, b, h, el, loss_bar(trim), eg, grad_bar(trim))
            assert (got['grad'][b, h][~given['inlier']] == 0).all(), (label, b, h)
            for k, x in (('loss', el / loss_bar(trim)), ('grad', eg / grad_bar(trim)), ('ambiguous', share), ('nn', ratio - 1.0)):
                WORST[k] = max(WORST[k], x)
            print("  %s row (%d, %d): visible %d of %d, inliers %d, ambiguous %.2f %%, loss err %.3e m^2 (bar %.2e), grad err %.3e (bar %.2e), "
                  "nn ratio - 1 %.2e" % (label, b, h, given['visible'], n, given['inliers'], 100 * share, el, loss_bar(trim), eg, grad_bar(trim),
                                         ratio - 1.0))
    return refs


# ---- inputs ----------------------------------------------------------------------------------------
FAR = np.array([[5.0, 5.0, 9.0], [5.0, 5.1, 9.0], [5.1, 5.0, 9.0]])      # a hand that is nowhere near: a facing triangle far off the rays


def pair(left, right, pts_left, pts_right=None):
    """Two small meshes (V [n_h, 3], tris [F_h, 3]) as the hands of one sample, padded to a common n with copies of vertex 0 and to a common Fc
    with zero-area faces -> (verts [1, 2, n, 3] float32, faces [2, Fc, 3], cloud [1, 2, P, 3] float32)."""
    (Vl, fl), (Vr, fr) = [(np.asarray(V, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)) for V, f in (left, right)]
    n, Fc = max(len(Vl), len(Vr)), max(len(fl), len(fr))
    V = [np.concatenate((W, np.repeat(W[:1], n - len(W), 0))) for W in (Vl, Vr)]
    f = [np.concatenate((x, np.zeros((Fc - len(x), 3), np.int64))) for x in (fl, fr)]
    pl = np.asarray(pts_left, np.float32).reshape(-1, 3)
    pr = pl if pts_right is None else np.asarray(pts_right, np.float32).reshape(-1, 3)
    return np.stack(V)[None].astype(np.float32), np.stack(f), np.stack((pl, pr))[None]


def alone(V, tris, pts, **kw):
    """A small mesh as the left hand beside the far triangle -> the left hand's outputs (checked against the restatement)."""
    args = pair((V, tris), (FAR, [0, 1, 2]), pts)
    got = run(*args, **kw)
    check(got, *args, None, kw.get('trim', TRIM), kw.get('margin', MARGIN), "alone")
    return {k: v[0, 0] for k, v in got.items()}


# three points 10, 20 and 30 mm from the corners a, b, c of TRI, each nearest to its own corner; a fourth behind the camera
TRI_POINTS = np.array([[0.0, 0.0, 0.49], [-0.02, 0.1, 0.5], [0.1, -0.03, 0.5], [0.0, 0.0, -0.49]], np.float32)
TRI_TRIMS = ((0.05, 3), (0.015, 1), (0.005, 0))
# margins of the hand values: the float32 0.1, 0.49 ... are up to 3e-8 m off the decimal numbers, so v - p moves by up to 6e-8 m:
# |v - p|^2 by 2 * 0.03 * 6e-8 = 3.6e-9 m^2, a gradient coordinate by 2 * 6e-8 = 1.2e-7; the kernel's own rounding is within the derived bars
HAND_BARS = {'loss': 5e-9, 'grad': 2e-7}
OCCLUDER = np.array([[-0.5, -0.5, 0.4], [-0.5, 1.0, 0.4], [1.0, -0.5, 0.4]])      # wound like TRI: faces the camera; every ray from TRI crosses it
# a quad at Z = 0.25 over [0, 0.125]^2 split along the diagonal (0, 0) - (0.125, 0.125), both halves wound like TRI
QUAD = (np.array([[0.0, 0.0, 0.25], [0.0, 0.125, 0.25], [0.125, 0.125, 0.25], [0.125, 0.0, 0.25]]), np.array([[0, 1, 2], [0, 2, 3]]))


def small_facing(at):
    """A triangle wound like TRI with its first corner at `at` and legs of 2^-6 m (exact in binary) -> (V [3, 3], tris)."""
    at = np.asarray(at, np.float64)
    return np.stack((at, at + [0, 0.015625, 0], at + [0.015625, 0, 0])), np.array([[0, 1, 2]])


def rect_mesh(rows, cols, z=0.5, pitch=0.004, shift=(0.0, 0.0)):
    """rows x cols vertices at depth z, triangulated like grid_mesh (facing the camera) -> (V [rows * cols, 3], tris)."""
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing='ij')
    V = np.stack((shift[0] + pitch * (j - (cols - 1) / 2), shift[1] + pitch * (i - (rows - 1) / 2), np.full(i.shape, z)), -1).reshape(-1, 3)
    c = (i[:-1, :-1] * cols + j[:-1, :-1]).ravel()
    return V.astype(np.float32), np.concatenate((np.stack((c, c + cols, c + 1), -1), np.stack((c + cols + 1, c + 1, c + cols), -1))).astype(np.int64)


SIZE_SHAPES = {1: (1, 1), 63: (7, 9), 65: (5, 13)}
# seeds for which the input conditions hold (tests/test_mesh_cloud_loss_cpu.py checks them)
SIZE_SEEDS = {(1, 1): 101, (1, 63): 163, (1, 65): 165, (1, 1024): 1124, (63, 1): 6301, (63, 63): 6364, (63, 65): 6365, (63, 1024): 7324,
              (65, 1): 6501, (65, 63): 6563, (65, 65): 6565, (65, 1024): 7524}
SIZE_TRIM = 0.01


def size_case(n, P):
    """The left hand a small grid at Z = 0.5, the right one the same grid 3 cm nearer and a third of its width across, so that it hides part of
    the left; P random points around both; padded with zero-area faces to Fc = 200."""
    rows, cols = SIZE_SHAPES[n]
    if n == 1:
        left = right = (np.array([[0.0, 0.0, 0.5]]), np.zeros((1, 3), np.int64))
    else:
        left, right = rect_mesh(rows, cols), rect_mesh(rows, cols, z=0.47, shift=(0.004 * cols / 3 + 0.0013, 0.001))
    g = np.random.default_rng(SIZE_SEEDS[(n, P)])
    pts = np.concatenate((g.uniform(-0.03, 0.03, (P, 2)), g.uniform(0.46, 0.51, (P, 1))), -1).astype(np.float32)
    pts[::7, 2] *= -1                                              # every seventh point is behind the camera (P = 1: the only one)
    verts, faces, cloud = pair(left, right, pts, pts[::-1])
    pad = np.zeros((2, 200 - faces.shape[1], 3), np.int64)
    return verts, np.concatenate((faces, pad), 1), cloud


GRID_SEEDS = {1: 11, 1024: 1031}          # likewise; the single point has inliers among the first hand's visible vertices


def grid_case(P):
    """grid_mesh() (n = 1,024, Fc = 2,048, 1,922 facing) as both hands, the second 5 cm nearer and half a grid across (and 1.1 / 0.7 mm off the
    lattice, so that no ray runs through one of its edges): it hides part of the first, and each hand alone has more facing occluders than one list holds."""
    V, tris = grid_mesh()
    g = np.random.default_rng(GRID_SEEDS[P])
    pts = np.concatenate((g.uniform(-0.12, 0.2, (P, 2)), g.uniform(0.38, 0.57, (P, 1))), -1).astype(np.float32)
    return np.stack((V, V + np.array([0.0811, 0.0007, -0.05], np.float32)))[None].astype(np.float32), np.stack((tris, tris)), np.stack((pts, pts[::-1]))[None]


@functools.lru_cache(maxsize=None)
def interacting_pair():
    """The left template hand at (0.03, 0, 0.46) in front of the right one at (0.05, 0, 0.5): most of the right hand's camera-facing vertices
    are hidden only by the left hand.  Clouds from sample_cloud on each hand's own surface.  -> (verts [1, 2, 778, 3], faces, cloud)."""
    left, right, faces = template()
    V = np.stack((left.astype(np.float64) + (0.03, 0.0, 0.46), right.astype(np.float64) + (0.05, 0.0, 0.5)))
    cloud = np.stack([sample_cloud(V[h], faces[h], 1000, 31 + h) for h in range(2)])
    return V[None].astype(np.float32), faces, cloud[None]


@functools.lru_cache(maxsize=None)
def template_got(trim):
    verts, _, faces, cloud, valid = template_scene()
    return run(verts, faces, cloud, valid, trim=trim)


# ---- hand-made cases ---------------------------------------------------------------------------------
def test_one_triangle_by_hand():
    p = TRI_POINTS.astype(np.float64)
    d = np.linalg.norm(TRI.astype(np.float64) - p[:3], axis=-1)     # 10, 20, 30 mm
    for trim, want in TRI_TRIMS:
        got = alone(TRI, [0, 1, 2], TRI_POINTS, trim=trim)
        m = d < trim
        assert (got['vis'] == 1).all() and got['visible'] == 3 and np.array_equal(got['nn'], [0, 1, 2])
        assert got['inliers'] == want == m.sum(), (trim, got['inliers'])
        loss = (d[m] ** 2).mean() if want else 0.0
        grad = np.where(m[:, None], (2.0 / max(want, 1)) * (TRI - p[:3]), 0.0)
        assert abs(got['loss'] - loss) <= HAND_BARS['loss'], (trim, got['loss'], loss)
        assert np.abs(got['grad'] - grad).max() <= HAND_BARS['grad'] and (got['grad'][~m] == 0).all(), (trim, got['grad'], grad)


def test_a_point_with_z_zero_or_less_is_never_matched():
    pts = TRI_POINTS.copy()
    pts[0, 2] = -0.49                                              # what was the nearest point of corner a
    got = alone(TRI, [0, 1, 2], pts, trim=0.2)
    assert (got['vis'] == 1).all() and got['nn'][0] in (1, 2) and np.array_equal(got['nn'][1:], [1, 2]) and got['inliers'] == 3
    pts[:, 2] = (0.0, -0.5, -0.5, 0.0)                             # no usable point: visibility as usual, the rest 0
    got = alone(TRI, [0, 1, 2], pts, trim=0.2)
    assert (got['vis'] == 1).all() and got['visible'] == 3 and (got['nn'] == -1).all()
    assert got['loss'] == 0 and got['inliers'] == 0 and (got['grad'] == 0).all()


def test_reversed_winding_is_not_visible():
    got = alone(TRI, [0, 2, 1], TRI_POINTS, trim=0.05)
    assert got['visible'] == 0 and (got['vis'] == 0).all() and got['loss'] == 0 and got['inliers'] == 0
    assert (got['grad'] == 0).all() and (got['nn'] == -1).all()


def test_an_occluder_of_the_same_hand_and_of_the_other_hand():
    both = (np.concatenate((TRI, OCCLUDER)), [[0, 1, 2], [3, 4, 5]])
    got = alone(*both, TRI_POINTS, trim=0.05)
    assert np.array_equal(got['vis'], [0, 0, 0, 1, 1, 1]) and (got['nn'][:3] == -1).all() and (got['grad'][:3] == 0).all()
    got = alone(both[0], [[0, 1, 2], [3, 5, 4]], TRI_POINTS, trim=0.05)        # the occluder turned away
    assert np.array_equal(got['vis'], [1, 1, 1, 0, 0, 0]) and got['inliers'] == 3
    for tris, valid, want in (([0, 1, 2], (1, 1), 0), ([0, 1, 2], (1, 0), 1), ([0, 2, 1], (1, 1), 1)):
        args = pair((TRI, [0, 1, 2]), (OCCLUDER, tris), TRI_POINTS)
        va = np.array([valid], np.float32)
        got = run(*args, va, trim=0.05)
        check(got, *args, va, 0.05, MARGIN, "occluding hand %s %s" % (tris, valid))
        assert (got['vis'][0, 0] == want).all() and got['visible'][0, 0] == 3 * want and got['inliers'][0, 0] == 3 * want, (tris, valid)
        assert (got['nn'][0, 0] == (np.arange(3) if want else -1)).all()


def test_the_margin():
    """A plane 1 mm in front of TRI (1.0 to 1.02 mm along the rays) hides nothing at margin 2 mm and everything at margin 0; at 3 mm it hides."""
    for dz, margin, want in ((0.001, 0.002, 1), (0.003, 0.002, 0), (0.001, 0.0, 0), (0.003, 0.0, 0)):
        occ = OCCLUDER.copy()
        occ[:, 2] = 0.5 - dz
        for args in (pair((np.concatenate((TRI, occ)), [[0, 1, 2], [3, 4, 5]]), (FAR, [0, 1, 2]), TRI_POINTS), pair((TRI, [0, 1, 2]), (occ, [0, 1, 2]), TRI_POINTS)):
            got = run(*args, trim=0.05, margin=margin)
            check(got, *args, None, 0.05, margin, "margin %g dz %g" % (margin, dz))
            assert (got['vis'][0, 0, :3] == want).all(), (dz, margin, got['vis'][0, 0])


def test_a_ray_through_a_shared_edge_and_through_a_shared_vertex_is_hit():
    """Every coordinate is exact in binary, so each s_k on the diagonal (and at the corner) is exactly 0: the vertex is hidden, there is no gap."""
    for at in ((0.0625, 0.0625, 0.5), (0.25, 0.25, 0.5), (0.0, 0.0, 0.5), (0.125, 0.125, 0.5)):      # through the diagonal; through its two ends
        V, tris = small_facing(at)
        for margin in (MARGIN, 0.0):
            same = run(*pair((np.concatenate((V, QUAD[0])), np.concatenate((tris, QUAD[1] + 3))), (FAR, [0, 1, 2]), TRI_POINTS), margin=margin)
            other = run(*pair((V, tris), QUAD, TRI_POINTS), margin=margin)
            assert same['vis'][0, 0, 0] == 0 and other['vis'][0, 0, 0] == 0, (at, margin)
            assert (same['vis'][0, 0, 3:7] == 1).all() and (other['vis'][0, 1, :4] == 1).all()
        clear = run(*pair((V, tris), (QUAD[0], QUAD[1][:, ::-1]), TRI_POINTS))      # the quad turned away hides nothing
        assert (clear['vis'][0, 0, :3] == 1).all()


def test_own_corners_never_hide():
    V, tris = TET
    got = alone(V, tris, TRI_POINTS, trim=0.2, margin=0.0)
    assert got['vis'][0] == 1 and got['nn'][0] == 0                # the apex, held by three facing triangles
    assert (got['vis'] == 1).all()                                 # the base corners look past the apex' faces


# ---- sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 65, 1024])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_sizes_that_are_no_multiple_of_64(n, P):
    verts, faces, cloud = size_case(n, P)
    assert verts.shape == (1, 2, n, 3) and faces.shape == (2, 200, 3) and cloud.shape == (1, 2, P, 3)
    got = run(verts, faces, cloud, trim=SIZE_TRIM)
    refs = check(got, verts, faces, cloud, None, SIZE_TRIM, MARGIN, "n=%d P=%d" % (n, P))
    if n == 1:
        assert (got['visible'] == 0).all() and (got['nn'] == -1).all() and (got['loss'] == 0).all()
    else:
        assert 0 < got['visible'][0, 0] < n and got['visible'][0, 1] == n      # the right hand hides part of the left and nothing hides it
        assert np.array_equal(got['vis'][0, 0] == 1, refs[(0, 0)]['vis'])


@pytest.mark.parametrize("P", [1, 1024])
def test_the_largest_mesh(P):
    verts, faces, cloud = grid_case(P)
    assert verts.shape == (1, 2, 1024, 3) and faces.shape == (2, 2048, 3)
    assert all((ref_facing(verts[0, h].astype(np.float64), faces[h])[0] < 0).sum() == 1922 for h in range(2))
    got = run(verts, faces, cloud, trim=TRIM)
    refs = check(got, verts, faces, cloud, None, TRIM, MARGIN, "grid P=%d" % P)
    assert 0 < got['visible'][0, 0] < 1024 and got['visible'][0, 1] == 1024
    assert np.array_equal(got['vis'][0, 0] == 1, refs[(0, 0)]['vis'])
    assert got['inliers'][0, 0] > 0 and (P == 1 or (got['inliers'] < got['visible']).all())      # the trim rejects something


# ---- template hands --------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", [TRIM, TIGHT_TRIM])
def test_template_hands_against_the_restatement(trim):
    verts, _, faces, cloud, valid = template_scene()
    got = template_got(trim)
    check(got, verts, faces, cloud, valid, trim, MARGIN, "template trim %g" % trim)
    rows = [(b, h) for b in range(3) for h in range(2) if (b, h) not in (INVALID, EMPTY)]
    share = np.array([1.0 - got['inliers'][r] / got['visible'][r] for r in rows])
    print("  template trim %g: rejected share per row %s" % (trim, np.round(share, 3).tolist()))
    assert (share == 0).all() if trim == TRIM else ((share > 0.05) & (share < 0.6)).all()
    b, h = INVALID
    assert got['loss'][b, h] == 0 and got['inliers'][b, h] == 0 and got['visible'][b, h] == 0 and (got['vis'][b, h] == 0).all()
    assert (got['grad'][b, h] == 0).all() and (got['nn'][b, h] == -1).all()
    b, h = EMPTY
    assert got['visible'][b, h] > 0 and got['vis'][b, h].sum() == got['visible'][b, h]
    assert got['loss'][b, h] == 0 and got['inliers'][b, h] == 0 and (got['grad'][b, h] == 0).all() and (got['nn'][b, h] == -1).all()


def test_interacting_hands():
    """The row the feature is for: the left hand in front of the right one.  Without the left hand most of what it hides is visible again."""
    verts, faces, cloud = interacting_pair()
    got = run(verts, faces, cloud)
    refs = check(got, verts, faces, cloud, None, TRIM, MARGIN, "interacting")
    off = np.array([[0, 1]], np.float32)
    solo = run(verts, faces, cloud, off)
    check(solo, verts, faces, cloud, off, TRIM, MARGIN, "interacting, left hand off")
    by_left = int(((solo['vis'][0, 1] == 1) & (got['vis'][0, 1] == 0)).sum())
    print("  interacting: right hand visible %d with the left hand, %d without: %d hidden only by the left hand" % (
        got['visible'][0, 1], solo['visible'][0, 1], by_left))
    assert by_left > 200 and not ((solo['vis'][0, 1] == 0) & (got['vis'][0, 1] == 1)).any()
    assert int((refs[(0, 1)]['vis'] != (got['vis'][0, 1] == 1)).sum()) <= 0.01 * 778
    print("  measured maxima so far: loss %.3f of its bar, grad %.3f of its bar, ambiguous share %.4f, nn ratio - 1 %.2e" % (
        WORST['loss'], WORST['grad'], WORST['ambiguous'], WORST['nn']))


def test_determinism_rows_alone_and_optional_outputs():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    f, c, va = cu(faces), cu(cloud), cu(valid)

    def call(sl=slice(None)):
        v = cu(verts)[sl].requires_grad_()
        out = F.mesh_cloud_loss(v, f, c[sl], va[sl], return_fields=True)
        out[0].sum().backward()
        return tuple(out) + (v.grad,)
    first, second = call(), call()
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    for b in range(verts.shape[0]):
        assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, call(slice(b, b + 1)))), b
    # every optional output NULL: loss, inliers and visible do not change
    L = __import__('pdfnet_amd.hip', fromlist=['lib']).lib()
    v, loss = cu(verts), torch.empty(3, 2, device='cuda')
    inl, seen = torch.empty(3, 2, dtype=torch.int32, device='cuda'), torch.empty(3, 2, dtype=torch.int32, device='cuda')
    L.pdf_mesh_cloud_loss(v.data_ptr(), f.data_ptr(), c.data_ptr(), va.data_ptr(), 3, 778, faces.shape[1], cloud.shape[2], TRIM, MARGIN, loss.data_ptr(),
                          inl.data_ptr(), seen.data_ptr(), None, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(loss, first[0]) and torch.equal(inl, first[1]) and torch.equal(seen, first[2])
    assert torch.equal(F.mesh_cloud_loss(v, f, c, va), first[0])


def test_autograd():
    from pdfnet_amd import functional as F
    verts, _, faces, cloud, valid = template_scene()
    g = np.array([[0.5, -2.0], [3.0, 0.25], [1.5, 7.0]], np.float32)
    unit, scaled = template_got(TRIM), run(verts, faces, cloud, valid, g=g)
    assert np.array_equal(scaled['grad'], g[..., None, None] * unit['grad']) and np.array_equal(scaled['loss'], unit['loss'])
    assert (unit['grad'] != 0).any()
    v, f, c = cu(verts).requires_grad_(), cu(faces), cu(cloud).requires_grad_()
    out = F.mesh_cloud_loss(v, f, c, cu(valid), return_fields=True)
    assert len(out) == 5 and out[0].requires_grad and not any(x.requires_grad for x in out[1:])
    out[0].sum().backward()
    assert v.grad is not None and c.grad is None and f.grad is None
    with torch.no_grad():
        quiet = F.mesh_cloud_loss(v, f, c, cu(valid))
    assert not quiet.requires_grad and torch.equal(quiet, out[0])
    assert np.array_equal(quiet.cpu().numpy(), unit['loss'])


def test_refusals():
    from pdfnet_amd import functional as F, hip
    c = hip.lib().cdll
    v, f, p = torch.zeros(1, 2, 1025, 3, device='cuda'), torch.zeros(2, 2049, 3, dtype=torch.long, device='cuda'), torch.zeros(1, 2, 1025, 3, device='cuda')
    outs = [torch.full((2,), 7.0, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'), torch.full((2,), 7, dtype=torch.int32, device='cuda'),
            torch.full((1, 2, 1025, 3), 7.0, device='cuda'), torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda'),
            torch.full((1, 2, 1025), 7, dtype=torch.int32, device='cuda')]
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(n=4, Fc=4, P=4, trim=0.03, margin=0.002, B=1, skip=None):
        o = [None if k == skip else P_(x) for k, x in enumerate(outs)]
        return c.pdf_mesh_cloud_loss(P_(v), P_(f), P_(p), None, B, n, Fc, P, ctypes.c_float(trim), ctypes.c_float(margin), *o, None)
    nan, inf = float('nan'), float('inf')
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(P=0), dict(P=1025), dict(trim=0.0), dict(trim=-1.0), dict(trim=inf),
               dict(trim=nan), dict(margin=-1e-9), dict(margin=inf), dict(margin=nan), dict(skip=0), dict(skip=1), dict(skip=2)):
        assert call(**kw) == -1, kw
    assert c.pdf_mesh_cloud_loss(None, P_(f), P_(p), None, 1, 4, 4, 4, ctypes.c_float(0.03), ctypes.c_float(0.0), *[P_(x) for x in outs], None) == -1
    assert call(B=0) == 0 and call(B=-1) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    x, fa, cl = v[:, :, :4], f[:, :4], p[:, :, :4]
    for bad in (lambda: F.mesh_cloud_loss(v, fa, cl), lambda: F.mesh_cloud_loss(x, f, cl), lambda: F.mesh_cloud_loss(x, fa, p),
                lambda: F.mesh_cloud_loss(x, fa, cl, trim=0.0), lambda: F.mesh_cloud_loss(x, fa, cl, trim=nan), lambda: F.mesh_cloud_loss(x, fa, cl[0]),
                lambda: F.mesh_cloud_loss(x, fa, cl, margin=-0.001), lambda: F.mesh_cloud_loss(x, fa, cl, margin=inf),
                lambda: F.mesh_cloud_loss(x, fa, cl, margin=nan), lambda: F.mesh_cloud_loss(x[:, :1], fa, cl[:, :1]),
                lambda: F.mesh_cloud_loss(x, fa, cl, valid=torch.ones(2, 2, device='cuda'))):
        with pytest.raises(ValueError):
            bad()
    assert F.mesh_cloud_loss(x, fa, cl, margin=0.0).shape == (1, 2)


# ---- the training term ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_training_term(fused, monkeypatch):
    """tests/test_cloud_loss_gpu.py::test_training_term for mesh_cloud_weight, with its fixture, CLOUD_TRIM and GRAD_NOISE_BAR (see there for why
    the parameter gradients are compared by a norm): absent / 0 enters no new code (the new functions are replaced by ones that raise), leaves
    loss and statistics bit-equal and the autograd graph the same; 0.01 adds 0.01 * mesh_cloud_term to the loss within one ulp, reports it,
    and moves the decoder gradients; both weights on report 'cloud_loss' then 'mesh_cloud_loss'."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains import simplified
    from tests.test_cloud_loss_gpu import CLOUD_TRIM, GRAD_NOISE_BAR, gradient_distance, train_step, trainer_fixture
    R, _, _, batch = trainer_fixture()
    monkeypatch.setattr(F, 'MESH_LOSS_FUSED', fused)
    real = (simplified.mesh_cloud_term, F.mesh_cloud_loss)

    def never(*a, **k):
        raise AssertionError("the mesh-to-cloud term ran with mesh_cloud_weight 0 or absent")
    monkeypatch.setattr(simplified, 'mesh_cloud_term', never)
    monkeypatch.setattr(F, 'mesh_cloud_loss', never)
    absent, zero = train_step(), train_step(mesh_cloud_weight=0, cloud_trim=CLOUD_TRIM)
    monkeypatch.setattr(simplified, 'mesh_cloud_term', real[0])
    monkeypatch.setattr(F, 'mesh_cloud_loss', real[1])
    on = train_step(mesh_cloud_weight=0.01, cloud_trim=CLOUD_TRIM)
    assert torch.equal(absent[0], zero[0]) and list(absent[1]) == list(zero[1]) and 'mesh_cloud_loss' not in zero[1]
    assert all(torch.equal(torch.as_tensor(absent[1][k]), torch.as_tensor(zero[1][k])) for k in absent[1])
    assert absent[5] == zero[5] and list(absent[2]) == list(zero[2])
    off = gradient_distance(zero[2], absent[2])[0]
    assert off <= GRAD_NOISE_BAR, off
    loss, stats, grads, (result, params, hand, other_info), crit, nodes = on
    ml = stats['mesh_cloud_loss']
    assert list(stats) == list(zero[1]) + ['mesh_cloud_loss'] and ml.shape == (3,) and bool(torch.isfinite(ml).all()) and bool((ml > 0).all())
    assert len(nodes) > len(zero[5])
    for k in zero[1]:
        if k != 'loss':
            assert torch.equal(torch.as_tensor(stats[k]), torch.as_tensor(zero[1][k])), k
    with torch.no_grad():
        direct = simplified.mesh_cloud_term(simplified._pair(result['verts3d']), simplified._pair(params['root']), batch['ind'], batch,
                                            crit.faces_pair, R, 4, CLOUD_TRIM, 0.002)
    assert torch.equal(direct, ml.detach()) and torch.equal(stats['loss'], loss)
    diff = (loss.double() - zero[0].double() - 0.01 * ml.detach().double()).abs().cpu().numpy()
    ulp = np.spacing(np.abs(loss.cpu().numpy()))
    print("  fused=%s loss %s mesh_cloud_loss mm^2 %s |loss - loss_off - 0.01 mesh_cloud_loss| %s ulp %s" % (fused, loss.tolist(), ml.tolist(), diff, ulp))
    assert (diff <= ulp).all()
    assert list(grads) == list(zero[2]) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    dec = [k for k in grads if k.startswith('decoder.')]
    moved = gradient_distance({k: grads[k] for k in dec}, {k: zero[2][k] for k in dec})[0]
    print("  fused=%s absent vs 0: %.3e of the gradients' norm; the term on moves the mesh-decoder gradients by %.3e of theirs" % (fused, off, moved))
    assert dec and moved > GRAD_NOISE_BAR
    both = train_step(cloud_weight=0.01, mesh_cloud_weight=0.01, cloud_trim=CLOUD_TRIM)
    assert list(both[1]) == list(zero[1]) + ['cloud_loss', 'mesh_cloud_loss'] and torch.equal(both[1]['mesh_cloud_loss'], ml)
    with pytest.raises(KeyError, match="cloud"):
        crit(result, params, hand, other_info, {k: v for k, v in batch.items() if k != 'cloud'}, 'train', 0)


# ---- Trainer.evaluation(two_sided=True) ------------------------------------------------------------------------
def test_two_sided_sums_on_a_hand_made_tuple():
    from pdfnet_amd.trains.base_trainer import REFINE_TRIM, TWO_SIDED_MARGIN, TWO_SIDED_SUMS, finish_two_sided, two_sided_sums
    from tests.test_icp_gpu import template_ref
    verts, gt, faces, cloud, valid = template_scene()
    assert (REFINE_TRIM, TWO_SIDED_MARGIN, TWO_SIDED_SUMS) == (TRIM, MARGIN, 21)
    z = torch.zeros(3, 2, 21, 3, device='cuda')
    tup = (cu(verts), z, cu(gt.astype(np.float32)), z, z, z, z, z, z)
    batch = {'cloud': cu(cloud), 'valid': cu(valid)}
    got = two_sided_sums(tup, batch, cu(faces))
    assert got.dtype == torch.float64 and got.shape == (21,) and got.is_cuda
    got = got.cpu().numpy()
    pred, truth, r0 = template_got(TRIM), run(gt.astype(np.float32), faces, cloud, valid), template_ref(0, False)
    want = np.zeros(21)
    want[0] = 3
    for b in range(3):
        for h in range(2):
            if valid[b, h] != 1:
                continue
            terms = (np.sqrt(np.float64(pred['loss'][b, h])), pred['visible'][b, h] / 778, pred['inliers'][b, h] / max(pred['visible'][b, h], 1),
                     np.sqrt(np.float64(truth['loss'][b, h])), r0['rms'][b, h], 1.0, float(pred['inliers'][b, h] > 0), float(pred['visible'][b, h] > 0),
                     float(truth['inliers'][b, h] > 0), float(r0['inliers'][b, h] > 0))
            for k, x in enumerate(terms):
                want[1 + 2 * k + h] += x
    print("  got %s\n  want %s" % (got.tolist(), want.tolist()))
    assert np.array_equal(got[11:], want[11:]) and got[0] == 3 and got[11] == 2 and got[12] == 3
    assert np.abs(got[1:9] - want[1:9]).max() <= 1e-12 and np.abs(got[9:11] - want[9:11]).max() <= 3 * 5.6e-10      # (test_icp_gpu's bar on rms at iters 0, three samples a sum)
    out = finish_two_sided(torch.from_numpy(got))
    assert out['gt_mesh_cloud_mm'] < out['mesh_cloud_mm'] and out['two_sided_samples'] == 3 and 0 < out['visible_share'] < 1
    with pytest.raises(KeyError, match="cloud"):
        two_sided_sums(tup, {'valid': batch['valid']}, cu(faces))


def test_evaluation_two_sided_keys():
    """The plumbing, on the fixture of tests/test_icp_gpu.py::evaluation_runs (R = 128, B = 3, two batches, random-init model; the synthetic clouds
    are random): the flag off changes nothing, the flag on changes no other key, alone or with every other block; cloud_mesh_mm is the refined
    block's cloud_res_mm; a batch without `cloud` raises KeyError."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import TWO_SIDED_KEYS, Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 3
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev))
    loader = [synthetic_train_batch(B, R, seed=s, consts=consts) for s in (21, 22)]
    plain, off, on = tr.evaluation(loader), tr.evaluation(loader, two_sided=False), tr.evaluation(loader, two_sided=True)
    others = tr.evaluation(loader, aligned=True, interaction=True, rendered=True, refined=True)
    every = tr.evaluation(loader, aligned=True, interaction=True, rendered=True, refined=True, two_sided=True)
    assert m.training and plain['samples'] == 6 and off == plain and list(off) == list(plain)
    for base, with_it in ((plain, on), (others, every)):
        assert sorted(with_it) == sorted(list(base) + list(TWO_SIDED_KEYS))
        for k, v in base.items():
            assert with_it[k] == v, k
        for k in TWO_SIDED_KEYS:
            assert np.isfinite(with_it[k]) and with_it[k] == on[k], k
    assert on['two_sided_samples'] == 6 and on['cloud_mesh_mm'] == others['cloud_res_mm']
    assert 0.0 <= on['visible_share'] <= 1.0 and 0.0 <= on['covered_share'] <= 1.0
    assert on['chamfer_mm'] == (on['cloud_mesh_mm'] + on['mesh_cloud_mm']) / 2
    for k in TWO_SIDED_KEYS:
        print("  %-20s %.6g" % (k, on[k]))
    with pytest.raises(KeyError, match="cloud"):
        tr.evaluation([{k: v for k, v in b.items() if k != 'cloud'} for b in loader], two_sided=True)
    assert m.training


def test_finish_two_sided_on_a_hand_made_accumulator():
    from pdfnet_amd.trains.base_trainer import TWO_SIDED_KEYS, TWO_SIDED_SUMS, finish_two_sided
    acc = torch.zeros(TWO_SIDED_SUMS, dtype=torch.float64)
    acc[0] = 4
    acc[1:3] = torch.tensor([0.004, 0.008], dtype=torch.float64)        # rms of the prediction: 3 hands with an inlier -> 4 mm
    acc[13:15] = torch.tensor([1.0, 2.0], dtype=torch.float64)
    acc[3:5] = torch.tensor([1.0, 1.5], dtype=torch.float64)            # visible / n over 5 valid hands -> 0.5
    acc[11:13] = torch.tensor([2.0, 3.0], dtype=torch.float64)
    acc[5:7] = torch.tensor([1.5, 1.5], dtype=torch.float64)            # inliers / visible over 4 hands with a visible vertex -> 0.75
    acc[15:17] = torch.tensor([2.0, 2.0], dtype=torch.float64)
    acc[7:9] = torch.tensor([0.001, 0.002], dtype=torch.float64)        # the ground truth: 3 hands -> 1 mm
    acc[17:19] = torch.tensor([1.0, 2.0], dtype=torch.float64)
    acc[9:11] = torch.tensor([0.004, 0.006], dtype=torch.float64)       # cloud to mesh: 5 hands -> 2 mm
    acc[19:21] = torch.tensor([2.0, 3.0], dtype=torch.float64)
    out = finish_two_sided(acc)
    assert list(out) == list(TWO_SIDED_KEYS)
    want = {'mesh_cloud_mm': 4.0, 'gt_mesh_cloud_mm': 1.0, 'cloud_mesh_mm': 2.0, 'chamfer_mm': 3.0, 'visible_share': 0.5, 'covered_share': 0.75,
            'two_sided_samples': 4}
    assert all(abs(out[k] - want[k]) <= 1e-12 for k in want), out
