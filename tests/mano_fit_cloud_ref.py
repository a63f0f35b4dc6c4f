"""Restatement of `pdf_mano_cloud_targets` and `pdf_mano_fit_cloud` (include/pdfnet_hip.h), written from those comments, and the scene the
CPU and the GPU tests share.  The association is tests/test_icp_gpu.py's rule (camera-facing triangles, seven regions, lowest face among
equals, strict trim) with tests/test_cloud_loss_gpu.py's weights; the inner loop is tests/mano_fit_ref.py's `fit`.  Every function runs in the
dtype of the arrays it is given: float64 is the reference, float32 on the CPU shows what an fp32 evaluation of the same formulas loses.

The synthetic MANO constants of oracle.synth have a random template, so there is no anatomical face list: `template_faces` triangulates the
template as a star-shaped surface about its centroid (the convex hull of the vertices' directions: every vertex is used, 2 n - 4 = 1,552
faces, closed, oriented outwards)."""
import functools

import numpy as np
import torch

from tests import mano_fit_ref as R
from tests.test_cloud_loss_gpu import ref_closest_weights
from tests.test_icp_gpu import TRIM, ref_facing, sample_cloud

NV = R.NV


# ---- a face list for the synthetic template -----------------------------------------------------------------
def sphere_hull(U):
    """U [n, 3] unit vectors, the origin inside their hull -> faces [2 n - 4, 3] of their convex hull, oriented outwards (incremental: the
    faces a new point sees are replaced by the fan from it to their horizon)."""
    n = len(U)
    first = [0, 1, 2, next(i for i in range(3, n) if abs(np.linalg.det(U[[1, 2, i]] - U[0])) > 1e-6)]
    inner = U[first].mean(0)
    faces = []
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        a, b, c = first[a], first[b], first[c]
        faces.append((a, b, c) if np.dot(np.cross(U[b] - U[a], U[c] - U[a]), U[a] - inner) > 0 else (a, c, b))
    faces = np.array(faces)
    for p in range(n):
        if p in first:
            continue
        A, B, C = U[faces[:, 0]], U[faces[:, 1]], U[faces[:, 2]]
        sees = ((np.cross(B - A, C - A) * (U[p] - A)).sum(-1) > 0)
        assert sees.any()
        edges = {(f[k], f[(k + 1) % 3]) for f in faces[sees] for k in range(3)}
        fan = [(a, b, p) for a, b in edges if (b, a) not in edges]
        faces = np.concatenate((faces[~sees], np.array(fan)))
    return faces.astype(np.int64)


def signed_volume(V, faces):
    A, B, C = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    return float((np.cross(A, B) * C).sum() / 6.0)


@functools.lru_cache(maxsize=None)
def template_faces(side='left'):
    v = R.consts_of(side)['v_template'].numpy()
    d = v - v.mean(0)
    return sphere_hull(d / np.linalg.norm(d, axis=-1, keepdims=True))


# ---- pdf_mano_cloud_targets ---------------------------------------------------------------------------------
def associate(V, faces, cloud):
    """-> tri [P] (-1: ignored point or no camera-facing triangle), bary [P, 3], closest [P, 3] in the dtype of V: every live point against
    every camera-facing triangle, the smallest squared distance, the lowest face among equals."""
    P = len(cloud)
    tri, bary, closest = np.full(P, -1, np.int64), np.zeros((P, 3), V.dtype), np.zeros((P, 3), V.dtype)
    faces = np.clip(faces, 0, len(V) - 1)
    idx = np.nonzero(ref_facing(V, faces)[0] < 0)[0]
    live = np.nonzero(cloud[:, 2] > 0)[0]
    if len(idx) and len(live):
        A, B, C = (V[faces[idx, k]][None] for k in range(3))
        q, w = ref_closest_weights(cloud[live][:, None], A, B, C)
        k = ((cloud[live][:, None] - q) ** 2).sum(-1).argmin(1)                  # (the first of equal minima: idx ascends)
        rows = np.arange(len(live))
        tri[live], bary[live], closest[live] = idx[k], w[rows, k], q[rows, k]
    return tri, bary, closest


def targets(V, faces, cloud, valid=1, trim=TRIM, anchor=None, alpha=0.0, fields=None):
    """One row of pdf_mano_cloud_targets in the dtype of V -> dict: target [n, 3], weight [n], W [n], S [n, 3], rms, inliers, tri, bary,
    closest, dist [P] (inf where tri = -1), inlier [P], absS [n, 3] = sum w |d| per coordinate (what the fp32 error of S scales with).
    fields = (tri, bary, closest): take the association from there (the kernel's own) instead of making it."""
    dt = V.dtype
    cloud = cloud.astype(dt)
    n, P = len(V), len(cloud)
    alpha = dt.type(alpha if anchor is not None else 0.0)
    if valid == 0 or not (cloud[:, 2] > 0).any():
        tri, bary, closest = np.full(P, -1, np.int64), np.zeros((P, 3), dt), np.zeros((P, 3), dt)
    elif fields is None:
        tri, bary, closest = associate(V, faces, cloud)
    else:
        tri, bary, closest = np.asarray(fields[0], np.int64), fields[1].astype(dt), fields[2].astype(dt)
    d = cloud - closest
    dist = np.where(tri >= 0, np.linalg.norm(d, axis=-1), np.inf)
    m = dist < trim
    W, S, absS = np.zeros(n, dt), np.zeros((n, 3), dt), np.zeros((n, 3), dt)
    corners = np.clip(faces, 0, n - 1)[np.where(m, tri, 0)]
    for k in range(3):
        np.add.at(W, corners[m, k], bary[m, k])
        np.add.at(S, corners[m, k], bary[m, k:k + 1] * d[m])
        np.add.at(absS, corners[m, k], bary[m, k:k + 1] * np.abs(d[m]))
    den = W + alpha
    a = anchor.astype(dt) if anchor is not None else np.zeros_like(V)
    with np.errstate(divide='ignore', invalid='ignore'):
        target = np.where(W[:, None] > 0, (W[:, None] * V + S + alpha * a) / den[:, None], a if alpha > 0 else V)
    return {'target': target, 'weight': den, 'W': W, 'S': S, 'absS': absS, 'rms': float(np.sqrt((dist[m] ** 2).mean())) if m.any() else 0.0,
            'inliers': int(m.sum()), 'tri': tri, 'bary': bary, 'closest': closest, 'dist': dist, 'inlier': m}


def association_energy(M, faces, cloud, t):
    """sum over the inliers of t (a `targets` result) of |sum_k w_ik M_k - p_i|^2: the point-to-surface energy with the association held."""
    m = t['inlier']
    k = faces[t['tri'][m]]
    q = (t['bary'][m][:, :, None] * M[k]).sum(1)
    return float(((q - cloud[m]) ** 2).sum())


def surrogate_energy(M, V, t):
    """sum_v W_v |M_v - (v + S_v / W_v)|^2 + const with const = sum_i |d_i|^2 - sum_v |S_v|^2 / W_v, so that it equals the association energy
    at M = V."""
    on = t['W'] > 0
    W, S = t['W'][on, None], t['S'][on]
    const = float((t['dist'][t['inlier']] ** 2).sum() - ((S ** 2) / W).sum())
    return float((W * (M[on] - V[on] - S / W) ** 2).sum()) + const


# ---- pdf_mano_fit_cloud ---------------------------------------------------------------------------------------
def fit_cloud(consts, faces, cloud, init, side='left', valid=1, anchor=None, alpha=0.0, outer=4, inner=3, trim=TRIM, prior_pose=0.0,
              prior_shape=0.0):
    """The loop of the contract in the dtype of init (a torch vector [61]; consts in that dtype) -> dict: p, verts [778, 3] (torch), rms
    [outer + 1], inliers [outer + 1], accepted [outer]."""
    dt = init.dtype
    p = init.clone()
    mesh = lambda q: R.model(consts, q, side)[0]
    rms, inl, acc = [], [], []
    with R.default_dtype(dt):
        for o in range(outer + 1):
            t = targets(mesh(p).numpy(), faces, cloud, valid, trim, anchor, alpha)
            rms.append(t['rms'])
            inl.append(t['inliers'])
            if o == outer:
                break
            f = R.fit(consts, torch.from_numpy(t['target']).to(dt), side, weight=torch.from_numpy(t['weight']).to(dt), init=p, iters=inner,
                      prior_pose=prior_pose, prior_shape=prior_shape, valid=bool(valid))
            p = f['p']
            acc.append(f['accepted'])
        verts = mesh(p)
    return {'p': p, 'verts': verts, 'rms': rms, 'inliers': inl, 'accepted': acc}


# ---- the scene ------------------------------------------------------------------------------------------------
SCENE_SEED, SCENE_P, SCENE_NOISE = 122, 200, 0.001
OUTER, INNER = 4, 3


@functools.lru_cache(maxsize=None)
def scene(seed=SCENE_SEED, side='left'):
    """-> dict: p_true [61] float64 (a state of tests/mano_fit_ref.py::case's magnitude, pose std 0.5, 0.45 m in front of the camera), gt [778,
    3] float64 = M(p_true), faces, cloud [200, 3] float32 on the camera-facing surface of gt with 1 mm noise, init [61] float32 = p_true with
    the translation moved by 1 cm and 0.1 rad of pose noise, visible [778] bool: the corners of gt's camera-facing triangles."""
    p, _ = R.case(seed, 0.5, side)
    p[58:] = torch.tensor([0.03, -0.02, 0.45], dtype=torch.float64)
    with R.default_dtype(torch.float64):
        gt = R.model(R.consts_of(side), p, side)[0].numpy()
    faces = template_faces(side)
    cloud = sample_cloud(gt, faces, SCENE_P, 100 + seed, SCENE_NOISE)
    g = np.random.default_rng(200 + seed)
    init = p.clone()
    init[:48] += torch.from_numpy(0.1 * g.standard_normal(48))
    shift = g.standard_normal(3)
    init[58:] += torch.from_numpy(0.01 * shift / np.linalg.norm(shift))
    visible = np.zeros(NV, bool)
    visible[faces[ref_facing(gt, faces)[0] < 0].ravel()] = True
    return {'p_true': p, 'gt': gt, 'faces': faces, 'cloud': cloud, 'init': init.float(), 'visible': visible}


@functools.lru_cache(maxsize=None)
def scene_fit(dtype=torch.float64, seed=SCENE_SEED, side='left'):
    """The restatement's OUTER x INNER steps on the scene in `dtype` (from the float32-rounded init, as the kernel starts)."""
    s = scene(seed, side)
    return fit_cloud(R.consts_of(side, dtype), s['faces'], s['cloud'], s['init'].to(dtype), side, outer=OUTER, inner=INNER)


def visible_distance(verts, s):
    """mean distance of the scene's visible vertices to the generating mesh, metres"""
    return float(np.linalg.norm(np.asarray(verts, np.float64) - s['gt'], axis=-1)[s['visible']].mean())
