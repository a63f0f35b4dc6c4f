"""Inter-hand penetration, contact distance and MRRPE on the GPU (csrc/metrics.hip pdf_mesh_penetration, F.mesh_penetration,
Trainer.evaluation(interaction=True)) against a float64 numpy restatement: the generalized winding number as the sum of the triangles'
Van Oosterom-Strackee solid angles / 4 pi, and the point-to-triangle distance by the closest point in the seven regions (three vertices, three
edges, the face) of Ericson's Real-Time Collision Detection 5.1.5.

Meshes come from committed data: the right hand is (dense_coor - mean) * 0.2 m of pdfnet_amd/data/gcn_core.npz with mesh_faces_right, the left
hand its mirror in x with mesh_faces_left.

Bars: wind 5.6e-6 absolute.  It started at 1e-5 (an fp32 numpy restatement of the same sum is within 3.8e-7 of float64 on these meshes; the
kernel's atan2f is not numpy's: a 25-fold margin); the kernel's measured maximum is 1.39e-6 (template hands, 1,538 atan2f terms per vertex), and
the bar is four times that.  dist, depth, gap 1e-6 m + 1e-5 relative (the bar of the nearest-neighbour distances); count exact.  A count is
discontinuous at wind = 0.5, so every exact comparison first checks ON THE FLOAT64 SIDE that no vertex has |wind - 0.5| < 1e-3 and that none
lies within 1e-7 m of the other surface (there the winding number itself jumps).  That is a condition on the inputs: no vertex is excluded."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

WIND_BAR = 5.6e-6
WIND_MARGIN, SURFACE_MARGIN = 1e-3, 1e-7
SHIFTS = ((0.25, 0.0, 0.0), (0.06, 0.01, 0.0), (0.02, 0.0, 0.03))     # of the left hand, metres; the right hand stays at the origin


# ---- float64 restatement -----------------------------------------------------------------------
def _dot(u, v):
    return (u * v).sum(-1)


def ref_wind(P, A, B, C):
    """Queries P [n, 3], triangle corners A, B, C [F, 3] -> winding numbers [n] (float64)."""
    a, b, c = A[None] - P[:, None], B[None] - P[:, None], C[None] - P[:, None]
    la, lb, lc = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1), np.linalg.norm(c, axis=-1)
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)


def ref_tri_dist(P, A, B, C):
    """Queries P [n, 3], triangle corners [F, 3] -> [n, F] distances from each query to the closest point of each triangle, the closest
    point taken by region: vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, face -- the first whose test holds."""
    A, B, C, P = A[None], B[None], C[None], P[:, None]
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
    d = np.linalg.norm(P - q, axis=-1)
    assert np.isfinite(d).all()
    return d


def ref_row(P, V, faces):
    """Vertices P [n, 3] against the mesh (V [m, 3], faces [F, 3]) -> (wind [n], dist [n]) in float64."""
    P, V = P.astype(np.float64), V.astype(np.float64)
    A, B, C = V[faces[:, 0]], V[faces[:, 1]], V[faces[:, 2]]
    return ref_wind(P, A, B, C), ref_tri_dist(P, A, B, C).min(-1)


def ref_penetration(verts, faces):
    """verts [B, 2, n, 3], faces [2, F, 3] -> dict of float64 wind, dist [B, 2, n], count [B, 2] (int), depth, gap [B, 2]."""
    wind, dist = np.zeros(verts.shape[:-1]), np.zeros(verts.shape[:-1])
    for b in range(verts.shape[0]):
        for h in range(2):
            wind[b, h], dist[b, h] = ref_row(verts[b, h], verts[b, 1 - h], faces[1 - h])
    inside = wind > 0.5
    return {'wind': wind, 'dist': dist, 'count': inside.sum(-1), 'depth': np.where(inside, dist, 0.0).max(-1), 'gap': dist.min(-1)}


def well_conditioned(ref):
    """The condition for an exact count comparison (module docstring), on the float64 side."""
    return np.abs(ref['wind'] - 0.5).min() >= WIND_MARGIN and ref['dist'].min() >= SURFACE_MARGIN


# ---- inputs --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def template():
    """-> (left [778, 3], right [778, 3] float32 metres, faces [2, 1538, 3] int64 (left, right))."""
    import os
    import pdfnet_amd
    z = np.load(os.path.join(os.path.dirname(pdfnet_amd.__file__), 'data', 'gcn_core.npz'))
    d = z['dense_coor'].astype(np.float64)
    right = ((d - d.mean(0)) * 0.2).astype(np.float32)
    left = right * np.array([-1, 1, 1], np.float32)
    return left, right, np.stack((z['mesh_faces_left'], z['mesh_faces_right'])).astype(np.int64)


def hands(shifts):
    """One sample per shift: the left template hand moved by it, the right one at the origin -> [B, 2, 778, 3] float32."""
    left, right, _ = template()
    return np.stack([np.stack((left + np.asarray(s, np.float32), right)) for s in shifts])


@functools.lru_cache(maxsize=None)
def template_case():
    verts, faces = hands(SHIFTS), template()[2]
    return verts, faces, ref_penetration(verts, faces)


def run(verts, faces):
    from pdfnet_amd import functional as F
    out = F.mesh_penetration(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), return_fields=True)
    return {k: v.cpu().numpy().astype(np.int64 if k == 'count' else np.float64) for k, v in zip(('count', 'depth', 'gap', 'wind', 'dist'), out)}


def check(got, ref, counts=True, label=""):
    ew = np.abs(got['wind'] - ref['wind']).max()
    ed = np.abs(got['dist'] - ref['dist']).max()
    print("  %s wind err max %.3e, dist err max %.3e (dist max %.3e), depth err %.3e, gap err %.3e" % (
        label, ew, ed, ref['dist'].max(), np.abs(got['depth'] - ref['depth']).max(), np.abs(got['gap'] - ref['gap']).max()))
    assert all(np.isfinite(v).all() for v in got.values())
    assert ew <= WIND_BAR, ew
    for k in ('dist', 'depth', 'gap'):
        assert (np.abs(got[k] - ref[k]) <= 1e-6 + 1e-5 * np.abs(ref[k])).all(), (k, np.abs(got[k] - ref[k]).max())
    if counts:
        assert well_conditioned(ref)
        assert np.array_equal(got['count'], ref['count']), (got['count'], ref['count'])


# ---- pdf_mesh_penetration ------------------------------------------------------------------------
TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * 0.05
TET_FACES = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)


def test_tetrahedron_pair():
    """B = 1, n = 4, Fc = 4: fewer vertices than a wave.  Two outward-oriented regular tetrahedra, the second moved by (40, 40, -40) mm:
    its corner (-50, -50, 50) mm lands at (-10, -10, 10) mm inside the first, nothing else is inside anything."""
    for f in TET_FACES:                                           # outward: the normal points away from the centroid (the origin)
        assert np.dot(np.cross(TET[f[1]] - TET[f[0]], TET[f[2]] - TET[f[0]]), TET[f].mean(0)) > 0
    second = TET + np.array([0.04, 0.04, -0.04])
    verts = np.stack((TET, second))[None].astype(np.float32)      # hand 0 = the first, hand 1 = the second
    faces = np.stack((TET_FACES, TET_FACES))
    ref = ref_penetration(verts, faces)
    assert ref['count'].tolist() == [[0, 1]], ref['count']
    got = run(verts, faces)
    check(got, ref, label="tetrahedra")
    inside = int(np.argmax(ref['wind'][0, 1]))
    want = np.zeros((1, 2, 4))
    want[0, 1, inside] = 1.0
    assert np.abs(got['wind'] - want).max() <= WIND_BAR
    assert got['count'].tolist() == [[0, 1]] and got['depth'][0, 0] == 0.0
    assert abs(got['depth'][0, 1] - ref['dist'][0, 1, inside]) <= 1e-6 + 1e-5 * ref['dist'][0, 1, inside]


def test_single_triangle():
    """Fc = 1, n = 5: queries above and below the triangle, in its plane outside it, at one of its corners, and off to the side.  wind is the
    signed fractional solid angle; reversing the index order negates it and leaves dist alone."""
    tri = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.3, 0.3, 0.3], [0.3, 0.3, 0.3]], np.float32)       # corners 0, 1, 2; the rest unused
    q = np.array([[0.02, 0.03, 0.05], [0.02, 0.03, -0.05], [0.2, 0.2, 0.0], [0.1, 0.0, 0.0], [-0.05, 0.02, 0.01]], np.float32)
    verts = np.stack((q, tri))[None]                               # hand 0 = the queries, hand 1 carries the triangle
    for order in ((0, 1, 2), (0, 2, 1)):
        faces = np.array([[[0, 0, 0]], [order]], np.int64)        # hand 0's own "mesh": one degenerate face
        ref = ref_penetration(verts, faces)
        got = run(verts, faces)
        check(got, ref, counts=False, label="triangle %s" % (order,))
        if order == (0, 1, 2):
            first = got
            assert ref['wind'][0, 0, 0] < -0.01 and ref['wind'][0, 0, 1] > 0.01         # (seen from +z the corners run counter-clockwise)
    assert got['wind'][0, 0, 2] == 0.0 and first['wind'][0, 0, 2] == 0.0               # in the plane
    assert got['wind'][0, 0, 3] == 0.0 and got['dist'][0, 0, 3] == 0.0                 # at a corner
    # float64 is exactly antisymmetric and both runs are within the bars of it (checked above): twice the bars between the two runs
    assert np.abs(got['wind'][0, 0] + first['wind'][0, 0]).max() <= 2 * WIND_BAR
    assert (np.abs(got['dist'][0, 0] - first['dist'][0, 0]) <= 2 * (1e-6 + 1e-5 * first['dist'][0, 0])).all()
    assert (got['wind'][0, 1] == 0.0).all()                                            # against the degenerate face
    assert np.abs(got['dist'][0, 1] - np.linalg.norm(tri.astype(np.float64) - q[0].astype(np.float64), axis=-1)).max() <= 1e-6


def test_template_hands():
    """B = 3, n = 778, Fc = 1538: apart (no vertex inside, gap about 110 mm) and two interpenetrating poses, all five outputs, both ways."""
    verts, faces, ref = template_case()
    print("  float64 counts %s, gap %s mm, depth %s mm" % (ref['count'].tolist(), (ref['gap'] * 1000).round(2).tolist(), (ref['depth'] * 1000).round(2).tolist()))
    assert ref['count'][0].tolist() == [0, 0] and abs(ref['gap'][0, 0] - 0.110) < 0.005 and (ref['depth'][0] == 0).all()
    assert ref['count'][1:, 0].tolist() == [121, 180] and (ref['count'][1:, 1] > 50).all()     # left in right; right in left
    check(run(verts, faces), ref, label="template")


def test_the_caps():
    """n = 1024 (vertices repeated) and Fc = 2048 (degenerate faces (0, 0, 0) appended).  A repeated vertex has its original's values; a
    degenerate face adds no solid angle, and its distance is that to vertex 0, which lies on the surface already: the float64 figures of the
    first 778 vertices are those of the unpadded case, and each count grows by the repeated vertices that are inside."""
    verts, faces, ref = template_case()
    rep = np.arange(1024) % 778
    pv = verts[:, :, rep]
    pf = np.concatenate((faces, np.zeros((2, 2048 - faces.shape[1], 3), np.int64)), 1)
    want = {'wind': ref['wind'][..., rep], 'dist': ref['dist'][..., rep]}
    inside = want['wind'] > 0.5
    want.update(count=inside.sum(-1), depth=ref['depth'], gap=ref['gap'])
    assert np.array_equal(want['count'], ref['count'] + (ref['wind'][..., :1024 - 778] > 0.5).sum(-1))
    got = run(pv, pf)
    check(got, want, label="caps")
    from pdfnet_amd import functional as F
    c, vp = F._L().cdll, ctypes.c_void_p
    x = torch.zeros(1, 2, 1025, 3, device='cuda')
    f = torch.zeros(2, 2049, 3, dtype=torch.int64, device='cuda')
    o = torch.zeros(8, device='cuda')
    args = lambda n, Fc: (vp(x.data_ptr()), vp(f.data_ptr()), 1, n, Fc, None, None, vp(o.data_ptr()), vp(o.data_ptr()), vp(o.data_ptr()), None)
    assert c.pdf_mesh_penetration(*args(1025, 4)) == -1 and c.pdf_mesh_penetration(*args(4, 2049)) == -1
    assert c.pdf_mesh_penetration(None, None, 0, 4, 4, None, None, None, None, None, None) == 0
    for call in (lambda: F.mesh_penetration(x, f[:, :4]), lambda: F.mesh_penetration(x[:, :, :4], f), lambda: F.mesh_penetration(x[:, :1, :4], f[:, :4]),
                 lambda: F.mesh_penetration(x[:, :, :4, :2], f[:, :4])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        F.mesh_penetration(x[:, :, :4].cpu(), f[:, :4].cpu())


def test_invalid_hand_is_all_zeros():
    """H2O marks an invalid hand with zeros: everything stays finite, nothing counts as inside either way."""
    verts, faces, _ = template_case()
    for h in range(2):
        v = verts[1:2].copy()
        v[:, h] = 0
        got = run(v, faces)
        assert all(np.isfinite(x).all() for x in got.values())
        assert got['count'].tolist() == [[0, 0]] and (got['depth'] == 0).all()
        assert (got['wind'][0, 1 - h] == 0).all()                 # against a mesh collapsed to a point
        want = np.linalg.norm(v[0, 1 - h].astype(np.float64), axis=-1)
        assert (np.abs(got['dist'][0, 1 - h] - want) <= 1e-6 + 1e-5 * want).all()
    both = run(np.zeros((1, 2, 778, 3), np.float32), faces)
    assert all(np.isfinite(x).all() for x in both.values()) and (both['count'] == 0).all() and (both['dist'] == 0).all()


def test_determinism_and_shapes():
    from pdfnet_amd import functional as F
    verts, faces, _ = template_case()
    v, f = torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda()
    first, second = F.mesh_penetration(v, f, return_fields=True), F.mesh_penetration(v, f, return_fields=True)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert first[0].dtype == torch.int32 and first[0].shape == first[1].shape == first[2].shape == (3, 2)
    assert first[3].shape == first[4].shape == (3, 2, 778)
    three = F.mesh_penetration(v, f)
    assert len(three) == 3 and all(torch.equal(x, y) for x, y in zip(three, first))
    lead = F.mesh_penetration(torch.stack((v, v.flip(0))).reshape(2, 3, 1, 2, 778, 3), f, return_fields=True)
    assert lead[0].shape == (2, 3, 1, 2) and lead[3].shape == (2, 3, 1, 2, 778)
    for x, y in zip(lead, first):
        assert torch.equal(x[0, :, 0], y) and torch.equal(x[1, :, 0], y.flip(0))


# ---- interaction_sums ------------------------------------------------------------------------------
def test_interaction_sums_on_a_hand_made_tuple():
    """B = 4; prediction and ground truth are template poses with different shifts (all from SHIFTS, so the float64 side is the cached one),
    sample 2 has valid = (1, 0).  Joints: random, with the roots set so that MRRPE is known."""
    from pdfnet_amd.trains.base_trainer import interaction_sums
    _, faces, ref = template_case()
    pred_s, gt_s = (1, 2, 1, 0), (2, 0, 0, 1)
    valid = np.array([[1, 1], [1, 1], [1, 0], [1, 1]], np.float32)
    vp, vg = hands([SHIFTS[i] for i in pred_s]), hands([SHIFTS[i] for i in gt_s])
    rng = np.random.default_rng(3)
    jp, jg = rng.uniform(-0.1, 0.1, (4, 2, 21, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, (4, 2, 21, 3)).astype(np.float32)
    jpo, jgo = rng.uniform(-0.1, 0.1, (4, 2, 21, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, (4, 2, 21, 3)).astype(np.float32)
    z = np.zeros((4, 2, 2), np.float32)
    tup = tuple(torch.from_numpy(a).cuda() for a in (vp, jp, vg, jg, z, vp, jpo, vg, jgo))
    got = interaction_sums(tup, {'valid': torch.from_numpy(valid).cuda()}, torch.from_numpy(faces).cuda())
    assert got.dtype == torch.float64 and got.shape == (12,) and got.is_cuda
    got = got.cpu().numpy()
    want = np.zeros(12)
    assert well_conditioned(ref)
    for b in range(4):
        if not (valid[b] == 1).all():
            continue
        rp, rg = (jp[b].astype(np.float64) - jpo[b])[:, 0], (jg[b].astype(np.float64) - jgo[b])[:, 0]
        want[0] += 1
        want[1] += np.linalg.norm((rp[1] - rp[0]) - (rg[1] - rg[0]))
        for o, s in ((2, pred_s[b]), (7, gt_s[b])):
            c = ref['count'][s]
            want[o:o + 5] += (c[0] / 778, c[1] / 778, ref['depth'][s].max(), float(c.sum() > 0), ref['gap'][s].min())
    print("  got  %s\n  want %s" % (got.tolist(), want.tolist()))
    assert got[0] == 3.0
    assert abs(got[1] - want[1]) <= 1e-6 * want[1]
    for i in (2, 3, 5, 7, 8, 10):                                 # count-based: the same integers, summed in another order
        assert abs(got[i] - want[i]) <= 1e-12, (i, got[i], want[i])
    for i in (4, 6, 9, 11):
        assert abs(got[i] - want[i]) <= 3 * 1e-6 + 1e-5 * want[i], (i, got[i], want[i])
    # the invalid sample contributes to nothing: garbage in it changes no sum
    vp2, jp2 = vp.copy(), jp.copy()
    vp2[2], jp2[2] = 7.0, -3.0
    tup2 = tuple(torch.from_numpy(a).cuda() for a in (vp2, jp2, vg, jg, z, vp2, jpo, vg, jgo))
    again = interaction_sums(tup2, {'valid': torch.from_numpy(valid).cuda()}, torch.from_numpy(faces).cuda()).cpu().numpy()
    assert np.array_equal(again, got)


# ---- Trainer.evaluation(interaction=True) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluation_runs():
    """The set-up of tests/test_eval_aligned_gpu.py::evaluation_runs: R = 128, B = 3, two batches, random-init model."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer, interaction_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 3
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev))
    loader = [synthetic_train_batch(B, R, seed=s, consts=consts) for s in (21, 22)]
    runs = {'plain': tr.evaluation(loader), 'off': tr.evaluation(loader, interaction=False), 'on': tr.evaluation(loader, interaction=True),
            'aligned': tr.evaluation(loader, aligned=True), 'both': tr.evaluation(loader, aligned=True, interaction=True)}
    assert m.training
    sums = torch.zeros(12, dtype=torch.float64, device=dev)
    tr.model_with_loss.eval()
    with torch.no_grad():
        for b in loader:
            bd = tree_to({k: v for k, v in b.items() if torch.is_tensor(v)}, dev)
            sums += interaction_sums(tr.model_with_loss(bd, 'test', None), bd, tr.model_with_loss.loss.faces_pair)
    tr.model_with_loss.train()
    return runs, sums.cpu()


def test_evaluation_interaction_keys():
    """The random model's meshes and the synthetic ground-truth clouds are no well-conditioned surfaces: this pins the plumbing (the flag off
    changes nothing, the flag on changes no other key with `aligned` on or off, the new keys are finish_interaction of the summed
    interaction_sums); the cases above pin the arithmetic."""
    from pdfnet_amd.trains.base_trainer import INTERACTION_KEYS, finish_interaction
    runs, sums = evaluation_runs()
    plain = runs['plain']
    assert plain['samples'] == 6 and runs['off'] == plain and list(runs['off']) == list(plain)
    for base, on in ((plain, runs['on']), (runs['aligned'], runs['both'])):
        assert list(on) == list(base) + list(INTERACTION_KEYS)
        for k, v in base.items():
            assert on[k] == v, k
    on = runs['on']
    want = finish_interaction(sums)
    assert list(want) == list(INTERACTION_KEYS) and want['interaction_samples'] > 0
    for k in INTERACTION_KEYS:
        print("  %-20s got %.9g want %.9g" % (k, on[k], want[k]))
        assert np.isfinite(on[k]) and abs(on[k] - want[k]) <= 1e-12, (k, on[k], want[k])
        assert runs['both'][k] == on[k], k
    for k in ('pen_ratio_left', 'pen_ratio_right', 'pen_ratio', 'pen_rate', 'gt_pen_ratio', 'gt_pen_rate'):
        assert 0.0 <= on[k] <= 1.0, (k, on[k])


def test_write_interaction_scores_appends_its_own_block(tmp_path):
    from pdfnet_amd.trains.base_trainer import INTERACTION_KEYS, write_aligned_scores, write_h2o_scores, write_interaction_scores
    both = evaluation_runs()[0]['both']
    path = str(tmp_path / 'H2O-val.txt')
    write_h2o_scores(path, both)
    write_aligned_scores(path, both)
    before = open(path).read()
    write_interaction_scores(path, both)
    text = open(path).read()
    assert text.startswith(before)
    assert text[len(before):].splitlines() == ['eval interaction '] + ['%s: %.2f' % (k, both[k]) for k in INTERACTION_KEYS]
