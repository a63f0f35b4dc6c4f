"""The hand renderer on the GPU (csrc/render.hip pdf_render_hands / pdf_render_compare, F.render_hands, F.render_compare, HandRenderer,
Trainer.evaluation(rendered=True)) against a float64 numpy restatement of the arithmetic contract in the header comment of csrc/render.hip:
a brute force over pixels x faces (`ref_render`; a face is tried on the pixels of its bounding box grown by a pixel).  Shading is pinned to this restatement of pytorch3d's documented HardPhongShader defaults,
not to a pytorch3d run.

Inputs: the template hands of tests/test_eval_interaction_gpu.py (left hand shifted, right hand at the origin) moved to (0, 0, 0.5) m, under
K = [[f, 0, W/2 + 0.3], [0, 0.98 f, H/2 - 0.2], [0, 0, 1]]:  A 64 x 64, f = 150, shift (0.06, 0.01, 0);  B 72 x 88, f = 170, (0.02, 0, 0.03),
interpenetrating, no multiple of the tile;  C 72 x 88, f = 170, (0.25, 0, 0), the left hand wholly off-screen.  Each alone, and all three in one
B = 3 call at 72 x 88 with per-sample K.

`face` is discontinuous at edges and at depth ties.  A pixel is AMBIGUOUS when, on the float64 side, some non-skipped face has it within 1e-3 px
of one of its edges (every signed edge distance >= -1e-3 px and the smallest < 1e-3 px: within that band rounding decides the coverage), or the
two nearest covering depths differ by less than 1e-6 relative.  Ambiguous pixels are left out of the comparisons; tests/test_render_cpu.py
asserts that they are at most 2 % of the covered pixels of each case.

Bars on the other pixels: face and background exact; depth DEPTH_BAR relative, bary BARY_BAR absolute, rgb (0 .. 255 colour scale) RGB_BAR
absolute.  They started at 1e-5, 2e-4 and 3e-3 (an fp32 numpy run of the same formulas is within 1.8e-6, 4.3e-5 and 6.8e-4 of float64) and are
four times the kernel's measured maxima where that is tighter; the measured maxima are in the comment at the constants."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_eval_interaction_gpu import hands, template
from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

# measured on an MI355X over every call to `check` below: depth 5.45e-7 relative, bary 2.63e-5, rgb 9.54e-4 (A, B, C in one call; B alone for
# rgb).  Four times that: 2.2e-6 and 1.1e-4, tighter than the starting bars; 3.8e-3 for rgb is not, so rgb keeps 3e-3.
DEPTH_BAR, BARY_BAR, RGB_BAR = 2.2e-6, 1.1e-4, 3e-3
EDGE_MARGIN, DEPTH_MARGIN = 1e-3, 1e-6
Z_NEAR = 0.01
CASES = {'A': ((64, 64), 150.0, (0.06, 0.01, 0.0)), 'B': ((72, 88), 170.0, (0.02, 0.0, 0.03)), 'C': ((72, 88), 170.0, (0.25, 0.0, 0.0))}
LEFT_COLOUR, RIGHT_COLOUR = (92.0, 73.0, 179.0), (150.0, 161.0, 105.0)


# ---- float64 restatement -----------------------------------------------------------------------
def ref_vertex_normals(v, faces):
    """v [2, n, 3], faces [2, Fc, 3] -> [2, n, 3]: sum of (p1 - p0) x (p2 - p0) over the faces at a vertex (each once), / max(|.|, 1e-6)."""
    out = np.zeros_like(v)
    for h in range(2):
        f = faces[h]
        fn = np.cross(v[h, f[:, 1]] - v[h, f[:, 0]], v[h, f[:, 2]] - v[h, f[:, 0]])
        for k, tri in enumerate(f):
            for i in set(tri.tolist()):
                out[h, i] += fn[k]
    return out / np.maximum(np.linalg.norm(out, axis=-1, keepdims=True), 1e-6)


def ref_render_sample(v, faces, K, H, W, valid=(1, 1), colour=None, ambient_only=False, z_near=Z_NEAR, dt=np.float64):
    """One sample.  v [2, n, 3], faces [2, Fc, 3], K [3, 3] -> dict: face [H, W] int, depth [H, W], bary, rgb [H, W, 3] (rgb with colour
    [2, n, 3]), ambiguous [H, W] bool."""
    v, K = v.astype(dt), K.astype(dt)
    Fc = faces.shape[1]
    idx = np.concatenate((faces[0], faces[1])).astype(np.int64)              # [2Fc, 3]
    hand = np.repeat(np.arange(2), Fc)
    P = v[hand[:, None], idx]                                                 # [2Fc, 3, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        Z = P[..., 2]
        x, y, iz = K[0, 0] * P[..., 0] / Z + K[0, 2], K[1, 1] * P[..., 1] / Z + K[1, 2], 1 / Z
        a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    keep = (np.asarray(valid)[hand] != 0) & (Z >= z_near).all(1) & (a2 != 0) & np.isfinite(a2)
    ids = np.nonzero(keep)[0]
    s = np.where(a2 > 0, 1.0, -1.0).astype(dt)
    ox, oy, dx, dy = (np.zeros((2 * Fc, 3), dt) for _ in range(4))
    for k in range(3):                                                        # the edge opposite vertex k, from the lower to the higher index
        a, b = (k + 1) % 3, (k + 2) % 3
        fwd = idx[:, a] < idx[:, b]
        o, t = np.where(fwd, a, b), np.where(fwd, b, a)
        r = np.arange(2 * Fc)
        ox[:, k], oy[:, k] = x[r, o], y[r, o]
        sg = np.where(fwd, s, -s)
        dx[:, k], dy[:, k] = sg * (x[r, t] - x[r, o]), sg * (y[r, t] - y[r, o])
    # every (face, pixel) pair that can matter: the pixels whose centre lies in the face's bounding box grown by one pixel (outside it the
    # face neither covers the centre nor has an edge within EDGE_MARGIN of it)
    n_px = H * W
    j0, j1 = np.clip(np.floor(x[ids].min(1) - 1.5), 0, W).astype(np.int64), np.clip(np.ceil(x[ids].max(1) + 0.5), 0, W).astype(np.int64)
    i0, i1 = np.clip(np.floor(y[ids].min(1) - 1.5), 0, H).astype(np.int64), np.clip(np.ceil(y[ids].max(1) + 0.5), 0, H).astype(np.int64)
    nx, cnt = j1 - j0, (j1 - j0) * (i1 - i0)
    k = np.repeat(np.arange(len(ids)), cnt)                                   # pair -> position in ids
    local = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    pj, pi, g = j0[k] + local % np.maximum(nx[k], 1), i0[k] + local // np.maximum(nx[k], 1), ids[k]
    px, py = (pj + 0.5).astype(dt), (pi + 0.5).astype(dt)
    w = dx[g] * (py[:, None] - oy[g]) - dy[g] * (px[:, None] - ox[g])         # [pairs, 3]
    sd = (w / np.hypot(dx[g], dy[g])).min(-1)
    near = np.zeros(n_px, bool)
    near[(pi * W + pj)[(sd >= -EDGE_MARGIN) & (sd < EDGE_MARGIN)]] = True
    ws = w.sum(-1)
    cover = (w >= 0).all(-1) & (ws > 0)
    pix, gc = (pi * W + pj)[cover], g[cover]
    d = ws[cover] / (w[cover] * iz[gc]).sum(-1)
    order = np.lexsort((gc, d, pix))                                          # per pixel: nearest first, equal depths by face index
    pix, gc, d = pix[order], gc[order], d[order]
    first = np.ones(len(pix), bool)
    first[1:] = pix[1:] != pix[:-1]
    best, second = np.full(n_px, np.inf), np.full(n_px, np.inf)
    bid = np.full(n_px, -1, np.int64)
    bid[pix[first]], best[pix[first]] = gc[first], d[first]
    runner = np.zeros(len(pix), bool)
    runner[1:] = first[:-1] & ~first[1:]
    second[pix[runner]] = d[runner]
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    px, py = (jj.reshape(-1) + 0.5).astype(dt), (ii.reshape(-1) + 0.5).astype(dt)
    hit = bid >= 0
    with np.errstate(invalid='ignore'):
        tie = hit & np.isfinite(second) & (second - best < DEPTH_MARGIN * best)
    out = {'face': bid.reshape(H, W), 'depth': np.where(hit, best, 0.0).reshape(H, W), 'ambiguous': (near | tie).reshape(H, W),
           'ties': int(tie.sum())}
    g = np.where(hit, bid, 0)
    w = dx[g] * (py[:, None] - oy[g]) - dy[g] * (px[:, None] - ox[g])         # [P, 3]
    q = w * iz[g]
    with np.errstate(divide='ignore', invalid='ignore'):
        bary = np.where(hit[:, None], q / q.sum(-1, keepdims=True), 0.0)
    out['bary'] = bary.reshape(H, W, 3)
    if colour is not None:
        col = colour.astype(dt)[hand[g][:, None], idx[g]]                     # [P, 3 corners, 3]
        c = (bary[..., None] * col).sum(1)
        if not ambient_only:
            nrm = ref_vertex_normals(v, faces)[hand[g][:, None], idx[g]]
            unit = lambda a: a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-6)
            p, n = (bary[..., None] * P[g]).sum(1), unit((bary[..., None] * nrm).sum(1))
            l, view = unit(np.array([0.0, 0.0, -1.0]) - p), unit(-p)
            ndl = (n * l).sum(-1, keepdims=True)
            r = 2 * ndl * n - l
            spec = np.maximum((r * view).sum(-1, keepdims=True), 0.0) ** 64 * (ndl > 0)
            c = (0.5 + 0.3 * np.maximum(ndl, 0.0)) * c + 0.2 * spec
        out['rgb'] = np.where(hit[:, None], c, 0.0).reshape(H, W, 3)
    return out


def ref_render(verts, faces, K, size, valid=None, colour=None, ambient_only=False, z_near=Z_NEAR, dt=np.float64):
    """verts [B, 2, n, 3], K [B, 3, 3] -> dict of stacked per-sample outputs of `ref_render_sample`."""
    rows = [ref_render_sample(verts[b], faces, K[b], size[0], size[1], (1, 1) if valid is None else valid[b],
                              colour if colour is None or colour.ndim == 3 else colour[b], ambient_only, z_near, dt) for b in range(verts.shape[0])]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---- inputs --------------------------------------------------------------------------------------
def camera(f, H, W):
    return np.array([[f, 0, W / 2 + 0.3], [0, 0.98 * f, H / 2 - 0.2], [0, 0, 1]], np.float32)


def colours():
    """The reference's two hand colours per vertex, with a gradient along the vertex index so that the interpolation shows: [2, 778, 3]."""
    ramp = np.linspace(-20.0, 20.0, 778, dtype=np.float32)[:, None]
    return np.stack((np.asarray(LEFT_COLOUR, np.float32) + ramp, np.asarray(RIGHT_COLOUR, np.float32) - ramp))


def case_inputs(name, size=None):
    """-> (verts [1, 2, 778, 3] float32, K [1, 3, 3] float32, (H, W))."""
    (H, W), f, shift = CASES[name]
    H, W = size or (H, W)
    return hands([shift]) + np.array([0, 0, 0.5], np.float32), camera(f, H, W)[None], (H, W)


@functools.lru_cache(maxsize=None)
def case_ref(name, size=None):
    """The float64 side of one case at its own size (or at `size`), shaded with `colours()`: computed once."""
    verts, K, size = case_inputs(name, size)
    return ref_render(verts, template()[2], K, size, colour=colours())


def ambiguous_share(ref):
    covered = ref['face'] >= 0
    return (ref['ambiguous'] & covered).sum() / max(covered.sum(), 1), int(covered.sum())


def run(verts, faces, K, size, valid=None, colour=None, ambient_only=False, bary=True, z_near=Z_NEAR):
    from pdfnet_amd import functional as F
    cu = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = F.render_hands(cu(verts), cu(faces), cu(K), size, valid=cu(valid), colour=cu(colour), ambient_only=ambient_only, z_near=z_near,
                         return_bary=bary)
    names = ['face', 'depth'] + (['bary'] if bary else []) + (['rgb'] if colour is not None else [])
    assert len(out) == len(names)
    return {k: v.cpu().numpy() for k, v in zip(names, out)}


def check(got, ref, label=""):
    """The bars of the module docstring on the unambiguous pixels; prints every figure before it asserts.  -> the measured maxima."""
    ok = ~ref['ambiguous']
    hit = ok & (ref['face'] >= 0)
    wrong = int((got['face'] != ref['face'])[ok].sum())
    ed = np.abs(got['depth'].astype(np.float64) - ref['depth'])[hit] / ref['depth'][hit]
    fig = {'wrong_face': wrong, 'depth_rel': float(ed.max()) if hit.any() else 0.0}
    for k in ('bary', 'rgb'):
        if k in got:
            fig[k] = float(np.abs(got[k].astype(np.float64) - ref[k])[ok].max())
    print("  %s: %d pixels, %d covered, %d ambiguous, figures %s" % (label, ok.size, (ref['face'] >= 0).sum(), (~ok).sum(), fig))
    assert got['face'].dtype == np.int32 and got['depth'].dtype == np.float32
    assert wrong == 0, wrong
    assert (got['depth'][ok & (ref['face'] < 0)] == 0).all()
    assert fig['depth_rel'] <= DEPTH_BAR, fig
    assert fig.get('bary', 0.0) <= BARY_BAR and fig.get('rgb', 0.0) <= RGB_BAR, fig
    for k in ('bary', 'rgb'):
        if k in got:
            assert (got[k][got['face'] < 0] == 0).all()
    return fig


# ---- pdf_render_hands on the template hands --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_alone(name):
    verts, K, size = case_inputs(name)
    ref = case_ref(name)
    share, covered = ambiguous_share(ref)
    assert share <= 0.02 and covered > 1000, (share, covered)
    got = run(verts, template()[2], K, size, colour=colours())
    check(got, {k: v for k, v in ref.items()}, label="case %s %s" % (name, size))
    Fc = template()[2].shape[1]
    if name == 'C':                                                   # the left hand is off-screen: nothing of it anywhere
        assert not ((got['face'] >= 0) & (got['face'] < Fc)).any() and (got['face'] >= Fc).sum() > 1000
    else:
        assert ((got['face'] >= 0) & (got['face'] < Fc)).sum() > 300 and (got['face'] >= Fc).sum() > 300


def test_three_cases_in_one_call_with_per_sample_cameras():
    """B = 3 at 72 x 88 (A re-rendered at that size): 5 x 6 tiles of which the last row and column overhang, a camera per sample."""
    size = (72, 88)
    parts = [case_inputs(n, size) for n in 'ABC']
    verts, K = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    refs = [case_ref(n, size if n == 'A' else None) for n in 'ABC']
    ref = {k: np.concatenate([r[k] for r in refs]) for k in ('face', 'depth', 'bary', 'rgb', 'ambiguous')}
    got = run(verts, template()[2], K, size, colour=colours())
    assert got['face'].shape == (3, 72, 88) and got['bary'].shape == got['rgb'].shape == (3, 72, 88, 3)
    check(got, ref, label="A, B, C in one call")
    for b, n in enumerate('BC'):                                       # a sample does not depend on its neighbours: bit-equal to the call alone
        alone = run(parts[b + 1][0], template()[2], parts[b + 1][1], size, colour=colours())
        for k in got:
            assert np.array_equal(got[k][b + 1], alone[k][0]), (n, k)


def test_optional_outputs_determinism_and_valid():
    """Two calls are bit-identical; leaving out bary and rgb leaves face / depth unchanged; valid = 0 removes exactly that hand's faces; a
    per-sample colour tensor gives what the shared one gives."""
    verts, K, size = case_inputs('B')
    faces = template()[2]
    Fc = faces.shape[1]
    first, again = run(verts, faces, K, size, colour=colours()), run(verts, faces, K, size, colour=colours())
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    plain = run(verts, faces, K, size, bary=False)
    assert sorted(plain) == ['depth', 'face'] and np.array_equal(plain['face'], first['face']) and np.array_equal(plain['depth'], first['depth'])
    per_sample = run(verts, faces, K, size, colour=colours()[None])
    assert np.array_equal(per_sample['rgb'], first['rgb'])
    for h in range(2):
        valid = np.ones((1, 2), np.float32)
        valid[0, h] = 0
        got = run(verts, faces, K, size, valid=valid, colour=colours())
        ref = ref_render(verts, faces, K, size, valid=valid, colour=colours())
        check(got, ref, label="valid[%d] = 0" % h)
        gone = (got['face'] >= h * Fc) & (got['face'] < (h + 1) * Fc)
        assert not gone.any() and (got['face'] >= 0).sum() > 500
        # what the other hand showed before, it still shows, with the same bits
        same = (first['face'] >= (1 - h) * Fc) & (first['face'] < (2 - h) * Fc)
        assert np.array_equal(got['face'][same], first['face'][same]) and np.array_equal(got['depth'][same], first['depth'][same])
    none = run(verts, faces, K, size, valid=np.zeros((1, 2), np.float32), colour=colours())
    assert (none['face'] == -1).all() and (none['depth'] == 0).all() and (none['rgb'] == 0).all() and (none['bary'] == 0).all()


def test_ambient_only_returns_the_interpolated_colour():
    verts, K, size = case_inputs('A')
    faces = template()[2]
    ref = ref_render(verts, faces, K, size, colour=colours(), ambient_only=True)
    got = run(verts, faces, K, size, colour=colours(), ambient_only=True)
    check(got, ref, label="ambient only")
    flat = np.stack((np.tile(np.array([0, 0, 255], np.float32), (778, 1)), np.tile(np.array([0, 255, 0], np.float32), (778, 1))))
    got = run(verts, faces, K, size, colour=flat, ambient_only=True)
    Fc = faces.shape[1]
    left, right = (got['face'] >= 0) & (got['face'] < Fc), got['face'] >= Fc
    assert np.abs(got['rgb'][left] - [0, 0, 255]).max() <= 255 * BARY_BAR and np.abs(got['rgb'][right] - [0, 255, 0]).max() <= 255 * BARY_BAR


# ---- exact small cases: f = 1, Z = 1, coordinates that fp32 holds exactly ---------------------------
EYE = np.eye(3, dtype=np.float32)[None]


def small(points, tris, size, right=None, **kw):
    """points [(x, y) or (x, y, z)] and triangles of the LEFT hand (the right hand: `right` = (points, tris), else one zero-area face), under
    K = identity, so that a vertex at Z = 1 lands on the pixel coordinates (x, y).  -> (got, ref), compared on EVERY pixel."""
    def pad(pts, n):
        p = np.array([(q[0], q[1], q[2] if len(q) > 2 else 1.0) for q in pts], np.float32)
        return np.concatenate((p, np.tile(p[:1], (n - len(p), 1))))
    rp, rt = right if right is not None else (points[:1], [(0, 0, 0)])
    n, Fc = max(len(points), len(rp)), max(len(tris), len(rt))
    padt = lambda t: np.array(list(t) + [(0, 0, 0)] * (Fc - len(t)), np.int64)
    verts = np.stack((pad(points, n), pad(rp, n)))[None]
    faces = np.stack((padt(tris), padt(rt)))
    colour = np.stack((np.linspace(10, 200, n * 3, dtype=np.float32).reshape(n, 3), np.full((n, 3), 50, np.float32)))
    got = {k: v[0] for k, v in run(verts, faces, EYE, size, colour=colour, **kw).items()}
    ref = {k: v[0] for k, v in ref_render(verts, faces, EYE, size, colour=colour, **kw).items()}
    assert np.array_equal(got['face'], ref['face']), (got['face'], ref['face'])
    assert np.abs(got['depth'] - ref['depth']).max() <= 1e-6 and np.abs(got['bary'] - ref['bary']).max() <= 1e-6
    assert np.abs(got['rgb'] - ref['rgb']).max() <= RGB_BAR
    return got, ref, Fc


@pytest.mark.parametrize("size,corner,side", [((8, 8), (1, 1), 6), ((16, 24), (2, 3), 12), ((16, 24), (9, 1), 14)])
def test_quad_has_no_hole_along_its_diagonal(size, corner, side):
    """Two triangles whose shared diagonal passes exactly through pixel centres: every centre inside the square is covered, nothing else is,
    the diagonal's pixels go to the lower face, and the depth is exactly 1 everywhere."""
    (x, y), H, W = corner, size[0], size[1]
    for tris in ([(0, 1, 2), (0, 2, 3)], [(2, 1, 0), (0, 2, 3)], [(0, 2, 3), (1, 2, 0)]):       # consistent and inconsistent windings
        got, _, _ = small([(x, y), (x + side, y), (x + side, y + side), (x, y + side)], tris, size)
        want = np.zeros(size, bool)
        want[y:min(y + side, H), x:min(x + side, W)] = True          # centres (j + 0.5, i + 0.5) inside [x, x + side] x [y, y + side]
        assert np.array_equal(got['face'] >= 0, want)
        assert (got['depth'][want] == 1.0).all()
        k = np.arange(min(side, H - y, W - x))
        assert (got['face'][y + k, x + k] == 0).all()                # on the diagonal both cover at equal depth: the lower index
        assert set(np.unique(got['face'][want]).tolist()) == {0, 1}


def test_identical_coplanar_triangles_lower_index_wins():
    tri = [(1, 1), (7, 2), (2, 7)]
    got, _, Fc = small(tri, [(0, 1, 2), (0, 1, 2), (1, 2, 0)], (8, 8), right=(tri, [(0, 1, 2)]))
    assert (got['face'] >= 0).sum() > 10 and set(np.unique(got['face']).tolist()) == {-1, 0}
    got, _, Fc = small(tri, [(0, 0, 0), (0, 1, 2)], (8, 8), right=(tri, [(0, 1, 2)]))           # left face 1 against right face Fc + 0
    assert set(np.unique(got['face']).tolist()) == {-1, 1}


def test_near_plane_and_zero_area_draw_nothing():
    got, _, _ = small([(1, 1, 1.0), (7, 2, 1.0), (2, 7, 0.005)], [(0, 1, 2)], (8, 8))           # one vertex nearer than z_near = 0.01
    assert (got['face'] == -1).all() and (got['depth'] == 0).all()
    got, _, _ = small([(1, 1, 1.0), (7, 2, 1.0), (2, 7, 0.015625)], [(0, 1, 2)], (8, 8))        # 1/64 m: drawn (x, y are X / Z, Y / Z)
    got, _, _ = small([(1, 1, 1.0), (7, 2, 1.0), (2, 7, 1.0)], [(0, 1, 2)], (8, 8), z_near=2.0)
    assert (got['face'] == -1).all()
    got, _, _ = small([(1, 1), (4, 4), (7, 7), (1, 1)], [(0, 1, 2), (0, 3, 1), (2, 2, 2)], (8, 8))   # collinear; two equal corners; a point
    assert (got['face'] == -1).all() and (got['rgb'] == 0).all()


@pytest.mark.parametrize("size", [(8, 8), (16, 24)])
def test_triangle_hanging_off_two_borders(size):
    H, W = size
    got, ref, _ = small([(W - 5, H - 6), (W + 9, H - 2), (W - 3, H + 7)], [(0, 1, 2)], size)
    assert 5 < (got['face'] == 0).sum() < 30 and got['face'][H - 1, W - 1] == 0
    got, _, _ = small([(-30, -20), (5, -2), (-3, 6)], [(0, 1, 2)], size)                        # the top left corner
    assert got['face'][0, 0] == 0 and (got['face'] == 0).sum() < 20


def test_tilted_triangle_depth_and_barycentrics():
    """Perspective-correct: a triangle tilted in depth, fewer vertices than a wave, one face per hand; the right hand's nearer face wins."""
    left = [(1 * 2.0, 1 * 2.0, 2.0), (14 * 4.0, 2 * 4.0, 4.0), (3 * 1.0, 13 * 1.0, 1.0)]      # (X, Y, Z) -> pixels (1, 1), (14, 2), (3, 13)
    right = [(2 * 0.5, 2 * 0.5, 0.5), (9 * 0.5, 3 * 0.5, 0.5), (4 * 0.5, 9 * 0.5, 0.5)]
    got, ref, Fc = small(left, [(0, 1, 2)], (16, 24), right=(right, [(0, 1, 2)]))
    assert (got['face'] == Fc).sum() > 10 and (got['face'] == 0).sum() > 20
    assert (got['depth'][got['face'] == Fc] == 0.5).all()
    lit = got['face'] == 0
    assert got['depth'][lit].min() >= 1.0 and got['depth'][lit].max() <= 4.0 and np.abs(got['bary'][lit].sum(-1) - 1).max() <= 1e-6


def test_refusals():
    from pdfnet_amd import functional as F
    c, vp = F._L().cdll, ctypes.c_void_p
    x = torch.zeros(1, 2, 1025, 3, device='cuda')
    f = torch.zeros(2, 2049, 3, dtype=torch.int64, device='cuda')
    k = torch.eye(3, device='cuda')[None]
    o = torch.zeros(64, device='cuda')
    oi = torch.zeros(64, dtype=torch.int32, device='cuda')
    P = lambda t: vp(t.data_ptr())

    def call(n=4, Fc=4, M=1, H=4, W=4, z=0.01, rgb=None, colour=None, table=None):
        return c.pdf_render_hands(P(x), P(f), P(k), None, colour, 0, table, 1, n, Fc, M, H, W, ctypes.c_float(z), 0, P(o), P(oi), P(o), None, rgb, None)
    for bad in (dict(n=1025), dict(n=0), dict(Fc=2049), dict(Fc=0), dict(M=33), dict(M=0), dict(H=2049), dict(W=0), dict(z=0.0),
                dict(rgb=P(o)), dict(rgb=P(o), colour=P(o))):
        assert call(**bad) == -1, bad
    assert (oi == 0).all() and (o == 0).all()                     # nothing was launched
    for call in (lambda: F.render_hands(x, f[:, :4], k, (4, 4)), lambda: F.render_hands(x[:, :, :4], f, k, (4, 4)),
                 lambda: F.render_hands(x[:, :1, :4], f[:, :4], k, (4, 4)), lambda: F.render_hands(x[:, :, :4], f[:, :4], k[0], (4, 4)),
                 lambda: F.render_hands(x[:, :, :4], f[:, :4], k, (4, 2049)), lambda: F.render_hands(x[:, :, :4], f[:, :4], k, 4),
                 lambda: F.render_hands(x[:, :, :4], f[:, :4], k, (4, 4), valid=o[:3].reshape(1, 3)),
                 lambda: F.render_hands(x[:, :, :4], f[:, :4], k, (4, 4), colour=o[:9].reshape(1, 3, 3)),
                 lambda: F.render_hands(x[:, :, :4], f[:, :4], k, (4, 4), colour=o[:24].reshape(2, 4, 3), table=oi[:10].reshape(2, 5, 1)),
                 lambda: F.render_hands(x[:, :, :4], f[:, :4], k, (4, 4), z_near=0.0),
                 lambda: F.render_compare(oi[:16].reshape(1, 4, 4), oi[:16].reshape(1, 4, 4), o[:16].reshape(1, 4, 4), 2049),
                 lambda: F.render_compare(oi[:16].reshape(1, 4, 4), oi[:16].reshape(4, 4), o[:16].reshape(1, 4, 4), 4),
                 lambda: F.render_compare(o[:16].reshape(1, 4, 4), oi[:16].reshape(1, 4, 4), o[:16].reshape(1, 4, 4), 4)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        F.render_hands(x[:, :, :4].cpu(), f[:, :4].cpu(), k.cpu(), (4, 4))
    lead = F.render_hands(torch.rand(2, 3, 2, 4, 3, device='cuda'), f[:, :4], k.expand(2, 3, 3, 3), (5, 7), return_bary=True)
    assert lead[0].shape == lead[1].shape == (2, 3, 5, 7) and lead[2].shape == (2, 3, 5, 7, 3)


# ---- pdf_render_compare -----------------------------------------------------------------------------
def ref_compare(fp, fg, dp, sensor, Fc, skip):
    """float64 maps of one sample, `skip` = pixels left out -> ((inter, union) x 2, residual sum, residual count)."""
    iou = []
    for h in range(2):
        a, b = (fp >= h * Fc) & (fp < (h + 1) * Fc) & ~skip, (fg >= h * Fc) & (fg < (h + 1) * Fc) & ~skip
        iou.append((int((a & b).sum()), int((a | b).sum())))
    m = (fp >= 0) & (sensor > 0) & ~skip
    return iou, float(np.abs(dp - sensor)[m].sum()), int(m.sum())


def test_render_compare_against_itself_and_against_another_pose():
    from pdfnet_amd import functional as F
    size, faces = (72, 88), template()[2]
    Fc = faces.shape[1]
    (va, Ka, _), (vb, _, _) = case_inputs('A', size), case_inputs('B', size)
    pred, gt = np.concatenate((va, va)), np.concatenate((va, vb))            # sample 0: A against itself; sample 1: A against B's meshes
    K = np.concatenate((Ka, Ka))
    rp = case_ref('A', size)
    rg = ref_render(vb, faces, Ka, size)
    rng = np.random.default_rng(11)
    own = np.where(rp['depth'][0] > 0, rp['depth'][0] + 0.002, 0.0).astype(np.float32)           # sample 0: its own surface + 2 mm
    other = (rg['depth'][0] + rng.uniform(-0.01, 0.01, size)).astype(np.float32) * (rng.uniform(0, 1, size) > 0.3)      # 30 % without a measurement
    other[:8] = -1.0
    sensor = np.stack((own, other))
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fp, dp = F.render_hands(cu(pred), cu(faces), cu(K), size)
    fg, _ = F.render_hands(cu(gt), cu(faces), cu(K), size)
    iou, res = F.render_compare(fp, fg, dp, Fc, cu(sensor))
    assert iou.dtype == torch.int32 and iou.shape == (2, 2, 2) and res.shape == (2, 2)
    again = F.render_compare(fp, fg, dp, Fc, cu(sensor))
    assert torch.equal(again[0], iou) and torch.equal(again[1], res)
    iou, res = iou.cpu().numpy(), res.cpu().numpy().astype(np.float64)
    print("  iou %s, residual %s" % (iou.tolist(), res.tolist()))
    assert (iou[0, :, 0] == iou[0, :, 1]).all() and (iou[0, :, 0] > 300).all()                   # against itself: IoU exactly 1
    zs = pred[..., 2]
    for b, ref_gt in enumerate((rp, rg)):
        amb = rp['ambiguous'][0] | ref_gt['ambiguous'][0]
        args = (rp['face'][0], ref_gt['face'][0], rp['depth'][0], sensor[b].astype(np.float64), Fc)
        want_iou, (_, want_sum, want_n) = ref_compare(*args, amb)[0], ref_compare(*args, rp['ambiguous'][0])      # (the residual reads one render)
        for h in range(2):
            for k in range(2):
                assert 0 <= iou[b, h, k] - want_iou[h][k] <= amb.sum(), (b, h, k, iou[b, h, k], want_iou[h][k], amb.sum())
        # an ambiguous pixel of the prediction's render adds at most the farthest a surface of this scene can be from its measurement
        m = rp['ambiguous'][0] & (sensor[b] > 0)
        slack = np.maximum(np.abs(zs.max() - sensor[b]), np.abs(zs.min() - sensor[b]))[m].sum()
        assert want_n <= res[b, 1] <= want_n + m.sum(), (res[b, 1], want_n, m.sum())
        assert want_sum * (1 - 1e-5) <= res[b, 0] <= want_sum * (1 + 1e-5) + slack, (res[b, 0], want_sum, slack)
        assert want_n > 500
    assert abs(res[0, 0] / res[0, 1] - 0.002) < 1e-5                                            # sample 0's sensor is its own surface + 2 mm
    none = F.render_compare(fp, fg, dp, Fc)
    assert torch.equal(none[0].cpu(), torch.from_numpy(iou)) and (none[1] == 0).all()


# ---- rendered_sums and Trainer.evaluation(rendered=True) --------------------------------------------
def test_rendered_sums_on_a_hand_made_tuple():
    """B = 3: A against itself, A against B's meshes, and A against itself with the left hand marked invalid; the sensor is the prediction's own
    float64 depth + 2 mm, so the residual is known."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.base_trainer import finish_rendered, rendered_sums
    size, faces = (72, 88), template()[2]
    Fc = faces.shape[1]
    (va, Ka, _), (vb, _, _) = case_inputs('A', size), case_inputs('B', size)
    rp = case_ref('A', size)
    vp, vg = np.concatenate((va, va, va)), np.concatenate((va, vb, va))
    valid = np.array([[1, 1], [1, 1], [0, 1]], np.float32)
    depth = np.where(rp['depth'][0] > 0, rp['depth'][0] + 0.002, 0.0).astype(np.float32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z = torch.zeros(3, 2, 21, 3, device='cuda')
    tup = (cu(vp), z, cu(vg), z, z, cu(vp), z, cu(vg), z)
    batch = {'K_new': cu(np.tile(Ka, (3, 1, 1))), 'valid': cu(valid), 'input': torch.zeros(3, 3, *size, device='cuda'),
             'depth': cu(np.tile(depth, (3, 1, 1, 1)))}
    got = rendered_sums(tup, batch, cu(faces))
    assert got.dtype == torch.float64 and got.shape == (8,) and got.is_cuda
    got = got.cpu().numpy()
    fp, dp = F.render_hands(cu(vp), cu(faces), batch['K_new'], size, valid=cu(valid))
    fg, _ = F.render_hands(cu(vg), cu(faces), batch['K_new'], size, valid=cu(valid))
    fp, fg, dp = fp.cpu().numpy(), fg.cpu().numpy(), dp.cpu().numpy().astype(np.float64)
    want = np.zeros(8)
    want[0] = want[7] = 3
    for b in range(3):
        for h in range(2):
            a, g = (fp[b] >= h * Fc) & (fp[b] < (h + 1) * Fc), (fg[b] >= h * Fc) & (fg[b] < (h + 1) * Fc)
            if valid[b, h] == 1 and (a | g).any():
                want[1 + h] += (a & g).sum() / (a | g).sum()
                want[3 + h] += 1
    seen = (fp >= 0) & (depth[None] > 0)                          # (the comparison's arithmetic is pinned above: here, the kernel's own maps)
    want[5], want[6] = np.abs(dp - depth[None])[seen].sum(), seen.sum()
    print("  got %s\n  want %s" % (got.tolist(), want.tolist()))
    assert got[0] == 3 and got[7] == 3 and got[3] == 2 and got[4] == 3 and np.abs(got[1:5] - want[1:5]).max() <= 1e-12
    assert 1.0 < got[1] < 2.0 and 2.0 < got[2] < 3.0              # IoU 1 against itself, below 1 against the other pose
    assert got[6] == want[6] and abs(got[5] - want[5]) <= 1e-6 * want[5]
    amb = int(rp['ambiguous'][0].sum())
    two = np.abs(dp[:2] - depth[None])[seen[:2]]                  # samples 0 and 1 show the surface the sensor map was made from
    assert (np.abs(two - 0.002) > 1e-5).sum() <= 2 * amb
    out = finish_rendered(torch.from_numpy(got))
    assert abs(out['sil_iou_left'] - got[1] / 2) <= 1e-12 and abs(out['sil_iou_right'] - got[2] / 3) <= 1e-12 and out['rendered_samples'] == 3
    without = rendered_sums(tup, {k: v for k, v in batch.items() if k != 'depth'}, cu(faces)).cpu().numpy()
    assert np.array_equal(without[:5], got[:5]) and (without[5:] == 0).all()


@functools.lru_cache(maxsize=None)
def evaluation_runs():
    """The fixture of tests/test_eval_interaction_gpu.py::evaluation_runs: R = 128, B = 3, two batches, random-init model."""
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer, rendered_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 3
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev))
    loader = [synthetic_train_batch(B, R, seed=s, consts=consts) for s in (21, 22)]
    runs = {'plain': tr.evaluation(loader), 'off': tr.evaluation(loader, rendered=False), 'on': tr.evaluation(loader, rendered=True),
            'others': tr.evaluation(loader, aligned=True, interaction=True), 'all': tr.evaluation(loader, aligned=True, interaction=True, rendered=True),
            'interaction': tr.evaluation(loader, interaction=True), 'interaction_on': tr.evaluation(loader, interaction=True, rendered=True)}
    assert m.training
    sums = torch.zeros(8, dtype=torch.float64, device=dev)
    tr.model_with_loss.eval()
    with torch.no_grad():
        for b in loader:
            bd = tree_to({k: v for k, v in b.items() if torch.is_tensor(v)}, dev)
            sums += rendered_sums(tr.model_with_loss(bd, 'test', None), bd, tr.model_with_loss.loss.faces_pair)
    tr.model_with_loss.train()
    return runs, sums.cpu()


def test_evaluation_rendered_keys():
    """The plumbing: the flag off changes nothing; the flag on changes no other key, alone or with `aligned` and `interaction` (whose block is
    read from the end of the shared buffer); the new keys are finish_rendered of the summed rendered_sums."""
    from pdfnet_amd.trains.base_trainer import RENDERED_KEYS, finish_rendered
    runs, sums = evaluation_runs()
    plain = runs['plain']
    assert plain['samples'] == 6 and runs['off'] == plain and list(runs['off']) == list(plain)
    want = finish_rendered(sums)
    print("  sums %s" % sums.tolist())
    assert list(want) == list(RENDERED_KEYS) and want['rendered_samples'] == 6
    for base, on in ((plain, runs['on']), (runs['others'], runs['all']), (runs['interaction'], runs['interaction_on'])):
        assert list(on) == list(base) + list(RENDERED_KEYS)
        for k, v in base.items():
            assert on[k] == v, k
        for k in RENDERED_KEYS:
            assert on[k] == runs['on'][k], k
    for k in RENDERED_KEYS:
        print("  %-18s got %.9g want %.9g" % (k, runs['on'][k], want[k]))
        assert np.isfinite(runs['on'][k]) and abs(runs['on'][k] - want[k]) <= 1e-12, (k, runs['on'][k], want[k])
    for k in ('sil_iou_left', 'sil_iou_right', 'sil_iou'):
        assert 0.0 <= runs['on'][k] <= 1.0
    assert runs['on']['depth_res_mm'] >= 0                       # (0 when the random model's hands cover no measured pixel)


def test_write_rendered_scores_appends_its_own_block(tmp_path):
    from pdfnet_amd.trains.base_trainer import RENDERED_KEYS, write_h2o_scores, write_rendered_scores
    ev = evaluation_runs()[0]['all']
    path = str(tmp_path / 'H2O-val.txt')
    write_h2o_scores(path, ev)
    before = open(path).read()
    write_rendered_scores(path, ev)
    text = open(path).read()
    assert text.startswith(before)
    assert text[len(before):].splitlines() == ['eval rendered '] + ['%s: %.2f' % (k, ev[k]) for k in RENDERED_KEYS]


# ---- HandRenderer -------------------------------------------------------------------------------------
def test_hand_renderer():
    from pdfnet_amd import functional as F
    from pdfnet_amd.render import HandRenderer
    verts, K, size = case_inputs('B')
    faces = template()[2]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    v, f, k = cu(verts), cu(faces), cu(K)
    r = HandRenderer(f, size)
    img, alpha = r.render_rgb(k, v[:, 0], v[:, 1])
    col = torch.tensor([LEFT_COLOUR, RIGHT_COLOUR], device='cuda')[:, None, :].expand(2, 778, 3)
    face, depth, rgb = F.render_hands(v, f, k, size, colour=col, table=F.vertex_face_table(f, 778))
    assert img.shape == (1, 72, 88, 3) and alpha.shape == (1, 72, 88)
    assert torch.equal(img, rgb / 255) and torch.equal(alpha, (face >= 0).float()) and 0.2 < float(alpha.mean()) < 0.8
    assert float(img.max()) <= 1.0 and float(img[alpha > 0].min()) > 0.1
    custom = torch.cat((col[0], col[1])) * 0.5                                                 # [2n, 3], the reference's layout
    assert torch.equal(r.render_rgb(k, v[:, 0], v[:, 1], v_color=custom)[0], F.render_hands(v, f, k, size, colour=col * 0.5)[2] / 255)
    assert torch.equal(r.render_depth(k, v[:, 0], v[:, 1]), depth)
    mask = r.render_mask(k, v[:, 0], v[:, 1])
    Fc = faces.shape[1]
    left, right = (face >= 0) & (face < Fc), face >= Fc
    assert (mask[left] - torch.tensor([0.0, 0.0, 1.0], device='cuda')).abs().max() <= BARY_BAR
    assert (mask[right] - torch.tensor([0.0, 1.0, 0.0], device='cuda')).abs().max() <= BARY_BAR and (mask[face < 0] == 0).all()
    image = torch.rand(1, 72, 88, 3, device='cuda')
    over = HandRenderer.overlay(img, alpha, image)
    assert torch.equal(over[alpha > 0], img[alpha > 0]) and torch.equal(over[alpha == 0], image[alpha == 0])
    assert torch.equal(over, img * alpha[..., None] + image * (1 - alpha[..., None]))
    assert HandRenderer(f, 32).size == (32, 32)
