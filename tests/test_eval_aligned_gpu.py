"""Aligned evaluation metrics on the GPU (csrc/metrics.hip, F.procrustes_dist / F.mesh_nn_counts, Trainer.evaluation(aligned=True)) against a
float64 numpy restatement of the reference's arithmetic: align_w_scale (lib/utils/eval.py:96-119, scipy's orthogonal_procrustes written
out with np.linalg.svd), calculate_fscore (eval.py:54-73, nearest neighbours by brute force) and EvalUtil.get_measures
(lib/utils/eval_util.py:53-94).

Bars: `sum` and `dist` 1e-4 relative (the MPJPE row of DESIGN.md section 2) + 1e-6 m, aligned coordinates and nearest-neighbour distances
1e-6 m + 1e-5 relative, counts exact.  A count is discontinuous at its threshold, so every exact comparison first checks ON THE FLOAT64 SIDE
that no distance lies within 1e-5 m of a threshold (fp32 distances of points in a 0.5 m box are good to ~1e-7 m); the seeds below pass that
check at the first draw, and a draw that does not is replaced by the next seed."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.util import make_opt, tree_to

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
F_THR = (0.005, 0.015)


# ---- float64 restatement -----------------------------------------------------------------------
def ref_align(gt, pred):
    """align_w_scale(gt, pred) -> the aligned prediction, float64 [n, 3]."""
    gt, pred = gt.astype(np.float64), pred.astype(np.float64)
    t1, t2 = gt.mean(0), pred.mean(0)
    a, b = gt - t1, pred - t2
    s1 = np.linalg.norm(a) + 1e-8
    a = a / s1
    s2 = np.linalg.norm(b) + 1e-8
    b = b / s2
    u, w, vt = np.linalg.svd(a.T.dot(b))                      # orthogonal_procrustes(a, b): R = u vt, scale = sum of the singular values
    return np.dot(b, u.dot(vt).T) * w.sum() * s1 + t1


def ref_procrustes(gt, pred):
    """[rows, n, 3] each -> (sum [rows], dist [rows, n], aligned [rows, n, 3]) in float64."""
    al = np.stack([ref_align(g, p) for g, p in zip(gt, pred)])
    d = np.linalg.norm(al - gt.astype(np.float64), axis=-1)
    return d.sum(-1), d, al


def ref_nn(gt, pred):
    """[n, 3] each -> (d_gt, d_pred): distance of every gt point to its nearest predicted point and the other way round (float64)."""
    d = np.linalg.norm(gt.astype(np.float64)[:, None] - pred.astype(np.float64)[None], axis=-1)
    return d.min(1), d.min(0)


def ref_fscore(d_gt, d_pred, th):
    recall = float((d_pred < th).sum()) / len(d_pred)
    precision = float((d_gt < th).sum()) / len(d_gt)
    return 2 * recall * precision / (recall + precision) if recall + precision > 0 else 0.0


def ref_auc(dists):
    """dists [N, 21] -> auc_all of EvalUtil.get_measures(0, 0.05, 100) fed N times with every keypoint visible."""
    t = np.linspace(0.0, 0.05, 100)
    trapz = lambda y: (np.diff(t) * (y[1:] + y[:-1]) / 2.0).sum()
    norm = trapz(np.ones_like(t))
    return float(np.mean([trapz(np.array([np.mean((dists[:, j] <= th).astype('float')) for th in t])) / norm for j in range(dists.shape[1])]))


def clear_of(d, thresholds):
    return all(np.abs(np.asarray(d) - th).min() > MARGIN for th in thresholds)


# ---- inputs --------------------------------------------------------------------------------------
def hand_cloud(rng, rows, n):
    """Hand-sized clouds as pdfnet_amd/synthetic.py places them: xy ~ U(-0.1, 0.1), z ~ U(0.4, 0.5) metres."""
    return np.concatenate((rng.uniform(-0.1, 0.1, (rows, n, 2)), rng.uniform(0.4, 0.5, (rows, n, 1))), -1).astype(np.float32)


def similarity(rng, gt, noise=0.005):
    """A random similarity image of every row (proper rotation, scale 0.7-1.4, shift up to 0.2 m) plus N(0, noise) per coordinate."""
    out = np.empty(gt.shape, np.float64)
    for r, g in enumerate(gt):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.linalg.det(q))
        out[r] = rng.uniform(0.7, 1.4) * g.astype(np.float64).dot(q.T) + rng.uniform(-0.2, 0.2, 3)
    return (out + rng.standard_normal(gt.shape) * noise).astype(np.float32)


@functools.lru_cache(maxsize=None)
def procrustes_case(rows, n):
    rng = np.random.default_rng(1000 * rows + n)
    gt = hand_cloud(rng, rows, n)
    pred = similarity(rng, gt)
    return gt, pred, ref_procrustes(gt, pred)


def run_procrustes(pred, gt):
    from pdfnet_amd import functional as F
    s, d, a = F.procrustes_dist(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), return_aligned=True)
    return s.cpu().double().numpy(), d.cpu().double().numpy(), a.cpu().double().numpy()


def check_dist(got_sum, got_dist, want_sum, want_dist):
    es, ed = np.abs(got_sum - want_sum), np.abs(got_dist - want_dist)
    print("  sum err max %.3e (sum max %.3e), dist err max %.3e (dist max %.3e)" % (es.max(), want_sum.max(), ed.max(), want_dist.max()))
    assert np.isfinite(got_sum).all() and np.isfinite(got_dist).all()
    assert (es <= 1e-4 * np.abs(want_sum) + 1e-6).all(), (es.max(), want_sum)
    assert (ed <= 1e-4 * np.abs(want_dist) + 1e-6).all(), ed.max()


def check_aligned(got, want):
    e = np.abs(got - want)
    print("  aligned err max %.3e" % e.max())
    assert (e <= 1e-6 + 1e-5 * np.abs(want)).all(), e.max()


# ---- pdf_procrustes_dist ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n", [(1, 21), (7, 21), (3, 778), (2, 1024), (2, 1)])
def test_procrustes_matches_float64(rows, n):
    """Fewer points than threads, an odd row count, a point count that is no multiple of 64 or 256, the cap, a single point."""
    from pdfnet_amd import functional as F
    gt, pred, (ws, wd, wa) = procrustes_case(rows, n)
    s, d, a = run_procrustes(pred, gt)
    assert s.shape == (rows,) and d.shape == (rows, n) and a.shape == (rows, n, 3)
    check_dist(s, d, ws, wd)
    check_aligned(a, wa)
    # without the optional outputs: the same sums; leading dimensions are kept
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    s2, d2 = F.procrustes_dist(p.reshape(rows, 1, n, 3), g.reshape(rows, 1, n, 3))
    assert s2.shape == (rows, 1) and d2.shape == (rows, 1, n)
    assert np.array_equal(s2.cpu().double().numpy().reshape(-1), s) and np.array_equal(d2.cpu().double().numpy().reshape(rows, n), d)
    sums = torch.full((rows,), -1.0, device='cuda')
    F._L().pdf_procrustes_dist(p.data_ptr(), g.data_ptr(), rows, n, sums.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(sums.cpu().double().numpy(), s)


@pytest.mark.parametrize("n", [21, 778])
def test_procrustes_exact_similarity_and_mirror_align_to_zero(n):
    """An exact similarity image of gt has no aligned error; neither has the MIRROR image (x negated): R is the orthogonal Procrustes solution
    without a determinant correction (scipy / FreiHAND convention)."""
    rng = np.random.default_rng(7 + n)
    gt = hand_cloud(rng, 3, n)
    for pred in (similarity(rng, gt, noise=0.0), gt * np.array([-1, 1, 1], np.float32)):
        ws, wd, wa = ref_procrustes(gt, pred)
        assert ws.max() < 1e-6 * n                             # (float64 side: what is left is the fp32 rounding of the inputs)
        s, d, a = run_procrustes(pred, gt)
        check_dist(s, d, ws, wd)
        check_aligned(a, wa)
        assert np.abs(a - gt).max() < 1e-6


@pytest.mark.parametrize("n", [21, 778])
def test_procrustes_coplanar_sets_give_the_float64_distances(n):
    """Rank-deficient cross products: pred coplanar (z constant), then gt coplanar.  The rotation is not unique -- the null singular direction
    is annihilated by the centred prediction, or mirrors across the plane of gt -- but the distances are; aligned coordinates are not compared."""
    rng = np.random.default_rng(11 + n)
    for which in ("pred", "gt"):
        gt = hand_cloud(rng, 3, n)
        pred = similarity(rng, gt)
        (pred if which == "pred" else gt)[..., 2] = 0.45
        ws, wd, _ = ref_procrustes(gt, pred)
        s, d, a = run_procrustes(pred, gt)
        assert np.isfinite(a).all()
        check_dist(s, d, ws, wd)


def test_procrustes_identical_predicted_points_align_to_the_gt_mean():
    rng = np.random.default_rng(13)
    gt = hand_cloud(rng, 3, 21)
    pred = np.repeat(similarity(rng, gt)[:, :1], 21, axis=1)
    ws, wd, wa = ref_procrustes(gt, pred)
    s, d, a = run_procrustes(pred, gt)
    mean = gt.astype(np.float64).mean(1, keepdims=True)
    assert np.abs(a - mean).max() <= 1e-6 and np.abs(wa - mean).max() <= 1e-6
    check_dist(s, d, ws, wd)


def test_procrustes_two_runs_are_bit_identical():
    gt, pred, _ = procrustes_case(3, 778)
    from pdfnet_amd import functional as F
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    first, second = F.procrustes_dist(p, g, return_aligned=True), F.procrustes_dist(p, g, return_aligned=True)
    for x, y in zip(first, second):
        assert torch.equal(x, y)


def test_more_than_1024_points_are_refused():
    """n = 1025: the library returns PDF_E_BADARG without a launch, the functional wrappers raise; so does a last dimension that is not 3."""
    from pdfnet_amd import functional as F
    c = F._L().cdll
    x = torch.zeros(1, 1025, 3, device='cuda')
    out = torch.zeros(1025 * 3, device='cuda')
    cnt = torch.zeros(4, dtype=torch.int32, device='cuda')
    thr = (ctypes.c_float * 2)(*F_THR)
    vp = ctypes.c_void_p
    assert c.pdf_procrustes_dist(vp(x.data_ptr()), vp(x.data_ptr()), 1, 1025, vp(out.data_ptr()), None, None, None) == -1
    assert c.pdf_mesh_nn_counts(vp(x.data_ptr()), vp(x.data_ptr()), 1, 1025, thr, 2, vp(cnt.data_ptr()), None, None, None) == -1
    assert c.pdf_mesh_nn_counts(vp(x.data_ptr()), vp(x.data_ptr()), 1, 21, thr, 5, vp(cnt.data_ptr()), None, None, None) == -1
    assert c.pdf_procrustes_dist(None, None, 0, 21, None, None, None, None) == 0 and c.pdf_procrustes_dist(None, None, 3, 0, None, None, None, None) == 0
    assert c.pdf_mesh_nn_counts(None, None, 0, 21, thr, 2, None, None, None, None) == 0
    for call in (lambda: F.procrustes_dist(x, x), lambda: F.mesh_nn_counts(x, x, F_THR),
                 lambda: F.procrustes_dist(x[:, :21, :2], x[:, :21, :2]), lambda: F.mesh_nn_counts(x[:, :21], x[:, :22], F_THR),
                 lambda: F.mesh_nn_counts(x[:, :21], x[:, :21], (0.001,) * 5)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        F.procrustes_dist(x.cpu(), x.cpu())


# ---- pdf_mesh_nn_counts ----------------------------------------------------------------------------
NN_SEEDS = {(1, 21): 0, (3, 778): 7, (2, 1024): 3}            # first draws that keep every distance clear of the thresholds (found on the CPU)


def nn_draw(rows, n, seed):
    """gt cloud and a prediction displaced per point by 0.5-4 mm, 6-13 mm or 17-30 mm in a random direction: both counts of every row fall
    strictly between 0 and n at 5 mm and at 15 mm, and few nearest-neighbour distances come near a threshold."""
    rng = np.random.default_rng([rows, n, seed])
    gt = hand_cloud(rng, rows, n)
    lo, hi = np.array([0.0005, 0.006, 0.017]), np.array([0.004, 0.013, 0.030])
    band = rng.choice(3, size=(rows, n), p=(0.4, 0.4, 0.2))
    band[:, :3] = np.arange(3)                                 # every band in every row, also at n = 21
    length = rng.uniform(lo[band], hi[band])
    dirs = rng.standard_normal((rows, n, 3))
    pred = (gt + dirs / np.linalg.norm(dirs, axis=-1, keepdims=True) * length[..., None]).astype(np.float32)
    nn = [ref_nn(g, p) for g, p in zip(gt, pred)]
    return gt, pred, np.stack([d[0] for d in nn]), np.stack([d[1] for d in nn])


def nn_counts(d_gt, d_pred):
    return np.stack([np.stack(((d_gt < th).sum(-1), (d_pred < th).sum(-1)), -1) for th in F_THR], -2)       # [rows, T, 2]


@functools.lru_cache(maxsize=None)
def nn_case(rows, n):
    for seed in range(NN_SEEDS[(rows, n)], NN_SEEDS[(rows, n)] + 1000):
        gt, pred, d_gt, d_pred = nn_draw(rows, n, seed)
        if clear_of(np.concatenate((d_gt, d_pred)), F_THR):
            break
    else:
        raise AssertionError("no draw keeps the distances clear of the thresholds")
    counts = nn_counts(d_gt, d_pred)
    assert clear_of(np.concatenate((d_gt, d_pred)), F_THR) and (counts > 0).all() and (counts < n).all(), counts
    return seed, gt, pred, d_gt, d_pred, counts


@pytest.mark.parametrize("rows,n", sorted(NN_SEEDS))
def test_nn_counts_equal_the_float64_counts(rows, n):
    from pdfnet_amd import functional as F
    seed, gt, pred, wg, wp, want = nn_case(rows, n)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    counts, d_gt, d_pred = F.mesh_nn_counts(p, g, F_THR, return_dist=True)
    assert counts.dtype == torch.int32 and counts.shape == (rows, 2, 2) and d_gt.shape == d_pred.shape == (rows, n)
    for got, ref in ((d_gt, wg), (d_pred, wp)):
        e = np.abs(got.cpu().double().numpy() - ref)
        print("  seed %d: nn distance err max %.3e" % (seed, e.max()))
        assert (e <= 1e-6 + 1e-5 * ref).all(), e.max()
    assert np.array_equal(counts.cpu().numpy(), want), (counts.cpu().numpy(), want)
    again = F.mesh_nn_counts(p.reshape(rows, 1, n, 3), g.reshape(rows, 1, n, 3), F_THR)        # counts alone; leading dimensions kept
    assert again.shape == (rows, 1, 2, 2) and torch.equal(again.reshape(rows, 2, 2), counts)
    one = F.mesh_nn_counts(p, g, F_THR[1:])                                                      # T = 1
    assert torch.equal(one, counts[:, 1:])


# ---- Trainer.evaluation(aligned=True) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluation_runs():
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    R, B = 128, 3
    dev = torch.device('cuda')
    opt = make_opt(R, size_train=[R, R], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(5)
    m = load_model_intag(opt).to(dev)
    tr = Trainer(opt, m, CtdetLoss(opt, consts).to(dev))
    loader = [synthetic_train_batch(B, R, seed=s, consts=consts) for s in (21, 22)]
    plain, off, on = tr.evaluation(loader), tr.evaluation(loader, aligned=False), tr.evaluation(loader, aligned=True)
    assert m.training
    tups = []
    tr.model_with_loss.eval()
    with torch.no_grad():
        for b in loader:
            bd = tree_to({k: v for k, v in b.items() if torch.is_tensor(v)}, dev)
            tups.append(tuple(t.cpu().numpy() for t in tr.model_with_loss(bd, 'test', None)))
    tr.model_with_loss.train()
    return plain, off, on, tups


def test_evaluation_aligned_keys_match_the_float64_restatement():
    """Pattern of test_loss_gpu.py::test_evaluation_loop_matches_the_reference_metric_formula: B = 3, two batches.  aligned=False returns what a
    call without the keyword returns; aligned=True leaves those keys bit-identical and adds the PA errors (1e-4 relative), the F-scores and
    auc_joints.  The last two are step functions of the distances: where the float64 distances keep 1e-5 m from every threshold the counts
    behind them are the same integers and the figures agree to the float64 rounding of a different summation order (1e-12; one flipped count
    moves an F-score by > 1e-5 and the AUC by > 1e-6), otherwise within 1e-6."""
    from pdfnet_amd.trains.base_trainer import ALIGNED_KEYS
    plain, off, on, tups = evaluation_runs()
    assert plain['samples'] == 6 and off == plain and list(off) == list(plain)
    assert set(on) == set(plain) | set(ALIGNED_KEYS)
    for k, v in plain.items():
        assert on[k] == v, k
    want = {k: 0.0 for k in ALIGNED_KEYS}
    jd_all, nn_all = [], []
    for vp, jp, vg, jg in (t[:4] for t in tups):
        fs = np.zeros((2, 2))
        for b in range(vp.shape[0]):
            for h, hand in enumerate(('left', 'right')):
                jd = np.linalg.norm(ref_align(jg[b, h], jp[b, h]) - jg[b, h], axis=-1)
                va = ref_align(vg[b, h], vp[b, h])
                want['pa_%s_joints' % hand] += jd.mean() * 1000 / 6
                want['pa_%s_verts' % hand] += np.linalg.norm(va - vg[b, h], axis=-1).mean() * 1000 / 6
                d_gt, d_pred = ref_nn(vg[b, h], va)
                for t, th in enumerate(F_THR):
                    fs[t, h] += ref_fscore(d_gt, d_pred, th)
                jd_all.append(jd)
                nn_all += [d_gt, d_pred]
        for t, name in enumerate(('f5', 'f15')):
            for h, hand in enumerate(('left', 'right')):
                want['%s_%s' % (name, hand)] += fs[t, h]
    for name in ('f5', 'f15'):
        for hand in ('left', 'right'):
            want['%s_%s' % (name, hand)] /= 6
        want[name] = (want[name + '_left'] + want[name + '_right']) / 2
    want['pa_mpjpe_mm'] = (want['pa_left_joints'] + want['pa_right_joints']) / 2
    want['pa_mpvpe_mm'] = (want['pa_left_verts'] + want['pa_right_verts']) / 2
    want['auc_joints'] = ref_auc(np.stack(jd_all))
    f_clear = clear_of(np.concatenate(nn_all), F_THR)
    auc_clear = clear_of(np.concatenate(jd_all), np.linspace(0.0, 0.05, 100))
    print("  F-score distances clear of the thresholds: %s, PCK distances: %s" % (f_clear, auc_clear))
    for k in ALIGNED_KEYS:
        print("  %-16s got %.9g want %.9g" % (k, on[k], want[k]))
    for k in ALIGNED_KEYS:
        if k.startswith('pa_'):
            assert abs(on[k] - want[k]) <= 1e-4 * abs(want[k]), (k, on[k], want[k])
        else:
            bar = 1e-12 if (auc_clear if k == 'auc_joints' else f_clear) else 1e-6
            assert abs(on[k] - want[k]) <= bar, (k, on[k], want[k], bar)
    assert 0.0 <= on['auc_joints'] <= 1.0 and all(0.0 <= on[k] <= 1.0 for k in ALIGNED_KEYS if k.startswith('f'))


def test_write_aligned_scores_appends_its_own_block(tmp_path):
    from pdfnet_amd.trains.base_trainer import ALIGNED_KEYS, write_aligned_scores, write_h2o_scores
    on = evaluation_runs()[2]
    path = str(tmp_path / 'H2O-val.txt')
    write_h2o_scores(path, on)
    before = open(path).read()
    write_aligned_scores(path, on)
    text = open(path).read()
    assert text.startswith(before)
    assert text[len(before):].splitlines() == ['eval aligned '] + ['%s: %.2f' % (k, on[k]) for k in ALIGNED_KEYS]
