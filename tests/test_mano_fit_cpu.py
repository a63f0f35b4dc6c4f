"""The float64 restatement of pdf_mano_fit's contract (tests/mano_fit_ref.py) checked on its own, and the host side of the evaluation block.
No GPU.  The GPU tests measure the kernel against this restatement, so what is asserted here is what makes it a reference: an exact Jacobian,
convergence to the generating hand, a cost that never rises, and the valid / weight / prior rules."""
import pytest
import torch

from tests import mano_fit_ref as R

SEEDS, POSE_STD = (0, 1, 2), (0.2, 0.5, 0.8)


@pytest.fixture(scope='module')
def consts():
    return R.consts_of('left')


@pytest.fixture(scope='module')
def clean_fits(consts):
    """(seed, pose std) -> (target, fit) of the noise-free cases from the default start; computed once."""
    out = {}
    for seed in SEEDS:
        for s in POSE_STD:
            p_true, t = R.case(seed, s)
            out[seed, s] = (p_true, t, R.fit(consts, t, 'left'))
    return out


@pytest.mark.parametrize('at', ['random', 'zero'])
def test_jacobian_against_central_differences(consts, at):
    """h = 1e-6 in float64: truncation ~ h^2 |M'''| ~ 1e-12, rounding ~ 1e-16 |M| / h ~ 1e-11; entries of J are up to ~0.2.  Bar 1e-8.
    At the zero start every rotation is the Rodrigues edge a = 0, where the derivative of |a| is taken as 0 and dR / da_k = skew(e_k)."""
    p, t = R.case(0, 0.5)
    if at == 'zero':
        p = R.start_point(consts, t)
        assert float(p[:58].abs().max()) == 0.0
    J = R.system(consts, p, t, 'left')[0]
    assert J.shape == (2334, 61)
    h, cols = 1e-6, []
    with R.default_dtype(torch.float64):
        for i in range(R.NP):
            e = torch.zeros(R.NP, dtype=torch.float64)
            e[i] = h
            cols.append((R.model(consts, p + e, 'left')[0] - R.model(consts, p - e, 'left')[0]).reshape(-1) / (2 * h))
    err = float((torch.stack(cols, 1) - J).abs().max())
    print('max |J - central differences| = %.3g, max |J| = %.3g' % (err, float(J.abs().max())))
    assert err < 1e-8


def test_noise_free_targets_are_recovered(clean_fits, consts):
    """rms vertex residual < 1e-9 mm, 20 trial steps, the cost never above the start cost nor rising, accepted + rejected = 20.
    A fit may end on the other axis-angle of the same rotation: a' = -(2 pi - |a|) a / |a|.  The contract's Rodrigues turns by
    |a| + 1e-8, so the two representations differ by 2e-8 rad about that joint and the generating mesh is no longer in the model exactly: with a
    lever of at most 0.3 m (the synthetic hand's extent) the floor there is 6e-9 m = 6e-6 mm.  Such a case is recognised by its parameters (the
    joint's two axis-angles are opposite and their lengths add to 2 pi), every other parameter must be the generating one, and it is held to that
    floor; every case that returns the generating parameters is held to 1e-9 mm, and these must be the majority."""
    exact = 0
    for (seed, s), (p_true, t, f) in clean_fits.items():
        with R.default_dtype(torch.float64):
            rms = R.rms_mm(R.model(consts, f['p'], 'left')[0], t)
        cond = float(torch.linalg.cond(f['A']))
        same, alias = R.same_or_alias(f['p'], p_true)
        print('seed %d pose std %.1f: rms %.3g mm, accepted %d, cond(A) %.3g, aliased joints %d' % (seed, s, rms, f['accepted'], cond, int(alias.sum())))
        assert bool((same | alias).all()) and float((f['p'][48:] - p_true[48:]).abs().max()) < 1e-6
        exact += bool(same.all())
        assert rms < (1e-9 if bool(same.all()) else R.ALIAS_FLOOR_MM)
        assert f['accepted'] + f['rejected'] == 20 and f['accepted'] >= 1
        assert f['cost'] <= f['cost0']
        assert all(b <= a for a, b in zip([f['cost0']] + f['costs'], f['costs']))
    assert exact >= 6


def test_noisy_target_leaves_the_noise(consts):
    """N(0, 2 mm) per coordinate: the residual of a least-squares fit of 61 unknowns to 2334 rows has rms sqrt(3) * 2 mm * sqrt(2273 / 2334)
    = 3.42 mm per vertex, with a standard deviation of 3.42 / sqrt(2 * 2273) = 0.05 mm: the bar is 4 of those.  The same restatement in float32
    ends at the same cost to 1e-4 relative (the bar the GPU test holds the kernel to)."""
    _, t = R.case(0, 0.5, noise=0.002)
    f = R.fit(consts, t, 'left')
    with R.default_dtype(torch.float64):
        rms = R.rms_mm(R.model(consts, f['p'], 'left')[0], t)
    f32 = R.fit(R.consts_of('left', torch.float32), t.float(), 'left')
    rel = abs(f32['cost'] - f['cost']) / f['cost']
    print('rms %.4f mm, E float64 %.9g, E float32 %.9g, relative difference %.3g' % (rms, f['cost'], f32['cost'], rel))
    assert abs(rms - 3.42) < 0.2
    assert f['cost'] < f['cost0']
    assert f32['cost'] <= f['cost'] * (1 + 1e-4)


def test_float32_restatement_meets_the_gpu_bar(consts):
    """What fp32 arithmetic can reach on a noise-free target: below the 1e-3 mm the GPU test asks of the kernel (one ulp of a coordinate at
    0.5 m is 3e-5 mm)."""
    _, t = R.case(0, 0.5)
    c32 = R.consts_of('left', torch.float32)
    f = R.fit(c32, t.float(), 'left')
    with R.default_dtype(torch.float32):
        rms = R.rms_mm(R.model(c32, f['p'], 'left')[0], t.float())
    print('float32 restatement: rms %.3g mm, accepted %d' % (rms, f['accepted']))
    assert rms < 1e-3 and f['cost'] <= f['cost0']


def test_invalid_row_takes_no_step(consts):
    _, t = R.case(1, 0.5)
    f = R.fit(consts, t, 'left', valid=False)
    assert torch.equal(f['p'], R.start_point(consts, t))
    assert (f['cost0'], f['cost'], f['accepted'], f['rejected'], f['lam']) == (0.0, 0.0, 0, 0, 1e-3)


def test_start_point_and_init(consts):
    p_true, t = R.case(1, 0.2)
    p0 = R.start_point(consts, t)
    assert float(p0[:58].abs().max()) == 0.0
    assert torch.allclose(p0[58:], t.mean(0) - consts['v_template'].mean(0), rtol=0, atol=1e-15)
    f = R.fit(consts, t, 'left', init=p_true, iters=3)           # started at the answer: nothing to gain
    assert f['cost0'] < 1e-25 and f['cost'] <= f['cost0']


def test_zero_weights_ignore_their_vertices(consts):
    """5 mm noise on a random half of the vertices, zero weight there: the weighted half is fitted as if there were no noise (to 1e-9 mm, or
    to the floor of an aliased axis-angle, see test_noise_free_targets_are_recovered)."""
    p_true, t = R.case(2, 0.5)
    g = torch.Generator().manual_seed(5)
    off = torch.randperm(R.NV, generator=g)[:R.NV // 2]
    w = torch.ones(R.NV, dtype=torch.float64)
    w[off] = 0
    noisy = t.clone()
    noisy[off] += 0.005 * torch.randn(len(off), 3, dtype=torch.float64, generator=g)
    f = R.fit(consts, noisy, 'left', weight=w)
    with R.default_dtype(torch.float64):
        v = R.model(consts, f['p'], 'left')[0]
    keep = w > 0
    same, alias = R.same_or_alias(f['p'], p_true)
    assert bool((same | alias).all())
    assert R.rms_mm(v[keep], t[keep]) < (1e-9 if bool(same.all()) else R.ALIAS_FLOOR_MM)
    assert R.rms_mm(v[~keep], noisy[~keep]) > 1.0                 # the noise is still there, unfitted


def test_priors(consts):
    _, t = R.case(0, 0.5)
    f = R.fit(consts, t, 'left', prior_shape=1e6)
    assert float(f['p'][48:58].norm()) < 1e-3 and f['cost'] < f['cost0']
    f = R.fit(consts, t, 'left', prior_pose=0.05, iters=6)
    p = f['p']
    with R.default_dtype(torch.float64):
        data = float(((R.model(consts, p, 'left')[0] - t) ** 2).sum())
    assert abs(f['cost'] - (data + 0.05 * float((p[3:48] ** 2).sum()))) <= 1e-12 * f['cost']
    assert f['cost'] == R.energy(consts, p, t, 'left', prior_pose=0.05)


def test_finish_mano_fit_on_a_hand_made_accumulator():
    from pdfnet_amd.trains.base_trainer import MANO_FIT_KEYS, MANO_FIT_SUMS, finish_mano_fit
    # 5 samples, the left hand valid in 4 of them and the right in 2; sums in metres of: residual, residual of the ground truth, verts, joints
    acc = torch.tensor([5.0, 0.008, 0.003, 0.0004, 0.0001, 0.04, 0.03, 0.048, 0.02, 4.0, 2.0], dtype=torch.float64)
    assert acc.numel() == MANO_FIT_SUMS
    out = finish_mano_fit(acc)
    assert list(out) == list(MANO_FIT_KEYS)
    want = {'mano_residual_left': 2.0, 'mano_residual_right': 1.5, 'mano_residual': 1.75,
            'mano_residual_gt_left': 0.1, 'mano_residual_gt_right': 0.05, 'mano_residual_gt': 0.075,
            'mano_abs_verts_left': 10.0, 'mano_abs_verts_right': 15.0, 'mano_abs_verts': 12.5,
            'mano_abs_joints_left': 12.0, 'mano_abs_joints_right': 10.0, 'mano_abs_joints': 11.0, 'mano_fit_samples': 5}
    assert set(want) == set(MANO_FIT_KEYS)
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-12, (k, out[k], v)
    assert isinstance(out['mano_fit_samples'], int)
    # a hand that is never valid: its means are 0 and the two-hand figure is the other hand's
    acc[2::2][:4] = 0
    acc[10] = 0
    out = finish_mano_fit(acc)
    assert out['mano_residual_right'] == 0.0 and out['mano_residual'] == out['mano_residual_left'] == 2.0
    assert finish_mano_fit(torch.zeros(MANO_FIT_SUMS, dtype=torch.float64)) == {'mano_fit_samples': 0}


def test_write_mano_fit_scores_format(tmp_path):
    from pdfnet_amd.trains.base_trainer import MANO_FIT_KEYS, write_mano_fit_scores
    ev = {k: 0.5 * (i + 1) for i, k in enumerate(MANO_FIT_KEYS)}
    path = str(tmp_path / 'scores.txt')
    write_mano_fit_scores(path, ev)
    write_mano_fit_scores(path, ev)                              # appends
    block = ['eval mano-fit '] + ['%s: %.2f' % (k, ev[k]) for k in MANO_FIT_KEYS]
    assert open(path).read().splitlines() == block + block


def test_header_declares_the_fit():
    from pdfnet_amd.hip import parse_header
    import ctypes
    protos = parse_header()
    ret, args = protos['pdf_mano_fit']
    assert ret is ctypes.c_int and len(args) == 24 and args[9:14] == [ctypes.c_int] * 3 + [ctypes.c_float] * 2
    assert protos['pdf_mano_fit_workspace_floats'] == (ctypes.c_long, [ctypes.c_int])
