"""Host side of the soft-silhouette loss: conditions on the float64 restatement of tests/test_silhouette_loss_gpu.py (its gradient against
central differences of its own loss, its dependence on the cutoff, the numbers worked out by hand), the input conditions of the GPU cases, the
prototype of pdf_silhouette_loss in the header and its refusals, and the errors of F.silhouette_loss and of the training term without a GPU.

The central differences move ONE coordinate of one vertex at a time by the 3-D step that moves its projection by 1e-4 px (X: Z / K00,
Y: Z / K11, Z: Z^2 / max(K00 |X|, K11 |Y|), at most ten times the step in X for a vertex near the optical axis), with the cutoff widened
to 40 sigma: a face whose inclusion flips inside a step then carries sigmoid(-40) = 4e-18."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT

FD_STEP_PX, FD_BAR, FD_CUTOFF = 1e-4, 1e-6, 40.0                  # px; of the case's max |grad|.  Measured: 9e-10 .. 6e-9, and 1.1e-7 with per-sample cameras


def restate(c, **over):
    from tests.test_silhouette_loss_gpu import ref_silhouette
    kw = dict(cutoff=16.0, budget=False)
    kw.update(over)
    return ref_silhouette(c['verts'], c['faces'], c['K'], c['mask'], c['weight'], c['valid'], c['sigma'], c['z_near'], **kw)


@pytest.mark.parametrize("name,top", [('octahedron', None), ('fractional', None), ('outside', None), ('cameras', None), ('strip', 2)])
def test_gradient_against_central_differences(name, top):
    """Every vertex of the small cases; the `top` vertices of largest gradient per hand of the strip.  (Not the by-hand case: its pixel
    centres on the line x = y are exactly as near to one leg of the triangle as to the other, where the minimum over the edges has a kink and
    a central difference averages the two one-sided derivatives; test_by_hand checks that gradient against plain arithmetic instead.)"""
    from tests.test_silhouette_loss_gpu import case
    c = case(name)
    base = restate(c, cutoff=FD_CUTOFF)
    grad = base['grad']
    peak = np.abs(grad).max()
    assert peak > 0
    V, K = c['verts'].astype(np.float64), c['K'].astype(np.float64)
    worst, moved = 0.0, 0
    for b in range(V.shape[0]):
        for h in range(2):
            norms = np.linalg.norm(grad[b, h], axis=-1)
            for i in (range(V.shape[2]) if top is None else np.argsort(-norms)[:top]):
                X, Y, Z = V[b, h, i]
                if not base['used'][b, h, i]:
                    assert (grad[b, h, i] == 0).all()
                    continue
                steps = (Z / K[b, 0, 0], Z / K[b, 1, 1], min(Z * Z / max(K[b, 0, 0] * abs(X), K[b, 1, 1] * abs(Y), 1e-300), 10 * Z / K[b, 0, 0]))
                for k in range(3):
                    ends = []
                    for sign in (1.0, -1.0):
                        W = dict(c, verts=V[b:b + 1].copy(), K=c['K'][b:b + 1], mask=c['mask'][b:b + 1],
                                 weight=None if c['weight'] is None else c['weight'][b:b + 1], valid=None if c['valid'] is None else c['valid'][b:b + 1])
                        W['verts'][0, h, i, k] += sign * FD_STEP_PX * steps[k]
                        ends.append(restate(W, cutoff=FD_CUTOFF)['loss'].sum())
                    worst = max(worst, abs((ends[0] - ends[1]) / (2 * FD_STEP_PX * steps[k]) - grad[b, h, i, k]))
                    moved += 1
    print("  %s: %d central differences within %.2e of max |grad| = %.3e" % (name, moved, worst / peak, peak))
    assert moved >= 12 and worst <= FD_BAR * peak, (name, worst, peak)


@pytest.mark.parametrize("name", ['octahedron', 'strip', 'cameras', 'by-hand'])
def test_cutoff(name):
    """rho^2 = 16 sigma against 40 sigma: a face that only the wider box includes lies at x <= -16, so T changes by at most
    T (exp(extra faces x log1p(exp(-16))) - 1) < 2e-7 per such face, and not at all where the two sets are the same."""
    from tests.test_silhouette_loss_gpu import case
    c = case(name)
    near, far = restate(c), restate(c, cutoff=40.0)
    extra = far['faces_at'] - near['faces_at']
    assert (extra >= 0).all() and extra.max() > 0
    d = np.abs(near['T'] - far['T'])
    print("  %s: up to %d more faces a pixel, max |T16 - T40| %.2e, loss differs by %.2e" % (name, extra.max(), d.max(), np.abs(near['loss'] - far['loss']).max()))
    assert (d <= 2e-7 * extra).all() and (d[extra == 0] == 0).all()
    assert np.abs(near['loss'] - far['loss']).max() <= 2e-7 * extra.max()


def test_by_hand():
    from tests.test_silhouette_loss_gpu import by_hand_loss_and_gradient, by_hand_pixels, case, sigmoid
    c = case('by-hand')
    r = restate(c)
    S = 1 - r['T']
    a, b, outside = by_hand_pixels(S[0, 0])
    assert abs(a) <= 1e-15 and abs(b) <= 1e-15 and outside == 0.0 and r['T'][0, 0, 20, 20] == 1.0
    assert r['faces_at'][0, 0].max() == 1 and r['faces_at'][0, 0, :16, :16].all() and r['faces_at'][0, 0, 16:].sum() == 0       # the zero-area face is skipped
    # the right hand: the same triangle and a second one, S = 1 - (1 - p1)(1 - p2)
    only = dict(c, faces=np.array([[[0, 1, 2], [3, 3, 4]], [[3, 4, 5], [3, 3, 4]]], np.int64))
    p2 = 1 - restate(only)['T'][0, 1]
    assert np.abs(S[0, 1] - (1 - (1 - S[0, 0]) * (1 - p2))).max() <= 1e-15 and r['faces_at'][0, 1].max() == 2 and (p2[6:8, 4:7] > 0.5).all() and (S[0, 0][6:8, 4:7] > 0.5).all()
    loss, I, U, grad = by_hand_loss_and_gradient()
    assert abs(r['loss'][0, 0] - loss) <= 1e-14 and abs(r['sums'][0, 0, 0] - I) <= 1e-11 and abs(r['sums'][0, 0, 1] - U) <= 1e-11
    assert np.abs(r['grad'][0, 0, :3] - grad).max() <= 1e-14 and (r['grad'][0, 0, 3:] == 0).all() and np.abs(grad).max() > 1e-3
    assert 0.05 < loss < 0.95 and abs(sigmoid(4.5) - 0.98901305736940681) < 1e-15 and abs(sigmoid(-2.25) - 0.09534946489910949) < 1e-15


def test_input_conditions_of_the_gpu_test():
    """Every case meant to carry signal does, on the float64 side, and holds what it is there for."""
    from tests.test_silhouette_loss_gpu import CASES, case, non_hollow, reference
    for name in CASES:
        c, r = case(name), reference(name)
        ok, figures = non_hollow(name)
        print("  %-12s delta-free bars: %s; faces per pixel <= %d, border pixels %d" % (name, figures, r['faces_at'].max(), r['flips'].sum()))
        assert ok, name
        assert np.isfinite(r['loss']).all() and np.isfinite(r['grad']).all() and np.isfinite(r['e_grad']).all()
    r = reference('skipped')
    assert not r['used'][0, 0, 6:].any() and not r['used'][0, 1, 4] and not r['used'][1, 0, 0] and not r['used'][1, 1, 5] and r['used'][0, 1, 5]
    r = reference('outside')
    assert r['loss'][0, 1] == 1.0 and (r['T'][0, 1] == 1).all() and (r['grad'][0, 1] == 0).all() and (r['grad'][0, 0] != 0).any()
    r = reference('invalid')
    assert r['loss'][0, 1] == 0 and r['loss'][1, 0] == 0 and (r['T'][0, 1] == 1).all() and (r['grad'][1, 0] == 0).all()
    r = reference('zero-mask')
    assert (r['loss'] == 1).all() and (r['grad'] == 0).all() and (r['T'] < 0.5).any()
    c = case('fractional')
    assert ((c['mask'] > 0) & (c['mask'] < 1)).any() and (c['weight'] == 0).any() and (c['weight'] > 0).any()
    assert case('strip')['faces'].shape == (2, 300, 3) and case('template-2')['verts'].shape == (1, 2, 778, 3)


def test_header_declares_silhouette_loss_and_the_library_refuses_without_a_launch():
    from pdfnet_amd import hip
    protos = hip.parse_header(os.path.join(ROOT, "include", "pdfnet_hip.h"))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["pdf_silhouette_loss"] == (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, Fl, Fl, P, P, P, P, P, P])
    c = hip.lib().cdll
    assert hasattr(c, "pdf_silhouette_loss")
    call = lambda B=1, n=778, Fc=1538, M=8, H=128, W=128, sigma=1.0: c.pdf_silhouette_loss(None, None, None, None, None, None, None, B, n, Fc, M, H, W,
                                                                                         Fl(sigma), Fl(0.01), None, None, None, None, None, None)
    assert call(B=0) == 0 and call(B=-1) == 0
    for kw in (dict(n=0), dict(n=1025), dict(Fc=0), dict(Fc=2049), dict(M=0), dict(M=33), dict(H=0), dict(H=2049), dict(W=0), dict(W=2049),
               dict(B=65536), dict(sigma=0.0), dict()):                # the last: no vertices, no outputs
        assert call(**kw) == -1, kw


def test_silhouette_loss_errors_without_a_gpu():
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains.simplified import CtdetLoss, silhouette_term
    v, f, K, m = torch.zeros(1, 2, 4, 3, requires_grad=True), torch.zeros(2, 4, 3, dtype=torch.long), torch.eye(3)[None], torch.zeros(1, 2, 8, 8)
    f[:] = torch.tensor([0, 1, 2])
    for bad, word in ((lambda: F.silhouette_loss(v[..., :2], f, K, m), "verts"), (lambda: F.silhouette_loss(v, f[:1], K, m), "faces"),
                      (lambda: F.silhouette_loss(v, f, K[0], m), "wants K"), (lambda: F.silhouette_loss(v, f, K, m[:, :1]), "wants mask"),
                      (lambda: F.silhouette_loss(v, f, K, m[0]), "wants mask"), (lambda: F.silhouette_loss(v, f, K, m, weight=m[..., :4]), "wants weight"),
                      (lambda: F.silhouette_loss(v, f, K, m, valid=torch.ones(2, 2)), "wants valid"), (lambda: F.silhouette_loss(v, f, K, m, sigma=0.0), "sigma"),
                      (lambda: F.silhouette_loss(v, f, K, m, z_near=0.0), "z_near"), (lambda: F.silhouette_loss(v, f, K, torch.zeros(1, 2, 8, 2049)), "1 to 2048 pixels"),
                      (lambda: F.silhouette_loss(torch.zeros(1, 2, 1025, 3), f, K, m), "1 to 1024 vertices"),
                      (lambda: F.silhouette_loss(v, f, K, m, table=torch.zeros(2, 5, 3, dtype=torch.int32)), "wants table")):
        with pytest.raises(ValueError, match=word):
            bad()
    with pytest.raises(RuntimeError, match="GPU"):                 # well-formed: it gets as far as the kernel's door
        F.silhouette_loss(v, f, K, m, return_fields=True)
    with pytest.raises(RuntimeError, match="GPU"):
        F.silhouette_loss(v.detach(), f, K, m, weight=1 - m, valid=torch.ones(1, 2))
    batch = {'valid': torch.ones(1, 2), 'K_new': torch.eye(3)[None], 'ind': torch.zeros(1, 2, dtype=torch.long)}
    faces = torch.zeros(2, 1538, 3, dtype=torch.long)
    with pytest.raises(KeyError, match="mask"):
        silhouette_term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, faces, 128)
    batch['mask'] = torch.zeros(1, 2, 128, 128)
    with pytest.raises(RuntimeError, match="GPU"):
        silhouette_term(torch.zeros(2, 1, 778, 3), torch.zeros(2, 1, 3), batch['ind'], batch, faces, 128)
    assert "silhouette_weight" in CtdetLoss.__doc__ and "silhouette_sigma" in CtdetLoss.__doc__ and "silhouette_down" in CtdetLoss.__doc__
