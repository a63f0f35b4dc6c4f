"""Restatement of `pdf_mano_fit`'s contract (include/pdfnet_hip.h), written from that comment: the oracle's `mano_lbs` as the model,
`torch.autograd.functional.jacobian` for J, the Levenberg-Marquardt rule verbatim.  Every function takes the dtype it runs in: float64 is the
reference, float32 on the CPU gives the error an fp32 evaluation of the same formulas has, which is what the GPU bars are multiples of."""
import contextlib

import numpy as np
import torch

from oracle.pdfnet_cpu import mano_lbs
from oracle.synth import synthetic_mano_consts

NP, NV = 61, 778
LAMBDA0 = 1e-3


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)          # the oracle builds its identities and zeros in the default dtype
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def consts_of(side, dtype=torch.float64):
    return {k: v.to(dtype) for k, v in synthetic_mano_consts(side).items()}


def model(consts, p, side):
    """p [61] -> (verts [778, 3], joints [21, 3])"""
    v, j = mano_lbs(consts, p[None, :3], p[None, 3:48], p[None, 48:58], trans=p[None, 58:], side=side)
    return v[0], j[0]


def prior_vector(prior_pose, prior_shape, dtype):
    pr = torch.zeros(NP, dtype=dtype)
    pr[3:48], pr[48:58] = prior_pose, prior_shape
    return pr


def start_point(consts, target):
    p = torch.zeros(NP, dtype=target.dtype)
    p[58:] = target.mean(0) - consts['v_template'].mean(0)
    return p


def energy(consts, p, target, side, weight=None, prior_pose=0.0, prior_shape=0.0):
    with default_dtype(p.dtype):
        r = (model(consts, p, side)[0] - target).reshape(-1)
        w = torch.ones(NV, dtype=p.dtype) if weight is None else weight
        return float((w.repeat_interleave(3) * r * r).sum() + (prior_vector(prior_pose, prior_shape, p.dtype) * p * p).sum())


def system(consts, p, target, side, weight=None, prior_pose=0.0, prior_shape=0.0):
    """-> J [2334, 61], r [2334], w [2334], A [61, 61], g [61], E"""
    with default_dtype(p.dtype):
        f = lambda q: model(consts, q, side)[0].reshape(-1)
        J = torch.autograd.functional.jacobian(f, p, vectorize=True, strategy='forward-mode')   # 61 tangents; equal to reverse mode to 1e-16
        r = f(p) - target.reshape(-1)
        w = (torch.ones(NV, dtype=p.dtype) if weight is None else weight).repeat_interleave(3)
        pr = prior_vector(prior_pose, prior_shape, p.dtype)
        A = J.T @ (w[:, None] * J) + torch.diag(pr)
        g = J.T @ (w * r) + pr * p
        E = float((w * r * r).sum() + (pr * p * p).sum())
    return J, r, w, A, g, E


def damped(A, lam):
    return A + lam * torch.diag(torch.clamp(torch.diagonal(A), min=1e-12))


def fit(consts, target, side, weight=None, init=None, iters=20, prior_pose=0.0, prior_shape=0.0, valid=True):
    """The loop of the contract -> dict(p, cost0, cost, accepted, rejected, lam, A, g, costs: E after every trial step)."""
    dtype = target.dtype
    p = start_point(consts, target) if init is None else init.clone().to(dtype)
    kw = dict(weight=weight, prior_pose=prior_pose, prior_shape=prior_shape)
    if not valid:
        return dict(p=p, cost0=0.0, cost=0.0, accepted=0, rejected=0, lam=LAMBDA0, A=torch.zeros(NP, NP, dtype=dtype), g=torch.zeros(NP, dtype=dtype), costs=[])
    lam, acc, rej, costs = LAMBDA0, 0, 0, []
    E = E0 = energy(consts, p, target, side, **kw)
    A = g = None
    build = True
    for _ in range(iters):
        if build:
            _, _, _, A, g, _ = system(consts, p, target, side, **kw)
            build = False
        L, info = torch.linalg.cholesky_ex(damped(A, lam))
        ok = int(info) == 0
        if ok:
            delta = torch.cholesky_solve(-g[:, None], L)[:, 0]
            Et = energy(consts, p + delta, target, side, **kw)
            ok = Et < E
        if ok:
            p, E, lam, acc, build = p + delta, Et, max(lam / 4, 1e-7), acc + 1, True
        else:
            lam, rej = min(8 * lam, 1e6), rej + 1
        costs.append(E)
    if iters == 0:
        _, _, _, A, g, _ = system(consts, p, target, side, **kw)
    return dict(p=p, cost0=E0, cost=E, accepted=acc, rejected=rej, lam=lam, A=A, g=g, costs=costs)


def case(seed, pose_std, side='left', noise=0.0, dtype=torch.float64):
    """The issue's generating parameters -> (p_true [61], target [778, 3]) in float64, then cast."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    p = np.concatenate((g.normal(0, 0.5, 3), g.normal(0, pose_std, 45), g.normal(0, 1.0, 10), [0.03, -0.02, 0.5]))
    p = torch.from_numpy(p)
    with default_dtype(torch.float64):
        t = model(consts_of(side), p, side)[0]
    if noise > 0:
        t = t + torch.from_numpy(g.normal(0, noise, (NV, 3)))
    return p.to(dtype), t.to(dtype)


ALIAS_FLOOR_MM = 6e-6        # 2e-8 rad (the two axis-angles of one rotation, each turned by |a| + 1e-8) times a lever of at most 0.3 m


def same_or_alias(p, p_true):
    """Per joint (root first): the axis-angle is the generating one to 1e-6; it is the other axis-angle of the same rotation,
    a' = -(2 pi - |a|) a / |a| (opposite axes, lengths adding to 2 pi), to 1e-6."""
    a, b = p[:48].reshape(16, 3).double(), p_true[:48].reshape(16, 3).double()
    na, nb = a.norm(dim=1), b.norm(dim=1)
    same = (a - b).norm(dim=1) < 1e-6
    alias = ((na + nb - 2 * torch.pi).abs() < 1e-6) & ((a / na[:, None] + b / nb[:, None]).norm(dim=1) < 1e-6)
    return same, alias


def rms_mm(a, b):
    return float(((a.double() - b.double()) ** 2).sum(-1).mean().sqrt()) * 1000


def normalised_errors(J, r, w, A, g, A_test, g_test):
    """Largest |A_test - A| / S and |g_test - g| / s with S_ij = sum_k w_k |J_ki| |J_kj|, s_i = sum_k w_k |J_ki| |r_k| (all float64)."""
    Ja = J.abs()
    S = Ja.T @ (w[:, None] * Ja)
    s = Ja.T @ (w * r.abs())
    eA = ((A_test.double() - A).abs() / S.clamp(min=1e-300)).max()
    eg = ((g_test.double() - g).abs() / s.clamp(min=1e-300)).max()
    return float(eA), float(eg)
