"""Every body of the streaming kernels of csrc/elementwise.hip (3x3/s2 max-pool, bilinear x2 upsample, activations, pad2d, fused Adam) and
the centre decode of csrc/pointops.hip, each against a plain reference computed on the CPU.

Which body a case runs follows from the entry points' dispatch: max-pool takes the float4 forward and the gather backward when
C % 4 == 0 (torch's allocations are 16-byte aligned), else the scalar forward and the atomic backward; the upsample takes its float4
kernels when C % 4 == 0 and N * 2H < 65536, the scalar gather backward when N * H < 65536, else the memset + scatter; every grid-stride
loop has 2048 * 256 = 524,288 threads, so a case with more elements than that takes a second trip.  Tests that call the C ABI directly
fill the outputs with a sentinel first: a body that writes nothing, or writes into the padding of a row, shows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests.util import adam_float64

pytestmark = pytest.mark.gpu

CL = torch.channels_last
U = 2.0 ** -24                      # unit roundoff of float32
GRID = 2048 * 256                   # threads of a capped grid (grid_for, csrc/common.h)
S = 12345.0                         # sentinel
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pdfnet_amd import functional as F
    return F


def dev(t):
    return t.cuda()


def close(a, b, atol, rtol=1e-5, what=""):
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    assert err <= lim, "%s: max err %.3e > %.3e (max|ref|=%.3e)" % (what, err, lim, b.abs().max().item())


def within(a, ref, rel, floor, what):
    """elementwise |a - ref| <= rel * |ref| + floor"""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    assert torch.isfinite(a).all(), "%s: non-finite values" % what
    over = (a - ref).abs() / (rel * ref.abs() + floor)
    i = int(over.argmax())
    print("%s: worst error / bar = %.3f" % (what, over.flatten()[i].item()))
    assert over.flatten()[i] <= 1, "%s: element %d is %.9e, reference %.9e: %.2f times the bar" % (
        what, i, a.flatten()[i], ref.flatten()[i], over.flatten()[i])


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def padded(t, ld, fill=S):
    """[R][C] -> [R][ld] with the sentinel in columns [C, ld)"""
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ---------------------------------------------------------------------------------------------- max-pool
POOL_CASES = [(2, 3, 7, 6), (1, 5, 1, 5), (1, 1, 1, 1), (2, 6, 13, 14),          # scalar forward, atomic backward
              (2, 8, 7, 6), (1, 4, 2, 2), (1, 4, 1, 1),                            # float4 forward, gather backward
              (4, 6, 300, 300), (4, 24, 300, 300)]                                 # second trip: scalar, float4


def pool_input(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "levels":
        return torch.randint(0, 3, shape, generator=g).float()
    x = torch.randn(shape, generator=g)
    return x.relu() if kind == "relu" else x


def window_ties(x):
    """Of the 3x3/s2/p1 windows of x [N,C,H,W] that hold more than one in-bounds tap: (how many, the share in which two taps hold the same
    value, the share whose MAXIMUM is held by two taps).  The first sample stands for a large map."""
    x = x if x.numel() <= 1 << 20 else x[:1]
    N, C, H, W = x.shape
    taps = TF.unfold(TF.pad(x.reshape(N * C, 1, H, W), (1, 1, 1, 1), value=NAN), 3, stride=2)        # [NC][9][windows], NaN = padding
    can = (~taps.isnan()).sum(1) >= 2
    if not can.any():
        return 0, 0.0, 0.0
    s = taps.sort(1).values                                                                           # (NaN sorts last and equals nothing)
    equal = (s[:, 1:] == s[:, :-1]).any(1)
    top = (taps == taps.nan_to_num(nan=-INF).amax(1, keepdim=True)).sum(1) >= 2
    return int(can.sum()), equal[can].float().mean().item(), top[can].float().mean().item()


@pytest.mark.parametrize("kind", ["randn", "relu", "levels"])
@pytest.mark.parametrize("shape", POOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_every_body_against_float64(F, shape, kind):
    """F.maxpool3s2 against torch.max_pool2d in float64 (exact values, so its arg-max is the float32 one) and its autograd.  Inputs: randn;
    relu(randn), what the model pools (half of every window ties at 0); integers of {0, 1, 2}, where the maximum itself ties in most
    windows and the first one in row-major order must take the gradient.  Forward: exact.  Backward: an input element collects at most 4
    window gradients, i.e. 3 roundings of a partial sum of at most 4 max|dy| in any order: |dx - ref| <= 3 * 2^-24 * 4 * max|dy|.
    The tie shares are taken over the windows with more than one in-bounds tap (a 1x1 map has none, there is nothing to tie)."""
    x = pool_input(kind, shape, seed=sum(shape))
    n, equal, top = window_ties(x)
    if n and kind == "relu":
        assert equal >= 0.25, "only %.2f of the windows tie" % equal
    if n and kind == "levels":
        assert top >= 0.25, "the maximum ties in only %.2f of the windows" % top
    xr = x.double().requires_grad_()
    ref = TF.max_pool2d(xr, 3, 2, 1)
    gy = rnd(*ref.shape, seed=2)
    ref.backward(gy.double())
    xd = dev(x).requires_grad_()
    out = F.maxpool3s2(xd)
    out.backward(dev(gy))
    assert out.shape == ref.shape
    assert torch.equal(out.detach().cpu().double(), ref.detach()), "maxpool forward"
    err = (xd.grad.cpu().double() - xr.grad).abs().max().item()
    bar = 3 * U * 4 * gy.abs().max().item()
    print("maxpool dx: max err %.3e, bar %.3e" % (err, bar))
    assert err <= bar, "maxpool dx: max err %.3e > %.3e" % (err, bar)


@pytest.mark.parametrize("C", [8, 3])
def test_maxpool_skip_adds_the_pool_gradient_onto_the_other_consumers(F, C, monkeypatch):
    """y, a = F.maxpool3s2(x, skip=True) under the loss (y * gy).sum() + (a * ga).sum(): dx = float64 pool gradient + ga, through
    pdf_maxpool3s2_bwd_add (counted: the gather body with accumulate at C = 8, the atomic body onto the filled tensor at C = 3).
    One term more than the plain backward: 4 roundings of a partial sum of at most 5 max(|gy|, |ga|)."""
    x = rnd(2, C, 13, 14, seed=C).relu()
    xr = x.double().requires_grad_()
    ref = TF.max_pool2d(xr, 3, 2, 1)
    gy, ga = rnd(*ref.shape, seed=5), rnd(*x.shape, seed=6)
    ref.backward(gy.double())
    want = xr.grad + ga.double()
    L, calls = F._L(), []
    add = L.pdf_maxpool3s2_bwd_add
    monkeypatch.setattr(L, "pdf_maxpool3s2_bwd_add", lambda *a: calls.append(1) or add(*a))
    xd = dev(x).contiguous(memory_format=CL).requires_grad_()
    y, a = F.maxpool3s2(xd, skip=True)
    torch.autograd.backward([y, a], [dev(gy).contiguous(memory_format=CL), dev(ga).contiguous(memory_format=CL)])
    torch.cuda.synchronize()
    assert calls == [1], "the skip gradient did not go through pdf_maxpool3s2_bwd_add"
    assert torch.equal(y.detach().cpu().double(), ref.detach()) and torch.equal(a.detach().cpu(), x)
    err = (xd.grad.cpu().double() - want).abs().max().item()
    bar = 4 * U * 5 * max(gy.abs().max().item(), ga.abs().max().item())
    print("maxpool skip dx: max err %.3e, bar %.3e" % (err, bar))
    assert err <= bar, "maxpool skip dx: max err %.3e > %.3e" % (err, bar)


def nonfinite_map(name, C):
    """NHWC maps whose windows have no finite maximum, or a NaN"""
    if name == "all -inf":
        return torch.full((2, 4, 4, C), -INF)
    if name == "one NaN":                                     # one per channel: also the leading in-bounds tap of the first window
        x = rnd(1, 5, 5, C, seed=11)
        for c, (iy, ix) in enumerate([(0, 0), (1, 1), (4, 4), (2, 3)][:C]):
            x[0, iy, ix, c] = NAN
        return x
    x = rnd(1, 5, 6, C, seed=12)                              # "-inf border": first row and column
    x[:, 0] = -INF
    x[:, :, 0] = -INF
    return x


@pytest.mark.parametrize("name", ["all -inf", "one NaN", "-inf border"])
@pytest.mark.parametrize("C", [4, 3])
def test_maxpool_argmax_stays_in_bounds_on_non_finite_maps(F, C, name):
    """pdf_maxpool3s2_fwd on maps where no comparison `v > best` succeeds for some window.  arg is read back and every tap it names must lie
    inside the image BEFORE the backward, which indexes dx with it, is launched; y equals torch.max_pool2d, NaN included; with dy of small
    integers no gradient may be lost (dx.sum() == dy.sum() exactly) and dx is ATen's (same scan: first in-bounds tap, then `>` or NaN)."""
    from pdfnet_amd import hip
    L = hip.lib()
    x = nonfinite_map(name, C)
    N, H, W, _ = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xr = x.permute(0, 3, 1, 2).double().requires_grad_()
    ref = TF.max_pool2d(xr, 3, 2, 1)
    dy = torch.randint(1, 6, (N, OH, OW, C), generator=torch.Generator().manual_seed(3)).float()
    ref.backward(dy.permute(0, 3, 1, 2).double())
    ref = ref.detach().permute(0, 2, 3, 1)
    xd, yd = dev(x), dev(torch.full((N, OH, OW, C), S))
    ad = dev(torch.full((N * OH * OW * C,), 255, dtype=torch.uint8))
    L.pdf_maxpool3s2_fwd(hip.ptr(xd), N, H, W, C, hip.ptr(yd), hip.ptr(ad), hip.stream())
    arg = ad.cpu().reshape(N, OH, OW, C).long()
    assert (arg < 9).all(), "arg not written"
    iy = torch.arange(OH).view(1, OH, 1, 1) * 2 - 1 + arg // 3
    ix = torch.arange(OW).view(1, 1, OW, 1) * 2 - 1 + arg % 3
    assert (iy >= 0).all() and (iy < H).all() and (ix >= 0).all() and (ix < W).all(), "arg names a tap outside the image"
    y = yd.cpu().double()
    assert torch.equal(y.isnan(), ref.isnan()) and torch.equal(y[~ref.isnan()], ref[~ref.isnan()]), "maxpool forward"
    if name == "one NaN":
        assert ref.isnan().any()
    # (the atomic body needs a zero-filled dx, the gather body writes every element)
    dyd, dxd = dev(dy), dev(torch.zeros(N, H, W, C) if C % 4 else torch.full((N, H, W, C), S))
    L.pdf_maxpool3s2_bwd(hip.ptr(dyd), hip.ptr(ad), N, H, W, C, hip.ptr(dxd), hip.stream())
    dx = dxd.cpu().double()
    assert dx.sum().item() == dy.sum().item(), "gradient lost: dx sums to %r, dy to %r" % (dx.sum().item(), dy.sum().item())
    assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1)), "maxpool dx"


# ---------------------------------------------------------------------------------------------- upsample
UP_CASES = [(2, 4, 1, 1), (2, 4, 1, 5), (2, 4, 3, 1), (2, 4, 2, 2), (2, 3, 2, 2), (2, 3, 1, 1),      # degenerate axes
            (40000, 4, 1, 1),            # N * 2H >= 65536: scalar forward at C % 4 == 0, scalar gather backward
            (65536, 4, 1, 2),            # N * H >= 65536: memset + scatter backward
            (2, 3, 160, 160)]            # 614,400 outputs: second trip through up2_fwd_kernel


@pytest.mark.parametrize("shape", UP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_upsample2x_every_body_against_aten(F, shape):
    """F.upsample2x against ATen's fp32 CPU interpolate(align_corners=True) and its backward (the source coordinate is defined in float32,
    so ATen fp32 is the specification), at the bars of test_ops_gpu.  The kernel gets an `empty` dx: before the backward the allocator's
    free blocks of that size are filled with NaN, so a scatter body that does not clear dx first cannot pass by finding fresh zeros."""
    x = rnd(*shape, seed=sum(shape) % 1000)
    xr = x.clone().requires_grad_()
    ref = TF.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=True)
    gy = rnd(*ref.shape, seed=3)
    ref.backward(gy)
    xd = dev(x).requires_grad_()
    out = F.upsample2x(xd)
    gd = dev(gy).contiguous(memory_format=CL)
    poison = [torch.full(shape, NAN, device="cuda") for _ in range(3)]
    del poison
    out.backward(gd)
    close(out, ref, 2e-6, what="upsample")
    close(xd.grad, xr.grad, 1e-5, what="upsample dx")


# ---------------------------------------------------------------------------------------------- activations
def planted(R, C, seed):
    x = rnd(R, C, seed=seed)
    for k, v in enumerate([0.0, -0.0, 1e-38, -1e-38, INF, -INF]):
        x.view(-1)[7 * k + 1] = v
        x.view(-1)[R * C - 7 * k - 2] = v
    return x


@pytest.mark.parametrize("R", [37, 105000])
@pytest.mark.parametrize("act", [1, 2])
def test_activation_on_strided_rows(F, act, R):
    """pdf_act_fwd / pdf_act_bwd (1 relu, 2 leaky 0.1) on rows of C = 5 at strides that differ between every operand (x 8, y 12, dy 16, dx 8);
    R * C = 525,000 takes the second trip.  Zeros of both signs, subnormals (+-1e-38) and infinities are planted.  ReLU forward: exact.
    Leaky forward: within 2^-22 relative of 0.1 * v in float64 (0.1f against 0.1 is 1.5e-8 relative, plus one rounding) -- plus one
    subnormal spacing, 2^-149, which is all a float32 result below 2^-126 can resolve (0.1f * -1e-38); an infinity stays one.  Both
    backwards: exact against the float32 expression on the CPU (the kernel reads the sign of y).  Columns [C, ld) keep the sentinel."""
    from pdfnet_amd import hip
    L = hip.lib()
    C, ldx, ldy, ldg = 5, 8, 12, 16
    assert R * C > 36 and (R < 100 or R * C > GRID)
    x, g = planted(R, C, seed=act), rnd(R, C, seed=9)
    xd, yd = dev(padded(x, ldx)), dev(torch.full((R, ldy), S))
    L.pdf_act_fwd(hip.ptr(xd), ldx, hip.ptr(yd), ldy, C, R, act, hip.stream())
    y = yd.cpu()
    assert (y[:, C:] == S).all(), "act forward wrote into the row padding"
    y = y[:, :C]
    if act == 1:
        assert torch.equal(y, x.clamp_min(0)), "relu forward"
    else:
        pos, fin = x > 0, torch.isfinite(x)
        assert torch.equal(y[pos], x[pos]) and torch.equal(y[~fin], x[~fin]), "leaky forward, positive / infinite inputs"
        want = 0.1 * x[~pos & fin].double()
        err = (y[~pos & fin].double() - want).abs()
        assert (err <= 2.0 ** -22 * want.abs() + 2.0 ** -149).all(), "leaky forward: worst %.3e relative" % (err / want.abs().clamp_min(1e-45)).max().item()
    gd, dxd = dev(padded(g, ldg)), dev(torch.full((R, ldx), S))
    L.pdf_act_bwd(hip.ptr(gd), ldg, hip.ptr(yd), ldy, hip.ptr(dxd), ldx, C, R, act, hip.stream())
    dx = dxd.cpu()
    assert (dx[:, C:] == S).all(), "act backward wrote into the row padding"
    want = torch.where(x > 0, g, torch.zeros_like(g) if act == 1 else g * torch.tensor(0.1, dtype=torch.float32))
    assert torch.equal(dx[:, :C], want), "act backward"
    assert torch.equal(xd.cpu(), padded(x, ldx)), "act forward changed its input"


# ---------------------------------------------------------------------------------------------- pad2d
def test_pad2d_takes_a_second_trip_padding_and_cropping(F):
    """pdf_pad2d (600, 900) -> (608, 912) and the crop back, 554,496 and 540,000 destination elements, at row strides wider than the
    rows: exact against torch.nn.functional.pad and the slice, the row padding keeps the sentinel."""
    from pdfnet_amd import hip
    L = hip.lib()
    R, C, R2, C2 = 600, 900, 608, 912
    assert R * C > GRID and R2 * C2 > GRID
    small, big = rnd(R, C, seed=1), rnd(R2, C2, seed=2)
    for src, (r, c, lds), (r2, c2, ldd), want in ((small, (R, C, 904), (R2, C2, 920), TF.pad(small, (0, C2 - C, 0, R2 - R))),
                                                  (big, (R2, C2, 920), (R, C, 904), big[:R, :C])):
        sd, dd = dev(padded(src, lds)), dev(torch.full((r2, ldd), S))
        L.pdf_pad2d(hip.ptr(sd), lds, r, c, hip.ptr(dd), ldd, r2, c2, hip.stream())
        d = dd.cpu()
        assert torch.equal(d[:, :c2], want), "pad2d %s -> %s" % ((r, c), (r2, c2))
        assert (d[:, c2:] == S).all(), "pad2d wrote into the row padding"


# ---------------------------------------------------------------------------------------------- Adam
ADAM = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)
ADAM_STEPS = 5
ADAM_LAYOUTS = {"ragged": (0, 4099, 4160),                   # n = 4099: a ragged tail
                "offset": (3, 4099, 4160),                   # [3, 4099) of a larger buffer: pointers only 4-byte aligned
                "second-trip": (0, 600001, 600064)}          # n = 600,001 > 524,288


def adam_run(p0, grads, corrs, lo, size, grad_scale):
    """pdf_adam_step over [lo, lo + n) of sentinel-filled buffers of `size` floats -> (p, m, v) of the range; everything outside it must be
    bit-unchanged."""
    from pdfnet_amd import hip
    L = hip.lib()
    n = p0.numel()

    def buf(t):
        b = torch.full((size,), S)
        b[lo:lo + n] = t
        return dev(b)
    pd, md, vd = buf(p0), buf(torch.zeros(n)), buf(torch.zeros(n))
    for g, c in zip(grads, corrs):
        gd, cd = buf(g), dev(c)
        L.pdf_adam_step(hip.ptr_at(pd, lo), hip.ptr_at(gd, lo), hip.ptr_at(md, lo), hip.ptr_at(vd, lo), n,
                        ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], hip.ptr(cd), grad_scale, hip.stream())
    out = []
    for name, t in (("p", pd), ("m", md), ("v", vd)):
        t = t.cpu()
        outside = torch.cat((t[:lo], t[lo + n:]))
        assert torch.equal(outside.view(torch.int32), torch.full_like(outside, S).view(torch.int32)), "adam wrote %s outside [lo, hi)" % name
        out.append(t[lo:lo + n])
    return out


def adam_inputs(n, kind):
    g = rnd(n, seed=2) * (1e-9 if kind == "tiny" else 1.0)
    g[100:200] = 0.0                                         # a block of exact zeros
    grads = [g * t for t in range(1, ADAM_STEPS + 1)]        # float32, what the kernel is given
    corrs = [torch.tensor([1 - ADAM["b1"] ** t, 1 - ADAM["b2"] ** t], dtype=torch.float32) for t in range(1, ADAM_STEPS + 1)]
    return grads, corrs


ADAM_REL, ADAM_FLOOR = 2.0 ** -18, 1e-30


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("kind", ["randn", "tiny"])
@pytest.mark.parametrize("layout", list(ADAM_LAYOUTS))
def test_adam_step_against_float64(F, layout, kind, grad_scale):
    """pdf_adam_step, 5 steps with g_t = t * g, against textbook Adam in float64 fed the kernel's own float32 inputs (tests.util.adam_float64).
    Gradients: randn, or randn * 1e-9 so that sqrt(v) is of the size of eps; 100 of them exactly 0, whose update must be exactly 0.
    grad_scale 0.125 is the multi-chip averaging of FlatAdam.apply.
      * from p0 = 0 the displacement is the update: p, m and v elementwise within 2^-18 relative (3.8e-6) + 1e-30.  The update has about 6
        float32 roundings, this is an order above; a 1 % error in any factor exceeds it more than 2,000-fold.
      * from p0 = randn: |p - ref| <= steps * 2^-24 * max|p| (one rounding of p per step) + the bar above on the displacement.
      * torch.optim.Adam in float64 with double constants: the displacement from p0 = 0 within 2e-5 relative (float32 constants alone shift
        v by 1.3e-5 and the displacement by 6.6e-6 on the CPU; three times that)."""
    lo, hi, size = ADAM_LAYOUTS[layout]
    n = hi - lo
    grads, corrs = adam_inputs(n, kind)
    zero = torch.zeros(n)
    pr, mr, vr = adam_float64(zero, grads, corrs, grad_scale=grad_scale, **ADAM)
    p, m, v = adam_run(zero, grads, corrs, lo, size, grad_scale)
    for name, a, r in (("p", p, pr), ("m", m, mr), ("v", v, vr)):
        within(a, r, ADAM_REL, ADAM_FLOOR, "adam %s from p0 = 0" % name)
        assert (a[100:200] == 0).all(), "adam %s: a zero gradient moved it" % name
    assert (p[:100] != 0).all() and (p[200:] != 0).any()
    # torch.optim.Adam semantics, all constants double
    pt = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    for g in grads:
        pt.grad = g.double() * grad_scale
        opt.step()
    within(p, pt, 2e-5, ADAM_FLOOR, "adam p against torch.optim.Adam")
    # from a random start
    p0 = rnd(n, seed=1)
    pr1, _, _ = adam_float64(p0, grads, corrs, grad_scale=grad_scale, **ADAM)
    p1, m1, v1 = adam_run(p0, grads, corrs, lo, size, grad_scale)
    assert torch.equal(m1, m) and torch.equal(v1, v)
    assert torch.equal(p1[100:200], p0[100:200]), "adam p: a zero gradient moved it"
    bar = ADAM_STEPS * U * pr1.abs().max().item() + ADAM_REL * (pr1 - p0.double()).abs() + ADAM_FLOOR
    err = (p1.double() - pr1).abs()
    print("adam p from p0 = randn: worst error / bar = %.3f" % (err / bar).max().item())
    assert (err <= bar).all(), "adam p from p0 = randn: %.2f times the bar" % (err / bar).max().item()


# ---------------------------------------------------------------------------------------------- centre decode
@pytest.mark.parametrize("H,W", [(7, 5), (24, 20)])
def test_nms_top1_index_stays_inside_the_map(F, H, W):
    """F.nms_top1 on maps where comparisons tie or fail: whatever the map holds, 0 <= ind < H * W (ind feeds the evaluation path's row gathers).
    A NaN never wins; a map of NaN alone gives index 0.  Ties go to the lowest index: 0 on a constant map, the first cell of a 3x3 plateau
    of equal maxima.  On finite maps score == hm[ind].  (7, 5) fits one trip of the block's 256 threads, (24, 20) takes two."""
    base = rnd(H, W, seed=H)
    one_nan = base.clone()
    one_nan[H // 2, W // 2] = NAN
    plateau = base * 0.1
    plateau[2:5, 1:4] = 3.0
    maps = torch.stack([torch.full((H, W), NAN), one_nan, torch.full((H, W), -INF), torch.full((H, W), 0.25), plateau])[None]
    ind, score = F.nms_top1(dev(maps))
    ind, score = ind.cpu()[0], score.cpu()[0]
    assert ((ind >= 0) & (ind < H * W)).all(), "index outside the map: %s" % ind.tolist()
    assert ind[0] == 0 and score[0].isnan()
    assert not one_nan.flatten()[ind[1]].isnan() and score[1] == one_nan.flatten()[ind[1]]
    assert ind[2] == 0 and score[2] == -INF
    assert ind[3] == 0 and score[3] == 0.25
    assert ind[4] == 2 * W + 1 and score[4] == 3.0
    for k in (3, 4):
        assert score[k] == maps[0, k].flatten()[ind[k]]
    # the one-NaN map decodes like the same map with the NaN cell removed from the contest
    no_nan = one_nan.clone()
    no_nan[H // 2, W // 2] = -INF
    ind2, score2 = F.nms_top1(dev(no_nan[None, None]))
    assert ind2.item() == ind[1].item() and score2.item() == score[1].item()
