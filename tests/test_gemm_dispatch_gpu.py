"""Which GEMM-family kernel every parity case runs, and that kernel against float64.

The host picks between some 25 kernels of csrc/gemm.hip, gemm_x3.hip and winograd.hip by shape thresholds (launch_igemm, launch_wgemm,
wino_plan / wino_wgrad_plan of csrc/winograd.hip, the streaming and stem special cases).  A test that only chooses a shape "for" a kernel goes on
passing when a threshold or a default moves the shape to another kernel.  Every row here therefore states the kernel records
(tests/util.py kernels_run: the names the sources give to KTimer) it expects of its forward and of its backward, in launch order and
in full -- so no other GEMM-family kernel can stand in -- and, for 3x3 stride-1 convolutions, which of the three launches take the
Winograd path (pdf_conv2d_winograd_workspace_floats > 0: forward, backward-data, weight gradient).  Output and all gradients are
compared with a float64 CPU evaluation at the bars of tests/test_ops_gpu.py (test_linear, test_conv2d, test_deconv2d).

Each shape is the smallest that still selects its kernel; the rule it sits on is quoted beside it.  Every row is compared in full: no
row's float64 reference needs the subset form (more than about 10 s on 16 threads).  Measured forward + backward on 16 threads: halo-w64-fwd 1.4 s,
halo-w64-bwd 0.8 s, the other halo-* and tile128-taps-* rows 0.5-0.6 s, every other row of the table less (on 8 threads: halo-w64-fwd
4.4 s, the x3 Winograd case at 8 images 1.7 s, deconv-x3 at 7 images 1.1 s); every row prints its own figure."""
import functools
import time

import pytest
import torch
import torch.nn.functional as TF

from tests.util import kernels_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pdfnet_amd import functional as F
    return F


def dev(t):
    return t.cuda()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def err_of(a, b):
    """-> (max |a - b|, rms of a - b), b the float64 reference."""
    d = a.detach().cpu().double() - b
    return d.abs().max().item(), d.pow(2).mean().sqrt().item()


def check(report, what, a, b, atol, rtol):
    """Notes `what`'s error and bar in `report` (printed before anything is asserted) -> the bar's violation message or None."""
    err = err_of(a, b)[0]
    lim = atol + rtol * b.abs().max().item()
    report.append("    %-10s max err %.3e  bar %.3e" % (what, err, lim))
    return None if err <= lim else "%s: max err %.3e > %.3e (max|ref|=%.3e)" % (what, err, lim, b.abs().max().item())


def ig(BM, BN, WM, WN, fast, b_kn, BK, buf):
    t = lambda v: "true" if v else "false"
    return "igemm_nt<%d, %d, %d, %d, %s, %s, %d, %s>" % (BM, BN, WM, WN, t(fast), t(b_kn), BK, t(buf))


# the names that occur below
IG128, IG128_KN = ig(128, 128, 2, 2, 1, 0, 16, 1), ig(128, 128, 2, 2, 1, 1, 16, 1)            # plain / with taps, [N][K] and [K][N] weights
IG128x64, IG128x64_KN, IG128x64_SLOW_KN = ig(128, 64, 4, 1, 1, 0, 16, 1), ig(128, 64, 4, 1, 1, 1, 16, 1), ig(128, 64, 4, 1, 0, 1, 16, 0)
IG64_32, IG64_32_KN = ig(64, 64, 2, 2, 1, 0, 32, 1), ig(64, 64, 2, 2, 1, 1, 32, 1)
IG64_16, IG64_16_KN = ig(64, 64, 2, 2, 1, 0, 16, 1), ig(64, 64, 2, 2, 1, 1, 16, 1)
IG64_SLOW, IG64_SLOW_KN = ig(64, 64, 2, 2, 0, 0, 16, 0), ig(64, 64, 2, 2, 0, 1, 16, 0)
IG32 = ig(32, 32, 1, 1, 1, 0, 16, 1)
HALO, HALO_KN = "igemm_halo3x3<false, true>", "igemm_halo3x3<true, true>"
WG_DMA, WG64, WG64_SLOW = "wgemm_tn_dma<3, true>", "wgemm_tn<64, 64, 2, 2, true, 32, true>", "wgemm_tn<64, 64, 2, 2, false, 16, false>"
RS, RS2D, SKF = "reduce_slabs", "reduce_slabs_2d", "splitk_finish"
X3NT_WIDE, X3NT, X3TN_WIDE = "x3gemm_nt<4, 2, 2, 2, 2, 6>", "x3gemm_nt<2, 4, 2, 1, 3, 6>", "x3gemm_tn<4, 2, 2, 2, 2, 6>"
X3NT_TAPS, X3TN_TAPS = "x3gemm_nt<2, 4, 2, 1, 3, 6, true>", "x3gemm_tn<2, 4, 2, 1, 3, 6, true>"          # implicit operand: the transposed convolutions
X3_ROWS, X3_TR, X3_RED = "x3_split_rows_kernel", "x3_split_transpose_kernel", "x3_slab_reduce_kernel"


# ---------------------------------------------------------------------------------------------- float64 references (computed once per shape)
@functools.lru_cache(maxsize=2)
def conv_case(cfg):
    """Inputs as in test_conv2d (seeded, weight scaled by fan_in ** -0.5) and the float64 evaluation of conv (+ bias, + ReLU).  With an
    activation, the output gradient is zeroed where the float64 pre-activation lies within the forward bar of zero: there the two
    implementations may legitimately disagree about the mask, and the gradients are ReLU-dependent.  -> dict."""
    N, Cin, H, W, Cout, k, s, p, act, bias = cfg
    x = rnd(N, Cin, H, W, seed=1)
    w = rnd(Cout, Cin, k, k, seed=2, scale=(Cin * k * k) ** -0.5)
    b = rnd(Cout, seed=3) if bias else None
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    pre = TF.conv2d(xr, wr, br, s, p)
    gy = rnd(*pre.shape, seed=4)
    share = 0.0
    if act:
        near = pre.detach().abs() <= conv_bars(cfg)['fwd'][0]
        share = near.double().mean().item()
        gy[near] = 0.0
    ref = TF.relu(pre) if act else pre
    ref.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, out=ref.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else None, share=share)


def conv_bars(cfg):
    """The bars of test_conv2d: (atol, rtol) of the output and of each gradient."""
    N, Cin, H, W, Cout, k, s, p, act, bias = cfg
    K = Cin * k * k
    return {'fwd': (3e-5 * max(1, K ** 0.5 / 16), 1e-5), 'dx': (1e-4, 2e-5), 'dw': (5e-5 * max(1, (N * H * W) ** 0.5 / 16), 5e-5), 'db': (1e-4, 5e-5)}


@functools.lru_cache(maxsize=2)
def linear_case(cfg):
    M, K, N, act, bias = cfg
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3) if bias else None
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    pre = TF.linear(xr, wr, br)
    gy = rnd(M, N, seed=4)
    share = 0.0
    if act:
        near = pre.detach().abs() <= linear_bars(cfg)['fwd'][0]
        share = near.double().mean().item()
        gy[near] = 0.0
    ref = TF.relu(pre) if act == 1 else (TF.leaky_relu(pre, 0.1) if act == 2 else pre)
    ref.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, out=ref.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else None, share=share)


def linear_bars(cfg):
    """The bars of test_linear."""
    M, K, N, act, bias = cfg
    tol = 2e-5 * max(1.0, K ** 0.5 / 8)
    return {'fwd': (tol, 1e-5), 'dx': (tol * 4, 1e-5), 'dw': (2e-5 * max(1.0, M ** 0.5 / 4), 2e-5), 'db': (2e-5 * max(1.0, M ** 0.5 / 4), 2e-5)}


@functools.lru_cache(maxsize=2)
def deconv_case(cfg):
    N, Cin, H, W, Cout, k, s, p = cfg
    x = rnd(N, Cin, H, W, seed=1)
    w = rnd(Cin, Cout, k, k, seed=2, scale=Cin ** -0.5)
    b = rnd(Cout, seed=3)
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    ref = TF.conv_transpose2d(xr, wr, br, s, p)
    gy = rnd(*ref.shape, seed=4)
    ref.backward(gy.double())
    return dict(x=x, w=w, b=b, gy=gy, out=ref.detach(), dx=xr.grad, dw=wr.grad, db=br.grad, share=0.0)


DECONV_BARS = {'fwd': (5e-5, 1e-5), 'dx': (2e-4, 2e-5), 'dw': (2e-4, 5e-5), 'db': (2e-4, 5e-5)}      # test_deconv2d


# ---------------------------------------------------------------------------------------------- the table
def row(id, op, cfg, fwd, bwd, wino=None, grad=True, x3=None):
    """op: 'conv' (N, Cin, H, W, Cout, k, stride, pad, act, bias) / 'linear' (M, K, N, act, bias) / 'deconv' (N, Cin, H, W, Cout, k, stride, pad).
    fwd / bwd: the records expected of the forward and of the backward (backward-data launches, then the weight gradient's), complete
    and in order.  wino: None = F.WINOGRAD off; else the (forward, backward-data, weight gradient) launches that must be Winograd ones,
    with F.WINOGRAD on.  grad=False: under torch.no_grad().  x3: argument of F.set_x3 (None: the default, everything on)."""
    return pytest.param(dict(op=op, cfg=cfg, fwd=fwd, bwd=bwd, wino=wino, grad=grad, x3=x3), id=id)


ROWS = [
    # --- igemm_halo3x3 (launch_igemm: 3x3 stride 1, W in {64, 32, 16}, M % 128 == 0, N > 64, Cin >= 256, >= 600 128x128 tiles).  20,480 rows
    # x 512 columns = 640 tiles is the smallest; with 256 columns on the other side that pass has 320 tiles and runs the 64x64 kernel, so
    # the forward (Cout = 512) and the backward-data (Cin = 512) kernel have a row each per map width.
    row("halo-w64-fwd", 'conv', (5, 256, 64, 64, 512, 3, 1, 1, 0, True), [HALO], [IG64_32_KN, WG_DMA, RS]),
    # ... and as production reaches it: Winograd on, but a forward nothing is differentiated through gets no workspace
    row("halo-w64-fwd-no-grad-winograd-on", 'conv', (5, 256, 64, 64, 512, 3, 1, 1, 0, True), [HALO], [], wino=(False, False, False), grad=False),
    row("halo-w64-bwd", 'conv', (5, 512, 64, 64, 256, 3, 1, 1, 0, False), [IG64_32], [HALO_KN, WG_DMA, RS]),
    row("halo-w32-fwd", 'conv', (20, 256, 32, 32, 512, 3, 1, 1, 0, False), [HALO], [IG64_32_KN, WG_DMA, RS]),
    row("halo-w32-bwd", 'conv', (20, 512, 32, 32, 256, 3, 1, 1, 0, True), [IG64_32], [HALO_KN, WG_DMA, RS]),
    row("halo-w16-fwd", 'conv', (80, 256, 16, 16, 512, 3, 1, 1, 0, True), [HALO], [IG64_32_KN, WG_DMA, RS]),
    row("halo-w16-bwd", 'conv', (80, 512, 16, 16, 256, 3, 1, 1, 0, False), [IG64_32], [HALO_KN, WG_DMA, RS]),
    # --- igemm_nt<128, 128> with taps: >= 600 tiles, fewer than PDF_IG_HALO_MINC = 256 channels under the reduction.  Forward (Cin = 128),
    # with a ragged last column tile (Cout = 264; 264 % 16 != 0 channels under the backward-data's reduction make that pass the
    # per-element 64x64 form), and the [K][N] form of the backward-data (Cout = 128 under the reduction)
    row("tile128-taps-fwd", 'conv', (10, 128, 64, 64, 256, 3, 1, 1, 0, True), [IG128], [IG64_32_KN, WG_DMA, RS2D]),
    row("tile128-taps-fwd-ragged-n", 'conv', (10, 128, 64, 64, 264, 3, 1, 1, 0, False), [IG128], [IG64_SLOW_KN, WG_DMA, RS2D]),
    row("tile128-taps-bwd", 'conv', (10, 256, 64, 64, 128, 3, 1, 1, 0, False), [IG64_32], [IG128_KN, WG_DMA, RS2D]),
    # --- igemm_nt<128, 128> plain: N > 64, >= 600 tiles and not short_k (K > 512 at M <= 262,144): 300 x 2 tiles, K = 528.  The
    # backward-data (K = 256: short_k) runs the 64x64 kernel; N = 250 makes dy's rows unaligned: per-element forms there and in the weight gradient
    row("tile128-linear", 'linear', (38400, 528, 256, 0, True), [IG128], [IG64_32_KN, WG_DMA, RS2D]),
    row("tile128-linear-n250", 'linear', (38400, 528, 250, 0, True), [IG128], [IG64_SLOW_KN, "wgemm_tn<128, 128, 2, 2, false, 16>", RS2D]),
    # --- igemm_nt<128, 64, 4, 1>: N <= 64 and >= 600 row blocks of 128: M = 76,801 (601 blocks, the last of one row)
    row("tile128x64-linear", 'linear', (76801, 64, 64, 0, True), [IG128x64], [IG128x64_KN, WG64, RS2D]),
    row("tile128x64-linear-n40", 'linear', (76801, 64, 40, 0, False), [IG128x64], ["small_k_gemm", WG64, RS2D]),
    # --- igemm_nt<64, 64>: K-step 32 (Cin % 32 == 0) and 16 (Cin = 48)
    row("tile64-k32", 'linear', (2016, 256, 256, 0, True), [IG64_32], [IG64_32_KN, WG64, RS2D]),
    row("tile64-k16", 'linear', (2016, 48, 256, 0, True), [IG64_16], [IG64_32_KN, WG64, RS2D]),
    # --- few 64x64 tiles under K >= 512: split-K takes every plain launch (splitk_finish behind the partial tiles) and every tap-walking
    # one whose reduction channels are a multiple of 32 (this row's backward-data: 64); the forward's 80 are not, so it is not split and
    # runs the one-wave 32x32 tile
    row("split-k", 'linear', (64, 1024, 1024, 0, True), [IG64_32, SKF], [IG64_32_KN, SKF, WG_DMA]),
    row("tile32", 'conv', (2, 80, 4, 4, 64, 3, 1, 1, 0, False), [IG32], [IG64_32_KN, SKF, WG64]),
    # --- small_k_gemm: rows not 16-byte aligned (K = 42), K <= 48, >= 2^20 outputs
    row("small-k", 'linear', (33000, 42, 130, 2, True), ["small_k_gemm"], [IG64_SLOW_KN, WG64_SLOW, RS2D]),
    # --- wgemm_tn_dma<3, true> (launch_wgemm: not `small`, i.e. NI x NJ > 2^18 here), Cq = 128, and its three issue forms (WGemm::uniform,
    # gemm.hip launch_wgemm: 2 = scalar offsets, QW % 16 == 0; 1 = per row, QW % 8 == 0; 0 = per lane): a 64-wide map (2), a 48-wide one
    # whose 16-pixel K-steps wrap every third step (2), stride 2 (2), a 40-wide map (1), a 36-wide map (0) and Cq = 144 (0).  The form is not
    # part of the record's name, so these rows select it by shape under the rule quoted here and do NOT assert it: a change of that rule
    # moves a row to another form with the record unchanged.  (Two images: the backward-data and some forwards are split over K.)
    row("wgrad-dma-w64", 'conv', (2, 128, 64, 64, 256, 3, 1, 1, 0, False), [IG64_32], [IG64_32_KN, SKF, WG_DMA, RS2D]),
    row("wgrad-dma-w48-wraps", 'conv', (2, 128, 48, 48, 256, 3, 1, 1, 0, False), [IG64_32], [IG64_32_KN, SKF, WG_DMA, RS2D]),
    row("wgrad-dma-stride2", 'conv', (4, 128, 64, 64, 256, 3, 2, 1, 0, False), [IG64_32, SKF], [IG64_32_KN] * 4 + [WG_DMA, RS2D]),
    row("wgrad-dma-w40-per-row", 'conv', (2, 128, 40, 40, 256, 3, 1, 1, 0, False), [IG64_32, SKF], [IG64_32_KN, SKF, WG_DMA, RS]),
    row("wgrad-dma-w36-per-lane", 'conv', (2, 128, 36, 36, 256, 3, 1, 1, 0, False), [IG64_32, SKF], [IG64_32_KN, SKF, WG_DMA, RS]),
    row("wgrad-dma-c144-per-lane", 'conv', (2, 144, 32, 32, 256, 3, 1, 1, 0, False), [IG64_16], [IG64_32_KN, SKF, WG_DMA, RS]),
    # --- wgemm_tn<64, 64>: a narrow side (NI = 64), and the per-element form (Cin = 6), whose forward and backward-data are per-element too
    row("wgrad-64", 'conv', (2, 64, 16, 16, 64, 3, 1, 1, 0, False), [IG64_32, SKF], [IG64_32_KN, SKF, WG64, RS]),
    row("wgrad-64-unaligned", 'conv', (2, 6, 9, 9, 20, 3, 1, 1, 1, True), [IG64_SLOW], [IG64_SLOW_KN, WG64_SLOW]),
    # --- the streaming and stem kernels, at their shapes in test_conv2d (the 3 -> 3 layer has no backward-data kernel of its own: the
    # per-element 128x64 tile)
    row("narrow-wgrad", 'conv', (2, 256, 64, 64, 2, 1, 1, 0, 0, True), [IG64_32], ["small_k_gemm", "narrow_wgrad_kernel + reduce_slabs_2d"]),
    row("stem7x7", 'conv', (3, 3, 128, 128, 64, 7, 2, 3, 0, False), ["stem7x7_fwd_kernel"], [IG64_SLOW_KN] * 4 + ["stem7x7_wgrad_kernel + reduce_slabs_2d"]),
    row("tiny-conv", 'conv', (2, 3, 192, 200, 3, 3, 1, 1, 1, False), ["tiny_conv_fwd_kernel<3, 3, 3, 3>"], [IG128x64_SLOW_KN, "tiny_conv_wgrad_kernel<3, 3, 3, 3> + reduce_slabs_2d"]),
    # --- transposed convolutions (the forward is the [K][N] launch per output parity, the backward-data the plain one): the direct kernels,
    # and the x3 form (gemm_x3.hip: kernel != stride takes the general form from 2 N H W K^2 Cin Cout >= 3e10 on, i.e. 7 images here -- at
    # test_deconv2d's 3 images this layer runs the direct kernels) on and off
    row("deconv-direct", 'deconv', (2, 32, 8, 8, 16, 4, 2, 1), [IG64_32_KN] * 4, [IG64_16, WG64]),
    row("deconv-x3", 'deconv', (7, 512, 32, 32, 256, 4, 2, 1), [X3_TR] + [X3NT_TAPS] * 4, [X3_ROWS, X3_ROWS, X3NT_TAPS, X3_ROWS, X3TN_TAPS, X3_RED]),
    row("deconv-x3-off", 'deconv', (7, 512, 32, 32, 256, 4, 2, 1), [IG64_32_KN] * 4, [IG64_32, WG_DMA, RS], x3=0),
]


# ---------------------------------------------------------------------------------------------- Winograd at the edges of its rules
WINO_ROWS = [
    # F(4x4), native products, the smallest launch: T = 2 x 16 x 16 = 512 tiles (36 T >= 16384), Cn = 64: the 36 products are one batched
    # 64x64-tile launch, the weight gradient's one batched wgemm_tn_dma launch.  The backward-data's reduction runs over Cout = 64 < 128
    # channels: direct (split over K)
    row("wino-f4-smallest", 'conv', (2, 128, 64, 64, 64, 3, 1, 1, 0, False), [IG64_32], [IG64_32_KN, SKF, WG_DMA], wino=(True, False, True)),
    # ... with bias and ReLU in wino4_output_kernel's epilogue
    row("wino-f4-bias-relu", 'conv', (2, 128, 64, 64, 64, 3, 1, 1, 1, True), [IG64_32], [IG64_32_KN, SKF, WG_DMA], wino=(True, False, True)),
    # Ck = 144 (% 32 != 0: K-step 16 products), Cn = 80.  The direct forward of this shape would leave the same single record (Cin % 32 != 0,
    # 256 tiles, not split over K): here only the workspace query tells the Winograd forward from the direct one, not the record
    row("wino-f4-c144-c80", 'conv', (2, 144, 64, 64, 80, 3, 1, 1, 0, False), [IG64_16], [IG64_16_KN, WG_DMA], wino=(True, False, True)),
    # H % 4 != 0: F(2x2), T = 4 x 17 x 17 = 1156 tiles (not a multiple of 128; 16 T >= 16384); no Winograd weight gradient (F(4x4) only)
    row("wino-f2-fallback", 'conv', (4, 128, 34, 34, 64, 3, 1, 1, 0, False), [IG64_32], [IG64_32_KN, SKF, WG64, RS], wino=(True, False, False)),
    # forward and backward-data Winograd, weight gradient direct: T = 3 x 13 x 13 = 507 is odd (wino_wgrad_plan: T % 16)
    row("wino-f4-odd-t", 'conv', (3, 128, 52, 52, 128, 3, 1, 1, 0, False), [IG64_32], [IG64_32, WG64, RS], wino=(True, True, False)),
]


def run_op(F, r, case):
    """-> (output, dx, dw, db, forward records, backward records) of the row's op on the GPU."""
    op, cfg = r['op'], r['cfg']
    cl = torch.channels_last
    if op == 'linear':
        xd, wd = dev(case['x']).requires_grad_(r['grad']), dev(case['w']).requires_grad_(r['grad'])
    else:
        xd = dev(case['x']).contiguous(memory_format=cl).requires_grad_(r['grad'])
        wd = dev(case['w']).contiguous(memory_format=cl).requires_grad_(r['grad'])
    bd = dev(case['b']).requires_grad_(r['grad']) if case['b'] is not None else None
    with kernels_run(F) as fwd:
        if op == 'linear':
            out = F.linear(xd, wd, bd, cfg[3])
        elif op == 'conv':
            out = F.conv2d(xd, wd, bd, cfg[6], cfg[7], cfg[8])
        else:
            out = F.deconv2d(xd, wd, bd, cfg[6], cfg[7])
    assert out.shape == case['out'].shape
    bwd = []
    if r['grad']:
        with kernels_run(F) as bwd:
            out.backward(dev(case['gy']))
    return out, xd.grad, wd.grad, bd.grad if bd is not None else None, fwd, bwd


def compare(report, case, bars, out, dx, dw, db, grad=True):
    bad = [check(report, 'fwd', out, case['out'], *bars['fwd'])]
    if grad:
        bad += [check(report, 'dx', dx, case['dx'], *bars['dx']), check(report, 'dw', dw, case['dw'], *bars['dw'])]
        if db is not None:
            bad.append(check(report, 'db', db, case['db'], *bars['db']))
    return [m for m in bad if m]


def wino_launches(F, cfg):
    N, Cin, H, W, Cout, k, s, p = cfg[:8]
    return tuple(F._L().pdf_conv2d_winograd_workspace_floats(N, H, W, Cin, Cout, k, k, s, p, b) > 0 for b in (0, 1, 2))


@pytest.mark.parametrize("r", ROWS + WINO_ROWS)
def test_kernel_and_float64_parity(F, r, monkeypatch, request):
    op, cfg = r['op'], r['cfg']
    t0 = time.perf_counter()
    case = {'conv': conv_case, 'linear': linear_case, 'deconv': deconv_case}[op](cfg)
    t_ref = time.perf_counter() - t0
    bars = {'conv': conv_bars, 'linear': linear_bars}[op](cfg) if op != 'deconv' else DECONV_BARS
    assert case['share'] <= 1e-3, "pre-activations within the forward bar of zero: %.2e of the outputs" % case['share']
    monkeypatch.setattr(F, "WINOGRAD", r['wino'] is not None)
    F.set_x3(r['x3'])
    try:
        if r['grad']:
            res = run_op(F, r, case)
        else:
            with torch.no_grad():
                res = run_op(F, r, case)
        out, dx, dw, db, fwd, bwd = res
        wino = wino_launches(F, cfg) if (op == 'conv' and r['wino'] is not None and r['grad']) else None
    finally:
        F.set_x3(None)
    report = ["%s %s %s (float64 reference: %.1f s on %d threads)" % (request.node.callspec.id, op, cfg, t_ref, torch.get_num_threads()), "    forward : %s" % fwd, "    backward: %s" % bwd]
    if r['wino'] is not None:
        report.append("    Winograd (forward, backward-data, weight gradient): %s" % (wino,))
    bad = compare(report, case, bars, out, dx, dw, db, r['grad'])
    print("\n" + "\n".join(report))
    assert fwd == r['fwd'], "forward ran %s, the row is for %s" % (fwd, r['fwd'])
    assert bwd == r['bwd'], "backward ran %s, the row is for %s" % (bwd, r['bwd'])
    if r['wino'] is not None and r['grad']:
        assert wino == r['wino']
    assert not bad, bad


def conv_on_gpu(F, case, cfg, skip=None):
    """conv2d (or conv2d_with_skip, the shortcut weighted by `skip`) forward and backward -> (out, dx, dw, db, forward records, backward records)."""
    cl = torch.channels_last
    xd = dev(case['x']).contiguous(memory_format=cl).requires_grad_()
    wd = dev(case['w']).contiguous(memory_format=cl).requires_grad_()
    bd = dev(case['b']).requires_grad_() if case['b'] is not None else None
    with kernels_run(F) as fwd:
        if skip is None:
            out = F.conv2d(xd, wd, bd, cfg[6], cfg[7], cfg[8])
        else:
            out, sc = F.conv2d_with_skip(xd, wd, bd, cfg[6], cfg[7], cfg[8])
    with kernels_run(F) as bwd:
        if skip is None:
            out.backward(dev(case['gy']))
        else:
            ((out * dev(case['gy'])).sum() + (sc * dev(skip).contiguous(memory_format=cl)).sum()).backward()
    return out, xd.grad, wd.grad, bd.grad if bd is not None else None, fwd, bwd


def test_x3_winograd_products_are_no_worse_than_the_native_ones(F, monkeypatch):
    """The smallest x3 launch (wino_x3: C >= 256, T >= 2048 tiles): (8, 256, 64, 64, 256).  With x3 on, all three launches' products are x3
    ones; off, the native fp32 MFMA kernels.  Both meet test_conv2d's bars against float64, and the x3 result's error does not exceed
    the native result's on the same operands (the gate of tests/test_x3_gpu.py: rms <= 1.0x, max <= 1.25x)."""
    cfg = (8, 256, 64, 64, 256, 3, 1, 1, 0, False)
    case, bars = conv_case(cfg), conv_bars(cfg)
    monkeypatch.setattr(F, "WINOGRAD", True)
    errs, names, bad = {}, {}, []
    for x3 in (None, 0):
        F.set_x3(x3)
        try:
            out, dx, dw, db, fwd, bwd = conv_on_gpu(F, case, cfg)
            assert wino_launches(F, cfg) == (True, True, True)
        finally:
            F.set_x3(None)
        report = ["x3 %s %s" % ("on" if x3 is None else "off", cfg), "    forward : %s" % fwd, "    backward: %s" % bwd]
        bad += compare(report, case, bars, out, dx, dw, db)
        errs[x3] = [err_of(a, case[k]) for a, k in ((out, 'out'), (dx, 'dx'), (dw, 'dw'))]
        report.append("    (max, rms) of out, dx, dw: %s" % (errs[x3],))
        print("\n" + "\n".join(report))
        names[x3] = (fwd, bwd)
    assert names[None] == ([X3NT_WIDE], [X3NT_WIDE, X3TN_WIDE]), names[None]
    assert names[0] == ([IG128], [IG128, WG_DMA]), names[0]
    assert not bad, bad
    for (mx, rms), (mx0, rms0), what in zip(errs[None], errs[0], ('out', 'dx', 'dw')):
        assert rms <= 1.0 * rms0 and mx <= 1.25 * mx0, "%s: x3 (max %.3e, rms %.3e) against native (max %.3e, rms %.3e)" % (what, mx, rms, mx0, rms0)


@pytest.mark.parametrize("keep_v", [True, False])
def test_x3_forward_whose_weight_gradient_is_native(F, monkeypatch, keep_v):
    """Cin = 256, T = 2048, Cout = 80 (% 32 != 0): the forward's V is x3, the weight gradient's products are native -- the cached V is in the
    other format -- the plan records both -- and the weight gradient must transform the input again, whether the forward's workspace was kept
    (F.WINOGRAD_KEEP_V) or not.  (The backward-data's reduction runs over 80 < 128 channels: direct.)"""
    cfg = (8, 256, 64, 64, 80, 3, 1, 1, 0, False)
    case, bars = conv_case(cfg), conv_bars(cfg)
    monkeypatch.setattr(F, "WINOGRAD", True)
    monkeypatch.setattr(F, "WINOGRAD_KEEP_V", keep_v)
    out, dx, dw, db, fwd, bwd = conv_on_gpu(F, case, cfg)
    report = ["keep V %s %s" % (keep_v, cfg), "    forward : %s" % fwd, "    backward: %s" % bwd]
    bad = compare(report, case, bars, out, dx, dw, db)
    print("\n" + "\n".join(report))
    assert wino_launches(F, cfg) == (True, False, True)
    assert fwd == [X3NT] and bwd == [IG64_16_KN, WG_DMA], (fwd, bwd)
    assert not bad, bad


def test_winograd_forwards_sharing_one_transformed_input(F, monkeypatch):
    """Two convolutions with different Cout on one input marked with F.share_winograd_input: the second forward and both weight gradients
    read the V the first forward left in its workspace.  Both outputs, both weight gradients and the summed input gradient against float64."""
    monkeypatch.setattr(F, "WINOGRAD", True)
    monkeypatch.setattr(F, "WINOGRAD_KEEP_V", True)
    N, Cin, H, W = 2, 128, 64, 64
    cfgs = [(N, Cin, H, W, 64, 3, 1, 1, 0, False), (N, Cin, H, W, 128, 3, 1, 1, 0, False)]
    x = rnd(N, Cin, H, W, seed=1)
    ws = [rnd(c[4], Cin, 3, 3, seed=2 + i, scale=(Cin * 9) ** -0.5) for i, c in enumerate(cfgs)]
    gys = [rnd(N, c[4], H, W, seed=7 + i) for i, c in enumerate(cfgs)]
    xr = x.double().requires_grad_()
    wr = [w.double().requires_grad_() for w in ws]
    refs = [TF.conv2d(xr, w, None, 1, 1) for w in wr]
    torch.autograd.backward(refs, [g.double() for g in gys])
    cl = torch.channels_last
    xd = F.share_winograd_input(dev(x).contiguous(memory_format=cl).requires_grad_())
    wd = [dev(w).contiguous(memory_format=cl).requires_grad_() for w in ws]
    with kernels_run(F) as fwd:
        outs = [F.conv2d(xd, w, None, 1, 1) for w in wd]
    assert len(xd._pdf_wino_share) == 1, "the first forward did not publish its V"
    with kernels_run(F) as bwd:
        torch.autograd.backward(outs, [dev(g) for g in gys])
    report = ["shared V %s" % (cfgs,), "    forward : %s" % fwd, "    backward: %s" % bwd]
    bad = []
    for i, c in enumerate(cfgs):
        assert wino_launches(F, c) == (True, c[4] >= 128, True)
        b = conv_bars(c)
        bad += [check(report, 'fwd %d' % i, outs[i], refs[i].detach(), *b['fwd']), check(report, 'dw %d' % i, wd[i].grad, wr[i].grad, *b['dw'])]
    bad.append(check(report, 'dx', xd.grad, xr.grad, *conv_bars(cfgs[0])['dx']))         # the sum of both backward-data results, at test_conv2d's dx bar
    print("\n" + "\n".join(report))
    assert not [m for m in bad if m], bad


def test_winograd_backward_data_accumulates_onto_the_shortcut_gradient(F, monkeypatch):
    """F.conv2d_with_skip at a shape whose backward-data is a Winograd launch (128 -> 128 channels, 64x64 maps, T = 512): the shortcut's
    gradient is added in wino4_output_kernel (accum).  (test_conv_with_skip...'s 1x1 convolution never takes this path.)"""
    cfg = (2, 128, 64, 64, 128, 3, 1, 1, 0, False)
    case, bars = conv_case(cfg), conv_bars(cfg)
    monkeypatch.setattr(F, "WINOGRAD", True)
    skip = rnd(*case['x'].shape, seed=9)
    out, dx, dw, db, fwd, bwd = conv_on_gpu(F, case, cfg, skip=skip)
    report = ["accum %s" % (cfg,), "    forward : %s" % fwd, "    backward: %s" % bwd]
    ref = dict(case, dx=case['dx'] + skip.double())
    bad = compare(report, ref, bars, out, dx, dw, db)
    print("\n" + "\n".join(report))
    assert wino_launches(F, cfg) == (True, True, True)
    assert fwd == [IG64_32] and bwd == [IG64_32, WG_DMA], (fwd, bwd)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- the lazy-BatchNorm consumer
@pytest.mark.parametrize("R,C,N,fwd,bwd", [(4096, 64, 128, ["igemm_nt_aff<64, 64, 2, 2, 32>"], [IG64_32_KN, "wgemm_tn64_aff", RS2D]),
                                           (20480, 128, 256, ["igemm_nt_aff<64, 64, 2, 2, 32>"], [IG64_32_KN, "wgemm_tn_dma_aff", RS2D])])
def test_lazy_batchnorm_consumer_kernels_against_float64(F, R, C, N, fwd, bwd):
    """igemm_nt_aff / wgemm_tn64_aff / wgemm_tn_dma_aff: F.batch_norm(..., relu=True, lazy=True) -> F.linear, where the GEMM applies
    relu(x * scale + shift) while it stages its operand (test_lazy_batchnorm_applied_by_the_consuming_linear compares it with the
    materialised form only).  Output, weight and bias gradient against float64 BatchNorm + ReLU + linear at test_linear's bars.
    The backward-data record (the plain [K][N] 64x64 tile, which tile64-k32 compares with float64) produces the gradient of the
    normalised rows; what leaves the layer -- dx, dgamma, dbeta -- has been through the BatchNorm's backward and its ReLU mask, where
    float32 and float64 may put a value within rounding of zero on different sides: an O(1) change of that element's gradient and of
    the column sums in either valid evaluation.  Those three are therefore left to
    test_lazy_batchnorm_applied_by_the_consuming_linear, which holds them to the materialised form (same mask), and to test_batchnorm."""
    x = rnd(R, C, seed=5) * 1.3 + 0.2
    w, b = rnd(N, C, seed=6) / C ** 0.5, rnd(N, seed=7)
    g, be = torch.rand(C, generator=torch.Generator().manual_seed(8)) + 0.5, rnd(C, seed=8) * 0.3
    dy = rnd(R, N, seed=9)
    wr, br = w.double().requires_grad_(), b.double().requires_grad_()
    z = TF.relu(TF.batch_norm(x.double(), None, None, g.double(), be.double(), True, 0.1, 1e-5))
    ref = TF.linear(z, wr, br)
    ref.backward(dy.double())
    xd, wd, bd = dev(x).requires_grad_(), dev(w).requires_grad_(), dev(b).requires_grad_()
    gd, bed = dev(g).requires_grad_(), dev(be).requires_grad_()
    zd = F.batch_norm(xd, gd, bed, dev(torch.zeros(C)), dev(torch.ones(C)), True, 0.1, 1e-5, relu=True, lazy=True)
    assert getattr(zd, '_pdf_lazy', None) is not None
    with kernels_run(F) as f:
        y = F.linear(zd, wd, bd, F.ACT_NONE)
    with kernels_run(F) as bw:
        y.backward(dev(dy))
    bw = [n for n in bw if n.startswith(("igemm", "wgemm", "reduce_slabs", "small_k", "splitk"))]      # (the BatchNorm's own kernels carry no GEMM-family record)
    report = ["lazy BatchNorm -> linear %s" % ((R, C, N),), "    forward : %s" % f, "    backward: %s" % bw]
    bars = linear_bars((R, C, N, 0, True))
    bad = [check(report, 'fwd', y, ref.detach(), *bars['fwd']), check(report, 'dw', wd.grad, wr.grad, *bars['dw']), check(report, 'db', bd.grad, br.grad, *bars['db'])]
    print("\n" + "\n".join(report))
    assert f == fwd and bw == bwd, (f, bw)
    assert not [m for m in bad if m], bad
