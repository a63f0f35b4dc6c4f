"""The launchers of the Winograd convolutions and the x3 transposed convolutions stay inside the workspace size their plan reports
(csrc/gemm_internal.h; tests/test_ws_plan_cpu.py checks the plans themselves, without a device).  Through the C ABI, per pass:
the workspace is total + G floats in ONE allocation (G = the plan's largest region, so a region placed one slot too far lands in the
guard, not outside the allocation), filled with a fixed bit pattern; the call is told ws_floats = total; afterwards the guard still
holds the pattern and the result equals, bit for bit, a second run told total + G.  Told total - 1, the same call takes the direct
kernels (pdf_debug_last_tile() != 128128 for the Winograd passes) and is correct within the bars of tests/test_headline_gpu.py."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as TF

from tests.test_ws_plan_cpu import plan

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5A5A5A
# N, H, W, Cin, Cout: fp32 planes; x3 planes; fp32 forward whose backward-data is x3; x3 forward whose weight gradient is fp32 (Cout % 32 != 0) and
# must refuse the forward's V; F(2x2) (forward only)
WINO = [(2, 64, 64, 128, 64), (2, 128, 128, 256, 256), (2, 128, 128, 128, 256), (2, 128, 128, 256, 80), (4, 34, 34, 128, 64)]
# N, H, W, Cin, Cout, k, stride, pad: the smallest shapes over the 3e10-flop bar of each form with the real channel counts (p4, p5; p3)
X3D = [(1, 64, 64, 1024, 256, 4, 4, 0), (1, 32, 32, 2048, 256, 8, 8, 0), (2, 64, 64, 512, 256, 4, 2, 1)]


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pdfnet_amd import functional as F
    return F


def _rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _close(a, b, atol, rtol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err, lim = float((a - b).abs().max()), atol + rtol * float(b.abs().max())
    assert err <= lim, "%s: max err %.3e > %.3e (max|ref| = %.3e)" % (what, err, lim, float(b.abs().max()))


@functools.lru_cache(maxsize=None)
def _reference(kind, cfg):
    """NCHW operands and the float32 CPU results of all three passes, computed once per shape."""
    torch.set_num_threads(16)
    if kind == 0:
        N, H, W, Cin, Cout = cfg
        x, w, b = _rnd(N, Cin, H, W, seed=1), _rnd(Cout, Cin, 3, 3, seed=2, scale=(Cin * 9) ** -0.5), _rnd(Cout, seed=3)
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        ref = TF.conv2d(xr, wr, br, 1, 1)
    else:
        N, H, W, Cin, Cout, k, s, p = cfg
        x, w, b = _rnd(N, Cin, H, W, seed=1), _rnd(Cin, Cout, k, k, seed=2, scale=Cin ** -0.5), _rnd(Cout, seed=3)
        xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
        ref = TF.conv_transpose2d(xr, wr, br, s, p)
    gy = _rnd(*ref.shape, seed=4)
    ref.backward(gy)
    return x, w, b, gy, ref.detach(), xr.grad, wr.grad, br.grad


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _guarded(L, F, kind, pas, shape, run):
    """Run `run(ws pointer, ws_floats, opts)` -> result tensors under the three workspace sizes; -> (result told total, result told total - 1)."""
    from pdfnet_amd import hip
    p = plan(L.cdll, kind, pas, shape)
    assert p["ok"] and p["total"] > 0, (kind, pas, shape, p)
    total, G = p["total"], max(ln for _, ln in p["regions"])
    buf = torch.empty(total + G, dtype=torch.int32, device="cuda")
    res = []
    for told in (total, total + G, total - 1):
        buf.fill_(PATTERN)
        o = hip.CallOpts()
        o.ws, o.ws_floats = buf.data_ptr(), told
        out = run(o)
        torch.cuda.synchronize()
        if told == total:
            assert bool((buf[total:] == PATTERN).all()), "a launcher wrote past the %d floats its plan reports (%s)" % (total, (kind, pas, shape))
            assert not bool((buf[:total] == PATTERN).all())
        if told == total - 1:
            assert bool((buf == PATTERN).all()), "a workspace one float short was used"
        res.append((out, L.pdf_debug_last_tile()))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b), (kind, pas, shape)
    if kind == 0 and pas < 2:                                 # (a Winograd run shows in its written workspace, above: its batched product reports its own tile)
        assert res[2][1] != 128128, [r[1] for r in res]
    return res[0][0], res[2][0], buf, p


@pytest.mark.parametrize("cfg", WINO)
def test_winograd_launchers_stay_inside_the_size_their_plan_reports(F, cfg):
    from pdfnet_amd import hip
    L, S = F._L(), hip.stream
    N, H, W, Cin, Cout = cfg
    shape = cfg + (3, 3, 1, 1)
    x, w, b, gy, ref, dx_ref, dw_ref, db_ref = _reference(0, cfg)
    xd, wd, bd, gd = _nhwc(x), _nhwc(w), b.cuda(), _nhwc(gy)
    M, K = N * H * W, 9 * Cin
    sizes = [L.pdf_conv2d_winograd_workspace_floats(*shape, pas) for pas in (0, 1, 2)]
    assert sizes[0] > 0

    def fwd(o):
        y = torch.empty(N, H, W, Cout, device="cuda")
        L.pdf_conv2d_fwd_x(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N, H, W, Cin, Cin, Cout, 3, 3, 1, 1, H, W, Cout, 0, S(), ctypes.byref(o))
        return (y,)
    (y,), (y_direct,), fbuf, fplan = _guarded(L, F, 0, 0, shape, fwd)
    f4 = 2e-4 if fplan["form"] == 4 else 0.0                  # (F(4x4)'s own arithmetic: tests/test_headline_gpu.py)
    _close(y.permute(0, 3, 1, 2), ref, 3e-5 * max(1, K ** 0.5 / 16) + f4, 1e-5, "Winograd fwd")
    _close(y_direct.permute(0, 3, 1, 2), ref, 3e-5 * max(1, K ** 0.5 / 16), 1e-5, "direct fwd")
    if sizes[1] > 0:
        def bwd(o):
            dx = torch.empty(N, H, W, Cin, device="cuda")
            L.pdf_conv2d_bwd_data_x(gd.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, Cin, Cin, Cout, 3, 3, 1, 1, H, W, Cout, S(), ctypes.byref(o))
            return (dx,)
        (dx,), (dx_direct,), _, bplan = _guarded(L, F, 0, 1, shape, bwd)
        _close(dx.permute(0, 3, 1, 2), dx_ref, 1e-4 + (2e-4 if bplan["form"] == 4 else 0.0), 2e-5, "Winograd dx")
        _close(dx_direct.permute(0, 3, 1, 2), dx_ref, 1e-4, 2e-5, "direct dx")
    if sizes[2] > 0:
        pws, pn = F._wgrad_ws(M, Cout, K, xd.device)

        def wgrad(o, v=None):
            dw, db = torch.empty(Cout, 3, 3, Cin, device="cuda"), torch.empty(Cout, device="cuda")
            if v is not None:
                o.wino_v = v
            L.pdf_conv2d_bwd_weight_x(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), db.data_ptr(), pws.data_ptr(), pn, N, H, W, Cin, Cin, Cout, 3, 3, 1, 1,
                                      H, W, Cout, 0, S(), ctypes.byref(o))
            return dw, db
        (dw, db), (dw_direct, db_direct), wbuf, wplan = _guarded(L, F, 0, 2, shape, wgrad)
        for got, what in ((dw, "Winograd"), (dw_direct, "direct")):
            _close(got.permute(0, 3, 1, 2), dw_ref, 5e-5 * max(1, M ** 0.5 / 16), 5e-5, what + " dw")
        for got, what in ((db, "Winograd"), (db_direct, "direct")):
            _close(got, db_ref, 1e-4 * max(1, M ** 0.5 / 64), 5e-5, what + " db")
        # ... and with the forward's V handed in: used when the plan's two formats agree, refused when they differ -- same bits either way
        voff = L.pdf_conv2d_winograd_v_offset(*shape)
        assert voff == fplan["v_offset"] >= 0
        if cfg[4] % 32 != 0 and fplan["x3"]:
            assert wplan["shared_v_x3"] == 1 and wplan["x3"] == 0
        fbuf.fill_(PATTERN)
        o = hip.CallOpts()
        o.ws, o.ws_floats = fbuf.data_ptr(), fplan["total"]
        fwd(o)
        wbuf.fill_(PATTERN)
        o = hip.CallOpts()
        o.ws, o.ws_floats = wbuf.data_ptr(), wplan["total"]
        dw_v, db_v = wgrad(o, fbuf.data_ptr() + 4 * voff)
        torch.cuda.synchronize()
        assert torch.equal(dw_v, dw) and torch.equal(db_v, db)
        assert bool((wbuf[wplan["total"]:] == PATTERN).all())
        used_own_v = not bool((wbuf[:wplan["regions"][0][1]] == PATTERN).all())
        assert used_own_v == (wplan["shared_v_x3"] != wplan["x3"])      # its own V region is written only when the forward's was refused


@pytest.mark.parametrize("cfg", X3D)
def test_x3_deconv_launchers_stay_inside_the_size_their_plan_reports(F, cfg):
    from pdfnet_amd import hip
    L, S = F._L(), hip.stream
    N, H, W, Cin, Cout, k, s, p = cfg
    shape = (N, H, W, Cin, Cout, k, k, s, p)
    x, w, b, gy, ref, dx_ref, dw_ref, _ = _reference(1, cfg)
    OH, OW = ref.shape[2], ref.shape[3]
    xd, wd, bd, gd = _nhwc(x), _nhwc(w), b.cuda(), _nhwc(gy)      # w [Cin][Cout][k][k] -> [Cin][k][k][Cout]
    M = N * H * W
    assert all(L.pdf_deconv2d_x3_workspace_floats(*shape, pas) > 0 for pas in (0, 1, 2))

    def fwd(o):
        y = torch.empty(N, OH, OW, Cout, device="cuda")
        L.pdf_deconv2d_fwd_x(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N, H, W, Cin, Cin, Cout, k, k, s, p, OH, OW, Cout, S(), ctypes.byref(o))
        return (y,)

    def bwd(o):
        dx = torch.empty(N, H, W, Cin, device="cuda")
        L.pdf_deconv2d_bwd_data_x(gd.data_ptr(), wd.data_ptr(), dx.data_ptr(), N, H, W, Cin, Cin, Cout, k, k, s, p, OH, OW, Cout, S(), ctypes.byref(o))
        return (dx,)
    pws, pn = F._wgrad_ws(M, Cin, k * k * Cout, xd.device)

    def wgrad(o):
        dw = torch.empty(Cin, k, k, Cout, device="cuda")
        L.pdf_deconv2d_bwd_weight_x(xd.data_ptr(), gd.data_ptr(), dw.data_ptr(), pws.data_ptr(), pn, N, H, W, Cin, Cin, Cout, k, k, s, p, OH, OW, Cout, 0, S(),
                                    ctypes.byref(o))
        return (dw,)
    for pas, run, want, bar, perm in ((0, fwd, ref, (5e-5 * max(1, Cin ** 0.5 / 16), 1e-5), (0, 3, 1, 2)), (1, bwd, dx_ref, (2e-4, 2e-5), (0, 3, 1, 2)),
                                     (2, wgrad, dw_ref, (5e-5 * max(1, M ** 0.5 / 16), 5e-5), (0, 3, 1, 2))):
        (got,), (direct,), _, _ = _guarded(L, F, 1, pas, shape, run)
        _close(got.permute(*perm), want, bar[0], bar[1], "x3 deconv pass %d" % pas)
        _close(direct.permute(*perm), want, bar[0], bar[1], "direct deconv pass %d" % pas)
