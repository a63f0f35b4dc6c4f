"""BatchNorm backward with frozen statistics against the training backward on the ResNet stem's shape (R = 32*128*128 rows, C = 64,
ReLU, no residual): pdf_bn_eval_bwd with sums (one pass: dy, x -> dx) and pdf_bn_train_bwd (two passes over (dy, x), then dx), timed
in one process in alternating windows with device events.  Bytes are the algorithmic ones: 3 resp. 5 tensors of R*C floats.
Usage: python tools/bn_frozen_bench.py [rounds]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pdfnet_amd import hip


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    iters = 200
    L = hip.lib()
    C, R, eps = 64, 32 * 128 * 128, 1e-5
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(R, C, device=dev, generator=g) * 2 + 0.5
    dy = torch.randn(R, C, device=dev, generator=g)
    gamma, beta = torch.rand(C, device=dev, generator=g) + 0.5, torch.randn(C, device=dev, generator=g)
    rm, rv = x.mean(0), x.var(0, unbiased=False)
    rstd = torch.rsqrt(rv + eps)
    scale = gamma * rstd
    shift = beta - rm * scale
    dx_e, dx_t = torch.empty_like(x), torch.empty_like(x)
    dg_e, db_e, dg_t, db_t = (torch.empty(C, device=dev) for _ in range(4))
    ws = torch.empty(L.pdf_bn_workspace_floats(C, R) + 3 * C, device=dev)
    p, s = hip.ptr, hip.stream

    def frozen():
        L.pdf_bn_eval_bwd(p(dy), C, None, C, 2, p(x), C, p(rm), p(rv), eps, p(scale), p(shift), C, R, p(dx_e), C, None, C, p(dg_e), p(db_e), 0, p(ws), s())

    def frozen_nosums():
        L.pdf_bn_eval_bwd(p(dy), C, None, C, 2, p(x), C, p(rm), p(rv), eps, p(scale), p(shift), C, R, p(dx_e), C, None, C, None, None, 0, None, s())

    def frozen_sums_only():
        L.pdf_bn_eval_bwd(p(dy), C, None, C, 2, p(x), C, p(rm), p(rv), eps, p(scale), p(shift), C, R, None, C, None, C, p(dg_e), p(db_e), 0, p(ws), s())

    def train():
        L.pdf_bn_train_bwd(p(dy), C, None, C, 2, p(x), C, p(rm), p(rstd), p(gamma), p(scale), p(shift), C, R, p(dx_t), C, None, C, p(dg_t), p(db_t), 0, p(ws), s())

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters

    fns = (("pdf_bn_train_bwd", train, 5), ("pdf_bn_eval_bwd, sums", frozen, 3), ("pdf_bn_eval_bwd, no sums", frozen_nosums, 3),
           ("pdf_bn_eval_bwd, sums only", frozen_sums_only, 2))
    for _, fn, _ in fns:                                      # warm up every shape of the timed windows
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    # same statistics, same mask: the two backward passes share dbeta and dgamma (summation order aside)
    print("dgamma / dbeta, frozen vs training backward: max |diff| %.3e / %.3e (max |value| %.3e / %.3e)"
          % (float((dg_e - dg_t).abs().max()), float((db_e - db_t).abs().max()), float(dg_t.abs().max()), float(db_t.abs().max())))
    times = {n: [] for n, _, _ in fns}
    for _ in range(rounds):                                   # alternating windows
        for n, fn, _ in fns:
            times[n].append(window(fn))
    nb = R * C * 4
    med = {}
    for n, _, k in fns:
        t = sorted(times[n])
        med[n] = t[len(t) // 2]
        print("%-26s %d x %.1f MB  median %.4f ms  (min %.4f, max %.4f)  %.2f TB/s" % (n, k, nb / 1e6, med[n] * 1e3, t[0] * 1e3, t[-1] * 1e3, k * nb / med[n] / 1e12), flush=True)
    print("frozen with sums / training backward: %.3f  (by bytes 0.600)" % (med["pdf_bn_eval_bwd, sums"] / med["pdf_bn_train_bwd"]))


if __name__ == "__main__":
    main()
