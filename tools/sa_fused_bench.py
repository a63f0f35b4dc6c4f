#!/usr/bin/env python3
"""The fused set-abstraction MLP (F.sa_mlp_fused, csrc/safused.hip) against the per-layer kernels it replaces:

  * per level (1: 512 x 64 neighbourhoods of 64/64/128 channels; 2: 128 x 64 of 128/128/256), B = 32 and 64, one hand: forward and
    backward times (median of CUDA-event times) of the fused op and of the unfused chain
    gather_sub -> BN -> ReLU -> linear -> BN -> ReLU -> linear -> bn_relu_max_over_k, and memory_allocated() after the forward;
  * the full train step (Trainer, B = 32, fp32, eager) with PDFNET_SA_FUSED off and on, each mode in a FRESH process: ms per step,
    memory_allocated() after the model forward (minus the allocation before it), and the step's peak above the allocation before the
    step (max_memory_allocated() after reset_peak_memory_stats(), minus memory_allocated() at the reset).

    python tools/sa_fused_bench.py [--steps 10] [--out profiles/r07_sa_fused_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


LEVELS = {1: (1024, 512, 64, 16, (64, 64, 128), 0.015), 2: (512, 128, 64, 144, (128, 128, 256), 0.04)}   # N, S, K, Cin_pad, (C1, C2, C3), r


def _level_inputs(level, B):
    """Seeded level-`level` inputs: a cloud of B point sets (absolute coordinates around 0.45 m), conv1 applied per point, kNN indices,
    and the MLP's parameters / running statistics."""
    from pdfnet_amd import functional as F
    N, S, K, Cin, C, r = LEVELS[level]
    g = torch.Generator().manual_seed(level)
    rows = torch.zeros(B, N, Cin)
    rows[..., :2] = torch.rand(B, N, 2, generator=g) * 0.2 - 0.1
    rows[..., 2] = 0.4 + 0.1 * torch.rand(B, N, generator=g)
    rows[..., 3:] = torch.randn(B, N, Cin - 3, generator=g) * 0.5
    rows = rows.cuda()
    w1, b1 = torch.randn(C[0], Cin, generator=g).cuda() * Cin ** -0.5, torch.randn(C[0], generator=g).cuda() * 0.1
    p = {'w2': torch.randn(C[1], C[0], generator=g) * C[0] ** -0.5, 'b2': torch.randn(C[1], generator=g) * 0.1,
         'w3': torch.randn(C[2], C[1], generator=g) * C[1] ** -0.5, 'b3': torch.randn(C[2], generator=g) * 0.1}
    for i, c in enumerate(C, 1):
        p['g%d' % i], p['be%d' % i] = 1.0 + 0.3 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
        p['rm%d' % i], p['rv%d' % i] = torch.zeros(c), torch.ones(c)
    p = {k: t.cuda() for k, t in p.items()}
    with torch.no_grad():
        idx = F.knn_ball_indices(rows, S, K, r * r)
        u = F.linear(rows, w1, b1, fp32=True)
        v = F.linear(torch.nn.functional.pad(rows[:, :S, :3], (0, Cin - 3)), w1, fp32=True)
    return u, v, idx, p


def _mlp(u, v, idx, q, st, fused, K):
    """The level's MLP after conv1: F.sa_mlp_fused, or the per-layer kernels it replaces."""
    from pdfnet_amd import functional as F
    if fused:
        return F.sa_mlp_fused(u, v, idx, q['w2'], q['b2'], q['w3'], q['b3'], q['g1'], q['g2'], q['g3'], q['be1'], q['be2'], q['be3'],
                              st['rm1'], st['rv1'], st['rm2'], st['rv2'], st['rm3'], st['rv3'], True)
    y1 = F.gather_sub(u, v, idx)
    x = F.batch_norm(y1.reshape(-1, y1.shape[-1]), q['g1'], q['be1'], st['rm1'], st['rv1'], True, relu=True)
    x = F.batch_norm(F.linear(x, q['w2'], q['b2'], stats=True), q['g2'], q['be2'], st['rm2'], st['rv2'], True, relu=True)
    return F.bn_relu_max_over_k(F.linear(x, q['w3'], q['b3'], stats=True), q['g3'], q['be3'], st['rm3'], st['rv3'], K, True)


def level_bench(level, B, reps):
    from pdfnet_amd import functional as F
    N, S, K, Cin, C, r = LEVELS[level]
    u0, v0, idx, p = _level_inputs(level, B)
    gout = torch.randn(B * S, C[2], device='cuda')
    out = {}
    for name, fused in (("unfused", False), ("fused", True)):
        q = {k: (t.clone().requires_grad_() if k[:2] not in ('rm', 'rv') else t) for k, t in p.items()}
        u, v = u0.clone().requires_grad_(), v0.clone().requires_grad_()

        def fwd():
            st = {k: p[k].clone() for k in p if k[:2] in ('rm', 'rv')}
            return _mlp(u, v, idx, q, st, fused, K)
        fwd().backward(gout)                              # warm-up
        F.join_wgrad()
        torch.cuda.synchronize()
        t_f = _median_ms(fwd, reps)
        holder = {}

        def run_f():
            holder['y'] = fwd()

        def run_b():
            holder['y'].backward(gout)
            F.join_wgrad()
        times_b = []
        for _ in range(reps):
            run_f()
            torch.cuda.synchronize()
            times_b.append(_median_ms(run_b, 1))
        times_b.sort()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        y = fwd()
        torch.cuda.synchronize()
        mem = torch.cuda.memory_allocated() - base
        del y, holder
        out[name] = {"fwd_ms": round(t_f, 3), "bwd_ms": round(times_b[len(times_b) // 2], 3), "kept_after_fwd_MB": round(mem / 2 ** 20, 1)}
    return out


def step_bench(fused, steps, B=32):
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    import types
    F.set_sa_fused(fused)
    opt = types.SimpleNamespace(                        # the model / loss options of bench.py (its configs[2] workload)
        depth=True, heads={'hm': 2, 'wh': 2, 'params': 122}, iterations=False, PCA_SZ=63, knn_K=64, ball_radius=0.015, ball_radius2=0.04,
        sample_num_level1=512, sample_num_level2=128, INPUT_FEATURE_NUM=3, SAMPLE_NUM=1024, default_resolution=256,
        DECONV_DIMS=[256, 256, 256, 256], GCN_IN_DIM=[512, 256, 128], GCN_OUT_DIM=[256, 128, 64], IMG_DIMS=[256, 128, 64], graph_k=2,
        graph_layer_num=4, size_train=[256, 256], down_ratio=4, center_weight=200.0, reproj_weight=1.0, bone_dir_weight=200.0)
    consts = synthetic_loss_constants()
    torch.manual_seed(0)
    m = load_model_intag(opt).cuda()
    tr = Trainer(opt, m, CtdetLoss(opt, consts).cuda(), lr=0.0)
    batch = to_device(synthetic_train_batch(B, 256, seed=1, consts=consts), 'cuda')
    for _ in range(3):
        tr.train_step(batch)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        tr.train_step(batch)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    # memory: what the model forward keeps for the backward, and the step's peak above what is allocated before it
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    res = m(batch['input'], batch['choose'], batch['cloud'], batch['depth'], batch['ind'], batch['K_new'], batch['valid'])
    torch.cuda.synchronize()
    kept = torch.cuda.memory_allocated() - base
    del res
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    tr.train_step(batch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return {"ms_per_step_median": round(ms[len(ms) // 2], 2), "ms_per_step_min": round(ms[0], 2),
            "forward_kept_GB": round(kept / 1e9, 3), "step_peak_above_start_GB": round(peak / 1e9, 3),
            "allocated_before_step_GB": round(before / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-only", choices=("off", "on"), help=argparse.SUPPRESS)     # (the child process of one step measurement)
    a = ap.parse_args()
    if a.step_only:
        print(json.dumps(step_bench(a.step_only == "on", a.steps)), flush=True)
        return
    res = {"device": torch.cuda.get_device_name(0), "levels": {}}
    for level in (1, 2):
        for B in (32, 64):
            res["levels"]["L%d_B%d" % (level, B)] = level_bench(level, B, a.reps)
            print(json.dumps({"L%d_B%d" % (level, B): res["levels"]["L%d_B%d" % (level, B)]}), flush=True)
    if not a.no_step:
        res["step_B32"] = {}
        for mode in ("off", "on"):                     # each mode in a fresh process: allocator state and peaks do not carry over
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-only", mode, "--steps", str(a.steps)],
                               capture_output=True, text=True, check=True)
            res["step_B32"][mode] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps({"step_B32": res["step_B32"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
