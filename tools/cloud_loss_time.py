"""Time the cloud-to-mesh loss: `python tools/cloud_loss_time.py [--reps 5] [--bench FILE] [--bench-parent FILE] [--out profiles/cloud_loss_time.json]`
-> one JSON line (also written to --out).  Everything in one process, on the inputs of tools/icp_time.py (the template hands at B = 32,
P = 1,024, each displaced by up to 2 cm from the surface its cloud was sampled on).  Device-event times over 20 calls of: `F.cloud_mesh_loss`
forward alone (no gradient asked for), forward with the gradient plus backward, and `F.mesh_icp(iters=0)`, the same association without weights
and gather; the three are timed in turn `reps` times and the medians reported, with `ratio` = forward + backward over mesh_icp(iters=0)
(expected <= 1.25).  Then the eager train step of a small trainer (--res 128) on a synthetic batch with cloud_weight 0 and 0.01 (cloud_trim 10 m,
so that the random synthetic cloud has inliers), alternating, each timing over 10 steps ending in one host sync.
--bench / --bench-parent: files holding the JSON line `python bench.py` printed with this change and on the parent commit; their headline
figures are copied into the result side by side."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.icp_time import template_scene
from tools.render_time import device_ms

BENCH_KEYS = ('metric', 'value', 'unit', 'steps', 'warmup', 'ms_per_step', 'median_step_ms', 'images_per_s_at_median_step')


def bench_line(path):
    """The last JSON line of a file bench.py's output was kept in -> its headline entries (whichever of BENCH_KEYS it has)."""
    if not path:
        return None
    rows = [json.loads(l) for l in open(path) if l.lstrip().startswith('{')]
    return {k: rows[-1][k] for k in BENCH_KEYS if k in rows[-1]} if rows else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--bench', default=None)
    ap.add_argument('--bench-parent', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench import make_opt
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    dev = torch.device('cuda', 0)
    verts, faces, cloud, facing = template_scene(args.batch, args.points, dev)
    leaf = verts.clone().requires_grad_()
    up = torch.ones(args.batch, 2, device=dev)

    def both():
        leaf.grad = None
        F.cloud_mesh_loss(leaf, faces, cloud).backward(up)
    calls = {'forward': lambda: F.cloud_mesh_loss(verts, faces, cloud), 'forward_backward': both,
             'mesh_icp_iters0': lambda: F.mesh_icp(verts, faces, cloud, iters=0)}
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    med = lambda v: sorted(v)[len(v) // 2]
    loss, inliers = F.cloud_mesh_loss(verts, faces, cloud, return_fields=True)[:2]
    rms = F.mesh_icp(verts, faces, cloud, iters=0)[3]

    opt = make_opt(args.res)
    torch.manual_seed(0)
    model = load_model_intag(opt).to(dev)
    consts = synthetic_loss_constants()
    crit = CtdetLoss(opt, consts).to(dev)
    tr = Trainer(opt, model, crit, lr=0.0)
    batch = to_device(synthetic_train_batch(args.batch, args.res, seed=1, consts=consts), dev)
    opt.cloud_trim = 10.0
    step_ms = {0: [], 0.01: []}
    for rep in range(args.reps + 1):                           # rep 0 = warm-up
        for w in step_ms:
            opt.cloud_weight = w
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last = tr.train_step(batch, 0)
            torch.cuda.synchronize()
            if rep:
                step_ms[w].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert bool(torch.isfinite(last).all())
    line = json.dumps({"batch": args.batch, "points": args.points, "facing_share": round(facing, 4),
                       "cloud_mesh_loss_forward_ms": round(med(ms['forward']), 4), "cloud_mesh_loss_forward_backward_ms": round(med(ms['forward_backward']), 4),
                       "mesh_icp_iters0_ms": round(med(ms['mesh_icp_iters0']), 4),
                       "all_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                       "ratio": round(med(ms['forward_backward']) / med(ms['mesh_icp_iters0']), 4), "ratio_bar": 1.25,
                       "loss_mm2_mean": round(float(loss.mean()) * 1e6, 4), "rms_mm_mean": round(float(rms.mean()) * 1e3, 4),
                       "inliers_mean": round(float(inliers.float().mean()), 1),
                       "train_step": {"res": args.res, "steps": args.steps, "off_ms": [round(x, 3) for x in step_ms[0]],
                                      "on_ms": [round(x, 3) for x in step_ms[0.01]], "median_off_ms": round(med(step_ms[0]), 3),
                                      "median_on_ms": round(med(step_ms[0.01]), 3)},
                       "bench": bench_line(args.bench), "bench_parent": bench_line(args.bench_parent)})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
