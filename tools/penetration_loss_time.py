"""Time the inter-hand penetration loss: `python tools/penetration_loss_time.py [--reps 5] [--out profiles/penetration_loss_time.json]`
-> one JSON line (also written to --out).  Everything in one process, on the interpenetrating template hands at B = 32 (the template hand of
pdfnet_amd/data/gcn_core.npz, 20 cm, and its mirror image moved by (6, 1, 0) cm or (2, 0, 3) cm plus up to 5 mm that differs per sample, at
Z = 0.45 m), and on the same hands 25 cm apart, where nothing is inside and the closest-point walk and the gather are skipped.  Device-event
times over 20 calls of: `F.penetration_loss` forward alone (no gradient asked for), forward with both gradients plus backward, and
`F.mesh_penetration` on the same input, the evaluation metric whose winding-number sum the loss repeats (it also computes a distance to every
triangle, for every vertex); the calls are timed in turn `reps` times and the medians reported, with `ratio` = forward + backward over
mesh_penetration.  Then the eager train step of a small trainer (--res 128) on a synthetic batch with penetration_weight 0 and 0.01,
alternating, each timing over 10 steps ending in one host sync."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.render_time import device_ms


def template_hands(batch, shifts, dev, seed=0):
    """-> verts [batch, 2, 778, 3] (left = the mirrored template moved by shifts[b % len(shifts)] plus a seeded jitter of up to 5 mm, right = the
    template, both at Z = 0.45 m) and faces [2, 1538, 3]."""
    import pdfnet_amd
    z = np.load(os.path.join(os.path.dirname(pdfnet_amd.__file__), 'data', 'gcn_core.npz'))
    d = z['dense_coor'].astype(np.float64)
    right = (d - d.mean(0)) * 0.2
    left = right * np.array([-1.0, 1.0, 1.0])
    g = np.random.default_rng(seed)
    verts = np.stack([np.stack((left + np.asarray(shifts[b % len(shifts)]) + g.uniform(-0.005, 0.005, 3), right)) for b in range(batch)])
    verts = (verts + np.array([0.0, 0.0, 0.45])).astype(np.float32)
    faces = np.stack((z['mesh_faces_left'], z['mesh_faces_right'])).astype(np.int64)
    return torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench import make_opt
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer
    from pdfnet_amd.trains.simplified import CtdetLoss
    dev = torch.device('cuda', 0)
    verts, faces = template_hands(args.batch, ((0.06, 0.01, 0.0), (0.02, 0.0, 0.03)), dev)
    apart, _ = template_hands(args.batch, ((0.25, 0.0, 0.0),), dev)
    up = torch.ones(args.batch, 2, device=dev)

    def both(v):
        leaf = v.clone().requires_grad_()

        def run():
            leaf.grad = None
            F.penetration_loss(leaf, faces).backward(up)
        return run
    calls = {'forward': lambda: F.penetration_loss(verts, faces), 'forward_backward': both(verts),
             'mesh_penetration': lambda: F.mesh_penetration(verts, faces),
             'apart_forward': lambda: F.penetration_loss(apart, faces), 'apart_forward_backward': both(apart),
             'apart_mesh_penetration': lambda: F.mesh_penetration(apart, faces)}
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    med = lambda v: sorted(v)[len(v) // 2]
    loss, count = F.penetration_loss(verts, faces, return_fields=True)[:2]
    metric_count = F.mesh_penetration(verts, faces)[0]
    assert torch.equal(count, metric_count) and int(F.penetration_loss(apart, faces, return_fields=True)[1].sum()) == 0

    opt = make_opt(args.res)
    torch.manual_seed(0)
    model = load_model_intag(opt).to(dev)
    consts = synthetic_loss_constants()
    crit = CtdetLoss(opt, consts).to(dev)
    tr = Trainer(opt, model, crit, lr=0.0)
    batch = to_device(synthetic_train_batch(args.batch, args.res, seed=1, consts=consts), dev)
    step_ms = {0: [], 0.01: []}
    for rep in range(args.reps + 1):                           # rep 0 = warm-up
        for w in step_ms:
            opt.penetration_weight = w
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last = tr.train_step(batch, 0)
            torch.cuda.synchronize()
            if rep:
                step_ms[w].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert bool(torch.isfinite(last).all())
    r4 = lambda x: round(x, 4)
    line = json.dumps({"batch": args.batch, "inside_mean": round(float(count.float().mean()), 1), "loss_mm2_mean": r4(float(loss.mean()) * 1e6),
                       "penetration_loss_forward_ms": r4(med(ms['forward'])), "penetration_loss_forward_backward_ms": r4(med(ms['forward_backward'])),
                       "mesh_penetration_ms": r4(med(ms['mesh_penetration'])),
                       "ratio": r4(med(ms['forward_backward']) / med(ms['mesh_penetration'])),
                       "apart_forward_ms": r4(med(ms['apart_forward'])), "apart_forward_backward_ms": r4(med(ms['apart_forward_backward'])),
                       "apart_mesh_penetration_ms": r4(med(ms['apart_mesh_penetration'])),
                       "apart_ratio": r4(med(ms['apart_forward_backward']) / med(ms['apart_mesh_penetration'])),
                       "all_ms": {k: [r4(x) for x in v] for k, v in ms.items()},
                       "train_step": {"res": args.res, "steps": args.steps, "off_ms": [round(x, 3) for x in step_ms[0]],
                                      "on_ms": [round(x, 3) for x in step_ms[0.01]], "median_off_ms": round(med(step_ms[0]), 3),
                                      "median_on_ms": round(med(step_ms[0.01]), 3)}})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
