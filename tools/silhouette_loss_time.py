"""Time the soft-silhouette loss: `python tools/silhouette_loss_time.py [--reps 5] [--out profiles/silhouette_loss_time.json]`
-> one JSON line (also written to --out).  Everything in one process, on the interacting template pair of tools/penetration_loss_time.py at
B = 32 (778 vertices, 1,538 faces per hand, Z = 0.45 m) under a camera that spreads the pair over a 128 x 128 mask; the masks are the soft
silhouettes of the same hands moved by 1 cm, thresholded at 0.5, the weight is 1 - the other hand's mask (as `silhouette_term` makes it).
Device-event times over 20 calls of `F.silhouette_loss` forward alone (no gradient asked for) and forward with the gradient plus backward, for
sigma = 0.5, 1 and 2 px^2; the calls are timed in turn `reps` times and the medians reported.  Then the eager train step of a small trainer
(--res 128) on a synthetic batch with silhouette_weight 0 and 1, alternating, each timing over 10 steps ending in one host sync."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.penetration_loss_time import template_hands
from tools.render_time import device_ms

SIGMAS = (0.5, 1.0, 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--res', type=int, default=128)
    ap.add_argument('--size', type=int, default=128)
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
    R = args.size
    verts, faces = template_hands(args.batch, ((0.06, 0.01, 0.0), (0.02, 0.0, 0.03)), dev)
    K = torch.tensor([[1.6 * R, 0, 0.38 * R], [0, 1.6 * R, 0.5 * R], [0, 0, 1]], device=dev).repeat(args.batch, 1, 1)
    table = F.vertex_face_table(faces, 778)
    moved = verts + torch.tensor([0.01, -0.005, 0.0], device=dev)
    empty = torch.zeros(args.batch, 2, R, R, device=dev)
    mask = (F.silhouette_loss(moved, faces, K, empty, sigma=1.0, return_fields=True)[2] > 0.5).float()
    weight = 1 - mask.flip(1)
    up = torch.ones(args.batch, 2, device=dev)
    leaf = verts.clone().requires_grad_()

    def both(sigma):
        def run():
            leaf.grad = None
            F.silhouette_loss(leaf, faces, K, mask, weight=weight, sigma=sigma, table=table).backward(up)
        return run
    calls = {}
    for s in SIGMAS:
        calls['forward_%g' % s] = lambda s=s: F.silhouette_loss(verts, faces, K, mask, weight=weight, sigma=s)
        calls['forward_backward_%g' % s] = both(s)
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    med = lambda v: sorted(v)[len(v) // 2]
    loss = {s: F.silhouette_loss(verts, faces, K, mask, weight=weight, sigma=s) for s in SIGMAS}
    assert all(bool(((v > 0) & (v < 1)).all()) for v in loss.values())      # the term is live: neither a perfect fit nor no overlap

    opt = make_opt(args.res)
    torch.manual_seed(0)
    model = load_model_intag(opt).to(dev)
    consts = synthetic_loss_constants()
    crit = CtdetLoss(opt, consts).to(dev)
    tr = Trainer(opt, model, crit, lr=0.0)
    batch = to_device(synthetic_train_batch(args.batch, args.res, seed=1, consts=consts), dev)
    step_ms = {0: [], 1.0: []}
    for rep in range(args.reps + 1):                           # rep 0 = warm-up
        for w in step_ms:
            opt.silhouette_weight = w
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last = tr.train_step(batch, 0)
            torch.cuda.synchronize()
            if rep:
                step_ms[w].append((time.perf_counter() - t0) * 1e3 / args.steps)
            assert bool(torch.isfinite(last).all())
    r4 = lambda x: round(x, 4)
    line = json.dumps({"batch": args.batch, "size": R, "mask_fill": r4(float(mask.mean())),
                       "loss_mean": {"%g" % s: r4(float(v.mean())) for s, v in loss.items()},
                       "silhouette_loss_forward_ms": {"%g" % s: r4(med(ms['forward_%g' % s])) for s in SIGMAS},
                       "silhouette_loss_forward_backward_ms": {"%g" % s: r4(med(ms['forward_backward_%g' % s])) for s in SIGMAS},
                       "all_ms": {k: [r4(x) for x in v] for k, v in ms.items()},
                       "train_step": {"res": args.res, "steps": args.steps, "sigma": 1.0, "down": 2, "off_ms": [round(x, 3) for x in step_ms[0]],
                                      "on_ms": [round(x, 3) for x in step_ms[1.0]], "median_off_ms": round(med(step_ms[0]), 3),
                                      "median_on_ms": round(med(step_ms[1.0]), 3)}})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
