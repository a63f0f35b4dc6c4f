"""Time the ICP refinement: `python tools/icp_time.py [--batches 2] [--reps 3] [--out profiles/icp_time.json]` -> one JSON line (also written
to --out).  Device-event times over 20 calls at B = 32, P = 1,024: one `F.mesh_icp` launch on the template hands half a metre from the camera,
each displaced by up to 2 cm from the surface its cloud was sampled on, with iters = 0 and 8, translation-only and rigid; one
`F.mesh_penetration` launch on the same hands for scale; `refined_sums` on a synthetic batch.  Then Trainer.evaluation on the synthetic loader
with and without `refined`, alternating inside one process after a warm-up of each; every timing of `evaluation` ends in its own host sync (it
returns floats)."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.render_time import device_ms


def template_scene(batch, points, dev):
    """The template hand (pdfnet_amd/data/gcn_core.npz, 20 cm) and its mirror image 10 cm apart at Z = 0.5 m; per sample and hand a cloud of
    `points` vertices of the mesh drawn among those of its camera-facing triangles, with 1 mm noise, and a prediction shifted by up to 2 cm.
    -> verts [B, 2, 778, 3], faces [2, 1538, 3], cloud [B, 2, points, 3], the share of camera-facing triangles."""
    import pdfnet_amd
    z = np.load(os.path.join(os.path.dirname(pdfnet_amd.__file__), 'data', 'gcn_core.npz'))
    d = z['dense_coor'].astype(np.float64)
    right = (d - d.mean(0)) * 0.2
    pair = np.stack((right * [-1, 1, 1] + [-0.05, 0, 0.5], right + [0.05, 0, 0.5]))
    faces = np.stack((z['mesh_faces_left'], z['mesh_faces_right'])).astype(np.int64)
    rng = np.random.default_rng(0)
    cloud, share = np.zeros((batch, 2, points, 3), np.float32), []
    for h in range(2):
        a, b, c = (pair[h][faces[h][:, k]] for k in range(3))
        front = faces[h][(np.cross(b - a, c - a) * (a + b + c)).sum(-1) < 0]
        share.append(len(front) / len(faces[h]))
        seen = np.unique(front)
        cloud[:, h] = pair[h][rng.choice(seen, (batch, points))] + rng.normal(0, 0.001, (batch, points, 3))
    verts = (pair[None] + rng.uniform(-0.0115, 0.0115, (batch, 2, 1, 3))).astype(np.float32)
    return torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(cloud).to(dev), float(np.mean(share))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--batches', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench import make_opt
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer, refined_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    dev = torch.device('cuda', 0)
    verts, faces, cloud, facing = template_scene(args.batch, args.points, dev)
    call_ms, res = {}, {}
    for iters in (0, 8):
        for rigid in (False, True):
            key = "iters%d_%s" % (iters, 'rigid' if rigid else 'translation')
            call_ms[key] = round(device_ms(lambda: F.mesh_icp(verts, faces, cloud, iters=iters, rigid=rigid)), 3)
            out = F.mesh_icp(verts, faces, cloud, iters=iters, rigid=rigid)
            res[key] = round(float(out[3].mean()) * 1000, 3)
    pen_ms = device_ms(lambda: F.mesh_penetration(verts, faces))

    opt = make_opt(args.res)
    torch.manual_seed(0)
    model = load_model_intag(opt).to(dev)
    consts = synthetic_loss_constants()
    tr = Trainer(opt, model, CtdetLoss(opt, consts).to(dev), lr=0.0)
    loader = [to_device(synthetic_train_batch(args.batch, args.res, seed=1 + i, consts=consts), dev) for i in range(args.batches)]
    modes = (False, True, 'rigid')
    ms = {m: [] for m in modes}
    for rep in range(args.reps + 1):                           # rep 0 = warm-up
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = tr.evaluation(loader, dev, refined=m)
            if rep:
                ms[m].append((time.perf_counter() - t0) * 1e3)
    mwl = tr.model_with_loss
    mwl.eval()
    with torch.no_grad():
        tup = mwl(loader[0], 'test', None)
    sums_ms = {m: device_ms(lambda: refined_sums(tup, loader[0], mwl.loss.faces_pair, m == 'rigid')) for m in (True, 'rigid')}
    med = lambda v: sorted(v)[len(v) // 2]
    line = json.dumps({"batch": args.batch, "points": args.points, "batches": args.batches, "facing_share": round(facing, 4),
                       "mesh_icp_ms": call_ms, "rms_mm": res, "mesh_penetration_ms": round(pen_ms, 3),
                       "refined_sums_ms_per_batch": round(sums_ms[True], 3), "refined_sums_rigid_ms_per_batch": round(sums_ms['rigid'], 3),
                       "evaluation_ms": [round(x, 2) for x in ms[False]], "evaluation_refined_ms": [round(x, 2) for x in ms[True]],
                       "evaluation_refined_rigid_ms": [round(x, 2) for x in ms['rigid']], "median_ms": round(med(ms[False]), 2),
                       "median_refined_ms": round(med(ms[True]), 2), "median_refined_rigid_ms": round(med(ms['rigid']), 2),
                       "added_ms_per_batch": round((med(ms[True]) - med(ms[False])) / args.batches, 3),
                       "added_rigid_ms_per_batch": round((med(ms['rigid']) - med(ms[False])) / args.batches, 3),
                       **{k: ev[k] for k in ('cloud_res_mm', 'ref_cloud_res_mm', 'refined_samples') if k in ev}})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
