"""Time the mesh-to-cloud loss against the cloud-to-mesh loss: `python tools/mesh_cloud_loss_time.py [--reps 5] [--bench FILE]
[--bench-parent FILE] [--out profiles/mesh_cloud_loss_time.json]` -> one JSON line (also written to --out).  Everything in one process, on the
inputs of tools/cloud_loss_time.py (the template hands at B = 32, P = 1,024, each displaced by up to 2 cm from the surface its cloud was sampled
on).  Device-event times over 20 calls of `F.mesh_cloud_loss` forward with the gradient plus backward and of `F.cloud_mesh_loss` forward with
the gradient plus backward, and of the two forwards alone; they are timed in turn `reps` times and the medians reported, with `ratio` = the new
term over the existing one.  The bar is 2: the yardstick is merged code, from the same run.
--bench / --bench-parent: files holding the JSON line `python bench.py` printed with this change and on the parent commit; their headline
figures are copied into the result side by side."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.cloud_loss_time import bench_line
from tools.icp_time import template_scene
from tools.render_time import device_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--bench', default=None)
    ap.add_argument('--bench-parent', default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from pdfnet_amd import functional as F
    dev = torch.device('cuda', 0)
    verts, faces, cloud, facing = template_scene(args.batch, args.points, dev)
    leaf = verts.clone().requires_grad_()
    up = torch.ones(args.batch, 2, device=dev)

    def both(fn):
        def run():
            leaf.grad = None
            fn(leaf, faces, cloud).backward(up)
        return run
    calls = {'mesh_cloud_forward_backward': both(F.mesh_cloud_loss), 'cloud_mesh_forward_backward': both(F.cloud_mesh_loss),
             'mesh_cloud_forward': lambda: F.mesh_cloud_loss(verts, faces, cloud), 'cloud_mesh_forward': lambda: F.cloud_mesh_loss(verts, faces, cloud)}
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(device_ms(fn))
    med = lambda v: sorted(v)[len(v) // 2]
    loss, inliers, visible = F.mesh_cloud_loss(verts, faces, cloud, return_fields=True)[:3]
    other = F.cloud_mesh_loss(verts, faces, cloud)
    ratio = med(ms['mesh_cloud_forward_backward']) / med(ms['cloud_mesh_forward_backward'])
    line = json.dumps({"batch": args.batch, "points": args.points, "facing_share": round(facing, 4),
                       "mesh_cloud_loss_forward_backward_ms": round(med(ms['mesh_cloud_forward_backward']), 4),
                       "cloud_mesh_loss_forward_backward_ms": round(med(ms['cloud_mesh_forward_backward']), 4),
                       "mesh_cloud_loss_forward_ms": round(med(ms['mesh_cloud_forward']), 4),
                       "cloud_mesh_loss_forward_ms": round(med(ms['cloud_mesh_forward']), 4),
                       "all_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                       "ratio": round(ratio, 4), "ratio_bar": 2.0, "within_bar": bool(ratio <= 2.0),
                       "mesh_cloud_loss_mm2_mean": round(float(loss.mean()) * 1e6, 4), "cloud_mesh_loss_mm2_mean": round(float(other.mean()) * 1e6, 4),
                       "visible_mean": round(float(visible.float().mean()), 1), "inliers_mean": round(float(inliers.float().mean()), 1),
                       "bench": bench_line(args.bench), "bench_parent": bench_line(args.bench_parent)})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
