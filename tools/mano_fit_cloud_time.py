"""Time the MANO fit against the sensor cloud: `python tools/mano_fit_cloud_time.py [--batch 64] [--points 1024] [--outer 8] [--inner 3]
[--out profiles/mano_fit_cloud_time.json]` -> one JSON line (also written to --out).
Device-event times over 20 calls at B = 64 rows (one hand each) on the synthetic MANO constants (oracle/synth.py) with the star-shaped face list
of tests/mano_fit_cloud_ref.py: every row a state drawn like the tests' (root N(0, 0.5^2), pose N(0, 0.5^2), shape N(0, 1), 0.45 m away), its
cloud P = 1,024 points on the camera-facing surface of that mesh with 1 mm noise, the start that state with the translation moved by 1 cm
and 0.1 rad of pose noise, the start mesh as anchor (weight 0.1).  Timed: `F.mano_fit_cloud` (2 outer + 2 launches), and its parts alone: one
`F.mano_cloud_targets` launch and one `F.mano_fit` launch of `inner` steps against those targets.  Also what the fit reached."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.render_time import device_ms


def scene(batch, points, dev, side='left'):
    """-> constants on the device, faces [Fc, 3], cloud [B, P, 3], init [B, 61]"""
    from oracle.synth import synthetic_mano_consts
    from pdfnet_amd import functional as F
    from tests.mano_fit_cloud_ref import template_faces
    from tests.test_icp_gpu import sample_cloud
    c = {k: v.to(dev).contiguous() for k, v in synthetic_mano_consts(side).items()}
    g = np.random.Generator(np.random.PCG64(0))
    p = np.concatenate((g.normal(0, 0.5, (batch, 3)), g.normal(0, 0.5, (batch, 45)), g.normal(0, 1.0, (batch, 10)),
                        np.tile([0.03, -0.02, 0.45], (batch, 1))), -1)
    pt = torch.from_numpy(p.astype(np.float32)).to(dev)
    gt = F.mano_lbs(c, pt[:, :3].contiguous(), pt[:, 3:48].contiguous(), pt[:, 48:58].contiguous(), pt[:, 58:].contiguous(), side=side)[0]
    faces = template_faces(side)
    cloud = np.stack([sample_cloud(v, faces, points, 100 + b, 0.001) for b, v in enumerate(gt.cpu().double().numpy())])
    init = p.copy()
    init[:, :48] += 0.1 * g.standard_normal((batch, 48))
    shift = g.standard_normal((batch, 3))
    init[:, 58:] += 0.01 * shift / np.linalg.norm(shift, axis=-1, keepdims=True)
    return c, torch.from_numpy(faces).to(dev), torch.from_numpy(cloud).to(dev), torch.from_numpy(init.astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--points', type=int, default=1024)
    ap.add_argument('--outer', type=int, default=8)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from pdfnet_amd import functional as F
    dev = torch.device('cuda', 0)
    c, faces, cloud, init = scene(args.batch, args.points, dev)
    anchor = F.mano_fit_cloud(c, cloud, faces, init, outer=0).verts
    kw = dict(anchor=anchor, anchor_weight=0.1, inner=args.inner)
    fit = F.mano_fit_cloud(c, cloud, faces, init, outer=args.outer, **kw)
    tg, w = F.mano_cloud_targets(anchor, faces, cloud, anchor=anchor, anchor_weight=0.1)[:2]
    ms = {'mano_fit_cloud_ms': device_ms(lambda: F.mano_fit_cloud(c, cloud, faces, init, outer=args.outer, **kw)),
          'mano_cloud_targets_ms': device_ms(lambda: F.mano_cloud_targets(anchor, faces, cloud, anchor=anchor, anchor_weight=0.1)),
          'mano_fit_inner_ms': device_ms(lambda: F.mano_fit(c, tg, weight=w, init=init, iters=args.inner))}
    live = (cloud[..., 2] > 0).sum(-1).clamp(min=1)
    line = json.dumps({"batch": args.batch, "points": args.points, "faces": int(faces.shape[0]), "outer": args.outer, "inner": args.inner,
                       **{k: round(v, 3) for k, v in ms.items()},
                       "rms_mm_first_last": [round(float(fit.rms[i].mean()) * 1000, 4) for i in (0, -1)],
                       "inlier_share_first_last": [round(float((fit.inliers[i] / live).mean()), 4) for i in (0, -1)],
                       "accepted_mean": round(float(fit.info[..., 0].sum(0).float().mean()), 2)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
