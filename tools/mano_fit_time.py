"""Time the MANO fit: `python tools/mano_fit_time.py [--batch 32] [--out profiles/mano_fit_time.json]` -> one JSON line (also written to --out).
Device-event times over 20 calls at B = 32 samples x 2 hands on the synthetic MANO constants (oracle/synth.py): `mano_fit_pair` (one
`F.mano_fit` launch per hand) on noise-free targets drawn like the tests' (root N(0, 0.5^2), pose N(0, 0.5^2), shape N(0, 1), half a metre
away) with iters = 0 (one build of the system), 1 and 20; the same with 2 mm noise at iters = 20; one `F.mano_fit` launch of one hand; and,
as a yardstick, one `pdf_mano_lbs_fwd` + `pdf_mano_lbs_bwd` pair per hand at the same B.  Also what the fits reached (rms residual in mm)."""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.render_time import device_ms


def scene(batch, dev, noise=0.0, pose_std=0.5):
    """-> lbs_consts {'left', 'right'} on the device, generating parameters [B, 2, 61], target meshes [B, 2, 778, 3]"""
    from oracle.synth import synthetic_mano_consts
    from pdfnet_amd import functional as F
    lbs = {s: {k: v.to(dev).contiguous() for k, v in synthetic_mano_consts(s).items()} for s in ('left', 'right')}
    g = np.random.Generator(np.random.PCG64(0))
    p = np.concatenate((g.normal(0, 0.5, (batch, 2, 3)), g.normal(0, pose_std, (batch, 2, 45)), g.normal(0, 1.0, (batch, 2, 10)),
                        np.tile([0.03, -0.02, 0.5], (batch, 2, 1))), -1).astype(np.float32)
    p = torch.from_numpy(p).to(dev)
    v = torch.stack([F.mano_lbs(lbs[s], p[:, h, :3].contiguous(), p[:, h, 3:48].contiguous(), p[:, h, 48:58].contiguous(),
                                p[:, h, 58:].contiguous(), side=s)[0] for h, s in enumerate(('left', 'right'))], 1)
    if noise > 0:
        v = v + torch.from_numpy(g.normal(0, noise, tuple(v.shape)).astype(np.float32)).to(dev)
    return lbs, p, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from pdfnet_amd import functional as F
    from pdfnet_amd.utils import mano_fit_pair
    dev = torch.device('cuda', 0)
    lbs, p, v = scene(args.batch, dev)
    _, _, vn = scene(args.batch, dev, noise=0.002)
    rms = lambda fit, tgt: [round(float(((f.verts - tgt[:, h]) ** 2).sum(-1).mean(-1).sqrt().max()) * 1000, 6) for h, f in enumerate(fit)]
    pair_ms, worst_rms = {}, {}
    for iters in (0, 1, 20):
        pair_ms['iters%d' % iters] = round(device_ms(lambda: mano_fit_pair(lbs, v, iters=iters)), 3)
        worst_rms['iters%d' % iters] = rms(mano_fit_pair(lbs, v, iters=iters), v)
    pair_ms['iters20_noisy'] = round(device_ms(lambda: mano_fit_pair(lbs, vn, iters=20)), 3)
    worst_rms['iters20_noisy'] = rms(mano_fit_pair(lbs, vn, iters=20), vn)
    fit = mano_fit_pair(lbs, v, iters=20)
    one_ms = device_ms(lambda: F.mano_fit(lbs['left'], v[:, 0], side='left', iters=20))

    def lbs_pair():
        for h, s in enumerate(('left', 'right')):
            q = [p[:, h, a:b].contiguous().requires_grad_() for a, b in ((0, 3), (3, 48), (48, 58), (58, 61))]
            out, _ = F.mano_lbs(lbs[s], *q, side=s)
            out.backward(v[:, h])
    line = json.dumps({"batch": args.batch, "hands": 2, "mano_fit_pair_ms": pair_ms, "mano_fit_one_hand_iters20_ms": round(one_ms, 3),
                       "mano_lbs_fwd_bwd_pair_ms": round(device_ms(lbs_pair), 3), "worst_rms_mm_left_right": worst_rms,
                       "accepted_mean": round(float(torch.cat([f.accepted for f in fit]).float().mean()), 2),
                       "rejected_mean": round(float(torch.cat([f.rejected for f in fit]).float().mean()), 2)})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
