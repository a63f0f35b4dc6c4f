"""Time Trainer.evaluation with and without the inter-hand metrics on the synthetic loader (256x256, B = 32), and its parts alone:
`python tools/eval_interaction_time.py [--batches 2] [--reps 3] [--out profiles/eval_interaction_time.json]` -> one JSON line (also written to
--out).  The two modes alternate inside one process after a warm-up of each; every timing of `evaluation` ends in its own host sync (it
returns floats).  The parts -- the model's test-mode pass, `interaction_sums`, one `F.mesh_penetration` launch -- are timed with device events
over 20 calls on one batch."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def device_ms(fn, calls=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--batches', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench import make_opt
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer, interaction_sums
    from pdfnet_amd.trains.simplified import CtdetLoss
    dev = torch.device('cuda', 0)
    opt = make_opt(args.res)
    torch.manual_seed(0)
    model = load_model_intag(opt).to(dev)
    consts = synthetic_loss_constants()
    tr = Trainer(opt, model, CtdetLoss(opt, consts).to(dev), lr=0.0)
    loader = [to_device(synthetic_train_batch(args.batch, args.res, seed=1 + i, consts=consts), dev) for i in range(args.batches)]
    ms = {False: [], True: []}
    for rep in range(args.reps + 1):                           # rep 0 = warm-up
        for interaction in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = tr.evaluation(loader, dev, interaction=interaction)
            if rep:
                ms[interaction].append((time.perf_counter() - t0) * 1e3)
    mwl = tr.model_with_loss
    mwl.eval()
    faces = mwl.loss.faces_pair
    with torch.no_grad():
        tup = mwl(loader[0], 'test', None)
        model_ms = device_ms(lambda: mwl(loader[0], 'test', None), calls=5)
    sums_ms = device_ms(lambda: interaction_sums(tup, loader[0], faces))
    kernel_ms = device_ms(lambda: F.mesh_penetration(tup[0], faces))
    med = lambda v: sorted(v)[len(v) // 2]
    line = json.dumps({"batch": args.batch, "res": args.res, "batches": args.batches, "evaluation_ms": [round(x, 2) for x in ms[False]],
                       "evaluation_interaction_ms": [round(x, 2) for x in ms[True]], "median_ms": round(med(ms[False]), 2),
                       "median_interaction_ms": round(med(ms[True]), 2),
                       "added_ms_per_batch": round((med(ms[True]) - med(ms[False])) / args.batches, 3),
                       "test_mode_pass_ms_per_batch": round(model_ms, 3), "interaction_sums_ms_per_batch": round(sums_ms, 3),
                       "mesh_penetration_ms_per_launch": round(kernel_ms, 3), "launches_per_batch": 2,
                       **{k: ev[k] for k in ('mrrpe_mm', 'pen_ratio', 'pen_depth_mm', 'contact_mm', 'interaction_samples')}})
    print(line)
    if args.out:
        with open(args.out, 'w') as fo:
            fo.write(line + '\n')


if __name__ == "__main__":
    main()
