"""Time Trainer.evaluation with and without the aligned metrics on the synthetic loader (256x256, B = 32), and the aligned part alone:
`python tools/eval_aligned_time.py [--batches 2] [--reps 3]` -> one JSON line.  The two modes alternate inside one process after a warm-up
of each; every timing ends in the evaluation's own host sync (it returns floats)."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--batches', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    from bench import make_opt
    from pdfnet_amd.networks.intaghand_model import load_model_intag
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from pdfnet_amd.trains.base_trainer import Trainer, aligned_sums
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
        for aligned in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev = tr.evaluation(loader, dev, aligned=aligned)
            if rep:
                ms[aligned].append((time.perf_counter() - t0) * 1e3)
    tr.model_with_loss.eval()
    with torch.no_grad():
        tup = tr.model_with_loss(loader[0], 'test', None)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    aligned_sums(tup)
    e0.record()
    for _ in range(20):
        aligned_sums(tup)
    e1.record()
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"batch": args.batch, "res": args.res, "batches": args.batches, "evaluation_ms": [round(x, 2) for x in ms[False]],
                      "evaluation_aligned_ms": [round(x, 2) for x in ms[True]], "median_ms": round(med(ms[False]), 2),
                      "median_aligned_ms": round(med(ms[True]), 2), "aligned_sums_ms_per_batch": round(e0.elapsed_time(e1) / 20, 3),
                      "pa_mpjpe_mm": ev['pa_mpjpe_mm'], "f15": ev['f15'], "auc_joints": ev['auc_joints']}))


if __name__ == "__main__":
    main()
