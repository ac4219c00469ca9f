"""Head-count probe at the flagship shape (8 layers, 256 hidden, bf16,
1024-graph batches, realistic vocab): for every head count in ``--heads``

  (t) train   — ms per captured training step (``GraphStepper``, full capture)
  (p) predict — ms per captured ``Predictor`` forward

All head counts and both modes run in ONE process and alternate per
repetition, so they see the same machine state; each window ends in a device
synchronise.  The order of the head counts ROTATES from one repetition to
the next (with ``--reps`` equal to the number of head counts every head count
is timed once in every position): a window's time depends on what ran just
before it, and a fixed order would book that to the head count.  Prints one
JSON line (and writes it to ``--out``); ``position`` is the window's place in
its repetition.

``--profile`` is the form to put under ``rocprofv3 --kernel-trace --stats``
(one head count per run): a few EAGER training steps and Predictor forwards,
no timing.  The four attention kernels show up by name
(``edge_attn_fused_{fwd,infer,bwd_row,bwd_col}_kernel``).

    python benchmarks/heads_probe.py [--heads 1,2,4,8] [--reps 4] [--iters 30]
"""
import argparse
import copy
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import bench as bench_mod  # noqa: E402
from pertgnn.infer import Predictor  # noqa: E402
from pertgnn.models import SAGEDeterministic  # noqa: E402
from pertgnn.ops.functional import set_gemm_precision  # noqa: E402
from pertgnn.train.capture import GraphStepper  # noqa: E402
from pertgnn.train.optim import FusedAdam  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--vocab", default="realistic")
    ap.add_argument("--profile", action="store_true",
                    help="eager steps only, for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    assert torch.cuda.is_available(), "heads_probe measures on a GPU only"
    dev = torch.device("cuda:0")
    heads_list = [int(x) for x in args.heads.split(",")]
    set_gemm_precision(args.precision)
    batches, stats = bench_mod.build_synthetic_batches(
        2, args.batch, seed=0, device=dev, vocab=args.vocab)

    def build(heads):
        torch.manual_seed(0)
        model = SAGEDeterministic(
            9, [stats["cat_max"] + 1], stats["entry_max"], stats["ifc_max"],
            stats["rpc_max"], args.hidden, args.layers, 0.0,
            heads=heads).to(dev)
        infer_model = copy.deepcopy(model)
        model.train()
        opt = FusedAdam(model.parameters(), lr=3e-4)
        stepper = GraphStepper(model, opt, None, None, 0.5, dev, batches)
        predictor = Predictor(infer_model)
        return stepper, predictor

    if args.profile:
        for h in heads_list:
            stepper, predictor = build(h)
            for i in range(6):
                stepper._full_step(i % 2)
            for i in range(6):
                predictor.predict_batch(batches[i % 2])
            torch.cuda.synchronize()
        print("profile pass done: heads", heads_list)
        return

    runs = {}
    for h in heads_list:
        stepper, predictor = build(h)
        mode = stepper.capture()
        assert mode == "full", mode
        assert predictor.capture(batches) == "graph"
        runs[h] = {
            "t": lambda i, s=stepper: s._graphs[i % 2].replay(),
            "p": lambda i, p=predictor: p.replay(i % 2),
            "keep": (stepper, predictor),
        }
    for h in heads_list:  # warm every path
        for m in "tp":
            for i in range(args.warmup):
                runs[h][m](i)
    torch.cuda.synchronize()

    times = {h: {"t": [], "p": []} for h in heads_list}
    places = {h: [] for h in heads_list}
    for r in range(args.reps):
        k = r % len(heads_list)
        order = heads_list[k:] + heads_list[:k]
        for pos, h in enumerate(order):
            places[h].append(pos)
        for m in "tp":
            for h in order:
                fn = runs[h][m]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    fn(i)
                torch.cuda.synchronize()
                times[h][m].append(
                    (time.perf_counter() - t0) / args.iters * 1e3)

    res = {
        "shape": {"layers": args.layers, "hidden": args.hidden,
                  "precision": args.precision, "graphs_per_batch": args.batch,
                  "vocab": args.vocab,
                  "nodes": [int(b.x.shape[0]) for b in batches],
                  "edges": [int(b.edge_index.shape[1]) for b in batches]},
        "reps": args.reps, "iters": args.iters, "heads": {},
    }
    for h in heads_list:
        entry = {"position": places[h]}
        for m, name in (("t", "train_step"), ("p", "predict")):
            ts = times[h][m]
            entry[name] = {"ms": ts, "median_ms": statistics.median(ts),
                           "min_ms": min(ts), "max_ms": max(ts)}
        res["heads"][str(h)] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
