"""Quantile-level probe at the flagship shape (8 layers, 256 hidden, bf16,
1024-graph batches, realistic vocab): for every level count in ``--levels``
(1 = the scalar-tau path, Q > 1 = ``[B, Q]`` decoder, summed pinball loss
with per-level sums in the captured graph, rearranged predictions)

  (t) train   — ms per captured training step (``GraphStepper``, full capture)
  (p) predict — ms per captured ``Predictor`` forward

All level counts and both modes run in ONE process and alternate per
repetition, so they see the same machine state; each window ends in a device
synchronise.  The order of the level counts ROTATES from one repetition to
the next: a window's time depends on what ran just before it, and a fixed
order would book that to the level count.  Prints one JSON line (and writes
it to ``--out``); ``position`` is the window's place in its repetition.

``--profile`` is the form to put under ``rocprofv3 --kernel-trace --stats``:
a few EAGER training steps, Predictor forwards and metric calls, no timing.
The per-level launches show up as ``quantile_loss_{fwd,bwd}_kernel`` and
``eval_metrics_kernel`` (Q calls each).

    python benchmarks/quantile_probe.py [--levels 1,3] [--reps 3] [--iters 30]
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
from pertgnn.ops import functional as F  # noqa: E402
from pertgnn.ops.functional import set_gemm_precision  # noqa: E402
from pertgnn.train.capture import GraphStepper  # noqa: E402
from pertgnn.train.optim import FusedAdam  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="1,3")
    ap.add_argument("--reps", type=int, default=3)
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

    assert torch.cuda.is_available(), "quantile_probe measures on a GPU only"
    dev = torch.device("cuda:0")
    q_list = [int(x) for x in args.levels.split(",")]
    set_gemm_precision(args.precision)
    batches, stats = bench_mod.build_synthetic_batches(
        2, args.batch, seed=0, device=dev, vocab=args.vocab)

    def taus_of(q):
        """0.5 alone (the scalar path), else q levels spread over (0, 1)"""
        return 0.5 if q == 1 else tuple((k + 1) / (q + 1) for k in range(q))

    def build(nq):
        torch.manual_seed(0)
        model = SAGEDeterministic(
            9, [stats["cat_max"] + 1], stats["entry_max"], stats["ifc_max"],
            stats["rpc_max"], args.hidden, args.layers, 0.0,
            num_quantiles=nq).to(dev)
        infer_model = copy.deepcopy(model)
        model.train()
        opt = FusedAdam(model.parameters(), lr=3e-4)
        stepper = GraphStepper(model, opt, None, None, taus_of(nq), dev,
                               batches)
        predictor = Predictor(infer_model)
        return stepper, predictor

    if args.profile:
        for nq in q_list:
            stepper, predictor = build(nq)
            for i in range(6):
                stepper._full_step(i % 2)
            for i in range(6):
                pred = predictor.predict_batch(batches[i % 2], rearrange=False)
                if nq > 1:
                    F.quantile_rearrange(pred)
                    F.eval_metrics(batches[i % 2].y, pred, taus_of(nq))
            torch.cuda.synchronize()
        print("profile pass done: levels", q_list)
        return

    runs = {}
    for nq in q_list:
        stepper, predictor = build(nq)
        mode = stepper.capture()
        assert mode == "full", mode
        assert predictor.capture(batches) == "graph"
        runs[nq] = {
            "t": lambda i, s=stepper: s._graphs[i % 2].replay(),
            "p": lambda i, p=predictor: p.replay(i % 2),
            "keep": (stepper, predictor),
        }
    for nq in q_list:  # warm every path
        for m in "tp":
            for i in range(args.warmup):
                runs[nq][m](i)
    torch.cuda.synchronize()

    times = {nq: {"t": [], "p": []} for nq in q_list}
    places = {nq: [] for nq in q_list}
    for r in range(args.reps):
        k = r % len(q_list)
        order = q_list[k:] + q_list[:k]
        for pos, nq in enumerate(order):
            places[nq].append(pos)
        for m in "tp":
            for nq in order:
                fn = runs[nq][m]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    fn(i)
                torch.cuda.synchronize()
                times[nq][m].append(
                    (time.perf_counter() - t0) / args.iters * 1e3)

    res = {
        "shape": {"layers": args.layers, "hidden": args.hidden,
                  "precision": args.precision, "graphs_per_batch": args.batch,
                  "vocab": args.vocab,
                  "nodes": [int(b.x.shape[0]) for b in batches],
                  "edges": [int(b.edge_index.shape[1]) for b in batches]},
        "reps": args.reps, "iters": args.iters, "levels": {},
    }
    for nq in q_list:
        entry = {"position": places[nq]}
        for m, name in (("t", "train_step"), ("p", "predict")):
            ts = times[nq][m]
            entry[name] = {"ms": ts, "median_ms": statistics.median(ts),
                           "min_ms": min(ts), "max_ms": max(ts)}
        res["levels"][str(nq)] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
