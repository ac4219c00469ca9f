"""Inference probe at the flagship shape (8 layers, 256 hidden, bf16,
1024-graph batches, realistic vocab): ms per batch of

  (a) model   — ``model.eval()`` + the training forward (the pre-Predictor path)
  (b) eager   — ``pertgnn.infer.Predictor.predict_batch``
  (c) graph   — the same Predictor, captured (``capture`` + ``replay``)

All three run in ONE process, alternating a/b/c per repetition, so they see
the same machine state; each window ends in a device synchronise.  Prints
one JSON line (and writes it to ``--out``).  ``--only b --reps 1`` is the
form to put under ``rocprofv3 --kernel-trace --stats``.

    python benchmarks/infer_probe.py [--reps 3] [--iters 30] [--out FILE]
"""
import argparse
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--vocab", default="realistic")
    ap.add_argument("--only", default="abc",
                    help="subset of modes to run, e.g. 'b' for a profile")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    assert torch.cuda.is_available(), "infer_probe measures on a GPU only"
    dev = torch.device("cuda:0")
    set_gemm_precision(args.precision)
    batches, stats = bench_mod.build_synthetic_batches(
        2, args.batch, seed=0, device=dev, vocab=args.vocab)
    torch.manual_seed(0)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], args.hidden,
                              args.layers, 0.0).to(dev)
    model.eval()
    predictor = Predictor(model)

    def run_model(i):
        b = batches[i % 2]
        gp, _ = model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                      b.pattern_num_nodes, b.rt_probs, b.entry_id, b.batch,
                      csr=b.csr, num_graphs=b.num_graphs)
        return gp.flatten()

    def run_eager(i):
        return predictor.predict_batch(batches[i % 2])

    def run_graph(i):
        return predictor.replay(i % 2)

    modes = {"a": ("model", run_model), "b": ("eager", run_eager),
             "c": ("graph", run_graph)}
    order = [m for m in "abc" if m in args.only]

    with torch.no_grad():
        # agreement of the three paths on the timed inputs
        ref_out = [run_model(i).float() for i in range(2)]
        eag_out = [run_eager(i).clone() for i in range(2)]
        if "c" in order:
            assert predictor.capture(batches) == "graph"
        rel = max(float((e - r).abs().max() / r.abs().max().clamp_min(1e-6))
                  for e, r in zip(eag_out, ref_out))
        bitwise = all(torch.equal(run_graph(i), eag_out[i])
                      for i in range(2)) if "c" in order else None

        for m in order:  # warm every path
            for i in range(args.warmup):
                modes[m][1](i)
        torch.cuda.synchronize()

        times = {m: [] for m in order}
        for _ in range(args.reps):
            for m in order:
                fn = modes[m][1]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    fn(i)
                torch.cuda.synchronize()
                times[m].append((time.perf_counter() - t0) / args.iters * 1e3)

    res = {
        "shape": {"layers": args.layers, "hidden": args.hidden,
                  "precision": args.precision, "graphs_per_batch": args.batch,
                  "vocab": args.vocab,
                  "nodes": [int(b.x.shape[0]) for b in batches],
                  "edges": [int(b.edge_index.shape[1]) for b in batches]},
        "reps": args.reps, "iters": args.iters,
        "predictor_vs_model_rel_max_err": rel,
        "graph_bitwise_equals_eager": bitwise,
    }
    for m in order:
        name = modes[m][0]
        ts = times[m]
        res[name] = {
            "ms_per_batch": ts,
            "median_ms": statistics.median(ts),
            "min_ms": min(ts), "max_ms": max(ts),
            "graphs_per_s": args.batch / (statistics.median(ts) * 1e-3),
        }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
