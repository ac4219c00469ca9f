"""Optimizer probe at the flagship shape (8 layers, 256 hidden, bf16,
1024-graph batches, realistic vocab): what FusedAdam's extended step
(global-norm clipping + decoupled weight decay + learning-rate table, all
three on) costs over the plain one.

  (o) optimizer — µs per ``FusedAdam.step()`` alone, at the flagship model's
      ``flat_param.numel()``, the step captured in a hipGraph and replayed so
      the figure is device time and not launch overhead
  (t) train     — ms per captured training step (``GraphStepper``, full capture)

Plain and extended run in ONE process and alternate per repetition, so they
see the same machine state; each window ends in a device synchronise and the
order rotates from one repetition to the next.  Prints one JSON line (and
writes it to ``--out``).

``--profile`` is the form to put under ``rocprofv3 --kernel-trace --stats``:
a few EAGER optimizer steps of both kinds on the flagship buffers, no timing.
The new kernels show up as ``grad_sumsq_partial_kernel``,
``grad_norm_fold_kernel``, ``adam_tick_ex_kernel`` and ``adam_ex_kernel``
next to ``adam_kernel``.

    python benchmarks/optim_probe.py [--reps 3] [--iters 30]
"""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import bench as bench_mod  # noqa: E402
from pertgnn.models import SAGEDeterministic  # noqa: E402
from pertgnn.ops.functional import set_gemm_precision  # noqa: E402
from pertgnn.train.capture import GraphStepper  # noqa: E402
from pertgnn.train.optim import (FusedAdam, decay_params_of,  # noqa: E402
                                 make_lr_table)

KINDS = ("plain", "extended")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--opt-iters", type=int, default=200,
                    help="optimizer-only replays per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--vocab", default="realistic")
    ap.add_argument("--profile", action="store_true",
                    help="eager optimizer steps only, for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    assert torch.cuda.is_available(), "optim_probe measures on a GPU only"
    dev = torch.device("cuda:0")
    set_gemm_precision(args.precision)
    batches, stats = bench_mod.build_synthetic_batches(
        2, args.batch, seed=0, device=dev, vocab=args.vocab)

    def build(kind):
        torch.manual_seed(0)
        model = SAGEDeterministic(
            9, [stats["cat_max"] + 1], stats["entry_max"], stats["ifc_max"],
            stats["rpc_max"], args.hidden, args.layers, 0.0).to(dev)
        model.train()
        extra = {}
        if kind == "extended":
            extra = dict(
                weight_decay=0.01, decay_filter=decay_params_of(model),
                max_grad_norm=1.0,
                lr_schedule=make_lr_table(3e-4, 100000, "cosine",
                                          warmup_steps=100))
        opt = FusedAdam(model.parameters(), lr=3e-4, **extra)
        return GraphStepper(model, opt, None, None, 0.5, dev, batches)

    steppers = {k: build(k) for k in KINDS}
    numel = steppers["plain"].optimizer.flat_param.numel()

    if args.profile:
        for k in KINDS:
            steppers[k]._full_step(0)  # real gradients in flat_grad
            for _ in range(6):
                steppers[k].optimizer.step()
        torch.cuda.synchronize()
        print("profile pass done: flat_param.numel() =", numel)
        return

    runs = {}
    for k in KINDS:
        s = steppers[k]
        assert s.capture() == "full"
        s._full_step(0)  # leaves real gradients for the optimizer-only graph
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            s.optimizer.step()
        runs[k] = {"o": lambda i, g=g: g.replay(),
                   "t": lambda i, s=s: s._graphs[i % 2].replay(),
                   "keep": (s, g)}
    iters = {"o": args.opt_iters, "t": args.iters}
    for k in KINDS:  # warm every path
        for m in "ot":
            for i in range(args.warmup):
                runs[k][m](i)
    torch.cuda.synchronize()

    times = {k: {"o": [], "t": []} for k in KINDS}
    for r in range(args.reps):
        order = KINDS[r % 2:] + KINDS[:r % 2]
        for m in "ot":
            for k in order:
                fn = runs[k][m]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(iters[m]):
                    fn(i)
                torch.cuda.synchronize()
                times[k][m].append((time.perf_counter() - t0) / iters[m] * 1e3)

    res = {
        "shape": {"layers": args.layers, "hidden": args.hidden,
                  "precision": args.precision, "graphs_per_batch": args.batch,
                  "vocab": args.vocab, "flat_param_numel": numel},
        "reps": args.reps, "iters": iters, "kinds": {},
        "grad_stats": steppers["extended"].optimizer.grad_stats(),
    }
    for k in KINDS:
        entry = {}
        for m, name in (("o", "optimizer_step"), ("t", "train_step")):
            ts = times[k][m]
            entry[name] = {"ms": ts, "median_ms": statistics.median(ts),
                           "min_ms": min(ts), "max_ms": max(ts)}
        res["kinds"][k] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
