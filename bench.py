"""Flagship training benchmark — driver contract (see repo instructions).

Measures training graphs/sec (whole job) for the 8-layer/256-dim PERT-GNN on
synthetic Alibaba-shaped call graphs, one process
per GPU over RCCL.  A plain run does only what that headline figure needs:
set up, warm up, time the steps, print one JSON result line.  `--full` also
appends the latency-MAE anchor (the second half of the BASELINE metric) from a
short training run on an ingested synthetic dataset.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 bench.py --gpus 8 --steps 20 --warmup 5

(`python bench.py --gpus 8` without torchrun re-execs itself under
torch.distributed.run with 8 local ranks.)

`--dump-outputs DIR` writes what the last timed step computed (loss,
predictions, gradients, updated parameters) as DIR/<name>.npy.  The batches and
the initial weights are seeded, and with this option the last timed step starts
again from that seeded initial model/optimizer state: the training kernels sum
with atomics, and Adam's first steps amplify that 1-ulp ordering noise into a
trajectory that differs from run to run, so only a step from a fixed state can
be compared output for output between runs or builds.  The step itself, and
what is timed, are the same with or without the option.

Batches are pre-collated once and held resident on HBM (the north-star
"graph-shard prefetch sized for 288 GB"); every timed step is a FULL training
step: forward + quantile loss + backward + DDP all-reduce + Adam update.

hipGraph stepping modes (--graph-mode):
  * full  — the whole step, collectives included, is captured and replayed.
  * split — fwd+loss+bwd captured; gradient all-reduce + Adam run eagerly
    after each replay.  The capture then contains no RCCL ops, so it cannot
    depend on collective-capture support; the eager comm tail costs ~3
    launches + one all-reduce of the flat grad buffer (~0.2 ms at 8L/256H
    over xGMI) — the safe default for world_size > 1.
  * eager — no capture.
  * auto  — full at world_size 1, split otherwise; every rank's chosen mode
    is min-reduced so all ranks step the same way even if capture fails on
    only some of them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch


def vocab_cfg(name: str, seed: int):
    """Synthetic scale presets: 'small' is the round-1 config;
    'realistic' approximates Alibaba-2021 vocabulary scale (reference scans
    thousands of interfaces / hundreds of entries over 100k traces,
    /root/reference/pert_gnn.py:298-299,325-328) — it exercises the grouped
    table-gradient scatters (embedding tables far beyond LDS capacity) and
    gives every batch a diverse pool of entry-union samples."""
    from pertgnn.data.synthetic import SyntheticConfig

    if name == "realistic":
        return SyntheticConfig(
            n_entries=320, patterns_per_entry=3, traces_per_entry=4,
            min_calls=8, max_calls=28, n_microservices=1024,
            n_interfaces=2048, seed=seed,
        )
    return SyntheticConfig(
        n_entries=8, patterns_per_entry=3, traces_per_entry=4,
        min_calls=8, max_calls=28, n_microservices=96, seed=seed,
    )


def build_synthetic_batches(n_batches: int, graphs_per_batch: int, seed: int,
                            device, vocab: str = "small") -> tuple[list, dict]:
    """Trace-scale synthetic PERT graphs -> pre-collated GPU-resident batches."""
    from pertgnn.data.collate import collate_native as collate
    from pertgnn.data.graphs import build_pert_graph
    from pertgnn.data.dataset import TraceSample

    from pertgnn.data.synthetic import generate_traces

    cfg = vocab_cfg(vocab, seed)
    call_df, resource_df = generate_traces(cfg)
    # factorize to int ids the way ingest does (vectorized, minimal)
    import pandas as pd

    for col in ("um", "dm"):
        call_df[col] = call_df[col].astype(str)
    ms_vals = pd.concat([call_df["um"], call_df["dm"]])
    codes, _ = pd.factorize(ms_vals)
    call_df["um"] = codes[: len(call_df)]
    call_df["dm"] = codes[len(call_df):]
    call_df["interface"] = pd.factorize(call_df["interface"])[0]
    call_df["rpctype"] = pd.factorize(call_df["rpctype"])[0]
    call_df["endTimestamp"] = call_df["timestamp"] + call_df["rt"].abs()

    # one PERT pattern-union per entry: concat all pattern graphs of the entry
    rng = torch.Generator().manual_seed(seed)
    entries = {}
    for (tid), tdf in call_df.groupby("traceid"):
        g = build_pert_graph(tdf)
        key = int(tdf["dm"].iloc[0])  # entry microservice identity
        entries.setdefault(key, []).append(g)

    samples = []
    for eid, (key, graphs) in enumerate(sorted(entries.items())):
        graphs = graphs[:3]
        nn = [g["num_nodes"] for g in graphs]
        offs = [0]
        for v in nn[:-1]:
            offs.append(offs[-1] + v)
        ei = torch.cat([g["edge_index"] + o for g, o in zip(graphs, offs)], dim=1)
        ea = torch.cat([g["edge_attr"] for g in graphs], dim=0)
        cat_X = torch.cat([g["ms_id"] for g in graphs], dim=0)
        nd = torch.cat([g["node_depth"] for g in graphs], dim=0)
        pnn = torch.tensor([[v] for v in nn for _ in range(v)], dtype=torch.float)
        probs = torch.full((sum(nn), 1), 1.0 / len(graphs))
        x = torch.rand(sum(nn), 9, generator=rng)
        samples.append(TraceSample(
            x=x, edge_index=ei, edge_attr=ea, cat_X=cat_X, node_depth=nd,
            pattern_num_nodes=pnn, pattern_probs=torch.full((len(graphs), 1), 1.0 / len(graphs)),
            rt_probs=probs, entry_id=torch.tensor([eid]),
            y=torch.rand((), generator=rng) * 100,
        ))

    batches = []
    idx = torch.randint(0, len(samples), (n_batches, graphs_per_batch), generator=rng)
    for bi in range(n_batches):
        batch = collate([samples[i] for i in idx[bi]])
        batches.append(batch.to(device) if device.type == "cuda" else batch)
    stats = {
        "avg_nodes": sum(b.x.shape[0] for b in batches) / len(batches),
        "avg_edges": sum(b.edge_index.shape[1] for b in batches) / len(batches),
        "distinct_unions": len(samples),
        "cat_max": max(int(b.cat_X.max()) for b in batches),
        "entry_max": max(int(b.entry_id.max()) for b in batches),
        "ifc_max": max(int(b.edge_attr[:, 0].max()) for b in batches),
        "rpc_max": max(int(b.edge_attr[:, 1].max()) for b in batches),
    }
    return batches, stats


def measure_latency_mae(epochs: int, device, seed: int = 7) -> dict:
    """The accuracy half of the BASELINE metric: ingest a synthetic
    Alibaba-shaped dataset through the full offline pipeline, train the
    reference-default-shaped model (2 effective convs, H=32) for a few
    epochs, and report the final test latency-MAE (reference epoch metric,
    /root/reference/pert_gnn.py:290-294,348-350)."""
    import tempfile

    from pertgnn.data.collate import BatchLoader, collate_native
    from pertgnn.data.dataset import build_data_list, split_60_20_20
    from pertgnn.data.ingest import run_ingest
    from pertgnn.data.synthetic import SyntheticConfig, write_dataset
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train import evaluate, train_epoch
    from pertgnn.train.optim import FusedAdam

    torch.manual_seed(seed)
    with tempfile.TemporaryDirectory() as root:
        cfg = SyntheticConfig(n_entries=12, traces_per_entry=400, seed=seed)
        write_dataset(root, cfg)
        pdir = os.path.join(root, "processed")
        run_ingest(data_root=os.path.join(root, "data"), processed_dir=pdir,
                   verbose=False)
        import joblib
        import pandas as pd

        tr2data = torch.load(os.path.join(pdir, "tr2data.pt"), weights_only=False)
        runtime2graph = torch.load(os.path.join(pdir, "runtime2pertgraph_map.pt"),
                                   weights_only=False)
        entry2runtimes = joblib.load(os.path.join(pdir, "entry2runtimes.joblib"))
        resource_df = pd.read_csv(os.path.join(pdir, "processed_resource_df.csv"))
        resource_df["msname"] = resource_df["msname"].astype(int)
        data_list = build_data_list(tr2data, entry2runtimes, runtime2graph,
                                    resource_df)
    train_list, _valid, test_list = split_60_20_20(data_list)
    train_loader = BatchLoader(train_list, 170, shuffle=True, seed=seed,
                               collate_fn=collate_native)
    test_loader = BatchLoader(test_list, 170, shuffle=False,
                              collate_fn=collate_native)
    unique_ms_max = max(int(g["ms_id"].max()) for g in runtime2graph.values())
    entry_id_max = max(int(s.entry_id) for s in data_list)
    interface_id_max = max(int(s.edge_attr[:, 0].max()) for s in data_list)
    rpctype_id_max = max(int(s.edge_attr[:, 1].max()) for s in data_list)
    model = SAGEDeterministic(9, [unique_ms_max + 1], entry_id_max,
                              interface_id_max, rpctype_id_max, 32, 1, 0.0)
    model = model.to(device)
    optimizer = FusedAdam(model.parameters(), lr=3e-3)
    for _ in range(epochs):
        train_epoch(model, train_loader, optimizer, 0.5, device)
    mae, mape, _q = evaluate(model, test_loader, 0.5, device)
    return {"latency_mae": mae, "mae_epochs": epochs,
            "mae_dataset_traces": len(data_list), "mae_model": "2conv/32H"}


# --dump-outputs budget: every array is float32, at most _DUMP_MAX_ELEMS
# elements each (5 arrays -> <= 40 MB in all, under the 64 MB cap)
_DUMP_MAX_ELEMS = 2 * 1024 * 1024
_DUMP_SAMPLE_SEED = 20230806


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """Write each tensor as out_dir/<name>.npy (float32).  An array above the
    per-array budget is reduced to a fixed, seeded sample of its flattened
    elements (sorted indices — the same elements in every run)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        a = np.ascontiguousarray(a).reshape(-1) if a.ndim == 0 else a
        if a.size > _DUMP_MAX_ELEMS:
            rng = np.random.default_rng(_DUMP_SAMPLE_SEED)
            idx = np.sort(rng.choice(a.size, _DUMP_MAX_ELEMS, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--batch-size", type=int, default=1024, help="graphs per GPU per step")
    ap.add_argument("--n-batches", type=int, default=4, help="distinct resident batches to cycle")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--precision", choices=["fp32", "bf16", "fp16"], default="bf16",
                    help="matmul compute precision (weights/activations stay fp32)")
    ap.add_argument("--vocab", choices=["small", "realistic"], default="realistic",
                    help="synthetic vocabulary scale (realistic = Alibaba-like: "
                         "2k interfaces / 1k microservices / 256 entry-unions)")
    ap.add_argument("--graph-mode", choices=["auto", "full", "split", "eager"],
                    default="auto", help="hipGraph stepping mode (see module doc)")
    ap.add_argument("--no-hipgraph", action="store_true",
                    help="disable hipGraph capture of the training step (= --graph-mode eager)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure "
                         "(the latency-MAE anchor probe)")
    ap.add_argument("--mae-epochs", type=int, default=25,
                    help="epochs for the latency-MAE anchor probe under "
                         "--full (0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed step's "
                         "outputs as DIR/<name>.npy (float32)")
    args = ap.parse_args()

    # `--gpus N` without a torchrun rendezvous: re-exec under
    # torch.distributed.run with N local ranks (the flag is then authoritative)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        os.execv(sys.executable, [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", f"--nproc-per-node={args.gpus}",
            "--master-addr", "127.0.0.1", "--master-port", "29531",
            os.path.abspath(__file__), *sys.argv[1:],
        ])

    from pertgnn.models import SAGEDeterministic
    from pertgnn.ops import functional as F
    from pertgnn.parallel import Comm
    from pertgnn.train.optim import FlatGradAllReduce, FusedAdam

    from pertgnn.ops.functional import set_gemm_precision

    comm = Comm()
    if args.gpus > 1 and comm.world_size != args.gpus and comm.rank == 0:
        print(f"# note: --gpus {args.gpus} but WORLD_SIZE={comm.world_size}; "
              "the rendezvous world size is authoritative", file=sys.stderr)
    on_gpu = torch.cuda.is_available()
    if on_gpu:
        set_gemm_precision(args.precision)
    device = comm.device if on_gpu else torch.device("cpu")
    torch.manual_seed(1234 + comm.rank)

    batches, stats = build_synthetic_batches(
        args.n_batches, args.batch_size, seed=100 + comm.rank, device=device,
        vocab=args.vocab,
    )
    # vocab sizes must agree across ranks (per-rank synthetic seeds differ)
    for key in ("cat_max", "entry_max", "ifc_max", "rpc_max"):
        stats[key] = int(comm.all_reduce_scalar(float(stats[key]), op="max"))

    model = SAGEDeterministic(
        9, [stats["cat_max"] + 1], stats["entry_max"], stats["ifc_max"],
        stats["rpc_max"], args.hidden, args.layers, 0.0,
    ).to(device)
    comm.broadcast_module_(model)
    optimizer = FusedAdam(model.parameters(), lr=args.lr)
    engine = FlatGradAllReduce(optimizer, comm) if comm.distributed else None

    model.train()

    # --dump-outputs: the seeded initial training state (weights, Adam moments
    # and step counters, BN running statistics), put back in place before the
    # last timed step so that step's inputs are the same in every run
    snapshot = None
    if args.dump_outputs:
        state = [optimizer.flat_param, optimizer.exp_avg, optimizer.exp_avg_sq,
                 optimizer.dev_state, *model.buffers()]
        snapshot = ([(t, t.detach().clone()) for t in state], optimizer.step_count)

    @torch.no_grad()
    def restore_snapshot():
        for t, t0 in snapshot[0]:
            t.copy_(t0)
        optimizer.step_count = snapshot[1]

    def step_compute(i):
        """zero_grad + forward + loss + backward (no collectives unless the
        engine hooks are enabled)."""
        b = batches[i % len(batches)]
        optimizer.zero_grad(set_to_none=False)
        gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                       b.pattern_num_nodes, b.rt_probs, b.entry_id, b.batch,
                       csr=b.csr, num_graphs=b.num_graphs)
        loss = F.quantile_loss(b.y, gp.flatten(), args.tau)
        loss.backward()
        # detached: holding the outputs must not keep the autograd graph (and
        # the activations it saved) alive past the step
        return loss.detach(), gp.detach(), lp.detach()

    def step(i):
        """Full eager training step (bucketed all-reduce overlapped with
        backward via the engine hooks)."""
        if engine is not None:
            engine.reset()
        outs = step_compute(i)
        if engine is not None:
            engine.finalize()
        optimizer.step()
        return outs

    mode = "eager" if args.no_hipgraph else args.graph_mode
    if mode == "auto":
        mode = "full" if comm.world_size == 1 else "split"
    if not on_gpu:
        mode = "eager"

    # hipGraph capture (guide: capture launch-bound inner loops).  Each rank
    # reports the capture level it achieved (2=full, 1=split, 0=eager) and
    # the MINIMUM over ranks decides the common stepping mode — a rank that
    # failed capture must not leave the others replaying graphs alone.
    def try_capture(body):
        for i in range(len(batches)):
            body(i)  # allocation warmup per batch shape
        torch.cuda.synchronize()
        gobjs = []
        gouts = []  # each graph's static (loss, gp, lp), refilled per replay
        pool = None
        for i in range(len(batches)):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                outs = body(i)
            if pool is None:
                pool = g.pool()
            gobjs.append(g)
            gouts.append(outs)
        torch.cuda.synchronize()
        return gobjs, gouts

    timed_step = step
    level = 0
    gobjs = gouts = None
    if mode == "full":
        try:
            gobjs, gouts = try_capture(step)
            level = 2
        except Exception as exc:  # pragma: no cover - hardware path
            print(f"# full-step hipGraph capture unavailable ({exc}); "
                  "trying compute-only capture", file=sys.stderr)
            mode = "split"
    if mode == "split" and level == 0:
        try:
            if engine is not None:
                engine.enabled = False
            try:
                gobjs, gouts = try_capture(step_compute)
            finally:
                if engine is not None:
                    engine.enabled = True
            level = 1
        except Exception as exc:  # pragma: no cover - hardware path
            print(f"# compute hipGraph capture unavailable ({exc}); "
                  "stepping eagerly", file=sys.stderr)
    if mode == "eager":
        level = 0

    level = int(comm.all_reduce_scalar(float(level), op="min"))
    if level == 2:
        def timed_step(i):
            gobjs[i % len(gobjs)].replay()
            return gouts[i % len(gobjs)]
    elif level == 1:
        inv_ws = 1.0 / comm.world_size

        def timed_step(i):
            gobjs[i % len(gobjs)].replay()
            if comm.distributed:
                comm.all_reduce_(optimizer.flat_grad)
                optimizer.flat_grad.mul_(inv_ws)
            optimizer.step()
            return gouts[i % len(gobjs)]
    else:
        timed_step = step
    mode_used = {2: "full", 1: "split", 0: "eager"}[level]

    for i in range(args.warmup):
        timed_step(i)

    comm.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        if snapshot is not None and i == args.steps - 1:
            restore_snapshot()
        last = timed_step(args.warmup + i)
    comm.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    # max over ranks
    elapsed = comm.all_reduce_scalar(elapsed, op="max")

    # what the last timed step handed back: loss + predictions, and the
    # gradients / updated parameters it left in the optimizer's flat buffers
    if args.dump_outputs and comm.rank == 0 and last is not None:
        loss, gp, lp = last
        dump_outputs(args.dump_outputs, {
            "loss": loss, "global_predict": gp, "local_predict": lp,
            "flat_grad": optimizer.flat_grad, "flat_param": optimizer.flat_param,
        })

    # latency-MAE anchor, --full only (rank 0 only; the other ranks idle at
    # the final barrier) — skipped on CPU to keep the no-GPU run fast
    mae_info = {"latency_mae": None}
    if args.full and args.mae_epochs > 0 and on_gpu and comm.rank == 0:
        try:
            mae_info = measure_latency_mae(args.mae_epochs, device)
        except Exception as exc:  # pragma: no cover
            print(f"# latency-MAE probe failed: {exc}", file=sys.stderr)

    graphs_per_sec = args.batch_size * comm.world_size * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1e3
    if comm.rank == 0:
        print(json.dumps({
            "metric": "training graphs/sec (whole node)",
            "value": graphs_per_sec,
            "unit": "graphs/s",
            "n_gpus": comm.world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.precision if on_gpu else "fp32",
            "data": "synthetic",
            "latency_mae": mae_info.get("latency_mae"),
            "mae_detail": {k: v for k, v in mae_info.items() if k != "latency_mae"},
            "config": {
                "model": f"PERT-GNN {args.layers}L/{args.hidden}H",
                "global_batch": args.batch_size * comm.world_size,
                "avg_nodes_per_batch": stats["avg_nodes"],
                "avg_edges_per_batch": stats["avg_edges"],
                "vocab": args.vocab,
                "interfaces": stats["ifc_max"] + 1,
                "entry_unions": stats["distinct_unions"],
                "graph_mode": mode_used,
                "parallelism": f"dp{comm.world_size}",
            },
        }))
    comm.finalize()


if __name__ == "__main__":
    main()
