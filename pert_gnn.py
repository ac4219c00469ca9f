"""Training entrypoint — CLI-compatible with the reference pert_gnn.py.

Accepts every reference flag verbatim (reference pert_gnn.py:15-34; the dead
flags --use_sage/--runs/--log_steps are accepted-and-ignored for compat,
SURVEY.md §8 quirk 4) plus additive MI355X-framework flags.

Single process:  python pert_gnn.py --graph_type pert --epochs 100
Multi-GPU DDP:   python -m torch.distributed.run --nproc-per-node 8 \
                     --master-addr 127.0.0.1 pert_gnn.py ...
"""
from __future__ import annotations

import argparse
import os

import torch

from pertgnn.data.collate import BatchLoader
from pertgnn.data.dataset import build_data_list, split_60_20_20
from pertgnn.models import SAGEDeterministic
from pertgnn.parallel import Comm
from pertgnn.train.optim import (FlatGradAllReduce, FusedAdam,
                                 decay_params_of, make_lr_table)
from pertgnn.train import evaluate, load_checkpoint, save_checkpoint, train_epoch
from pertgnn.train.checkpoint import check_heads, check_taus
from pertgnn.utils import JsonlLogger


def parse_taus(text):
    """``--taus`` value: comma-separated, 1..8 strictly increasing levels
    in (0, 1)."""
    from pertgnn.ops.reference import check_taus as check_levels

    try:
        return check_levels([float(t) for t in text.split(",")])
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc)) from None


def build_parser():
    parser = argparse.ArgumentParser(description="Alibaba traces")
    # --- reference flags, verbatim (pert_gnn.py:15-33) ---
    parser.add_argument("--device", type=int, default=0)
    parser.add_argument("--log_steps", type=int, default=1)        # dead (compat)
    parser.add_argument("--use_sage", action="store_true")         # dead (compat)
    parser.add_argument("--num_layers", type=int, default=1)
    parser.add_argument("--hidden_channels", type=int, default=32)
    parser.add_argument("--dropout", type=float, default=0)
    parser.add_argument("--lr", type=float, default=0.0003)
    # default None = "not given" (resolved to the reference's 0.5 by
    # resolve_levels), so --taus can tell an explicit --tau apart
    parser.add_argument("--tau", type=float, default=None,
                        help="the quantile level, real number between 0 and 1, 0.5 (median) by default")
    parser.add_argument("--epochs", type=int, default=100)
    parser.add_argument("--runs", type=int, default=10)            # dead (compat)
    parser.add_argument("--batch_size", type=int, default=170)
    parser.add_argument("--graph_type", type=str, default="span", help="span or pert")
    # --- additive framework flags ---
    parser.add_argument("--processed_dir", type=str, default="processed")
    parser.add_argument("--max_traces", type=int, default=100000)
    parser.add_argument("--checkpoint", type=str, default=None,
                        help="path to write/read checkpoints (resume if exists)")
    parser.add_argument("--checkpoint_every", type=int, default=10)
    parser.add_argument("--metrics_jsonl", type=str, default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--synthetic", action="store_true",
                        help="generate a synthetic dataset in-place if processed/ is missing")
    parser.add_argument("--sync_bn", action="store_true",
                        help="exact-parity BatchNorm under DDP (statistics all-reduced)")
    parser.add_argument("--loss_scale", type=str, default="1.0",
                        help="loss scaling (fp16 mode): a float S for static "
                             "scaling (loss*S backward, optimizer unscales) or "
                             "'dynamic' for GradScaler-style scaling with "
                             "device-side overflow skip/backoff/growth")
    parser.add_argument("--precision", choices=["fp32", "bf16", "fp16"], default="fp32",
                        help="matmul compute precision on GPU")
    parser.add_argument("--hipgraph", action="store_true",
                        help="hipGraph-captured training over HBM-resident fixed-"
                             "composition batches (one seeded shuffle; only the "
                             "batch ORDER reshuffles per epoch — documented "
                             "deviation from the reference's per-epoch re-draw)")
    parser.add_argument("--predict", type=str, default=None, metavar="OUT.npy",
                        help="inference mode: load the model from --checkpoint, "
                             "predict the latency of every trace of "
                             "--predict_split, write the float32 predictions "
                             "(split order) with numpy.save, print the split's "
                             "metrics and exit without training; --hipgraph "
                             "replays captured forwards")
    parser.add_argument("--predict_split", default="test",
                        choices=["test", "valid", "train", "all"],
                        help="which split --predict runs over ('all' = train, "
                             "valid, test concatenated)")
    parser.add_argument("--heads", type=int, default=1,
                        help="attention heads per conv (must divide "
                             "--hidden_channels; 1 = the reference model). "
                             "Recorded in the checkpoint: resuming or "
                             "predicting with another value is refused")
    parser.add_argument("--taus", type=parse_taus, default=None,
                        metavar="T1,T2,...",
                        help="quantile levels of ONE model, e.g. 0.5,0.9,0.99 "
                             "(1..8 strictly increasing values in (0, 1)): "
                             "the decoder emits one column per level and "
                             "training minimises the summed pinball loss. "
                             "Not combinable with --tau. Recorded in the "
                             "checkpoint: resuming or predicting with other "
                             "levels is refused")
    parser.add_argument("--fast_eval", action="store_true",
                        help="per-epoch valid/test passes through the inference "
                             "path (pertgnn.infer.Predictor, refreshed after "
                             "every training epoch; captured once over the "
                             "resident eval batches under --hipgraph)")
    parser.add_argument("--weight_decay", type=float, default=0.0,
                        help="decoupled (AdamW) weight decay on the weight "
                             "matrices; embedding tables, BatchNorm affines "
                             "and biases are never decayed")
    parser.add_argument("--clip_grad_norm", type=float, default=None,
                        metavar="N",
                        help="clip the global gradient norm to N (off by "
                             "default)")
    parser.add_argument("--lr_schedule", default="constant",
                        choices=["constant", "linear", "cosine"],
                        help="learning-rate schedule over epochs x batches "
                             "per epoch steps, from --lr down to --min_lr")
    parser.add_argument("--warmup_steps", type=int, default=0,
                        help="linear warm-up from 0 to --lr over this many "
                             "steps")
    parser.add_argument("--min_lr", type=float, default=0.0,
                        help="final rate of the linear and cosine schedules")
    return parser


# the optimizer flags and the value that leaves each of them off
OPTIM_FLAGS = {"weight_decay": 0.0, "clip_grad_norm": None,
               "lr_schedule": "constant", "warmup_steps": 0, "min_lr": 0.0}


def parse_args(argv=None):
    """Parsed arguments with the levels resolved: ``args.tau`` is the scalar
    level (0.5 unless given), ``args.levels`` the tuple of levels of a
    --taus run or None, ``args.levels_given`` whether either flag was
    passed."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.taus is not None and args.tau is not None:
        parser.error("--taus cannot be combined with --tau: give the levels "
                     "of a multi-level model with --taus alone")
    args.levels_given = args.taus is not None or args.tau is not None
    args.levels = args.taus
    if args.levels is not None and len(args.levels) == 1:
        # one level is the scalar run at that level
        args.tau, args.levels = args.levels[0], None
    if args.tau is None:
        args.tau = 0.5
    if args.weight_decay < 0:
        parser.error("--weight_decay must be non-negative")
    if args.clip_grad_norm is not None and not args.clip_grad_norm > 0:
        parser.error("--clip_grad_norm must be positive")
    if args.warmup_steps < 0:
        parser.error("--warmup_steps must be non-negative")
    args.optim_ext = any(getattr(args, k) != v for k, v in OPTIM_FLAGS.items())
    return args


def run_predict(args, model, device, samples):
    """--predict: one pass of ``samples`` through a Predictor over
    HBM-resident batches; writes the predictions and prints the metrics."""
    import numpy as np

    from pertgnn.data.collate import collate_native
    from pertgnn.infer import Predictor
    from pertgnn.ops import functional as ops
    from pertgnn.train.capture import make_resident_batches

    resident = make_resident_batches(samples, args.batch_size, device, 0,
                                     collate_fn=collate_native, shuffle=False)
    predictor = Predictor(model)
    if args.hipgraph:
        mode = predictor.capture(resident)
        print(f"# predict stepping mode: {mode} "
              f"({len(resident)} resident batches)")
    levels, tau = args.levels, args.tau
    nq = len(levels) if levels else 1
    acc = torch.zeros(3 if levels is None else 3 + 2 * nq,
                      dtype=torch.float64, device=device)
    preds = []
    n = 0
    with torch.no_grad():
        for i, b in enumerate(resident):
            pred = (predictor.replay(i) if args.hipgraph
                    else predictor.predict_batch(b))
            if levels is None:
                sums = ops.eval_metrics(b.y, pred, tau)
                for j, v in enumerate(sums):
                    acc[j] += v.double() if torch.is_tensor(v) else v
            else:
                # the metrics of what is written out: the rearranged rows
                acc += ops.eval_metrics(b.y, pred, levels).double()
            preds.append(pred)
            n += b.num_graphs
    out = (torch.cat(preds).cpu() if preds
           else torch.empty((0,) if levels is None else (0, nq),
                            dtype=torch.float32))  # the one host sync
    with open(args.predict, "wb") as f:
        np.save(f, out.numpy().astype(np.float32, copy=False))
    if levels is None:
        mae, mape, qloss = (acc / max(n, 1)).tolist()
        print(f"Predict: n={n}, mae={mae!r}, mape={mape!r}, q loss={qloss!r}")
        return
    from pertgnn.train import QuantileReport

    rep = QuantileReport.from_sums(levels, acc.tolist(), n)
    per_level = ", ".join(
        f"tau={t!r}: q loss={q!r}, coverage={c!r}"
        for t, q, c in zip(rep.taus, rep.qloss, rep.coverage))
    print(f"Predict: n={n}, mae={rep.mae!r}, mape={rep.mape!r}, "
          f"q loss={rep.qloss_total!r}, {per_level}")


def load_artifacts(args, comm=None):
    import joblib
    import pandas as pd

    pdir = args.processed_dir
    if not os.path.isfile(os.path.join(pdir, "tr2data.pt")):
        if args.synthetic:
            # rank 0 generates, everyone else waits at the barrier — all
            # ranks racing to write the same processed/ dir corrupts it
            if comm is None or comm.rank == 0:
                from pertgnn.data.ingest import run_ingest
                from pertgnn.data.synthetic import SyntheticConfig, write_dataset

                root = os.path.dirname(pdir) or "."
                write_dataset(root, SyntheticConfig())
                run_ingest(data_root=os.path.join(root, "data"), processed_dir=pdir, verbose=False)
            if comm is not None:
                comm.barrier()
        else:
            raise FileNotFoundError(
                f"{pdir}/tr2data.pt not found — run `python preprocess.py` first "
                "(or pass --synthetic to generate synthetic data)"
            )
    tr2data = torch.load(os.path.join(pdir, "tr2data.pt"), weights_only=False)
    tr2data = {tr: tr2data[tr] for tr in list(tr2data.keys())[: args.max_traces]}
    runtime2graph = torch.load(
        os.path.join(pdir, f"runtime2{args.graph_type}graph_map.pt"), weights_only=False
    )
    entry2runtimes = joblib.load(os.path.join(pdir, "entry2runtimes.joblib"))
    resource_df = pd.read_csv(os.path.join(pdir, "processed_resource_df.csv"))
    resource_df["msname"] = resource_df["msname"].astype(int)
    return tr2data, entry2runtimes, runtime2graph, resource_df


def main(argv=None):
    args = parse_args(argv)
    shown = argparse.Namespace(**vars(args))
    del shown.levels, shown.levels_given
    if not args.optim_ext:
        # a run without the optimizer flags prints the line it always did
        for k in OPTIM_FLAGS:
            delattr(shown, k)
    del shown.optim_ext
    if shown.taus is None:
        del shown.taus  # a run without --taus prints the line it always did
    print(shown)
    comm = Comm()
    torch.manual_seed(args.seed + comm.rank)
    if args.predict:
        if comm.distributed:
            raise SystemExit("--predict runs in a single process; start it "
                             "without a distributed launcher")
        if not args.checkpoint or not os.path.exists(args.checkpoint):
            raise SystemExit("--predict needs an existing --checkpoint "
                             f"(got {args.checkpoint!r})")
        # loaded once, here: the levels decide the decoder width below
        predict_state = torch.load(args.checkpoint, map_location="cpu",
                                   weights_only=False)
        if not args.levels_given:
            # the levels come from the checkpoint; one without the field
            # means unknown: the default
            saved = predict_state.get("taus")
            if saved is not None and len(saved) > 1:
                args.levels = tuple(float(t) for t in saved)
            elif saved is not None:
                args.tau = float(saved[0])

    if torch.cuda.is_available():
        # reference semantics: single process honors --device (pert_gnn.py:36);
        # under torchrun each rank uses its LOCAL_RANK device
        if comm.distributed:
            device = comm.device
        else:
            device = torch.device(f"cuda:{args.device % torch.cuda.device_count()}")
            torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    tr2data, entry2runtimes, runtime2graph, resource_df = load_artifacts(args, comm)

    cache_path = os.path.join(args.processed_dir, f"full_{args.graph_type}_data_list.pt")
    if os.path.exists(cache_path):
        # accepts our TraceSample caches AND the reference's PyG Data
        # pickles (no PyG needed — shim unpickler, pertgnn/data/pyg_compat)
        from pertgnn.data.pyg_compat import load_data_list_any
        data_list = load_data_list_any(cache_path)
    else:
        data_list = build_data_list(
            tr2data, entry2runtimes, runtime2graph, resource_df, limit=args.max_traces
        )
        if comm.rank == 0:
            torch.save(data_list, cache_path)

    train_list, valid_list, test_list = split_60_20_20(data_list)
    # per-rank shard of the training set; eval sets sharded too (metrics are
    # sum-all-reduced so global averages are exact)
    train_shard = comm.shard(train_list)
    valid_shard = comm.shard(valid_list)
    test_shard = comm.shard(test_list)

    on_gpu = torch.cuda.is_available()
    from pertgnn.data.collate import collate_native
    from pertgnn.data.prefetch import PrefetchLoader

    collate_fn = (lambda samples: collate_native(samples, pin=True)) if on_gpu else collate_native
    train_loader = BatchLoader(train_shard, args.batch_size, shuffle=True,
                               seed=args.seed + comm.rank, collate_fn=collate_fn)
    valid_loader = BatchLoader(valid_shard, args.batch_size, shuffle=False, collate_fn=collate_fn)
    test_loader = BatchLoader(test_shard, args.batch_size, shuffle=False, collate_fn=collate_fn)
    if on_gpu:
        from pertgnn.data.prefetch import ThreadedLoader

        train_loader = PrefetchLoader(ThreadedLoader(train_loader), comm.device)
        valid_loader = PrefetchLoader(ThreadedLoader(valid_loader), comm.device)
        test_loader = PrefetchLoader(ThreadedLoader(test_loader), comm.device)

    # vocab scans (pert_gnn.py:306-328)
    unique_ms_max = max(int(g["ms_id"].max()) for g in runtime2graph.values())
    entry_id_max = max(int(s.entry_id) for s in data_list)
    interface_id_max = max(int(s.edge_attr[:, 0].max()) for s in data_list)
    rpctype_id_max = max(int(s.edge_attr[:, 1].max()) for s in data_list)
    num_features = resource_df.shape[1] - 2  # minus timestamp, msname

    model = SAGEDeterministic(
        num_features + 1, [unique_ms_max + 1], entry_id_max, interface_id_max,
        rpctype_id_max, args.hidden_channels, args.num_layers, args.dropout,
        heads=args.heads,
        num_quantiles=len(args.levels) if args.levels else 1,
    ).to(device)
    # the levels of this run: the tuple of a --taus run, else the scalar
    run_levels = tuple(args.levels) if args.levels else (args.tau,)
    model.taus = run_levels
    comm.broadcast_module_(model)
    if args.sync_bn and comm.distributed:
        model.enable_sync_bn(comm)
    if torch.cuda.is_available():
        from pertgnn.ops.functional import set_gemm_precision
        set_gemm_precision(args.precision)
    if args.predict:
        # model state only: no optimizer, no RNG restore
        state = predict_state  # load_state_dict copies it to the device
        check_heads(state, model, args.checkpoint)
        check_taus(state, run_levels if args.levels_given else None,
                   args.checkpoint)
        model.load_state_dict(state["model"])
        samples = {"test": test_list, "valid": valid_list, "train": train_list,
                   "all": train_list + valid_list + test_list}[args.predict_split]
        run_predict(args, model, device, samples)
        comm.finalize()
        return
    dynamic_scale = str(args.loss_scale).lower() == "dynamic"
    static_scale = 1.0 if dynamic_scale else float(args.loss_scale)
    args.loss_scale = static_scale  # loops use optimizer.scale_loss anyway
    lr_table = None
    if args.optim_ext:
        # one step per training batch of this rank: the count the epoch
        # loop runs (the resident batches of --hipgraph are cut the same way)
        total_steps = max(args.epochs * len(train_loader), 1)
        lr_table = make_lr_table(
            args.lr, total_steps, args.lr_schedule,
            warmup_steps=min(args.warmup_steps, total_steps),
            min_lr=args.min_lr)
    optimizer = FusedAdam(model.parameters(), lr=args.lr,
                          grad_scale=static_scale,
                          dynamic_scale=dynamic_scale,
                          weight_decay=args.weight_decay,
                          decay_filter=decay_params_of(model),
                          max_grad_norm=args.clip_grad_norm,
                          lr_schedule=lr_table)
    engine = FlatGradAllReduce(optimizer, comm) if comm.distributed else None
    log = JsonlLogger(args.metrics_jsonl, rank=comm.rank)

    start_epoch = 1
    if args.checkpoint and os.path.exists(args.checkpoint):
        ep, _ = load_checkpoint(args.checkpoint, model, optimizer,
                                map_location=device, taus=run_levels)
        start_epoch = ep + 1
        log.print0(f"resumed from {args.checkpoint} at epoch {ep}")

    # what the loops take as ``tau``: the scalar, or the tuple of levels
    tau_arg = args.levels if args.levels else args.tau

    stepper = None
    if args.hipgraph:
        from pertgnn.train.capture import GraphStepper, make_resident_batches

        resident = make_resident_batches(
            train_shard, args.batch_size, device, args.seed + comm.rank,
            collate_fn=collate_native,
        )
        stepper = GraphStepper(model, optimizer, engine, comm, tau_arg,
                               device, resident, loss_scale=args.loss_scale,
                               seed=args.seed + comm.rank)
        mode = stepper.capture()
        log.print0(f"# hipgraph stepping mode: {mode} "
                   f"({len(resident)} resident batches)")
        # eval sets collated once and held resident too (order preserved)
        valid_loader = make_resident_batches(
            valid_shard, args.batch_size, device, 0, collate_fn=collate_native,
            shuffle=False)
        test_loader = make_resident_batches(
            test_shard, args.batch_size, device, 0, collate_fn=collate_native,
            shuffle=False)

    predictor = None
    if args.fast_eval:
        from pertgnn.infer import Predictor

        was_training = model.training
        predictor = Predictor(model)
        model.train(was_training)
        if args.hipgraph:
            mode = predictor.capture(list(valid_loader) + list(test_loader))
            log.print0(f"# fast_eval stepping mode: {mode}")

    import time as _time

    def run_train_epoch(epoch_stats):
        if stepper is None:
            return train_epoch(
                model, train_loader, optimizer, tau_arg, device, engine=engine,
                comm=comm, stats_out=epoch_stats, loss_scale=args.loss_scale,
            )
        t0 = _time.perf_counter()
        loss_sum, mape_sum, n = stepper.run_epoch_sums()
        elapsed = _time.perf_counter() - t0
        if comm.distributed:
            loss_sum = comm.all_reduce_scalar(loss_sum)
            mape_sum = comm.all_reduce_scalar(mape_sum)
            n = int(comm.all_reduce_scalar(float(n)))
            elapsed = comm.all_reduce_scalar(elapsed, op="max")
        epoch_stats.update({
            "epoch_s": elapsed,
            "graphs_per_s": n / max(elapsed, 1e-9),
        })
        if stepper.last_q_loss is not None:
            # rank-local averages -> global: weight by this rank's graphs
            ql = [v * stepper.n_graphs for v in stepper.last_q_loss]
            if comm.distributed:
                ql = [comm.all_reduce_scalar(v) for v in ql]
            epoch_stats["q_loss"] = [v / max(n, 1) for v in ql]
        if stepper.last_grad_stats is not None:
            epoch_stats["grad_stats"] = stepper.last_grad_stats
        n = max(n, 1)
        return loss_sum / n, mape_sum / n

    for epoch in range(start_epoch, args.epochs + 1):
        epoch_stats: dict = {}
        train_mae, train_mape = run_train_epoch(epoch_stats)
        grad_stats = epoch_stats.pop("grad_stats", None)
        if predictor is not None:
            predictor.refresh()  # the epoch above changed the weights
        valid_rep = evaluate(
            model, valid_loader, tau_arg, device, comm=comm, predictor=predictor)
        test_rep = evaluate(
            model, test_loader, tau_arg, device, comm=comm, predictor=predictor)
        if args.levels:
            # point-level MAE/MAPE and the summed pinball loss on the line
            valid_mae, valid_mape, valid_q = (
                valid_rep.mae, valid_rep.mape, valid_rep.qloss_total)
            test_mae, test_mape, test_q = (
                test_rep.mae, test_rep.mape, test_rep.qloss_total)
        else:
            valid_mae, valid_mape, valid_q = valid_rep
            test_mae, test_mape, test_q = test_rep
        # reference epoch line format (pert_gnn.py:348-350)
        log.print0(
            f"Epoch: {epoch}, Train: {train_mae}, Test mae: {test_mae}, "
            f"Train mape: {train_mape}, Test mape: {test_mape}, Test q95 loss: {test_q}"
        )
        record = {
            "epoch": epoch, "train_loss": train_mae, "train_mape": train_mape,
            **epoch_stats,
            "valid_mae": valid_mae, "valid_mape": valid_mape, "valid_q": valid_q,
            "test_mae": test_mae, "test_mape": test_mape, "test_q": test_q,
        }
        if args.levels:
            for t, q, c in zip(test_rep.taus, test_rep.qloss, test_rep.coverage):
                log.print0(f"  tau={t}: test q loss={q}, coverage={c}")
            log.print0(f"  crossing={test_rep.crossing}")
            record.update({
                "taus": list(args.levels),
                "valid_q_levels": valid_rep.qloss,
                "test_q_levels": test_rep.qloss,
                "valid_coverage": valid_rep.coverage,
                "test_coverage": test_rep.coverage,
                "valid_crossing": valid_rep.crossing,
                "test_crossing": test_rep.crossing,
            })
        if grad_stats is not None:
            log.print0(
                f"  lr={grad_stats['lr']}, grad norm mean="
                f"{grad_stats['norm_mean']}, max={grad_stats['norm_max']}, "
                f"clipped={100.0 * grad_stats['clipped_frac']}%")
            record.update({
                "lr": grad_stats["lr"],
                "grad_norm_mean": grad_stats["norm_mean"],
                "grad_norm_max": grad_stats["norm_max"],
                "clipped_frac": grad_stats["clipped_frac"],
            })
        log.log(record)
        if args.checkpoint and epoch % args.checkpoint_every == 0:
            save_checkpoint(args.checkpoint, model, optimizer, epoch, comm=comm,
                            taus=run_levels)
    if args.checkpoint:
        save_checkpoint(args.checkpoint, model, optimizer, args.epochs, comm=comm,
                        taus=run_levels)
    log.close()
    comm.finalize()


if __name__ == "__main__":
    main()
