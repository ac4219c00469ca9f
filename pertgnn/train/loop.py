"""Training / evaluation loops (reference pert_gnn.py:213-294 semantics).

Differences from the reference that are performance-only (behavior-identical):
  * per-node rt_probs come precomputed from the collator instead of being
    rebuilt on CPU per batch (pert_gnn.py:220-230) — same values;
  * batches move to device with a single async H2D copy of the collated batch;
  * under DDP, gradient buckets all-reduce overlapped with backward and the
    summed metrics are all-reduced once per epoch.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import functional as F
from ..ops import reference as ref


class _nvtx:
    """roctx phase ranges (torch.cuda.nvtx maps to roctx on ROCm) — makes
    collate/H2D/fwd/bwd/allreduce/step phases visible in rocprofv3 traces."""

    def __init__(self, name):
        self.name = name
        self.on = torch.cuda.is_available()

    def __enter__(self):
        if self.on:
            torch.cuda.nvtx.range_push(self.name)

    def __exit__(self, *a):
        if self.on:
            torch.cuda.nvtx.range_pop()


def _forward(model, b):
    return model(
        b.x, b.cat_X, b.edge_index, b.edge_attr,
        b.pattern_num_nodes, b.rt_probs, b.entry_id, b.batch,
        csr=b.csr, num_graphs=b.num_graphs,
    )


@dataclass
class QuantileReport:
    """What ``evaluate`` returns for a sequence of levels: MAE and MAPE of
    the point level (the one closest to 0.5), and per level the mean pinball
    loss and the empirical coverage (fraction of rows with ``y <= y_hat``);
    ``crossing`` is the fraction of rows whose raw predictions are not
    non-decreasing; ``qloss_total`` is the sum of ``qloss``."""
    taus: tuple
    point: int
    mae: float
    mape: float
    qloss: list
    coverage: list
    crossing: float
    qloss_total: float

    @classmethod
    def from_sums(cls, taus, sums, n):
        """From the ``[3 + 2Q]`` sums of ``F.eval_metrics`` over ``n``
        rows (n = 0: all zeros)."""
        taus = ref.check_taus(taus)
        q = len(taus)
        sums = [float(v) for v in sums]
        if len(sums) != 3 + 2 * q:
            raise ValueError(f"expected {3 + 2 * q} sums for {q} levels, "
                             f"got {len(sums)}")
        d = max(int(n), 1)
        qloss = [v / d for v in sums[3:3 + q]]
        return cls(taus=taus, point=ref.point_level(taus), mae=sums[0] / d,
                   mape=sums[1] / d, qloss=qloss,
                   coverage=[v / d for v in sums[3 + q:]],
                   crossing=sums[2] / d, qloss_total=sum(qloss))


def _levels(tau):
    """None for one scalar level (every line then behaves as before the
    multi-level heads existed), else the validated tuple of levels."""
    return None if F._is_level(tau) else ref.check_taus(tau)


def train_epoch(model, loader, optimizer, tau, device, engine=None, comm=None,
                non_blocking=True, stats_out=None, loss_scale=1.0):
    """Returns (avg_loss, avg_mape); with stats_out (dict) also records
    graphs/sec, edges/sec and nodes/sec for the epoch (whole job).
    ``loss_scale`` > 1 enables static loss scaling (fp16 mode): the scaled
    loss drives backward, the optimizer unscales (FusedAdam ``grad_scale``
    must match), and the REPORTED loss stays unscaled.

    ``tau`` may be a sequence of Q levels: the model then emits ``[B, Q]``,
    training minimises the pinball loss summed over the levels, avg_loss is
    that sum, avg_mape is of the point level, and ``stats_out["q_loss"]``
    receives the per-level averages.

    With FusedAdam's extended step active (clipping, weight decay or a
    learning-rate table) ``stats_out["grad_stats"]`` receives
    ``optimizer.grad_stats()`` of the epoch (rank-local; under DDP every
    rank sees the norm of the same averaged gradient)."""
    import time as _time

    levels = _levels(tau)
    point = ref.point_level(levels) if levels is not None else 0
    q_sums = None
    model.train()
    n_graphs = 0
    n_edges = 0
    n_nodes = 0
    acc = None  # [loss*B sum, mape sum] accumulated ON DEVICE — the only
    # host sync is the one .tolist() after the epoch (reference semantics
    # float()'d per batch, pert_gnn.py:248-250, which serializes every step)
    t0 = _time.perf_counter()
    for batch in loader:
        with _nvtx("h2d"):
            b = batch.to(device, non_blocking=non_blocking) if device is not None else batch
        optimizer.zero_grad(set_to_none=False)
        if engine is not None:
            engine.reset()
        with _nvtx("forward"):
            global_pred, _local_pred = _forward(model, b)
            if levels is None:
                pred = global_pred.flatten()
                loss = F.quantile_loss(b.y, pred, tau)
            else:
                loss, q_sums = F.quantile_loss_parts(b.y, global_pred, levels)
                pred = global_pred[:, point]
        with _nvtx("backward"):
            # FusedAdam.scale_loss handles static AND dynamic loss scaling
            # (the dynamic scale is a device tensor — no host sync)
            if hasattr(optimizer, "scale_loss"):
                optimizer.scale_loss(loss).backward()
            elif loss_scale != 1.0:
                (loss * loss_scale).backward()
            else:
                loss.backward()
        with _nvtx("allreduce"):
            if engine is not None:
                engine.finalize()
        with _nvtx("optimizer"):
            optimizer.step()
        with torch.no_grad():
            if acc is None:
                acc = torch.zeros(2 + (len(levels) if levels else 0),
                                  dtype=torch.float64, device=pred.device)
            acc[0] += loss.detach().double() * b.num_graphs
            acc[1] += ((pred.detach() - b.y).abs() / b.y).sum().double()
            if levels is not None:
                acc[2:] += q_sums.double()
            n_graphs += b.num_graphs
            n_edges += b.edge_index.shape[1]
            n_nodes += b.x.shape[0]
    if device is not None and torch.cuda.is_available():
        torch.cuda.synchronize()
    sums = (acc.tolist() if acc is not None
            else [0.0] * (2 + (len(levels) if levels else 0)))
    total_loss, mape_sum, level_sums = sums[0], sums[1], sums[2:]
    grad_stats = (optimizer.grad_stats()
                  if getattr(optimizer, "extended", False) else None)
    elapsed = _time.perf_counter() - t0
    if comm is not None and comm.distributed:
        total_loss = comm.all_reduce_scalar(total_loss)
        mape_sum = comm.all_reduce_scalar(mape_sum)
        level_sums = [comm.all_reduce_scalar(v) for v in level_sums]
        n_graphs = int(comm.all_reduce_scalar(float(n_graphs)))
        n_edges = int(comm.all_reduce_scalar(float(n_edges)))
        n_nodes = int(comm.all_reduce_scalar(float(n_nodes)))
        elapsed = comm.all_reduce_scalar(elapsed, op="max")
    if stats_out is not None:
        stats_out.update({
            "epoch_s": elapsed,
            "graphs_per_s": n_graphs / max(elapsed, 1e-9),
            "edges_per_s": n_edges / max(elapsed, 1e-9),
            "nodes_per_s": n_nodes / max(elapsed, 1e-9),
        })
    n = max(n_graphs, 1)
    if stats_out is not None and levels is not None:
        stats_out["q_loss"] = [v / n for v in level_sums]
    if stats_out is not None and grad_stats is not None:
        stats_out["grad_stats"] = grad_stats
    return total_loss / n, mape_sum / n


@torch.no_grad()
def evaluate(model, loader, tau, device, comm=None, predictor=None):
    """``predictor`` (a ``pertgnn.infer.Predictor`` over ``model``, refreshed
    since the last weight update) supplies the predictions instead of the
    model forward; batches it was captured over (the same resident batch
    objects) replay their graphs.  Metric kernel and accumulation are
    unchanged.

    With a sequence of levels as ``tau`` the result is a ``QuantileReport``
    over the RAW (not rearranged) ``[B, Q]`` predictions; the ``[3 + 2Q]``
    metric sums accumulate on device and, under a distributed ``comm``, the
    whole vector and the row count are all-reduced."""
    levels = _levels(tau)
    if levels is not None:
        return _evaluate_levels(model, loader, levels, device, comm, predictor)
    model.eval()
    acc = None  # [mae, mape, qloss] sums on device; one sync per eval pass
    n_graphs = 0
    for batch in loader:
        ri = predictor.resident_index(batch) if predictor is not None else None
        if ri is not None:
            b = batch
            pred = predictor.replay(ri)
        else:
            b = batch.to(device) if device is not None else batch
            if predictor is not None:
                pred = predictor.predict_batch(b)
            else:
                global_pred, _ = _forward(model, b)
                pred = global_pred.flatten()
        mae_s, mape_s, q_s = F.eval_metrics(b.y, pred, tau)
        if acc is None:
            acc = torch.zeros(3, dtype=torch.float64, device=pred.device)
        acc[0] += mae_s.double() if torch.is_tensor(mae_s) else mae_s
        acc[1] += mape_s.double() if torch.is_tensor(mape_s) else mape_s
        acc[2] += q_s.double() if torch.is_tensor(q_s) else q_s
        n_graphs += b.num_graphs
    mae, mape, qloss = (acc.tolist() if acc is not None else (0.0, 0.0, 0.0))
    if comm is not None and comm.distributed:
        mae = comm.all_reduce_scalar(mae)
        mape = comm.all_reduce_scalar(mape)
        qloss = comm.all_reduce_scalar(qloss)
        n_graphs = int(comm.all_reduce_scalar(float(n_graphs)))
    n = max(n_graphs, 1)
    return mae / n, mape / n, qloss / n


def _evaluate_levels(model, loader, levels, device, comm, predictor):
    model.eval()
    nq = len(levels)
    acc = None  # [3 + 2Q] sums on device; one sync per eval pass
    n_graphs = 0
    for batch in loader:
        ri = predictor.resident_index(batch) if predictor is not None else None
        if ri is not None:
            b = batch
            pred = predictor.replay(ri, rearrange=False)
        else:
            b = batch.to(device) if device is not None else batch
            if predictor is not None:
                pred = predictor.predict_batch(b, rearrange=False)
            else:
                pred, _ = _forward(model, b)
        pred = pred.reshape(b.num_graphs, nq)
        sums = F.eval_metrics(b.y, pred, levels)
        if acc is None:
            acc = torch.zeros(3 + 2 * nq, dtype=torch.float64,
                              device=pred.device)
        acc += sums.double()
        n_graphs += b.num_graphs
    sums = acc.tolist() if acc is not None else [0.0] * (3 + 2 * nq)
    if comm is not None and comm.distributed:
        # the whole vector and the row count in one all-reduce
        on_dev = getattr(comm, "backend", None) == "nccl"
        t = torch.tensor(sums + [float(n_graphs)], dtype=torch.float64,
                         device=comm.device if on_dev else "cpu")
        comm.all_reduce_(t)
        *sums, n_graphs = t.tolist()
        n_graphs = int(n_graphs)
    return QuantileReport.from_sums(levels, sums, n_graphs)
