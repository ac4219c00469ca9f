"""GraphStepper — hipGraph-captured training for the production CLI.

The bench (bench.py) holds a few resident batches and captures one hipGraph
per batch; real training shuffles batch COMPOSITION every epoch (reference
pert_gnn.py:201-209), which defeats capture (shapes and addresses change
every step).  GraphStepper makes the production path benchable by fixing the
batch composition ONCE (one seeded shuffle at construction) and re-permuting
only the batch ORDER per epoch; every batch is then collated once, held
HBM-resident (north-star graph-shard prefetch; 288 GB holds any realistic
shard), and its training step is captured once and replayed every epoch.

DEVIATION (documented, opt-in via pert_gnn.py --hipgraph): batches are
re-drawn every epoch in the reference; here membership is fixed across
epochs and only the visit order reshuffles.  Optimization dynamics are
equivalent in expectation but not step-identical — leave the flag off for
exact-reference semantics.

Per-epoch metrics accumulate on device INSIDE the captured graph ([loss*B,
sum |err|/y] into a persistent accumulator, with a sequence of quantile
levels also every level's pinball sum), so an epoch costs one host sync.  World-size > 1 uses the compute-only capture with an eager gradient
all-reduce + optimizer tail (the same safe 'split' schedule bench.py
defaults to over RCCL); world-size 1 captures the optimizer step too.  On
CPU (tests) the stepper degrades to eager stepping over the same fixed
batches.
"""
from __future__ import annotations

import torch

from ..ops import functional as F
from ..ops import reference as ref


class GraphStepper:
    def __init__(self, model, optimizer, engine, comm, tau, device,
                 batches, loss_scale: float = 1.0, seed: int = 0):
        self.model = model
        self.optimizer = optimizer
        self.engine = engine
        self.comm = comm
        self.tau = tau
        self.device = device
        self.loss_scale = loss_scale
        self.batches = batches
        self.on_gpu = device is not None and device.type == "cuda"
        # a sequence of Q levels trains on the pinball loss summed over them;
        # the accumulator then also carries the per-level pinball sums
        self.levels = None if F._is_level(tau) else ref.check_taus(tau)
        self.point = ref.point_level(self.levels) if self.levels else 0
        self.last_q_loss = None  # per-level averages of the last epoch
        # FusedAdam.grad_stats() of the last epoch (extended step only)
        self.last_grad_stats = None
        self.acc = torch.zeros(2 + (len(self.levels) if self.levels else 0),
                               dtype=torch.float32,
                               device=device if self.on_gpu else "cpu")
        self.generator = torch.Generator().manual_seed(seed)
        self.n_graphs = sum(b.num_graphs for b in batches)
        self._graphs = None
        self._mode = "eager"

    # -- one training step over batch i (captured or eager) -----------------
    def _compute(self, i):
        b = self.batches[i]
        self.optimizer.zero_grad(set_to_none=False)
        gp, _ = self.model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                           b.pattern_num_nodes, b.rt_probs, b.entry_id,
                           b.batch, csr=b.csr, num_graphs=b.num_graphs)
        if self.levels is None:
            pred = gp.flatten()
            loss = F.quantile_loss(b.y, pred, self.tau)
        else:
            loss, q_sums = F.quantile_loss_parts(b.y, gp, self.levels)
            pred = gp[:, self.point]
        if hasattr(self.optimizer, "scale_loss"):
            self.optimizer.scale_loss(loss).backward()
        elif self.loss_scale != 1.0:
            (loss * self.loss_scale).backward()
        else:
            loss.backward()
        with torch.no_grad():
            self.acc[0] += loss.detach() * b.num_graphs
            self.acc[1] += ((pred.detach() - b.y).abs() / b.y).sum()
            if self.levels is not None:
                self.acc[2:] += q_sums
        return loss

    def _full_step(self, i):
        if self.engine is not None:
            self.engine.reset()
        self._compute(i)
        if self.engine is not None:
            self.engine.finalize()
        self.optimizer.step()

    def _snapshot(self):
        """Training state touched by the warmup steps: master params (the
        model's parameters are views into flat_param), optimizer moments and
        the BN running-stat buffers."""
        opt = self.optimizer
        return {
            "flat_param": opt.flat_param.detach().clone(),
            "flat_grad": opt.flat_grad.detach().clone(),
            "exp_avg": opt.exp_avg.detach().clone(),
            "exp_avg_sq": opt.exp_avg_sq.detach().clone(),
            "dev_state": opt.dev_state.detach().clone(),
            "sstate": (opt.sstate.detach().clone()
                       if getattr(opt, "sstate", None) is not None else None),
            # learning rate, clip coefficient and norm statistics: the
            # warmup steps walked the schedule and counted themselves
            "hstate": (opt.hstate.detach().clone()
                       if getattr(opt, "hstate", None) is not None else None),
            "step_count": opt.step_count,
            "buffers": [(b, b.detach().clone()) for b in self.model.buffers()
                        if torch.is_tensor(b) and b.numel() > 0],
        }

    def _restore(self, snap):
        opt = self.optimizer
        with torch.no_grad():
            opt.flat_param.copy_(snap["flat_param"])
            opt.flat_grad.copy_(snap["flat_grad"])
            opt.exp_avg.copy_(snap["exp_avg"])
            opt.exp_avg_sq.copy_(snap["exp_avg_sq"])
            opt.dev_state.copy_(snap["dev_state"])
            if snap["sstate"] is not None:
                opt.sstate.copy_(snap["sstate"])
            if snap["hstate"] is not None:
                opt.hstate.copy_(snap["hstate"])
            opt.step_count = snap["step_count"]
            for b, saved in snap["buffers"]:
                b.copy_(saved)

    def capture(self):
        """Capture per-batch graphs; returns the stepping mode achieved
        ('full', 'split' or 'eager'), agreed across ranks.  The eager
        allocation-warmup steps run REAL optimizer updates, so training
        state is snapshotted before and restored after — epoch 1 then
        starts from exactly the state the caller handed in (capture itself
        records kernels without executing them)."""
        if not self.on_gpu:
            self._mode = "eager"
            return self._mode
        distributed = self.comm is not None and self.comm.distributed
        want_full = not distributed  # split is the safe schedule over RCCL
        level = 0
        body = self._full_step if want_full else self._compute
        snap = self._snapshot()
        try:
            for i in range(len(self.batches)):
                self._full_step(i)  # allocation warmup (eager, exact step)
            torch.cuda.synchronize()
            if self.engine is not None and not want_full:
                self.engine.enabled = False
            try:
                graphs = []
                pool = None
                for i in range(len(self.batches)):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, pool=pool):
                        body(i)
                    if pool is None:
                        pool = g.pool()
                    graphs.append(g)
            finally:
                if self.engine is not None:
                    self.engine.enabled = True
            torch.cuda.synchronize()
            self._graphs = graphs
            level = 2 if want_full else 1
        except Exception as exc:  # pragma: no cover - hardware path
            import sys
            print(f"# hipGraph capture unavailable ({exc}); stepping eagerly",
                  file=sys.stderr)
            self._graphs = None
            level = 0
        self._restore(snap)
        if self.comm is not None:
            level = int(self.comm.all_reduce_scalar(float(level), op="min"))
            if level == 0:
                self._graphs = None
        self._mode = {2: "full", 1: "split", 0: "eager"}[level]
        return self._mode

    def run_epoch_sums(self):
        """One pass over all resident batches in a fresh random order.
        Returns rank-local (loss_sum, mape_sum, n_graphs) — the caller
        all-reduces the sums across ranks exactly like train_epoch."""
        order = torch.randperm(len(self.batches), generator=self.generator)
        with torch.no_grad():
            self.acc.zero_()
        inv_ws = 1.0 / self.comm.world_size if self.comm is not None else 1.0
        for i in order.tolist():
            if self._graphs is None:
                self._full_step(i)
            elif self._mode == "full":
                self._graphs[i].replay()
            else:  # split: captured compute + eager comm/optimizer tail
                self._graphs[i].replay()
                if self.comm is not None and self.comm.distributed:
                    self.comm.all_reduce_(self.optimizer.flat_grad)
                    self.optimizer.flat_grad.mul_(inv_ws)
                self.optimizer.step()
        if self.on_gpu:
            torch.cuda.synchronize()
        total_loss, mape_sum, *level_sums = self.acc.tolist()
        if getattr(self.optimizer, "extended", False):
            self.last_grad_stats = self.optimizer.grad_stats()
        if self.levels is not None:
            # rank-local, like the sums returned
            self.last_q_loss = [v / max(self.n_graphs, 1) for v in level_sums]
        return total_loss, mape_sum, self.n_graphs

    def run_epoch(self):
        """(avg_loss, avg_mape) over this rank's graphs."""
        total_loss, mape_sum, n = self.run_epoch_sums()
        n = max(n, 1)
        return total_loss / n, mape_sum / n


def make_resident_batches(data_list, batch_size, device, seed, collate_fn,
                          shuffle=True):
    """Fixed-composition batches (one seeded shuffle, or insertion order
    for eval sets), collated once and moved resident to ``device``."""
    if shuffle:
        idx = torch.randperm(len(data_list),
                             generator=torch.Generator().manual_seed(seed)).tolist()
    else:
        idx = list(range(len(data_list)))
    batches = []
    for lo in range(0, len(idx), batch_size):
        samples = [data_list[i] for i in idx[lo:lo + batch_size]]
        b = collate_fn(samples)
        batches.append(b.to(device) if device is not None and
                       device.type == "cuda" else b)
    return batches
