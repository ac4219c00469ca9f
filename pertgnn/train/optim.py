"""FusedAdam — Adam on flat master buffers (reference K14, torch.optim.Adam
math bit-for-bit in fp32).

All trainable parameters are re-viewed into ONE contiguous fp32 buffer at
construction (their values preserved); gradients accumulate directly into a
matching flat buffer (``p.grad`` is pre-set to a view), so:

  * zero_grad = one memset, step = ONE kernel launch for the whole model
    (HIP ``adam_step`` on GPU, the same flat math eagerly on CPU);
  * DDP gradient all-reduce operates on slices of the flat grad buffer with
    zero packing copies (see FlatGradAllReduce).

Three optional features take the step onto the extended kernels (HIP
``adam_step_ex``): global-norm gradient clipping (``max_grad_norm``),
decoupled weight decay (``weight_decay`` over the parameters ``decay_filter``
selects, torch.optim.AdamW order) and a per-step learning-rate table
(``lr_schedule``).  The rate of the step, the clip coefficient and the
gradient-norm statistics live on the device (``hstate``) next to the step
counter, so a captured step walks the schedule across replays.  With all
three off the step is the plain one, call for call.
"""
from __future__ import annotations

import math

import torch

from ..ops.backend import ext, has_hip


def _trainable(params):
    return [
        p for p in params
        if p.requires_grad and not isinstance(p, torch.nn.parameter.UninitializedParameter)
    ]


def make_lr_table(base_lr, total_steps, kind="constant", warmup_steps=0,
                  min_lr=0.0):
    """The learning rate of steps 1..total_steps as an fp32 tensor: linear
    warm-up ``base * t / W`` for ``t <= W``, then with
    ``s = (t - W) / (T - W)`` constant ``base``, linear
    ``base + (min - base) * s`` or cosine
    ``min + (base - min) * (1 + cos(pi * s)) / 2``.  Computed in fp64 on the
    host and rounded once."""
    if kind not in ("constant", "linear", "cosine"):
        raise ValueError(f"unknown lr schedule {kind!r}")
    T, W = int(total_steps), int(warmup_steps)
    if T < 1:
        raise ValueError("total_steps must be at least 1")
    if not 0 <= W <= T:
        raise ValueError("warmup_steps must lie in [0, total_steps]")
    base, low = float(base_lr), float(min_lr)
    out = []
    for t in range(1, T + 1):
        if t <= W:
            out.append(base * t / W)
            continue
        s = (t - W) / (T - W)
        if kind == "cosine":
            out.append(low + (base - low) * 0.5 * (1.0 + math.cos(math.pi * s)))
        elif kind == "linear":
            out.append(base + (low - base) * s)
        else:
            out.append(base)
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def decay_params_of(model):
    """The ``decay_filter`` the CLI uses: weights of at least 2 dimensions,
    minus every ``nn.Embedding`` table (category, interface, rpc, entry);
    BatchNorm affines and biases are 1-D and so never decayed."""
    skip = set()
    for mod in model.modules():
        if isinstance(mod, (torch.nn.Embedding,
                            torch.nn.modules.batchnorm._BatchNorm)):
            skip.update(id(p) for p in mod.parameters(recurse=False))
    keep = {id(p) for p in _trainable(model.parameters())
            if p.dim() >= 2 and id(p) not in skip}
    return lambda p: id(p) in keep


HSTATE_LEN = 8   # [lr, clip coef, norm, norm sum, norm max, clipped, steps, -]
SLAB_LEN = 4096  # one partial sum per block of the norm kernel (grid cap)


class FusedAdam:
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 grad_scale=1.0, dynamic_scale=False, init_scale=2.0 ** 16,
                 growth_interval=2000, backoff=0.5, growth=2.0,
                 weight_decay=0.0, decay_filter=None, max_grad_norm=None,
                 lr_schedule=None):
        self.params = _trainable(list(params))
        assert self.params, "no trainable parameters"
        assert all(p.dtype == torch.float32 for p in self.params), "fp32 master params only"
        self.lr = lr
        self.betas = betas
        self.eps = eps
        # static loss scaling: the loop multiplies the loss by grad_scale,
        # the optimizer divides the gradients back before the moment update
        self.grad_scale = float(grad_scale)
        # dynamic loss scaling (GradScaler semantics, fp16 configs): the
        # loop multiplies the loss by the DEVICE-resident scale (scale_loss),
        # the fused step scans grads for non-finites, skips-and-backs-off on
        # overflow and grows the scale after `growth_interval` clean steps —
        # all device-side, so a captured step replays correctly
        self.dynamic_scale = bool(dynamic_scale)
        self.backoff = float(backoff)
        self.growth = float(growth)
        self.growth_interval = float(growth_interval)
        self.step_count = 0
        device = self.params[0].device
        self.sstate = None
        if self.dynamic_scale:
            assert self.grad_scale == 1.0, "static and dynamic scaling are exclusive"
            self.sstate = torch.tensor([float(init_scale), 0.0, 0.0],
                                       dtype=torch.float32, device=device)

        total = sum(p.numel() for p in self.params)
        self.flat_param = torch.empty(total, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=device)
        # device-side [step, 1-b1^t, 1-b2^t] so the step is hipGraph-replayable
        self.dev_state = torch.zeros(3, dtype=torch.float32, device=device)
        self.offsets = []
        off = 0
        for p in self.params:
            n = p.numel()
            self.offsets.append(off)
            self.flat_param[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat_param[off:off + n].view_as(p.data)
            self._pin_grad(p, off)
            off += n

        self.weight_decay = float(weight_decay)
        self.max_grad_norm = (None if max_grad_norm is None
                              else float(max_grad_norm))
        if self.weight_decay < 0.0:
            raise ValueError("weight_decay must be non-negative")
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:
            raise ValueError("max_grad_norm must be positive")
        self.lr_table = None
        if lr_schedule is not None:
            table = torch.as_tensor(lr_schedule, dtype=torch.float32)
            if table.dim() != 1 or table.numel() == 0:
                raise ValueError("lr_schedule must be a non-empty 1-D sequence")
            self.lr_table = table.detach().clone().contiguous().to(device)
        self.decay_mask = None
        if self.weight_decay != 0.0:
            keep = decay_filter or (lambda p: p.dim() >= 2)
            # built once: one uint8 per element of the flat buffers
            self.decay_mask = torch.cat([
                torch.full((p.numel(),), 1 if keep(p) else 0, dtype=torch.uint8)
                for p in self.params]).to(device)
        # the extended step: taken only when a feature is on
        self.extended = (self.weight_decay != 0.0
                         or self.max_grad_norm is not None
                         or self.lr_table is not None)
        # device-side [lr, clip coef, norm, norm sum, norm max, clipped
        # steps, applied steps, spare]; slab is the norm kernel's scratch
        self.hstate = torch.zeros(HSTATE_LEN, dtype=torch.float32, device=device)
        self.hstate[1] = 1.0
        self.slab = (torch.zeros(SLAB_LEN, dtype=torch.float32, device=device)
                     if self.extended else None)

    def _pin_grad(self, p, off):
        """Point ``p.grad`` at its ``flat_grad`` slice and record that slice
        as the parameter's gradient sink: the native backward ops add a
        parameter's gradient straight into it (ops.functional.grad_sink)
        for as long as ``p.grad`` still aliases it."""
        view = self.flat_grad[off:off + p.numel()].view_as(p.data)
        p.grad = view
        p._grad_sink = view

    def zero_grad(self, set_to_none: bool = False):
        self.flat_grad.zero_()
        # autograd may have replaced p.grad (e.g. set_to_none elsewhere) — re-pin
        for p, off in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.flat_grad[off:off + p.numel()].data_ptr():
                self._pin_grad(p, off)

    def scale_loss(self, loss):
        """Multiply the loss by the active scale before backward: the
        device-resident dynamic scale (a 0-d tensor multiply, capturable),
        the static grad_scale, or a no-op."""
        if self.dynamic_scale:
            return loss * self.sstate[0]
        if self.grad_scale != 1.0:
            return loss * self.grad_scale
        return loss

    @torch.no_grad()
    def step(self):
        b1, b2 = self.betas
        if self.flat_param.is_cuda and has_hip():
            self.step_count += 1
            if self.extended:
                ext().adam_step_ex(
                    self.flat_param, self.flat_grad, self.exp_avg,
                    self.exp_avg_sq, self.dev_state, self.sstate, self.hstate,
                    self.slab, self.decay_mask, self.lr_table, self.lr,
                    b1, b2, self.eps, 1.0 / self.grad_scale,
                    self.weight_decay,
                    math.inf if self.max_grad_norm is None
                    else self.max_grad_norm,
                    self.backoff, self.growth, self.growth_interval)
            elif self.dynamic_scale:
                ext().adam_step_dynamic(
                    self.flat_param, self.flat_grad, self.exp_avg,
                    self.exp_avg_sq, self.dev_state, self.sstate, self.lr,
                    b1, b2, self.eps, self.backoff, self.growth,
                    self.growth_interval)
            else:
                ext().adam_step(self.flat_param, self.flat_grad, self.exp_avg,
                                self.exp_avg_sq, self.dev_state, self.lr, b1, b2,
                                self.eps, 1.0 / self.grad_scale)
            return
        # eager fallback — identical formula (torch.optim.Adam)
        g = self.flat_grad
        if self.dynamic_scale:
            if not bool(torch.isfinite(g).all()):
                self.sstate[0] = max(float(self.sstate[0]) * self.backoff, 1.0)
                self.sstate[1] = 0.0
                return  # skipped step: moments and counter untouched
            inv = 1.0 / float(self.sstate[0])
            self.sstate[1] += 1.0
            if float(self.sstate[1]) >= self.growth_interval:
                self.sstate[0] = min(float(self.sstate[0]) * self.growth,
                                     4294967296.0)
                self.sstate[1] = 0.0
        else:
            inv = 1.0 / self.grad_scale
        if self.extended:
            self._eager_step_ex(g, inv)
            return
        self.step_count += 1
        self.exp_avg.mul_(b1).add_(g, alpha=(1 - b1) * inv)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=(1 - b2) * inv * inv)
        bias1 = 1 - b1 ** self.step_count
        bias2 = 1 - b2 ** self.step_count
        denom = (self.exp_avg_sq.sqrt() / (bias2 ** 0.5)).add_(self.eps)
        self.flat_param.addcdiv_(self.exp_avg, denom, value=-self.lr / bias1)

    def _eager_step_ex(self, g, inv):
        """The extended step, eagerly: unscale, norm, clip, the rate of the
        new applied-step count, decoupled decay, Adam."""
        b1, b2 = self.betas
        h = self.hstate
        g = g * inv
        norm = torch.linalg.vector_norm(g)
        coef = torch.ones((), dtype=torch.float32, device=g.device)
        if self.max_grad_norm is not None:
            coef = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        self.step_count += 1
        t = self.step_count
        lr = self.lr
        if self.lr_table is not None:
            lr = float(self.lr_table[min(t, self.lr_table.numel()) - 1])
        h[0] = lr
        h[1] = coef
        h[2] = norm
        h[3] += norm
        h[4] = torch.maximum(h[4], norm)
        if bool(coef < 1.0):
            h[5] += 1.0
        h[6] += 1.0
        lr = float(h[0])  # the fp32 rate, as the kernel reads it
        g = g * coef
        if self.decay_mask is not None:
            keep = torch.where(self.decay_mask.bool(),
                               1.0 - lr * self.weight_decay, 1.0)
            self.flat_param.mul_(keep.to(torch.float32))
        self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        bias1 = 1 - b1 ** t
        bias2 = 1 - b2 ** t
        denom = (self.exp_avg_sq.sqrt() / (bias2 ** 0.5)).add_(self.eps)
        self.flat_param.addcdiv_(self.exp_avg, denom, value=-lr / bias1)

    def grad_stats(self, reset=True):
        """Learning rate and gradient-norm statistics of the extended step
        since the last reset, from ONE read of the device state: ``lr`` and
        ``norm_last`` of the latest applied step, ``norm_mean`` / ``norm_max``
        over the applied steps, the fraction of them that were clipped, and
        their count.  ``reset`` zeroes the running statistics."""
        lr, _coef, last, total, peak, clipped, steps, _ = self.hstate.tolist()
        if reset:
            self.hstate[3:7].zero_()
        return {
            "lr": lr,
            "norm_last": last,
            "norm_mean": total / steps if steps else 0.0,
            "norm_max": peak,
            "clipped_frac": clipped / steps if steps else 0.0,
            "steps": int(steps),
        }

    def _synced_step_count(self) -> int:
        """True step count on GPU: the device-side counter is authoritative —
        hipGraph replays advance only it, and dynamic-scale overflow skips
        advance only the Python counter."""
        if self.flat_param.is_cuda and has_hip():
            self.step_count = int(self.dev_state[0].item())
        return self.step_count

    # -- torch-optimizer-compatible surface ---------------------------------
    def state_dict(self):
        sd = {
            "step": self._synced_step_count(),
            "dev_state": self.dev_state,
            "exp_avg": self.exp_avg,
            "exp_avg_sq": self.exp_avg_sq,
            "lr": self.lr,
            "betas": self.betas,
            "eps": self.eps,
        }
        if self.sstate is not None:
            sd["sstate"] = self.sstate
        sd["weight_decay"] = self.weight_decay
        sd["max_grad_norm"] = self.max_grad_norm
        sd["hstate"] = self.hstate
        return sd

    def load_state_dict(self, sd):
        self.step_count = sd["step"]
        if "dev_state" in sd:
            self.dev_state.copy_(sd["dev_state"].to(self.dev_state.device))
        if "sstate" in sd and self.sstate is not None:
            self.sstate.copy_(sd["sstate"].to(self.sstate.device))
        self.exp_avg.copy_(sd["exp_avg"].to(self.exp_avg.device))
        self.exp_avg_sq.copy_(sd["exp_avg_sq"].to(self.exp_avg_sq.device))
        self.lr = sd.get("lr", self.lr)
        # the statistics and the rate last used; weight_decay, max_grad_norm
        # and the table stay the constructor's (resuming with other flags is
        # legitimate), the schedule position is dev_state[0]
        if "hstate" in sd:
            self.hstate.copy_(sd["hstate"].to(self.hstate.device))


class FlatGradAllReduce:
    """Bucketed all-reduce over contiguous slices of FusedAdam's flat grad
    buffer — no packing copies.  Buckets are cut from the END of the buffer
    (parameters late in the module tree get grads first during backward);
    each bucket launches its async all-reduce from the post-accumulate hook
    of its last-pending parameter, on a dedicated comm stream.
    """

    def __init__(self, optimizer: FusedAdam, comm, bucket_cap_mb: float = 32.0):
        self.opt = optimizer
        self.comm = comm
        # `enabled=False` silences the backward hooks (and finalize): used
        # while capturing a compute-only hipGraph, where collectives must
        # stay out of the captured stream (bench.py --graph-mode split)
        self.enabled = True
        self.use_stream = comm.device.type == "cuda"
        self.comm_stream = torch.cuda.Stream() if self.use_stream else None

        cap = int(bucket_cap_mb * 1024 * 1024 / 4)
        self.buckets = []  # list of dicts {lo, hi, params(set ids), pending, work}
        cur_params = []
        cur_lo = None
        cur_hi = None
        items = list(zip(self.opt.params, self.opt.offsets))
        for p, off in reversed(items):
            if cur_hi is None:
                cur_hi = off + p.numel()
            cur_lo = off
            cur_params.append(p)
            if cur_hi - cur_lo >= cap:
                self._seal(cur_lo, cur_hi, cur_params)
                cur_params, cur_lo, cur_hi = [], None, None
        if cur_params:
            self._seal(cur_lo, cur_hi, cur_params)

        self.param2bucket = {}
        for b in self.buckets:
            for p in b["params"]:
                self.param2bucket[id(p)] = b
        for p in self.opt.params:
            p.register_post_accumulate_grad_hook(self._hook)
            # a sunk parameter enters its autograd node detached, so its hooks
            # would never fire: while this engine is live (enabled,
            # distributed) the ops keep returning gradients instead of adding
            # into the sinks (ops.functional.grad_sink reads this)
            p._grad_sink_engine = self

    def _seal(self, lo, hi, params):
        self.buckets.append({"lo": lo, "hi": hi, "params": list(params),
                             "pending": 0, "work": None})

    def reset(self):
        for b in self.buckets:
            b["pending"] = len(b["params"])
            b["work"] = None

    def _launch(self, b):
        flat = self.opt.flat_grad[b["lo"]:b["hi"]]
        if self.use_stream:
            self.comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                b["work"] = self.comm.all_reduce_(flat, async_op=True)
        else:
            b["work"] = self.comm.all_reduce_(flat, async_op=True)

    def _hook(self, p):
        if not self.comm.distributed or not self.enabled:
            return
        b = self.param2bucket[id(p)]
        b["pending"] -= 1
        if b["pending"] == 0:
            self._launch(b)

    def finalize(self):
        if not self.comm.distributed or not self.enabled:
            return
        for b in self.buckets:
            if b["work"] is None:
                self._launch(b)  # params outside the loss (dead heads)
        for b in self.buckets:
            if b["work"] is not None:
                b["work"].wait()
        if self.use_stream:
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        self.opt.flat_grad.mul_(1.0 / self.comm.world_size)
