"""Inference path: ``Predictor`` — forward-only prediction from a trained
``SAGEDeterministic``.

The training ``forward`` with ``training=False`` does work a prediction does
not need: every conv's attention saves a per-edge ``alpha`` for a backward
that never runs, every non-final conv is followed by a separate BN-apply
pass over the whole ``[N,H]`` activation, and both per-vocab P tables of
every conv are recomputed per batch although they depend on weights only.

``Predictor`` folds and caches everything that depends on weights only

  * eval-mode BatchNorm ``i``  ->  per-channel ``(scale, shift)`` (``fold_bn``)
  * conv ``i``'s P tables      ->  ``ifc_table @ we_ifc^T``, ``rpc_table @ we_rpc^T``

and runs each conv as the QKVS GEMM plus ONE forward-only attention kernel
(``ops.edge_attention_fused_infer``) whose epilogue applies the folded BN
and the ReLU.  ``capture()`` records the whole forward of each resident
batch into a hipGraph.

CONTRACT: the caches are snapshots of the weights.  Call ``refresh()`` after
ANY weight update (optimizer step, ``load_state_dict``, manual edit) before
the next prediction.  ``refresh()`` rewrites the caches in place, so graphs
captured earlier stay valid and see the new values on their next replay.
"""
from __future__ import annotations

import torch
import torch.nn.functional as tF

from .ops import functional as ops
from .ops.backend import use_hip


def fold_bn(bn):
    """Eval-mode BatchNorm1d as a per-channel affine ``y = x*scale + shift``:
    ``scale = weight * rsqrt(running_var + eps)``,
    ``shift = bias - running_mean * scale`` (both fp32)."""
    var = bn.running_var.detach().float()
    mean = bn.running_mean.detach().float()
    scale = torch.rsqrt(var + bn.eps)
    if bn.weight is not None:
        scale = scale * bn.weight.detach().float()
    shift = -mean * scale
    if bn.bias is not None:
        shift = shift + bn.bias.detach().float()
    return scale, shift


class Predictor:
    """Forward-only predictor over a ``SAGEDeterministic``.

    ``precision`` (``"fp32"``/``"bf16"``/``"fp16"``), when given, sets the
    process-wide GEMM precision first.  The precision in force at
    construction decides the dtype of the cached P tables (bf16 exactly when
    the training forward would use bf16 tables) and must stay in force for
    the predictor's lifetime.

    The model is put in eval mode.  ``refresh()`` MUST be called after any
    weight update — predictions otherwise come from the stale caches."""

    def __init__(self, model, precision: str | None = None):
        self.model = model
        model.eval()
        if precision is not None:
            ops.set_gemm_precision(precision)
        self.precision = ops.gemm_precision()
        p = next(model.parameters())
        self.device = p.device
        self.hidden = model.convs[0].out_channels
        self._fused = use_hip(p)
        # same gates as SAGEDeterministic.forward / forward_fused
        self._act16 = (self._fused and self.precision in ("bf16", "fp16")
                       and self.hidden % 256 == 0 and ops.act16_enabled())
        self._p16 = self._act16 and ops.p16_enabled()
        h = self.hidden
        f32 = dict(dtype=torch.float32, device=self.device)
        pdt = dict(dtype=torch.bfloat16 if self._p16 else torch.float32,
                   device=self.device)
        self.bn_affine = [(torch.empty(h, **f32), torch.empty(h, **f32))
                          for _ in model.bns]
        vi = model.interface_embeds.weight.shape[0]
        vr = model.rpctype_embeds.weight.shape[0]
        self.p_tables = [(torch.empty(vi, h, **pdt), torch.empty(vr, h, **pdt))
                         for _ in model.convs]
        self.num_quantiles = m_q = int(model.global_linear2.weight.shape[0])
        if not 1 <= m_q <= 8:
            raise ValueError(f"the model emits {m_q} quantile levels; 1..8 "
                             "are supported")
        self._graphs = None
        self._batches = None
        self._out = None
        self._raw = None
        self._index = {}
        self.mode = "eager"
        self.refresh()

    @property
    def taus(self):
        """The quantile levels of the model's output columns, read from
        ``model.taus`` (set by the CLI / checkpoint loader); None if
        unknown."""
        t = getattr(self.model, "taus", None)
        return tuple(t) if t is not None else None

    # -- weight-only caches --------------------------------------------------
    @torch.no_grad()
    def refresh(self):
        """Recompute every cached tensor from the model's current weights,
        IN PLACE (``copy_`` into the storage allocated at construction), so
        captured graphs stay valid.  Must be called after any weight
        update."""
        m = self.model
        for bn, (scale, shift) in zip(m.bns, self.bn_affine):
            s, t = fold_bn(bn)
            scale.copy_(s)
            shift.copy_(t)
        ifc_w = m.interface_embeds.weight.detach()
        rpc_w = m.rpctype_embeds.weight.detach()
        for conv, (pifc, prpc) in zip(m.convs, self.p_tables):
            if self._p16:
                pifc.copy_(ops.linear16(ifc_w, conv.we_ifc.detach()))
                prpc.copy_(ops.linear16(rpc_w, conv.we_rpc.detach()))
            else:
                pifc.copy_(ops.linear(ifc_w, conv.we_ifc.detach(), None))
                prpc.copy_(ops.linear(rpc_w, conv.we_rpc.detach(), None))

    # -- one batch -------------------------------------------------------------
    def _check_precision(self):
        if self._fused and ops.gemm_precision() != self.precision:
            raise RuntimeError(
                f"GEMM precision changed from {self.precision!r} to "
                f"{ops.gemm_precision()!r} after this Predictor was built; "
                "its cached P tables no longer match — build a new Predictor")

    @torch.no_grad()
    def predict_batch(self, b, return_local: bool = False,
                      rearrange: bool = True):
        """Global latency prediction for one collated batch, fp32: flattened
        ``[num_graphs]`` for a one-level model, ``[num_graphs, Q]`` for a
        model with Q quantile levels — with ``rearrange`` (the default)
        every row sorted ascending, so the levels never cross; the raw
        decoder output otherwise (with ``return_local`` also the per-node
        local prediction ``[N,1]``).  Same embed, QKVS GEMM, pool and decoder ops
        as ``SAGEDeterministic.forward``; each conv is the QKVS GEMM plus
        the forward-only attention kernel with the cached P tables, the
        folded BN of the layer and the ReLU in its epilogue.  CPU batches
        (and batches without CSR arrays) run the same composition through
        the fp32 reference ops; the result equals ``model.eval()``'s."""
        self._check_precision()
        m = self.model
        edge_attr = b.edge_attr
        csr = getattr(b, "csr", None)
        if csr is None:
            # arbitrary-order edge list: sort by destination once
            perm, csr = ops._device_csr(b.edge_index, b.x.shape[0])
            edge_attr = edge_attr.index_select(0, perm)
        act16 = self._act16 and use_hip(b.x)
        x = ops.embed_concat_node(b.x, b.cat_X,
                                  [t.weight for t in m.cat_embedding],
                                  out16=act16, pad_to=m.convs[0].k_padded)
        last = len(m.convs) - 1
        for i, conv in enumerate(m.convs):
            if x.shape[1] != conv.k_padded:
                x = tF.pad(x, (0, conv.k_padded - x.shape[1]))
            qkvs = (ops.linear16(x, conv.w4, conv.b4) if act16
                    else ops.linear(x, conv.w4, conv.b4))
            pifc, prpc = self.p_tables[i]
            if i < last:
                scale, shift = self.bn_affine[i]
                x = ops.edge_attention_fused_infer(
                    qkvs, pifc, prpc, edge_attr, csr, scale, shift,
                    relu=True, out16=act16, heads=conv.heads)
            else:
                x = ops.edge_attention_fused_infer(qkvs, pifc, prpc,
                                                   edge_attr, csr,
                                                   heads=conv.heads)
        num_graphs = b.num_graphs
        mean_x = ops.pattern_pool(x, b.rt_probs, b.pattern_num_nodes, b.batch,
                                  num_graphs)
        entry_vec = ops.embedding(b.entry_id, m.entry_embeds.weight)
        g = torch.cat([mean_x, entry_vec], dim=1)
        hid = ops.linear(g, m.global_linear1.weight, m.global_linear1.bias)
        pred = ops.linear(tF.relu(hid), m.global_linear2.weight,
                          m.global_linear2.bias).float()
        if self.num_quantiles == 1:
            pred = pred.flatten()
        elif rearrange:
            pred = ops.quantile_rearrange(pred)
        if return_local:
            local = ops.linear(x, m.local_linear.weight, m.local_linear.bias)
            return pred, local
        return pred

    # -- many batches ------------------------------------------------------------
    def resident_index(self, b):
        """Index of ``b`` among the resident batches of the last
        ``capture()`` (matched by identity), or None."""
        if self._batches is None:
            return None
        return self._index.get(id(b))

    def captured_over(self, batches) -> bool:
        """True when ``batches`` are exactly the resident batches this
        predictor was captured over (same objects, same order)."""
        return (self._batches is not None
                and isinstance(batches, (list, tuple))
                and len(batches) == len(self._batches)
                and all(a is c for a, c in zip(batches, self._batches)))

    def predict(self, batches, rearrange: bool = True):
        """Predictions for every batch, concatenated in order into one fp32
        CPU tensor (``[n]``, or ``[n, Q]`` for Q > 1 levels).  One host
        sync, at the end."""
        if self.captured_over(batches):
            outs = [self.replay(i, rearrange=rearrange)
                    for i in range(len(self._batches))]
        else:
            outs = []
            for b in batches:
                if b.x.device != self.device:
                    b = b.to(self.device)
                outs.append(self.predict_batch(b, rearrange=rearrange))
        if not outs:
            return torch.empty((0,) if self.num_quantiles == 1
                               else (0, self.num_quantiles),
                               dtype=torch.float32)
        return torch.cat(outs).cpu()

    def capture(self, resident_batches):
        """Capture the forward of every resident batch into its own hipGraph
        (one shared memory pool), after an eager warm-up pass that primes
        the allocator.  Each batch gets a static output buffer
        (``[num_graphs]``, or ``[num_graphs, Q]`` for Q > 1 levels);
        ``replay(i)`` returns it.  For Q > 1 the graph ends with the
        rearrangement kernel and keeps the raw decoder output in a second
        static buffer for ``replay(i, rearrange=False)``.  The captured forward runs on a single stream with no
        parallel branches.  On CPU the predictor keeps stepping eagerly.
        Returns ``mode``: ``"graph"`` or ``"eager"``.  A capture failure is
        raised to the caller — there is no silent eager fallback."""
        batches = list(resident_batches)
        self._graphs = None
        self._out = None
        self._raw = None
        self._batches = batches  # held: keeps the ids below unique
        self._index = {id(b): i for i, b in enumerate(batches)}
        if not self._fused:
            self.mode = "eager"
            return self.mode
        for b in batches:
            if not use_hip(b.x):
                raise ValueError("capture() needs device-resident batches")
        nq = self.num_quantiles
        outs = [torch.empty((b.num_graphs,) if nq == 1 else (b.num_graphs, nq),
                            dtype=torch.float32, device=self.device)
                for b in batches]
        raws = [torch.empty_like(o) for o in outs] if nq > 1 else outs
        for b in batches:  # allocation warm-up (eager)
            self.predict_batch(b)
        torch.cuda.synchronize()
        graphs = []
        pool = None
        try:
            for b, out, raw in zip(batches, outs, raws):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    raw.copy_(self.predict_batch(b, rearrange=False))
                    if nq > 1:  # the sort is the graph's last op
                        out.copy_(ops.quantile_rearrange(raw))
                if pool is None:
                    pool = g.pool()
                graphs.append(g)
        except Exception as exc:
            self._batches = None
            raise RuntimeError(
                f"hipGraph capture of the inference forward failed: {exc}"
            ) from exc
        torch.cuda.synchronize()
        self._graphs = graphs
        self._out = outs
        self._raw = raws
        self.mode = "graph"
        return self.mode

    def replay(self, i: int, rearrange: bool = True):
        """Prediction for resident batch ``i`` of the last ``capture()``:
        replays its graph and returns the batch's static output buffer (the
        next ``replay(i)`` overwrites it); eager mode computes it afresh.
        ``rearrange=False`` returns the raw decoder output instead of the
        sorted rows (the same thing for a one-level model)."""
        if self._batches is None:
            raise RuntimeError("replay() before capture()")
        if self._graphs is None:
            return self.predict_batch(self._batches[i], rearrange=rearrange)
        self._check_precision()
        self._graphs[i].replay()
        return self._out[i] if rearrange else self._raw[i]


__all__ = ["fold_bn", "Predictor"]
