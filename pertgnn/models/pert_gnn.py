"""PERT-GNN graph-transformer model — MI355X-native re-implementation.

State_dict-compatible with the reference ``model.py`` (SAGEDeterministic,
/root/reference/model.py:10-114) WITHOUT any PyG dependency: the conv is our
own TransformerConv equivalent whose submodule names match PyG 2.4.0
(``lin_key``/``lin_query``/``lin_value``/``lin_edge``/``lin_skip``) so
checkpoints keep the same keys, and whose math runs through
``pertgnn.ops.functional`` (HIP kernels on GPU, eager oracle on CPU).

Reference quirks intentionally reproduced:
  * ``num_layers=1`` still builds 2 convs (model.py:24-52).
  * dead ``edge_linear`` lazy module kept in the state_dict (model.py:68).
  * ``local_pred`` returned but unused by the training loss (pert_gnn.py:245).
  * pattern_probs consumed per-NODE (the rebuilt rt_probs of pert_gnn.py:224-230).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from ..ops import functional as ops


class _EdgeLinearView:
    """Read-through view of the conv's split edge-projection parameters
    (``we_ifc``/``we_rpc``) as the reference's single ``lin_edge.weight``
    [H, 2H] (bias=False)."""

    def __init__(self, conv):
        object.__setattr__(self, "_conv", conv)

    @property
    def weight(self):
        c = self._conv
        return torch.cat([c.we_ifc, c.we_rpc], dim=1)

    bias = None


class _SegLinearView:
    """Read-through view of one H-row segment of the conv's fused ``w4``/``b4``
    parameters — keeps the PyG-style ``conv.lin_query.weight`` access (and the
    eager CPU forward) working while the storage is the single fused tensor
    the QKVS GEMM consumes."""

    def __init__(self, conv, seg, has_bias=True):
        object.__setattr__(self, "_conv", conv)
        object.__setattr__(self, "_seg", seg)
        object.__setattr__(self, "_has_bias", has_bias)

    @property
    def weight(self):
        c = self._conv
        h = c.out_channels
        return c.w4[self._seg * h:(self._seg + 1) * h, :c.in_channels]

    @property
    def bias(self):
        if not self._has_bias:
            return None
        c = self._conv
        h = c.out_channels
        return c.b4[self._seg * h:(self._seg + 1) * h]


class TransformerConv(nn.Module):
    """Graph transformer conv, PyG-2.4.0 semantics with concat=True,
    root_weight=True, beta=False (reference model.py:25-52 configuration,
    which uses heads=1).

    out_i = W_skip x_i + b + sum_{e:(j->i)} softmax_i(<W_q x_i, W_k x_j + W_e e_ij>/sqrt(H))
            * (W_v x_j + W_e e_ij)

    ``out_channels`` is the TOTAL output width H (the reference passes
    heads=1, where PyG's per-head width and the total coincide).  With
    ``heads`` > 1 the H channels split into ``heads`` heads of
    C = H / heads channels: head t owns channels [tC, (t+1)C), its logits
    are scaled by 1/sqrt(C) and its softmax runs on its own.  That is PyG's
    ``TransformerConv(in, C, heads=heads, concat=True, edge_dim=2H)``:
    the same parameter shapes and state_dict keys at any head count
    (``lin_*.weight`` [H, in], ``lin_edge.weight`` [H, 2H]), and glorot
    init over the same shapes.  ``heads`` must divide ``out_channels``.

    The four projection matrices live in ONE fused parameter ``w4`` [4H, Kp]
    (rows: query, key, value, skip; Kp = K padded to a multiple of 8 with
    zero columns so the GEMM staging vectorizes) + fused bias ``b4`` [4H] —
    the hot QKVS GEMM and its weight-grad then touch a single tensor with no
    per-step cat/slice glue.  ``lin_query``/``lin_key``/``lin_value``/
    ``lin_skip`` stay accessible as views, and the state_dict still uses the
    reference's per-projection keys (checkpoint compatibility), remapped in
    ``_save_to_state_dict``/``_load_from_state_dict``."""

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, edge_dim: int | None = None):
        super().__init__()
        if not isinstance(heads, int) or heads < 1 or out_channels % heads != 0:
            raise ValueError(
                f"heads={heads!r} must be a positive integer that divides "
                f"out_channels={out_channels}")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.edge_dim = edge_dim
        # pad K to a multiple of 32 so the layer-1 QKVS GEMM qualifies for
        # the glds (direct-to-LDS) fast path (k % BK == 0), and up to a
        # multiple of 128 when that costs <= 35% extra zero-column FLOPs:
        # the 128-multiple makes the layer's dgrad (N out = K) and wgrad
        # (k2 = K) glds-eligible too — measured: the K=288 wgrad on the
        # register-staging path alone cost ~0.75 ms/step at trace scale.
        # Zero columns stay zero under Adam, so the math is unchanged.
        k32 = (in_channels + 31) // 32 * 32
        k128 = (in_channels + 127) // 128 * 128
        self.k_padded = k128 if k128 <= 1.35 * k32 else k32
        self.w4 = nn.Parameter(torch.zeros(4 * out_channels, self.k_padded))
        self.b4 = nn.Parameter(torch.zeros(4 * out_channels))
        self.lin_query = _SegLinearView(self, 0)
        self.lin_key = _SegLinearView(self, 1)
        self.lin_value = _SegLinearView(self, 2)
        self.lin_skip = _SegLinearView(self, 3)
        # lin_edge [H, 2H] stored as the two halves the fused path consumes
        # (P_ifc = ifc_table @ we_ifc^T, P_rpc = rpc_table @ we_rpc^T) — no
        # per-step slicing or slice-grad padding
        assert edge_dim == 2 * out_channels
        self.we_ifc = nn.Parameter(torch.empty(out_channels, out_channels))
        self.we_rpc = nn.Parameter(torch.empty(out_channels, out_channels))
        self.lin_edge = _EdgeLinearView(self)
        self.reset_parameters()

    def reset_parameters(self):
        # PyG Linear default init is glorot for weight, zeros for bias.
        with torch.no_grad():
            self.w4.zero_()
            self.b4.zero_()
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        # glorot over the FULL [H, 2H] edge matrix (fan_in = 2H, matching the
        # reference's single lin_edge), then split into the stored halves
        h = self.out_channels
        w = torch.empty(h, 2 * h)
        nn.init.xavier_uniform_(w)
        with torch.no_grad():
            self.we_ifc.copy_(w[:, :h])
            self.we_rpc.copy_(w[:, h:])

    _SEG_NAMES = ("lin_query", "lin_key", "lin_value", "lin_skip")

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        # emit the reference's per-projection keys instead of w4/b4/we_*
        super()._save_to_state_dict(destination, prefix, keep_vars)
        del destination[prefix + "w4"]
        del destination[prefix + "b4"]
        del destination[prefix + "we_ifc"]
        del destination[prefix + "we_rpc"]
        for i, name in enumerate(self._SEG_NAMES):
            view = getattr(self, name)
            w = view.weight
            b = view.bias
            destination[prefix + name + ".weight"] = w if keep_vars else w.detach().clone()
            destination[prefix + name + ".bias"] = b if keep_vars else b.detach().clone()
        we = self.lin_edge.weight
        destination[prefix + "lin_edge.weight"] = we if keep_vars else we.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict,
                              missing_keys, unexpected_keys, error_msgs):
        h = self.out_channels
        with torch.no_grad():
            for i, name in enumerate(self._SEG_NAMES):
                wk, bk = prefix + name + ".weight", prefix + name + ".bias"
                if wk in state_dict:
                    self.w4[i * h:(i + 1) * h, :self.in_channels].copy_(state_dict[wk])
                    self.w4[i * h:(i + 1) * h, self.in_channels:].zero_()
                    state_dict = {k: v for k, v in state_dict.items() if k != wk}
                else:
                    # nn.Module semantics: missing keys are COLLECTED
                    # regardless of strict (strict only controls raising)
                    missing_keys.append(wk)
                if bk in state_dict:
                    self.b4[i * h:(i + 1) * h].copy_(state_dict[bk])
                    state_dict = {k: v for k, v in state_dict.items() if k != bk}
                else:
                    missing_keys.append(bk)
        we_key = prefix + "lin_edge.weight"
        if we_key in state_dict:
            with torch.no_grad():
                w = state_dict[we_key]
                self.we_ifc.copy_(w[:, :h])
                self.we_rpc.copy_(w[:, h:])
        else:
            missing_keys.append(we_key)
        filtered = {k: v for k, v in state_dict.items()
                    if k != we_key
                    and not any(k == prefix + n + s for n in self._SEG_NAMES
                                for s in (".weight", ".bias"))}
        super()._load_from_state_dict(filtered, prefix, local_metadata, strict,
                                      missing_keys, unexpected_keys, error_msgs)
        for k in (prefix + "w4", prefix + "b4", prefix + "we_ifc",
                  prefix + "we_rpc"):
            if k in missing_keys:
                missing_keys.remove(k)

    def forward(self, x, edge_index, edge_embeds, csr=None, num_nodes=None):
        n = x.shape[0] if num_nodes is None else num_nodes
        q = ops.linear(x, self.lin_query.weight.contiguous(), self.lin_query.bias)
        k = ops.linear(x, self.lin_key.weight.contiguous(), self.lin_key.bias)
        v = ops.linear(x, self.lin_value.weight.contiguous(), self.lin_value.bias)
        e = ops.linear(edge_embeds, self.lin_edge.weight, None)
        skip = ops.linear(x, self.lin_skip.weight.contiguous(), self.lin_skip.bias)
        return ops.edge_attention(q, k, v, e, skip, edge_index, n, csr=csr,
                                  heads=self.heads)

    def forward_fused(self, x, edge_attr, ifc_weight, rpc_weight, csr,
                      out16=False, pifc=None, prpc=None):
        """HIP fast path: one [N,K]x[4H,K]^T GEMM for q/k/v/skip and
        L2-resident per-vocab P tables instead of the [E,2H] edge-embed
        stream (exact refactoring by linearity of lin_edge).  In bf16/fp16
        precision with H%256==0 the qkvs tensor is kept bf16-resident
        through the attention kernels.  ``pifc`` / ``prpc``: this layer's
        bf16 P tables when the caller computed all layers' at once
        (``ops.ptables_grouped``); without them they are computed here."""
        qkvs, pifc, prpc = self._fused_operands(x, ifc_weight, rpc_weight,
                                                pifc, prpc)
        return ops.edge_attention_fused(qkvs, pifc, prpc, edge_attr, csr,
                                        out16=out16, heads=self.heads)

    def forward_fused_bn(self, x, edge_attr, ifc_weight, rpc_weight, csr, bn,
                         comm=None, dropout_p=0.0, pifc=None, prpc=None):
        """``forward_fused(..., out16=True)`` followed by the training
        BN+ReLU(+dropout) of ``bn`` as one autograd node, whose attention
        backward applies the BN backward (act16 mode only; the caller checks
        ``ops.bn_attn_fuse_enabled``)."""
        qkvs, pifc, prpc = self._fused_operands(x, ifc_weight, rpc_weight,
                                                pifc, prpc)
        return ops.edge_attention_fused_bn_relu(
            qkvs, pifc, prpc, edge_attr, csr, bn.weight, bn.bias,
            bn.running_mean, bn.running_var, bn.momentum, bn.eps,
            heads=self.heads, comm=comm, dropout_p=dropout_p)

    def forward_fused_pool(self, x, edge_attr, ifc_weight, rpc_weight, csr,
                           probs, nnodes, batch, num_graphs, pifc=None,
                           prpc=None):
        """``forward_fused(...)`` (fp32 out) and the pattern pool over it ->
        ``(x, mean_x)``: one autograd node where ``ops.pool_attn_fuse_enabled``
        holds, whose backward forms the pool's gradient inside the attention
        backward; the two separate ops otherwise."""
        qkvs, pifc, prpc = self._fused_operands(x, ifc_weight, rpc_weight,
                                                pifc, prpc)
        return ops.edge_attention_fused_pool(
            qkvs, pifc, prpc, edge_attr, csr, probs, nnodes, batch,
            num_graphs, heads=self.heads)

    def _fused_operands(self, x, ifc_weight, rpc_weight, pifc, prpc):
        """qkvs and the two P tables of the fused attention op."""
        h = self.out_channels
        # w4/b4 ARE the parameters (no per-step cat); the storage is
        # pre-padded to k_padded with zero columns (zero-grad columns stay
        # zero under Adam), so only x needs padding for the vectorized
        # staging path
        if x.shape[1] != self.k_padded:
            x = torch.nn.functional.pad(x, (0, self.k_padded - x.shape[1]))
        act16 = (ops.gemm_precision() in ("bf16", "fp16") and h % 256 == 0
                 and ops.act16_enabled())
        if act16:
            # the first conv's x is the embed concat: where its only
            # gradient would be the category table's, that one is formed
            # from dqkvs directly and no dgrad runs (linear16 otherwise)
            qkvs = ops.linear16_embed(x, self.w4, self.b4)
            if pifc is not None and prpc is not None:
                pass  # grouped: computed once for all layers by the caller
            elif ops.p16_enabled():
                # bf16 P tables: halves the per-edge ec gather bytes AND the
                # L2 footprint of the tables (2x256H fp32 = 4 MB at realistic
                # vocab vs 4 MB L2 per XCD); logits/softmax stay fp32
                pifc = ops.linear16(ifc_weight, self.we_ifc)
                prpc = ops.linear16(rpc_weight, self.we_rpc)
            else:
                pifc = ops.linear(ifc_weight, self.we_ifc, None)
                prpc = ops.linear(rpc_weight, self.we_rpc, None)
        else:
            qkvs = ops.linear(x, self.w4, self.b4)
            pifc = ops.linear(ifc_weight, self.we_ifc, None)
            prpc = ops.linear(rpc_weight, self.we_rpc, None)
        return qkvs, pifc, prpc


class SAGEDeterministic(nn.Module):
    """API- and checkpoint-compatible with reference model.py:10-114.
    ``heads`` (keyword-only, default 1 = the reference) is the attention
    head count of every conv; it must divide ``hidden_channels``.
    ``num_quantiles`` (keyword-only, default 1 = the reference) is the width
    of the global decoder's output: ``forward`` returns ``global_predict
    [B, num_quantiles]``, one column per quantile level.  ``taus`` holds the
    levels the model is trained for (set by the CLI and the checkpoint
    loader; None = unknown)."""

    def __init__(
        self,
        in_channels,
        cat_dims,
        entry_id_max,
        interface_id_max,
        rpctype_id_max,
        hidden_channels,
        num_layers,
        dropout,
        *,
        heads=1,
        num_quantiles=1,
    ):
        super().__init__()
        if not isinstance(num_quantiles, int) or not 1 <= num_quantiles <= 8:
            raise ValueError(
                f"num_quantiles={num_quantiles!r} must be an integer in 1..8")
        self.heads = heads
        self.num_quantiles = num_quantiles
        self.taus = None
        self.convs = nn.ModuleList()
        self.convs.append(
            TransformerConv(
                in_channels=in_channels + hidden_channels,
                out_channels=hidden_channels,
                heads=heads,
                edge_dim=hidden_channels * 2,
            )
        )
        self.bns = nn.ModuleList()
        self.bns.append(nn.BatchNorm1d(hidden_channels))
        for _ in range(num_layers - 2):
            self.convs.append(
                TransformerConv(
                    in_channels=hidden_channels,
                    out_channels=hidden_channels,
                    heads=heads,
                    edge_dim=hidden_channels * 2,
                )
            )
            self.bns.append(nn.BatchNorm1d(hidden_channels))
        self.convs.append(
            TransformerConv(
                in_channels=hidden_channels,
                out_channels=hidden_channels,
                heads=heads,
                edge_dim=hidden_channels * 2,
            )
        )
        self.local_linear = nn.Linear(hidden_channels, 1)
        self.global_linear1 = nn.Linear(hidden_channels * 2, hidden_channels)
        self.global_linear2 = nn.Linear(hidden_channels, num_quantiles)
        self.cat_embedding = nn.ModuleList()
        for num_categories in cat_dims:
            self.cat_embedding.append(nn.Embedding(num_categories, hidden_channels))

        self.dropout = dropout
        self.entry_embeds = nn.Embedding(entry_id_max + 1, hidden_channels)
        self.interface_embeds = nn.Embedding(interface_id_max + 1, hidden_channels)
        self.rpctype_embeds = nn.Embedding(rpctype_id_max + 1, hidden_channels)
        # Dead module, never called in forward — kept lazily-uninitialized so the
        # state_dict matches the reference (model.py:68).
        self.edge_linear = nn.LazyLinear(hidden_channels * 2)
        # sync-BN comm (None = per-replica BN, the fast default under DDP)
        self._bn_comm = None

    def enable_sync_bn(self, comm):
        """Exact-parity BN under DDP: batch statistics all-reduced across
        ranks (SURVEY.md §7 hard part 4). Pass None to disable."""
        self._bn_comm = comm

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()

    def forward(
        self,
        x,
        cat_X,
        edge_index,
        edge_attr,
        pattern_num_nodes,
        pattern_probs,
        entry_id,
        batch,
        csr=None,
        num_graphs=None,
    ):
        if num_graphs is None:
            num_graphs = int(batch.max().item()) + 1 if batch.numel() else 0
        from ..ops.backend import use_hip

        fused = csr is not None and use_hip(x)
        hidden = self.bns[0].weight.shape[0] if len(self.bns) else 0
        out16 = (fused and ops.gemm_precision() in ("bf16", "fp16")
                 and hidden % 256 == 0 and ops.act16_enabled())
        # fused path: the concat comes out at the first conv's padded GEMM
        # width, so forward_fused finds nothing left to pad
        x = ops.embed_concat_node(x, cat_X,
                                  [t.weight for t in self.cat_embedding],
                                  out16=out16,
                                  pad_to=self.convs[0].k_padded if fused else None)
        edge_embeds = None
        if not fused:
            edge_embeds = ops.embed_concat_edge(
                edge_attr, self.interface_embeds.weight, self.rpctype_embeds.weight
            )
        n = x.shape[0]

        # the embedding tables do not change inside a step: with bf16 P
        # tables, all layers' table @ we^T products (and their backward) run
        # as grouped launches instead of per layer
        ptables = {}
        if out16 and ops.p16_enabled() and ops.ptable_group_enabled():
            pifcs, prpcs = ops.ptables_grouped(
                self.interface_embeds.weight, self.rpctype_embeds.weight,
                [c.we_ifc for c in self.convs], [c.we_rpc for c in self.convs])
            ptables = {id(c): pair
                       for c, pair in zip(self.convs, zip(pifcs, prpcs))}

        def run_conv(conv, x, out16=False):
            if fused:
                pifc, prpc = ptables.get(id(conv), (None, None))
                return conv.forward_fused(
                    x, edge_attr, self.interface_embeds.weight,
                    self.rpctype_embeds.weight, csr, out16=out16,
                    pifc=pifc, prpc=prpc,
                )
            return conv(x, edge_index, edge_embeds, csr=csr, num_nodes=n)

        # act16: BN (and the embed concat above) emit bf16 activations so
        # every conv's fused QKVS GEMM and its backward read/write 16-bit
        # streams; gate matches the linear16 gate in forward_fused.
        # training in act16 mode: conv + BN are one autograd node, so that the
        # attention backward applies the BN backward (the BN keep mask exists
        # for n > 0 at the widths bn_attn_fuse_enabled names)
        fuse_bn = (out16 and self.training and n > 0
                   and ops.bn_attn_fuse_enabled(hidden))
        for i, conv in enumerate(self.convs[:-1]):
            bn = self.bns[i]
            if fuse_bn:
                pifc, prpc = ptables.get(id(conv), (None, None))
                x = conv.forward_fused_bn(
                    x, edge_attr, self.interface_embeds.weight,
                    self.rpctype_embeds.weight, csr, bn,
                    comm=self._bn_comm, dropout_p=self.dropout,
                    pifc=pifc, prpc=prpc,
                )
            else:
                x = run_conv(conv, x, out16=out16)
                # dropout fused into the BN epilogue (K8); the CPU oracle
                # path applies torch dropout inside batchnorm_relu
                x = ops.batchnorm_relu(
                    x, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                    bn.momentum, bn.eps, self.training, fuse_relu=True,
                    comm=self._bn_comm, out16=out16, dropout_p=self.dropout,
                )
            if self.training and bn.track_running_stats and bn.num_batches_tracked is not None:
                bn.num_batches_tracked += 1
        if fused:
            # last conv + pool as one op: a loss on global_predict alone
            # then never spreads the pool's gradient over [N, H]
            conv = self.convs[-1]
            pifc, prpc = ptables.get(id(conv), (None, None))
            x, mean_x = conv.forward_fused_pool(
                x, edge_attr, self.interface_embeds.weight,
                self.rpctype_embeds.weight, csr, pattern_probs,
                pattern_num_nodes, batch, num_graphs, pifc=pifc, prpc=prpc)
        else:
            x = run_conv(self.convs[-1], x)
            mean_x = ops.pattern_pool(x, pattern_probs, pattern_num_nodes,
                                      batch, num_graphs)
        local_predict = ops.linear(x, self.local_linear.weight, self.local_linear.bias)
        entry_vec = ops.embedding(entry_id, self.entry_embeds.weight)
        global_predict = torch.cat([mean_x, entry_vec], dim=1)
        h = ops.linear(global_predict, self.global_linear1.weight, self.global_linear1.bias)
        global_predict = ops.linear(F.relu(h), self.global_linear2.weight, self.global_linear2.bias)
        # reference comment says "ensure non-negative" but applies no clamp
        # (model.py:113-114) — reproduced as-is.
        return global_predict, local_predict
