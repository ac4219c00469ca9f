"""Pure-PyTorch (eager) reference implementations of every op in the framework.

These are the numerical oracle: each HIP kernel is tested against the function
here of the same name (fp32, deterministic).  The math mirrors the reference
repo's dependency-internal op surface (kernels K1–K14):

  * edge attention  = PyG 2.4.0 TransformerConv semantics (reference
    model.py:25-52 uses heads=1; per-head form in ``edge_attention``):
      out_i = W_skip x_i + b_skip
            + sum_e softmax_i(<q_i, k_src(e)+e_e>/sqrt(H)) * (v_src(e)+e_e)
  * segment softmax = torch_geometric.utils.softmax (max-subtracted, per dst)
  * pattern pool    = x * p / n  ->  segment-sum by graph (model.py:106-107)
  * quantile loss   = mean(max(tau*e, (tau-1)*e)) (pert_gnn.py:191-193)
"""
from __future__ import annotations

import math

import torch


# ---------------------------------------------------------------------------
# segment primitives
# ---------------------------------------------------------------------------

def segment_softmax(logits: torch.Tensor, dst: torch.Tensor, num_nodes: int) -> torch.Tensor:
    """Numerically-stable softmax over edge logits grouped by destination node.

    Mirrors ``torch_geometric.utils.softmax`` (reference dependency surface,
    SURVEY.md K5).  ``logits``: [E], ``dst``: [E] int64, returns alpha [E].
    """
    if logits.numel() == 0:
        return logits
    seg_max = torch.full((num_nodes,), float("-inf"), dtype=logits.dtype, device=logits.device)
    seg_max = seg_max.scatter_reduce(0, dst, logits, reduce="amax", include_self=True)
    shifted = logits - seg_max.index_select(0, dst)
    expv = shifted.exp()
    seg_sum = torch.zeros(num_nodes, dtype=logits.dtype, device=logits.device)
    seg_sum = seg_sum.index_add(0, dst, expv)
    # rows with no incoming edges never appear in dst; no div-by-zero possible
    return expv / seg_sum.index_select(0, dst)


def scatter_sum(src: torch.Tensor, index: torch.Tensor, dim_size: int) -> torch.Tensor:
    """Segment sum of row vectors: out[index[e]] += src[e].  src: [E,H]."""
    out = torch.zeros(dim_size, *src.shape[1:], dtype=src.dtype, device=src.device)
    return out.index_add(0, index, src)


# ---------------------------------------------------------------------------
# K3-K6: fused edge attention (TransformerConv semantics, concat heads)
# ---------------------------------------------------------------------------

def edge_attention(
    q: torch.Tensor,        # [N,H]  W_q x (dst side)
    k: torch.Tensor,        # [N,H]  W_k x (src side)
    v: torch.Tensor,        # [N,H]  W_v x (src side)
    e: torch.Tensor,        # [E,H]  W_e edge_embed — added to both key and value
    edge_index: torch.Tensor,  # [2,E] (src, dst)
    num_nodes: int,
    skip: torch.Tensor | None = None,  # [N,H] W_skip x + b — added to output
    return_alpha: bool = False,
    heads: int = 1,
):
    """PyG-2.4.0 TransformerConv message+aggregate (concat=True).

    Reference call site: model.py:100,104 via SURVEY.md §2.3 semantics
    (the reference model uses heads=1).  With ``heads`` > 1 head ``t`` owns
    channels ``[tC, (t+1)C)``, ``C = H / heads``:

        logit[e,t] = <q_dst[t], (k_src + e_e)[t]> / sqrt(C)
        alpha[:,t] = softmax over the in-edges of dst, per head
        out_dst[t] = skip_dst[t] + sum_e alpha[e,t] * (v_src + e_e)[t]

    ``return_alpha`` gives alpha as [E] for heads=1 and [E,heads] otherwise.
    """
    src, dst = edge_index[0], edge_index[1]
    h = q.shape[1]
    if heads != 1:
        if heads < 1 or h % heads != 0:
            raise ValueError(f"heads={heads} does not divide H={h}")
        c = h // heads
        ke = (k.index_select(0, src) + e).view(-1, heads, c)
        ve = (v.index_select(0, src) + e).view(-1, heads, c)
        qd = q.index_select(0, dst).view(-1, heads, c)
        logits = (qd * ke).sum(-1) / math.sqrt(c)          # [E,heads]
        alpha = torch.stack(
            [segment_softmax(logits[:, t], dst, num_nodes)
             for t in range(heads)], dim=1)
        out = scatter_sum((alpha.unsqueeze(-1) * ve).reshape(-1, h), dst,
                          num_nodes)
        if skip is not None:
            out = out + skip
        if return_alpha:
            return out, alpha
        return out
    ke = k.index_select(0, src) + e
    ve = v.index_select(0, src) + e
    logits = (q.index_select(0, dst) * ke).sum(-1) / math.sqrt(h)
    alpha = segment_softmax(logits, dst, num_nodes)
    out = scatter_sum(alpha.unsqueeze(-1) * ve, dst, num_nodes)
    if skip is not None:
        out = out + skip
    if return_alpha:
        return out, alpha
    return out


def edge_attention_fused_infer(
    qkvs: torch.Tensor,       # [N,4H]  q | k | v | skip segments
    pifc: torch.Tensor,       # [Vi,H]  interface_table @ we_ifc^T
    prpc: torch.Tensor,       # [Vr,H]  rpctype_table  @ we_rpc^T
    edge_attr: torch.Tensor,  # [E,>=2] int64, CSR (destination-sorted) order
    csr,                      # (row_ptr, csr_src, ...) from the collator
    bn_scale: torch.Tensor | None = None,  # [H] folded eval-mode BN scale
    bn_shift: torch.Tensor | None = None,  # [H] folded eval-mode BN shift
    relu: bool = False,
    out16: bool = False,
    heads: int = 1,
):
    """fp32 oracle of the forward-only fused attention (K-inference):
    ``edge_attention`` on the four segments of ``qkvs`` with the per-edge
    embedding P_ifc[a0] + P_rpc[a1], then the folded BatchNorm affine, then
    the ReLU.  All math is fp32 whatever the input dtypes; ``out16`` rounds
    the result to bf16 once at the end, like the kernel's single store."""
    row_ptr, csr_src = csr[0], csr[1]
    n = qkvs.shape[0]
    h = qkvs.shape[1] // 4
    q, k, v, skip = (t.float() for t in qkvs.split(h, dim=1))
    e = (pifc.float().index_select(0, edge_attr[:, 0])
         + prpc.float().index_select(0, edge_attr[:, 1]))
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(
        torch.arange(n, dtype=torch.long, device=qkvs.device), deg)
    edge_index = torch.stack([csr_src.long(), dst])
    out = edge_attention(q, k, v, e, edge_index, n, skip, heads=heads)
    if bn_scale is not None:
        out = out * bn_scale.float() + bn_shift.float()
    if relu:
        out = torch.relu(out)
    return out.to(torch.bfloat16) if out16 else out


# ---------------------------------------------------------------------------
# K1 + K11: categorical embedding sum + feature concat
# ---------------------------------------------------------------------------

def embed_concat_node(x_raw: torch.Tensor, cat_X: torch.Tensor, tables: list[torch.Tensor]) -> torch.Tensor:
    """x = [x_raw ‖ sum_i table_i[cat_X[:,i]]]  (model.py:87-90)."""
    acc = tables[0].index_select(0, cat_X[:, 0])
    for i in range(1, len(tables)):
        acc = acc + tables[i].index_select(0, cat_X[:, i])
    return torch.cat([x_raw, acc], dim=1)


def embed_concat_edge(edge_attr: torch.Tensor, interface_table: torch.Tensor, rpctype_table: torch.Tensor) -> torch.Tensor:
    """edge_embeds = [ifc[attr[:,0]] ‖ rpc[attr[:,1]]]  (model.py:91-97)."""
    return torch.cat(
        [interface_table.index_select(0, edge_attr[:, 0]),
         rpctype_table.index_select(0, edge_attr[:, 1])],
        dim=1,
    )


# ---------------------------------------------------------------------------
# K9 + K10: pattern-probability weighting + global add pool
# ---------------------------------------------------------------------------

def pattern_pool(
    x: torch.Tensor,                  # [N,H]
    pattern_probs: torch.Tensor,      # [N,1] per-node pattern probability
    pattern_num_nodes: torch.Tensor,  # [N,1] nodes in the node's pattern
    batch: torch.Tensor,              # [N] graph id per node
    num_graphs: int,
) -> torch.Tensor:
    """x*p/n -> segment-sum by graph (model.py:106-107)."""
    weighted = x * pattern_probs / pattern_num_nodes
    return scatter_sum(weighted, batch, num_graphs)


# ---------------------------------------------------------------------------
# K12/K13: loss + eval metrics
# ---------------------------------------------------------------------------

def quantile_loss(y: torch.Tensor, y_hat: torch.Tensor, tau: float) -> torch.Tensor:
    """Pinball loss, mean over batch (pert_gnn.py:191-193)."""
    e = y - y_hat
    return torch.mean(torch.maximum(tau * e, (tau - 1) * e))


def eval_metrics(y: torch.Tensor, y_hat: torch.Tensor, tau: float):
    """Returns (sum |err|, sum |err|/y, sum pinball) — reference accumulates
    sums then divides by dataset size (pert_gnn.py:284-289).  Division by y is
    reproduced as-is (quirk 13: MAPE undefined at y==0)."""
    err = y_hat - y
    abs_err = err.abs()
    mae_sum = abs_err.sum()
    mape_sum = (abs_err / y).sum()
    e = y - y_hat
    q_sum = torch.maximum(tau * e, (tau - 1) * e).sum()
    return mae_sum, mape_sum, q_sum


# ---------------------------------------------------------------------------
# multi-level quantile heads: y [B], y_hat [B, Q], taus 1..8 increasing levels
# ---------------------------------------------------------------------------

MAX_QUANTILES = 8


def check_taus(taus) -> tuple:
    """``taus`` as a tuple of floats: 1..8 strictly increasing levels in
    (0, 1); anything else is a ValueError."""
    try:
        levels = tuple(float(t) for t in taus)
    except TypeError:
        raise ValueError(f"taus must be a sequence of levels, got {taus!r}") from None
    if not 1 <= len(levels) <= MAX_QUANTILES:
        raise ValueError(
            f"taus must hold 1..{MAX_QUANTILES} levels, got {len(levels)}: {levels}")
    for q, t in enumerate(levels):
        if not 0.0 < t < 1.0:  # also refuses NaN
            raise ValueError(f"taus[{q}]={t} is outside (0, 1)")
        if q and not t > levels[q - 1]:
            raise ValueError(f"taus must be strictly increasing, got {levels}")
    return levels


def point_level(taus) -> int:
    """Index of the level closest to 0.5 (the lower index on a tie): the
    column MAE and MAPE are reported for."""
    levels = check_taus(taus)
    return min(range(len(levels)), key=lambda q: (abs(levels[q] - 0.5), q))


def _check_multi(y: torch.Tensor, y_hat: torch.Tensor, levels: tuple):
    if y.dim() != 1 or y_hat.dim() != 2:
        raise ValueError(
            f"expected y [B] and y_hat [B, Q], got {tuple(y.shape)} and "
            f"{tuple(y_hat.shape)}")
    if y_hat.shape[0] != y.shape[0] or y_hat.shape[1] != len(levels):
        raise ValueError(
            f"y_hat {tuple(y_hat.shape)} does not match y {tuple(y.shape)} "
            f"and {len(levels)} levels")


def _pinball_terms(y, y_hat, levels):
    tau = torch.tensor(levels, dtype=y_hat.dtype, device=y_hat.device)
    e = y.unsqueeze(1) - y_hat
    return torch.maximum(tau * e, (tau - 1) * e)


def quantile_loss_multi(y: torch.Tensor, y_hat: torch.Tensor, taus):
    """(loss, per_level_sums): the pinball loss summed over the Q levels and
    averaged over the B rows, and the undivided pinball sum of every level
    ``[Q]``.  Q = 1 is ``quantile_loss``; B = 0 gives NaN and zeros."""
    levels = check_taus(taus)
    _check_multi(y, y_hat, levels)
    terms = _pinball_terms(y, y_hat, levels)
    sums = terms.sum(dim=0)
    if y.shape[0] == 0:
        return sums.sum() + float("nan"), sums
    return sums.sum() / y.shape[0], sums


def eval_metrics_multi(y: torch.Tensor, y_hat: torch.Tensor, taus,
                       point: int | None = None) -> torch.Tensor:
    """``[3 + 2Q]`` sums: ``[mae, mape, crossing rows, pinball[Q],
    covered rows[Q]]``.  MAE and MAPE are of column ``point`` (default
    ``point_level(taus)``), MAPE divides by y as it is (quirk 13); level q
    covers row i when ``y_i <= y_hat_iq``; a row crosses when any of its
    predictions is below the one before it."""
    levels = check_taus(taus)
    _check_multi(y, y_hat, levels)
    if point is None:
        point = point_level(levels)
    abs_err = (y_hat[:, point] - y).abs()
    cross = (y_hat[:, 1:] < y_hat[:, :-1]).any(dim=1)
    cover = y.unsqueeze(1) <= y_hat
    dt = y_hat.dtype
    return torch.cat([
        torch.stack([abs_err.sum(), (abs_err / y).sum(), cross.to(dt).sum()]),
        _pinball_terms(y, y_hat, levels).sum(dim=0),
        cover.to(dt).sum(dim=0),
    ])


def quantile_rearrange(y_hat: torch.Tensor) -> torch.Tensor:
    """Every row sorted ascending: the monotone rearrangement of crossing
    quantile predictions.  With increasing levels it never increases a
    row's summed pinball loss."""
    if y_hat.dim() != 2:
        raise ValueError(f"expected y_hat [B, Q], got {tuple(y_hat.shape)}")
    return torch.sort(y_hat, dim=1).values
