"""Dispatching functional ops: HIP kernels on GPU, eager oracle on CPU.

Every op takes/returns plain tensors so the model code is path-agnostic.
Edge order contract: edges are ALWAYS destination-sorted (CSR order) inside a
collated batch — the collator (pertgnn/data/collate.py, reference K17) emits
them that way, so ``row_ptr``/``csr_src`` describe ``edge_attr``/``e`` rows
directly and no per-kernel permutation is needed.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import reference as ref
from .backend import ext, use_hip


def deterministic() -> bool:
    """PERTGNN_DETERMINISTIC=1 makes training bitwise run-to-run
    reproducible: BN statistics reduce through per-block slabs in fixed
    order, vocab/embedding table grads take the two-phase grouped scatter
    (stable sort, no atomics; the attention's two P-table grads at H=256/512
    take the fixed-order list sums of ``edge_table_grad`` instead, which
    large interface tables use in every mode), and the split-K wgrad GEMMs collapse to one
    K-slice (the C++ launchers read the same env).  The activation-gradient
    path is deterministic either way.  Verification/debugging mode: combine
    with --no-hipgraph (the first grouping per batch uses bincount, which
    syncs); eager stepping dominates the cost at small batches."""
    import os
    return os.environ.get("PERTGNN_DETERMINISTIC", "0") == "1"


def grad_sink(p):
    """The gradient sink of parameter ``p`` for the forward being recorded,
    or None.  The sink is the slice of FusedAdam's ``flat_grad`` that
    ``p.grad`` is pinned to; a backward op given one adds the parameter's
    gradient straight into it and returns None for ``p``, so autograd's
    AccumulateGrad (one small add launch per parameter) never runs and the
    op clears no buffer of its own.  The wrappers hand such a parameter to
    their autograd node detached (``_sunk``), so no AccumulateGrad node and
    none of its hooks exist for that use.  Used only while all of these hold:
    grad mode is on and ``p`` requires grad; ``p.grad`` still aliases the
    sink (``zero_grad(set_to_none=True)`` or a re-pointed ``.grad`` restore
    the return path until the optimizer's ``zero_grad`` re-pins); no live
    FlatGradAllReduce (enabled, distributed) waits for ``p``'s
    post-accumulate hook, which needs autograd to see the parameter;
    PERTGNN_NO_GRAD_SINK is not 1 (read per call, so one process can run
    both paths)."""
    sink = getattr(p, "_grad_sink", None)
    if sink is None or not p.requires_grad or not torch.is_grad_enabled():
        return None
    import os
    if os.environ.get("PERTGNN_NO_GRAD_SINK", "0") == "1":
        return None
    g = p.grad
    if g is None or g.data_ptr() != sink.data_ptr() or g.shape != sink.shape:
        return None
    engine = getattr(p, "_grad_sink_engine", None)
    if engine is not None and engine.enabled and engine.comm.distributed:
        return None
    return sink


def _sunk(p, sink):
    """``p`` as its autograd node takes it: detached when its gradient goes
    to ``sink`` (the node returns None for it either way, but a detached
    input has no AccumulateGrad node whose hooks would still run)."""
    return p if sink is None or p is None else p.detach()


_SINK_ANCHOR: dict = {}


def _sink_anchor(device):
    """An empty leaf that requires grad, passed to every node that may take
    its parameters detached: with no other input requiring grad (the first
    layer's linear16 reads the input features) the node would otherwise
    drop out of the graph and its backward, which fills the sinks, would
    never run.  Its own gradient is always None."""
    key = str(device)
    a = _SINK_ANCHOR.get(key)
    if a is None:
        a = torch.empty(0, device=device, requires_grad=True)
        _SINK_ANCHOR[key] = a
    return a


def _table_grad(m, g, idx, rows, h, col_off):
    """dtable[v] = segment-sum of g[:, col_off:col_off+h] by idx — LDS vocab
    accumulator for small tables, work-balanced deterministic grouped
    scatter otherwise (always, under PERTGNN_DETERMINISTIC=1).  bf16 g is
    consumed DIRECTLY by both paths (fp32 accumulation inside the kernels —
    no upcast pass, half the gather traffic)."""
    if rows * h * 4 <= 160 * 1024 and not deterministic():
        if g.dtype == torch.bfloat16 and (
                h % 64 != 0 or 4 * rows * 64 * 4 > 160 * 1024):
            g = g.float()
        return m.vocab_scatter(g, idx, rows, h, col_off)
    order, ptr, row_map, wave_start, row_map2, wave_start2 = _group_by(idx, rows)
    if g.dtype not in (torch.float32, torch.bfloat16):
        g = g.float()
    return m.embed_grouped_scatter_bal(g, order, ptr, row_map, wave_start,
                                       row_map2, wave_start2, rows, h, col_off)


_GROUP_CACHE: "dict" = __import__("collections").OrderedDict()
_GROUP_CACHE_BYTES = [0]
_GROUP_CACHE_CAP = 64 * 1024 * 1024  # bytes of cached order/ptr tensors


_SCATTER_ITERS = None


def _scatter_iters() -> int:
    """Gathers per wave in the balanced scatter (PERTGNN_SCATTER_ITERS):
    smaller = more waves and more partial traffic, larger = longer serial
    chains per wave."""
    global _SCATTER_ITERS
    if _SCATTER_ITERS is None:
        import os
        try:
            _SCATTER_ITERS = max(8, int(os.environ.get("PERTGNN_SCATTER_ITERS", "64")))
        except ValueError:
            _SCATTER_ITERS = 64
    return _SCATTER_ITERS


def _group_by(idx: torch.Tensor, rows: int, iters_target: int | None = None):
    """Group positions by index value: returns (order int32, ptr
    int32[rows+1], row_map int32[n_waves], wave_start int32[rows+1]) for the
    work-balanced deterministic grouped scatter.  Cached so the sort +
    bincount (which sync) run once per resident batch.

    ``row_map``/``wave_start`` assign GPU waves per row PROPORTIONAL to its
    group size (~``iters_target`` gathers per wave): a uniform sub-wave
    count collapses under skew — PERT intra-ms edges all carry interface id
    0, putting ~half the batch's edges in one row
    (measured 39 ms vs 1 ms for the same volume evenly spread).

    The key is taken from the VIEW the caller holds (data_ptr + stride +
    numel), before any ``.contiguous()`` copy — callers like the fused
    attention backward pass ``edge_attr[:, 0]`` column views, which are
    stable across steps while a fresh ``.contiguous()`` tensor never is.
    LRU-evicted at a byte budget (the cached view reference pins its base
    storage so the allocator cannot recycle the keyed data_ptr while the
    entry is live)."""
    if iters_target is None:
        iters_target = _scatter_iters()
    key = (idx.data_ptr(), idx.numel(), tuple(idx.stride()), rows,
           iters_target)
    hit = _GROUP_CACHE.get(key)
    if hit is not None:
        _GROUP_CACHE.move_to_end(key)
        return hit[1], hit[2], hit[3], hit[4], hit[5], hit[6]
    idx_c = idx.contiguous()
    order = torch.argsort(idx_c, stable=True)  # ties in input order: the
    # grouped kernels' reduction order is then fully determined
    counts = torch.bincount(idx_c, minlength=rows)
    ptr = torch.zeros(rows + 1, dtype=torch.int32, device=idx.device)
    ptr[1:] = counts.cumsum(0).to(torch.int32)
    order32 = order.to(torch.int32)

    def assign(counts_h):
        """waves per row ~ group size (empty rows still get one wave so the
        final fold writes their zeros); returns (row_map, wave_start) CPU."""
        wpr = torch.clamp_min((counts_h + iters_target - 1) // iters_target, 1)
        ws = torch.zeros(counts_h.numel() + 1, dtype=torch.int32)
        ws[1:] = wpr.cumsum(0).to(torch.int32)
        rm = torch.repeat_interleave(
            torch.arange(counts_h.numel(), dtype=torch.int32), wpr)
        return rm, ws, wpr

    counts_h = counts.cpu()  # bincount above synced already
    row_map, wave_start, wpr = assign(counts_h)
    # second reduction level when any row's partial count is itself big
    # (the interface-0 mega-group: ~half the edges in one row)
    if int(wpr.max()) > 64:
        row_map2, wave_start2, _ = assign(wpr)
    else:
        row_map2 = torch.empty(0, dtype=torch.int32)
        wave_start2 = torch.empty(0, dtype=torch.int32)
    dev = idx.device
    row_map, wave_start = row_map.to(dev), wave_start.to(dev)
    row_map2, wave_start2 = row_map2.to(dev), wave_start2.to(dev)
    nbytes = (order32.numel() + ptr.numel() + row_map.numel()
              + wave_start.numel() + row_map2.numel()
              + wave_start2.numel()) * 4
    while _GROUP_CACHE and _GROUP_CACHE_BYTES[0] + nbytes > _GROUP_CACHE_CAP:
        _, old = _GROUP_CACHE.popitem(last=False)
        _GROUP_CACHE_BYTES[0] -= old[-1]
    _GROUP_CACHE[key] = (idx, order32, ptr, row_map, wave_start, row_map2,
                         wave_start2, nbytes)
    _GROUP_CACHE_BYTES[0] += nbytes
    return order32, ptr, row_map, wave_start, row_map2, wave_start2


# ---------------------------------------------------------------------------
# edge-table gradient plan: both P-table grads from ONE pass over de
# ---------------------------------------------------------------------------

class EdgeTablePlan(NamedTuple):
    """Three levels of row lists (all int32; list w of a level is
    ``idx[lptr[w]:lptr[w+1]]``) that turn de [E, h] into the V ifc rows
    followed by the R rpc rows:

    level 1  chunks of at most C edges with one (ifc, rpc) key -> partial
             rows 0..n1 (idx1 = the stable sort order over the edges)
    level 2  for every output row with more than C members, groups of at
             most C of them -> partial rows n1..n1+n2
    level 3  one list per output row over the partial rows: its members, or
             its level-2 rows if it has any (longer than C only when a row
             has more than C*C members); empty for an unused table row
    """
    idx1: torch.Tensor
    lptr1: torch.Tensor
    idx2: torch.Tensor
    lptr2: torch.Tensor
    idx3: torch.Tensor
    lptr3: torch.Tensor
    n1: int
    n2: int
    V: int
    R: int
    C: int

    def tensors(self):
        return (self.idx1, self.lptr1, self.idx2, self.lptr2, self.idx3,
                self.lptr3)


def _chunk_segments(counts: torch.Tensor, c: int):
    """Cut back-to-back segments of the given lengths into chunks of at most
    ``c``: returns (segment id per chunk, chunk bounds [n_chunks+1])."""
    total = int(counts.sum())
    cps = (counts + c - 1) // c
    n_chunks = int(cps.sum())
    seg = torch.repeat_interleave(torch.arange(counts.numel()), cps)
    first = cps.cumsum(0) - cps
    seg_start = counts.cumsum(0) - counts
    start = seg_start[seg] + (torch.arange(n_chunks) - first[seg]) * c
    return seg, torch.cat([start, torch.tensor([total])])


def _build_edge_table_plan(ifc, rpc, V: int, R: int, C: int):
    """Host-side plan construction on CPU int64 index vectors."""
    E = ifc.numel()
    if E and (int(ifc.min()) < 0 or int(ifc.max()) >= V
              or int(rpc.min()) < 0 or int(rpc.max()) >= R):
        raise IndexError("edge_attr index outside the P tables")
    key = ifc * R + rpc
    order = torch.argsort(key, stable=True)
    ukeys, runs = torch.unique_consecutive(key[order], return_counts=True)
    # level 1: a chunk never crosses a key
    run_of_chunk, lptr1 = _chunk_segments(runs, C)
    ck = ukeys[run_of_chunk]
    n1 = ck.numel()
    # members of the V + R outputs among the level-1 rows (ck is ascending:
    # an ifc row's members are contiguous; an rpc row's come out ascending
    # from the stable sort)
    members = torch.cat([torch.arange(n1),
                         torch.argsort(ck % R, stable=True)])
    cnt = torch.cat([torch.bincount(ck // R, minlength=V),
                     torch.bincount(ck % R, minlength=R)])
    out_of_member = torch.repeat_interleave(torch.arange(V + R), cnt)
    big = cnt > C
    in_big = big[out_of_member]
    # level 2 over the member lists of the over-long outputs
    idx2 = members[in_big]
    _, lptr2 = _chunk_segments(cnt[big], C)
    n2 = lptr2.numel() - 1
    # level 3: members directly, or the output's level-2 rows
    len3 = torch.where(big, (cnt + C - 1) // C, cnt)
    lptr3 = torch.cat([torch.zeros(1, dtype=torch.long), len3.cumsum(0)])
    from_l2 = big[torch.repeat_interleave(torch.arange(V + R), len3)]
    idx3 = torch.empty(int(len3.sum()), dtype=torch.long)
    idx3[from_l2] = n1 + torch.arange(n2)
    idx3[~from_l2] = members[~in_big]
    # what the kernels rely on (they do not bounds-check)
    assert order.numel() == E and int(lptr1[-1]) == E
    assert int(lptr2[-1]) == idx2.numel() and int(lptr3[-1]) == idx3.numel()
    assert idx2.numel() == 0 or int(idx2.max()) < n1
    assert idx3.numel() == 0 or int(idx3.max()) < n1 + n2
    assert max(E, n1 + n2, idx3.numel(), idx2.numel()) < 2 ** 31
    i32 = lambda t: t.to(torch.int32)
    return EdgeTablePlan(i32(order), i32(lptr1), i32(idx2), i32(lptr2),
                         i32(idx3), i32(lptr3), n1, n2, V, R, C)


def edge_table_plan(edge_attr: torch.Tensor, V: int, R: int,
                    C: int | None = None) -> EdgeTablePlan:
    """Plan for ``edge_table_grad`` over ``edge_attr[:, 0]`` (ifc, < V) and
    ``edge_attr[:, 1]`` (rpc, < R); ``C`` defaults to ``_scatter_iters()``.
    Built on the host (syncs once) and cached like ``_group_by``: keyed on
    the ``edge_attr`` view, in the same LRU byte budget, so a resident batch
    pays for it in the warm-up steps and a hit neither syncs nor launches."""
    if C is None:
        C = _scatter_iters()
    key = ("edge_table", edge_attr.data_ptr(), edge_attr.numel(),
           tuple(edge_attr.stride()), V, R, C)
    hit = _GROUP_CACHE.get(key)
    if hit is not None:
        _GROUP_CACHE.move_to_end(key)
        return hit[1]
    ea = edge_attr[:, :2].cpu().long()
    plan = _build_edge_table_plan(ea[:, 0].contiguous(), ea[:, 1].contiguous(),
                                  V, R, C)
    dev = edge_attr.device
    plan = plan._replace(**{f: getattr(plan, f).to(dev) for f in
                            ("idx1", "lptr1", "idx2", "lptr2", "idx3",
                             "lptr3")})
    nbytes = sum(t.numel() for t in plan.tensors()) * 4
    while _GROUP_CACHE and _GROUP_CACHE_BYTES[0] + nbytes > _GROUP_CACHE_CAP:
        _, old = _GROUP_CACHE.popitem(last=False)
        _GROUP_CACHE_BYTES[0] -= old[-1]
    _GROUP_CACHE[key] = (edge_attr, plan, nbytes)
    _GROUP_CACHE_BYTES[0] += nbytes
    return plan


def _build_cat_table_plan(idx, rows: int, C: int):
    """Single-key plan on a CPU int64 index vector: the ``EdgeTablePlan``
    levels for ``rows`` outputs keyed by ``idx`` alone (V = rows, R = 0)."""
    n = idx.numel()
    if n and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        raise IndexError("category index outside the embedding table")
    order = torch.argsort(idx, stable=True)
    counts = torch.bincount(idx, minlength=rows)
    # level 1: chunks of one category, ascending by category
    out_of_member, lptr1 = _chunk_segments(counts, C)
    n1 = out_of_member.numel()
    members = torch.arange(n1)
    cnt = (counts + C - 1) // C
    big = cnt > C
    in_big = big[out_of_member]
    idx2 = members[in_big]
    _, lptr2 = _chunk_segments(cnt[big], C)
    n2 = lptr2.numel() - 1
    len3 = torch.where(big, (cnt + C - 1) // C, cnt)
    lptr3 = torch.cat([torch.zeros(1, dtype=torch.long), len3.cumsum(0)])
    from_l2 = big[torch.repeat_interleave(torch.arange(rows), len3)]
    idx3 = torch.empty(int(len3.sum()), dtype=torch.long)
    idx3[from_l2] = n1 + torch.arange(n2)
    idx3[~from_l2] = members[~in_big]
    # what the kernels rely on (they do not bounds-check)
    assert order.numel() == n and int(lptr1[-1]) == n
    assert int(lptr2[-1]) == idx2.numel() and int(lptr3[-1]) == idx3.numel()
    assert idx2.numel() == 0 or int(idx2.max()) < n1
    assert idx3.numel() == 0 or int(idx3.max()) < n1 + n2
    assert max(n, n1 + n2, idx3.numel(), idx2.numel()) < 2 ** 31
    i32 = lambda t: t.to(torch.int32)
    return EdgeTablePlan(i32(order), i32(lptr1), i32(idx2), i32(lptr2),
                         i32(idx3), i32(lptr3), n1, n2, rows, 0, C)


def cat_table_plan(cat_idx: torch.Tensor, rows: int,
                   C: int | None = None) -> EdgeTablePlan:
    """Plan for ``embed_dgrad_fold`` over the category index of every node
    (< rows); ``C`` defaults to ``_scatter_iters()``.  Built on the host
    (validates the indices, syncs once) and cached like ``edge_table_plan``:
    keyed on the index view, in the same LRU byte budget, so a hit neither
    syncs nor launches."""
    if C is None:
        C = _scatter_iters()
    key = ("cat_table", cat_idx.data_ptr(), cat_idx.numel(),
           tuple(cat_idx.stride()), rows, C)
    hit = _GROUP_CACHE.get(key)
    if hit is not None:
        _GROUP_CACHE.move_to_end(key)
        return hit[1]
    plan = _build_cat_table_plan(cat_idx.cpu().long().contiguous(), rows, C)
    dev = cat_idx.device
    plan = plan._replace(**{f: getattr(plan, f).to(dev) for f in
                            ("idx1", "lptr1", "idx2", "lptr2", "idx3",
                             "lptr3")})
    nbytes = sum(t.numel() for t in plan.tensors()) * 4
    while _GROUP_CACHE and _GROUP_CACHE_BYTES[0] + nbytes > _GROUP_CACHE_CAP:
        _, old = _GROUP_CACHE.popitem(last=False)
        _GROUP_CACHE_BYTES[0] -= old[-1]
    _GROUP_CACHE[key] = (cat_idx, plan, nbytes)
    _GROUP_CACHE_BYTES[0] += nbytes
    return plan


def apply_plan_reference(plan: EdgeTablePlan, de: torch.Tensor):
    """The three passes of ``edge_table_grad`` with plain torch indexing
    (fp32 accumulation, fp64 for fp64 input): returns (dP_ifc [V, h],
    dP_rpc [R, h]).  Test oracle for the plan and the kernel."""
    acc = torch.float64 if de.dtype == torch.float64 else torch.float32
    h = de.shape[1]

    def level(src, idx, lptr):
        lens = (lptr[1:] - lptr[:-1]).long()
        seg = torch.repeat_interleave(
            torch.arange(lens.numel(), device=src.device), lens)
        out = torch.zeros(lens.numel(), h, dtype=acc, device=src.device)
        return out.index_add_(0, seg, src.index_select(0, idx.long()))

    p1 = level(de.to(acc), plan.idx1, plan.lptr1)
    p2 = level(p1, plan.idx2, plan.lptr2)
    out = level(torch.cat([p1, p2]), plan.idx3, plan.lptr3)
    return out[:plan.V], out[plan.V:]


def _edge_table_grads(m, de, pifc, prpc, edge_attr):
    """dP_ifc, dP_rpc from de.  Large ifc tables (or deterministic mode) at
    h in {256, 512} take the single-pass list-sum op, which stores the
    tables' dtype directly; everything else is the two per-table scatters
    plus the cast."""
    V, R, h = pifc.shape[0], prpc.shape[0], de.shape[1]
    if h in (256, 512) and (V * h * 4 > 160 * 1024 or deterministic()):
        if de.dtype not in (torch.float32, torch.bfloat16):
            de = de.float()
        plan = edge_table_plan(edge_attr, V, R)
        od = pifc.dtype if pifc.dtype == torch.bfloat16 else torch.float32
        out = m.edge_table_grad(de, *plan.tensors(), V, R, od).to(pifc.dtype)
        return out[:V], out[V:]
    dpifc = _table_grad(m, de, edge_attr[:, 0], V, h, 0)
    dprpc = _table_grad(m, de, edge_attr[:, 1], R, h, 0)
    if dpifc.dtype != pifc.dtype:  # bf16 P tables: match grad dtype
        dpifc = dpifc.to(pifc.dtype)
        dprpc = dprpc.to(prpc.dtype)
    return dpifc, dprpc


# ---------------------------------------------------------------------------
# fused edge attention (K3-K6 fwd, K15 bwd)
# ---------------------------------------------------------------------------

class _EdgeAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, e, skip, row_ptr, csr_src, col_ptr, csc_dst, csc_eid):
        m = ext()
        out, alpha = m.edge_attn_fwd(q, k, v, e, row_ptr, csr_src, skip)
        ctx.save_for_backward(q, k, v, e, alpha, row_ptr, csr_src, col_ptr, csc_dst, csc_eid)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, e, alpha, row_ptr, csr_src, col_ptr, csc_dst, csc_eid = ctx.saved_tensors
        m = ext()
        dq, dk, dv, de = m.edge_attn_bwd(
            g.contiguous(), q, k, v, e, alpha, row_ptr, csr_src, col_ptr, csc_dst, csc_eid
        )
        # skip grad is g itself
        return dq, dk, dv, de, g, None, None, None, None, None


def _device_csr(edge_index, num_nodes):
    """CSR/CSC arrays for an arbitrary-order edge list, on its own device.
    Returns (perm, csr_tuple): ``perm`` maps original edge order -> CSR
    order.  The collator normally provides these (pre-sorted, no perm);
    this path serves direct module-API callers (reference call signature,
    model.py:76-86) who pass only ``edge_index``."""
    dev = edge_index.device
    src, dst = edge_index[0], edge_index[1]
    perm = torch.argsort(dst, stable=True)
    src_s = src.index_select(0, perm)
    dst_s = dst.index_select(0, perm)
    row_ptr = torch.zeros(num_nodes + 1, dtype=torch.int32, device=dev)
    row_ptr[1:] = torch.bincount(dst_s, minlength=num_nodes).cumsum(0).to(torch.int32)
    perm2 = torch.argsort(src_s, stable=True)
    col_ptr = torch.zeros(num_nodes + 1, dtype=torch.int32, device=dev)
    col_ptr[1:] = torch.bincount(src_s, minlength=num_nodes).cumsum(0).to(torch.int32)
    csr = (row_ptr, src_s.to(torch.int32), col_ptr,
           dst_s.index_select(0, perm2).to(torch.int32), perm2.to(torch.int32))
    return perm, csr


def edge_attention(q, k, v, e, skip, edge_index, num_nodes, csr=None,
                   heads=1):
    """out_i = skip_i + sum_e softmax_i(<q_i, k_src+e>/sqrt(H)) (v_src+e).

    ``heads`` > 1 (concat, C = H/heads): the same formula per head on its
    channel slice, scaled by 1/sqrt(C).  The reference-layout HIP kernel
    behind this op is the op-parity path and stays single-head, so on device
    tensors it runs ONCE PER HEAD on contiguous channel slices and the
    results are concatenated — correct, not fast (heads x the launches and
    index traffic, plus the slice copies).  The production path is
    ``edge_attention_fused``, whose kernels are multi-head natively.

    ``csr``: (row_ptr, csr_src, col_ptr, csc_dst, csc_eid) from the collator
    (edges already CSR-ordered).  When absent on the HIP path — the reference
    module-API call signature — CSR is built on the fly from ``edge_index``
    and ``e`` is permuted to match (autograd routes ``de`` back through the
    index_select).
    """
    if use_hip(q):
        if csr is None:
            perm, csr = _device_csr(edge_index, num_nodes)
            e = e.index_select(0, perm)
        row_ptr, csr_src, col_ptr, csc_dst, csc_eid = csr
        if heads == 1:
            return _EdgeAttentionFn.apply(q, k, v, e, skip, row_ptr, csr_src, col_ptr, csc_dst, csc_eid)
        h = q.shape[1]
        if heads < 1 or h % heads != 0:
            raise ValueError(f"heads={heads} does not divide H={h}")
        c = h // heads
        outs = [
            _EdgeAttentionFn.apply(
                *(t[:, i * c:(i + 1) * c].contiguous()
                  for t in (q, k, v, e, skip)),
                row_ptr, csr_src, col_ptr, csc_dst, csc_eid)
            for i in range(heads)
        ]
        return torch.cat(outs, dim=1)
    return ref.edge_attention(q, k, v, e, edge_index, num_nodes, skip,
                              heads=heads)


class _Linear16Fn(torch.autograd.Function):
    """bf16-activation-mode linear: fp32 x/w in, bf16 out (the QKVS tensor
    stays bf16 through the attention kernels — halves the edge-gather traffic
    and the largest C-writes; operands were already bf16-rounded inside the
    matrix cores, so numerics match the plain bf16-GEMM mode)."""

    @staticmethod
    def forward(ctx, x, w, b, w_sink=None, b_sink=None, anchor=None):
        m = ext()
        bb = b if b is not None else torch.empty(0, dtype=torch.float32, device=x.device)
        fp16c = gemm_precision() == "fp16"  # fp16 matrix cores, bf16 IO
        # gradient sinks of w and b (grad_sink): the wgrad adds into them
        ctx.w_sink, ctx.b_sink = w_sink, b_sink
        # the forward's weight-convert launch also writes the transposed bf16
        # image the dgrad needs (w cannot change in between: it stays a saved
        # tensor, so autograd's version check catches an in-place update)
        ctx.wt16 = None
        if x.dtype == torch.bfloat16:
            if any(ctx.needs_input_grad):
                y, wt16 = m.linear_fwd_a16o16_wt(x, w, bb, fp16c)
                ctx.wt16 = wt16 if wt16.numel() else None
            else:
                y = m.linear_fwd_a16o16(x, w, bb, fp16c)   # x16 in, bf16 out
        else:
            y = m.linear_fwd_bf16_o16(x, w, bb)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.fp16c = fp16c
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        if x.dtype == torch.bfloat16:
            dx = m.linear_dgrad16_o16(g, w, ctx.fp16c, ctx.wt16)
            dw, db = m.linear_wgrad16_b16(g, x, ctx.has_bias, ctx.fp16c,
                                          ctx.w_sink, ctx.b_sink)
        else:
            dx = m.linear_dgrad16(g, w)
            dw, db = m.linear_wgrad16(g, x, ctx.has_bias, ctx.w_sink,
                                      ctx.b_sink)
        if ctx.w_sink is not None:  # dw and db are in the sinks
            return dx, None, None, None, None, None
        return dx, dw, (db if ctx.has_bias else None), None, None, None


def linear16(x, w, b=None):
    # w and b sink together or not at all: one launcher flag covers both
    w_sink = grad_sink(w)
    b_sink = grad_sink(b) if b is not None else None
    if w_sink is None or (b is not None and b_sink is None):
        w_sink = b_sink = None
    if w_sink is None:
        return _Linear16Fn.apply(x, w, b)
    return _Linear16Fn.apply(x, _sunk(w, w_sink), _sunk(b, b_sink), w_sink,
                             b_sink, _sink_anchor(x.device))


def embed_dgrad_fold_enabled() -> bool:
    """Layer-1 dgrad folded into the category-table gradient
    (PERTGNN_NO_EMBED_DGRAD_FOLD=1 keeps the dgrad GEMM and the grouped
    scatter over its output; read per call so one process can run both)."""
    import os
    return os.environ.get("PERTGNN_NO_EMBED_DGRAD_FOLD", "0") != "1"


class EmbedSource(NamedTuple):
    """What produced an ``embed_concat_node`` output (recorded on it as
    ``_embed_src``): columns ``f .. f+h`` of row i are ``table[cat_idx[i]]``,
    the first ``f`` are ``x_raw``, the rest +0."""
    cat_idx: torch.Tensor
    table: torch.Tensor
    f: int
    h: int
    x_raw_requires_grad: bool


class _Linear16EmbedFn(torch.autograd.Function):
    """``linear16`` of the first layer when the only gradient its operand
    ``x`` = [x_raw | table[cat_idx] | 0] would carry is the category table's:
    the table is a direct input and x comes in detached.  With G[c] the sum
    of the dqkvs rows of category c,  dtable = G . bf16(w)[:, f:f+h]
    (``embed_dgrad_fold``): the [N, k_padded] dgrad GEMM, its output and the
    strided gather over it never run, and the dqkvs rows are summed in fp32
    before the one multiplication instead of being rounded to bf16 per node.
    dw and db are ``linear_wgrad16_b16``'s, bit for bit."""

    @staticmethod
    def forward(ctx, x, w, b, table, cat_idx, f, w_sink, b_sink, t_sink,
                anchor):
        m = ext()
        bb = b if b is not None else torch.empty(0, dtype=torch.float32, device=x.device)
        ctx.w_sink, ctx.b_sink, ctx.t_sink = w_sink, b_sink, t_sink
        # no transposed weight image: nothing runs a dgrad
        y = m.linear_fwd_a16o16(x, w, bb, False)
        ctx.save_for_backward(x, w, cat_idx)
        ctx.has_bias = b is not None
        ctx.f, ctx.rows, ctx.h = f, table.shape[0], table.shape[1]
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, cat_idx = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        dw, db = m.linear_wgrad16_b16(g, x, ctx.has_bias, False, ctx.w_sink,
                                      ctx.b_sink)
        dtable = None
        if ctx.t_sink is not None or ctx.needs_input_grad[3]:
            plan = cat_table_plan(cat_idx, ctx.rows)
            dtable = m.embed_dgrad_fold(g, *plan.tensors(), w, ctx.f, ctx.h,
                                        ctx.rows, ctx.t_sink)
            if ctx.t_sink is not None:
                dtable = None
        if ctx.w_sink is not None:  # dw and db are in the sinks
            dw = db = None
        return (None, dw, (db if ctx.has_bias else None), dtable, None, None,
                None, None, None, None)


def linear16_embed(x, w, b=None):
    """``linear16(x, w, b)`` for an ``x`` that ``embed_concat_node`` wrote:
    where the eligibility conditions hold (bf16 operand and bf16 matrix
    cores, one category table that requires grad, no gradient wanted for
    ``x_raw``, h in {256, 512}, the switch on) the fold node above replaces
    ``linear16``; anything else is ``linear16`` unchanged."""
    src = getattr(x, "_embed_src", None)
    if (src is None or not embed_dgrad_fold_enabled()
            or not torch.is_grad_enabled()
            or x.dtype != torch.bfloat16 or gemm_precision() != "bf16"
            or src.x_raw_requires_grad or src.h not in (256, 512)
            or not src.table.requires_grad or not x.requires_grad
            or w.shape[0] != 4 * src.h or src.f + src.h > w.shape[1]
            or x.shape[1] != w.shape[1]):
        return linear16(x, w, b)
    w_sink = grad_sink(w)
    b_sink = grad_sink(b) if b is not None else None
    if w_sink is None or (b is not None and b_sink is None):
        w_sink = b_sink = None
    t_sink = grad_sink(src.table)
    return _Linear16EmbedFn.apply(
        x.detach(), _sunk(w, w_sink), _sunk(b, b_sink),
        _sunk(src.table, t_sink), src.cat_idx, src.f, w_sink, b_sink, t_sink,
        _sink_anchor(x.device))


class _PTablesFn(torch.autograd.Function):
    """All layers' bf16 P tables (``linear16(table, we_l)`` for both embedding
    tables) in one grouped launch.  The 2L tables are separate outputs, so
    autograd hands the backward every ``dP`` at once, after the first layer's
    attention backward: one dgrad launch sums over the layers into the two
    table gradients and one wgrad launch fills all 2L weight gradients."""

    @staticmethod
    def forward(ctx, sinks, anchor, ifc_table, rpc_table, *weights):
        layers = len(weights) // 2
        we_ifc, we_rpc = list(weights[:layers]), list(weights[layers:])
        # gradient sinks (grad_sink) of the two tables and the 2L weights,
        # None where an input has none
        ctx.sinks = sinks
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(ifc_table, rpc_table, *weights)
        return tuple(ext().ptables_fwd(ifc_table, rpc_table, we_ifc, we_rpc))

    @staticmethod
    def backward(ctx, *dps):
        ifc_table, rpc_table, *weights = ctx.saved_tensors
        layers = len(weights) // 2
        none = torch.empty(0, dtype=torch.bfloat16, device=ifc_table.device)
        t_sinks, w_sinks = ctx.sinks[:2], list(ctx.sinks[2:])
        d_ifc, d_rpc, dw = ext().ptables_bwd(
            [none if g is None else g.contiguous() for g in dps],
            ifc_table, rpc_table, weights[:layers], weights[layers:],
            ptable_dgrad_splits(), t_sinks[0], t_sinks[1], w_sinks)
        # dw holds the groups without a sink, in order
        slot, dws = 0, []
        for g, sink in zip(dps, w_sinks):
            dws.append(None if g is None or sink is not None else dw[slot])
            slot += sink is None
        return (None, None,
                None if t_sinks[0] is not None else d_ifc,
                None if t_sinks[1] is not None else d_rpc, *dws)


def ptables_grouped(ifc_table, rpc_table, we_ifc, we_rpc):
    """-> ([pifc_l], [prpc_l]): bf16, each bit-equal to ``linear16(table,
    we_l)``; ``we_ifc`` / ``we_rpc`` are the per-layer [H,H] weights."""
    if len(we_ifc) != len(we_rpc):
        raise ValueError(f"{len(we_ifc)} we_ifc vs {len(we_rpc)} we_rpc")
    layers = len(we_ifc)
    params = (ifc_table, rpc_table, *we_ifc, *we_rpc)
    sinks = tuple(grad_sink(p) for p in params)
    out = _PTablesFn.apply(sinks, _sink_anchor(ifc_table.device),
                           *(_sunk(p, s) for p, s in zip(params, sinks)))
    return list(out[:layers]), list(out[layers:])


def ptable_group_enabled() -> bool:
    """Grouped P-table GEMMs (PERTGNN_NO_PTABLE_GROUP=1 keeps the per-layer
    launches; read per call so one process can run both for comparison)."""
    import os
    return os.environ.get("PERTGNN_NO_PTABLE_GROUP", "0") != "1"


def ptable_dgrad_splits() -> int:
    """Blocks sharing one output tile's layer sum in the grouped table dgrad
    (PERTGNN_PTABLE_DGRAD_SPLIT, default 4: 98 -> 55 us for the whole
    backward at 8 layers, profiles/16; >1 adds atomically into the memset
    buffer and is ignored under PERTGNN_DETERMINISTIC=1; never more than the
    layer count)."""
    import os
    return int(os.environ.get("PERTGNN_PTABLE_DGRAD_SPLIT", "4"))


_ACT16 = None
_P16 = None


def p16_enabled() -> bool:
    """bf16 P tables in act16 mode (PERTGNN_NO_P16=1 keeps them fp32)."""
    global _P16
    if _P16 is None:
        import os
        _P16 = os.environ.get("PERTGNN_NO_P16", "0") != "1"
    return _P16


def act16_enabled() -> bool:
    """bf16-resident qkvs activations (bf16/fp16 precision modes, H%256==0).
    Disable with PERTGNN_NO_ACT16=1."""
    global _ACT16
    if _ACT16 is None:
        import os
        _ACT16 = os.environ.get("PERTGNN_NO_ACT16", "0") != "1"
    return _ACT16


# ---------------------------------------------------------------------------
# fused-layout edge attention: qkvs [N,4H] + per-vocab P tables (fast path)
# ---------------------------------------------------------------------------

class _EdgeAttentionFusedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkvs, pifc, prpc, edge_attr, row_ptr, csr_src, col_ptr,
                csc_dst, csc_eid, out16=False, heads=1):
        m = ext()
        out, alpha = m.edge_attn_fused_fwd(qkvs, pifc, prpc, edge_attr, row_ptr, csr_src, out16, heads)
        ctx.save_for_backward(qkvs, pifc, prpc, edge_attr, alpha,
                              row_ptr, csr_src, col_ptr, csc_dst, csc_eid)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, g):
        (qkvs, pifc, prpc, edge_attr, alpha, row_ptr, csr_src, col_ptr,
         csc_dst, csc_eid) = ctx.saved_tensors
        m = ext()
        dqkvs, de = m.edge_attn_fused_bwd(
            g.contiguous(), qkvs, pifc, prpc, edge_attr, alpha,
            row_ptr, csr_src, col_ptr, csc_dst, csc_eid, ctx.heads,
        )
        dpifc, dprpc = _attn_table_grads(m, de, pifc, prpc, edge_attr)
        return dqkvs, dpifc, dprpc, None, None, None, None, None, None, None, None


def _attn_table_grads(m, de, pifc, prpc, edge_attr):
    """dP_ifc, dP_rpc of a fused attention backward from its de."""
    # dP tables (per-vocab segment sums of de) are independent of the
    # CSC dk/dv pass queued above — overlap them on the side stream.
    if not _overlap_enabled():
        h = de.shape[1]
        if (h % 256 == 0 and not deterministic()
                and (pifc.shape[0] + prpc.shape[0]) * h * 4 <= 160 * 1024):
            dpifc, dprpc = m.vocab_scatter_dual(de, edge_attr, pifc.shape[0], prpc.shape[0])
            if dpifc.dtype != pifc.dtype:  # bf16 P tables: match grad dtype
                dpifc = dpifc.to(pifc.dtype)
                dprpc = dprpc.to(prpc.dtype)
        else:
            dpifc, dprpc = _edge_table_grads(m, de, pifc, prpc, edge_attr)
        return dpifc, dprpc
    cur = torch.cuda.current_stream()
    side = _side_stream()
    ev = torch.cuda.Event()
    ev.record(cur)
    side.wait_event(ev)
    with torch.cuda.stream(side):
        dpifc, dprpc = _edge_table_grads(m, de, pifc, prpc, edge_attr)
    ev2 = torch.cuda.Event()
    ev2.record(side)
    cur.wait_event(ev2)
    _mark_cross_stream(dpifc, cur)
    _mark_cross_stream(dprpc, cur)
    return dpifc, dprpc


def _fused_eager(qkvs, pifc, prpc, edge_attr, csr, heads):
    """Differentiable fp32 composition of the fused op from the oracle."""
    row_ptr, csr_src = csr[0], csr[1]
    n = qkvs.shape[0]
    h = qkvs.shape[1] // 4
    q, k, v, skip = qkvs.float().split(h, dim=1)
    e = (pifc.float().index_select(0, edge_attr[:, 0])
         + prpc.float().index_select(0, edge_attr[:, 1]))
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(
        torch.arange(n, dtype=torch.long, device=qkvs.device), deg)
    edge_index = torch.stack([csr_src.long(), dst])
    return ref.edge_attention(q, k, v, e, edge_index, n, skip, heads=heads)


def edge_attention_fused(qkvs, pifc, prpc, edge_attr, csr, out16=False,
                         heads=1):
    """Fast path: out_i = skip_i + softmax-weighted aggregate where
    q/k/v/skip are the four H-segments of ``qkvs`` and the edge embedding is
    P_ifc[a0] + P_rpc[a1] (exact refactoring of lin_edge(concat(ifc, rpc))).
    ``out16`` writes the aggregate bf16 (non-final layers feed BN, whose
    act16 path consumes/produces bf16 streams).  ``heads`` > 1 splits H into
    that many heads of C = H/heads channels (concat), each with its own
    softmax and a 1/sqrt(C) scale; the kernels raise the shape error for a
    (H, heads) pair their lane mapping cannot express.  CPU tensors and
    PERTGNN_FORCE_EAGER=1 take the fp32 oracle in ``reference``."""
    if not use_hip(qkvs):
        out = _fused_eager(qkvs, pifc, prpc, edge_attr, csr, heads)
        return out.to(torch.bfloat16) if out16 else out
    row_ptr, csr_src, col_ptr, csc_dst, csc_eid = csr
    return _EdgeAttentionFusedFn.apply(
        qkvs, pifc, prpc, edge_attr, row_ptr, csr_src, col_ptr, csc_dst,
        csc_eid, out16, heads
    )


def edge_attention_fused_infer(qkvs, pifc, prpc, edge_attr, csr,
                               bn_scale=None, bn_shift=None, relu=False,
                               out16=False, heads=1):
    """Forward-only ``edge_attention_fused`` for inference (K-inference):
    saves nothing for a backward, and applies the eval-mode BatchNorm — folded
    to the per-channel affine ``bn_scale``/``bn_shift`` (fp32 [H], see
    ``pertgnn.infer.fold_bn``) — and the optional ReLU in the kernel's
    epilogue, so a non-final layer is one kernel instead of attention plus
    a BN-apply pass.  NOT differentiable: raises when grad mode is on and an
    input requires grad.  CPU tensors and PERTGNN_FORCE_EAGER=1 take the
    fp32 oracle in ``reference``.  ``heads`` as in ``edge_attention_fused``."""
    if (bn_scale is None) != (bn_shift is None):
        raise ValueError("bn_scale and bn_shift must be given together")
    if torch.is_grad_enabled() and any(
            t is not None and t.requires_grad
            for t in (qkvs, pifc, prpc, bn_scale, bn_shift)):
        raise RuntimeError(
            "edge_attention_fused_infer is forward-only (no backward); call "
            "it under torch.no_grad() or use edge_attention_fused")
    if not use_hip(qkvs):
        return ref.edge_attention_fused_infer(
            qkvs, pifc, prpc, edge_attr, csr, bn_scale, bn_shift, relu, out16,
            heads)
    if bn_scale is None:
        bn_scale = bn_shift = torch.empty(0, dtype=torch.float32,
                                          device=qkvs.device)
    return ext().edge_attn_fused_infer(qkvs, pifc, prpc, edge_attr, csr[0],
                                       csr[1], bn_scale, bn_shift, bool(relu),
                                       bool(out16), int(heads))


# ---------------------------------------------------------------------------
# pattern pool (K9+K10)
# ---------------------------------------------------------------------------

def _pool_forward(m, x, probs, nnodes, batch, num_graphs):
    """The pattern pool's forward launches (shared by its two autograd
    nodes)."""
    # nodes are contiguous per graph (collation order) -> batch_ptr.
    # scatter_add instead of bincount: bincount syncs on the device max,
    # which would break hipGraph capture of the training step.
    counts = torch.zeros(num_graphs, dtype=torch.long, device=x.device)
    counts.scatter_add_(0, batch, torch.ones_like(batch))
    batch_ptr = torch.zeros(num_graphs + 1, dtype=torch.int32, device=x.device)
    batch_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return m.seg_pool_fwd(x, probs.contiguous(), nnodes.contiguous(), batch_ptr, num_graphs)


class _PatternPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, probs, nnodes, batch, num_graphs):
        out = _pool_forward(ext(), x, probs, nnodes, batch, num_graphs)
        ctx.save_for_backward(probs, nnodes, batch)
        return out

    @staticmethod
    def backward(ctx, g):
        probs, nnodes, batch = ctx.saved_tensors
        m = ext()
        dx = m.seg_pool_bwd(g.contiguous(), probs, nnodes, batch)
        return dx, None, None, None, None


def pattern_pool(x, pattern_probs, pattern_num_nodes, batch, num_graphs):
    if use_hip(x):
        return _PatternPoolFn.apply(x, pattern_probs, pattern_num_nodes, batch, num_graphs)
    return ref.pattern_pool(x, pattern_probs, pattern_num_nodes, batch, num_graphs)


# ---------------------------------------------------------------------------
# embedding gathers (K1 + K11)
# ---------------------------------------------------------------------------

class _EmbedNodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_raw, cat_idx, table, out16=False, pad_to=0):
        m = ext()
        out = m.embed_node_fwd(x_raw, cat_idx, table, out16, pad_to)
        ctx.save_for_backward(cat_idx)
        ctx.f = x_raw.shape[1]
        ctx.h = table.shape[1]
        ctx.rows = table.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        (cat_idx,) = ctx.saved_tensors
        m = ext()
        # g is [n, f + h] or the padded [n, pad_to]: the table gradient reads
        # its h columns in place (row stride g.shape[1], offset f)
        g = g.contiguous()
        dx_raw = None
        if ctx.needs_input_grad[0]:
            dx_raw = g[:, : ctx.f].contiguous()
            if dx_raw.dtype != torch.float32:
                dx_raw = dx_raw.float()
        dtable = None
        if ctx.needs_input_grad[2]:
            dtable = _table_grad(m, g, cat_idx, ctx.rows, ctx.h, ctx.f)
        return dx_raw, None, dtable, None, None


class _EmbedEdgeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, edge_attr, ifc_table, rpc_table):
        m = ext()
        out = m.embed_edge_fwd(edge_attr, ifc_table, rpc_table)
        ctx.save_for_backward(edge_attr)
        ctx.rows = (ifc_table.shape[0], rpc_table.shape[0])
        return out

    @staticmethod
    def backward(ctx, g):
        (edge_attr,) = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        h = g.shape[1] // 2
        d_ifc = _table_grad(m, g, edge_attr[:, 0], ctx.rows[0], h, 0)
        d_rpc = _table_grad(m, g, edge_attr[:, 1], ctx.rows[1], h, h)
        return None, d_ifc, d_rpc


def embed_concat_node(x_raw, cat_X, tables, out16=False, pad_to=None):
    """``out16`` emits the concat bf16 so layer 1's QKVS GEMM takes the
    bf16-A path — numerically identical to the fp32 tensor (the GEMM staging
    rounds operands to bf16 either way).  ``pad_to`` (None = no padding)
    widens the rows to that many columns, +0 past the concat: the first
    conv's ``k_padded``, so that its GEMM operand is written once, already
    padded, and the gradient that comes back is read in place."""
    if len(tables) == 1 and use_hip(x_raw):
        cat_idx = cat_X[:, 0]
        out = _EmbedNodeFn.apply(x_raw, cat_idx.contiguous(), tables[0],
                                 out16, 0 if pad_to is None else int(pad_to))
        # what produced it, for the first conv (linear16_embed); the index
        # VIEW is recorded: it is what stays the same from step to step
        out._embed_src = EmbedSource(cat_idx, tables[0], x_raw.shape[1],
                                     tables[0].shape[1], x_raw.requires_grad)
        return out
    out = ref.embed_concat_node(x_raw, cat_X, tables)
    if pad_to is not None:
        if pad_to < out.shape[1]:
            raise ValueError(f"pad_to={pad_to} is below the concat width "
                             f"{out.shape[1]}")
        out = torch.nn.functional.pad(out, (0, pad_to - out.shape[1]))
    return out


def embed_concat_edge(edge_attr, interface_table, rpctype_table):
    if use_hip(interface_table):
        return _EmbedEdgeFn.apply(edge_attr, interface_table, rpctype_table)
    return ref.embed_concat_edge(edge_attr, interface_table, rpctype_table)


# ---------------------------------------------------------------------------
# row-gather embedding (entry_embeds, K1)
# ---------------------------------------------------------------------------

class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, table):
        m = ext()
        out = m.gather_rows(idx, table)
        ctx.save_for_backward(idx)
        ctx.rows = table.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        return None, _table_grad(m, g, idx, ctx.rows, g.shape[1], 0)


def embedding(idx, table):
    """out[i] = table[idx[i]] — row gather with scatter-add backward."""
    if use_hip(table):
        return _EmbeddingFn.apply(idx.contiguous(), table)
    return table.index_select(0, idx)


# ---------------------------------------------------------------------------
# batchnorm + relu (K7+K8)
# ---------------------------------------------------------------------------

_RNG_COUNTER = {}


def _rng_counter(device):
    """Device-resident dropout step counter: the fused-dropout kernels read
    it and a 1-thread kernel bumps it after each use, so captured hipGraphs
    draw FRESH masks on every replay.  Seeded from torch's global RNG (so
    torch.manual_seed reproduces mask sequences)."""
    key = str(device)
    t = _RNG_COUNTER.get(key)
    if t is None:
        t = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device)
        _RNG_COUNTER[key] = t
    return t


def _bn_forward(m, x, gamma, beta, running_mean, running_var, momentum, eps,
                training, fuse_relu, comm, dropout_p):
    """BN(+ReLU+dropout) forward ops, local or sync.  Returns (y, save_mean,
    save_invstd, mask or None, sync, keep_inv)."""
    sync = comm is not None and getattr(comm, "distributed", False) and training
    drop = float(dropout_p) if training else 0.0
    if drop > 0.0:
        assert fuse_relu, "fused dropout rides the ReLU mask (model.py:102-103)"
    seed = _rng_counter(x.device) if drop > 0.0 else torch.empty(
        0, dtype=torch.int64, device=x.device)
    if sync:
        # sync-BN (SURVEY.md §7 hard part 4, exact-parity mode): ONE
        # all-reduce carries the partial sums AND the row count (tail
        # slot of the [2h+1] partials) — no host round-trip per layer,
        # so the whole step stays launch-async (and hipGraph-capturable
        # where the backend supports captured collectives).
        partials = m.bn_stats(x)
        comm.all_reduce_(partials)
        fin = (m.bn_finalize_apply16 if x.dtype == torch.bfloat16
               else m.bn_finalize_apply)
        out = fin(
            x, partials, gamma, beta, running_mean, running_var,
            momentum, eps, training, fuse_relu, drop, seed)
    else:
        fwd = (m.bn_relu_fwd16 if x.dtype == torch.bfloat16
               else m.bn_relu_fwd)
        out = fwd(
            x, gamma, beta, running_mean, running_var, momentum, eps,
            training, fuse_relu, drop, seed
        )
    y, save_mean, save_invstd = out[:3]
    # the bf16 training forward with ReLU also returns a bit-packed keep
    # mask [n, h/8] (uint8); the backward reads that instead of y, and
    # the next layer's linear still holds y for its own wgrad
    mask = out[3] if len(out) > 3 and out[3].numel() > 0 else None
    # post-dropout y==0 <=> dropped-or-relu-negative, so the backward
    # only needs the keep scale on the existing y<=0 mask (no RNG)
    keep_inv = 1.0 / (1.0 - drop) if drop > 0.0 else 1.0
    return y, save_mean, save_invstd, mask, sync, keep_inv


class _BNReLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps,
                training, fuse_relu, comm, out16=False, dropout_p=0.0,
                sinks=(None, None), anchor=None):
        y, save_mean, save_invstd, mask, sync, keep_inv = _bn_forward(
            ext(), x, gamma, beta, running_mean, running_var, momentum, eps,
            training, fuse_relu, comm, dropout_p)
        ctx.sinks = sinks  # gradient sinks of gamma and beta, both or neither
        ctx.save_for_backward(x, gamma, save_mean, save_invstd,
                              y if mask is None else mask)
        ctx.y16 = y.dtype == torch.bfloat16
        ctx.fuse_relu = fuse_relu
        ctx.comm = comm if sync else None
        ctx.keep_inv = keep_inv
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, save_mean, save_invstd, y = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        y16 = ctx.y16  # y may be the uint8 keep mask (act16 path only)
        if ctx.comm is not None:
            bwd_partials = m.bn_bwd_partials16 if y16 else m.bn_bwd_partials
            bwd_apply = m.bn_bwd_apply16 if y16 else m.bn_bwd_apply
            # [2h+1] partials: sums + local count; one all-reduce gives the
            # global sums and count together (device-side, no .item()).
            partials_local = bwd_partials(g, x, y, save_mean, save_invstd,
                                          ctx.fuse_relu, ctx.keep_inv)
            partials_global = partials_local.clone()
            ctx.comm.all_reduce_(partials_global)
            dx, dgamma, dbeta = bwd_apply(
                g, x, y, save_mean, save_invstd, gamma,
                partials_global, partials_local, ctx.fuse_relu, ctx.keep_inv,
                *ctx.sinks)
        else:
            bwd = m.bn_relu_bwd16 if y16 else m.bn_relu_bwd
            dx, dgamma, dbeta = bwd(
                g, x, gamma, save_mean, save_invstd, y, ctx.fuse_relu,
                ctx.keep_inv, *ctx.sinks
            )
        if ctx.sinks[0] is not None:  # dgamma and dbeta are in the sinks
            dgamma = dbeta = None
        return (dx, dgamma, dbeta) + (None,) * 11


def _bn_sinks(gamma, beta):
    """(dgamma sink, dbeta sink) as the BN backward ops take them: both or
    (None, None)."""
    sinks = (grad_sink(gamma), grad_sink(beta))
    return sinks if None not in sinks else (None, None)


def bn_attn_fuse_enabled(h: int) -> bool:
    """The attention backward applies the BN backward of the BN that follows
    it (act16 training, h in {256, 512}: the widths both the keep mask and
    the bf16 attention kernels cover).  PERTGNN_NO_BN_ATTN_FUSE=1 keeps the
    two separate Functions; read per call so one process can run both."""
    import os
    return (h in (256, 512)
            and os.environ.get("PERTGNN_NO_BN_ATTN_FUSE", "0") != "1")


class _AttnBNReLUFn(torch.autograd.Function):
    """Fused attention forward -> BN+ReLU(+dropout) training forward, act16.
    The forward is the two existing ops; the backward hands the BN output
    gradient to the attention backward, whose row kernel applies the BN
    backward to each row it loads — the [N, H] dx between the two is never
    written."""

    @staticmethod
    def forward(ctx, qkvs, pifc, prpc, gamma, beta, edge_attr, row_ptr,
                csr_src, col_ptr, csc_dst, csc_eid, heads, running_mean,
                running_var, momentum, eps, comm, dropout_p,
                sinks=(None, None), anchor=None):
        m = ext()
        ctx.sinks = sinks  # gradient sinks of gamma and beta, both or neither
        x, alpha = m.edge_attn_fused_fwd(qkvs, pifc, prpc, edge_attr, row_ptr,
                                         csr_src, True, heads)
        y, save_mean, save_invstd, mask, sync, keep_inv = _bn_forward(
            m, x, gamma, beta, running_mean, running_var, momentum, eps,
            True, True, comm, dropout_p)
        if mask is None:
            raise RuntimeError(
                "fused attention+BN needs the BN keep mask (n > 0, H in "
                f"{{256, 512}}); got x {tuple(x.shape)}")
        ctx.save_for_backward(qkvs, pifc, prpc, gamma, edge_attr, alpha,
                              row_ptr, csr_src, col_ptr, csc_dst, csc_eid,
                              x, save_mean, save_invstd, mask)
        ctx.heads = heads
        ctx.comm = comm if sync else None
        ctx.keep_inv = keep_inv
        return y

    @staticmethod
    def backward(ctx, g):
        (qkvs, pifc, prpc, gamma, edge_attr, alpha, row_ptr, csr_src, col_ptr,
         csc_dst, csc_eid, x, save_mean, save_invstd, mask) = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        partials = (None, None)
        if ctx.comm is not None:
            # as _BNReLUFn.backward: local [2h+1] partials, one all-reduce
            # for the global sums and count
            partials_local = m.bn_bwd_partials16(
                g, x, mask, save_mean, save_invstd, True, ctx.keep_inv)
            partials_global = partials_local.clone()
            ctx.comm.all_reduce_(partials_global)
            partials = (partials_global, partials_local)
        dqkvs, de, dgamma, dbeta = m.edge_attn_bn_bwd16(
            g, x, mask, gamma, save_mean, save_invstd, ctx.keep_inv, qkvs,
            pifc, prpc, edge_attr, alpha, row_ptr, csr_src, col_ptr, csc_dst,
            csc_eid, ctx.heads, *partials, *ctx.sinks)
        dpifc, dprpc = _attn_table_grads(m, de, pifc, prpc, edge_attr)
        if ctx.sinks[0] is not None:  # dgamma and dbeta are in the sinks
            dgamma = dbeta = None
        return (dqkvs, dpifc, dprpc, dgamma, dbeta) + (None,) * 15


def edge_attention_fused_bn_relu(qkvs, pifc, prpc, edge_attr, csr, gamma,
                                 beta, running_mean, running_var, momentum,
                                 eps, heads=1, comm=None, dropout_p=0.0):
    """``batchnorm_relu(edge_attention_fused(..., out16=True), training=True,
    fuse_relu=True, out16=True)`` as one autograd node (bf16 ``qkvs`` on the
    GPU, ``bn_attn_fuse_enabled(h)``): same forward ops, same results, one
    pass over [N, H] less in the backward."""
    row_ptr, csr_src, col_ptr, csc_dst, csc_eid = csr
    sinks = _bn_sinks(gamma, beta)
    return _AttnBNReLUFn.apply(
        qkvs, pifc, prpc, _sunk(gamma, sinks[0]), _sunk(beta, sinks[1]),
        edge_attr, row_ptr, csr_src, col_ptr, csc_dst, csc_eid, heads,
        running_mean, running_var, momentum, eps, comm, dropout_p, sinks,
        _sink_anchor(qkvs.device))


def pool_attn_fuse_enabled(h: int) -> bool:
    """The last conv's attention backward forms the pattern pool's gradient
    itself (bf16 ``qkvs`` on the GPU, h in {256, 512}: the widths of the
    act16 attention kernels that carry the mode).
    PERTGNN_NO_POOL_ATTN_FUSE=1 keeps the two separate Functions; read per
    call so one process can run both."""
    import os
    return (h in (256, 512)
            and os.environ.get("PERTGNN_NO_POOL_ATTN_FUSE", "0") != "1")


class _AttnPoolFn(torch.autograd.Function):
    """Fused attention forward (fp32 out) -> pattern pool forward, returning
    both.  The forward is the two existing ops.  When only the pooled output
    carries a gradient (the training loss reads ``global_predict`` alone) the
    attention backward forms each node's gradient ``gmean[batch[i]] *
    probs[i] / nnodes[i]`` itself — the fp32 [N, H] tensor that
    ``seg_pool_bwd`` writes and both attention kernels read back never
    exists.  A gradient on ``x`` takes the two existing backward ops."""

    @staticmethod
    def forward(ctx, qkvs, pifc, prpc, edge_attr, row_ptr, csr_src, col_ptr,
                csc_dst, csc_eid, heads, probs, nnodes, batch, num_graphs):
        m = ext()
        ctx.set_materialize_grads(False)
        x, alpha = m.edge_attn_fused_fwd(qkvs, pifc, prpc, edge_attr, row_ptr,
                                         csr_src, False, heads)
        probs = probs.contiguous()
        nnodes = nnodes.contiguous()
        mean_x = _pool_forward(m, x, probs, nnodes, batch, num_graphs)
        ctx.save_for_backward(qkvs, pifc, prpc, edge_attr, alpha, row_ptr,
                              csr_src, col_ptr, csc_dst, csc_eid, probs,
                              nnodes, batch)
        ctx.heads = heads
        return x, mean_x

    @staticmethod
    def backward(ctx, gx, gmean):
        (qkvs, pifc, prpc, edge_attr, alpha, row_ptr, csr_src, col_ptr,
         csc_dst, csc_eid, probs, nnodes, batch) = ctx.saved_tensors
        none = (None,) * 11
        if gx is None and gmean is None:
            return (None, None, None) + none
        m = ext()
        attn = (qkvs, pifc, prpc, edge_attr, alpha, row_ptr, csr_src,
                col_ptr, csc_dst, csc_eid, ctx.heads)
        if gx is None:
            dqkvs, de = m.edge_attn_pool_bwd16(gmean.contiguous(), probs,
                                               nnodes, batch, *attn)
        else:
            g = gx.contiguous()
            if gmean is not None:
                g = m.seg_pool_bwd(gmean.contiguous(), probs, nnodes,
                                   batch) + g
            dqkvs, de = m.edge_attn_fused_bwd(g, *attn)
        dpifc, dprpc = _attn_table_grads(m, de, pifc, prpc, edge_attr)
        return (dqkvs, dpifc, dprpc) + none


def edge_attention_fused_pool(qkvs, pifc, prpc, edge_attr, csr, probs,
                              nnodes, batch, num_graphs, heads=1):
    """``x = edge_attention_fused(...)`` (fp32 out) and ``pattern_pool(x,
    ...)`` -> ``(x, mean_x)``: one autograd node where
    ``pool_attn_fuse_enabled`` holds for bf16 ``qkvs`` on the GPU, the two
    separate ops everywhere else.  Same forward ops, same results."""
    h = qkvs.shape[1] // 4
    if (use_hip(qkvs) and qkvs.dtype == torch.bfloat16
            and pool_attn_fuse_enabled(h)):
        row_ptr, csr_src, col_ptr, csc_dst, csc_eid = csr
        return _AttnPoolFn.apply(qkvs, pifc, prpc, edge_attr, row_ptr,
                                 csr_src, col_ptr, csc_dst, csc_eid, heads,
                                 probs, nnodes, batch, num_graphs)
    x = edge_attention_fused(qkvs, pifc, prpc, edge_attr, csr, heads=heads)
    return x, pattern_pool(x, probs, nnodes, batch, num_graphs)


class _EagerSyncBNFn(torch.autograd.Function):
    """Eager sync-BN with the explicit cross-rank backward: the gradient of
    x_i includes every rank's loss through the SHARED mean/var, so the
    backward all-reduces the per-channel sums of gm and gm*xhat and divides
    by the GLOBAL count (torch.nn.SyncBatchNorm semantics)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps,
                fuse_relu, comm):
        with torch.no_grad():
            n_local = x.shape[0]
            h = x.shape[1]
            pack = torch.cat([x.sum(0), (x * x).sum(0),
                              torch.tensor([float(n_local)], dtype=x.dtype, device=x.device)])
            comm.all_reduce_(pack)
            count = float(pack[-1])
            mean = pack[:h] / count
            var = (pack[h:2 * h] / count - mean * mean).clamp_min(0)
            invstd = (var + eps).rsqrt()
            unbiased = var * (count / max(count - 1.0, 1.0))
            running_mean.mul_(1 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1 - momentum).add_(unbiased, alpha=momentum)
            y = (x - mean) * invstd * gamma + beta
            if fuse_relu:
                y = torch.nn.functional.relu(y)
        ctx.save_for_backward(x, gamma, mean, invstd, y)
        ctx.fuse_relu = fuse_relu
        ctx.comm = comm
        ctx.count = count
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma, mean, invstd, y = ctx.saved_tensors
        gm = g.clone()
        if ctx.fuse_relu:
            gm[y <= 0] = 0
        xhat = (x - mean) * invstd
        s1_local = gm.sum(0)
        s2_local = (gm * xhat).sum(0)
        pack = torch.cat([s1_local, s2_local])
        ctx.comm.all_reduce_(pack)
        h = x.shape[1]
        s1_g = pack[:h] / ctx.count
        s2_g = pack[h:] / ctx.count
        dx = gamma * invstd * (gm - s1_g - xhat * s2_g)
        return dx, s2_local, s1_local, None, None, None, None, None, None


def _eager_sync_batchnorm(x, gamma, beta, running_mean, running_var, momentum,
                          eps, fuse_relu, comm):
    return _EagerSyncBNFn.apply(x, gamma, beta, running_mean, running_var,
                                momentum, eps, fuse_relu, comm)


def batchnorm_relu(x, gamma, beta, running_mean, running_var, momentum, eps,
                   training, fuse_relu=True, comm=None, out16=False,
                   dropout_p=0.0):
    """BatchNorm1d over N per channel, optional fused ReLU (model.py:101-102)
    and fused dropout (reference K8: the model applies dropout right after
    BN+ReLU, model.py:103; the HIP path folds mask+scale into the BN
    epilogue, the CPU path applies torch dropout after).  With ``comm``
    (distributed) and training=True, runs sync-BN: statistics over the
    GLOBAL batch (exact single-process parity).  ``out16`` emits the
    normalized activations as bf16 (act16 mode): statistics/affine math
    stays fp32, only the activation stream narrows — the downstream QKVS
    GEMM and its wgrad then read half the bytes."""
    if use_hip(x):
        sinks = _bn_sinks(gamma, beta)
        return _BNReLUFn.apply(x, _sunk(gamma, sinks[0]),
                               _sunk(beta, sinks[1]), running_mean,
                               running_var, momentum, eps, training,
                               fuse_relu, comm, out16, dropout_p, sinks,
                               _sink_anchor(x.device))
    if comm is not None and getattr(comm, "distributed", False) and training:
        y = _eager_sync_batchnorm(x, gamma, beta, running_mean, running_var,
                                  momentum, eps, fuse_relu, comm)
    else:
        y = torch.nn.functional.batch_norm(
            x, running_mean, running_var, gamma, beta, training, momentum, eps
        )
        if fuse_relu:
            y = torch.nn.functional.relu(y)
    if dropout_p > 0.0:
        y = torch.nn.functional.dropout(y, p=dropout_p, training=training)
    return y


# ---------------------------------------------------------------------------
# loss + metrics (K12/K13)
# ---------------------------------------------------------------------------

class _QuantileLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, y_hat, tau):
        m = ext()
        loss = m.quantile_loss_fwd(y, y_hat, tau)
        ctx.save_for_backward(y, y_hat)
        ctx.tau = tau
        return loss

    @staticmethod
    def backward(ctx, g):
        y, y_hat = ctx.saved_tensors
        m = ext()
        dy_hat = m.quantile_loss_bwd(g, y, y_hat, ctx.tau)
        return None, dy_hat, None


def _is_level(tau) -> bool:
    """True for one scalar level (a number or a 0-d tensor), False for a
    sequence of levels."""
    if torch.is_tensor(tau):
        return tau.dim() == 0
    return not hasattr(tau, "__len__") and not hasattr(tau, "__iter__")


def quantile_loss_parts(y, y_hat, taus):
    """``(loss, per_level_sums)`` for ``y [B]``, ``y_hat [B, Q]`` and Q
    levels: the pinball loss summed over levels and averaged over rows, and
    the undivided pinball sum of every level ``[Q]`` (no gradient)."""
    levels = ref.check_taus(taus)
    ref._check_multi(y, y_hat, levels)
    if use_hip(y_hat):
        # STOPGAP until single-pass multi-level kernels exist: one launch of
        # the scalar HIP loss per level, each on its own contiguous column.
        # Every level sees the gradient scale g/B it would have alone, and
        # one level is the scalar op bit for bit.
        cols = [y_hat[:, q].contiguous() for q in range(len(levels))]
        losses = [_QuantileLossFn.apply(y, c, t) for c, t in zip(cols, levels)]
        if len(losses) == 1:
            loss = losses[0]
        else:
            # the levels are added in fp64 and rounded to fp32 once, so the
            # sum costs one rounding, not Q - 1
            loss = torch.stack(losses).double().sum().float()
        if y.shape[0] == 0:
            return loss, y_hat.new_zeros(len(levels))
        # the undivided per-level sums come from the scalar metric kernel
        # (loss_q * B would round twice more at a B that is no power of two)
        with torch.no_grad():
            sums = torch.stack([ext().eval_metrics(y, c.detach(), t)[2]
                                for c, t in zip(cols, levels)])
        return loss, sums
    loss, sums = ref.quantile_loss_multi(y, y_hat, levels)
    return loss, sums.detach()


def quantile_loss(y, y_hat, tau):
    """Pinball loss.  A scalar ``tau`` takes ``[B]`` predictions; a sequence
    of Q levels takes ``[B, Q]`` predictions and sums the levels."""
    if not _is_level(tau):
        return quantile_loss_parts(y, y_hat, tau)[0]
    if y_hat.dim() != y.dim():
        raise ValueError(
            f"a scalar tau takes predictions shaped like y {tuple(y.shape)}, "
            f"got {tuple(y_hat.shape)}; pass the levels as a sequence for "
            "[B, Q] predictions")
    if use_hip(y_hat):
        return _QuantileLossFn.apply(y, y_hat, tau)
    return ref.quantile_loss(y, y_hat, tau)


def eval_metrics(y, y_hat, tau):
    """Scalar ``tau``: the (mae, mape, pinball) sums.  A sequence of Q
    levels with ``[B, Q]`` predictions: the ``[3 + 2Q]`` vector ``[mae,
    mape, crossing rows, pinball[Q], covered rows[Q]]`` with MAE/MAPE of the
    point level.  The counts are fp32 sums of ones: exact below 2^24 rows
    per call."""
    if not _is_level(tau):
        levels = ref.check_taus(tau)
        ref._check_multi(y, y_hat, levels)
        point = ref.point_level(levels)
        if use_hip(y_hat):
            # STOPGAP until a single-pass kernel exists: the scalar HIP
            # metric reduction once per level; the two counts are
            # comparisons summed by torch (evaluation only)
            cols = [ext().eval_metrics(y, y_hat[:, q].contiguous(), t)
                    for q, t in enumerate(levels)]
            cross = (y_hat[:, 1:] < y_hat[:, :-1]).any(dim=1).sum()
            cover = (y.unsqueeze(1) <= y_hat).sum(dim=0)
            return torch.cat([
                torch.stack([cols[point][0], cols[point][1],
                             cross.to(y_hat.dtype)]),
                torch.stack([c[2] for c in cols]),
                cover.to(y_hat.dtype)])
        return ref.eval_metrics_multi(y, y_hat, levels, point)
    if y_hat.dim() != y.dim():
        raise ValueError(
            f"a scalar tau takes predictions shaped like y {tuple(y.shape)}, "
            f"got {tuple(y_hat.shape)}")
    if use_hip(y_hat):
        return ext().eval_metrics(y, y_hat, tau)
    return ref.eval_metrics(y, y_hat, tau)


def quantile_rearrange(y_hat):
    """Rows of ``[B, Q]`` predictions sorted ascending (Q = 1: the input
    itself, nothing launched)."""
    if y_hat.dim() != 2:
        raise ValueError(f"expected y_hat [B, Q], got {tuple(y_hat.shape)}")
    if y_hat.shape[1] > ref.MAX_QUANTILES:
        raise ValueError(f"at most {ref.MAX_QUANTILES} levels are supported, "
                         f"got {y_hat.shape[1]}")
    if y_hat.shape[1] == 1:
        return y_hat
    if use_hip(y_hat):
        # STOPGAP until a HIP kernel exists: torch elementwise min/max over
        # the columns in odd-even transposition order (Q stages).  They
        # move values and compute none, and need no sort temporaries, so
        # the Predictor can capture them in its hipGraph
        cols = list(y_hat.unbind(dim=1))
        for stage in range(len(cols)):
            for j in range(stage & 1, len(cols) - 1, 2):
                lo = torch.minimum(cols[j], cols[j + 1])
                cols[j + 1] = torch.maximum(cols[j], cols[j + 1])
                cols[j] = lo
        return torch.stack(cols, dim=1)
    return ref.quantile_rearrange(y_hat)


# ---------------------------------------------------------------------------
# linear (K2) — MFMA GEMM on the HIP path
# ---------------------------------------------------------------------------

_GEMM_PRECISION = "fp32"
_SIDE_STREAM = None
_OVERLAP = None


def _overlap_enabled() -> bool:
    """Side-stream overlap of independent backward branches.  Measured A/B
    under hipGraph replay: the event-join edges cost more than the overlap
    buys (11.1 vs 10.55 ms/step), so this is OFF by default (opt in with
    PERTGNN_SIDE_STREAM=1 for eager multi-stream experiments)."""
    global _OVERLAP
    if _OVERLAP is None:
        import os
        _OVERLAP = os.environ.get("PERTGNN_SIDE_STREAM", "0") == "1"
    return _OVERLAP


def _side_stream():
    """Side stream for independent backward branches (wgrad overlaps dgrad);
    cross-stream edges are captured into hipGraphs as graph dependencies."""
    global _SIDE_STREAM
    if _SIDE_STREAM is None:
        _SIDE_STREAM = torch.cuda.Stream()
    return _SIDE_STREAM


def _mark_cross_stream(t, consumer_stream):
    """Tensors allocated on the side stream are consumed on the main stream:
    tell the caching allocator (no-op during graph capture, where the private
    pool owns the memory for the whole graph)."""
    if not torch.cuda.is_current_stream_capturing():
        t.record_stream(consumer_stream)


def set_gemm_precision(prec: str):
    """Select the matmul compute precision on the HIP path: "fp32" (exact,
    v_mfma_f32_16x16x4_f32), "bf16" or "fp16" (operands rounded to 16-bit in
    the matrix cores, fp32 accumulate — BASELINE configs 2/5 mixed-precision
    modes).  Everything outside the matmuls stays fp32 either way."""
    global _GEMM_PRECISION
    assert prec in ("fp32", "bf16", "fp16"), prec
    _GEMM_PRECISION = prec


def gemm_precision() -> str:
    return _GEMM_PRECISION


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        m = ext()
        prec = _GEMM_PRECISION
        bb = b if b is not None else torch.empty(0, dtype=x.dtype, device=x.device)
        if prec == "bf16":
            y = m.linear_fwd_bf16(x, w, bb)
        elif prec == "fp16":
            y = m.linear_fwd_fp16(x, w, bb)
        else:
            y = m.linear_fwd(x, w, bb)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        ctx.prec = prec
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        m = ext()
        g = g.contiguous()
        prec = {"fp32": 0, "bf16": 1, "fp16": 2}[ctx.prec]
        if not _overlap_enabled():
            dw, db = m.linear_wgrad(g, x, ctx.has_bias, prec)
            dx = m.linear_dgrad(g, w, prec)
            return dx, dw, (db if ctx.has_bias else None)
        cur = torch.cuda.current_stream()
        side = _side_stream()
        ev = torch.cuda.Event()
        ev.record(cur)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            dw, db = m.linear_wgrad(g, x, ctx.has_bias, prec)
        dx = m.linear_dgrad(g, w, prec)  # current stream, overlapped with wgrad
        ev2 = torch.cuda.Event()
        ev2.record(side)
        cur.wait_event(ev2)
        _mark_cross_stream(dw, cur)
        if ctx.has_bias:
            _mark_cross_stream(db, cur)
        return dx, dw, (db if ctx.has_bias else None)


def linear(x, w, b=None):
    """y = x @ w^T + b with torch.nn.Linear weight layout [out,in]."""
    if use_hip(x) and hasattr(ext(), "linear_fwd"):
        return _LinearFn.apply(x, w, b)
    return torch.nn.functional.linear(x, w, b)


__all__ = [
    "set_gemm_precision",
    "p16_enabled",
    "gemm_precision",
    "linear16",
    "ptables_grouped",
    "ptable_group_enabled",
    "act16_enabled",
    "edge_attention",
    "edge_attention_fused",
    "edge_attention_fused_infer",
    "edge_attention_fused_bn_relu",
    "bn_attn_fuse_enabled",
    "embedding",
    "pattern_pool",
    "embed_concat_node",
    "embed_concat_edge",
    "batchnorm_relu",
    "quantile_loss",
    "quantile_loss_parts",
    "quantile_rearrange",
    "eval_metrics",
    "linear",
]
