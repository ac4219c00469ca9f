"""The two ends of the training step.

Head: ``embed_node_fwd(..., pad_to)`` writes the layer-1 GEMM operand at its
padded width itself, and ``_EmbedNodeFn.backward`` reads the padded dgrad
output in place.  Tail: the last conv's attention backward forms the pattern
pool's gradient itself (``edge_attn_pool_bwd16`` / ``_AttnPoolFn``), so no
[N, H] gradient lies between the pool and the attention.

Everything is compared by bit pattern against the composition it replaces:
the unpadded op (plus ``torch.nn.functional.pad``), and ``seg_pool_bwd``
followed by ``edge_attn_fused_bwd``.  Neither attention backward kernel has
atomics and the pool gradient comes from one shared helper, so the unfused
path repeats itself bit for bit.  The table gradients of the embed autograd
test use operands whose sums are exact in every order (small integers), so
the LDS-atomic scatter is order-independent there.

Graphs as in tests/test_attn_bn_bwd.py: node 0 has no in-edges, node 1 no
out-edges, node 2 in-degree 70, node 3 out-degree 70; n = 11 and 67 are no
multiples of the rows per block; n = 1 carries 70 self-loops; E = 0 has no
edges at all.  With three graphs the middle graph has exactly one node.
"""
import functools

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

BF16 = torch.bfloat16
VI, VR = 37, 5
HUB = 70


def _ext():
    import pertgnn._C as C
    return C


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _assert_same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, \
        (what, got.dtype, want.dtype, got.shape, want.shape)
    ndiff = int((_bits(got) != _bits(want)).sum())
    assert ndiff == 0, (what, ndiff, got.numel())


# ---------------------------------------------------------------------------
# embed_node_fwd(pad_to)
# ---------------------------------------------------------------------------

ROWS_SMALL = 7


def _pad_values(f, h):
    w = f + h
    m8 = (w + 7) // 8 * 8
    if m8 == w:
        m8 += 8
    m4 = (w + 3) // 4 * 4
    if m4 % 8 == 0:
        m4 += 4
    odd = w + 4 if w % 2 else w + 5
    vals = [w, m8, m4, odd]
    if h == 256:
        vals.append(384)
    assert any(v % 8 == 0 for v in vals) and any(v % 2 for v in vals)
    assert any(v % 4 == 0 and v % 8 for v in vals)
    return vals


def _embed_inputs(n, f, h, rows=ROWS_SMALL):
    g = torch.Generator().manual_seed(7 * n + 100 * f + h)
    x_raw = torch.randn(n, f, generator=g)
    table = torch.randn(rows, h, generator=g)
    idx = torch.randint(0, rows, (n,), generator=g)
    if n >= 1:
        idx[-1] = rows - 1
    if n >= 2:
        idx[0] = 0
    return x_raw.to(DEV), idx.to(DEV), table.to(DEV)


@gpu
@needs_gpu
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("f,h", [(9, 256), (1, 32), (16, 8)])
def test_embed_padded_equals_unpadded(f, h, out16):
    C = _ext()
    w = f + h
    esize = 2 if out16 else 4
    for n in (0, 1, 63, 64, 65, 1000):
        x_raw, idx, table = _embed_inputs(n, f, h)
        want = C.embed_node_fwd(x_raw, idx, table, out16)
        assert want.shape == (n, w)
        for pad_to in _pad_values(f, h):
            # the allocator hands the output the block this NaN tensor held
            poison = torch.full((max(n * pad_to * esize, 1),), 0xFF,
                                dtype=torch.uint8, device=DEV)
            del poison
            got = C.embed_node_fwd(x_raw, idx, table, out16, pad_to)
            torch.cuda.synchronize()
            what = (f, h, out16, n, pad_to)
            assert got.shape == (n, pad_to) and got.is_contiguous(), what
            assert got.dtype == want.dtype, what
            _assert_same_bits(got[:, :w], want, what)
            pad = _bits(got[:, w:])
            assert int((pad != 0).sum()) == 0, (what, "pad columns not +0")


@gpu
@needs_gpu
def test_embed_pad_below_width_raises():
    C = _ext()
    x_raw, idx, table = _embed_inputs(5, 9, 256)
    for out16 in (False, True):
        with pytest.raises(RuntimeError, match="pad_to"):
            C.embed_node_fwd(x_raw, idx, table, out16, 264)
        with pytest.raises(RuntimeError, match="pad_to"):
            C.embed_node_fwd(x_raw, idx, table, out16, 8)
    torch.cuda.synchronize()
    # pad_to = 0 is today's op
    a = C.embed_node_fwd(x_raw, idx, table, True, 0)
    b = C.embed_node_fwd(x_raw, idx, table, True)
    _assert_same_bits(a, b, "pad_to=0")


def _draw(seed, shape, values):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(len(values), shape, generator=g)
    return torch.tensor(values, dtype=torch.float32)[idx].to(DEV)


@gpu
@needs_gpu
@pytest.mark.parametrize("x_grad", [False, True])
@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("rows", [4, 200], ids=["lds", "grouped"])
def test_embed_autograd_padded_vs_torch_pad(rows, out16, x_grad, monkeypatch):
    """embed_concat_node(pad_to=384) -> linear16 against embed_concat_node ->
    F.pad -> linear16 on the same leaves.  Operands in {-1, 0, 1} over 64
    outputs: every dgrad element is an integer of magnitude <= 64 (exact in
    bf16) and every table-gradient sum stays below 2^24, so all sums are
    exact in any order and both table-gradient kernels (LDS atomics at 4
    rows; the grouped scatter above 160 rows at h = 256) give order-free
    bits."""
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    n, f, h, k, nout = 1000, 9, 256, 384, 64
    assert (rows * h * 4 <= 160 * 1024) == (rows == 4)
    x_raw0 = _draw(1, (n, f), [-1.0, 0.0, 1.0, 0.5])
    table0 = _draw(2, (rows, h), [-1.0, 0.0, 1.0, 0.5])
    cat = torch.randint(0, rows, (n, 1),
                        generator=torch.Generator().manual_seed(3)).to(DEV)
    cat[0, 0], cat[-1, 0] = 0, rows - 1
    w = _draw(4, (nout, k), [-1.0, 0.0, 1.0])
    gy = _draw(5, (n, nout), [-1.0, 0.0, 1.0]).to(BF16)
    res = []
    for padded in (True, False):
        x_raw = x_raw0.clone().requires_grad_(x_grad)
        table = table0.clone().requires_grad_(True)
        if padded:
            x = F.embed_concat_node(x_raw, cat, [table], out16=out16,
                                    pad_to=k)
        else:
            x = F.embed_concat_node(x_raw, cat, [table], out16=out16)
            assert x.shape == (n, f + h)
            x = torch.nn.functional.pad(x, (0, k - x.shape[1]))
        assert x.shape == (n, k) and x.dtype == (BF16 if out16
                                                 else torch.float32)
        y = F.linear16(x, w)
        y.backward(gy)
        torch.cuda.synchronize()
        res.append((x.detach(), y.detach(), table.grad, x_raw.grad))
    (x_p, y_p, dt_p, dx_p), (x_t, y_t, dt_t, dx_t) = res
    _assert_same_bits(x_p, x_t, "x")
    _assert_same_bits(y_p, y_t, "y")
    _assert_same_bits(dt_p, dt_t, "dtable")
    # and against fp64: g = gy @ w, summed by table row over columns f..f+h
    g64 = gy.double() @ w.double()
    assert float(g64.abs().max()) <= 64
    want = torch.zeros(rows, h, dtype=torch.float64, device=DEV)
    want.index_add_(0, cat[:, 0], g64[:, f:f + h])
    assert float(want.abs().max()) < 2 ** 24 and float(want.abs().max()) > 0
    _assert_same_bits(dt_p, want.float(), "dtable vs fp64")
    if x_grad:
        _assert_same_bits(dx_p, dx_t, "dx_raw")
        _assert_same_bits(dx_p, g64[:, :f].float(), "dx_raw vs fp64")
    else:
        assert dx_p is None and dx_t is None


class _Ctx:
    """What _EmbedNodeFn.backward reads of its ctx."""

    def __init__(self, idx, f, h, rows, needs):
        self.saved_tensors = (idx,)
        self.f, self.h, self.rows = f, h, rows
        self.needs_input_grad = needs


@gpu
@needs_gpu
def test_embed_backward_skips_dx_raw_without_grad():
    n, f, h, rows, k = 65, 9, 256, 4, 384
    g = _draw(6, (n, k), [-1.0, 0.0, 1.0, 2.0]).to(BF16)
    idx = torch.randint(0, rows, (n,),
                        generator=torch.Generator().manual_seed(8)).to(DEV)
    off = F._EmbedNodeFn.backward(
        _Ctx(idx, f, h, rows, (False, False, True, False, False)), g)
    on = F._EmbedNodeFn.backward(
        _Ctx(idx, f, h, rows, (True, False, True, False, False)), g)
    torch.cuda.synchronize()
    assert len(off) == 5 and off[0] is None and off[1] is None
    assert on[0].dtype == torch.float32
    _assert_same_bits(on[0], g[:, :f].float(), "dx_raw")
    _assert_same_bits(off[2], on[2], "dtable")
    want = torch.zeros(rows, h, dtype=torch.float64, device=DEV)
    want.index_add_(0, idx, g[:, f:f + h].double())
    _assert_same_bits(off[2], want.float(), "dtable vs fp64")


# ---------------------------------------------------------------------------
# pool-fused attention backward, op level
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _graph(n, edges=True):
    """CSR/CSC arrays of ``build_csr`` and edge_attr [E, 4] in CSR order, on
    the GPU; built once per size and never written to."""
    from pertgnn.data.collate import build_csr

    g = torch.Generator().manual_seed(40 + n)
    src, dst = [], []
    if edges and n == 1:
        src, dst = [0] * HUB, [0] * HUB
    elif edges:
        assert n >= 8
        s = torch.randint(4, n, (HUB,), generator=g).tolist()
        src += s
        dst += [2] * HUB
        d = torch.randint(4, n, (HUB,), generator=g).tolist()
        src += [3] * HUB
        dst += d
        for i in range(4, n):
            deg = 1 + i % 3
            s = torch.randint(4, n, (deg,), generator=g).tolist()
            src += s
            dst += [i] * deg
        src += [5, 6]
        dst += [1, 1]
    ei = torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)
    _, row_ptr, csr_src, col_ptr, csc_dst, csc_eid = build_csr(ei, n)
    e = ei.shape[1]
    if edges and n > 1:
        indeg = (row_ptr[1:] - row_ptr[:-1]).tolist()
        outdeg = (col_ptr[1:] - col_ptr[:-1]).tolist()
        assert indeg[0] == 0 and outdeg[1] == 0
        assert indeg[2] == HUB and outdeg[3] == HUB
    ea = torch.stack([torch.randint(0, VI, (e,), generator=g),
                      torch.randint(0, VR, (e,), generator=g),
                      torch.ones(e, dtype=torch.long),
                      torch.zeros(e, dtype=torch.long)], dim=1)
    csr = tuple(t.to(DEV) for t in (row_ptr, csr_src, col_ptr, csc_dst,
                                    csc_eid))
    return csr, ea.to(DEV)


def _batch_of(n, graphs):
    """Nondecreasing graph ids; with three graphs the middle one has one node
    (at n = 1 it is the only populated graph)."""
    if graphs == 1:
        return torch.zeros(n, dtype=torch.long)
    if n == 1:
        return torch.ones(1, dtype=torch.long)
    k = n // 2
    b = torch.cat([torch.zeros(k, dtype=torch.long),
                   torch.ones(1, dtype=torch.long),
                   torch.full((n - k - 1,), 2, dtype=torch.long)])
    assert int((b == 1).sum()) == 1
    return b


@functools.lru_cache(maxsize=None)
def _pool_case(h, heads, n, graphs, p16, edges=True):
    """Operands of one backward from the real attention forward, and the
    unfused backward of them; computed once per case, never written to."""
    C = _ext()
    csr, ea = _graph(n, edges)
    g = torch.Generator().manual_seed(1000 * h + 100 * heads + 10 * n + graphs)
    pdt = BF16 if p16 else torch.float32
    qkvs = torch.randn(n, 4 * h, generator=g).to(BF16).to(DEV)
    pifc = torch.randn(VI, h, generator=g).to(BF16).to(pdt).to(DEV)
    prpc = torch.randn(VR, h, generator=g).to(BF16).to(pdt).to(DEV)
    gout = torch.randn(graphs, h, generator=g).to(DEV)
    # quotients p / n that no float holds exactly
    probs = (torch.rand(n, generator=g) * 0.9 + 0.05)
    nn = torch.tensor([3.0, 5.0, 6.0, 7.0, 11.0])[
        torch.randint(0, 5, (n,), generator=g)]
    probs[0], nn[0] = 0.3, 7.0
    probs, nn = probs.to(DEV), nn.to(DEV)
    batch = _batch_of(n, graphs).to(DEV)
    x, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea, csr[0], csr[1],
                                     False, heads)
    assert x.dtype == torch.float32
    attn = (qkvs, pifc, prpc, ea, alpha, *csr, heads)
    gfull = C.seg_pool_bwd(gout, probs, nn, batch)
    dqkvs, de = C.edge_attn_fused_bwd(gfull, *attn)
    torch.cuda.synchronize()
    return dict(pool=(gout, probs, nn, batch), attn=attn, g=gfull,
                want=(dqkvs, de))


def _assert_pool_equal(got, want, what):
    for name, a, b in zip(("dqkvs", "de"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        ndiff = int((_bits(a) != _bits(b)).sum())
        assert ndiff == 0, (what, name, ndiff, a.numel())


@gpu
@needs_gpu
@pytest.mark.parametrize("graphs", [1, 3])
@pytest.mark.parametrize("n", [1, 11, 67])
@pytest.mark.parametrize("p16", [True, False], ids=["p16", "p32"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("h", [256, 512])
def test_pool_fused_equals_unfused(h, heads, p16, n, graphs):
    C = _ext()
    c = _pool_case(h, heads, n, graphs, p16)
    gout, probs, nn, batch = c["pool"]
    # the inputs tell a pre-divided p / n apart from (gout * p) / n
    pre = gout[batch] * (probs / nn)[:, None]
    assert not torch.equal(pre, c["g"]), "p / n is exact here: weak inputs"
    assert bool(torch.isfinite(c["g"]).all())
    got = C.edge_attn_pool_bwd16(*c["pool"], *c["attn"])
    torch.cuda.synchronize()
    # dskip is the pool gradient, rounded to bf16
    _assert_same_bits(got[0].view(n, 4 * h)[:, 3 * h:], c["g"].to(BF16),
                      (h, heads, p16, n, graphs, "dskip"))
    _assert_pool_equal(got, c["want"], (h, heads, p16, n, graphs))


@gpu
@needs_gpu
@pytest.mark.parametrize("h,heads,p16", [(256, 1, True), (512, 4, False)])
def test_pool_fused_no_edges(h, heads, p16):
    C = _ext()
    c = _pool_case(h, heads, 11, 3, p16, edges=False)
    assert c["attn"][3].shape[0] == 0
    got = C.edge_attn_pool_bwd16(*c["pool"], *c["attn"])
    torch.cuda.synchronize()
    assert got[1].shape == (0, h)
    _assert_pool_equal(got, c["want"], (h, heads, "E=0"))


@gpu
@needs_gpu
def test_pool_binding_rejects_what_it_does_not_cover():
    C = _ext()
    c = _pool_case(256, 1, 11, 3, True)
    gout, probs, nn, batch = c["pool"]
    attn = c["attn"]
    with pytest.raises(RuntimeError, match="bf16 qkvs"):
        C.edge_attn_pool_bwd16(*c["pool"], attn[0].float(), *attn[1:])
    with pytest.raises(RuntimeError, match="gout"):
        C.edge_attn_pool_bwd16(gout[:, :128].contiguous(), probs, nn, batch,
                               *attn)
    with pytest.raises(RuntimeError, match="one entry per node"):
        C.edge_attn_pool_bwd16(gout, probs[:5].contiguous(), nn, batch, *attn)
    with pytest.raises(RuntimeError, match="one entry per node"):
        C.edge_attn_pool_bwd16(gout, probs, nn, batch.int(), *attn)
    torch.cuda.synchronize()
    got = C.edge_attn_pool_bwd16(*c["pool"], *attn)
    _assert_pool_equal(got, c["want"], "after the rejected calls")


# ---------------------------------------------------------------------------
# autograd node
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("mode", ["gmean", "gx", "both"])
@pytest.mark.parametrize("heads", [1, 4])
def test_autograd_node_matches_the_two_nodes(heads, mode, monkeypatch):
    """F.edge_attention_fused_pool with the switch on (one node) and off (the
    two existing nodes) on the same leaves: x, mean_x and the three
    gradients bit-equal, for a gradient on mean_x only (the pool mode of the
    kernels), on x only, and on both.  PERTGNN_DETERMINISTIC=1 puts the
    P-table gradients on the fixed-order list sums."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    h, n, graphs = 256, 67, 3
    c = _pool_case(h, heads, n, graphs, True)
    qkvs0, pifc0, prpc0, ea = c["attn"][:4]
    csr = c["attn"][5:10]
    gout, probs, nn, batch = c["pool"]
    gx = torch.randn(n, h, generator=torch.Generator().manual_seed(5)).to(DEV)
    res = []
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("PERTGNN_NO_POOL_ATTN_FUSE", raising=False)
        else:
            monkeypatch.setenv("PERTGNN_NO_POOL_ATTN_FUSE", "1")
        leaves = [t.detach().clone().requires_grad_(True)
                  for t in (qkvs0, pifc0, prpc0)]
        x, mean_x = F.edge_attention_fused_pool(
            *leaves, ea, csr, probs, nn, batch, graphs, heads=heads)
        one_node = type(x.grad_fn).__name__.startswith("_AttnPoolFn")
        assert one_node == fused, type(x.grad_fn).__name__
        assert (x.grad_fn is mean_x.grad_fn) == fused
        outs, grads = [], []
        if mode in ("gmean", "both"):
            outs.append(mean_x)
            grads.append(gout)
        if mode in ("gx", "both"):
            outs.append(x)
            grads.append(gx)
        torch.autograd.backward(outs, grads)
        torch.cuda.synchronize()
        res.append([x.detach(), mean_x.detach()] + [t.grad for t in leaves])
    for name, a, b in zip(["x", "mean_x", "dqkvs", "dpifc", "dprpc"], *res):
        assert a is not None and b is not None, name
        _assert_same_bits(a, b, (name, heads, mode))
    assert bool(res[0][2].float().abs().max() > 0)
    if mode == "gmean":
        _assert_same_bits(res[0][2], c["want"][0], "dqkvs vs the op-level case")


# ---------------------------------------------------------------------------
# model level (3 layers, H = 256, bf16)
# ---------------------------------------------------------------------------

def _gpu_model(heads=1):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2,
                                                       device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0, heads=heads).to(DEV)
    return model, batches


def _live_params(model):
    return [(n, p) for n, p in model.named_parameters()
            if not isinstance(p, torch.nn.parameter.UninitializedParameter)]


def _model_grads(model, b, local_in_loss):
    """loss, both predictions and the gradient of every parameter the loss
    reaches (None elsewhere), without touching .grad."""
    gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                   b.pattern_num_nodes, b.rt_probs, b.entry_id, b.batch,
                   csr=b.csr, num_graphs=b.num_graphs)
    loss = F.quantile_loss(b.y, gp.flatten(), 0.5)
    if local_in_loss:
        loss = loss + lp.float().mean()
    params = [p for _, p in _live_params(model)]
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return loss.detach(), gp.detach(), lp.detach(), grads


@gpu
@needs_gpu
@pytest.mark.parametrize("local_in_loss", [False, True])
def test_model_switch_on_off_and_captured_bitwise(local_in_loss, monkeypatch):
    """Same model, same batch under PERTGNN_DETERMINISTIC=1 (every kernel then
    repeats itself bit for bit): loss, both predictions and every parameter
    gradient are bit-equal with and without PERTGNN_NO_POOL_ATTN_FUSE=1, and
    the default path captured into a graph and replayed gives the eager bits.
    With ``local_predict`` in the loss the node takes its gx branch."""
    model, batches = _gpu_model()
    model.train()
    b = batches[0]
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    calls = []
    real = F.edge_attention_fused_pool
    real_embed = F.embed_concat_node
    pads = []

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def spy_embed(*a, **k):
        out = real_embed(*a, **k)
        pads.append((k.get("pad_to"), out.shape[1]))
        return out

    names = [n for n, _ in _live_params(model)]
    try:
        F.set_gemm_precision("bf16")
        monkeypatch.setattr(F, "edge_attention_fused_pool", spy)
        monkeypatch.setattr(F, "embed_concat_node", spy_embed)
        monkeypatch.delenv("PERTGNN_NO_POOL_ATTN_FUSE", raising=False)
        on = _model_grads(model, b, local_in_loss)
        assert calls == [1] and pads == [(384, 384)], (calls, pads)
        monkeypatch.setenv("PERTGNN_NO_POOL_ATTN_FUSE", "1")
        off = _model_grads(model, b, local_in_loss)
        monkeypatch.delenv("PERTGNN_NO_POOL_ATTN_FUSE", raising=False)
        torch.cuda.synchronize()

        # captured and replayed (the eager runs above warmed every cache)
        static = [None if g is None else torch.zeros_like(g) for g in on[3]]
        s_out = [torch.zeros_like(t) for t in on[:3]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _model_grads(model, b, local_in_loss)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = _model_grads(model, b, local_in_loss)
            for s, t in zip(s_out, cap[:3]):
                s.copy_(t)
            for s, t in zip(static, cap[3]):
                assert (s is None) == (t is None)
                if s is not None:
                    s.copy_(t)
        for _ in range(2):
            for s in s_out + [s for s in static if s is not None]:
                s.zero_()
            graph.replay()
        torch.cuda.synchronize()
    finally:
        F.set_gemm_precision("fp32")
    for what, other in (("switch off", off), ("captured", (*s_out, static))):
        for name, a, c in zip(("loss", "global_predict", "local_predict"),
                              on[:3], other[:3]):
            _assert_same_bits(a.float(), c.float(), (what, name))
        reached = 0
        for name, a, c in zip(names, on[3], other[3]):
            assert (a is None) == (c is None), (what, name)
            if a is None:
                continue
            reached += 1
            assert bool(torch.isfinite(a).all()), name
            _assert_same_bits(a, c, (what, name))
        assert reached > 10
    reached_names = {n for n, g in zip(names, on[3]) if g is not None}
    assert "cat_embedding.0.weight" in reached_names
    assert ("local_linear.weight" in reached_names) == local_in_loss
