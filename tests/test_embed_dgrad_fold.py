"""The layer-1 dgrad folded into the category-table gradient.

With G[c, :] the sum of the bf16 ``dqkvs`` rows of category c (fp32, list
order) the table gradient is ``G . bf16(w4)[:, f:f+h]`` (``embed_dgrad_fold``):
no [N, k_padded] dgrad, no gather over it.

References are never the code under test: fp64 formed from the same bf16
``dqkvs``, the same bf16-rounded weights and the same indices, and the path
this replaces (``linear_dgrad16_o16`` followed by ``_table_grad``).

Exact operands: ``dqkvs`` from {-2..2}, weights from {-1, 0, 1} with at most
64 non-zeros per input column, so |dx| <= 128 is exact in bf16 and every
fp32 sum is an integer below 2^24: all three agree bit for bit.  Index
vectors put half of all nodes on key 0 and leave every table row r with
r % 3 == 1 unused (a zero row).  n = 4200 with C = 4 has 525 chunks on key 0:
a level 2, and a level-3 list of 132 > C rows.

Random-normal operands: each element's error against fp64 is at most
``terms * 2^-24 * sum|g . w|`` with terms = (nodes of the category) + 4h, the
length of the longest chain of fp32 additions an element can go through, and
the maximum and mean errors are no larger than the replaced path's.
"""
import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

BF16 = torch.bfloat16


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
# operands
# ---------------------------------------------------------------------------

def _indices(n, rows, seed):
    """Half of the nodes on key 0, the rest on rows with r % 3 != 1."""
    g = torch.Generator().manual_seed(seed)
    used = torch.tensor([r for r in range(rows) if r % 3 != 1] or [0])
    idx = used[torch.randint(0, used.numel(), (n,), generator=g)]
    idx[torch.randperm(n, generator=g)[: n // 2]] = 0
    return idx


def _exact_operands(n, f, h, kp, seed):
    g = torch.Generator().manual_seed(seed)
    dq = torch.randint(-2, 3, (n, 4 * h), generator=g).to(BF16)
    w = torch.zeros(4 * h, kp)
    pick = torch.rand(4 * h, kp, generator=g).argsort(0)[:64]   # rows per column
    sign = torch.randint(0, 2, (64, kp), generator=g).float() * 2 - 1
    w.scatter_(0, pick, sign)
    assert int((w != 0).sum(0).max()) <= 64
    return dq, w


def _normal_operands(n, f, h, kp, seed):
    g = torch.Generator().manual_seed(seed)
    dq = torch.randn(n, 4 * h, generator=g).to(BF16)
    w = torch.randn(4 * h, kp, generator=g) / (4 * h) ** 0.5
    return dq, w


def _fp64(dq, w, idx, rows, f, h):
    """(dtable, sum |g . w| per element) in fp64 on the CPU."""
    wb = w[:, f:f + h].to(BF16).double()
    G = torch.zeros(rows, dq.shape[1], dtype=torch.float64)
    G.index_add_(0, idx, dq.double())
    A = torch.zeros(rows, dq.shape[1], dtype=torch.float64)
    A.index_add_(0, idx, dq.double().abs())
    return G @ wb, A @ wb.abs()


def _nan_fill_free_memory(nbytes):
    """Leave NaN bytes in the blocks the caching allocator hands out next."""
    junk = [torch.full((max(nbytes // 4, 1),), float("nan"), device=DEV)
            for _ in range(2)]
    del junk


def _fold(dq, w, idx, rows, f, h, C, sink=None, **kw):
    plan = F.cat_table_plan(idx, rows, C)
    return _ext().embed_dgrad_fold(dq, *plan.tensors(), w, f, h, rows, sink,
                                   **kw), plan


def _parent(dq, w, idx, rows, f, h):
    m = _ext()
    dx = m.linear_dgrad16_o16(dq, w, False, None)
    return F._table_grad(m, dx, idx, rows, h, f)


# ---------------------------------------------------------------------------
# plan (CPU)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,rows,C", [(0, 3, 4), (1, 1, 4), (65, 3, 64),
                                      (1000, 161, 4), (4200, 1024, 4),
                                      (4200, 161, 64)])
def test_plan_structure(n, rows, C):
    idx = _indices(n, rows, seed=n + rows)
    plan = F._build_cat_table_plan(idx, rows, C)
    i1, l1, i2, l2, i3, l3 = [t.long() for t in plan.tensors()]
    assert (plan.V, plan.R, plan.C) == (rows, 0, C)
    # level 1: the stable sort order, cut into chunks of one key, <= C long
    assert torch.equal(i1, torch.argsort(idx, stable=True))
    assert int(l1[0]) == 0 and int(l1[-1]) == n and l1.numel() == plan.n1 + 1
    lens = l1[1:] - l1[:-1]
    assert plan.n1 == 0 or (int(lens.min()) >= 1 and int(lens.max()) <= C)
    key = idx[i1]
    for a, b in zip(l1[:-1].tolist(), l1[1:].tolist()):
        assert int(key[a]) == int(key[b - 1])
    counts = torch.bincount(idx, minlength=rows)
    assert plan.n1 == int(((counts + C - 1) // C).sum())
    # level 2 exists exactly when a row has more than C chunks
    chunks = (counts + C - 1) // C
    assert (plan.n2 > 0) == bool((chunks > C).any())
    assert l2.numel() == plan.n2 + 1 and int(l2[-1]) == i2.numel()
    if plan.n2:
        assert int((l2[1:] - l2[:-1]).max()) <= C
    # level 3: one list per row, empty for an unused one
    assert l3.numel() == rows + 1 and int(l3[-1]) == i3.numel()
    assert torch.equal((l3[1:] - l3[:-1]) == 0, counts == 0)
    if n == 4200 and C == 4:
        assert plan.n2 > 0 and int((l3[1:] - l3[:-1]).max()) > C
    # the three passes reproduce the segment sum exactly
    de = torch.randint(-2, 3, (n, 8)).float()
    out, none = F.apply_plan_reference(plan, de)
    want = torch.zeros(rows, 8).index_add_(0, idx, de)
    assert none.shape[0] == 0 and torch.equal(out, want)


def test_plan_rejects_out_of_range():
    with pytest.raises(IndexError):
        F._build_cat_table_plan(torch.tensor([0, 3]), 3, 4)
    with pytest.raises(IndexError):
        F._build_cat_table_plan(torch.tensor([-1, 0]), 3, 4)
    with pytest.raises(IndexError):
        F.cat_table_plan(torch.tensor([5]), 5)


def test_plan_cache_hit_and_eviction(monkeypatch):
    import collections
    monkeypatch.setattr(F, "_GROUP_CACHE", collections.OrderedDict())
    monkeypatch.setattr(F, "_GROUP_CACHE_BYTES", [0])
    idx = _indices(100, 7, seed=0)
    p1 = F.cat_table_plan(idx, 7, 4)
    calls = []
    real = F._build_cat_table_plan
    monkeypatch.setattr(F, "_build_cat_table_plan",
                        lambda *a: calls.append(1) or real(*a))
    assert F.cat_table_plan(idx, 7, 4) is p1 and calls == []     # hit
    assert F.cat_table_plan(idx[:], 7, 4) is p1 and calls == []  # same view key
    F.cat_table_plan(idx, 7, 8)                                  # other C
    assert calls == [1]
    # eviction at the byte budget: the oldest entry goes first
    key = ("cat_table", idx.data_ptr(), idx.numel(), tuple(idx.stride()), 7, 4)
    assert key in F._GROUP_CACHE
    monkeypatch.setattr(F, "_GROUP_CACHE_CAP", F._GROUP_CACHE_BYTES[0])
    other = _indices(50, 7, seed=1)
    F.cat_table_plan(other, 7, 4)
    assert F._GROUP_CACHE_BYTES[0] <= F._GROUP_CACHE_CAP
    assert ("cat_table", other.data_ptr(), 50, (1,), 7, 4) in F._GROUP_CACHE
    assert key not in F._GROUP_CACHE
    assert F._GROUP_CACHE_BYTES[0] == sum(v[-1] for v in F._GROUP_CACHE.values())


# ---------------------------------------------------------------------------
# binding
# ---------------------------------------------------------------------------

_EXACT = {}


def _exact_case(n, rows, h):
    """Operands, fp64 reference and the replaced path's result, computed once
    per (n, rows, h) and shared by both chunk sizes."""
    k = (n, rows, h)
    if k not in _EXACT:
        f, kp = 9, (384 if h == 256 else 640)
        dq, w = _exact_operands(n, f, h, kp, seed=n * 7 + rows)
        idx = _indices(n, rows, seed=n + rows)
        want, _ = _fp64(dq, w, idx, rows, f, h)
        assert float(want.abs().max()) < 2 ** 24
        dqd, wd, idxd = dq.to(DEV), w.to(DEV), idx.to(DEV)
        parent = _parent(dqd, wd, idxd, rows, f, h)
        _EXACT[k] = (dqd, wd, idxd, f, kp, want.float().to(DEV), parent)
    return _EXACT[k]


@gpu
@needs_gpu
@pytest.mark.parametrize("C", [4, 64])
@pytest.mark.parametrize("rows", [1, 3, 161, 1024])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 4200])
def test_fold_exact_equals_fp64_and_parent(n, rows, C):
    dq, w, idx, f, kp, want, parent = _exact_case(n, rows, 256)
    _nan_fill_free_memory(64 << 20)
    got, plan = _fold(dq, w, idx, rows, f, 256, C)
    if n == 4200 and C == 4:
        assert plan.n2 > 0
    _assert_same_bits(got, want, "fold vs fp64")
    _assert_same_bits(got, parent, "fold vs dgrad + table_grad")
    unused = torch.bincount(idx, minlength=rows) == 0
    assert n == 0 or rows == 1 or bool(unused.any())
    assert int(_bits(got[unused]).ne(0).sum()) == 0   # +0 rows


@gpu
@needs_gpu
@pytest.mark.parametrize("C,seg", [(4, 256), (64, 512)])
def test_fold_exact_h512(C, seg):
    dq, w, idx, f, kp, want, parent = _exact_case(1000, 161, 512)
    _nan_fill_free_memory(64 << 20)
    got, _ = _fold(dq, w, idx, 161, f, 512, C, seg_cols=seg)
    _assert_same_bits(got, want, "fold vs fp64")
    _assert_same_bits(got, parent, "fold vs dgrad + table_grad")


@gpu
@needs_gpu
@pytest.mark.parametrize("unroll,seg", [(4, 256), (8, 512), (4, 512)])
def test_fold_other_instantiations(unroll, seg):
    dq, w, idx, f, kp, want, _ = _exact_case(4200, 161, 256)
    got, _ = _fold(dq, w, idx, 161, f, 256, 4, unroll=unroll, seg_cols=seg)
    _assert_same_bits(got, want, (unroll, seg))


@gpu
@needs_gpu
@pytest.mark.parametrize("h", [256, 512])
def test_fold_random_normal_error(h):
    n, rows, f, kp = 4200, 161, 9, (384 if h == 256 else 640)
    dq, w = _normal_operands(n, f, h, kp, seed=h)
    idx = _indices(n, rows, seed=3)
    want, mag = _fp64(dq, w, idx, rows, f, h)
    terms = (torch.bincount(idx, minlength=rows) + 4 * h).double()[:, None]
    got, _ = _fold(dq.to(DEV), w.to(DEV), idx.to(DEV), rows, f, h, 64)
    par = _parent(dq.to(DEV), w.to(DEV), idx.to(DEV), rows, f, h)
    err = (got.double().cpu() - want).abs()
    perr = (par.double().cpu() - want).abs()
    print(f"h={h}: fold max/mean err {err.max():.3e}/{err.mean():.3e}  "
          f"parent {perr.max():.3e}/{perr.mean():.3e}  "
          f"worst err/bound {(err / (terms * 2.0 ** -24 * mag + 1e-300)).max():.3e}")
    assert bool((err <= terms * 2.0 ** -24 * mag).all())
    assert float(err.max()) <= float(perr.max())
    assert float(err.mean()) <= float(perr.mean())


@gpu
@needs_gpu
@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("n,rows,C", [(65, 3, 64), (4200, 161, 4)])
def test_fold_sink_adds(n, rows, C, offset):
    """+= into a slice of a flat buffer (4-byte aligned, 16-byte aligned only
    for offset 0) equals pre-fill + stored form; its neighbours stay."""
    h = 256
    dq, w, idx, f, kp, want, _ = _exact_case(n, rows, h)
    stored, _ = _fold(dq, w, idx, rows, f, h, C)
    g = torch.Generator().manual_seed(offset)
    flat = torch.randint(-8, 9, (offset + rows * h + 5,), generator=g).float().to(DEV)
    before = flat.clone()
    sink = flat[offset:offset + rows * h].view(rows, h)
    assert sink.data_ptr() % 16 == (4 * offset) % 16
    ret, _ = _fold(dq, w, idx, rows, f, h, C, sink=sink)
    assert ret.numel() == 0
    _assert_same_bits(sink, before[offset:offset + rows * h].view(rows, h) + stored,
                      "sink")
    _assert_same_bits(flat[:offset], before[:offset], "before the slice")
    _assert_same_bits(flat[offset + rows * h:], before[offset + rows * h:],
                      "after the slice")
    # no nodes: the sink stays, nothing is launched
    p0 = F.cat_table_plan(idx[:0], rows, C)
    _ext().embed_dgrad_fold(dq[:0], *p0.tensors(), w, f, h, rows, sink)
    _assert_same_bits(flat[:offset + rows * h], torch.cat(
        [before[:offset], (before[offset:offset + rows * h].view(rows, h)
                           + stored).flatten()]), "n = 0 with a sink")


@gpu
@needs_gpu
def test_fold_shape_errors():
    dq, w, idx, f, kp, want, _ = _exact_case(65, 3, 256)
    plan = F.cat_table_plan(idx, 3, 4)
    m = _ext()
    t = plan.tensors()
    with pytest.raises(RuntimeError):   # h not covered
        m.embed_dgrad_fold(dq, *t, w, f, 128, 3)
    with pytest.raises(RuntimeError):   # dqkvs not bf16
        m.embed_dgrad_fold(dq.float(), *t, w, f, 256, 3)
    with pytest.raises(RuntimeError):   # table columns outside w4
        m.embed_dgrad_fold(dq, *t, w, kp - 255, 256, 3)
    with pytest.raises(RuntimeError):   # plan of another table size
        m.embed_dgrad_fold(dq, *t, w, f, 256, 4)
    with pytest.raises(RuntimeError):   # plan of another node count
        m.embed_dgrad_fold(dq[:64], *t, w, f, 256, 3)
    with pytest.raises(RuntimeError):   # sink of the wrong shape
        m.embed_dgrad_fold(dq, *t, w, f, 256, 3,
                           torch.zeros(3, 255, device=DEV))
    with pytest.raises(RuntimeError):   # column segment not covered
        m.embed_dgrad_fold(dq, *t, w, f, 256, 3, None, 8, 128)


# ---------------------------------------------------------------------------
# autograd node
# ---------------------------------------------------------------------------

class _SpyExt:
    """The extension module, recording which bindings are reached."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._real, name)


def _node_inputs(n, rows, seed, x_grad=False, tables=1):
    f, h, kp = 9, 256, 384
    g = torch.Generator().manual_seed(seed)
    dq, w = _exact_operands(n, f, h, kp, seed)
    w[:, f + h:] = 0
    x_raw = torch.randint(-2, 3, (n, f), generator=g).float().to(DEV)
    x_raw.requires_grad_(x_grad)
    cat_X = torch.stack([_indices(n, rows, seed + t) for t in range(tables)],
                        1).to(DEV)
    tabs = [torch.randint(-2, 3, (rows, h), generator=g).float().to(DEV)
            .requires_grad_(True) for _ in range(tables)]
    w = w.to(DEV).requires_grad_(True)
    b = torch.randint(-2, 3, (4 * h,), generator=g).float().to(DEV)
    b.requires_grad_(True)
    return x_raw, cat_X, tabs, w, b, dq.to(DEV), (f, h, kp)


def _run_node(x_raw, cat_X, tabs, w, b, dq, out16, monkeypatch):
    calls = []
    monkeypatch.setattr(F, "ext", lambda: _SpyExt(_ext(), calls))
    x = F.embed_concat_node(x_raw, cat_X, tabs, out16=out16, pad_to=384)
    qkvs = F.linear16_embed(x, w, b)
    ins = [w, b, *tabs] + ([x_raw] if x_raw.requires_grad else [])
    grads = torch.autograd.grad(qkvs, ins, dq, allow_unused=True)
    monkeypatch.undo()
    return qkvs.detach(), grads, calls


@gpu
@needs_gpu
@pytest.mark.parametrize("n,rows", [(65, 3), (1000, 161)])
def test_node_matches_linear16(n, rows, monkeypatch):
    x_raw, cat_X, tabs, w, b, dq, (f, h, kp) = _node_inputs(n, rows, seed=n)
    try:
        F.set_gemm_precision("bf16")
        monkeypatch.delenv("PERTGNN_NO_EMBED_DGRAD_FOLD", raising=False)
        y_on, g_on, c_on = _run_node(x_raw, cat_X, tabs, w, b, dq, True,
                                     monkeypatch)
        monkeypatch.setenv("PERTGNN_NO_EMBED_DGRAD_FOLD", "1")
        y_off, g_off, c_off = _run_node(x_raw, cat_X, tabs, w, b, dq, True,
                                        monkeypatch)
    finally:
        F.set_gemm_precision("fp32")
    assert "embed_dgrad_fold" in c_on and "linear_dgrad16_o16" not in c_on
    assert "linear_fwd_a16o16" in c_on and "linear_fwd_a16o16_wt" not in c_on
    assert "embed_dgrad_fold" not in c_off and "linear_dgrad16_o16" in c_off
    _assert_same_bits(y_on, y_off, "qkvs")
    _assert_same_bits(g_on[0], g_off[0], "dw")
    _assert_same_bits(g_on[1], g_off[1], "db")
    want, _ = _fp64(dq.cpu(), w.detach().cpu(), cat_X[:, 0].cpu(), rows, f, h)
    _assert_same_bits(g_on[2], want.float().to(DEV), "dtable vs fp64")
    _assert_same_bits(g_on[2], g_off[2], "dtable vs the dgrad path")


@gpu
@needs_gpu
@pytest.mark.parametrize("why", ["x_raw_grad", "two_tables", "fp32_operand",
                                 "fp16_cores", "no_grad_table"])
def test_node_ineligible_takes_the_dgrad(why, monkeypatch):
    monkeypatch.delenv("PERTGNN_NO_EMBED_DGRAD_FOLD", raising=False)
    x_raw, cat_X, tabs, w, b, dq, _ = _node_inputs(
        65, 3, seed=5, x_grad=why == "x_raw_grad",
        tables=2 if why == "two_tables" else 1)
    if why == "two_tables":   # the concat is 9 + 2 * 256 wide: its own weight
        w = torch.zeros(1024, 521 + 23, device=DEV, requires_grad=True)
    if why == "no_grad_table":
        tabs[0].requires_grad_(False)
        x_raw.requires_grad_(True)
    try:
        F.set_gemm_precision("fp16" if why == "fp16_cores" else "bf16")
        calls = []
        monkeypatch.setattr(F, "ext", lambda: _SpyExt(_ext(), calls))
        x = F.embed_concat_node(x_raw, cat_X, tabs,
                                out16=why != "fp32_operand",
                                pad_to=w.shape[1])
        qkvs = F.linear16_embed(x, w, b)
        torch.autograd.grad(qkvs, [w], dq)
    finally:
        F.set_gemm_precision("fp32")
    assert "embed_dgrad_fold" not in calls, calls
    assert "linear_dgrad16_o16" in calls or "linear_dgrad16" in calls, calls


# ---------------------------------------------------------------------------
# model level (3 layers, H = 256, bf16, PERTGNN_DETERMINISTIC=1)
# ---------------------------------------------------------------------------

TABLE = "cat_embedding.0.weight"


def _gpu_model():
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2,
                                                       device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0).to(DEV)
    model.train()
    return model, batches


def _live_params(model):
    return [(n, p) for n, p in model.named_parameters()
            if not isinstance(p, torch.nn.parameter.UninitializedParameter)]


def _model_grads(model, b):
    gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                   b.pattern_num_nodes, b.rt_probs, b.entry_id, b.batch,
                   csr=b.csr, num_graphs=b.num_graphs)
    loss = F.quantile_loss(b.y, gp.flatten(), 0.5)
    params = [p for _, p in _live_params(model)]
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    return loss.detach(), gp.detach(), lp.detach(), grads


@gpu
@needs_gpu
def test_model_switch_and_captured(monkeypatch):
    """Switch on against PERTGNN_NO_EMBED_DGRAD_FOLD=1: loss, predictions and
    every gradient but the category table's are bit-equal; the table's is
    judged against fp64 formed from the layer-1 dqkvs the model produced, and
    is no further from it than the dgrad path's.  Captured and replayed equals
    eager for everything."""
    model, batches = _gpu_model()
    b = batches[0]
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    names = [n for n, _ in _live_params(model)]
    seen = {}
    real_fold = _ext().embed_dgrad_fold

    class Tap(_SpyExt):
        def __getattr__(self, name):
            if name == "embed_dgrad_fold":
                def tap(dq, *a, **k):
                    seen["dq"] = dq.detach().clone()
                    seen["calls"] = seen.get("calls", 0) + 1
                    return real_fold(dq, *a, **k)
                return tap
            return getattr(self._real, name)

    try:
        F.set_gemm_precision("bf16")
        monkeypatch.delenv("PERTGNN_NO_EMBED_DGRAD_FOLD", raising=False)
        monkeypatch.setattr(F, "ext", lambda: Tap(_ext(), []))
        on = _model_grads(model, b)
        monkeypatch.setattr(F, "ext", _ext)
        assert seen.get("calls") == 1
        monkeypatch.setenv("PERTGNN_NO_EMBED_DGRAD_FOLD", "1")
        off = _model_grads(model, b)
        monkeypatch.delenv("PERTGNN_NO_EMBED_DGRAD_FOLD", raising=False)
        torch.cuda.synchronize()

        static = [None if g is None else torch.zeros_like(g) for g in on[3]]
        s_out = [torch.zeros_like(t) for t in on[:3]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _model_grads(model, b)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap = _model_grads(model, b)
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
        for name, a, c in zip(names, on[3], other[3]):
            assert (a is None) == (c is None), (what, name)
            if a is None or (what == "switch off" and name == TABLE):
                continue
            _assert_same_bits(a, c, (what, name))
    # the table gradient against fp64 from the same dqkvs, weights, indices
    conv = model.convs[0]
    h, f = 256, 9
    rows = model.cat_embedding[0].weight.shape[0]
    idx = b.cat_X[:, 0].cpu()
    want, mag = _fp64(seen["dq"].cpu(), conv.w4.detach().cpu(), idx, rows, f, h)
    terms = (torch.bincount(idx, minlength=rows) + 4 * h).double()[:, None]
    k = names.index(TABLE)
    err = (on[3][k].double().cpu() - want).abs()
    perr = (off[3][k].double().cpu() - want).abs()
    print(f"model table grad: fold max/mean err {err.max():.3e}/{err.mean():.3e}"
          f"  dgrad path {perr.max():.3e}/{perr.mean():.3e}")
    assert bool(want.abs().max() > 0)
    assert bool((err <= terms * 2.0 ** -24 * mag).all())
    assert float(err.max()) <= float(perr.max())
    assert float(err.mean()) <= float(perr.mean())


@gpu
@needs_gpu
def test_model_table_sink_on_off_bitwise(monkeypatch):
    """With a FusedAdam the table gradient goes into flat_grad: bit-equal to
    PERTGNN_NO_GRAD_SINK=1 after one and after two backwards, and the table's
    AccumulateGrad stays silent on the sink path."""
    from pertgnn.train.optim import FusedAdam

    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    monkeypatch.delenv("PERTGNN_NO_EMBED_DGRAD_FOLD", raising=False)
    model, batches = _gpu_model()
    b = batches[0]
    opt = FusedAdam(model.parameters(), lr=1e-3)
    fired = []
    model.cat_embedding[0].weight.register_post_accumulate_grad_hook(
        lambda p: fired.append(1))
    res = {}
    try:
        F.set_gemm_precision("bf16")
        for mode in ("sink", "return"):
            if mode == "sink":
                monkeypatch.delenv("PERTGNN_NO_GRAD_SINK", raising=False)
            else:
                monkeypatch.setenv("PERTGNN_NO_GRAD_SINK", "1")
            opt.zero_grad()
            del fired[:]
            out = []
            for _ in range(2):
                gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr,
                               b.pattern_num_nodes, b.rt_probs, b.entry_id,
                               b.batch, csr=b.csr, num_graphs=b.num_graphs)
                loss = F.quantile_loss(b.y, gp.flatten(), 0.5)
                loss.backward()
                out.append((loss.detach().clone(),
                            opt.flat_grad.detach().clone()))
            torch.cuda.synchronize()
            res[mode] = (out, len(fired))
    finally:
        F.set_gemm_precision("fp32")
    (s, fired_s), (r, fired_r) = res["sink"], res["return"]
    assert fired_s == 0 and fired_r == 2, (fired_s, fired_r)
    for i in range(2):
        _assert_same_bits(s[i][0], r[i][0], f"loss {i}")
        _assert_same_bits(s[i][1], r[i][1], f"flat_grad after {i + 1}")
    assert bool(model.cat_embedding[0].weight.grad.abs().max() > 0)
