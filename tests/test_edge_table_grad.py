"""Edge-table gradient: the grouping plan (CPU) and the single-pass list-sum
op that turns de [E, h] into dP_ifc [V, h] and dP_rpc [R, h] (GPU).

CPU and GPU tests share this file, so the GPU ones carry the ``gpu`` mark
and the no-GPU skip one by one (as tests/test_multihead.py does) instead of
a module-level ``pytestmark``.

Run on an MI355X box:  python -m pytest tests/test_edge_table_grad.py -m gpu -q
"""
import functools

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

# fp32 table rows: tests/test_gpu_ops.py::test_large_table_skewed_scatter_parity
FP32_OUT = dict(atol=5e-3, rtol=1e-4)
# bf16 table rows: one round-to-nearest at the store is 2^-9 relative; x2
BF16_OUT = dict(atol=5e-3, rtol=2.0 ** -8)
# tests/test_multihead.py::test_fused_bf16_fwd_bwd
BF16_TOL = dict(atol=1e-2, rtol=1e-2)


# ---------------------------------------------------------------------------
# index sets
# ---------------------------------------------------------------------------

def _one_key(n, V=3, R=2, ifc=1, rpc=1):
    return (torch.full((n,), ifc, dtype=torch.long),
            torch.full((n,), rpc, dtype=torch.long), V, R)


def _random_half_on_zero(E, V, R, seed):
    g = torch.Generator().manual_seed(seed)
    ifc = torch.randint(0, V, (E,), generator=g)
    ifc[torch.randperm(E, generator=g)[: E // 2]] = 0
    rpc = torch.randint(0, R, (E,), generator=g)
    return ifc, rpc, V, R


def _cases(C):
    """name -> (ifc, rpc, V, R, expects a level 2).  ``over_ccc`` has more
    than C*C level-1 rows on one key, so its level-3 lists are longer than
    C (a run of C*C+1 edges is only C+1 level-1 rows)."""
    return {
        "empty": (torch.zeros(0, dtype=torch.long),
                  torch.zeros(0, dtype=torch.long), 3, 2, False),
        "five_edges_row_unused": (torch.tensor([2, 0, 2, 0, 0]),
                                  torch.tensor([1, 0, 0, 1, 1]), 3, 2, False),
        "run_c": _one_key(C) + (False,),
        "run_c_plus_1": _one_key(C + 1) + (False,),
        "run_cc_plus_1": _one_key(C * C + 1) + (True,),
        "over_ccc": _one_key(C * C * C + 1) + (True,),
        "random_2000": _random_half_on_zero(2000, 50, 5, 0) + (True,),
        "no_level_2": (torch.arange(6) % 3, torch.arange(6) % 2, 3, 2, False),
    }


CASE_NAMES = sorted(_cases(4))


def _oracle(ifc, rpc, V, R, de):
    """index_add_ in de's (floating) dtype."""
    dp = torch.zeros(V, de.shape[1], dtype=de.dtype).index_add_(0, ifc, de)
    dr = torch.zeros(R, de.shape[1], dtype=de.dtype).index_add_(0, rpc, de)
    return dp, dr


def _lists(idx, lptr):
    return [idx[lptr[w]:lptr[w + 1]] for w in range(lptr.numel() - 1)]


# ---------------------------------------------------------------------------
# the plan (CPU)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_NAMES)
def test_plan_invariants(name):
    C = 4
    ifc, rpc, V, R, has_l2 = _cases(C)[name]
    E = ifc.numel()
    ea = torch.stack([ifc, rpc, torch.ones_like(ifc), torch.zeros_like(ifc)],
                     dim=1)
    plan = F.edge_table_plan(ea, V, R, C=C)
    assert all(t.dtype == torch.int32 for t in plan.tensors())
    assert (plan.V, plan.R, plan.C) == (V, R, C)
    # every edge exactly once at level 1
    assert torch.equal(plan.idx1.long().sort().values, torch.arange(E))
    key = ifc * R + rpc
    l1 = _lists(plan.idx1.long(), plan.lptr1.long())
    assert len(l1) == plan.n1
    for lst in l1:
        assert 1 <= lst.numel() <= C
        assert key[lst].unique().numel() == 1     # no chunk crosses a key
    l2 = _lists(plan.idx2.long(), plan.lptr2.long())
    assert len(l2) == plan.n2 and (plan.n2 > 0) == has_l2
    for lst in l2:
        assert 1 <= lst.numel() <= C
        assert int(lst.max()) < plan.n1
    # exactly one level-3 list per output row, over existing partial rows
    assert plan.lptr3.numel() == V + R + 1
    assert int(plan.lptr3[0]) == 0 and int(plan.lptr3[-1]) == plan.idx3.numel()
    assert bool((plan.lptr3[1:] >= plan.lptr3[:-1]).all())
    assert plan.idx3.numel() == 0 or int(plan.idx3.max()) < plan.n1 + plan.n2
    l3 = _lists(plan.idx3.long(), plan.lptr3.long())
    if name == "over_ccc":
        assert max(lst.numel() for lst in l3) > C
    elif name != "random_2000":
        assert max(lst.numel() for lst in l3) <= C
    # the three passes give the segment sums
    de = torch.randn(E, 8, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(1))
    dp, dr = F.apply_plan_reference(plan, de)
    want_p, want_r = _oracle(ifc, rpc, V, R, de)
    assert dp.dtype == torch.float64 and dp.shape == (V, 8) and dr.shape == (R, 8)
    assert torch.allclose(dp, want_p, atol=1e-9, rtol=0)
    assert torch.allclose(dr, want_r, atol=1e-9, rtol=0)
    used = torch.zeros(V, dtype=torch.bool).index_fill_(0, ifc, True)
    assert bool((dp[~used] == 0).all())


def test_plan_is_cached_per_view_and_checks_range():
    ifc, rpc, V, R, _ = _cases(4)["random_2000"]
    ea = torch.stack([ifc, rpc], dim=1)
    a = F.edge_table_plan(ea, V, R, C=4)
    assert F.edge_table_plan(ea, V, R, C=4) is a
    assert F.edge_table_plan(ea, V, R, C=8) is not a
    assert F.edge_table_plan(ea.clone(), V, R, C=4) is not a
    with pytest.raises(IndexError):
        F.edge_table_plan(ea.clone(), V - 49, R, C=4)


# ---------------------------------------------------------------------------
# the op (GPU)
# ---------------------------------------------------------------------------

def _ea(ifc, rpc):
    return torch.stack([ifc, rpc, torch.ones_like(ifc), torch.zeros_like(ifc)],
                       dim=1).contiguous()


def _op(de, ea, V, R, out_dtype, C=None):
    import pertgnn._C as m

    plan = F.edge_table_plan(ea, V, R, C=C)
    out = m.edge_table_grad(de, *plan.tensors(), V, R, out_dtype)
    assert out.shape == (V + R, de.shape[1]) and out.dtype == out_dtype
    return out[:V], out[V:], plan


def _close(name, got, want, tol):
    got = got.detach().float().cpu()
    want = want.float().cpu()
    err = float((got - want).abs().max()) if got.numel() else 0.0
    ref = float(want.abs().max()) if want.numel() else 0.0
    print(f"  {name}: max abs err {err:.3e} (max |ref| {ref:.3e})")
    bad = (got - want).abs() > tol["atol"] + tol["rtol"] * want.abs()
    assert not bool(bad.any()), (name, err, int(bad.sum()))


@functools.lru_cache(maxsize=None)
def _big(h, in16):
    """E=60000 over V=2048, R=5, half the edges on interface 0: level 2 for
    ifc row 0 and for every rpc row.  Returns CPU index vectors, de (rounded
    to bf16 when in16) and the fp32 index_add_ oracle on the upcast de."""
    ifc, rpc, V, R = _random_half_on_zero(60_000, 2048, 5, 3)
    de = torch.randn(60_000, h, generator=torch.Generator().manual_seed(4))
    if in16:
        de = de.to(torch.bfloat16)
    return ifc, rpc, V, R, de, _oracle(ifc, rpc, V, R, de.float())


@gpu
@needs_gpu
@pytest.mark.parametrize("h,in16,out16", [
    (256, True, False), (256, True, True), (256, False, False),
    (256, False, True), (512, True, True),
])
def test_parity_with_index_add(h, in16, out16):
    ifc, rpc, V, R, de, (want_p, want_r) = _big(h, in16)
    out_dtype = torch.bfloat16 if out16 else torch.float32
    tol = BF16_OUT if out16 else FP32_OUT
    ea = _ea(ifc, rpc).to(DEV)
    de_d = de.to(DEV)
    dp, dr, plan = _op(de_d, ea, V, R, out_dtype)
    assert plan.n2 >= 1 + R
    _close("dP_ifc", dp, want_p, tol)
    _close("dP_rpc", dr, want_r, tol)
    used = torch.zeros(V, dtype=torch.bool).index_fill_(0, ifc, True)
    assert bool((dp.cpu()[~used] == 0).all())
    # the same three passes in torch
    rp, rr = F.apply_plan_reference(plan, de_d)
    _close("dP_ifc vs plan reference", dp, rp, tol)
    _close("dP_rpc vs plan reference", dr, rr, tol)
    # bitwise reproducible
    dp2, dr2, _ = _op(de_d, ea, V, R, out_dtype)
    assert torch.equal(dp, dp2) and torch.equal(dr, dr2)


@gpu
@needs_gpu
@pytest.mark.parametrize("unroll", [4, 8])
def test_unroll_variants_agree(unroll):
    import pertgnn._C as m

    ifc, rpc, V, R, de, (want_p, want_r) = _big(256, True)
    ea = _ea(ifc, rpc).to(DEV)
    plan = F.edge_table_plan(ea, V, R)
    out = m.edge_table_grad(de.to(DEV), *plan.tensors(), V, R, torch.float32,
                            unroll=unroll)
    _close("dP_ifc", out[:V], want_p, FP32_OUT)
    _close("dP_rpc", out[V:], want_r, FP32_OUT)


@gpu
@needs_gpu
@pytest.mark.parametrize("name", [
    "empty", "five_edges_row_unused", "run_c", "run_c_plus_1",
    "run_cc_plus_1", "no_level_2"])
@pytest.mark.parametrize("C", [None, 8])
def test_edge_cases(name, C):
    """The toy and boundary shapes at the default chunk size, and at C=8
    where the same shapes reach level 2 (runs of 8, 9 and 65)."""
    c = F._scatter_iters() if C is None else C
    ifc, rpc, V, R, _ = _cases(c)[name]
    E = ifc.numel()
    de = torch.randn(E, 256, generator=torch.Generator().manual_seed(5))
    de = de.to(torch.bfloat16)
    want_p, want_r = _oracle(ifc, rpc, V, R, de.float())
    ea = _ea(ifc, rpc).to(DEV)
    for out_dtype, tol in ((torch.float32, FP32_OUT),
                           (torch.bfloat16, BF16_OUT)):
        dp, dr, plan = _op(de.to(DEV), ea, V, R, out_dtype, C=C)
        _close("dP_ifc", dp, want_p, tol)
        _close("dP_rpc", dr, want_r, tol)
        rp, rr = F.apply_plan_reference(plan, de.to(DEV))
        _close("dP_ifc vs plan reference", dp, rp, tol)
        _close("dP_rpc vs plan reference", dr, rr, tol)
        used = torch.zeros(V, dtype=torch.bool).index_fill_(0, ifc, True)
        assert bool((dp.cpu()[~used] == 0).all())
        if E == 0:
            assert bool((dp == 0).all()) and bool((dr == 0).all())


@gpu
@needs_gpu
def test_over_long_level3_list():
    """More than C*C level-1 rows on one key at C=8 (513 edges): the
    level-3 lists of that ifc row and that rpc row are longer than C."""
    ifc, rpc, V, R, _ = _cases(8)["over_ccc"]
    de = torch.randn(ifc.numel(), 256,
                     generator=torch.Generator().manual_seed(6))
    want_p, want_r = _oracle(ifc, rpc, V, R, de)
    dp, dr, plan = _op(de.to(DEV), _ea(ifc, rpc).to(DEV), V, R,
                       torch.float32, C=8)
    assert int((plan.lptr3[1:] - plan.lptr3[:-1]).max()) > 8
    _close("dP_ifc", dp, want_p, FP32_OUT)
    _close("dP_rpc", dr, want_r, FP32_OUT)


@gpu
@needs_gpu
@pytest.mark.parametrize("out16", [False, True])
def test_agrees_with_the_two_table_scatters(out16):
    """Against the path it replaces: two _table_grad calls plus the cast."""
    import pertgnn._C as m

    ifc, rpc, V, R, de, _ = _big(256, True)
    ea = _ea(ifc, rpc).to(DEV)
    de_d = de.to(DEV)
    out_dtype = torch.bfloat16 if out16 else torch.float32
    old_p = F._table_grad(m, de_d, ea[:, 0], V, 256, 0).to(out_dtype)
    old_r = F._table_grad(m, de_d, ea[:, 1], R, 256, 0).to(out_dtype)
    dp, dr, _ = _op(de_d, ea, V, R, out_dtype)
    tol = BF16_OUT if out16 else FP32_OUT
    _close("dP_ifc", dp, old_p, tol)
    _close("dP_rpc", dr, old_r, tol)


@gpu
@needs_gpu
def test_unsupported_width_and_bad_plan_raise():
    import pertgnn._C as m

    ifc, rpc, V, R, _ = _cases(8)["five_edges_row_unused"]
    ea = _ea(ifc, rpc).to(DEV)
    plan = F.edge_table_plan(ea, V, R)
    with pytest.raises(RuntimeError, match="unsupported shape"):
        m.edge_table_grad(torch.zeros(5, 128, device=DEV), *plan.tensors(),
                          V, R, torch.float32)
    with pytest.raises(RuntimeError, match="V\\+R\\+1"):
        m.edge_table_grad(torch.zeros(5, 256, device=DEV), *plan.tensors(),
                          V + 1, R, torch.float32)
    with pytest.raises(RuntimeError, match="every row of de"):
        m.edge_table_grad(torch.zeros(6, 256, device=DEV), *plan.tensors(),
                          V, R, torch.float32)


# ---------------------------------------------------------------------------
# through the attention op and a captured training step (GPU)
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _attention_case():
    """The skewed n=333, e=2000, h=256 graph of tests/test_gpu_ops.py with a
    V=2048 interface table (half the edges on interface 0); bf16-rounded
    operands on the CPU."""
    from pertgnn.data.collate import build_csr

    n, e, h, V, R = 333, 2000, 256, 2048, 5
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.cat([torch.zeros(e // 2, dtype=torch.long),
                     torch.randint(0, n, (e - e // 2,), generator=g)])
    edge_index = torch.stack([src, dst])
    perm, row_ptr, csr_src, col_ptr, csc_dst, csc_eid = build_csr(edge_index, n)
    ifc, rpc, _, _ = _random_half_on_zero(e, V, R, 7)
    qkvs = torch.randn(n, 4 * h, generator=g).to(torch.bfloat16)
    pifc = torch.randn(V, h, generator=g).to(torch.bfloat16)
    prpc = torch.randn(R, h, generator=g).to(torch.bfloat16)
    gout = torch.randn(n, h, generator=g).to(torch.bfloat16)
    return ((row_ptr, csr_src, col_ptr, csc_dst, csc_eid), _ea(ifc, rpc),
            qkvs, pifc, prpc, gout)


@functools.lru_cache(maxsize=None)
def _attention_reference(heads):
    """fp32 _fused_eager gradients on the rounded operands, and per table
    row the sum of |de| (each de is stored as bf16 before it is summed)."""
    from pertgnn.ops import reference as ref

    csr, ea, qkvs, pifc, prpc, gout = _attention_case()
    pf = pifc.float().requires_grad_(True)
    pr = prpc.float().requires_grad_(True)
    out = F._fused_eager(qkvs.float(), pf, pr, ea, csr, heads)
    (out * gout.float()).sum().backward()
    n, h = qkvs.shape[0], qkvs.shape[1] // 4
    q, k, v, skip = qkvs.float().split(h, dim=1)
    e = (pifc.float()[ea[:, 0]] + prpc.float()[ea[:, 1]]).requires_grad_(True)
    deg = (csr[0][1:] - csr[0][:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n), deg)
    o = ref.edge_attention(q, k, v, e, torch.stack([csr[1].long(), dst]), n,
                           skip, heads=heads)
    (de,) = torch.autograd.grad((o * gout.float()).sum(), e)
    abs_p, abs_r = _oracle(ea[:, 0], ea[:, 1], pifc.shape[0], prpc.shape[0],
                           de.abs())
    return pf.grad, pr.grad, abs_p, abs_r


@gpu
@needs_gpu
@pytest.mark.parametrize("heads", [1, 4])
def test_attention_backward_table_grads(heads):
    csr, ea, qkvs, pifc, prpc, gout = _attention_case()
    want_p, want_r, abs_p, abs_r = _attention_reference(heads)
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    pf = pifc.to(DEV).requires_grad_(True)
    pr = prpc.to(DEV).requires_grad_(True)
    out = F.edge_attention_fused(qkvs.to(DEV), pf, pr, ea_d, csr_d,
                                 out16=True, heads=heads)
    out.backward(gout.to(DEV))
    assert pf.grad.dtype == torch.bfloat16 and pf.grad.shape == pifc.shape
    assert pr.grad.dtype == torch.bfloat16 and pr.grad.shape == prpc.shape
    # the new op ran: its plan is cached under this edge_attr
    assert any(k[0] == "edge_table" and k[1] == ea_d.data_ptr()
               for k in F._GROUP_CACHE if isinstance(k[0], str))
    for name, got, want, extra in (("dP_ifc", pf.grad, want_p, abs_p),
                                   ("dP_rpc", pr.grad, want_r, abs_r)):
        got = got.float().cpu()
        err = float((got - want).abs().max())
        print(f"  {name}: max abs err {err:.3e} "
              f"(max |ref| {float(want.abs().max()):.3e})")
        bound = (BF16_TOL["atol"] + BF16_TOL["rtol"] * want.abs()
                 + extra * 2.0 ** -9)
        assert not bool(((got - want).abs() > bound).any()), (name, err)


@gpu
@needs_gpu
def test_captured_training_step_large_vocab():
    """2 layers, H=256, bf16, interface table of 2048 rows: after the
    warm-up the plan is a cache hit, so the step captures (a sync would
    abort the capture) and two replays give the two eager steps' losses."""
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train.capture import GraphStepper
    from pertgnn.train.optim import FusedAdam

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2,
                                                       device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              2047, stats["rpc_max"], 256, 2, 0.0).to(DEV)
    model.train()
    try:
        F.set_gemm_precision("bf16")
        opt = FusedAdam(model.parameters(), lr=1e-3)
        stepper = GraphStepper(model, opt, None, None, 0.5, DEV, batches)
        snap = stepper._snapshot()
        eager = []
        for _ in range(2):
            stepper.acc.zero_()
            stepper._full_step(0)
            eager.append(float(stepper.acc[0]) / batches[0].num_graphs)
        stepper._restore(snap)
        ea = batches[0].edge_attr
        assert any(k[0] == "edge_table" and k[1] == ea.data_ptr()
                   for k in F._GROUP_CACHE if isinstance(k[0], str))
        assert stepper.capture() == "full"
        replay = []
        for _ in range(2):
            total, _, n = stepper.run_epoch_sums()
            replay.append(total / n)
        print("eager", eager, "replayed", replay)
        assert all(torch.isfinite(torch.tensor(replay)))
        for a, b in zip(replay, eager):
            assert abs(a - b) <= BF16_TOL["atol"] + BF16_TOL["rtol"] * abs(b)
    finally:
        F.set_gemm_precision("fp32")
