"""The act16 attention backward applies the BN backward of the BN that follows
the attention (``edge_attn_bn_bwd16`` / ``F.edge_attention_fused_bn_relu``).

Everything here is a bit-for-bit comparison against the unfused composition
``bn_relu_bwd16`` (or ``bn_bwd_apply16`` for the count-pointer path) followed
by ``edge_attn_fused_bwd``: the fused row kernel forms the same bf16 value the
stand-alone BN kernel stores as ``dx`` (one shared helper with its contraction
pinned), and from there on both paths run the same instructions on the same
bits.  The slab combine of the BN partials and both attention backward kernels
are free of atomics, so the unfused path repeats itself bit for bit.

The graphs: node 0 has no in-edges, node 1 no out-edges, node 2 has in-degree
70 and node 3 out-degree 70 (more than any lanes-per-head or lanes-per-row, so
the alpha/dal slot striding wraps), every other node a few random in-edges.
n = 11 and 67 are no multiples of the 8 rows per block (two rows per wave at
both widths) and 67 leaves a partial last wave; at n = 1 the one node carries 70
self-loops (in- and out-degree 70), and the E = 0 case has the nodes without
edges.
"""
import functools

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

VI, VR = 37, 5
HUB = 70


def _ext():
    import pertgnn._C as C
    return C


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
        # node 2: in-degree 70, from the ordinary nodes 4..n-1
        s = torch.randint(4, n, (HUB,), generator=g).tolist()
        src += s
        dst += [2] * HUB
        # node 3: out-degree 70, to the ordinary nodes
        d = torch.randint(4, n, (HUB,), generator=g).tolist()
        src += [3] * HUB
        dst += d
        for i in range(4, n):
            deg = 1 + i % 3
            s = torch.randint(4, n, (deg,), generator=g).tolist()
            src += s
            dst += [i] * deg
        # node 1 receives, and never sends
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


@functools.lru_cache(maxsize=None)
def _case(h, heads, n, dropout_p, edges=True):
    """Operands of one backward, taken from the real forwards (attention with
    out16, then the training BN+ReLU(+dropout)), and the unfused backward of
    them; computed once per case and never written to."""
    C = _ext()
    csr, ea = _graph(n, edges)
    g = torch.Generator().manual_seed(1000 * h + 100 * heads + n)
    bf = torch.bfloat16
    qkvs = torch.randn(n, 4 * h, generator=g).to(bf).to(DEV)
    pifc = torch.randn(VI, h, generator=g).to(bf).to(DEV)
    prpc = torch.randn(VR, h, generator=g).to(bf).to(DEV)
    gout = torch.randn(n, h, generator=g).to(bf).to(DEV)
    gamma = (torch.rand(h, generator=g) * 1.5 + 0.5).to(DEV)
    beta = (torch.randn(h, generator=g) * 0.5).to(DEV)
    rm = torch.zeros(h, device=DEV)
    rv = torch.ones(h, device=DEV)
    seed = torch.tensor([12345 + n], dtype=torch.int64, device=DEV)
    x, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea, csr[0], csr[1],
                                     True, heads)
    y, mean, invstd, mask = C.bn_relu_fwd16(x, gamma, beta, rm, rv, 0.1, 1e-5,
                                            True, True, dropout_p, seed)
    assert mask.dtype == torch.uint8 and mask.shape == (n, h // 8)
    keep_inv = 1.0 / (1.0 - dropout_p) if dropout_p > 0 else 1.0
    attn = (qkvs, pifc, prpc, ea, alpha, *csr, heads)
    dx, dgamma, dbeta = C.bn_relu_bwd16(gout, x, gamma, mean, invstd, mask,
                                        True, keep_inv)
    dqkvs, de = C.edge_attn_fused_bwd(dx, *attn)
    torch.cuda.synchronize()
    return dict(g=gout, x=x, mask=mask, gamma=gamma, mean=mean, invstd=invstd,
                keep_inv=keep_inv, attn=attn, dx=dx,
                want=(dqkvs, de, dgamma, dbeta))


def _fused(c, *partials):
    return _ext().edge_attn_bn_bwd16(
        c["g"], c["x"], c["mask"], c["gamma"], c["mean"], c["invstd"],
        c["keep_inv"], *c["attn"], *partials)


def _assert_equal(got, want, what):
    for name, a, b in zip(("dqkvs", "de", "dgamma", "dbeta"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        ndiff = int((a != b).sum())
        assert torch.equal(a, b), (what, name, ndiff, a.numel())


@gpu
@needs_gpu
@pytest.mark.parametrize("dropout_p", [0.0, 0.25])
@pytest.mark.parametrize("n", [1, 11, 67])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("h", [256, 512])
def test_fused_equals_unfused(h, heads, n, dropout_p):
    c = _case(h, heads, n, dropout_p)
    h4 = 4 * h
    # the inputs are real: finite, part of the mask clear, dskip is the dx
    assert bool(torch.isfinite(c["dx"].float()).all())
    got = _fused(c)
    torch.cuda.synchronize()
    assert torch.equal(got[0].view(n, h4)[:, 3 * h:], c["dx"])
    _assert_equal(got, c["want"], (h, heads, n, dropout_p))


@gpu
@needs_gpu
@pytest.mark.parametrize("h,heads", [(256, 1), (512, 4)])
def test_no_edges(h, heads):
    c = _case(h, heads, 11, 0.25, edges=False)
    assert c["attn"][3].shape[0] == 0
    got = _fused(c)
    torch.cuda.synchronize()
    assert got[1].shape == (0, h)
    _assert_equal(got, c["want"], (h, heads, "E=0"))


@gpu
@needs_gpu
@pytest.mark.parametrize("h,heads", [(256, 1), (256, 4), (512, 1), (512, 4)])
def test_count_pointer_path(h, heads):
    """Sync-BN form: [2h+1] partials that carry the global count (here twice
    the local sums over three times the local rows), dgamma/dbeta from the
    local partials; against bn_bwd_apply16 followed by the attention backward."""
    C = _ext()
    n = 67
    c = _case(h, heads, n, 0.25)
    local = C.bn_bwd_partials16(c["g"], c["x"], c["mask"], c["mean"],
                                c["invstd"], True, c["keep_inv"])
    assert local.shape == (2 * h + 1,) and float(local[-1]) == n
    glob = local * 2.0
    glob[-1] = 3.0 * n
    dx, dgamma, dbeta = C.bn_bwd_apply16(
        c["g"], c["x"], c["mask"], c["mean"], c["invstd"], c["gamma"], glob,
        local, True, c["keep_inv"])
    assert not torch.equal(dx, c["dx"]), "the global count changed nothing"
    dqkvs, de = C.edge_attn_fused_bwd(dx, *c["attn"])
    got = _fused(c, glob, local)
    torch.cuda.synchronize()
    _assert_equal(got, (dqkvs, de, dgamma, dbeta), (h, heads, "count_ptr"))


@gpu
@needs_gpu
def test_binding_rejects_what_it_does_not_cover():
    C = _ext()
    c = _case(256, 1, 11, 0.0)
    args = [c["g"], c["x"], c["mask"], c["gamma"], c["mean"], c["invstd"],
            c["keep_inv"], *c["attn"]]
    with pytest.raises(RuntimeError, match="keep mask"):
        C.edge_attn_bn_bwd16(*args[:2], c["x"], *args[3:])
    with pytest.raises(RuntimeError, match="bf16"):
        C.edge_attn_bn_bwd16(c["g"].float(), *args[1:])
    with pytest.raises(RuntimeError, match="keep mask"):
        C.edge_attn_bn_bwd16(*args[:2], c["mask"][:5].contiguous(), *args[3:])
    torch.cuda.synchronize()
    _assert_equal(_fused(c), c["want"], "after the rejected calls")


class _TwoEqualRanks:
    """Stand-in for the sync-BN comm on one process: the all-reduce of two
    ranks holding the same shard (sums and the row count double)."""
    distributed = True

    def all_reduce_(self, t):
        t.mul_(2.0)
        return t


@gpu
@needs_gpu
@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_autograd_function_matches_the_two_functions(heads, sync, monkeypatch):
    """F.edge_attention_fused_bn_relu against F.edge_attention_fused followed
    by F.batchnorm_relu on the same leaves (dropout 0): output, running
    statistics and all five gradients bit-equal, with a local BN and through
    the sync-BN branch (partials -> all_reduce_ -> the count pointer).
    PERTGNN_DETERMINISTIC=1 puts the P-table gradients on the fixed-order
    list sums, so the composition repeats itself bit for bit."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    h, n = 256, 67
    c = _case(h, heads, n, 0.0)
    qkvs0, pifc0, prpc0, ea = c["attn"][:4]
    csr = c["attn"][5:10]
    comm = _TwoEqualRanks() if sync else None
    res = []
    for fused in (True, False):
        leaves = [t.detach().clone().requires_grad_(True)
                  for t in (qkvs0, pifc0, prpc0, c["gamma"],
                            torch.zeros_like(c["gamma"]))]
        qkvs, pifc, prpc, gamma, beta = leaves
        rm = torch.zeros(h, device=DEV)
        rv = torch.ones(h, device=DEV)
        if fused:
            y = F.edge_attention_fused_bn_relu(
                qkvs, pifc, prpc, ea, csr, gamma, beta, rm, rv, 0.1, 1e-5,
                heads=heads, comm=comm, dropout_p=0.0)
        else:
            x = F.edge_attention_fused(qkvs, pifc, prpc, ea, csr, out16=True,
                                       heads=heads)
            y = F.batchnorm_relu(x, gamma, beta, rm, rv, 0.1, 1e-5, True,
                                 fuse_relu=True, comm=comm, out16=True)
        y.backward(c["g"])
        torch.cuda.synchronize()
        res.append([y.detach(), rm, rv] + [t.grad for t in leaves])
    names = ["y", "running_mean", "running_var", "dqkvs", "dpifc", "dprpc",
             "dgamma", "dbeta"]
    for name, a, b in zip(names, *res):
        assert a is not None and b is not None, name
        assert torch.equal(a, b), (name, heads, sync)
    assert bool(res[0][3].float().abs().max() > 0)


# ---------------------------------------------------------------------------
# model level (3 layers, H = 256, bf16), built as tests/test_ptable_grouped.py
# builds its model
# ---------------------------------------------------------------------------

def _gpu_model(heads):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2, device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0, heads=heads).to(DEV)
    return model, batches


def _model_step(model, b):
    model.zero_grad(set_to_none=True)
    gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                   b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                   num_graphs=b.num_graphs)
    loss = F.quantile_loss(b.y, gp.flatten(), 0.5)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    return loss.detach().clone(), gp.detach().clone(), lp.detach().clone(), grads


@gpu
@needs_gpu
@pytest.mark.parametrize("heads", [1, 4])
def test_model_switch_on_off_bitwise(heads, monkeypatch):
    """Same model, same batch, with and without PERTGNN_NO_BN_ATTN_FUSE=1
    under PERTGNN_DETERMINISTIC=1 (every kernel then repeats itself bit for
    bit): loss, both predictions and every parameter gradient are bit-equal,
    and the fused Function really ran for the two non-final convs."""
    model, batches = _gpu_model(heads)
    model.train()
    b = batches[0]
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    calls = []
    real = F.edge_attention_fused_bn_relu

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    try:
        F.set_gemm_precision("bf16")
        monkeypatch.setattr(F, "edge_attention_fused_bn_relu", spy)
        monkeypatch.delenv("PERTGNN_NO_BN_ATTN_FUSE", raising=False)
        loss_f, gp_f, lp_f, grads_f = _model_step(model, b)
        assert len(calls) == 2, "the fused path did not run"
        monkeypatch.setenv("PERTGNN_NO_BN_ATTN_FUSE", "1")
        loss_u, gp_u, lp_u, grads_u = _model_step(model, b)
        assert len(calls) == 2, "PERTGNN_NO_BN_ATTN_FUSE=1 still fused"
        torch.cuda.synchronize()
    finally:
        F.set_gemm_precision("fp32")
    assert torch.equal(loss_f, loss_u)
    assert torch.equal(gp_f, gp_u) and torch.equal(lp_f, lp_u)
    assert grads_f.keys() == grads_u.keys() and len(grads_f) > 10
    for name in grads_f:
        assert bool(torch.isfinite(grads_f[name]).all()), name
        assert torch.equal(grads_f[name], grads_u[name]), name
