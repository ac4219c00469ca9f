"""Argument checks of the linear, BatchNorm and fused-attention bindings.

Each rejected call raises a RuntimeError that names the binding, before
anything is launched (the device still synchronizes afterwards).  Every
offending tensor is LARGER than the op expects, never smaller, so code
without the check would still have stayed inside its buffers.  One valid call
per family at the same shapes, against torch in float64 at the tolerances
test_gpu_ops.py uses for that family, keeps a check that rejects everything
from passing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pertgnn.data.collate import build_csr
    from pertgnn.ops import reference as ref
    from pertgnn.ops.backend import require_ext
else:
    pytest.skip("no GPU available", allow_module_level=True)

DEV = torch.device("cuda:0")
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
M, N, K = 8, 16, 24


def _rand(*shape, seed, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).to(dtype)


def _rejects(name, *args):
    C = require_ext()
    with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
        getattr(C, name)(*args)
    torch.cuda.synchronize()


def _d(t):
    """float64 on the CPU: where every reference is computed"""
    return t.detach().cpu().to(F64)


def _close(got, want, atol, rtol, what):
    got, want = _d(got), _d(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    assert bool((err <= atol + rtol * want.abs()).all()), (what, err.max().item())


# --- linear -----------------------------------------------------------------

# (binding, dtype of x) of the five forwards
FORWARDS = [("linear_fwd", F32), ("linear_fwd_bf16", F32),
            ("linear_fwd_fp16", F32), ("linear_fwd_bf16_o16", F32),
            ("linear_fwd_a16o16", BF16)]


@pytest.mark.parametrize("name,xdt", FORWARDS)
def test_forward_rejects_wide_weight(name, xdt):
    x = _rand(M, K, seed=1, dtype=xdt)
    w = _rand(N, K + 8, seed=2)  # [16, 32]: 32 columns against x's 24
    _rejects(name, x, w, _rand(N, seed=3))


# (binding, dtype of g, arguments after (g, w))
DGRADS = [("linear_dgrad", F32, (0,)), ("linear_dgrad", F32, (1,)),
          ("linear_dgrad", F32, (2,)), ("linear_dgrad16", BF16, ()),
          ("linear_dgrad16_o16", BF16, ())]


@pytest.mark.parametrize("name,gdt,rest", DGRADS)
def test_dgrad_rejects_wide_gradient(name, gdt, rest):
    g = _rand(M, K, seed=4, dtype=gdt)  # [8, 24]: 24 columns against w's 16 rows
    w = _rand(N, K, seed=2)
    _rejects(name, g, w, *rest)


@pytest.mark.parametrize("name", ["linear_bwd", "linear_bwd_bf16",
                                  "linear_bwd_fp16"])
def test_bwd_rejects_wide_gradient(name):
    g = _rand(M, K, seed=4)
    _rejects(name, g, _rand(M, K, seed=1), _rand(N, K, seed=2), True)


# (binding, dtype of g, dtype of x, arguments after (g, x))
WGRADS = [("linear_wgrad", F32, F32, (True, 0)),
          ("linear_wgrad", F32, F32, (True, 1)),
          ("linear_wgrad", F32, F32, (True, 2)),
          ("linear_wgrad16", BF16, F32, (True,)),
          ("linear_wgrad16_b16", BF16, BF16, (True,))]


@pytest.mark.parametrize("name,gdt,xdt,rest", WGRADS)
def test_wgrad_rejects_tall_gradient(name, gdt, xdt, rest):
    g = _rand(2 * M, N, seed=5, dtype=gdt)  # [16, 16]: 16 rows against x's 8
    x = _rand(M, K, seed=1, dtype=xdt)
    _rejects(name, g, x, *rest)


def _bf(t):
    return _d(t.to(BF16))


def _half(t):
    return _d(t.to(torch.float16))


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_linear_f32io_valid(prec):
    """fp32 in and out; the reference rounds the operands as the matrix cores
    take them (test_gemm_parity / test_gemm_bf16_parity / test_gemm_fp16_parity
    and their tolerances)."""
    C = require_ext()
    sfx = ["", "_bf16", "_fp16"][prec]
    rnd = [_d, _bf, _half][prec]
    nt, tn, db_tol = [((1e-3, 1e-4), (5e-2, 1e-3), (1e-2, 1e-3)),
                      ((1e-2, 1e-2), (0.5, 1e-2), (0.5, 1e-2)),
                      ((1e-2, 1e-2), (0.5, 1e-2), (0.5, 1e-2))][prec]
    x, w, b = _rand(M, K, seed=1), _rand(N, K, seed=2), _rand(N, seed=3)
    g = _rand(M, N, seed=6)
    y = getattr(C, "linear_fwd" + sfx)(x, w, b)
    dx, dw, db = getattr(C, "linear_bwd" + sfx)(g, x, w, True)
    dx2 = C.linear_dgrad(g, w, prec)
    dw2, db2 = C.linear_wgrad(g, x, True, prec)
    torch.cuda.synchronize()
    _close(y, rnd(x) @ rnd(w).t() + _d(b), *nt, "y")
    for got in (dx, dx2):
        _close(got, rnd(g) @ rnd(w), *nt, "dx")
    for got in (dw, dw2):
        _close(got, rnd(g).t() @ rnd(x), *tn, "dw")
    for got in (db, db2):
        _close(got, _d(g).sum(0), *db_tol, "db")
    if prec < 2:
        _close(getattr(C, "gemm_nt" + sfx)(x, w), rnd(x) @ rnd(w).t(), *nt,
               "gemm_nt")
        _close(getattr(C, "gemm_nn" + sfx)(g, w), rnd(g) @ rnd(w), *nt,
               "gemm_nn")
        _close(getattr(C, "gemm_tn" + sfx)(g, x), rnd(g).t() @ rnd(x), *tn,
               "gemm_tn")


@pytest.mark.parametrize("a16", [False, True])
def test_linear_16_valid(a16):
    """o16 (fp32 x) and a16 (bf16 x): bf16 y and g, bf16 operands in the
    matrix cores; tolerances of test_glds_odd_m_tail_parity."""
    C = require_ext()
    x = _rand(M, K, seed=1, dtype=BF16 if a16 else F32)
    w, b = _rand(N, K, seed=2), _rand(N, seed=3)
    g = _rand(M, N, seed=6, dtype=BF16)
    if a16:
        y = C.linear_fwd_a16o16(x, w, b)
        y2, _ = C.linear_fwd_a16o16_wt(x, w, b)
        dx = C.linear_dgrad16_o16(g, w)
        dw, db = C.linear_wgrad16_b16(g, x, True)
        assert torch.equal(y, y2)
    else:
        y = C.linear_fwd_bf16_o16(x, w, b)
        dx = C.linear_dgrad16(g, w)
        dw, db = C.linear_wgrad16(g, x, True)
    torch.cuda.synchronize()
    assert y.dtype == BF16 and dx.dtype == (BF16 if a16 else F32)
    assert dw.dtype == F32 and db.dtype == F32
    _close(y, _bf(x) @ _bf(w).t() + _d(b), 0.05, 1e-2, "y")
    _close(dx, _bf(g) @ _bf(w), 0.3, 1e-2, "dx")
    _close(dw, _bf(g).t() @ _bf(x), 0.5, 1e-3, "dw")
    _close(db, _bf(g).sum(0), 0.2, 1e-3, "db")


# --- BatchNorm --------------------------------------------------------------

BN_N, BN_H = 8, 64
BN_TOL = (5e-3, 1e-3)  # test_batchnorm_relu_parity


def _bn_inputs(dtype):
    x = (_rand(BN_N, BN_H, seed=7) * 3 + 1).to(dtype)
    gamma = _rand(BN_H, seed=8).abs() + 0.5
    beta = _rand(BN_H, seed=9)
    g = _rand(BN_N, BN_H, seed=10).to(dtype)
    return x, gamma, beta, g


def _bn_fwd_args(x, gamma, beta):
    """training forward with ReLU, no dropout (an empty seed)"""
    rm = torch.zeros(BN_H, device=DEV)
    rv = torch.ones(BN_H, device=DEV)
    seed = torch.empty(0, dtype=torch.int64, device=DEV)
    return (x, gamma, beta, rm, rv, 0.1, 1e-5, True, True, 0.0, seed)


def _bn_fwd(C, name, x, gamma, beta):
    return getattr(C, name)(*_bn_fwd_args(x, gamma, beta))


def test_bn16_rejects_fp32_activations():
    C = require_ext()
    x, gamma, beta, g = _bn_inputs(F32)  # 4-byte elements where 2 are expected
    _rejects("bn_relu_fwd16", *_bn_fwd_args(x, gamma, beta))
    y, mean, invstd = _bn_fwd(C, "bn_relu_fwd", x, gamma, beta)
    _rejects("bn_bwd_partials16", g, x, y, mean, invstd, True, 1.0)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bn_valid(dtype):
    """Forward and backward partials under the name that takes the dtype.
    The statistics and partial sums are fp32 outputs in both; the bf16 y
    carries its own rounding on top, half an ulp = 2^-9 relative."""
    C = require_ext()
    sfx = "16" if dtype == BF16 else ""
    x, gamma, beta, g = _bn_inputs(dtype)
    out = _bn_fwd(C, "bn_relu_fwd" + sfx, x, gamma, beta)
    assert len(out) == (4 if dtype == BF16 else 3)
    y, mean, invstd = out[:3]
    part = getattr(C, "bn_bwd_partials" + sfx)(g, x, y, mean, invstd, True, 1.0)
    torch.cuda.synchronize()
    assert y.dtype == dtype and mean.dtype == F32 and part.dtype == F32
    xd = _d(x)
    mu = xd.mean(0)
    istd = (xd.var(0, unbiased=False) + 1e-5).rsqrt()
    xhat = (xd - mu) * istd
    want_y = torch.relu(xhat * _d(gamma) + _d(beta))
    atol, rtol = BN_TOL
    _close(mean, mu, atol, rtol, "mean")
    _close(invstd, istd, atol, rtol, "invstd")
    _close(y, want_y, atol, rtol + (2.0 ** -9 if dtype == BF16 else 0.0), "y")
    # the partials of what the op was given: its own y, mean and invstd
    gm = _d(g) * (_d(y) > 0)
    xh = (xd - _d(mean)) * _d(invstd)
    want = torch.cat([gm.sum(0), (gm * xh).sum(0),
                      torch.tensor([float(BN_N)], dtype=F64)])
    _close(part, want, atol, rtol, "partials")


# --- fused attention --------------------------------------------------------

def _attn_case():
    n, h = 4, 64
    ei = torch.tensor([[0, 1, 2, 3, 1, 0], [1, 1, 2, 0, 3, 3]])  # 6 edges
    perm, *csr = build_csr(ei, n)
    ei = ei.index_select(1, perm)
    ea = torch.tensor([[0, 1], [1, 0], [2, 2], [0, 0], [1, 2], [2, 1]])
    qkvs = _rand(n, 4 * h, seed=11)
    pifc, prpc = _rand(3, h, seed=12), _rand(3, h, seed=13)
    g = _rand(n, h, seed=14)
    return (n, h, ei.to(DEV), qkvs, pifc, prpc, ea.to(DEV),
            [t.to(DEV) for t in csr], g)


def test_attn_bwd_rejects_long_row_ptr():
    C = require_ext()
    n, h, ei, qkvs, pifc, prpc, ea, csr, g = _attn_case()
    _, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea, csr[0], csr[1],
                                     False)
    long_row_ptr = torch.cat([csr[0], csr[0][-1:]])  # n + 2 entries
    _rejects("edge_attn_fused_bwd", g, qkvs, pifc, prpc, ea, alpha,
             long_row_ptr, *csr[1:])


def test_attn_valid():
    """edge_attn_fused_fwd / _bwd against autograd through the float64
    reference; tolerances of test_edge_attention_parity."""
    C = require_ext()
    n, h, ei, qkvs, pifc, prpc, ea, csr, g = _attn_case()
    out, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea, csr[0], csr[1],
                                       False)
    dqkvs, de = C.edge_attn_fused_bwd(g, qkvs, pifc, prpc, ea, alpha, *csr)
    torch.cuda.synchronize()
    qd = _d(qkvs).requires_grad_(True)
    eac = ea.cpu()
    ed = (_d(pifc)[eac[:, 0]] + _d(prpc)[eac[:, 1]]).requires_grad_(True)
    q, k, v, skip = qd.split(h, dim=1)
    want = ref.edge_attention(q, k, v, ed, ei.cpu(), n, skip)
    want.backward(_d(g))
    _close(out, want.detach(), 2e-4, 1e-4, "out")
    _close(dqkvs, qd.grad, 5e-4, 1e-3, "dqkvs")
    _close(de, ed.grad, 5e-4, 1e-3, "de")
