"""GPU tests of the wide-load BatchNorm reductions and the bit-packed ReLU
keep mask (bf16 activation streams).

Fast-path shapes (h % 8 == 0 and 256 % (h/8) == 0) run the 8-channels-per-
lane kernels; h = 40 and h = 36 must stay on the pair-per-thread kernels.
Bounds are derived, not measured: u = 2**-24 is the fp32 unit roundoff and
(n + 4) * u * sum|term| the recursive-summation bound (n - 1 additions plus
the roundings that form each term).

Run on an MI355X box:  python -m pytest tests/test_bn_wide.py -m gpu -q
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pertgnn.ops import functional as F
    from pertgnn.ops.backend import require_ext
else:
    pytest.skip("no GPU available", allow_module_level=True)


DEV = torch.device("cuda:0")
U32 = 2.0 ** -24

NS = [1, 7, 63, 1000, 4099]
HS = [256, 512, 64, 40, 36]
SHAPES = [(n, h) for h in HS for n in NS]
# (n, h, PERTGNN_BN_BLOCKS): 3 blocks, and 512 blocks >> 63 rows
BLOCK_CASES = [(63, 256, "3"), (63, 256, "512")]


def _wide(h):
    return h % 8 == 0 and 256 % (h // 8) == 0


_CACHE = {}


def _inputs(n, h):
    """bf16 x and g, fp32 affine parameters — built once per shape."""
    key = (n, h)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(1000 * h + n)
        x = (torch.randn(n, h, generator=gen) * 3 + 1).to(torch.bfloat16)
        g = torch.randn(n, h, generator=gen).to(torch.bfloat16)
        gamma = torch.rand(h, generator=gen) + 0.5
        beta = torch.randn(h, generator=gen) * 0.5
        _CACHE[key] = tuple(t.to(DEV) for t in (x, g, gamma, beta))
    return _CACHE[key]


def _fwd(C, x, gamma, beta, relu=True, dropout_p=0.0, training=True):
    h = x.shape[1]
    rm = torch.zeros(h, device=DEV)
    rv = torch.ones(h, device=DEV)
    seed = (torch.full((1,), 12345, dtype=torch.int64, device=DEV)
            if dropout_p > 0 else torch.empty(0, dtype=torch.int64, device=DEV))
    out = C.bn_relu_fwd16(x, gamma, beta, rm, rv, 0.1, 1e-5, training, relu,
                          dropout_p, seed)
    return out, rm, rv


def _unpack(mask, h):
    """uint8 [n, h/8] -> bool [n, h]; bit u of byte (r, c/8) is channel c+u."""
    bits = (mask.long().unsqueeze(-1) >> torch.arange(8, device=mask.device)) & 1
    return bits.reshape(mask.shape[0], h).bool()


def _bf16_ulp(ref):
    """spacing of bf16 (8 significant bits) at the magnitude of ref"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=ref.dtype, device=ref.device), e - 7)


def _check_stats(C, n, h):
    x = _inputs(n, h)[0]
    p = C.bn_stats(x).double()
    xd = x.double()
    assert p[2 * h].item() == n
    bound_s = (n + 4) * U32 * xd.abs().sum(0)
    bound_q = (n + 4) * U32 * (xd * xd).sum(0)
    err_s = (p[:h] - xd.sum(0)).abs()
    err_q = (p[h:2 * h] - (xd * xd).sum(0)).abs()
    print(f"stats n={n} h={h}: max err/bound sum "
          f"{(err_s / bound_s.clamp_min(1e-300)).max().item():.3f} sumsq "
          f"{(err_q / bound_q.clamp_min(1e-300)).max().item():.3f}")
    assert (err_s <= bound_s).all()
    assert (err_q <= bound_q).all()


# 1. forward statistics against float64 on the bf16-rounded x
@pytest.mark.parametrize("n,h", SHAPES)
def test_stats_bound(n, h):
    C = require_ext()
    _check_stats(C, n, h)


@pytest.mark.parametrize("n,h,blocks", BLOCK_CASES)
def test_stats_bound_block_override(n, h, blocks, monkeypatch):
    C = require_ext()
    monkeypatch.setenv("PERTGNN_BN_BLOCKS", blocks)
    _check_stats(C, n, h)


# 2. mask content: bit == ~(y <= 0) on the returned bf16 y, with and
# without fused dropout; eval mode, relu=False and other shapes write none
@pytest.mark.parametrize("dropout_p", [0.0, 0.3])
@pytest.mark.parametrize("n,h", [(n, h) for h in (256, 512, 64) for n in NS])
def test_mask_content(n, h, dropout_p):
    C = require_ext()
    x, _, gamma, beta = _inputs(n, h)
    (y, _, _, mask), _, _ = _fwd(C, x, gamma, beta, True, dropout_p)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (n, h // 8)
    assert torch.equal(_unpack(mask, h), ~(y <= 0))
    if dropout_p > 0 and n >= 1000:  # dropout really ran
        (y0, _, _, _), _, _ = _fwd(C, x, gamma, beta, True, 0.0)
        extra = ((y == 0).float().mean() - (y0 == 0).float().mean()).item()
        assert extra > 0.1


@pytest.mark.parametrize("h", [256, 40, 36])
def test_no_mask_when_not_needed(h):
    C = require_ext()
    x, _, gamma, beta = _inputs(63, h)
    for relu, training in [(False, True), (True, False)]:
        out, _, _ = _fwd(C, x, gamma, beta, relu, 0.0, training)
        assert out[3].numel() == 0
    out, _, _ = _fwd(C, x, gamma, beta, True, 0.0, True)
    assert (out[3].numel() > 0) == _wide(h)


def _bwd_all(C, g, x, ym, mean, invstd, gamma, relu, keep_inv=1.0):
    """fused and sync-BN backward entry points on the same operands"""
    h = x.shape[1]
    dx, dgamma, dbeta = C.bn_relu_bwd16(g, x, gamma, mean, invstd, ym, relu,
                                        keep_inv)
    part = C.bn_bwd_partials16(g, x, ym, mean, invstd, relu, keep_inv)
    dx2, dgamma2, dbeta2 = C.bn_bwd_apply16(g, x, ym, mean, invstd, gamma,
                                            part, part, relu, keep_inv)
    assert part[2 * h].item() == x.shape[0]
    return dx, dgamma, dbeta, part, dx2, dgamma2, dbeta2


# 3. mask == y: bitwise-equal backward in deterministic mode, relu on; with
# relu off neither y nor the mask may matter (poisoned with zeros)
@pytest.mark.parametrize("n,h", [(n, h) for h in (256, 512, 64) for n in NS])
def test_mask_equals_y(n, h, monkeypatch):
    C = require_ext()
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    x, g, gamma, beta = _inputs(n, h)
    (y, mean, invstd, mask), _, _ = _fwd(C, x, gamma, beta, True, 0.3)
    keep_inv = 1.0 / 0.7
    with_y = _bwd_all(C, g, x, y, mean, invstd, gamma, True, keep_inv)
    with_m = _bwd_all(C, g, x, mask, mean, invstd, gamma, True, keep_inv)
    for a, b in zip(with_y, with_m):
        assert torch.equal(a, b)
    # fused and sync entry points agree too
    assert torch.equal(with_m[0], with_m[4])
    assert torch.equal(with_m[1], with_m[5])
    assert torch.equal(with_m[2], with_m[6])

    plain = _bwd_all(C, g, x, y, mean, invstd, gamma, False)
    zero_y = _bwd_all(C, g, x, torch.zeros_like(y), mean, invstd, gamma, False)
    zero_m = _bwd_all(C, g, x, torch.zeros_like(mask), mean, invstd, gamma,
                      False)
    for a, b, c in zip(plain, zero_y, zero_m):
        assert torch.equal(a, b)
        assert torch.equal(a, c)


@pytest.mark.parametrize("h", [40, 36])
def test_relu_off_ignores_y_old_kernels(h, monkeypatch):
    C = require_ext()
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    x, g, gamma, beta = _inputs(63, h)
    (y, mean, invstd, _), _, _ = _fwd(C, x, gamma, beta, False)
    plain = _bwd_all(C, g, x, y, mean, invstd, gamma, False)
    zero_y = _bwd_all(C, g, x, torch.zeros_like(y), mean, invstd, gamma, False)
    for a, b in zip(plain, zero_y):
        assert torch.equal(a, b)


def _check_bwd(C, n, h, relu):
    """4. backward against float64 on the same bf16 g/x and fp32 statistics.

    Partial sums: (n + 4) u sum|term|.  dx = gamma invstd (gm - S1/n -
    xhat S2/n) is stored as bf16: one bf16 ulp of the reference value, plus
    the partial-sum bounds e1, e2 carried through gamma invstd (e1 + |xhat|
    e2) / n, plus 8 u on the magnitudes of the three terms for the fp32
    elementwise arithmetic (1/n, xhat, products, two subtractions)."""
    x, g, gamma, beta = _inputs(n, h)
    (y, mean, invstd, mask), _, _ = _fwd(C, x, gamma, beta, relu)
    ym = mask if mask.numel() else y
    dx, dgamma, dbeta, part, dx2, _, _ = _bwd_all(C, g, x, ym, mean, invstd,
                                                  gamma, relu)
    gd, xd = g.double(), x.double()
    md, isd, gad = mean.double(), invstd.double(), gamma.double()
    gm = torch.where(y <= 0, torch.zeros_like(gd), gd) if relu else gd
    xhat = (xd - md) * isd
    s1, s2 = gm.sum(0), (gm * xhat).sum(0)
    e1 = (n + 4) * U32 * gm.abs().sum(0)
    e2 = (n + 4) * U32 * (gm * xhat).abs().sum(0)
    for got1, got2 in ((part[:h], part[h:2 * h]), (dbeta, dgamma)):
        assert ((got1.double() - s1).abs() <= e1).all()
        assert ((got2.double() - s2).abs() <= e2).all()
    ref = gad * isd * (gm - s1 / n - xhat * s2 / n)
    tol = (_bf16_ulp(ref)
           + gad * isd * (e1 + xhat.abs() * e2) / n
           + 8 * U32 * gad * isd * (gm.abs() + s1.abs() / n
                                    + (xhat * s2).abs() / n))
    for d in (dx, dx2):
        err = (d.double() - ref).abs()
        print(f"bwd n={n} h={h} relu={relu}: max err/tol "
              f"{(err / tol).max().item():.3f}")
        assert (err <= tol).all()


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("n,h", SHAPES)
def test_backward_bound(n, h, relu):
    C = require_ext()
    _check_bwd(C, n, h, relu)


@pytest.mark.parametrize("n,h,blocks", BLOCK_CASES)
def test_backward_bound_block_override(n, h, blocks, monkeypatch):
    C = require_ext()
    monkeypatch.setenv("PERTGNN_BN_BLOCKS", blocks)
    _check_bwd(C, n, h, True)


def _autograd_run(n, h, device, relu=True):
    """F.batchnorm_relu forward+backward; upstream grad is a fixed bf16-exact
    weight so both sides differentiate the same function of y."""
    x, g, gamma, beta = _inputs(n, h)
    bf = device.type == "cuda"
    xx = (x if bf else x.float()).detach().to(device).requires_grad_(True)
    ga = gamma.detach().to(device).requires_grad_(True)
    be = beta.detach().to(device).requires_grad_(True)
    rm = torch.zeros(h, device=device)
    rv = torch.ones(h, device=device)
    y = F.batchnorm_relu(xx, ga, be, rm, rv, 0.1, 1e-5, True, fuse_relu=relu,
                         out16=bf)
    (y.float() * g.float().to(device)).sum().backward()
    return [t.detach().clone() for t in (y, xx.grad, ga.grad, be.grad, rm, rv)]


# 5. end to end against torch batch_norm + relu on the fp32 CPU oracle
@pytest.mark.parametrize("n,h", [(1000, 256), (4099, 64), (63, 40)])
def test_end_to_end_vs_cpu_oracle(n, h):
    require_ext()
    got = _autograd_run(n, h, DEV)
    ref = _autograd_run(n, h, torch.device("cpu"))
    assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.bfloat16
    for k, (a, b) in enumerate(zip(got, ref)):
        a, b = a.float().cpu(), b.float()
        tol = 5e-3 + 1e-3 * b.abs()
        if k < 2:  # bf16 outputs (y, dx): one bf16 ulp on top
            tol = tol + _bf16_ulp(b)
        assert ((a - b).abs() <= tol).all(), (k, (a - b).abs().max())


# 6. deterministic mode: bitwise reproducible run to run
def test_deterministic_bitwise(monkeypatch):
    require_ext()
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    a = _autograd_run(4099, 256, DEV)
    b = _autograd_run(4099, 256, DEV)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


# 7. hipGraph capture: the per-call slab must be capture-safe
def test_graph_capture_matches_eager():
    require_ext()
    n, h = 1000, 256
    eager = _autograd_run(n, h, DEV)
    x, g, gamma, beta = _inputs(n, h)
    xs = x.clone().requires_grad_(True)
    ga = gamma.clone().requires_grad_(True)
    be = beta.clone().requires_grad_(True)
    rm = torch.zeros(h, device=DEV)
    rv = torch.ones(h, device=DEV)
    gf = g.float()

    def step():
        y = F.batchnorm_relu(xs, ga, be, rm, rv, 0.1, 1e-5, True,
                             fuse_relu=True, out16=True)
        grads = torch.autograd.grad((y.float() * gf).sum(), (xs, ga, be))
        return (y,) + grads

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside capture (allocator, lazy init)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        rm.zero_()
        rv.fill_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        # the slab fold has a fixed order, so replay == eager bitwise
        for a, b in zip(outs + (rm, rv), eager):
            assert torch.equal(a, b)


# fp32 streams take the same wide reductions (two 16-B loads per lane and
# row); they keep y in the backward (no mask).  Same derived bounds, without
# the bf16 output ulp: the fp32 store is inside the 8 u elementwise term.
FP32_SHAPES = [(n, h) for h in (256, 32, 40) for n in (7, 63, 4099)]


@pytest.mark.parametrize("n,h", FP32_SHAPES)
def test_fp32_stream_bounds(n, h):
    C = require_ext()
    x16, g16, gamma, beta = _inputs(n, h)
    gen = torch.Generator().manual_seed(77 + n + h)
    # full-precision fp32 operands (not bf16-representable)
    x = x16.float() + torch.randn(n, h, generator=gen).to(DEV) * 1e-3
    g = g16.float() + torch.randn(n, h, generator=gen).to(DEV) * 1e-3
    xd, gd = x.double(), g.double()

    p = C.bn_stats(x).double()
    assert p[2 * h].item() == n
    assert ((p[:h] - xd.sum(0)).abs() <= (n + 4) * U32 * xd.abs().sum(0)).all()
    assert ((p[h:2 * h] - (xd * xd).sum(0)).abs()
            <= (n + 4) * U32 * (xd * xd).sum(0)).all()

    rm = torch.zeros(h, device=DEV)
    rv = torch.ones(h, device=DEV)
    seed = torch.empty(0, dtype=torch.int64, device=DEV)
    for relu in (True, False):
        y, mean, invstd = C.bn_relu_fwd(x, gamma, beta, rm.clone(), rv.clone(),
                                        0.1, 1e-5, True, relu, 0.0, seed)[:3]
        dx, dgamma, dbeta = C.bn_relu_bwd(g, x, gamma, mean, invstd, y, relu,
                                          1.0)
        part = C.bn_bwd_partials(g, x, y, mean, invstd, relu, 1.0)
        dx2 = C.bn_bwd_apply(g, x, y, mean, invstd, gamma, part, part, relu,
                             1.0)[0]
        md, isd, gad = mean.double(), invstd.double(), gamma.double()
        # mean/invstd themselves: sums within bound => compare to float64
        m_ref = xd.mean(0)
        assert torch.allclose(md, m_ref, atol=1e-5, rtol=1e-5)
        gm = torch.where(y <= 0, torch.zeros_like(gd), gd) if relu else gd
        xhat = (xd - md) * isd
        s1, s2 = gm.sum(0), (gm * xhat).sum(0)
        e1 = (n + 4) * U32 * gm.abs().sum(0)
        e2 = (n + 4) * U32 * (gm * xhat).abs().sum(0)
        for got1, got2 in ((part[:h], part[h:2 * h]), (dbeta, dgamma)):
            assert ((got1.double() - s1).abs() <= e1).all()
            assert ((got2.double() - s2).abs() <= e2).all()
        ref = gad * isd * (gm - s1 / n - xhat * s2 / n)
        tol = (gad * isd * (e1 + xhat.abs() * e2) / n
               + 8 * U32 * gad * isd * (gm.abs() + s1.abs() / n
                                        + (xhat * s2).abs() / n))
        for d in (dx, dx2):
            assert ((d.double() - ref).abs() <= tol).all()


def test_fp32_deterministic_bitwise(monkeypatch):
    C = require_ext()
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    x16, g16, gamma, beta = _inputs(4099, 256)
    x, g = x16.float() * 1.0001, g16.float() * 1.0001
    seed = torch.empty(0, dtype=torch.int64, device=DEV)

    def run():
        rm = torch.zeros(256, device=DEV)
        rv = torch.ones(256, device=DEV)
        y, mean, invstd = C.bn_relu_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5,
                                        True, True, 0.0, seed)[:3]
        return (y, mean, invstd, rm, rv) + tuple(
            C.bn_relu_bwd(g, x, gamma, mean, invstd, y, True, 1.0))

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)
