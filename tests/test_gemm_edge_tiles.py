"""The glds GEMMs run their partial last row tile inside the main launch
(``csrc/hip/gemm_bf16.hip``): the NT kernel (forward, dgrad) clamps the edge
tile's A rows and skips the stores past ``m``; the TN kernel (wgrad) runs the
``m % 64`` rows as a zero-padded last step of its last split-K slice; one
launch writes both bf16 weight images.

Forward / dgrad: rows of an MFMA tile are independent, so ``op(x[:m])`` must be
**bitwise** ``op(x_pad)[:m]`` where ``x_pad`` has ``ceil(m/128)*128`` valid
rows, whatever lies behind ``x[:m]`` in memory (NaN here).  m = 513 / 639 / 767
leave 1 / 127 / 127 tail rows after 4 / 4 / 5 full tiles, 640 has none;
131098 = 1024*128 + 26 takes the 128x256 single-column-tile variant.

wgrad: against the fp64 product of the bf16 operands, the maximum error may be
at most that of the same call on the first ``m - m % 64`` rows (the tail-free
main path) plus one fp32 ulp of the largest output: the tail step adds at most
27..63 products to one slice's fp32 accumulators, one rounding of a partial
sum that is no larger than the output.  m = 513 / 575 / 577 / 4123 leave
1 / 63 / 1 / 27 rows, 576 none.
"""
import functools
import math

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

N, K = 1024, 256
M_NT = [513, 639, 640, 767]
M_BIG = 1024 * 128 + 26
M_TN = [513, 575, 576, 577, 4123]


def _ext():
    import pertgnn._C as C
    return C


def _bits(t):
    return t.contiguous().view(torch.int16)


def _randn(seed, *shape):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


@functools.lru_cache(maxsize=None)
def _weights(k):
    """fp32 w [N, k], bias [N] and the fp64 value of the bf16-rounded w."""
    w = _randn(7 + k, N, k) * 0.05
    b = _randn(8 + k, N)
    return w, b, w.to(torch.bfloat16).double()


def _with_nan_behind(a_pad, m):
    """The first m rows of a_pad as a contiguous view of a larger buffer whose
    remaining rows (at least 128) are NaN."""
    extra = a_pad.shape[0] - m + 128
    buf = torch.cat([a_pad[:m], torch.full((extra, a_pad.shape[1]),
                                           float("nan"), device=DEV,
                                           dtype=a_pad.dtype)])
    v = buf[:m]
    assert v.is_contiguous() and bool(torch.isnan(buf[m:]).all())
    return v


def _check_fwd(m, k):
    C = _ext()
    w, b, w64 = _weights(k)
    mp = -(-m // 128) * 128
    x_pad = _randn(m, mp, k).to(torch.bfloat16)
    x = _with_nan_behind(x_pad, m)
    y = C.linear_fwd_a16o16(x, w, b)
    y_pad = C.linear_fwd_a16o16(x_pad, w, b)
    assert y.shape == (m, N) and y.dtype == torch.bfloat16
    assert not bool(torch.isnan(y).any())
    ndiff = int((_bits(y) != _bits(y_pad[:m])).sum())
    ref = x.double() @ w64.t() + b.double()
    err = float((y.double() - ref).abs().max())
    print(f"fwd m={m} k={k}: differing elements {ndiff}, max err vs fp64 {err:.4g}")
    assert ndiff == 0
    assert torch.allclose(y.double(), ref, atol=0.05, rtol=1e-2), err


def _check_dgrad(m):
    C = _ext()
    w, _, w64 = _weights(K)
    mp = -(-m // 128) * 128
    g_pad = _randn(m + 1, mp, N).to(torch.bfloat16)
    g = _with_nan_behind(g_pad, m)
    dx = C.linear_dgrad16_o16(g, w)
    dx_pad = C.linear_dgrad16_o16(g_pad, w)
    assert dx.shape == (m, K) and dx.dtype == torch.bfloat16
    assert not bool(torch.isnan(dx).any())
    ndiff = int((_bits(dx) != _bits(dx_pad[:m])).sum())
    ref = g.double() @ w64
    err = float((dx.double() - ref).abs().max())
    print(f"dgrad m={m}: differing elements {ndiff}, max err vs fp64 {err:.4g}")
    assert ndiff == 0
    assert torch.allclose(dx.double(), ref, atol=0.3, rtol=1e-2), err


@gpu
@needs_gpu
@pytest.mark.parametrize("k", [K, 384])
@pytest.mark.parametrize("m", M_NT)
def test_forward_tail_rows_equal_interior_rows(m, k):
    _check_fwd(m, k)


@gpu
@needs_gpu
@pytest.mark.parametrize("m", M_NT)
def test_dgrad_tail_rows_equal_interior_rows(m):
    _check_dgrad(m)


@gpu
@needs_gpu
def test_dgrad_wide_tile_tail_rows_equal_interior_rows():
    """m / 128 >= 1024 and an output width of 256: the 128x256 variant."""
    _check_dgrad(M_BIG)


def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23)


@gpu
@needs_gpu
@pytest.mark.parametrize("m", M_TN)
def test_wgrad_tail_step(m):
    C = _ext()
    g = _with_nan_behind(_randn(m + 2, m, N).to(torch.bfloat16), m)
    x = _with_nan_behind(_randn(m + 3, m, K).to(torch.bfloat16), m)
    dw, db = C.linear_wgrad16_b16(g, x, True)
    assert dw.shape == (N, K) and db.shape == (N,)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    ref_dw = g.double().t() @ x.double()
    ref_db = g.double().sum(0)
    err_dw = float((dw.double() - ref_dw).abs().max())
    err_db = float((db.double() - ref_db).abs().max())

    mf = m - m % 64  # the tail-free call: main loop only
    g0, x0 = g[:mf], x[:mf]
    dw0, db0 = C.linear_wgrad16_b16(g0, x0, True)
    err_dw0 = float((dw0.double() - g0.double().t() @ x0.double()).abs().max())
    err_db0 = float((db0.double() - g0.double().sum(0)).abs().max())
    bound_dw = err_dw0 + _ulp32(float(ref_dw.abs().max()))
    bound_db = err_db0 + _ulp32(float(ref_db.abs().max()))
    print(f"wgrad m={m}: dw err {err_dw:.4g} (tail-free {err_dw0:.4g}, bound "
          f"{bound_dw:.4g}); db err {err_db:.4g} (tail-free {err_db0:.4g}, "
          f"bound {bound_db:.4g})")
    assert err_dw <= bound_dw
    assert err_db <= bound_db
    # and the absolute tolerances of test_glds_odd_m_tail_parity
    assert torch.allclose(dw.double(), ref_dw, atol=0.5, rtol=1e-3)
    assert torch.allclose(db.double(), ref_db, atol=0.2, rtol=1e-3)


@gpu
@needs_gpu
@pytest.mark.parametrize("shape", [(1024, 256), (1024, 384), (128, 32),
                                   (100, 37)])
def test_weight_images_bit_equal(shape):
    C = _ext()
    w = _randn(11, *shape) * 0.05
    w16, wt16 = C.convert_w16_both(w)
    ref = w.to(torch.bfloat16)
    assert w16.shape == shape and wt16.shape == shape[::-1]
    assert torch.equal(_bits(w16), _bits(ref))
    assert torch.equal(_bits(wt16), _bits(ref.t().contiguous()))


@gpu
@needs_gpu
def test_saved_image_gives_the_same_dx():
    """linear16 keeps the forward's transposed image for the dgrad; dx is
    bit-equal to the dgrad that converts the weight itself, and the forward
    without a gradient (straight image only) gives the same y."""
    C = _ext()
    w, b, _ = _weights(K)
    m = 639
    x = _randn(21, m, K).to(torch.bfloat16)
    gy = _randn(22, m, N).to(torch.bfloat16)

    y2, wt16 = C.linear_fwd_a16o16_wt(x, w, b)
    assert torch.equal(_bits(wt16),
                       _bits(w.to(torch.bfloat16).t().contiguous()))
    dx_conv = C.linear_dgrad16_o16(gy, w)
    dx_img = C.linear_dgrad16_o16(gy, w, False, wt16)
    assert torch.equal(_bits(dx_img), _bits(dx_conv))
    # below the dgrad gate (m < 512) no image is made
    assert C.linear_fwd_a16o16_wt(x[:100].contiguous(), w, b)[1].numel() == 0

    calls = []
    real = C.linear_dgrad16_o16

    class Spy:
        def __getattr__(self, name):
            if name == "linear_dgrad16_o16":
                def f(g, w_, fp16c, img):
                    calls.append(img)
                    return real(g, w_, fp16c, img)
                return f
            return getattr(C, name)

    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    ext = F.ext
    try:
        F.ext = lambda: Spy()
        y = F.linear16(xr, wr, b)
        y.backward(gy)
    finally:
        F.ext = ext
    assert len(calls) == 1 and calls[0] is not None, "no saved image"
    assert torch.equal(_bits(xr.grad), _bits(dx_conv))
    with torch.no_grad():
        y0 = F.linear16(x, w, b)
    assert torch.equal(_bits(y0), _bits(y.detach()))
    assert torch.equal(_bits(y0), _bits(y2))


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
def test_model_bit_reproducible_with_row_tail(monkeypatch):
    """3 layers, H = 256, bf16, a node count that is no multiple of 128: two
    steps on the same batch under PERTGNN_DETERMINISTIC=1 are bit-equal."""
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2, device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0).to(DEV)
    model.train()
    b = batches[0]
    n_nodes = b.x.shape[0]
    assert n_nodes >= 512 and n_nodes % 128 != 0, n_nodes
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    try:
        F.set_gemm_precision("bf16")
        loss_a, gp_a, lp_a, grads_a = _model_step(model, b)
        loss_b, gp_b, lp_b, grads_b = _model_step(model, b)
        torch.cuda.synchronize()
    finally:
        F.set_gemm_precision("fp32")
    assert torch.equal(loss_a, loss_b)
    assert torch.equal(gp_a, gp_b) and torch.equal(lp_a, lp_b)
    assert grads_a.keys() == grads_b.keys() and len(grads_a) > 10
    for name in grads_a:
        assert bool(torch.isfinite(grads_a[name]).all()), name
        assert torch.equal(grads_a[name], grads_b[name]), name
