"""The A-resident glds NT forward kernel against the streaming one.

``linear_fwd_a16o16`` (bf16 x and y, bf16 matrix cores) has two kernels for
the k = 256 forward: the streaming one (every block stages its own A and W
K-tiles) and the A-resident one (a block keeps its row tile of A in LDS and
sweeps the 128-wide column tiles).  Both run the same MFMA chain per output
element, so ``y`` must be equal by bit pattern on any input.  Which one runs
(in either of its two geometries, ``PERTGNN_FWD_RES_GEOM``)
is ``csrc/hip/gemm_dispatch.h``'s ``fwd_variant`` (reported by the binding of
that name); ``set_fwd_variant`` forces one for every shape the resident
kernel can run (k = 256, n a multiple of 128, any m >= 1), and
``linear_fwd_a16o16(..., variant=v)`` forces one per call and refuses a shape
the kernel cannot take.  ``PERTGNN_NO_FWD_RESIDENT=1`` keeps the streaming
kernel.  ``linear_path`` reports the family and does not change.

The rows cover one partial row tile (1, 63, 127), exactly one (128), a tile
plus one row (129), several with a tail (513, 1413) and without (640), for
both row-tile heights (64 and 128) of the kernel's two geometries; the widths
one column tile, two, and the model's eight.  The exact-operand cases are
those of tests/test_gemm_dispatch.py: activations from {-2, -1, 1, 2}, weights
from {+-0.5, +-1.5}, biases multiples of 1/8, NaN behind every operand,
compared bit for bit with the fp64 product.

Mutants (work dropped in the kernel, run against this file and the earlier
suite): see profiles/25_fwd_resident.md.
"""
import functools
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

BF16, F32 = torch.bfloat16, torch.float32
BN = 128
K = 256            # the only k the predicate admits
MS = (1, 63, 127, 128, 129, 513, 640, 1413)
NS = (BN, 2 * BN, 1024)
STREAM, RESIDENT = 1, 2
SENTINEL = -77.0   # exactly representable in bf16, never a product below
MIN_M = 57344      # gemm_dispatch.h FWD_RESIDENT_MIN_M, restated on purpose
M_ON = 90112       # a row count well past the hand-over
# PERTGNN_FWD_RES_GEOM (read per call): 128-row tiles / 64-row tiles / default
GEOMS = ("1", "2", "0")


def _ext():
    import pertgnn._C as C
    return C


def _tgd():
    """The operand, poison and comparison helpers of the suite whose
    conventions this file follows."""
    sys.path.insert(0, str(ROOT / "tests"))
    try:
        import test_gemm_dispatch as tgd
    finally:
        sys.path.pop(0)
    return tgd


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = _bits(a) != _bits(b)
    n = int(bad.sum())
    if n:
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(
            f"{what}: {n} of {bad.numel()} elements differ, first at flat "
            f"index {i}: {a.flatten()[i].item()} vs {b.flatten()[i].item()}")


def _empty():
    return torch.empty(0, device=DEV, dtype=F32)


class _forced:
    """set_fwd_variant(v) for the body, the automatic choice afterwards."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        _ext().set_fwd_variant(self.v)

    def __exit__(self, *exc):
        _ext().set_fwd_variant(0)
        return False


@functools.lru_cache(maxsize=None)
def _random_operands(m, n):
    """Random-normal bf16 x [m, K], fp32 w [n, K] and b [n], behind NaN; made
    once per shape, nothing writes to them."""
    tgd = _tgd()
    x = tgd._poison(tgd._randn(m * 1009 + n * 13 + 1, (m, K), BF16))
    w = tgd._poison(tgd._randn(m * 1013 + n * 17 + 2, (n, K), F32))
    b = tgd._poison(tgd._randn(m * 1019 + n * 19 + 3, (n,), F32))
    return x, w, b


@functools.lru_cache(maxsize=None)
def _exact_operands(m, n):
    """Exact operands and the fp64 product (without the bias)."""
    tgd = _tgd()
    x = tgd._poison(tgd._draw(m * 1009 + n * 13 + 4, (m, K), tgd.ACT, BF16))
    w = tgd._poison(tgd._draw(m * 1013 + n * 17 + 5, (n, K), tgd.WH, F32))
    b = tgd._poison(tgd._bias(m * 1019 + n * 19 + 6, n))
    return x, w, b, x.double() @ w.double().t()


# ---------------------------------------------------------------------------
# dispatch report: host only
# ---------------------------------------------------------------------------

def test_fwd_variant_report(monkeypatch):
    C = _ext()
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT", raising=False)
    C.set_fwd_variant(0)
    # the hand-over row count: one below, at, one above
    assert C.fwd_variant(MIN_M - 1, 1024, K) == ("stream" if MIN_M > 512
                                                 else "none")
    assert C.fwd_variant(MIN_M, 1024, K) == "resident"
    assert C.fwd_variant(MIN_M + 1, 1024, K) == "resident"
    assert C.fwd_variant(180762, 1024, K) == "resident"
    assert C.fwd_variant(0, 1024, K) == "none"
    # k: only 256; the other multiples of 32 stay on the streaming kernel
    assert C.fwd_variant(M_ON, 1024, 224) == "stream"
    assert C.fwd_variant(M_ON, 1024, 288) == "stream"
    assert C.fwd_variant(M_ON, 1024, 384) == "stream"
    assert C.fwd_variant(M_ON, 1024, 250) == "none"
    # n: whole 128-wide column tiles
    assert C.fwd_variant(M_ON, BN - 1, K) == "none"
    assert C.fwd_variant(M_ON, BN, K) == "resident"
    assert C.fwd_variant(M_ON, BN + 64, K) == "none"
    # the 128x256 tile keeps the shape where it already streams A once
    assert C.fwd_variant(1024 * 128, 256, K) == "stream"
    assert C.fwd_variant(1024 * 128 - 1, 256, K) == "resident"
    # the switch
    monkeypatch.setenv("PERTGNN_NO_FWD_RESIDENT", "1")
    assert C.fwd_variant(M_ON, 1024, K) == "stream"
    assert C.fwd_variant(180762, 1024, K) == "stream"
    monkeypatch.setenv("PERTGNN_NO_FWD_RESIDENT", "0")
    assert C.fwd_variant(M_ON, 1024, K) == "resident"
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT")
    assert C.fwd_variant(M_ON, 1024, K) == "resident"


def test_forced_variant_report(monkeypatch):
    C = _ext()
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT", raising=False)
    try:
        for v, name in ((STREAM, "stream"), (RESIDENT, "resident")):
            C.set_fwd_variant(v)
            for m in MS + (4096,):
                for n in NS:
                    assert C.fwd_variant(m, n, K) == name, (v, m, n)
            # shapes the resident kernel cannot run keep the automatic choice
            assert C.fwd_variant(4096, 1024, 384) == "stream"
            assert C.fwd_variant(129, 1024, 384) == "none"
            assert C.fwd_variant(4096, BN - 1, K) == "none"
            assert C.fwd_variant(0, 1024, K) == "none"
        # a forced variant outlasts the switch: the switch is for the default
        monkeypatch.setenv("PERTGNN_NO_FWD_RESIDENT", "1")
        C.set_fwd_variant(RESIDENT)
        assert C.fwd_variant(M_ON, 1024, K) == "resident"
        for bad in (-1, 3):
            with pytest.raises(RuntimeError, match="set_fwd_variant"):
                C.set_fwd_variant(bad)
    finally:
        C.set_fwd_variant(0)
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT")
    assert C.fwd_variant(M_ON, 1024, K) == "resident"


def test_linear_path_unchanged(monkeypatch):
    """The label is the family's, whichever variant runs."""
    C = _ext()
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT", raising=False)
    shapes = [(511, 1024, K, "reg_nt_64"), (512, 1024, K, "glds_nt_128x128"),
              (513, 1024, K, "glds_nt_128x128"),
              (4096, 1024, 224, "glds_nt_128x128"),
              (4096, 1024, 288, "glds_nt_128x128"),
              (4096, BN - 1, K, "reg_nt_64"), (4096, BN, K, "glds_nt_128x128"),
              (180762, 1024, K, "glds_nt_128x128"),
              (1024 * 128, 256, K, "glds_nt_128x256")]
    try:
        for v in (0, STREAM, RESIDENT):
            C.set_fwd_variant(v)
            for m, n, k, label in shapes:
                assert C.linear_path("fwd", m, n, k, "a16", 1) == label, \
                    (v, m, n, k)
    finally:
        C.set_fwd_variant(0)
    assert "a16|1|fwd|glds_nt_128x128" in C.linear_path_labels()
    assert not [l for l in C.linear_path_labels() if "resident" in l]


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("geom", GEOMS)
def test_bits_against_streaming(geom, m, n, monkeypatch):
    """Random-normal operands: variant 2 against variant 1, by bit pattern,
    through the hook and through the per-call argument."""
    monkeypatch.setenv("PERTGNN_FWD_RES_GEOM", geom)
    C = _ext()
    x, w, b = _random_operands(m, n)
    for bias in (b, _empty()):
        with _forced(STREAM):
            assert C.fwd_variant(m, n, K) == "stream"
            y1 = C.linear_fwd_a16o16(x, w, bias, False)
        with _forced(RESIDENT):
            assert C.fwd_variant(m, n, K) == "resident"
            y2 = C.linear_fwd_a16o16(x, w, bias, False)
        what = f"{m}x{n}x{K} bias={bias.numel() > 0}"
        assert y2.shape == (m, n) and y2.dtype == BF16
        assert bool(torch.isfinite(y2.float()).all()), what
        _same_bits(y2, y1, what)
        _same_bits(C.linear_fwd_a16o16(x, w, bias, False, RESIDENT), y1,
                   what + " per call")
        _same_bits(C.linear_fwd_a16o16(x, w, bias, False, STREAM), y1,
                   what + " per call stream")


@gpu
@needs_gpu
@pytest.mark.parametrize("n", (BN, 1024))
@pytest.mark.parametrize("m", (129, 513))
@pytest.mark.parametrize("geom", GEOMS)
def test_exact_against_fp64(geom, m, n, monkeypatch):
    monkeypatch.setenv("PERTGNN_FWD_RES_GEOM", geom)
    C = _ext()
    tgd = _tgd()
    x, w, b, ref0 = _exact_operands(m, n)
    with _forced(RESIDENT):
        for bias in (b, None):
            ref = ref0 + b.double() if bias is not None else ref0
            y = C.linear_fwd_a16o16(x, w, bias if bias is not None
                                    else _empty(), False)
            tgd._assert_exact(y, ref, f"resident {m}x{n} bias={bias is not None}")
            y2, wt16 = C.linear_fwd_a16o16_wt(
                x, w, bias if bias is not None else _empty(), False)
            _same_bits(y2, y, f"resident {m}x{n} _wt y")
            if m >= 512:
                _same_bits(wt16, w.to(BF16).t().contiguous(), "wt16")
            else:
                assert wt16.numel() == 0


@gpu
@needs_gpu
@pytest.mark.parametrize("m", (129, 513))
@pytest.mark.parametrize("geom", GEOMS)
def test_nothing_written_past_m(geom, m, monkeypatch):
    """y as the first m rows of a sentinel-filled buffer: the rows of the
    partial last tile that lie past m keep the sentinel."""
    monkeypatch.setenv("PERTGNN_FWD_RES_GEOM", geom)
    C = _ext()
    tgd = _tgd()
    for n in (BN, 1024):
        x, w, b, ref0 = _exact_operands(m, n)
        for v in (STREAM, RESIDENT):
            out = torch.full((m + 256, n), SENTINEL, device=DEV, dtype=BF16)
            y = C.linear_fwd_a16o16(x, w, b, False, v, out)
            assert y.data_ptr() == out.data_ptr() and y.shape == (m, n)
            tgd._assert_exact(out[:m], ref0 + b.double(), f"v{v} {m}x{n}")
            assert bool((out[m:] == SENTINEL).all()), (v, m, n)


@gpu
@needs_gpu
@pytest.mark.parametrize("m", (129, 513))
@pytest.mark.parametrize("geom", GEOMS)
def test_inf_in_the_last_row(geom, m, monkeypatch):
    """The partial tile stages copies of row m - 1 behind the tail.  An Inf
    there must come out in row m - 1 alone; an Inf in the first row of the
    partial tile, whose slot neighbours the clamped copies, likewise."""
    monkeypatch.setenv("PERTGNN_FWD_RES_GEOM", geom)
    C = _ext()
    n = 1024
    x0, w, b, _ = _exact_operands(m, n)
    tgd = _tgd()
    for row in (m - 1, m - 1 - (m - 1) % 64):
        x = tgd._poison(x0.clone())
        x[row, 5] = float("inf")
        ref = x.double() @ w.double().t() + b.double()
        assert not bool(torch.isnan(ref).any())
        assert int(torch.isinf(ref).sum()) == n
        with _forced(STREAM):
            y1 = C.linear_fwd_a16o16(x, w, b, False)
        with _forced(RESIDENT):
            y2 = C.linear_fwd_a16o16(x, w, b, False)
        _same_bits(y2, ref.to(BF16), f"resident, Inf in row {row} of {m}")
        _same_bits(y2, y1, f"resident vs stream, Inf in row {row} of {m}")


@gpu
@needs_gpu
def test_forced_variant_errors():
    C = _ext()
    tgd = _tgd()

    def ops(m, n, k):
        return (tgd._draw(1, (m, k), tgd.ACT, BF16),
                tgd._draw(2, (n, k), tgd.WH, F32), tgd._bias(3, n))

    bad = [
        (640, 1024, 224, RESIDENT, False),   # k is not 256
        (640, 1024, 288, RESIDENT, False),
        (640, 1024, 384, RESIDENT, False),
        (640, BN - 1, K, RESIDENT, False),   # no whole column tile
        (640, BN + 64, K, RESIDENT, False),
        (640, BN - 1, K, STREAM, False),
        (640, 1024, 250, STREAM, False),     # k no multiple of 32
        (640, 1024, K, RESIDENT, True),      # fp16 matrix cores
        (640, 1024, K, 3, False),            # no such variant
        (640, 1024, K, -1, False),
    ]
    for m, n, k, v, fp16c in bad:
        x, w, b = ops(m, n, k)
        with pytest.raises(RuntimeError, match="variant"):
            C.linear_fwd_a16o16(x, w, b, fp16c, v)
    x, w, b = ops(640, 1024, K)
    with pytest.raises(RuntimeError, match="out must be"):
        C.linear_fwd_a16o16(x, w, b, False, RESIDENT,
                            torch.empty(639, 1024, device=DEV, dtype=BF16))


# ---------------------------------------------------------------------------
# autograd and model level
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
def test_linear16_autograd(monkeypatch):
    """F.linear16 on a [640, 256] -> 1024 layer: y, dx, dw, db bit-equal with
    the streaming and the resident forward (deterministic mode, so that the
    wgrad is order-stable)."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    C = _ext()
    tgd = _tgd()
    m, n = 640, 1024
    x0 = tgd._randn(11, (m, K), BF16)
    w0 = tgd._randn(12, (n, K), F32) * 0.1
    b0 = tgd._randn(13, (n,), F32)
    g = tgd._randn(14, (m, n), BF16)
    got = {}
    try:
        F.set_gemm_precision("bf16")
        for v in (STREAM, RESIDENT):
            x = x0.clone().requires_grad_(True)
            w = w0.clone().requires_grad_(True)
            b = b0.clone().requires_grad_(True)
            with _forced(v):
                assert C.fwd_variant(m, n, K) == ("stream", "resident")[v - 1]
                y = F.linear16(x, w, b)
                y.backward(g)
            got[v] = (y.detach(), x.grad, w.grad, b.grad)
    finally:
        F.set_gemm_precision("fp32")
    for name, a, c in zip(("y", "dx", "dw", "db"), got[STREAM], got[RESIDENT]):
        assert a is not None and c is not None, name
        _same_bits(c, a, f"linear16 {name}")
    ref = x0.float() @ w0.to(BF16).float().t() + b0
    assert float((got[RESIDENT][0].float() - ref).abs().max()) <= \
        2.0 ** -7 * float(ref.abs().max())


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
def test_model_variants_and_captured(monkeypatch):
    """A 3-layer H = 256 model on one small batch: loss, predictions and
    every gradient bit-equal with the streaming and the resident forward, and
    the resident run captured and replayed equal to eager."""
    sys.path.insert(0, str(ROOT))
    try:
        model, batches = _gpu_model()
    finally:
        sys.path.pop(0)
    b = batches[0]
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    monkeypatch.delenv("PERTGNN_NO_FWD_RESIDENT", raising=False)
    names = [n for n, _ in _live_params(model)]
    C = _ext()
    rows = b.x.shape[0]
    launched = []
    real = C.linear_fwd_a16o16_wt

    class Tap:
        def __getattr__(self, name):
            if name == "linear_fwd_a16o16_wt":
                def tap(x, w, *a, **k):
                    launched.append(C.fwd_variant(x.shape[0], w.shape[0],
                                                  x.shape[1]))
                    return real(x, w, *a, **k)
                return tap
            return getattr(C, name)

    try:
        F.set_gemm_precision("bf16")
        with _forced(STREAM):
            off = _model_grads(model, b)
        with _forced(RESIDENT):
            monkeypatch.setattr(F, "ext", lambda: Tap())
            on = _model_grads(model, b)
            monkeypatch.setattr(F, "ext", _ext)
            assert launched.count("resident") >= 2, (rows, launched)
            torch.cuda.synchronize()

            static = [None if g is None else torch.zeros_like(g)
                      for g in on[3]]
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
        C.set_fwd_variant(0)

    assert bool(torch.isfinite(on[0]))
    for what, other in (("streaming", off), ("captured", (*s_out, static))):
        for name, a, c in zip(("loss", "global_predict", "local_predict"),
                              on[:3], other[:3]):
            _same_bits(a.float(), c.float(), f"{what} {name}")
        for name, a, c in zip(names, on[3], other[3]):
            assert (a is None) == (c is None), (what, name)
            if a is not None:
                _same_bits(a, c, f"{what} {name}")
