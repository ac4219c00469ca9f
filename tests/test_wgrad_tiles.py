"""The glds TN wgrad kernel at every output tile: 128x128, 256x128, 256x256.

``linear_wgrad16_b16(..., tile=t)`` forces a tile for any shape the kernel
supports; the default dispatch (``csrc/hip/gemm_dispatch.h``, reported by
``wgrad_tile``) is 128x128 at every shape, the wide tiles having measured
slower (profiles/21_wgrad_tiles.md).  Operands and comparison are those of tests/test_gemm_dispatch.py: ``g`` and ``x`` from
{-2, -1, 1, 2} as leading views of buffers whose remainder is NaN, so every
summation order and the split-K atomics give the exact value, compared bit for
bit with the fp64 product.  The sink cases are those of tests/test_grad_sink.py
(zeroed, pre-filled, carved at element offset 1 between sentinels).

The rows cover, per tile, 2 to 64 split-K slices, a tail step on the last
non-empty slice (513, 575, 577, 4123, 8319), tail-free splits (512, 576) and
slices that the ceil split leaves empty (576 and 577: 9 steps in 4 slices of
3; 8319: 129 steps in 64 slices of 3).

``linear_wgrad16`` (fp32 x) reaches no glds kernel at any shape, so there is
no tile to force on it: it must refuse one.

Model level: three chained ``F.linear16`` layers at H = 256 whose weights have
one +-1 per row and whose biases are small integers, so activations and all
three gradients stay small integers and exact through the stack; the backward
of the eager stack against a captured and replayed one, bit for bit and
against fp64, on the default tile and with 256x256 forced through
``set_wgrad_tile``.

Mutants (work dropped in the kernel, run against this file and the earlier
suite): see profiles/21_wgrad_tiles.md.
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
TILES = {"128x128": 1, "256x128": 2, "256x256": 3}
MS = (512, 513, 575, 576, 577, 4123, 8319)
NK = ((256, 256), (256, 512), (512, 256), (512, 512))
M_BIG = 1024 * 128 + 26


def _ext():
    import pertgnn._C as C
    return C


def _helpers():
    """The operand, poison and comparison helpers of the two suites whose
    conventions this file follows."""
    sys.path.insert(0, str(ROOT / "tests"))
    try:
        import test_gemm_dispatch as tgd
        import test_grad_sink as tgs
    finally:
        sys.path.pop(0)
    return tgd, tgs


def _slices(m, tiles):
    """gemm_dispatch.h glds_tn_slices, restated."""
    s = 1
    while tiles * s < 512 and s < 64 and s * 64 * 4 < m - m % 64:
        s *= 2
    return s


def _tile_dims(name):
    r, c = name.split("x")
    return int(r), int(c)


@functools.lru_cache(maxsize=None)
def _operands(m, n, k):
    """g [m, n], x [m, k] and the fp64 dw, db: made once per shape and shared
    by every tile and test; nothing writes to them."""
    tgd, _ = _helpers()
    g = tgd._poison(tgd._draw(m * 1009 + n * 13 + k + 6, (m, n), tgd.ACT, BF16))
    x = tgd._poison(tgd._draw(m * 1013 + n * 17 + k + 7, (m, k), tgd.ACT, BF16))
    return g, x, g.double().t() @ x.double(), g.double().sum(0)


def test_slice_coverage():
    """The rows reach 2 and 64 slices on every tile, and leave slices empty."""
    seen = {t: set() for t in TILES}
    empty = {t: 0 for t in TILES}
    for t in TILES:
        r, c = _tile_dims(t)
        for m in MS:
            for n, k in NK:
                s = _slices(m, (n // r) * (k // c))
                seen[t].add(s)
                steps = m // 64
                per = -(-steps // s)
                empty[t] += sum(1 for i in range(s) if i * per >= steps)
        assert min(seen[t]) == 2 and max(seen[t]) == 64, (t, seen[t])
        assert empty[t] > 0, t


@gpu
@needs_gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("tile", sorted(TILES))
def test_forced_tile_exact(tile, m, monkeypatch):
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    tgd, _ = _helpers()
    for n, k in NK:
        g, x, ref_dw, ref_db = _operands(m, n, k)
        for hb in (True, False):
            dw, db = C.linear_wgrad16_b16(g, x, hb, False, None, None,
                                          TILES[tile])
            what = f"{tile} {m}x{n}x{k} bias={hb}"
            tgd._assert_exact(dw, ref_dw, what + " dw")
            if hb:
                tgd._assert_exact(db, ref_db, what + " db")
            else:
                assert db.numel() == 0


@gpu
@needs_gpu
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("tile", sorted(TILES))
def test_forced_tile_sinks(tile, m, monkeypatch):
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    _, tgs = _helpers()
    for n, k in NK:
        g, x, ref_dw, ref_db = _operands(m, n, k)
        for hb in (True, False):
            def call(sinks):
                dw_s, db_s = (None, None) if sinks is None else (
                    sinks[0], sinks[1] if hb else None)
                dw, db = C.linear_wgrad16_b16(g, x, hb, False, dw_s, db_s,
                                              TILES[tile])
                if sinks is not None:
                    assert dw.numel() == 0 and db.numel() == 0
                return [dw, db] if hb else [dw]

            what = f"{tile} {m}x{n}x{k} bias={hb}"
            want = tgs._three_cases(what, call, seed=m + n + k)
            tgs._assert_bits(want[0], ref_dw.float(), what + " dw")
            if hb:
                tgs._assert_bits(want[1], ref_db.float(), what + " db")


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", sorted(TILES))
def test_inf_in_the_last_row(tile, monkeypatch):
    """The tail step stages copies of row m - 1 behind the tail and zeroes
    them in both images: an Inf in that row of g and of x must come out as
    the Inf sums of its own row and column, never as 0 * Inf = NaN."""
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    tgd, tgs = _helpers()
    m, n, k = 4123, 256, 512
    g0, x0, _, _ = _operands(m, n, k)
    g, x = tgd._poison(g0.clone()), tgd._poison(x0.clone())
    g[m - 1, 3] = float("inf")
    x[m - 1, 5] = float("-inf")
    ref_dw = (g.double().t() @ x.double()).float()
    ref_db = g.double().sum(0).float()
    assert not bool(torch.isnan(ref_dw).any())
    assert int(torch.isinf(ref_dw).sum()) == n + k - 1
    dw, db = C.linear_wgrad16_b16(g, x, True, False, None, None, TILES[tile])
    tgs._assert_bits(dw, ref_dw, f"{tile} dw with an Inf row")
    tgs._assert_bits(db, ref_db, f"{tile} db with an Inf row")


@gpu
@needs_gpu
def test_forced_tile_errors(monkeypatch):
    C = _ext()
    tgd, _ = _helpers()

    def ops(m, n, k, xdt=BF16):
        return (tgd._draw(1, (m, n), tgd.ACT, BF16),
                tgd._draw(2, (m, k), tgd.ACT, xdt))

    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    bad = [
        (511, 256, 256, 1),   # too few rows for the glds kernel
        (512, 384, 256, 2),   # n no multiple of 256
        (512, 384, 256, 3),
        (512, 256, 384, 3),   # k no multiple of 256
        (512, 192, 128, 1),   # n no multiple of 128
        (512, 256, 256, 4),   # no such tile
        (512, 256, 256, -1),
    ]
    for m, n, k, t in bad:
        g, x = ops(m, n, k)
        with pytest.raises(RuntimeError):
            C.linear_wgrad16_b16(g, x, True, False, None, None, t)
    g, x = ops(512, 256, 256)
    with pytest.raises(RuntimeError):  # fp16 compute is another kernel
        C.linear_wgrad16_b16(g, x, True, True, None, None, 3)
    g, x = ops(512, 256, 384)  # 256x128 fits k = 384
    dw, _ = C.linear_wgrad16_b16(g, x, True, False, None, None, 2)
    tgd._assert_exact(dw, g.double().t() @ x.double(), "256x128 k=384")
    # fp32 x never runs on the glds kernel
    g, x = ops(512, 256, 256, F32)
    with pytest.raises(RuntimeError):
        C.linear_wgrad16(g, x, True, None, None, 3)
    C.linear_wgrad16(g, x, True, None, None, 0)
    # the deterministic mode stays on the register kernel
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    g, x = ops(512, 256, 256)
    with pytest.raises(RuntimeError):
        C.linear_wgrad16_b16(g, x, True, False, None, None, 3)
    assert C.wgrad_tile(512, 256, 256, True) == "none"
    torch.cuda.synchronize()


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", sorted(TILES))
def test_random_normal_within_derived_bound(tile, monkeypatch):
    """m = 4123, fp32 outputs: within terms * 2^-24 * sum|a_i b_i|."""
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    tgd, _ = _helpers()
    m, n, k = 4123, 512, 256
    g = tgd._poison(tgd._randn(61, (m, n), BF16))
    x = tgd._poison(tgd._randn(67, (m, k), BF16))
    dw, db = C.linear_wgrad16_b16(g, x, True, False, None, None, TILES[tile])
    tgd._assert_within(dw, g.double().t() @ x.double(),
                       g.double().abs().t() @ x.double().abs(), m,
                       f"{tile} dw")
    tgd._assert_within(db, g.double().sum(0), g.double().abs().sum(0), m,
                       f"{tile} db")


@gpu
@needs_gpu
@pytest.mark.parametrize("tile", [0] + sorted(TILES.values()))
def test_long_contraction(tile, monkeypatch):
    """m = 1024 * 128 + 26, n = 1024, k = 256: the shape class of the flagship
    QKVS wgrad (64 slices on the 256x256 tile, a 26-row tail).  The default
    (tile 0) is the 128x128 tile at every shape: the wide tiles measured
    slower (profiles/21_wgrad_tiles.md), so they run only when forced."""
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    tgd, _ = _helpers()
    C.set_wgrad_tile(0)
    m, n, k = M_BIG, 1024, 256
    if tile == 0:
        for shape in ((m, n, k), (8319, 256, 256), (m, 1024, 384)):
            assert C.wgrad_tile(*shape) == "128x128"
        assert C.linear_path("wgrad", m, n, k, "a16", 1) == \
            f"glds_tn/s={_slices(m, (n // 128) * (k // 128))}"
        assert C.linear_path("wgrad", 8319, 256, 256, "a16", 1) == \
            f"glds_tn/s={_slices(8319, 4)}"
    g, x, ref_dw, ref_db = _operands(m, n, k)
    dw, db = C.linear_wgrad16_b16(g, x, True, False, None, None, tile)
    tgd._assert_exact(dw, ref_dw, f"tile {tile} dw")
    tgd._assert_exact(db, ref_db, f"tile {tile} db")


# ---------------------------------------------------------------------------
# model level: three chained linear16 layers, eager against captured
# ---------------------------------------------------------------------------

H, LAYERS, ROWS = 256, 3, 4123


def _stack_operands():
    tgd, _ = _helpers()
    gen = torch.Generator().manual_seed(11)
    ws, bs = [], []
    for l in range(LAYERS):
        w = torch.zeros(H, H)
        w[torch.arange(H), torch.randperm(H, generator=gen)] = \
            torch.tensor([-1.0, 1.0])[torch.randint(2, (H,), generator=gen)]
        ws.append(w.to(DEV))
        bs.append(torch.randint(-1, 2, (H,), generator=gen).float().to(DEV))
    x = tgd._poison(tgd._draw(21, (ROWS, H), tgd.ACT, BF16))
    gy = tgd._poison(tgd._draw(22, (ROWS, H), tgd.ACT, BF16))
    return x, gy, ws, bs


def _stack_reference(x, gy, ws, bs):
    """fp64 forward and backward of the stack: dw, db per layer."""
    acts = [x.double()]
    for w, b in zip(ws, bs):
        acts.append(acts[-1] @ w.double().t() + b.double())
    assert float(acts[-1].abs().max()) <= 2 + LAYERS
    g = gy.double()
    out = []
    for l in reversed(range(LAYERS)):
        out.append((g.t() @ acts[l], g.sum(0)))
        g = g @ ws[l].double()
    return out[::-1]


def _stack_grads(x, gy, params):
    h = x
    for l in range(LAYERS):
        h = F.linear16(h, params[2 * l], params[2 * l + 1])
    return torch.autograd.grad(h, params, gy)


def _run_stack(expect_tile):
    """Eager and captured backward of the stack, both bit-equal to fp64."""
    C = _ext()
    tgd, _ = _helpers()
    assert C.wgrad_tile(ROWS, H, H) == expect_tile
    x, gy, ws, bs = _stack_operands()
    ref = _stack_reference(x, gy, ws, bs)
    params = [p.clone().requires_grad_(True)
              for wb in zip(ws, bs) for p in wb]
    eager = [t.clone() for t in _stack_grads(x, gy, params)]
    static = [torch.zeros_like(p) for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _stack_grads(x, gy, params)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for s, t in zip(static, _stack_grads(x, gy, params)):
            s.copy_(t)
    for _ in range(2):
        for s in static:
            s.zero_()
        graph.replay()
    torch.cuda.synchronize()
    for l in range(LAYERS):
        for j, what in ((0, "dw"), (1, "db")):
            tgd._assert_exact(eager[2 * l + j], ref[l][j],
                              f"eager layer {l} {what}")
            assert torch.equal(tgd._bits(static[2 * l + j]),
                               tgd._bits(eager[2 * l + j])), \
                f"captured layer {l} {what} differs from eager"


@gpu
@needs_gpu
def test_stack_eager_vs_captured_forced_256x256(monkeypatch):
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    C.set_wgrad_tile(3)
    try:
        _run_stack("256x256")
    finally:
        C.set_wgrad_tile(0)
    assert C.wgrad_tile(ROWS, H, H) == "128x128"


@gpu
@needs_gpu
def test_stack_eager_vs_captured_default(monkeypatch):
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    _ext().set_wgrad_tile(0)
    _run_stack("128x128")
