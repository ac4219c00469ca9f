"""Gradient sinks: backward ops that add a parameter's gradient straight into
its slice of FusedAdam's ``flat_grad`` instead of returning it.

A sink-taking op must leave in the sink exactly what the return path leaves
there after autograd's AccumulateGrad: ``sink + v``.  Three cases per op and
kernel branch: a zeroed sink (``0 + v``, signed zeros included), a sink
pre-filled with small integers (``prefill + v``), and a sink carved at element
offset 1 of a larger buffer (only 4-byte aligned, as ``flat_grad`` slices
are) with sentinel cells around it that must keep their bits.

The GEMM and P-table operands make every sum independent of its order, as in
tests/test_gemm_dispatch.py: activations and gradients from {-2, -1, 1, 2},
weights and tables from small dyadic values, so split-K atomics are exact and
everything is compared by bit pattern.  The BN operands are the real forwards
of tests/test_attn_bn_bwd.py (shared through its cache); its partial sums
fold in a fixed order, so they repeat bit for bit too.

Model level: 3 layers, H = 256, bf16, PERTGNN_DETERMINISTIC=1, sinks on
against PERTGNN_NO_GRAD_SINK=1.
"""
import math
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
ACT = (-2.0, -1.0, 1.0, 2.0)
W3 = (-1.0, 0.0, 1.0)
TBL = (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)
BEFORE, AFTER = -7777.25, 9999.5  # sentinels around a carved sink
PAD_AFTER = 5


def _ext():
    import pertgnn._C as C
    return C


def _draw(seed, shape, values, dtype):
    g = torch.Generator(device=DEV).manual_seed(seed)
    idx = torch.randint(len(values), shape, generator=g, device=DEV)
    return torch.tensor(values, device=DEV, dtype=F32)[idx].to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_bits(got, want, what):
    assert got.dtype == F32 and want.dtype == F32, what
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    nbad = int(bad.sum())
    if nbad:
        i = bad.flatten().nonzero()[0].item()
        raise AssertionError(
            f"{what}: {nbad} of {bad.numel()} elements differ, first at flat "
            f"index {i}: got {got.flatten()[i].item()!r} want "
            f"{want.flatten()[i].item()!r}")


def _prefill(seed, shape):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g, device=DEV).to(F32)


class _Carved:
    """A sink of `shape` at element offset 1 of a larger buffer."""

    def __init__(self, shape, fill=None):
        n = math.prod(shape)
        self.buf = torch.empty(1 + n + PAD_AFTER, device=DEV, dtype=F32)
        self.buf[0] = BEFORE
        self.buf[1 + n:] = AFTER
        self.sink = self.buf[1:1 + n].view(shape)
        if fill is None:
            self.sink.zero_()
        else:
            self.sink.copy_(fill)
        assert self.sink.is_contiguous()
        assert self.sink.data_ptr() % 16 == 4, "want a 4-byte-aligned sink"
        self.n = n

    def check_sentinels(self, what):
        want = torch.empty_like(self.buf)
        want[0] = BEFORE
        want[1 + self.n:] = AFTER
        assert torch.equal(_bits(self.buf[:1]), _bits(want[:1])), \
            f"{what}: the cell before the sink changed"
        assert torch.equal(_bits(self.buf[1 + self.n:]),
                           _bits(want[1 + self.n:])), \
            f"{what}: a cell behind the sink changed"


def _three_cases(what, call, seed=0):
    """call(sinks) runs the op: `sinks` is a list with a tensor or None per
    parameter-gradient output; it returns the list of RETURNED gradients (an
    entry is ignored where a sink was given).  With every entry None that is
    the return path."""
    want = call(None)
    k = len(want)
    assert all(w.dtype == F32 for w in want), what
    for w in want:
        assert bool(torch.isfinite(w).all()), what
        assert float(w.abs().max()) < 2 ** 20, (what, float(w.abs().max()))
    # what AccumulateGrad leaves in a zeroed flat_grad slice: 0 + v
    zero_sum = [torch.zeros_like(w) + w for w in want]
    # 1. zeroed sinks
    sinks = [torch.zeros_like(w) for w in want]
    call(sinks)
    for i in range(k):
        _assert_bits(sinks[i], zero_sum[i], f"{what}: zeroed sink {i}")
    # 2. pre-filled sinks
    fills = [_prefill(seed + 17 * i + 1, w.shape) for i, w in enumerate(want)]
    sinks = [f.clone() for f in fills]
    call(sinks)
    for i in range(k):
        _assert_bits(sinks[i], fills[i] + want[i], f"{what}: pre-filled sink {i}")
    # 3. carved sinks, once zeroed and once pre-filled
    for tag, fs in (("zeroed", [None] * k), ("pre-filled", fills)):
        carved = [_Carved(tuple(w.shape), f) for w, f in zip(want, fs)]
        call([c.sink for c in carved])
        torch.cuda.synchronize()
        for i, c in enumerate(carved):
            c.check_sentinels(f"{what}: carved {tag} sink {i}")
            base = zero_sum[i] if fs[i] is None else fs[i] + want[i]
            _assert_bits(c.sink, base, f"{what}: carved {tag} sink {i}")
    return want


# ---------------------------------------------------------------------------
# CPU: the gate in front of the sinks
# ---------------------------------------------------------------------------

class _Comm:
    """Stand-in for a distributed comm on one process."""
    world_size = 1

    def __init__(self, device, distributed=True):
        self.device = device
        self.distributed = distributed
        self.calls = []

    def all_reduce_(self, t, async_op=False):
        self.calls.append(t.numel())
        return self if async_op else t

    def wait(self):
        return None


def test_gate(monkeypatch):
    from pertgnn.train.optim import FlatGradAllReduce, FusedAdam

    monkeypatch.delenv("PERTGNN_NO_GRAD_SINK", raising=False)
    lin = torch.nn.Linear(3, 1)  # a one-element bias: the weight's neighbour
    free = torch.nn.Parameter(torch.zeros(2))
    assert F.grad_sink(free) is None and F.grad_sink(torch.zeros(2)) is None
    opt = FusedAdam(list(lin.parameters()), lr=1e-3)
    for p, off in zip(opt.params, opt.offsets):
        s = F.grad_sink(p)
        assert s is not None and s.shape == p.shape and s.dtype == F32
        assert s.data_ptr() == opt.flat_grad[off:].data_ptr()
        assert s.data_ptr() == p.grad.data_ptr()
    w = lin.weight
    with torch.no_grad():
        assert F.grad_sink(w) is None
    monkeypatch.setenv("PERTGNN_NO_GRAD_SINK", "1")
    assert F.grad_sink(w) is None
    monkeypatch.setenv("PERTGNN_NO_GRAD_SINK", "0")
    assert F.grad_sink(w) is not None
    monkeypatch.delenv("PERTGNN_NO_GRAD_SINK")
    w.requires_grad_(False)
    assert F.grad_sink(w) is None
    w.requires_grad_(True)
    # a dropped or re-pointed .grad turns the sink off until zero_grad re-pins
    lin.zero_grad(set_to_none=True)
    assert w.grad is None and F.grad_sink(w) is None
    w.grad = torch.zeros_like(w)
    assert F.grad_sink(w) is None
    opt.zero_grad()
    assert F.grad_sink(w) is not None
    assert w.grad.data_ptr() == opt.flat_grad.data_ptr()
    # a live all-reduce engine needs the post-accumulate hooks
    comm = _Comm(torch.device("cpu"))
    engine = FlatGradAllReduce(opt, comm)
    assert F.grad_sink(w) is None
    engine.enabled = False
    assert F.grad_sink(w) is not None
    engine.enabled = True
    comm.distributed = False
    assert F.grad_sink(w) is not None


# ---------------------------------------------------------------------------
# GPU: linear wgrad, every branch
# ---------------------------------------------------------------------------

# (m, n, k, fp16 compute, deterministic, x dtype, expected linear_path label)
WGRAD = [
    (513, 128, 128, False, False, BF16, "glds_tn/s=2"),
    (577, 128, 128, False, False, BF16, "glds_tn/s=4"),
    (513, 4096, 2048, False, False, BF16, "glds_tn/s=1"),
    (17, 64, 64, False, False, BF16, "reg_tn_64/s=1"),
    (513, 64, 64, False, False, BF16, "reg_tn_64/s=4"),
    (17, 192, 128, False, False, BF16, "reg_tn_128/s=1"),
    (513, 192, 128, False, False, BF16, "reg_tn_128/s=4"),
    (513, 128, 128, False, True, BF16, "reg_tn_128/s=1"),
    (640, 256, 256, True, False, BF16, None),
    (17, 65, 64, True, False, BF16, None),
    (513, 129, 192, True, True, BF16, None),
    (513, 128, 384, False, False, F32, None),
    (17, 64, 384, False, False, F32, None),
    (513, 129, 384, False, True, F32, None),
]


def _wgrad_id(c):
    m, n, k, fp16c, det, xdt, _ = c
    return (f"{m}x{n}x{k}" + ("-fp16" if fp16c else "") + ("-det" if det else "")
            + ("-x32" if xdt == F32 else ""))


def _wgrad_call(g, x, hb, fp16c):
    C = _ext()

    def call(sinks):
        dw_s, db_s = (None, None) if sinks is None else (
            sinks[0], sinks[1] if hb else None)
        if x.dtype == BF16:
            dw, db = C.linear_wgrad16_b16(g, x, hb, fp16c, dw_s, db_s)
        else:
            dw, db = C.linear_wgrad16(g, x, hb, dw_s, db_s)
        if sinks is not None:
            assert dw.numel() == 0 and db.numel() == 0, \
                "a sunk gradient must not be returned as well"
        return [dw, db] if hb else [dw]

    return call


@gpu
@needs_gpu
@pytest.mark.parametrize("case", WGRAD, ids=_wgrad_id)
def test_linear_wgrad_sinks(case, monkeypatch):
    m, n, k, fp16c, det, xdt, label = case
    C = _ext()
    if det:
        monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    path = C.linear_path("wgrad", m, n, k, "a16" if xdt == BF16 else "o16",
                         2 if fp16c else 1, det)
    print(_wgrad_id(case), "->", path)
    if label is not None:
        assert path == label
    g = _draw(m * 31 + n, (m, n), ACT, BF16)
    x = _draw(m * 37 + k, (m, k), ACT, xdt)
    for hb in (True, False):
        want = _three_cases(f"{_wgrad_id(case)} bias={hb}",
                            _wgrad_call(g, x, hb, fp16c), seed=n + k)
        _assert_bits(want[0], (g.double().t() @ x.double()).float(), "dw")
        if hb:
            _assert_bits(want[1], g.double().sum(0).float(), "db")


@gpu
@needs_gpu
def test_linear_wgrad_no_rows_and_bad_sinks():
    C = _ext()
    n, k = 128, 256
    for xdt in (BF16, F32):
        g = torch.empty(0, n, device=DEV, dtype=BF16)
        x = torch.empty(0, k, device=DEV, dtype=xdt)
        fill_w, fill_b = _prefill(1, (n, k)), _prefill(2, (n,))
        dw_s, db_s = fill_w.clone(), fill_b.clone()
        _wgrad_call(g, x, True, False)([dw_s, db_s])
        _assert_bits(dw_s, fill_w, "m = 0 dw sink")
        _assert_bits(db_s, fill_b, "m = 0 db sink")
    g = _draw(3, (64, n), ACT, BF16)
    x = _draw(4, (64, k), ACT, BF16)
    ok_w = torch.zeros(n, k, device=DEV)
    ok_b = torch.zeros(n, device=DEV)
    bad = [
        (torch.zeros(n, k, device=DEV, dtype=torch.float16), ok_b),  # dtype
        (torch.zeros(n, k + 1, device=DEV), ok_b),                   # shape
        (torch.zeros(k, n, device=DEV).t(), ok_b),                   # strides
        (torch.zeros(n, k), ok_b),                                   # device
        (ok_w, None),                                                # no db sink
        (None, ok_b),                                                # no dw sink
        (ok_w, torch.zeros(n + 1, device=DEV)),
    ]
    for dw_s, db_s in bad:
        with pytest.raises(RuntimeError):
            C.linear_wgrad16_b16(g, x, True, False, dw_s, db_s)
    with pytest.raises(RuntimeError):
        C.linear_wgrad16_b16(g, x, False, False, ok_w, ok_b)
    torch.cuda.synchronize()
    assert not bool(ok_w.any()) and not bool(ok_b.any())


# ---------------------------------------------------------------------------
# GPU: grouped P-table backward
# ---------------------------------------------------------------------------

def _pt_operands(h, layers, v, r):
    s = 1000 * h + 10 * layers + v + r
    ifc = _draw(s + 1, (v, h), TBL, F32)
    rpc = _draw(s + 2, (r, h), TBL, F32)
    we_ifc = [_draw(s + 10 + l, (h, h), W3, F32) for l in range(layers)]
    we_rpc = [_draw(s + 20 + l, (h, h), W3, F32) for l in range(layers)]
    dps = [_draw(s + 30 + i, (rows, h), ACT, BF16)
           for i, rows in enumerate([v] * layers + [r] * layers)]
    return ifc, rpc, we_ifc, we_rpc, dps


def _pt_call(ops, dps, splits, sunk=None):
    """Adapter for _three_cases over the outputs listed in `sunk` (indices
    into [d_ifc, d_rpc, dW_0 .. dW_2L-1]; default all).  Outputs outside
    `sunk` are returned by the op in every call and must not change."""
    C = _ext()
    ifc, rpc, we_ifc, we_rpc = ops
    layers = len(we_ifc)
    nout = 2 + 2 * layers
    sunk = list(range(nout)) if sunk is None else sunk
    none = torch.empty(0, dtype=BF16, device=DEV)
    dp_in = [none if d is None else d for d in dps]
    rest = {}

    def call(sinks):
        full = [None] * nout
        if sinks is not None:
            for i, s in zip(sunk, sinks):
                full[i] = s
        d_ifc, d_rpc, dw = C.ptables_bwd(dp_in, ifc, rpc, we_ifc, we_rpc,
                                         splits, full[0], full[1], full[2:])
        out, slot = [d_ifc, d_rpc], 0
        for gi in range(2 * layers):
            if full[2 + gi] is None:
                out.append(dw[slot])
                slot += 1
            else:
                out.append(none)
        assert dw.shape[0] == slot, "dW must hold only the groups without a sink"
        for i in range(nout):
            if full[i] is not None:
                assert out[i].numel() == 0, "a sunk gradient must not be returned"
            elif sinks is not None:  # mixed call: the returned rest is stable
                _assert_bits(out[i], rest[i], f"returned output {i} next to sinks")
            else:
                rest[i] = out[i]
        return [out[i] for i in sunk]

    return call


@gpu
@needs_gpu
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("splits", [1, 4])
@pytest.mark.parametrize("v,r", [(130, 5), (5, 17), (2048, 40)])
@pytest.mark.parametrize("layers", [1, 3])
def test_ptables_bwd_sinks(layers, v, r, splits, det, monkeypatch):
    if det:
        monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    h = 256
    ifc, rpc, we_ifc, we_rpc, dps = _pt_operands(h, layers, v, r)
    ops = (ifc, rpc, we_ifc, we_rpc)
    tag = f"L{layers} v{v} r{r} s{splits} det{det}"
    want = _three_cases(tag, _pt_call(ops, dps, splits), seed=v + r)
    # the return path itself is exact on these operands
    ref_t = [sum(dps[t * layers + l].double() @ ws[l].double()
                 for l in range(layers))
             for t, ws in enumerate((we_ifc, we_rpc))]
    _assert_bits(want[0], ref_t[0].float(), tag + " d_ifc")
    _assert_bits(want[1], ref_t[1].float(), tag + " d_rpc")
    for gi, d in enumerate(dps):
        table = ifc if gi < layers else rpc
        _assert_bits(want[2 + gi], (d.double().t() @ table.double()).float(),
                     f"{tag} dW {gi}")
    # mixed: only every other output has a sink
    nout = 2 + 2 * layers
    for sunk in (list(range(0, nout, 2)), list(range(1, nout, 2))):
        _three_cases(f"{tag} sinks {sunk}", _pt_call(ops, dps, splits, sunk),
                     seed=v)


@gpu
@needs_gpu
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("splits", [1, 4])
def test_ptables_bwd_missing_dp(splits, det, monkeypatch):
    """The sink of a missing dP keeps its bits; with a table's dPs all
    missing the table's sink does too."""
    if det:
        monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    else:
        monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    C = _ext()
    h, layers, v, r = 256, 3, 130, 17
    ifc, rpc, we_ifc, we_rpc, dps = _pt_operands(h, layers, v, r)
    ops = (ifc, rpc, we_ifc, we_rpc)
    none = torch.empty(0, dtype=BF16, device=DEV)
    for gone in ([1], [3, 4, 5]):
        part = [None if i in gone else d for i, d in enumerate(dps)]
        tag = f"missing {gone} s{splits} det{det}"
        want = _three_cases(tag, _pt_call(ops, part, splits), seed=7)
        for gi in gone:
            assert not bool(want[2 + gi].any()), "dW of a missing dP is zero"
        if gone == [3, 4, 5]:
            assert not bool(want[1].any())
        # NaN in the sink of a missing group: any read-modify-write, add of
        # zero or memset would show
        shapes = [(v, h), (r, h)] + [(h, h)] * (2 * layers)
        sinks = [torch.zeros(s, device=DEV) for s in shapes]
        poison = [2 + gi for gi in gone] + ([1] if gone == [3, 4, 5] else [])
        for i in poison:
            sinks[i].fill_(float("nan"))
        C.ptables_bwd([none if d is None else d for d in part], ifc, rpc,
                      we_ifc, we_rpc, splits, sinks[0], sinks[1], sinks[2:])
        for i, s in enumerate(sinks):
            if i in poison:
                assert bool(torch.isnan(s).all()), f"{tag}: sink {i} was written"
            else:
                _assert_bits(s, torch.zeros_like(want[i]) + want[i],
                             f"{tag}: sink {i}")


@gpu
@needs_gpu
def test_ptables_bwd_bad_sinks():
    C = _ext()
    h, layers, v, r = 256, 1, 5, 5
    ifc, rpc, we_ifc, we_rpc, dps = _pt_operands(h, layers, v, r)
    args = (dps, ifc, rpc, we_ifc, we_rpc, 1)
    t_ok = torch.zeros(v, h, device=DEV)
    w_ok = torch.zeros(h, h, device=DEV)
    with pytest.raises(RuntimeError):
        C.ptables_bwd(*args, torch.zeros(v + 1, h, device=DEV), None, [])
    with pytest.raises(RuntimeError):
        C.ptables_bwd(*args, t_ok.double(), None, [])
    with pytest.raises(RuntimeError):
        C.ptables_bwd(*args, None, None, [w_ok])  # 2L entries or none
    with pytest.raises(RuntimeError):
        C.ptables_bwd(*args, None, None,
                      [w_ok, torch.zeros(h, 2 * h, device=DEV)[:, :h]])
    with pytest.raises(RuntimeError):
        C.ptables_bwd(*args, None, None, [w_ok, torch.zeros(h, h)])
    torch.cuda.synchronize()
    assert not bool(t_ok.any()) and not bool(w_ok.any())


# ---------------------------------------------------------------------------
# GPU: BN dgamma / dbeta
# ---------------------------------------------------------------------------

def _attn_bn_cases():
    sys.path.insert(0, str(ROOT / "tests"))
    try:
        import test_attn_bn_bwd as tab
    finally:
        sys.path.pop(0)
    return tab


@gpu
@needs_gpu
@pytest.mark.parametrize("dropout_p", [0.0, 0.25])
@pytest.mark.parametrize("n", [1, 11, 67])
@pytest.mark.parametrize("h", [256, 512])
def test_bn_sinks(h, n, dropout_p):
    """bn_relu_bwd16 and edge_attn_bn_bwd16 (E > 0 and E = 0) on the operands
    of tests/test_attn_bn_bwd.py: dgamma and dbeta in the sinks, and every
    other output bit-equal to the return path's."""
    C = _ext()
    tab = _attn_bn_cases()
    for edges in (True, False):
        c = tab._case(h, 1, n, dropout_p, edges)
        dgamma, dbeta = c["want"][2], c["want"][3]

        def unfused(sinks):
            s = (None, None) if sinks is None else sinks
            dx, dg, db = C.bn_relu_bwd16(c["g"], c["x"], c["gamma"], c["mean"],
                                         c["invstd"], c["mask"], True,
                                         c["keep_inv"], *s)
            assert torch.equal(dx, c["dx"])
            assert sinks is None or (dg.numel() == 0 and db.numel() == 0)
            return [dg, db]

        def fused(sinks):
            s = (None, None) if sinks is None else sinks
            dqkvs, de, dg, db = C.edge_attn_bn_bwd16(
                c["g"], c["x"], c["mask"], c["gamma"], c["mean"], c["invstd"],
                c["keep_inv"], *c["attn"], None, None, *s)
            assert torch.equal(dqkvs, c["want"][0])
            assert torch.equal(de, c["want"][1])
            assert sinks is None or (dg.numel() == 0 and db.numel() == 0)
            return [dg, db]

        for name, call in (("bn_relu_bwd16", unfused),
                           ("edge_attn_bn_bwd16", fused)):
            tag = f"{name} h{h} n{n} p{dropout_p} edges{edges}"
            want = _three_cases(tag, call, seed=h + n)
            _assert_bits(want[0], dgamma, tag + " dgamma")
            _assert_bits(want[1], dbeta, tag + " dbeta")


@gpu
@needs_gpu
@pytest.mark.parametrize("h", [64, 256])
def test_bn_other_forms_sinks(h):
    """The fp32 BN backward, the bf16 one without a keep mask (h = 64 is off
    the wide path: the affine kernel writes the sinks) and the two sync-BN
    apply forms."""
    C = _ext()
    n = 67
    g0 = torch.Generator().manual_seed(h)
    x = torch.randn(n, h, generator=g0).to(DEV)
    gout = torch.randn(n, h, generator=g0).to(DEV)
    gamma = (torch.rand(h, generator=g0) + 0.5).to(DEV)
    beta = torch.zeros(h, device=DEV)
    seed = torch.empty(0, dtype=torch.int64, device=DEV)

    def stats():
        return torch.zeros(h, device=DEV), torch.ones(h, device=DEV)

    y, mean, invstd = C.bn_relu_fwd(x, gamma, beta, *stats(), 0.1, 1e-5, True,
                                    True, 0.0, seed)[:3]
    x16, g16 = x.to(BF16), gout.to(BF16)
    out16 = C.bn_relu_fwd16(x16, gamma, beta, *stats(), 0.1, 1e-5, True, True,
                            0.0, seed)
    y16, mean16, invstd16 = out16[:3]
    y16 = out16[3] if out16[3].numel() else y16  # the keep mask where there is one

    def both(sinks):
        return (None, None) if sinks is None else sinks

    def f32(sinks):
        return list(C.bn_relu_bwd(gout, x, gamma, mean, invstd, y, True, 1.0,
                                  *both(sinks))[1:])

    def b16(sinks):
        return list(C.bn_relu_bwd16(g16, x16, gamma, mean16, invstd16, y16,
                                    True, 1.0, *both(sinks))[1:])

    pl = C.bn_bwd_partials(gout, x, y, mean, invstd, True, 1.0)
    pl16 = C.bn_bwd_partials16(g16, x16, y16, mean16, invstd16, True, 1.0)

    def apply32(sinks):
        return list(C.bn_bwd_apply(gout, x, y, mean, invstd, gamma, pl, pl,
                                   True, 1.0, *both(sinks))[1:])

    def apply16(sinks):
        return list(C.bn_bwd_apply16(g16, x16, y16, mean16, invstd16, gamma,
                                     pl16, pl16, True, 1.0, *both(sinks))[1:])

    for name, call in (("bn_relu_bwd", f32), ("bn_relu_bwd16", b16),
                       ("bn_bwd_apply", apply32), ("bn_bwd_apply16", apply16)):
        want = _three_cases(f"{name} h{h}", call, seed=h)
        assert want[0].shape == (h,) and bool(want[0].abs().max() > 0)
    with pytest.raises(RuntimeError):
        C.bn_relu_bwd(gout, x, gamma, mean, invstd, y, True, 1.0,
                      torch.zeros(h, device=DEV), None)
    with pytest.raises(RuntimeError):
        C.bn_relu_bwd16(g16, x16, gamma, mean16, invstd16, y16, True, 1.0,
                        torch.zeros(h + 1, device=DEV),
                        torch.zeros(h, device=DEV))


# ---------------------------------------------------------------------------
# GPU: model level
# ---------------------------------------------------------------------------

def _gpu_model(heads=1):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train.optim import FusedAdam

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2, device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0, heads=heads).to(DEV)
    model.train()
    b = batches[0]
    assert b.x.shape[0] % 128 != 0, "want a batch with a row tail"
    opt = FusedAdam(model.parameters(), lr=1e-3)
    return model, opt, batches


def _forward_backward(model, b):
    gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                   b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                   num_graphs=b.num_graphs)
    loss = F.quantile_loss(b.y, gp.flatten(), 0.5)
    loss.backward()
    return loss.detach().clone(), gp.detach().clone(), lp.detach().clone()


def _watch(model):
    """Post-accumulate hooks on every parameter -> list of fired names."""
    fired = []
    for name, p in model.named_parameters():
        if isinstance(p, torch.nn.parameter.UninitializedParameter):
            continue
        p.register_post_accumulate_grad_hook(
            lambda p, name=name: fired.append(name))
    return fired


# parameters whose only use is an op that takes a sink
SUNK = ([f"convs.{l}.{w}" for l in range(3)
         for w in ("w4", "b4", "we_ifc", "we_rpc")]
        + [f"bns.{l}.{w}" for l in range(2) for w in ("weight", "bias")])


@gpu
@needs_gpu
@pytest.mark.parametrize("heads", [1, 4])
def test_model_sinks_on_off_bitwise(heads, monkeypatch):
    """flat_grad, loss and both predictions with sinks against
    PERTGNN_NO_GRAD_SINK=1, after one backward and after two without a
    zero_grad in between; the post-accumulate hooks of the sunk parameters
    stay silent on the sink path and fire once per backward on the other."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    model, opt, batches = _gpu_model(heads)
    b = batches[0]
    fired = _watch(model)
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
            one = _forward_backward(model, b)
            g1 = opt.flat_grad.detach().clone()
            n1 = list(fired)
            two = _forward_backward(model, b)
            g2 = opt.flat_grad.detach().clone()
            torch.cuda.synchronize()
            res[mode] = (one, g1, two, g2, n1, list(fired))
    finally:
        F.set_gemm_precision("fp32")
    (one_s, g1_s, two_s, g2_s, n1_s, n2_s) = res["sink"]
    (one_r, g1_r, two_r, g2_r, n1_r, n2_r) = res["return"]
    for a, c, what in zip(one_s + two_s, one_r + two_r,
                          ("loss", "global", "local") * 2):
        assert torch.equal(a, c), what
    assert bool(g1_r.abs().max() > 0)
    _assert_bits(g1_s, g1_r, "flat_grad after one backward")
    _assert_bits(g2_s, g2_r, "flat_grad after two backwards")
    assert not torch.equal(g2_r, g1_r)
    names = dict(model.named_parameters())
    for n in SUNK:
        assert n in names, n
        assert n not in n2_s, f"{n}: AccumulateGrad ran on the sink path"
        assert n1_r.count(n) == 1 and n2_r.count(n) == 2, (n, n2_r.count(n))
    # the tables' P-table share goes to the sink as well; other uses may not
    assert n2_s.count("interface_embeds.weight") <= \
        n2_r.count("interface_embeds.weight")
    print("sink path accumulated through autograd:", sorted(set(n2_s)))


@gpu
@needs_gpu
def test_model_set_to_none_and_repin(monkeypatch):
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    monkeypatch.delenv("PERTGNN_NO_GRAD_SINK", raising=False)
    model, opt, batches = _gpu_model()
    b = batches[0]
    fired = _watch(model)
    try:
        F.set_gemm_precision("bf16")
        opt.zero_grad()
        _forward_backward(model, b)
        want = opt.flat_grad.detach().clone()
        assert "convs.0.w4" not in fired
        # .grad dropped: the return path, into fresh tensors
        model.zero_grad(set_to_none=True)
        opt.flat_grad.zero_()
        del fired[:]
        _forward_backward(model, b)
        assert not bool(opt.flat_grad.any()), "a stale sink was written"
        for n in SUNK:
            assert fired.count(n) == 1, n
        for p, off in zip(opt.params, opt.offsets):
            if p.grad is None:  # a parameter outside the loss
                assert not bool(want[off:off + p.numel()].any())
                continue
            assert p.grad.data_ptr() != opt.flat_grad[off:].data_ptr()
            _assert_bits(p.grad.reshape(-1), want[off:off + p.numel()],
                         "grad on the return path")
        # the optimizer re-pins: sinks again
        opt.zero_grad()
        del fired[:]
        _forward_backward(model, b)
        torch.cuda.synchronize()
        for n in SUNK:
            assert n not in fired, n
        _assert_bits(opt.flat_grad, want, "flat_grad after re-pinning")
    finally:
        F.set_gemm_precision("fp32")


@gpu
@needs_gpu
def test_model_allreduce_engine_switch(monkeypatch):
    """With a live FlatGradAllReduce every parameter's hook fires and every
    bucket launches; with enabled = False (as bench.py sets it around the
    split-mode capture) the sinks are used again."""
    from pertgnn.train.optim import FlatGradAllReduce

    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    monkeypatch.delenv("PERTGNN_NO_GRAD_SINK", raising=False)
    model, opt, batches = _gpu_model()
    b = batches[0]
    comm = _Comm(DEV)
    engine = FlatGradAllReduce(opt, comm, bucket_cap_mb=0.25)
    assert len(engine.buckets) > 1
    fired = _watch(model)
    try:
        F.set_gemm_precision("bf16")
        opt.zero_grad()
        engine.reset()
        _forward_backward(model, b)
        engine.finalize()
        torch.cuda.synchronize()
        want = opt.flat_grad.detach().clone()
        used = set(fired)
        for n in SUNK:
            assert fired.count(n) == 1, n
        for bk in engine.buckets:
            assert bk["work"] is not None
            live = [p for p in bk["params"]
                    if any(p is q for n, q in model.named_parameters()
                           if n in used)]
            assert bk["pending"] == len(bk["params"]) - len(live)
        assert len(comm.calls) == len(engine.buckets)
        assert sum(comm.calls) == opt.flat_grad.numel()

        engine.enabled = False
        opt.zero_grad()
        del fired[:]
        del comm.calls[:]
        _forward_backward(model, b)
        engine.finalize()
        torch.cuda.synchronize()
        assert not comm.calls
        for n in SUNK:
            assert n not in fired, n
        _assert_bits(opt.flat_grad, want, "flat_grad with the engine off")
    finally:
        F.set_gemm_precision("fp32")


@gpu
@needs_gpu
def test_captured_steps_match_eager(monkeypatch):
    """Three GraphStepper replays against three eager steps from the same
    state, sinks on in both, at the tolerance of the test of the same name in
    tests/test_ptable_grouped.py."""
    from pertgnn.train.capture import GraphStepper

    monkeypatch.delenv("PERTGNN_NO_GRAD_SINK", raising=False)
    monkeypatch.delenv("PERTGNN_DETERMINISTIC", raising=False)
    model, opt, batches = _gpu_model()
    fired = _watch(model)
    try:
        F.set_gemm_precision("bf16")
        stepper = GraphStepper(model, opt, None, None, 0.5, DEV, batches)
        snap = stepper._snapshot()
        eager_losses = []
        for _ in range(3):
            stepper.acc.zero_()
            stepper._full_step(0)
            eager_losses.append(float(stepper.acc[0]) / batches[0].num_graphs)
        torch.cuda.synchronize()
        g_eager = opt.flat_grad.detach().clone()
        p_eager = opt.flat_param.detach().clone()
        stepper._restore(snap)
        assert stepper.capture() == "full"
        losses = []
        for _ in range(3):
            total, _, n = stepper.run_epoch_sums()
            losses.append(total / n)
        g_graph = opt.flat_grad.detach().clone()
        p_graph = opt.flat_param.detach().clone()
    finally:
        F.set_gemm_precision("fp32")
    for n in SUNK:
        assert n not in fired, f"{n}: the steps did not use the sink"
    print("captured", losses, "eager", eager_losses)
    for a, e in zip(losses, eager_losses):
        assert math.isfinite(a) and abs(a - e) <= 1e-2 * abs(e), (a, e)
    assert bool(g_eager.abs().max() > 0)
    assert torch.allclose(g_graph, g_eager, atol=1e-2, rtol=1e-2), \
        (g_graph - g_eager).abs().max()
    assert torch.allclose(p_graph, p_eager, atol=1e-2, rtol=1e-2), \
        (p_graph - p_eager).abs().max()
