"""Edge shapes of the kernels at the two ends of the training step, all in
csrc/hip/segops.hip outside its BatchNorm section: the embedding gathers and
their table gradients (``_table_grad`` -> ``vocab_scatter``, the dual scatter
of the attention backward, the balanced grouped scatter over ``_group_by``
plans), the pattern pool, the quantile loss and eval metrics, Adam and its
dynamic loss scaler.

How the reductions are compared:

* exact inputs.  Gradients and activations are integers in [-8, 8] (exact in
  bf16 and fp32), pool weights are powers of two, so every partial sum is an
  exact fp32 number in ANY summation order, with atomics or without
  (terms * 8 < 2^24 by a wide margin at these sizes).  The result must be
  ``torch.equal`` to an int64 / fp64 CPU ``index_add_``: a dropped, doubled
  or mis-indexed row cannot hide behind a tolerance.
* one random-normal case per kernel family against an fp64 reference, within
  the first-order bound of any summation order, per element
  ``terms * 2^-24 * sum|x_i|`` (fp32 output; plus ``2^-8 * |ref|`` for a
  bf16 output, as BF16_OUT of tests/test_edge_table_grad.py).  Rows that
  receive nothing must be exactly zero.

Findings recorded here and not tested:

* ``vocab_scatter_vec_kernel`` and ``vocab_scatter_dual_kernel`` (the
  LDS-atomic variants) cannot be reached through the bindings.  The vec
  kernel needs h % 256 == 0 and a shape the wave-private kernels refuse,
  i.e. 4*rows*64*4 > 163840 (rows > 160); the binding admits only
  rows*h*4 <= 163840, which at h >= 256 is rows <= 160.  The dual binding
  admits (rows0+rows1)*h*4 <= 163840 with h % 256 == 0, so rows0+rows1 <= 160
  and 4*(rows0+rows1)*64*4 <= 163840: the private-64 kernel always takes it.
* No scatter kernel checks its indices: an index >= rows writes outside the
  LDS table or dtable.  ``edge_table_plan`` validates on the host;
  ``_group_by``, ``vocab_scatter`` and ``vocab_scatter_dual`` trust their
  caller.  A test of that could only fault, so there is none.

CPU and GPU tests share this file, so the GPU ones carry the ``gpu`` mark
and the no-GPU skip one by one, as tests/test_edge_table_grad.py does.

Run on an MI355X box:  python -m pytest tests/test_segops_edges.py -m gpu -q
"""
import pytest
import torch

from pertgnn.ops import functional as F
from pertgnn.ops.backend import ext, require_ext

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

U32 = 2.0 ** -24          # fp32 unit roundoff
BF16_REL = 2.0 ** -8      # one bf16 store rounding is 2^-9 relative; x2
N_LIST = (0, 1, 3, 16, 17, 600, 1000)
# 0/1/3: fewer rows than the block's 4 waves; 16: exactly one unrolled round
# (4 waves x U = 4); 17: one more row (tail loop); 600: 3 blocks of the
# wave-private kernels ((600+255)/256) and 10 of the fallback ((600+63)/64);
# 1000: 4 blocks of 250 rows, the last wave rounds ragged.
DTYPES = (torch.float32, torch.bfloat16)


def _C():
    require_ext()
    return ext()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, seed):
    """integers in [-8, 8] as fp32 (exact in bf16 too)"""
    return torch.randint(-8, 9, shape, generator=_gen(seed)).float()


def _scatter_ref(g, idx, rows, h, col_off):
    """fp64 index_add_ of g[:, col_off:col_off+h] (exact for the integer
    inputs), the per-row term counts and the per-element sum of |x_i|."""
    x = g[:, col_off:col_off + h].double()
    ref = torch.zeros(rows, h, dtype=torch.float64).index_add_(0, idx, x)
    mag = torch.zeros(rows, h, dtype=torch.float64).index_add_(0, idx, x.abs())
    cnt = torch.bincount(idx, minlength=rows)
    return ref, cnt, mag


def _assert_sum_close(out, ref, cnt, mag, what):
    """terms * 2^-24 * sum|x_i| (+ 2^-8 |ref| for a bf16 result); rows that
    receive nothing exactly zero."""
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    bound = cnt.double().reshape(-1, *([1] * (ref.dim() - 1))) * U32 * mag
    if out.dtype == torch.bfloat16:
        bound = bound + BF16_REL * ref.abs()
    err = (out.double() - ref).abs()
    worst = (err - bound).max() if err.numel() else torch.tensor(0.0)
    assert bool((err <= bound).all()), (what, float(worst), float(err.max()))
    empty = cnt == 0
    assert bool((out[empty] == 0).all()), (what, "unused row not zero")


def _idx(n, rows, kind, seed):
    g = _gen(seed)
    if kind == "one_row":          # every index on one row
        return torch.full((n,), rows - 1, dtype=torch.long)
    if kind == "half_unused":      # odd table rows never named
        return torch.randint(0, (rows + 1) // 2, (n,), generator=g) * 2
    if kind == "mega":             # half of the rows of g on table row 0
        idx = torch.randint(0, rows, (n,), generator=g)
        idx[torch.randperm(n, generator=g)[: n // 2]] = 0
        return idx
    return torch.randint(0, rows, (n,), generator=g)


def _strided_cols(ifc, rpc):
    """[n, 4] attribute tensor on the GPU whose columns 0 and 1 are the
    strided index views the model passes."""
    ea = torch.stack([ifc, rpc, torch.ones_like(ifc), torch.zeros_like(ifc)],
                     dim=1).to(DEV)
    return ea


# ---------------------------------------------------------------------------
# _group_by (CPU)
# ---------------------------------------------------------------------------

@pytest.fixture
def clean_group_cache():
    saved, saved_bytes = list(F._GROUP_CACHE.items()), F._GROUP_CACHE_BYTES[0]
    F._GROUP_CACHE.clear()
    F._GROUP_CACHE_BYTES[0] = 0
    yield
    F._GROUP_CACHE.clear()
    F._GROUP_CACHE.update(saved)
    F._GROUP_CACHE_BYTES[0] = saved_bytes


def _check_level(counts, iters_target, row_map, wave_start):
    """every row has max(1, ceil(count / iters_target)) waves, and row_map
    names the row of every wave in wave_start's order"""
    want = torch.clamp_min((counts + iters_target - 1) // iters_target, 1)
    assert wave_start.dtype == torch.int32 and row_map.dtype == torch.int32
    assert int(wave_start[0]) == 0
    assert torch.equal((wave_start[1:] - wave_start[:-1]).long(), want)
    assert row_map.numel() == int(wave_start[-1])
    for r in range(counts.numel()):
        assert bool((row_map[wave_start[r]:wave_start[r + 1]] == r).all())
    return want


GROUP_CASES = {
    # name: (n, rows, kind, iters_target, expects a second level)
    "empty_n0": (0, 5, "uniform", 2, False),
    "one_row_table": (300, 1, "uniform", 2, True),      # 150 waves > 64
    "one_row_table_it64": (300, 1, "uniform", 64, False),   # 5 waves
    "exactly_64_waves": (128, 3, "one_row", 2, False),  # 128/2 = 64, not > 64
    "65_waves": (129, 3, "one_row", 2, True),           # ceil(129/2) = 65
    "mega_half": (600, 40, "mega", 2, True),            # >= 300 on row 0
    "mega_half_it64": (600, 40, "mega", 64, False),
    "half_unused": (17, 40, "half_unused", 2, False),
}


@pytest.mark.parametrize("name", sorted(GROUP_CASES))
def test_group_by_invariants(name, clean_group_cache):
    n, rows, kind, it, has_l2 = GROUP_CASES[name]
    idx = _idx(n, rows, kind, seed=3)
    order, ptr, row_map, wave_start, row_map2, wave_start2 = \
        F._group_by(idx, rows, it)
    counts = torch.bincount(idx, minlength=rows)
    # ptr is the bincount prefix, order a stable argsort
    assert ptr.dtype == torch.int32 and order.dtype == torch.int32
    assert torch.equal(ptr.long(),
                       torch.cat([torch.zeros(1, dtype=torch.long),
                                  counts.cumsum(0)]))
    assert torch.equal(order.long(), torch.argsort(idx, stable=True))
    for r in range(rows):
        members = order[ptr[r]:ptr[r + 1]].long()
        assert bool((idx[members] == r).all())
        assert bool((members[1:] > members[:-1]).all())   # input order kept
    wpr = _check_level(counts, it, row_map, wave_start)
    # a second level exactly when some row has more than 64 waves; it then
    # follows the same rule over the wave counts
    assert (int(wpr.max()) > 64) == has_l2
    if has_l2:
        _check_level(wpr, it, row_map2, wave_start2)
    else:
        assert row_map2.numel() == 0 and wave_start2.numel() == 0


def test_group_by_cache_hit_and_iters_target_in_key(clean_group_cache):
    base = torch.stack([_idx(300, 7, "mega", 5), _idx(300, 7, "uniform", 6)],
                       dim=1)
    view = base[:, 0]                                  # strided column view
    a = F._group_by(view, 7, 2)
    again = F._group_by(base[:, 0], 7, 2)              # same view, new object
    assert all(x is y for x, y in zip(a, again))
    # another target on the same view is another plan
    b = F._group_by(view, 7, 64)
    assert b[2] is not a[2]
    counts = torch.bincount(view, minlength=7)
    _check_level(counts, 2, a[2], a[3])
    _check_level(counts, 64, b[2], b[3])
    assert a[4].numel() > 0 and b[4].numel() == 0      # 150 waves vs 3
    assert all(x is y for x, y in zip(a, F._group_by(view, 7, 2)))
    # other column, other row count, a copy: all misses
    assert F._group_by(base[:, 1], 7, 2)[0] is not a[0]
    assert F._group_by(view, 8, 2)[0] is not a[0]
    assert F._group_by(view.clone(), 7, 2)[0] is not a[0]


def test_group_by_evicts_at_byte_cap(clean_group_cache, monkeypatch):
    i1, i2, i3 = (_idx(200, 10, "uniform", s) for s in (1, 2, 3))
    a = F._group_by(i1, 10, 64)
    one = F._GROUP_CACHE_BYTES[0]
    # order 200 + ptr 11 + one wave per row 10 + wave_start 11, int32
    assert one == (200 + 11 + 10 + 11) * 4 and len(F._GROUP_CACHE) == 1
    monkeypatch.setattr(F, "_GROUP_CACHE_CAP", 2 * one)
    b = F._group_by(i2, 10, 64)
    assert len(F._GROUP_CACHE) == 2 and F._GROUP_CACHE_BYTES[0] == 2 * one
    assert F._group_by(i1, 10, 64)[0] is a[0]          # i1 is now the newest
    F._group_by(i3, 10, 64)                            # evicts i2, the oldest
    assert len(F._GROUP_CACHE) == 2 and F._GROUP_CACHE_BYTES[0] == 2 * one
    assert F._group_by(i1, 10, 64)[0] is a[0]
    assert F._group_by(i2, 10, 64)[0] is not b[0]


# ---------------------------------------------------------------------------
# A. single-table gradient: F._table_grad / _C.vocab_scatter
# ---------------------------------------------------------------------------

TABLE_SHAPES = [
    # (rows, h, branch)
    (80, 128, "priv128_limit"),     # 4*80*128*4 = 163840 = 160 KB exactly
    (81, 128, "priv64_first"),      # 4*81*128*4 = 165888 > 160 KB; 4*81*64*4 = 82944
    (160, 64, "priv64_limit"),      # 4*160*64*4 = 163840
    (161, 64, "fallback_past_priv64"),  # 4*161*64*4 = 164864; 161*64*4 = 41216
    (7, 32, "fallback_h32"),        # h % 64 != 0: LDS-atomic scalar kernel
    (30, 96, "fallback_h96"),       # 96 % 64 != 0; two column rounds per lane
    (1280, 32, "fallback_lds_160k"),    # 1280*32*4 = 163840: > 64 KB attribute
    (1281, 32, "grouped_first"),    # 1281*32*4 = 163968 > 160 KB: _group_by
    (5, 256, "priv128_two_slices"),     # grid.y = 256/128 = 2
    (1, 64, "priv64_one_row"),      # 64 % 128 != 0
]


def _run_table_grad(rows, h, dtype, col_off, n, kind, seed, exact=True):
    m = _C()
    g = (_ints((n, col_off + h), seed) if exact
         else torch.randn(n, col_off + h, generator=_gen(seed)))
    g = g.to(dtype)
    ifc = _idx(n, rows, kind, seed + 1)
    ea = _strided_cols(ifc, _idx(n, rows, "uniform", seed + 2))
    out = F._table_grad(m, g.to(DEV), ea[:, 0], rows, h, col_off)
    assert out.dtype == torch.float32 and out.shape == (rows, h)
    return out.cpu(), _scatter_ref(g, ifc, rows, h, col_off)


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,h,branch", TABLE_SHAPES,
                         ids=[f"{r}x{h}-{b}" for r, h, b in TABLE_SHAPES])
def test_table_grad_exact(rows, h, branch, dtype):
    """bf16 reaches the kernels directly where 4*rows*64*4 <= 160 KB and
    h % 64 == 0, and on the grouped path; (161, 64), (7, 32), (30, 96) and
    (1280, 32) are upcast by ``_table_grad``."""
    for n in N_LIST:
        out, (ref, _, _) = _run_table_grad(rows, h, dtype, 0, n, "uniform",
                                           seed=10 + n)
        assert torch.equal(out, ref.float()), (branch, n)


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", [32, 64, 128])
def test_table_grad_node_embedding_layout_exact(h, dtype):
    """col_off = 9, row stride h + 9 (odd: no packed load is aligned);
    h = 32 fallback, 64 private-64, 128 private-128."""
    for n in N_LIST:
        out, (ref, _, _) = _run_table_grad(40, h, dtype, 9, n, "uniform",
                                           seed=20 + n)
        assert torch.equal(out, ref.float()), n


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["one_row", "half_unused"])
@pytest.mark.parametrize("rows,h", [(80, 128), (160, 64), (30, 96),
                                    (1281, 32)])
def test_table_grad_skewed_indices_exact(rows, h, kind, dtype):
    out, (ref, cnt, _) = _run_table_grad(rows, h, dtype, 0, 1000, kind,
                                         seed=31)
    assert torch.equal(out, ref.float())
    assert int((cnt == 0).sum()) >= rows // 2 and bool((out[cnt == 0] == 0).all())


@gpu
@needs_gpu
def test_table_grad_second_column_is_strided_view():
    """idx = ea[:, 1]: the base pointer is offset by one element"""
    m = _C()
    n, rows, h = 600, 30, 96
    g = _ints((n, h), 40)
    rpc = _idx(n, rows, "uniform", 41)
    ea = _strided_cols(_idx(n, rows, "uniform", 42), rpc)
    for hh, sl in ((96, g), (64, g[:, :64].contiguous())):
        out = F._table_grad(m, sl.to(DEV), ea[:, 1], rows, hh, 0).cpu()
        assert torch.equal(out, _scatter_ref(sl, rpc, rows, hh, 0)[0].float())


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_table_grad_deterministic_mode_takes_grouped_path(dtype, monkeypatch):
    """PERTGNN_DETERMINISTIC=1: the balanced grouped scatter at a shape the
    wave-private kernel would take, bitwise the same twice"""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    m = _C()
    n, rows, h = 1000, 80, 128
    g = torch.randn(n, h, generator=_gen(50)).to(dtype)
    idx = _idx(n, rows, "mega", 51)
    idx_d = idx.to(DEV)
    out = F._table_grad(m, g.to(DEV), idx_d, rows, h, 0).cpu()
    out2 = F._table_grad(m, g.to(DEV), idx_d, rows, h, 0).cpu()
    assert torch.equal(out, out2)
    ref, cnt, mag = _scatter_ref(g, idx, rows, h, 0)
    _assert_sum_close(out, ref, cnt, mag, "deterministic")


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,h,col_off", [
    (80, 128, 0), (160, 64, 0), (161, 64, 0), (30, 96, 0), (1280, 32, 0),
    (1281, 32, 0), (40, 128, 9)])
def test_table_grad_random_normal(rows, h, col_off, dtype):
    out, (ref, cnt, mag) = _run_table_grad(rows, h, dtype, col_off, 1000,
                                           "mega", seed=60, exact=False)
    _assert_sum_close(out, ref, cnt, mag, (rows, h))


@gpu
@needs_gpu
def test_vocab_scatter_binding_refuses_what_it_cannot_run():
    m = _C()
    idx = torch.zeros(4, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):      # 1281*32*4 > 160 KB
        m.vocab_scatter(torch.zeros(4, 32, device=DEV), idx, 1281, 32, 0)
    g16 = torch.zeros(4, 64, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):      # bf16 past the private-64 limit
        m.vocab_scatter(g16, idx, 161, 64, 0)
    with pytest.raises(RuntimeError):      # bf16, h % 64 != 0
        m.vocab_scatter(g16[:, :32].contiguous(), idx, 7, 32, 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# B. dual-table scatter and F._attn_table_grads
# ---------------------------------------------------------------------------

DUAL_SHAPES = [
    # (rows0, rows1, h, branch)
    (47, 5, 256, "priv128"),            # 4*52*128*4 = 106496
    (76, 4, 256, "priv128_limit"),      # 4*80*128*4 = 163840
    (77, 4, 256, "priv64_first"),       # 4*81*128*4 = 165888; 4*81*64*4 = 82944
    (155, 5, 256, "priv64_limit"),      # 4*160*64*4 = 163840 = 160*256*4
    (75, 5, 512, "priv128_four_slices"),    # 80*512*4 = 163840, grid.y = 4
]


def _dual_inputs(n, rows0, rows1, h, dtype, acols, seed, exact=True):
    de = (_ints((n, h), seed) if exact
          else torch.randn(n, h, generator=_gen(seed))).to(dtype)
    ifc = _idx(n, rows0, "mega", seed + 1)
    rpc = _idx(n, rows1, "uniform", seed + 2)
    ea = _strided_cols(ifc, rpc)
    if acols == 2:
        ea = ea[:, :2].contiguous()
    return de, ifc, rpc, ea


@gpu
@needs_gpu
@pytest.mark.parametrize("acols", [2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows0,rows1,h,branch", DUAL_SHAPES,
                         ids=[f"{a}+{b}x{h}-{n}" for a, b, h, n in DUAL_SHAPES])
def test_vocab_scatter_dual_exact(rows0, rows1, h, branch, dtype, acols):
    m = _C()
    for n in N_LIST:
        de, ifc, rpc, ea = _dual_inputs(n, rows0, rows1, h, dtype, acols,
                                        seed=70 + n)
        d0, d1 = m.vocab_scatter_dual(de.to(DEV), ea, rows0, rows1)
        assert d0.dtype == torch.float32 and d0.shape == (rows0, h)
        assert d1.dtype == torch.float32 and d1.shape == (rows1, h)
        assert torch.equal(d0.cpu(),
                           _scatter_ref(de, ifc, rows0, h, 0)[0].float()), n
        assert torch.equal(d1.cpu(),
                           _scatter_ref(de, rpc, rows1, h, 0)[0].float()), n


@gpu
@needs_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows0,rows1,h", [(76, 4, 256), (155, 5, 256),
                                           (75, 5, 512)])
def test_vocab_scatter_dual_random_normal(rows0, rows1, h, dtype):
    m = _C()
    de, ifc, rpc, ea = _dual_inputs(1000, rows0, rows1, h, dtype, 4, seed=80,
                                    exact=False)
    d0, d1 = m.vocab_scatter_dual(de.to(DEV), ea, rows0, rows1)
    _assert_sum_close(d0.cpu(), *_scatter_ref(de, ifc, rows0, h, 0), "ifc")
    _assert_sum_close(d1.cpu(), *_scatter_ref(de, rpc, rows1, h, 0), "rpc")


@gpu
@needs_gpu
def test_vocab_scatter_dual_binding_refuses():
    m = _C()
    ea = torch.zeros(4, 2, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError):      # 161*256*4 > 160 KB
        m.vocab_scatter_dual(torch.zeros(4, 256, device=DEV), ea, 156, 5)
    with pytest.raises(RuntimeError):      # h % 256 != 0
        m.vocab_scatter_dual(torch.zeros(4, 128, device=DEV), ea, 5, 5)
    torch.cuda.synchronize()


ATTN_TABLES = [
    # (V, R, served by) at h = 256
    (155, 5, "dual"),           # 160 rows: 160*256*4 = 163840, the dual scatter
    (156, 5, "two_singles"),    # 161 rows, V*256*4 = 159744 <= 160 KB: two
                                # private-64 single-table scatters
    (161, 5, "edge_table_grad"),    # V*256*4 = 164864 > 160 KB: the list sums
]


@gpu
@needs_gpu
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("tdtype", DTYPES, ids=["p32", "p16"])
@pytest.mark.parametrize("ddtype", DTYPES, ids=["de32", "de16"])
@pytest.mark.parametrize("V,R,path", ATTN_TABLES,
                         ids=[f"{v}+{r}-{p}" for v, r, p in ATTN_TABLES])
def test_attn_table_grads_handover_exact(V, R, path, ddtype, tdtype, det,
                                         monkeypatch):
    """One reference for whichever kernel serves the shape; the gradient
    dtype matches the table (a bf16 table gets the exact fp32 sum rounded
    once).  Under PERTGNN_DETERMINISTIC=1 all three take the list sums."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1" if det else "0")
    m = _C()
    h = 256
    pifc = torch.empty(V, h, dtype=tdtype, device=DEV)
    prpc = torch.empty(R, h, dtype=tdtype, device=DEV)
    for n in (0, 17, 1000):
        de, ifc, rpc, ea = _dual_inputs(n, V, R, h, ddtype, 4, seed=90 + n)
        dp, dr = F._attn_table_grads(m, de.to(DEV), pifc, prpc, ea)
        assert dp.dtype == tdtype and dr.dtype == tdtype
        assert dp.shape == (V, h) and dr.shape == (R, h)
        want_p = _scatter_ref(de, ifc, V, h, 0)[0].float().to(tdtype)
        want_r = _scatter_ref(de, rpc, R, h, 0)[0].float().to(tdtype)
        assert torch.equal(dp.cpu(), want_p), (path, n)
        assert torch.equal(dr.cpu(), want_r), (path, n)


@gpu
@needs_gpu
@pytest.mark.parametrize("tdtype", DTYPES, ids=["p32", "p16"])
@pytest.mark.parametrize("V,R,path", ATTN_TABLES,
                         ids=[f"{v}+{r}-{p}" for v, r, p in ATTN_TABLES])
def test_attn_table_grads_random_normal(V, R, path, tdtype):
    m = _C()
    h = 256
    pifc = torch.empty(V, h, dtype=tdtype, device=DEV)
    prpc = torch.empty(R, h, dtype=tdtype, device=DEV)
    de, ifc, rpc, ea = _dual_inputs(1000, V, R, h, torch.bfloat16, 4, seed=95,
                                    exact=False)
    dp, dr = F._attn_table_grads(m, de.to(DEV), pifc, prpc, ea)
    _assert_sum_close(dp.cpu(), *_scatter_ref(de, ifc, V, h, 0), path)
    _assert_sum_close(dr.cpu(), *_scatter_ref(de, rpc, R, h, 0), path)


# ---------------------------------------------------------------------------
# C. balanced grouped scatter over _group_by plans
# ---------------------------------------------------------------------------

BAL_PLANS = {
    # name: (n, rows, index kind)
    "mega_half_rows_unused": (600, 40, "mega_sparse"),
    "one_table_row": (300, 1, "uniform"),
    "no_gradient_rows": (0, 5, "uniform"),
    "fewer_rows_than_table": (17, 40, "uniform"),
}
# h -> columns per lane vpt = ceil(h/64): 32 -> 1, 96 -> 2 (ragged), 128 -> 2,
# 256 -> 4 (packed loads), 265 -> 5 (ragged), 512 -> 8 (packed loads)
BAL_H = (32, 96, 128, 256, 265, 512)


def _bal_idx(n, rows, kind, seed):
    if kind != "mega_sparse":
        return _idx(n, rows, kind, seed)
    # half of g on table row 0 (> 128 rows: a second level at iters_target
    # 2), the rest on even table rows: odd rows are empty groups
    idx = _idx(n, rows, "half_unused", seed)
    idx[torch.randperm(n, generator=_gen(seed + 7))[: n // 2]] = 0
    return idx


def _run_bal(name, h, dtype, it, col_off, seed, exact=True):
    m = _C()
    n, rows, kind = BAL_PLANS[name]
    g = (_ints((n, col_off + h), seed) if exact
         else torch.randn(n, col_off + h, generator=_gen(seed))).to(dtype)
    idx = _bal_idx(n, rows, kind, seed + 1)
    idx_d = idx.to(DEV)                    # a fresh tensor per target
    plan = F._group_by(idx_d, rows, it)
    counts = torch.bincount(idx, minlength=rows)
    wpr = torch.clamp_min((counts + it - 1) // it, 1)
    assert (plan[4].numel() > 0) == (int(wpr.max()) > 64)
    out = m.embed_grouped_scatter_bal(g.to(DEV), *plan, rows, h, col_off)
    assert out.dtype == torch.float32 and out.shape == (rows, h)
    return out.cpu(), _scatter_ref(g, idx, rows, h, col_off), plan


@gpu
@needs_gpu
@pytest.mark.parametrize("it", [2, 64], ids=["it2", "it64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", BAL_H)
@pytest.mark.parametrize("name", sorted(BAL_PLANS))
def test_grouped_scatter_bal_exact(name, h, dtype, it):
    """iters_target 2 puts the 300-row groups on ceil(300/2) = 150 > 64
    waves (two-level fold); 64 gives 5 (single-level fold)."""
    out, (ref, _, _), plan = _run_bal(name, h, dtype, it, 0, seed=100)
    n = BAL_PLANS[name][0]
    assert (plan[4].numel() > 0) == (it == 2 and n >= 300)
    assert torch.equal(out, ref.float())


@gpu
@needs_gpu
@pytest.mark.parametrize("it", [2, 64], ids=["it2", "it64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_grouped_scatter_bal_node_embedding_layout(dtype, it):
    """col_off = 9, row stride 265, h = 256: the flagship's node-embedding
    gradient; vpt = 4 on the strided scalar mapping (265 % 4 != 0)."""
    out, (ref, _, _), _ = _run_bal("mega_half_rows_unused", 256, dtype, it, 9,
                                   seed=110)
    assert torch.equal(out, ref.float())
    out, (ref, cnt, mag), _ = _run_bal("mega_half_rows_unused", 256, dtype,
                                       it, 9, seed=111, exact=False)
    _assert_sum_close(out, ref, cnt, mag, "col_off 9")


@gpu
@needs_gpu
@pytest.mark.parametrize("it", [2, 64], ids=["it2", "it64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("h", [96, 256])
def test_grouped_scatter_bal_random_normal(h, dtype, it):
    out, (ref, cnt, mag), _ = _run_bal("mega_half_rows_unused", h, dtype, it,
                                       0, seed=120, exact=False)
    _assert_sum_close(out, ref, cnt, mag, (h, it))


@gpu
@needs_gpu
def test_grouped_scatter_unsupported_width_raises():
    """h = 577: vpt = ceil(577/64) = 10, no such instantiation — a Python
    error from both grouped entry points, nothing launched"""
    m = _C()
    n, rows, h = 17, 4, 577
    idx = _idx(n, rows, "uniform", 130).to(DEV)
    plan = F._group_by(idx, rows, 64)
    g = torch.zeros(n, h, device=DEV)
    with pytest.raises(RuntimeError, match="vpt"):
        m.embed_grouped_scatter_bal(g, *plan, rows, h, 0)
    with pytest.raises(RuntimeError, match="vpt"):
        m.embed_grouped_scatter(g, plan[0], plan[1], rows, h, 0)
    torch.cuda.synchronize()


@gpu
@needs_gpu
@pytest.mark.parametrize("h", [96, 256])
@pytest.mark.parametrize("rows", [1, 40])
def test_grouped_scatter_uniform_subwaves_exact(rows, h):
    """the older entry point: P sub-waves per row chosen by the binding
    (rows = 1: min(16384, 300) capped at 256; rows = 40: ceil(300/40) = 8)"""
    m = _C()
    n = 300
    g = _ints((n, h), 140)
    idx = _idx(n, rows, "uniform", 141)
    order, ptr = F._group_by(idx.to(DEV), rows, 64)[:2]
    out = m.embed_grouped_scatter(g.to(DEV), order, ptr, rows, h, 0).cpu()
    assert torch.equal(out, _scatter_ref(g, idx, rows, h, 0)[0].float())


# ---------------------------------------------------------------------------
# D. pattern pool
# ---------------------------------------------------------------------------

POOL_SHAPES = [
    # (b, n, branch); P = clamp(min(8192 // b, ceil(n / b)), 1, 64)
    (1, 1, "P1_single_node"),           # min(8192, 1) = 1
    (1, 200, "P_cap_64"),               # min(8192, 200) = 200 -> 64
    (300, 100, "P1_mostly_empty"),      # min(27, ceil(100/300) = 1) = 1
    (17, 500, "P30_one_node_graph"),    # min(481, ceil(500/17) = 30) = 30
    (0, 0, "no_graphs"),
]
POOL_H = (32, 64, 96, 256, 265, 512)


def _pool_inputs(b, n, h, seed, exact=True):
    """nodes contiguous per graph; graph 0 has exactly one node when there
    are nodes to spare, the rest are spread at random (empty graphs and
    graphs with fewer nodes than P included); weights are powers of two so
    x * p / n is exact"""
    g = _gen(seed)
    if b == 0:
        batch = torch.zeros(0, dtype=torch.long)
    elif b == 1 or n < 2:
        batch = torch.zeros(n, dtype=torch.long)
    else:
        rest = torch.randint(1, b, (n - 1,), generator=g).sort().values
        batch = torch.cat([torch.zeros(1, dtype=torch.long), rest])
    x = (_ints((n, h), seed + 1) if exact
         else torch.randn(n, h, generator=g))
    probs = 2.0 ** -torch.randint(0, 3, (n, 1), generator=g).float()
    nn = 2.0 ** torch.randint(0, 4, (n, 1), generator=g).float()
    gout = (_ints((b, h), seed + 2) if exact
            else torch.randn(b, h, generator=g))
    return x, probs, nn, batch, gout


def _pool_ref(x, probs, nn, batch, gout, b):
    w = (probs / nn).double()
    xw = x.double() * w
    h = x.shape[1]
    out = torch.zeros(b, h, dtype=torch.float64).index_add_(0, batch, xw)
    mag = torch.zeros(b, h, dtype=torch.float64).index_add_(0, batch, xw.abs())
    cnt = torch.bincount(batch, minlength=b)
    dx = gout.double().index_select(0, batch) * w
    return out, cnt, mag, dx


def _batch_ptr(batch, b):
    ptr = torch.zeros(b + 1, dtype=torch.int32)
    ptr[1:] = torch.bincount(batch, minlength=b).cumsum(0).to(torch.int32)
    return ptr.to(DEV)


@gpu
@needs_gpu
@pytest.mark.parametrize("h", POOL_H)
@pytest.mark.parametrize("b,n,branch", POOL_SHAPES,
                         ids=[f"{b}g{n}n-{k}" for b, n, k in POOL_SHAPES])
def test_pattern_pool_exact(b, n, branch, h):
    """forward and backward through F.pattern_pool, then the same through
    the bindings and their bf16 twins (bf16 x in, bf16 dx out)"""
    m = _C()
    x, probs, nn, batch, gout = _pool_inputs(b, n, h, seed=200)
    ref, _, _, dx_ref = _pool_ref(x, probs, nn, batch, gout, b)
    xd = x.to(DEV).requires_grad_(True)
    pd, nd, bd = probs.to(DEV), nn.to(DEV), batch.to(DEV)
    out = F.pattern_pool(xd, pd, nd, bd, b)
    assert out.shape == (b, h) and torch.equal(out.detach().cpu(), ref.float())
    out.backward(gout.to(DEV))
    assert xd.grad.shape == (n, h)
    assert torch.equal(xd.grad.cpu(), dx_ref.float())
    ptr = _batch_ptr(batch, b)
    pc, nc = pd.contiguous(), nd.contiguous()
    assert torch.equal(m.seg_pool_fwd(xd.detach(), pc, nc, ptr, b).cpu(),
                       ref.float())
    out16 = m.seg_pool_fwd16(x.to(torch.bfloat16).to(DEV), pc, nc, ptr, b)
    assert out16.dtype == torch.float32
    assert torch.equal(out16.cpu(), ref.float())
    dx16 = m.seg_pool_bwd16(gout.to(DEV), pc, nc, bd)
    assert dx16.dtype == torch.bfloat16 and dx16.shape == (n, h)
    assert torch.equal(dx16.cpu(), dx_ref.float().to(torch.bfloat16))


@gpu
@needs_gpu
def test_pattern_pool_more_graphs_than_8192():
    """b = n = 8193, h = 32: 8192 // 8193 = 0, clamped to P = 1"""
    m = _C()
    b = n = 8193
    x, probs, nn, _, gout = _pool_inputs(b, n, 32, seed=210)
    batch = torch.arange(n)
    batch[100:200] = 100                   # one graph of 100 nodes, 99 empty
    ref, _, _, dx_ref = _pool_ref(x, probs, nn, batch, gout, b)
    xd = x.to(DEV).requires_grad_(True)
    out = F.pattern_pool(xd, probs.to(DEV), nn.to(DEV), batch.to(DEV), b)
    assert torch.equal(out.detach().cpu(), ref.float())
    out.backward(gout.to(DEV))
    assert torch.equal(xd.grad.cpu(), dx_ref.float())
    out16 = m.seg_pool_fwd16(x.to(torch.bfloat16).to(DEV),
                             probs.to(DEV), nn.to(DEV), _batch_ptr(batch, b), b)
    assert torch.equal(out16.cpu(), ref.float())


@gpu
@needs_gpu
def test_pattern_pool_backward_past_grid_cap():
    """n = 4100, h = 256: 1,049,600 elements > 4096 blocks * 256 lanes =
    1,048,576 — the last 1024 elements come from the second grid pass"""
    m = _C()
    b, n, h = 17, 4100, 256
    x, probs, nn, batch, gout = _pool_inputs(b, n, h, seed=220, exact=False)
    ref, cnt, mag, dx_ref = _pool_ref(x, probs, nn, batch, gout, b)
    pd, nd, bd = probs.to(DEV), nn.to(DEV), batch.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = F.pattern_pool(xd, pd, nd, bd, b)
    _assert_sum_close(out.detach().cpu(), ref, cnt, mag, "pool fwd")
    out.backward(gout.to(DEV))
    # elementwise, weights are powers of two: exact even for random gout
    assert torch.equal(xd.grad.cpu(), dx_ref.float())
    dx16 = m.seg_pool_bwd16(gout.to(DEV), pd, nd, bd)
    assert torch.equal(dx16.cpu(), dx_ref.float().to(torch.bfloat16))


@gpu
@needs_gpu
@pytest.mark.parametrize("b,n", [(1, 200), (17, 500), (300, 100)])
@pytest.mark.parametrize("h", [96, 256])
def test_pattern_pool_random_normal(b, n, h):
    m = _C()
    x, probs, nn, batch, gout = _pool_inputs(b, n, h, seed=230, exact=False)
    ref, cnt, mag, _ = _pool_ref(x, probs, nn, batch, gout, b)
    pd, nd = probs.to(DEV), nn.to(DEV)
    out = F.pattern_pool(x.to(DEV), pd, nd, batch.to(DEV), b)
    _assert_sum_close(out.cpu(), ref, cnt, mag, "fp32 x")
    x16 = x.to(torch.bfloat16)
    ref16, cnt, mag16, _ = _pool_ref(x16, probs, nn, batch, gout, b)
    out16 = m.seg_pool_fwd16(x16.to(DEV), pd, nd, _batch_ptr(batch, b), b)
    _assert_sum_close(out16.cpu(), ref16, cnt, mag16, "bf16 x")


@gpu
@needs_gpu
def test_pattern_pool_too_wide_raises():
    """h = 577 > 512: vpt = 10 has no instantiation"""
    m = _C()
    b, n, h = 3, 10, 577
    x, probs, nn, batch, _ = _pool_inputs(b, n, h, seed=240)
    args = (probs.to(DEV), nn.to(DEV), batch.to(DEV), b)
    with pytest.raises(RuntimeError, match="vpt"):
        F.pattern_pool(x.to(DEV), *args)
    with pytest.raises(RuntimeError, match="vpt"):
        m.seg_pool_fwd16(x.to(torch.bfloat16).to(DEV), args[0], args[1],
                         _batch_ptr(batch, b), b)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# E. gathers (copies: bit-equal)
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("out16", [False, True], ids=["fp32", "out16"])
@pytest.mark.parametrize("n,h", [(0, 32), (1, 32), (300, 32), (0, 128),
                                 (1, 128), (300, 128), (0, 256), (1, 256),
                                 (300, 256),
                                 (4000, 256)])   # 4000*265 = 1,060,000 > 1,048,576
def test_embed_concat_node_is_a_copy(n, h, out16):
    _C()
    f, rows = 9, 50
    x_raw = torch.randn(n, f, generator=_gen(300))
    table = torch.randn(rows, h, generator=_gen(301))
    cat = torch.stack([_idx(n, rows, "uniform", 302),
                       torch.zeros(n, dtype=torch.long)], dim=1)
    out = F.embed_concat_node(x_raw.to(DEV), cat.to(DEV), [table.to(DEV)],
                              out16)
    want = torch.cat([x_raw, table.index_select(0, cat[:, 0])], dim=1)
    if out16:
        want = want.to(torch.bfloat16)
    assert out.dtype == want.dtype and out.shape == (n, f + h)
    assert torch.equal(out.cpu(), want)


@gpu
@needs_gpu
@pytest.mark.parametrize("acols", [2, 4])
@pytest.mark.parametrize("e", [0, 1, 800])
@pytest.mark.parametrize("h", [32, 256])
def test_embed_concat_edge_is_a_copy(e, h, acols):
    _C()
    V, R = 47, 5
    ifc_t = torch.randn(V, h, generator=_gen(310))
    rpc_t = torch.randn(R, h, generator=_gen(311))
    ifc, rpc = _idx(e, V, "mega", 312), _idx(e, R, "uniform", 313)
    ea = _strided_cols(ifc, rpc)
    if acols == 2:
        ea = ea[:, :2].contiguous()
    out = F.embed_concat_edge(ea, ifc_t.to(DEV), rpc_t.to(DEV))
    want = torch.cat([ifc_t.index_select(0, ifc),
                      rpc_t.index_select(0, rpc)], dim=1)
    assert out.shape == (e, 2 * h) and torch.equal(out.cpu(), want)


@gpu
@needs_gpu
@pytest.mark.parametrize("n,h", [(0, 64), (1, 64), (100, 64), (100, 96),
                                 (4200, 256)])   # 1,075,200 > 1,048,576
def test_embedding_is_a_copy(n, h):
    _C()
    rows = 33
    table = torch.randn(rows, h, generator=_gen(320))
    idx = _idx(n, rows, "uniform", 321)
    out = F.embedding(idx.to(DEV), table.to(DEV))
    assert out.shape == (n, h)
    assert torch.equal(out.cpu(), table.index_select(0, idx))


# ---------------------------------------------------------------------------
# F. quantile loss and eval metrics
# ---------------------------------------------------------------------------

LOSS_B = (1, 255, 256, 257, 65539)
# 255/256/257: one block short of full, full, one element in a second block;
# 65539 > 256 blocks * 256 lanes = 65536: three lanes take a second element
TAUS = (0.1, 0.5, 0.9)
UPSTREAM = 1024.0     # the loss scale


def _loss_inputs(b, seed):
    """y in [1, 3] (bounded away from 0 for MAPE); a quarter of the elements
    tie exactly (y == y_hat)"""
    g = _gen(seed)
    y = 1.0 + 2.0 * torch.rand(b, generator=g)
    y_hat = y + torch.randn(b, generator=g)
    tie = torch.arange(b) % 4 == 0
    y_hat[tie] = y[tie]
    return y, y_hat, tie


def _pinball_terms(y, y_hat, tau):
    """The summands as the kernel forms them: fp32 subtract, fp32 tau - 1,
    two fp32 products, max.  These are single IEEE operations with nothing
    to contract, so the CPU gives the same bits; the reference sums them in
    fp64 and the bound is for the summation alone, as the formula says."""
    t = torch.tensor(tau, dtype=torch.float32)
    e = y - y_hat
    return torch.maximum(t * e, (t - 1.0) * e)


def _ulp32(ref64):
    a = ref64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


@gpu
@needs_gpu
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("b", LOSS_B)
def test_quantile_loss_forward_and_backward(b, tau):
    y, y_hat, tie = _loss_inputs(b, seed=400 + b)
    yh = y_hat.to(DEV).requires_grad_(True)
    loss = F.quantile_loss(y.to(DEV), yh, tau)
    x = _pinball_terms(y, y_hat, tau).double()
    ref = x.sum() / b
    # b terms: b - 1 additions in any order, one division by b
    bound = b * U32 * x.abs().sum() / b
    assert abs(float(loss.detach().cpu().double()) - float(ref)) <= float(bound), \
        (float(loss), float(ref), float(bound))
    (loss * UPSTREAM).backward()
    got = yh.grad.cpu()
    # fp64 formula on the fp32 tau the kernel receives
    t = float(torch.tensor(tau, dtype=torch.float32))
    e = y.double() - y_hat.double()
    d = torch.where(e > 0, torch.full_like(e, -t),
                    torch.where(e < 0, torch.full_like(e, 1.0 - t),
                                torch.full_like(e, 0.5 - t)))
    want = UPSTREAM / b * d
    assert bool((e[tie] == 0).all()) and int(tie.sum()) == (b + 3) // 4
    err = (got.double() - want).abs()
    assert bool((err <= 2 * _ulp32(want)).all()), \
        float((err / _ulp32(want)).max())


@gpu
@needs_gpu
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("b", LOSS_B)
def test_eval_metrics_sums(b, tau):
    y, y_hat, _ = _loss_inputs(b, seed=450 + b)
    got = F.eval_metrics(y.to(DEV), y_hat.to(DEV), tau)
    a = (y_hat - y).abs()
    # fp32 elementwise terms (|err|, the correctly rounded |err| / y, the
    # pinball term), summed in fp64
    terms = (a, a / y, _pinball_terms(y, y_hat, tau))
    for name, val, x in zip(("mae", "mape", "pinball"), got, terms):
        x = x.double()
        bound = b * U32 * x.abs().sum()
        assert abs(float(val.cpu().double()) - float(x.sum())) <= float(bound), \
            (name, float(val), float(x.sum()), float(bound))


@gpu
@needs_gpu
def test_loss_and_metrics_on_an_empty_batch():
    """nothing is launched: the mean over no elements is NaN, as
    reference.quantile_loss gives on the CPU; its gradient is empty; the
    metric sums are three zeros"""
    from pertgnn.ops import reference as ref
    y = torch.zeros(0, device=DEV)
    yh = torch.zeros(0, device=DEV, requires_grad=True)
    loss = F.quantile_loss(y, yh, 0.7)
    assert loss.shape == () and bool(torch.isnan(loss))
    assert bool(torch.isnan(ref.quantile_loss(y.cpu(), yh.detach().cpu(), 0.7)))
    loss.backward()
    assert yh.grad.shape == (0,)
    got = F.eval_metrics(y, yh.detach(), 0.7)
    want = ref.eval_metrics(y.cpu(), yh.detach().cpu(), 0.7)
    assert [float(v) for v in got] == [0.0, 0.0, 0.0]
    assert [float(v) for v in want] == [0.0, 0.0, 0.0]
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# G. Adam and the dynamic loss scaler
# ---------------------------------------------------------------------------

ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
BIG = 1_048_653       # 4096 blocks * 256 lanes = 1,048,576, plus 77


def _adam_ref(p0, grad, steps):
    """torch Adam in fp64: final p and the sum over steps of |delta p|"""
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]),
                           eps=ADAM["eps"])
    moved = torch.zeros_like(p0, dtype=torch.float64)
    for _ in range(steps):
        before = p.detach().clone()
        p.grad = grad.double().clone()
        opt.step()
        moved += (p.detach() - before).abs()
    return p.detach(), moved


@gpu
@needs_gpu
@pytest.mark.parametrize("prescale", [1.0, 1024.0], ids=["gscale1", "gscale1_1024"])
@pytest.mark.parametrize("numel", [1, 255, BIG])
def test_adam_step_three_steps(numel, prescale):
    """Per element: sum_steps |dp_ref| * 2^-12 + 2 * steps * 2^-24 * |p_ref|.
    The first term is four times the fp32 cancellation in 1 - powf(0.999, t)
    at t = 1 (about 6e-5 relative); a skipped element or a wrong bias
    correction is off by |dp| itself."""
    m = _C()
    steps = 3
    p0 = torch.randn(numel, generator=_gen(500))
    grad = torch.randn(numel, generator=_gen(501))
    p_ref, moved = _adam_ref(p0, grad, steps)
    p = p0.clone().to(DEV)
    mom = torch.zeros(numel, device=DEV)
    var = torch.zeros(numel, device=DEV)
    state = torch.zeros(3, device=DEV)
    g_in = (grad * prescale).to(DEV)       # exact: a power of two
    for _ in range(steps):
        m.adam_step(p, g_in, mom, var, state, ADAM["lr"], ADAM["b1"],
                    ADAM["b2"], ADAM["eps"], 1.0 / prescale)
    assert float(state[0]) == steps
    bound = moved * 2.0 ** -12 + 2 * steps * U32 * p_ref.abs()
    err = (p.cpu().double() - p_ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    # and every element did move
    assert bool(((p.cpu() - p0).abs() > 0.5 * moved.float()).all())


def _dyn_buffers(numel, scale, counter, seed=510):
    p = torch.randn(numel, generator=_gen(seed)).to(DEV)
    mom = (0.1 * torch.randn(numel, generator=_gen(seed + 1))).to(DEV)
    var = (0.01 * torch.rand(numel, generator=_gen(seed + 2))).to(DEV)
    state = torch.tensor([2.0, 1 - 0.9 ** 2, 1 - 0.999 ** 2], device=DEV)
    sstate = torch.tensor([scale, counter, 0.0], device=DEV)
    return p, mom, var, state, sstate


def _dyn_step(m, bufs, g, backoff=0.5, growth=2.0, interval=3.0):
    p, mom, var, state, sstate = bufs
    m.adam_step_dynamic(p, g, mom, var, state, sstate, ADAM["lr"], ADAM["b1"],
                        ADAM["b2"], ADAM["eps"], backoff, growth, interval)


@gpu
@needs_gpu
@pytest.mark.parametrize("where,bad", [("last", float("inf")),
                                       ("first", float("nan")),
                                       ("middle", float("-inf"))])
@pytest.mark.parametrize("scale,want_scale", [(1024.0, 512.0), (1.5, 1.0)],
                         ids=["backoff", "floor_at_1"])
def test_adam_dynamic_skips_on_one_non_finite(where, bad, scale, want_scale):
    """one bad value among 1,048,653; the last element is only seen by the
    second pass of the scan's grid-stride loop (index 1,048,652 >= 1,048,576)"""
    m = _C()
    bufs = _dyn_buffers(BIG, scale, counter=2.0)
    before = [t.clone() for t in bufs[:4]]
    g = torch.randn(BIG, generator=_gen(520)).to(DEV)
    g[{"last": BIG - 1, "first": 0, "middle": BIG // 2}[where]] = bad
    _dyn_step(m, bufs, g)
    for name, now, was in zip("p m v state".split(), bufs[:4], before):
        assert torch.equal(now, was), name         # bit-unchanged
    sstate = bufs[4].cpu()
    assert float(sstate[0]) == want_scale          # backoff 0.5, never < 1
    assert float(sstate[1]) == 0.0                 # clean-step counter reset
    assert float(sstate[2]) == 1.0
    # the next clean step does update, with the reduced scale
    g_clean = torch.randn(BIG, generator=_gen(521)).to(DEV)
    _dyn_step(m, bufs, g_clean)
    assert float(bufs[3][0]) == 3.0 and float(bufs[4][1]) == 1.0
    assert float(bufs[4][2]) == 0.0
    # 0.9 m + 0.1 g == m needs g == m to ~1e-6 relative: well under one
    # element in a million
    assert int((bufs[1] == before[1]).sum()) < 16


@gpu
@needs_gpu
def test_adam_dynamic_clean_step_matches_reference_past_grid_cap():
    """a clean dynamic step unscales by 1 / sstate[0] and is one Adam step"""
    m = _C()
    p0 = torch.randn(BIG, generator=_gen(530))
    grad = torch.randn(BIG, generator=_gen(531))
    p_ref, moved = _adam_ref(p0, grad, 1)
    p = p0.clone().to(DEV)
    bufs = (p, torch.zeros(BIG, device=DEV), torch.zeros(BIG, device=DEV),
            torch.zeros(3, device=DEV),
            torch.tensor([1024.0, 0.0, 0.0], device=DEV))
    _dyn_step(m, bufs, (grad * 1024.0).to(DEV))
    bound = moved * 2.0 ** -12 + 2 * U32 * p_ref.abs()
    err = (p.cpu().double() - p_ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


@gpu
@needs_gpu
def test_adam_dynamic_growth_interval_and_cap():
    m = _C()
    numel = 255
    g = torch.randn(numel, generator=_gen(540)).to(DEV)
    bufs = _dyn_buffers(numel, 1024.0, counter=0.0)
    seen = []
    for _ in range(7):                     # interval 3: grows after 3 and 6
        _dyn_step(m, bufs, g)
        seen.append((float(bufs[4][0]), float(bufs[4][1])))
    assert seen == [(1024.0, 1.0), (1024.0, 2.0), (2048.0, 0.0),
                    (2048.0, 1.0), (2048.0, 2.0), (4096.0, 0.0),
                    (4096.0, 1.0)]
    assert float(bufs[3][0]) == 2.0 + 7
    # growth stops at 2^32: 3 * 2^30 * 2 is capped, 2^32 stays
    bufs = _dyn_buffers(numel, 3.0 * 2.0 ** 30, counter=2.0)
    _dyn_step(m, bufs, g)
    assert (float(bufs[4][0]), float(bufs[4][1])) == (2.0 ** 32, 0.0)
    bufs[4][1] = 2.0
    _dyn_step(m, bufs, g)
    assert (float(bufs[4][0]), float(bufs[4][1])) == (2.0 ** 32, 0.0)
