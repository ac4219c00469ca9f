"""The extended Adam step on the GPU (``adam_step_ex``): the global gradient
norm, clipping, decoupled weight decay, the learning-rate table, the device
statistics, hipGraph capture, and FusedAdam / GraphStepper on top of them.

Conventions of tests/test_segops_edges.py section G: seeded generators,
BIG = 1,048,653 (one more than 4096 blocks x 256 lanes, plus 76), U32 = 2^-24.
The fp64 references take the hyper-parameters as the kernels receive them
(rounded to fp32): 1 - fl32(0.9) differs from 0.1 by 4 * 2^-24 relative, which
is the whole bound of the moment checks and no property of the kernel.
"""
import math

import numpy as np
import pytest
import torch

from pertgnn.ops.backend import ext, require_ext

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

U32 = 2.0 ** -24
BIG = 1_048_653
INF = float("inf")


def f32(x):
    return float(np.float32(x))


ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def _C():
    require_ext()
    return ext()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _hstate():
    h = torch.zeros(8, device=DEV)
    h[1] = 1.0
    return h


def _slab():
    # never initialised by the caller: the kernels must not rely on a memset
    return torch.full((4096,), float("nan"), device=DEV)


def _ex(m, p, g, mom, var, state, hstate, slab=None, sstate=None, mask=None,
        table=None, lr=ADAM["lr"], gscale=1.0, wd=0.0, max_norm=INF,
        backoff=0.5, growth=2.0, interval=3.0):
    m.adam_step_ex(p, g, mom, var, state, sstate, hstate,
                   _slab() if slab is None else slab, mask, table, lr,
                   ADAM["b1"], ADAM["b2"], ADAM["eps"], gscale, wd, max_norm,
                   backoff, growth, interval)


def _zeros(numel):
    return (torch.zeros(numel, device=DEV), torch.zeros(numel, device=DEV),
            torch.zeros(numel, device=DEV), torch.zeros(3, device=DEV))


def _norm_of(m, g, gscale=1.0):
    """the norm the extended step reports for g (one step on zero buffers)"""
    p, mom, var, state = _zeros(g.numel())
    h = _hstate()
    _ex(m, p, g, mom, var, state, h, gscale=gscale)
    return h.cpu()


def _moments(numel, seed=510):
    """non-zero moments at step 2, as section G's _dyn_buffers"""
    p = torch.randn(numel, generator=_gen(seed))
    mom = 0.1 * torch.randn(numel, generator=_gen(seed + 1))
    var = 0.01 * torch.rand(numel, generator=_gen(seed + 2))
    state = torch.tensor([2.0, 1 - 0.9 ** 2, 1 - 0.999 ** 2])
    return p, mom, var, state


def _adam64(p, mom, var, g, t, lr, decay=None):
    """One fp64 Adam step at step count t (torch.optim.Adam / AdamW math) on
    fp64 tensors; ``decay`` is the factor 1 - lr * wd per element or None.
    Returns (p, m, v, |delta p|)."""
    p0 = p
    if decay is not None:
        p = p * decay
    mom = B1 * mom + (1 - B1) * g
    var = B2 * var + (1 - B2) * g * g
    denom = var.sqrt() / math.sqrt(1 - B2 ** t) + EPS
    p = p - (lr / (1 - B1 ** t)) * mom / denom
    return p, mom, var, (p - p0).abs()


# ---------------------------------------------------------------------------
# the norm
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("variant", ["plain", "view", "gscale"])
@pytest.mark.parametrize("numel", [1, 3, 255, 1027, BIG])
def test_norm_exact(numel, variant):
    """integers in [-3, 3]: the sum of squares stays below 2^24 at BIG, so
    it is exact in fp32 in any order and the norm is one correctly rounded
    square root.  'view' starts 4 bytes past a 16-byte boundary; 'gscale'
    unscales g * 1024 by 1/1024 before squaring."""
    m = _C()
    g = torch.randint(-3, 4, (numel,), generator=_gen(600 + numel % 97)).float()
    want = f32(math.sqrt(float((g.double() ** 2).sum())))
    if variant == "view":
        buf = torch.full((numel + 1,), 100.0)   # a stray read of [0] shows
        buf[1:] = g
        dev = buf.to(DEV)[1:]
        assert dev.data_ptr() % 16 == 4
        h = _norm_of(m, dev)
    elif variant == "gscale":
        h = _norm_of(m, (g * 1024.0).to(DEV), gscale=1.0 / 1024.0)
    else:
        h = _norm_of(m, g.to(DEV))
    assert float(h[2]) == want, (float(h[2]), want)
    assert float(h[1]) == 1.0 and float(h[6]) == 1.0 and float(h[5]) == 0.0


@gpu
@needs_gpu
@pytest.mark.parametrize("where", [0, BIG - 1, 1_048_576])
def test_norm_finds_a_single_non_zero(where):
    """index 1,048,576 is the first element past 4096 blocks x 256 lanes"""
    m = _C()
    g = torch.zeros(BIG)
    g[where] = 3.0
    assert float(_norm_of(m, g.to(DEV))[2]) == 3.0


@gpu
@needs_gpu
def test_norm_random_and_reproducible():
    m = _C()
    g = torch.randn(BIG, generator=_gen(610))
    sumsq = float((g.double() ** 2).sum())
    slabs = [_slab(), _slab()]
    hs = []
    for slab in slabs:
        p, mom, var, state = _zeros(BIG)
        h = _hstate()
        _ex(m, p, g.to(DEV), mom, var, state, h, slab=slab)
        hs.append(h.cpu())
    got = float(hs[0][2].double()) ** 2
    print("norm^2", got, "fp64", sumsq, "rel", abs(got - sumsq) / sumsq)
    assert abs(got - sumsq) <= BIG * U32 * sumsq
    # a far tighter figure than the bound asked for: the value is sane
    assert abs(got - sumsq) <= 1e-5 * sumsq
    assert torch.equal(hs[0], hs[1])
    used = ~torch.isnan(slabs[0])
    assert torch.equal(slabs[0][used], slabs[1][used])
    assert torch.equal(used, ~torch.isnan(slabs[1]))


# ---------------------------------------------------------------------------
# with every feature neutral the step is the plain kernel's, to the bit
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("numel", [255, BIG])
def test_neutral_path_equals_adam_step(numel):
    m = _C()
    p0 = torch.randn(numel, generator=_gen(620))
    grad = torch.randn(numel, generator=_gen(621)).to(DEV)
    a = (p0.clone().to(DEV),) + _zeros(numel)[1:]
    b = (p0.clone().to(DEV),) + _zeros(numel)[1:]
    h = _hstate()
    for _ in range(3):
        m.adam_step(a[0], grad, a[1], a[2], a[3], ADAM["lr"], ADAM["b1"],
                    ADAM["b2"], ADAM["eps"], 1.0)
        _ex(m, b[0], grad, b[1], b[2], b[3], h)
    for name, x, y in zip("p m v state".split(), a, b):
        assert torch.equal(x, y), name
    assert float(h[0]) == f32(ADAM["lr"]) and float(h[6]) == 3.0


@gpu
@needs_gpu
@pytest.mark.parametrize("numel", [255, BIG])
def test_neutral_path_equals_adam_step_dynamic(numel):
    """scale 1024 growing to 2048 at the third step (interval 3)"""
    m = _C()
    grad = (torch.randn(numel, generator=_gen(631)) * 1024.0).to(DEV)
    runs = []
    for _ in range(2):
        p, mom, var, state = (t.to(DEV) for t in _moments(numel, seed=630))
        runs.append((p, mom, var, state,
                     torch.tensor([1024.0, 0.0, 0.0], device=DEV)))
    a, b = runs
    h = _hstate()
    for _ in range(3):
        m.adam_step_dynamic(a[0], grad, a[1], a[2], a[3], a[4], ADAM["lr"],
                            ADAM["b1"], ADAM["b2"], ADAM["eps"], 0.5, 2.0, 3.0)
        _ex(m, b[0], grad, b[1], b[2], b[3], h, sstate=b[4])
    for name, x, y in zip("p m v state sstate".split(), a, b):
        assert torch.equal(x, y), name
    assert float(b[4][0]) == 2048.0 and float(b[3][0]) == 5.0


# ---------------------------------------------------------------------------
# clipping
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("numel", [1027, BIG])
def test_clipping(numel):
    """max_norm at half the norm, from non-zero moments (Adam's first step
    from zero moments is invariant to the gradient's scale).

    coefficient: bit-equal to torch's fp32 expression on the reported norm.
    m, v: within 4 * 2^-24 * (|b1 m0| + |(1 - b1) g coef|) (v likewise) of
    fp64 with the reported fp32 coefficient - per element the kernel rounds
    g * coef, the product with 1 - b, the product b * m0 and the sum (v: one
    product more), which that bound covers; the coefficient itself is held
    to the fp64 one separately, within the 4 roundings (norm, sum, quotient,
    and the fp32 partial sums) that produce it.
    p: section G's bound against fp64 clip_grad_norm_ + Adam throughout."""
    m = _C()
    p0, m0, v0, state0 = _moments(numel, seed=640)
    g = torch.randn(numel, generator=_gen(643))
    norm64 = math.sqrt(float((g.double() ** 2).sum()))
    max_norm = f32(norm64 / 2)

    def run(mx):
        bufs = [t.clone().to(DEV) for t in (p0, m0, v0, state0)]
        h = _hstate()
        _ex(m, bufs[0], g.to(DEV), bufs[1], bufs[2], bufs[3], h, max_norm=mx)
        return [t.cpu() for t in bufs], h.cpu()

    (p, mom, var, state), h = run(max_norm)
    want_coef = torch.clamp(
        torch.tensor(max_norm, dtype=torch.float32) / (h[2] + 1e-6), max=1.0)
    assert float(h[1]) == float(want_coef)
    coef64 = max_norm / (norm64 + 1e-6)
    assert abs(float(h[1]) - coef64) <= 4 * U32 * coef64
    assert float(h[5]) == 1.0 and float(h[6]) == 1.0 and float(state[0]) == 3.0

    coef = float(h[1].double())
    gd, md, vd = g.double(), m0.double(), v0.double()
    _, m_ref, v_ref, _ = _adam64(p0.double(), md, vd, gd * coef, 3, ADAM["lr"])
    m_bound = 4 * U32 * ((B1 * md).abs() + ((1 - B1) * gd * coef).abs())
    v_bound = 4 * U32 * ((B2 * vd).abs() + ((1 - B2) * gd * gd * coef * coef))
    m_err = (mom.double() - m_ref).abs()
    v_err = (var.double() - v_ref).abs()
    print("m err/bound", float((m_err / m_bound).max()),
          "v err/bound", float((v_err / v_bound).max()))
    assert bool((m_err <= m_bound).all())
    assert bool((v_err <= v_bound).all())

    # p: fp64 throughout, the clip by torch itself
    g_ref = torch.nn.Parameter(p0.double().clone())
    g_ref.grad = gd.clone()
    torch.nn.utils.clip_grad_norm_([g_ref], max_norm)
    p_ref, _, _, moved = _adam64(p0.double(), md, vd, g_ref.grad, 3, ADAM["lr"])
    bound = moved * 2.0 ** -12 + 2 * U32 * p_ref.abs()
    err = (p.double() - p_ref).abs()
    print("p err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())

    # the clip is what made the difference: an unclipped run is off by more
    # than the bound nearly everywhere (a condition on the seeds, checked on
    # the references first)
    _, m_unclipped, _, _ = _adam64(p0.double(), md, vd, gd, 3, ADAM["lr"])
    assert float(((m_unclipped - m_ref).abs() > 2 * m_bound).double().mean()) >= 0.99
    (_, mom_u, _, _), h_u = run(INF)
    assert float(((mom_u.double() - m_ref).abs() > m_bound).double().mean()) >= 0.99
    assert float(h_u[1]) == 1.0 and float(h_u[5]) == 0.0

    # twice the norm: the coefficient is exactly 1, nothing counts as clipped
    (_, mom_2, _, _), h_2 = run(f32(norm64 * 2))
    assert float(h_2[1]) == 1.0 and float(h_2[5]) == 0.0
    assert torch.equal(mom_2, mom_u)


# ---------------------------------------------------------------------------
# decoupled weight decay
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("numel", [1100, BIG])
def test_weight_decay_follows_the_mask(numel):
    """mask boundaries at 5, 1030 and 1033: inside 16-byte groups of four"""
    m = _C()
    lr, wd, steps = 1e-2, 0.1, 3
    mask = torch.zeros(numel, dtype=torch.uint8)
    mask[0:5] = 1
    mask[1030:1033] = 1
    on = mask.bool()
    p0 = torch.randn(numel, generator=_gen(650))
    g = torch.randn(numel, generator=_gen(651))

    def run(wd_, mask_):
        p, mom, var, state = _zeros(numel)
        p.copy_(p0)
        h = _hstate()
        for _ in range(steps):
            _ex(m, p, g.to(DEV), mom, var, state, h, lr=lr, wd=wd_,
                mask=mask_)
        return p.cpu()

    p_wd = run(wd, mask.to(DEV))
    p_plain = run(0.0, None)
    assert torch.equal(p_wd[~on], p_plain[~on])

    def ref(weight_decay):
        q = p0[on].double().clone().requires_grad_(True)
        opt = torch.optim.AdamW([q], lr=f32(lr), betas=(B1, B2), eps=EPS,
                                weight_decay=weight_decay)
        moved = torch.zeros_like(q)
        for _ in range(steps):
            before = q.detach().clone()
            q.grad = g[on].double().clone()
            opt.step()
            moved += (q.detach() - before).abs()
        return q.detach(), moved.detach()

    p_ref, moved = ref(f32(wd))
    p_undecayed, _ = ref(0.0)
    bound = moved * 2.0 ** -12 + 2 * steps * U32 * p_ref.abs()
    err = (p_wd[on].double() - p_ref).abs()
    print("err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())
    # the seeds keep the decayed values apart from the undecayed ones
    assert bool(((p_ref - p_undecayed).abs() > 2 * bound).all())
    assert bool(((p_wd[on].double() - p_undecayed).abs() > bound).all())


# ---------------------------------------------------------------------------
# the learning-rate table
# ---------------------------------------------------------------------------

TABLE = [1e-3, 3e-3, 2e-3, 5e-4, 1e-4]


@gpu
@needs_gpu
def test_schedule_walks_the_table_and_clamps_at_its_end():
    m = _C()
    numel, steps = 255, 7
    table = torch.tensor(TABLE, dtype=torch.float32)
    p0 = torch.randn(numel, generator=_gen(660))
    g = torch.randn(numel, generator=_gen(661))
    p, mom, var, state = _zeros(numel)
    p.copy_(p0)
    h = _hstate()
    ref = (p0.double(), torch.zeros(numel, dtype=torch.float64),
           torch.zeros(numel, dtype=torch.float64))
    moved = torch.zeros(numel, dtype=torch.float64)
    for t in range(1, steps + 1):
        _ex(m, p, g.to(DEV), mom, var, state, h, table=table.to(DEV),
            lr=123.0)                      # the by-value rate is not used
        want = table[min(t, 5) - 1]
        assert float(h[0]) == float(want), t
        *ref, d = _adam64(*ref, g.double(), t, float(want.double()))
        moved += d
    bound = moved * 2.0 ** -12 + 2 * steps * U32 * ref[0].abs()
    err = (p.cpu().double() - ref[0]).abs()
    print("err/bound", float((err / bound).max()))
    assert bool((err <= bound).all())


@gpu
@needs_gpu
def test_skipped_dynamic_step_holds_the_schedule_and_the_statistics():
    m = _C()
    numel = 1027
    table = torch.tensor(TABLE, dtype=torch.float32).to(DEV)
    p, mom, var, state = (t.to(DEV) for t in _moments(numel, seed=670))
    sstate = torch.tensor([1024.0, 0.0, 0.0], device=DEV)
    h = _hstate()
    g = (torch.randn(numel, generator=_gen(673)) * 1024.0).to(DEV)

    def step(grad):
        _ex(m, p, grad, mom, var, state, h, sstate=sstate, table=table,
            max_norm=1.0, interval=100.0)

    step(g)                                 # t = 3
    assert float(state[0]) == 3.0 and float(h[0]) == f32(TABLE[2])
    before = [t.clone() for t in (p, mom, var, state, h)]
    bad = g.clone()
    bad[numel // 2] = INF
    step(bad)                               # skipped
    for name, now, was in zip("p m v state".split(), (p, mom, var, state),
                              before):
        assert torch.equal(now, was), name
    assert float(h[0]) == float(before[4][0])
    assert torch.equal(h[3:7], before[4][3:7])
    assert float(sstate[0]) == 512.0 and float(sstate[2]) == 1.0
    step(g)                                 # t = 4: the entry the skip left
    assert float(state[0]) == 4.0 and float(h[0]) == f32(TABLE[3])
    assert float(h[6]) == 2.0
    assert not torch.equal(p, before[0])


# ---------------------------------------------------------------------------
# statistics, non-finite gradients, empty input
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
def test_statistics_are_exact_and_grad_stats_resets_them():
    from pertgnn.train.optim import FusedAdam

    require_ext()
    w = torch.nn.Parameter(torch.zeros(13, 79, device=DEV))   # 1027 elements
    opt = FusedAdam([w], lr=1e-3, max_grad_norm=11.0)
    for a, b in ((3.0, 4.0), (5.0, 12.0), (6.0, 8.0), (8.0, 15.0)):
        opt.zero_grad()
        opt.flat_grad[7] = a
        opt.flat_grad[1026] = b
        opt.step()
    h = opt.hstate.cpu()
    assert h[2:7].tolist() == [17.0, 45.0, 17.0, 2.0, 4.0]
    stats = opt.grad_stats(reset=True)
    assert stats == {"lr": f32(1e-3), "norm_last": 17.0, "norm_mean": 11.25,
                     "norm_max": 17.0, "clipped_frac": 0.5, "steps": 4}
    assert opt.hstate[3:7].cpu().tolist() == [0.0] * 4
    again = opt.grad_stats()
    assert again["steps"] == 0 and again["norm_mean"] == 0.0
    assert again["lr"] == f32(1e-3) and again["norm_last"] == 17.0
    assert opt.grad_stats(reset=False)["steps"] == 0


@gpu
@needs_gpu
def test_non_finite_gradient_on_the_static_path():
    """torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): the norm
    is inf, the coefficient max_norm / inf = 0, finite gradients become 0
    and the infinite one 0 * inf = NaN."""
    m = _C()
    numel = 1027
    p0, m0, v0, state0 = _moments(numel, seed=680)
    g = torch.randn(numel, generator=_gen(683))
    g[600] = INF
    bufs = [t.clone().to(DEV) for t in (p0, m0, v0, state0)]
    h = _hstate()
    _ex(m, bufs[0], g.to(DEV), bufs[1], bufs[2], bufs[3], h, max_norm=1.0)
    torch.cuda.synchronize()
    p, mom, var, state = (t.cpu() for t in bufs)
    assert float(h[2]) == INF and float(h[1]) == 0.0
    ok = torch.ones(numel, dtype=torch.bool)
    ok[600] = False
    assert torch.equal(mom[ok], (torch.tensor(B1, dtype=torch.float32) * m0)[ok])
    assert bool(torch.isfinite(p[ok]).all()) and bool(torch.isfinite(var[ok]).all())
    assert bool(torch.isnan(mom[600])) and bool(torch.isnan(p[600]))
    # the reference behaviour itself
    q = torch.nn.Parameter(p0.clone())
    q.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([q], 1.0, error_if_nonfinite=False)
    assert float(total) == INF
    assert bool((q.grad[ok] == 0).all()) and bool(torch.isnan(q.grad[600]))
    # without clipping the norm is still reported
    bufs = [t.clone().to(DEV) for t in (p0, m0, v0, state0)]
    h = _hstate()
    _ex(m, bufs[0], g.to(DEV), bufs[1], bufs[2], bufs[3], h)
    assert float(h[2]) == INF and float(h[1]) == 1.0


@gpu
@needs_gpu
def test_empty_input_launches_nothing():
    m = _C()
    p, mom, var, state = _zeros(0)
    h = _hstate()
    _ex(m, p, torch.zeros(0, device=DEV), mom, var, state, h,
        table=torch.tensor(TABLE, device=DEV), max_norm=1.0)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [0.0, 0.0, 0.0]
    assert h.cpu().tolist() == [0.0, 1.0] + [0.0] * 6


# ---------------------------------------------------------------------------
# capture, FusedAdam, GraphStepper
# ---------------------------------------------------------------------------

def _all_on(params, dynamic, table):
    from pertgnn.train.optim import FusedAdam

    kw = dict(dynamic_scale=True, init_scale=8.0, growth_interval=3) if dynamic else {}
    return FusedAdam(params, lr=1e-2, weight_decay=0.1, max_grad_norm=0.05,
                     lr_schedule=table, **kw)


@gpu
@needs_gpu
@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_captured_step_replays_like_eager_steps(dynamic):
    require_ext()
    table = [1e-2, 8e-3, 6e-3, 4e-3, 2e-3, 1e-3]
    x = torch.randn(16, 8, generator=_gen(690)).to(DEV)
    opts = []
    for _ in range(3):      # [0]: loads every kernel before the capture
        torch.manual_seed(0)
        net = torch.nn.Linear(8, 4).to(DEV)
        opt = _all_on(net.parameters(), dynamic, table)
        opt.zero_grad()
        opt.scale_loss(net(x).pow(2).mean()).backward()
        opts.append(opt)
    warm, captured, eager = opts
    assert torch.equal(captured.flat_grad, eager.flat_grad)
    warm.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.step()
    assert int(captured.dev_state[0].item()) == 0    # recorded, not run
    for _ in range(4):
        graph.replay()
        eager.step()
    torch.cuda.synchronize()
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "hstate", "dev_state"):
        assert torch.equal(getattr(captured, name), getattr(eager, name)), name
    if dynamic:
        assert torch.equal(captured.sstate, eager.sstate)
        assert float(captured.sstate[0]) == 16.0     # grew once, at step 3
    assert float(captured.hstate[0]) == f32(table[3])
    stats = captured.grad_stats()
    assert stats["steps"] == 4 and stats["clipped_frac"] == 1.0


@gpu
@needs_gpu
def test_fused_adam_gpu_matches_the_eager_path():
    """test_adam_parity's case (10,000 elements, 3 steps, atol 1e-6) with
    every feature on, against the same optimizer stepping eagerly on the
    CPU."""
    require_ext()
    from pertgnn.train.optim import FusedAdam

    gen = _gen(9)
    p0 = torch.randn(100, 100, generator=gen)
    b0 = torch.randn(100, generator=gen)
    grads = [torch.randn(10100, generator=gen) for _ in range(3)]
    got = []
    for dev in (DEV, torch.device("cpu")):
        params = [torch.nn.Parameter(p0.clone().to(dev)),
                  torch.nn.Parameter(b0.clone().to(dev))]
        opt = FusedAdam(params, lr=1e-3, weight_decay=0.1, max_grad_norm=50.0,
                        lr_schedule=[5e-4, 1e-3, 8e-4])
        assert int(opt.decay_mask.sum()) == 10000
        for g in grads:
            opt.flat_grad.copy_(g.to(dev))
            opt.step()
        got.append((opt.flat_param.cpu(), opt.grad_stats(reset=False)))
    (p_gpu, s_gpu), (p_cpu, s_cpu) = got
    assert torch.allclose(p_gpu, p_cpu, atol=1e-6), (p_gpu - p_cpu).abs().max()
    assert s_gpu["steps"] == s_cpu["steps"] == 3
    assert s_gpu["clipped_frac"] == s_cpu["clipped_frac"] == 1.0
    assert s_gpu["lr"] == s_cpu["lr"] == f32(8e-4)
    assert s_gpu["norm_mean"] == pytest.approx(s_cpu["norm_mean"], rel=1e-5)


@gpu
@needs_gpu
def test_graph_stepper_rolls_the_warmup_steps_back():
    require_ext()
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train.capture import GraphStepper
    from pertgnn.train.optim import FusedAdam, decay_params_of, make_lr_table

    torch.manual_seed(0)
    batches, stats = bench_mod.build_synthetic_batches(2, 8, seed=0, device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 64, 2,
                              0.0).to(DEV)
    model.train()
    table = make_lr_table(1e-3, 8, "cosine", warmup_steps=1)
    opt = FusedAdam(model.parameters(), lr=1e-3, weight_decay=0.01,
                    decay_filter=decay_params_of(model), max_grad_norm=1.0,
                    lr_schedule=table)
    stepper = GraphStepper(model, opt, None, None, 0.5, DEV, batches)
    assert stepper.capture() == "full"
    assert opt.hstate.cpu().tolist() == [0.0, 1.0] + [0.0] * 6
    assert float(opt.dev_state[0]) == 0.0
    stepper.run_epoch_sums()
    stats_ = stepper.last_grad_stats
    assert stats_["steps"] == 2
    assert stats_["lr"] == float(table[1])
    assert 0.0 < stats_["norm_mean"] <= stats_["norm_max"] < INF
    stepper.run_epoch_sums()
    assert stepper.last_grad_stats["steps"] == 2
    assert stepper.last_grad_stats["lr"] == float(table[3])
