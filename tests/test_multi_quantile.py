"""Multi-quantile latency heads: the ``[B, Q]`` forms of
``F.quantile_loss`` / ``F.quantile_loss_parts`` / ``F.eval_metrics`` and
``F.quantile_rearrange`` (on the GPU one launch of the scalar HIP loss and
metric kernels per level, the two counts and the compare-exchange network in
elementwise torch ops), their fp32 oracles, the ``[B, Q]`` decoder of
``SAGEDeterministic``, the loops, ``Predictor``, the checkpoint field and the
``--taus`` CLI.

How the reductions are compared:

* exact inputs.  ``y`` is +-2^k with |y| <= 8 (non-zero, so MAPE's division
  is exact), ``y_hat`` an integer in [-8, 8] (ties and crossings are
  frequent) and the levels are multiples of 1/8 — of 1/16 at Q = 8, where
  (0, 1) holds only seven multiples of 1/8.  Every pinball term is then a
  multiple of 1/16 with |term| <= 16, every partial sum of ANY fp32 summation
  order is exact while ``rows * Q * 256 < 2^24``, and the result must be
  ``torch.equal`` to the fp64 oracle on the CPU.  Larger cases narrow the
  values to |.| <= 2 (|term| <= 4): exact while ``rows * Q * 64 < 2^24``.
  ``_exact`` applies the rule and asserts it.
* a level's loss is a sum of per-block quotients ``block_sum / B``: exact
  when B is a power of two, otherwise each of the ``blocks`` quotients and
  each of the ``blocks - 1`` atomic adds rounds once, each by at most
  ``2^-24 * |loss|`` (all terms are >= 0): ``blocks * 2^-24 * |loss|``.  A
  rounding is in fact half of that (2^-25), which leaves room for the one
  more rounding of the sum over the levels (added in fp64, rounded once).
* one random-normal case per kernel against fp64 (with the levels rounded to
  fp32 as the kernel receives them) within the first-order bound of any
  summation order, ``(terms + 4) * 2^-24 * sum|x_i|``: ``terms`` additions
  plus the four roundings inside one term (e, tau - 1, two products).
* the rearrangement moves values and computes none: bit-equal to
  ``torch.sort`` on every input.

Every GPU input lies inside a NaN-filled buffer, so a read past either end
turns a sum into NaN or puts a NaN into a sorted row.

CPU and GPU tests share this file, so the GPU ones carry the ``gpu`` mark and
the no-GPU skip one by one, as tests/test_segops_edges.py does.

Run on an MI355X box:  python -m pytest tests/test_multi_quantile.py -m gpu -q
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pertgnn.ops import functional as F
from pertgnn.ops import reference as ref

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U32 = 2.0 ** -24
Q_LIST = (1, 2, 3, 5, 8)
# 1/3: fewer rows than a wave; 255/256/257: around one block; 1000: four
# blocks, the last ragged; 8193: 33 blocks (one past 2^13)
B_LIST = (0, 1, 3, 255, 256, 257, 1000, 8193)
# one row past the 256-block x 256-thread row grid of the reducing kernels:
# thread 0 of block 0 takes a second row
B_PAST_ROW_GRID = 256 * 256 + 257  # 65,793


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _levels(q):
    """q strictly increasing exact levels, 0.5 among them when q is odd"""
    if q == 8:
        return tuple(k / 16 for k in (1, 3, 5, 7, 9, 11, 13, 15))
    return {1: (0.625,), 2: (0.5, 0.875), 3: (0.125, 0.5, 0.875),
            5: (0.125, 0.25, 0.5, 0.75, 0.875)}[q]


@functools.lru_cache(maxsize=None)
def _exact(b, q, seed=0, summed=True):
    """(y [b], y_hat [b, q]) exact fp32 inputs on the CPU, see the module
    docstring; shared among the tests and never modified.  ``summed=False``
    is for a case that only runs the elementwise kernels, where no sum has
    to stay exact."""
    wide = b * q * 256 < 2 ** 24
    lim, kmax = (8, 4) if wide else (2, 2)
    assert wide or not summed or b * q * 64 < 2 ** 24, (b, q)
    g = _gen(1000 * q + b + seed)
    y = (2.0 ** torch.randint(0, kmax, (b,), generator=g)) * \
        (torch.randint(0, 2, (b,), generator=g) * 2 - 1)
    y_hat = torch.randint(-lim, lim + 1, (b, q), generator=g).float()
    return y.float(), y_hat


def _poison(t, lead=4):
    """t copied into a NaN-filled flat GPU buffer, ``lead`` floats from its
    16-byte aligned start (lead = 4: aligned for 16-byte row accesses, 2:
    for 8-byte ones only, 1: for single floats only)."""
    n = t.numel()
    buf = torch.full((lead + n + 128,), float("nan"), device=DEV,
                     dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[lead:lead + n].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous()
    assert bool(torch.isnan(buf[:lead]).all())
    assert bool(torch.isnan(buf[lead + n:]).all())
    return v


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _grad_rule(y, y_hat, taus, g=1.0):
    """the kernel's gradient in fp64: d * fl32(g / B) with d = -tau for
    e > 0, 1 - tau for e < 0 and the even split of the two at e = 0 (exact
    for levels in sixteenths); round with ``.float()`` for the fp32 product
    the kernel stores"""
    tau = torch.tensor(taus, dtype=torch.float64)
    e = y.double().unsqueeze(1) - y_hat.double()
    d = torch.where(e > 0, -tau, 1 - tau).expand_as(e).clone()
    tie = 0.5 * (-tau) + 0.5 * (1 - tau)
    d = torch.where(e == 0, tie.expand_as(e), d)
    gs = torch.tensor(float(g)) / torch.tensor(float(max(y.shape[0], 1)))
    return d * float(gs)


def _blocks(b):
    return min((b + 255) // 256, 256)


# ---------------------------------------------------------------------------
# A. oracles and plumbing (CPU)
# ---------------------------------------------------------------------------

def test_oracle_loss_against_double_loop():
    y, y_hat = _exact(7, 3)
    taus = (0.1, 0.5, 0.9)
    total = 0.0
    per = [0.0, 0.0, 0.0]
    for i in range(7):
        for q in range(3):
            e = float(y[i]) - float(y_hat[i, q])
            t = max(taus[q] * e, (taus[q] - 1) * e)
            total += t
            per[q] += t
    loss, sums = ref.quantile_loss_multi(y.double(), y_hat.double(), taus)
    assert abs(float(loss) - total / 7) < 1e-12
    assert np.allclose(sums.numpy(), per, atol=1e-12)
    # Q = 1 is the scalar loss
    one, _ = ref.quantile_loss_multi(y, y_hat[:, :1].contiguous(), (0.7,))
    assert torch.equal(one, ref.quantile_loss(y, y_hat[:, 0], 0.7))
    # B = 0: NaN loss, zero sums
    loss0, sums0 = ref.quantile_loss_multi(torch.empty(0), torch.empty(0, 3),
                                           taus)
    assert bool(torch.isnan(loss0)) and torch.equal(sums0, torch.zeros(3))


def test_oracle_tie_gradient_is_the_kernel_rule():
    y, y_hat = _exact(256, 5)  # 1/256 is exact: no rounding to argue about
    assert int((y.unsqueeze(1) == y_hat).sum()) > 20  # ties are present
    taus = _levels(5)
    yh = y_hat.double().requires_grad_(True)
    F.quantile_loss(y.double(), yh, taus).backward()
    assert torch.equal(yh.grad, _grad_rule(y, y_hat, taus))


def test_point_level():
    assert ref.point_level((0.5,)) == 0
    assert ref.point_level((0.1, 0.5, 0.9)) == 1
    assert ref.point_level((0.25, 0.75)) == 0      # tie: the lower index
    assert ref.point_level((0.9, 0.95, 0.99)) == 0
    assert ref.point_level((0.05, 0.3, 0.45, 0.6)) == 2


def test_oracle_metrics_layout():
    y = torch.tensor([1.0, 2.0, -4.0])
    y_hat = torch.tensor([[0.0, 2.0], [3.0, 1.0], [-4.0, -5.0]])
    m = ref.eval_metrics_multi(y, y_hat, (0.5, 0.75))
    # point = column 0: |err| = 1, 1, 0; mape = 1 + 0.5 + 0
    assert m.tolist()[:3] == [2.0, 1.5, 2.0]  # rows 1 and 2 cross
    # pinball: col 0 (0.5): .5 + .5 + 0; col 1 (0.75): .25 + .75 + .75
    assert m.tolist()[3:5] == [1.0, 1.75]
    # covered (y <= y_hat): col 0: rows 1, 2; col 1: rows 0
    assert m.tolist()[5:] == [2.0, 1.0]


@pytest.mark.parametrize("taus", [(0.5, 0.5), (0.9, 0.5), (0.0, 0.5),
                                  (0.5, 1.0), (-0.1,), (float("nan"),), (),
                                  tuple(k / 10 for k in range(1, 10))])
def test_bad_levels_are_refused(taus):
    y, y_hat = torch.ones(4), torch.zeros(4, max(len(taus), 1))
    with pytest.raises(ValueError):
        F.quantile_loss(y, y_hat, taus)
    with pytest.raises(ValueError):
        F.eval_metrics(y, y_hat, taus)


def test_rank_mismatch_is_refused():
    y = torch.ones(4)
    with pytest.raises(ValueError):
        F.quantile_loss(y, torch.zeros(4), (0.5, 0.9))
    with pytest.raises(ValueError):
        F.quantile_loss(y, torch.zeros(4, 2), 0.5)
    with pytest.raises(ValueError):
        F.quantile_loss(y, torch.zeros(4, 3), (0.5, 0.9))
    with pytest.raises(ValueError):
        F.eval_metrics(y, torch.zeros(4, 2), 0.5)
    with pytest.raises(ValueError):
        F.quantile_rearrange(torch.zeros(4))
    with pytest.raises(ValueError):
        F.quantile_rearrange(torch.zeros(4, 9))


def test_quantile_report_arithmetic():
    from pertgnn.train import QuantileReport

    sums = [8.0, 2.0, 1.0, 4.0, 6.0, 10.0, 2.0, 3.0, 4.0]
    r = QuantileReport.from_sums((0.25, 0.5, 0.9), sums, 4)
    assert r.taus == (0.25, 0.5, 0.9) and r.point == 1
    assert (r.mae, r.mape, r.crossing) == (2.0, 0.5, 0.25)
    assert r.qloss == [1.0, 1.5, 2.5] and r.qloss_total == 5.0
    assert r.coverage == [0.5, 0.75, 1.0]
    r0 = QuantileReport.from_sums((0.5, 0.9), [0.0] * 7, 0)
    assert r0.qloss == [0.0, 0.0] and r0.crossing == 0.0
    with pytest.raises(ValueError):
        QuantileReport.from_sums((0.5, 0.9), sums, 4)


def test_taus_parser_and_conflict(capsys):
    sys.path.insert(0, ROOT)
    import pert_gnn as cli

    args = cli.parse_args(["--taus", "0.5,0.9,0.99"])
    assert args.levels == (0.5, 0.9, 0.99) and args.levels_given
    args = cli.parse_args([])
    assert args.levels is None and args.tau == 0.5 and not args.levels_given
    args = cli.parse_args(["--tau", "0.95"])
    assert args.levels is None and args.tau == 0.95 and args.levels_given
    args = cli.parse_args(["--taus", "0.9"])  # one level: the scalar run
    assert args.levels is None and args.tau == 0.9
    for bad in (["--taus", "0.9,0.5"], ["--taus", "0.5,1.5"],
                ["--taus", "a,b"], ["--tau", "0.5", "--taus", "0.5,0.9"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    assert "--taus cannot be combined with --tau" in capsys.readouterr().err


def _tiny_model(num_quantiles=1, hidden=16, seed=0):
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(seed)
    return SAGEDeterministic(9, [5], 3, 4, 2, hidden, 2, 0.0,
                             num_quantiles=num_quantiles)


def test_checkpoint_round_trip_and_refusal(tmp_path):
    from pertgnn.train import load_checkpoint, save_checkpoint

    model = _tiny_model(2)
    path = str(tmp_path / "m.ckpt")
    save_checkpoint(path, model, None, 3, taus=(0.5, 0.9))
    state = torch.load(path, weights_only=False)
    assert state["taus"] == [0.5, 0.9]
    fresh = _tiny_model(2, seed=1)
    ep, _ = load_checkpoint(path, fresh, taus=(0.5, 0.9))
    assert ep == 3 and fresh.taus == (0.5, 0.9)
    assert torch.equal(fresh.global_linear2.weight, model.global_linear2.weight)
    load_checkpoint(path, _tiny_model(2))  # no levels requested: no check
    with pytest.raises(ValueError) as exc:
        load_checkpoint(path, _tiny_model(2), taus=(0.5, 0.95))
    assert "[0.5, 0.9]" in str(exc.value) and "[0.5, 0.95]" in str(exc.value)
    # a scalar run records [tau]
    one = _tiny_model(1)
    save_checkpoint(path, one, None, 1, taus=0.95)
    assert torch.load(path, weights_only=False)["taus"] == [0.95]
    with pytest.raises(ValueError):
        load_checkpoint(path, _tiny_model(1), taus=0.5)
    # a checkpoint without the field loads under any levels
    state = torch.load(path, weights_only=False)
    del state["taus"]
    torch.save(state, path)
    m = _tiny_model(1)
    load_checkpoint(path, m, taus=0.5)
    assert m.taus == (0.5,)


def test_q1_model_keeps_state_dict():
    a, b = _tiny_model(1), _tiny_model(3)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    assert sa["global_linear2.weight"].shape == (1, 16)
    assert sb["global_linear2.weight"].shape == (3, 16)
    assert sb["local_linear.weight"].shape == (1, 16)
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError):
            _tiny_model(bad)


class _StandInComm:
    """two ranks that saw the same data: all_reduce_ doubles"""
    distributed = True
    backend = "gloo"
    device = torch.device("cpu")
    world_size = 2

    def __init__(self):
        self.reduced = []

    def all_reduce_(self, t, op="sum"):
        self.reduced.append(t.clone())
        t.mul_(2)


# ---------------------------------------------------------------------------
# B. model level (CPU and GPU)
# ---------------------------------------------------------------------------

TAUS3 = (0.25, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def _batches(device_type, n=1):
    sys.path.insert(0, ROOT)
    import bench as bench_mod

    dev = DEV if device_type == "cuda" else torch.device("cpu")
    return bench_mod.build_synthetic_batches(n, 8, seed=0, device=dev)


def _model(device_type, hidden, num_quantiles, seed=1):
    from pertgnn.models import SAGEDeterministic

    batches, stats = _batches(device_type)
    torch.manual_seed(seed)
    m = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                          stats["ifc_max"], stats["rpc_max"], hidden, 2, 0.0,
                          num_quantiles=num_quantiles)
    return m.to(DEV if device_type == "cuda" else "cpu")


def _to64(b):
    """the batch on the CPU with its floating tensors in fp64"""
    import dataclasses

    b = b.to("cpu")
    return dataclasses.replace(b, **{
        f.name: getattr(b, f.name).double() for f in dataclasses.fields(b)
        if torch.is_tensor(getattr(b, f.name))
        and getattr(b, f.name).is_floating_point()})


def _fwd(model, b):
    return model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                 b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                 num_graphs=b.num_graphs)


# (device, hidden, precision): H = 64 runs the fp32 attention path, H = 256
# in bf16 the act16 one
CONFIGS = [
    pytest.param("cpu", 64, "fp32", id="cpu-h64-fp32"),
    pytest.param("cuda", 64, "fp32", id="gpu-h64-fp32",
                 marks=[gpu, needs_gpu]),
    pytest.param("cuda", 256, "bf16", id="gpu-h256-bf16",
                 marks=[gpu, needs_gpu]),
]


class _precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        F.set_gemm_precision(self.prec)

    def __exit__(self, *a):
        F.set_gemm_precision("fp32")


@pytest.mark.parametrize("dev,hidden,prec", CONFIGS)
def test_model_three_levels_forward_backward(dev, hidden, prec, monkeypatch):
    """[B, 3] out, finite gradients everywhere, and column q is the
    one-level model that holds row q of the decoder: predictions bit-equal,
    the encoder's gradient the sum of the three one-level gradients.

    Bit-equal holds for the project's GEMM, whose output element does not
    depend on the column count.  On the CPU ``ops.linear`` is torch's BLAS,
    which sums a one-column product (gemv) in another order than a
    three-column one (gemm) — measured here: 1 ulp, 5.96e-8 at 0.29 — so
    there the columns are compared within the first-order bound of any
    summation order of the H-term dot product,
    ``(H + 1) * 2^-24 * (|h| @ |w_q| + |b_q|)``."""
    b = _batches(dev)[0][0]
    decoder_in = []
    real_linear = F.linear

    def recording_linear(x, w, bias=None):
        if w.shape[0] == 3 and bias is not None and w.shape[1] == hidden:
            decoder_in.append(x.detach())
        return real_linear(x, w, bias)

    monkeypatch.setattr(F, "linear", recording_linear)
    with _precision(prec):
        m3 = _model(dev, hidden, 3)
        m3.train()
        gp, lp = _fwd(m3, b)
        assert len(decoder_in) == 1 and decoder_in[0].shape == (b.num_graphs, hidden)
        hid = decoder_in[0].double().abs().cpu()
        assert gp.shape == (b.num_graphs, 3) and lp.shape[1] == 1
        F.quantile_loss(b.y, gp, TAUS3).backward()
        g3 = {}
        for name, p in m3.named_parameters():
            if isinstance(p, torch.nn.parameter.UninitializedParameter):
                continue
            if name.startswith("local_linear"):
                # the per-node head: a loss on global_predict alone does
                # not reach it
                assert p.grad is None
                continue
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            g3[name] = p.grad.detach().double().cpu()
        gsum = {k: torch.zeros_like(v) for k, v in g3.items()}
        gabs = {k: torch.zeros_like(v) for k, v in g3.items()}
        for q in range(3):
            m1 = _model(dev, hidden, 1)
            sd = dict(m3.state_dict())
            sd["global_linear2.weight"] = sd["global_linear2.weight"][q:q + 1]
            sd["global_linear2.bias"] = sd["global_linear2.bias"][q:q + 1]
            m1.load_state_dict(sd)
            m1.train()
            gp1, _ = _fwd(m1, b)
            diff = (gp1[:, 0] - gp[:, q]).abs().max()
            if dev == "cuda":
                assert torch.equal(gp1[:, 0], gp[:, q]), (q, diff)
            else:
                w = m3.global_linear2.weight[q].detach().double().abs()
                bound = (hidden + 1) * U32 * (
                    hid @ w + m3.global_linear2.bias[q].detach().double().abs())
                assert bool(((gp1[:, 0] - gp[:, q]).detach().double().abs()
                             <= bound).all()), (q, diff)
            F.quantile_loss(b.y, gp1.flatten(), TAUS3[q]).backward()
            for name, p in m1.named_parameters():
                if name in gsum and not name.startswith("global_linear2"):
                    gsum[name] += p.grad.detach().double().cpu()
                    gabs[name] += p.grad.detach().double().cpu().abs()
        # the truth: the three-level gradient in fp64 through the reference
        # ops on the CPU, same weights
        m64 = _model("cpu", hidden, 3)
        m64.load_state_dict({k: (v if isinstance(v, torch.nn.parameter.UninitializedParameter)
                                 else v.detach().cpu())
                             for k, v in m3.state_dict().items()})
        m64 = m64.double().train()
        b64 = _to64(b)
        gp64, _ = _fwd(m64, b64)
        F.quantile_loss(b64.y, gp64, TAUS3).backward()
        truth = {n: p.grad for n, p in m64.named_parameters() if n in gsum}
    # Both sides run the same ops with the same roundings (fp32: 2^-24;
    # act16: bf16 stores, 2^-9) and differ from the fp64 gradient by rounding
    # alone, the reference by three passes of it.  So the three-level
    # gradient must agree with the reference as well as the reference agrees
    # with the truth: per tensor within 8 x the reference's own largest
    # error (a factor for the spread between two maxima of the same noise),
    # plus 4 roundings of the summed gradient itself.
    eps = 2.0 ** -9 if prec == "bf16" else U32
    for name in gsum:
        if name.startswith("global_linear2"):
            continue
        scale = float(gabs[name].max())
        ref_err = float((gsum[name] - truth[name]).abs().max())
        err = float((g3[name] - gsum[name]).abs().max())
        print(f"{name}: max|g3 - sum g1| = {err:.3e}, reference error "
              f"{ref_err:.3e}, scale {scale:.3e}")
        assert err <= 8 * ref_err + 4 * eps * scale, (name, err, ref_err, scale)


@pytest.mark.parametrize("dev,hidden,prec", CONFIGS)
def test_stepper_two_epochs_three_levels(dev, hidden, prec):
    from pertgnn.train.capture import GraphStepper
    from pertgnn.train.optim import FusedAdam

    batches = _batches(dev)[0]
    device = DEV if dev == "cuda" else torch.device("cpu")
    with _precision(prec):
        model = _model(dev, hidden, 3)
        model.train()
        opt = FusedAdam(model.parameters(), lr=1e-2)
        stepper = GraphStepper(model, opt, None, None, TAUS3, device, batches)
        mode = stepper.capture()
        assert mode == ("full" if dev == "cuda" else "eager")
        losses = []
        for _ in range(2):
            loss, mape = stepper.run_epoch()
            assert np.isfinite(loss) and np.isfinite(mape)
            assert len(stepper.last_q_loss) == 3
            # the epoch's loss is the sum of its per-level averages
            assert abs(sum(stepper.last_q_loss) - loss) <= 1e-5 * abs(loss)
            losses.append(loss)
        if dev == "cuda":
            torch.cuda.synchronize()
    assert losses[1] < losses[0], losses


@pytest.mark.parametrize("dev,hidden,prec", CONFIGS)
def test_train_epoch_and_evaluate_three_levels(dev, hidden, prec):
    from pertgnn.train import QuantileReport, evaluate, train_epoch
    from pertgnn.train.optim import FusedAdam

    batches = _batches(dev)[0]
    device = DEV if dev == "cuda" else torch.device("cpu")
    with _precision(prec):
        model = _model(dev, hidden, 3)
        opt = FusedAdam(model.parameters(), lr=1e-2)
        stats = {}
        loss, mape = train_epoch(model, batches, opt, TAUS3, device,
                                 stats_out=stats)
        assert np.isfinite(loss) and len(stats["q_loss"]) == 3
        assert abs(sum(stats["q_loss"]) - loss) <= 1e-5 * abs(loss)
        rep = evaluate(model, batches, TAUS3, device)
        assert isinstance(rep, QuantileReport) and rep.point == 1
        model.eval()
        with torch.no_grad():
            gp, _ = _fwd(model, batches[0])
        want = ref.eval_metrics_multi(batches[0].y.double().cpu(),
                                      gp.double().cpu(), TAUS3)
        n = batches[0].num_graphs
        got = [rep.mae, rep.mape, rep.crossing] + rep.qloss + rep.coverage
        assert np.allclose(got, (want / n).numpy(), rtol=1e-5, atol=1e-6)
        # a distributed comm all-reduces the whole vector and n, once
        comm = _StandInComm()
        rep2 = evaluate(model, batches, TAUS3, device, comm=comm)
        assert len(comm.reduced) == 1 and comm.reduced[0].numel() == 3 + 6 + 1
        assert float(comm.reduced[0][-1]) == n
        assert rep2.mae == rep.mae and rep2.coverage == rep.coverage
        # the scalar path still returns its triple
        m1 = _model(dev, hidden, 1)
        out = evaluate(m1, batches, 0.5, device)
        assert isinstance(out, tuple) and len(out) == 3


def _randomize_bn(model, seed):
    g = _gen(seed)
    with torch.no_grad():
        for bn in model.bns:
            h = bn.num_features
            bn.running_mean.copy_(torch.randn(h, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(h, generator=g) + 0.5)
            bn.weight.copy_(torch.rand(h, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(h, generator=g) * 0.1)


@pytest.mark.parametrize("dev,hidden,prec", CONFIGS)
def test_predictor_three_levels(dev, hidden, prec):
    from pertgnn.infer import Predictor
    from pertgnn.train import evaluate

    batches = _batches(dev)[0]
    b = batches[0]
    device = DEV if dev == "cuda" else torch.device("cpu")
    with _precision(prec):
        model = _model(dev, hidden, 3)
        _randomize_bn(model, 3)
        # a decoder whose rows disagree, so that raw rows do cross
        with torch.no_grad():
            model.global_linear2.weight[1].neg_()
        model.eval()
        model.taus = TAUS3
        with torch.no_grad():
            gp, _ = _fwd(model, b)
        p = Predictor(model)
        assert p.taus == TAUS3 and p.num_quantiles == 3
        raw = p.predict_batch(b, rearrange=False)
        assert raw.shape == (b.num_graphs, 3) and raw.dtype == torch.float32
        # the tolerances of tests/test_infer.py for the precision
        if dev == "cpu":
            assert torch.allclose(raw, gp, atol=1e-5), (raw - gp).abs().max()
        elif prec == "fp32":
            assert torch.allclose(raw, gp.float(), atol=2e-3, rtol=1e-3), \
                (raw - gp).abs().max()
        else:
            rel = (raw - gp.float()).abs().max() / gp.abs().max().clamp_min(1e-6)
            print(f"{prec}: relative max error {float(rel):.4f}")
            assert rel < 0.05, rel
        assert bool((raw[:, 1:] < raw[:, :-1]).any()), "no crossing row"
        srt = p.predict_batch(b)
        assert torch.equal(srt, torch.sort(raw, dim=1).values)
        assert p.predict([b]).shape == (b.num_graphs, 3)
        mode = p.capture(batches)
        assert mode == ("graph" if dev == "cuda" else "eager")
        assert torch.equal(p.replay(0), srt)
        assert torch.equal(p.replay(0, rearrange=False), raw)
        # evaluate with the predictor feeds the raw rows to the metrics
        rep_p = evaluate(model, batches, TAUS3, device, predictor=p)
        want = ref.eval_metrics_multi(b.y.double().cpu(), raw.double().cpu(),
                                      TAUS3)
        assert rep_p.crossing == float(want[2]) / b.num_graphs > 0
        # refresh() after a weight change is picked up by a replay
        with torch.no_grad():
            model.global_linear2.bias.add_(1.0)
            for bn in model.bns:
                bn.weight.mul_(1.5)
        p.refresh()
        fresh = p.replay(0, rearrange=False).clone()
        assert not torch.equal(fresh, raw)
        assert torch.equal(fresh, p.predict_batch(b, rearrange=False))
        assert torch.equal(p.replay(0), torch.sort(fresh, dim=1).values)


# the epoch line of this scalar run as printed by the commit before the
# multi-level heads (recorded from a run of that commit on the CPU, one
# thread, PYTHONHASHSEED=0: the synthetic ingest iterates over sets, so the
# dataset order follows the hash seed): the default path must not move by a
# bit
PARENT_EPOCH_LINE_CPU = (
    "Epoch: 1, Train: 151.3060952645761, Test mae: 307.0374247233073, "
    "Train mape: 0.9989195223207827, Test mape: 0.9985815220408969, "
    "Test q95 loss: 153.51871236165366")
CLI_COMMON = ["--num_layers", "2", "--hidden_channels", "32", "--seed", "0",
              "--batch_size", "64", "--max_traces", "400"]


def _cli(args, cpu):
    env = dict(os.environ, OMP_NUM_THREADS="1", PYTHONHASHSEED="0")
    if cpu:
        env["HIP_VISIBLE_DEVICES"] = ""
        env["CUDA_VISIBLE_DEVICES"] = ""
    return subprocess.run([sys.executable, os.path.join(ROOT, "pert_gnn.py")]
                          + args, env=env, cwd=ROOT, capture_output=True,
                          text=True, timeout=600)


def _cli_round_trip(tmp_path, cpu):
    pdir = str(tmp_path / "processed")
    ckpt = str(tmp_path / "q.ckpt")
    out = str(tmp_path / "pred.npy")
    jsonl = str(tmp_path / "m.jsonl")
    base = ["--processed_dir", pdir] + CLI_COMMON
    r = _cli(base + ["--synthetic", "--epochs", "1", "--taus", "0.5,0.9",
                     "--checkpoint", ckpt, "--metrics_jsonl", jsonl], cpu)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert any(ln.startswith("Epoch: 1, Train: ") for ln in lines)
    assert any(ln.startswith("  tau=0.5: test q loss=") and "coverage=" in ln
               for ln in lines)
    assert any(ln.startswith("  tau=0.9: test q loss=") for ln in lines)
    assert any(ln.startswith("  crossing=") for ln in lines)
    rec = json.loads(open(jsonl).read().splitlines()[-1])
    assert rec["taus"] == [0.5, 0.9]
    for key in ("valid_q_levels", "test_q_levels", "valid_coverage",
                "test_coverage"):
        assert len(rec[key]) == 2, key
    assert "valid_crossing" in rec and "test_crossing" in rec
    assert torch.load(ckpt, weights_only=False)["taus"] == [0.5, 0.9]
    # --predict takes the levels from the checkpoint
    r = _cli(base + ["--checkpoint", ckpt, "--predict", out], cpu)
    assert r.returncode == 0, r.stderr[-2000:]
    pred = np.load(out)
    assert pred.dtype == np.float32 and pred.ndim == 2 and pred.shape[1] == 2
    assert pred.shape[0] > 0 and bool((np.diff(pred, axis=1) >= 0).all())
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Predict: ")]
    assert line and "tau=0.5: q loss=" in line[0] and "tau=0.9: q loss=" in line[0]
    # other levels are refused, naming both sets
    r = _cli(base + ["--checkpoint", ckpt, "--predict", out, "--taus",
                     "0.5,0.95"], cpu)
    assert r.returncode != 0
    assert "[0.5, 0.9]" in r.stderr and "[0.5, 0.95]" in r.stderr
    return base


def test_cli_two_levels_cpu(tmp_path):
    base = _cli_round_trip(tmp_path, cpu=True)
    # the scalar run on the same data and seed prints the parent's line
    r = _cli(base + ["--epochs", "1"], cpu=True)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch: 1,")]
    assert len(line) == 1, r.stdout[-1500:]
    # Same text, and the same numbers: the figures are fp32 CPU sums, whose
    # last bits follow the host's vector width (the previous commit itself
    # prints 307.0374247 on one host and 307.0373671 on another, 2e-7
    # apart), so they are held to 1e-5 relative — 100 fp32 roundings —
    # not to the digit.
    import re

    num = r"-?\d+(?:\.\d+)?(?:e[-+]?\d+)?"
    shape = re.sub(num, "#", PARENT_EPOCH_LINE_CPU)
    assert re.sub(num, "#", line[0]) == shape, line[0]
    want = [float(v) for v in re.findall(num, PARENT_EPOCH_LINE_CPU)]
    got = [float(v) for v in re.findall(num, line[0])]
    assert np.allclose(got, want, rtol=1e-5, atol=0), (line[0],
                                                        PARENT_EPOCH_LINE_CPU)


@gpu
@needs_gpu
def test_cli_two_levels_gpu(tmp_path):
    _cli_round_trip(tmp_path, cpu=False)


# ---------------------------------------------------------------------------
# C. kernels (GPU)
# ---------------------------------------------------------------------------

def _check_kernels(b, q, lead=4):
    """every op on the exact inputs of (b, q) against the fp64 oracle"""
    taus = _levels(q)
    y, y_hat = _exact(b, q)
    yd, yhd = _poison(y, lead), _poison(y_hat, lead).requires_grad_(True)
    y64, yh64 = y.double(), y_hat.double()

    loss, sums = F.quantile_loss_parts(yd, yhd, taus)
    want_loss, want_sums = ref.quantile_loss_multi(y64, yh64, taus)
    assert sums.shape == (q,) and not sums.requires_grad
    assert torch.equal(sums.cpu().double(), want_sums), (b, q, "level sums")
    got_loss = float(loss.detach())
    if b == 0:
        assert bool(torch.isnan(loss))
    elif b & (b - 1) == 0:
        assert got_loss == float(want_loss), (b, q, got_loss)
    else:
        tol = _blocks(b) * U32 * abs(float(want_loss))
        assert abs(got_loss - float(want_loss)) <= tol, (b, q, got_loss)

    loss.backward()
    assert yhd.grad.shape == (b, q)
    assert torch.equal(_bits(yhd.grad), _bits(_grad_rule(y, y_hat, taus).float())), \
        (b, q, "grad")

    m = F.eval_metrics(yd, yhd.detach(), taus)
    want_m = ref.eval_metrics_multi(y64, yh64, taus)
    assert m.shape == (3 + 2 * q,)
    assert torch.equal(m.cpu().double(), want_m), (b, q, m.cpu(), want_m)

    srt = F.quantile_rearrange(yhd.detach())
    assert srt.shape == (b, q)
    assert torch.equal(_bits(srt), _bits(torch.sort(y_hat, dim=1).values))
    if q == 1:
        assert srt.data_ptr() == yhd.data_ptr()  # identity, nothing launched
    # rearranged rows never score worse than the raw rows, row by row
    tau = torch.tensor(taus, dtype=torch.float64)

    def row_loss(p):
        e = y64.unsqueeze(1) - p
        return torch.maximum(tau * e, (tau - 1) * e).sum(dim=1)

    raw, better = row_loss(yh64), row_loss(srt.cpu().double())
    assert bool((better <= raw).all())
    # a row that crosses is strictly better, by at least 1/8: exchanging a
    # crossing pair a > b at levels t1 < t2 lowers the row's loss by
    # exactly (t2 - t1) * (a - b) wherever y lies, sorting is a sequence of
    # such exchanges, the levels here are 1/8 apart or more and a - b >= 1
    crossing = (y_hat[:, 1:] < y_hat[:, :-1]).any(dim=1)
    assert bool((raw[crossing] - better[crossing] >= 0.125).all()), (b, q)


@gpu
@needs_gpu
@pytest.mark.parametrize("b", B_LIST)
@pytest.mark.parametrize("q", Q_LIST)
def test_kernels_exact(q, b):
    _check_kernels(b, q)


@gpu
@needs_gpu
@pytest.mark.parametrize("lead", [1, 2])
@pytest.mark.parametrize("q", [2, 3, 8])
def test_kernels_exact_misaligned_rows(q, lead):
    """predictions that start 4 bytes (lead 1) or 8 bytes (lead 2) past a
    16-byte line: nothing may assume wider alignment of the rows"""
    _check_kernels(257, q, lead=lead)


@gpu
@needs_gpu
def test_backward_past_its_grid():
    """one row past the 4096-block x 256-thread grid of the loss backward:
    thread 0 of block 0 takes a second element"""
    b, q = 4096 * 256 + 1, 2
    taus = _levels(q)
    y, y_hat = _exact(b, q, summed=False)
    yd, yhd = _poison(y), _poison(y_hat).requires_grad_(True)
    (F.quantile_loss(yd, yhd, taus) * 4).backward()
    assert torch.equal(_bits(yhd.grad),
                       _bits(_grad_rule(y, y_hat, taus, 4.0).float()))


@gpu
@needs_gpu
def test_reducing_kernels_past_the_row_grid():
    _check_kernels(B_PAST_ROW_GRID, 3)


@gpu
@needs_gpu
@pytest.mark.parametrize("b", [1, 3, 255, 256])
def test_one_level_equals_scalar_ops_random(b):
    """one block: the scalar kernels are reproducible, so equal bits"""
    g = _gen(b)
    y = (torch.randn(b, generator=g).abs() + 0.5)
    y_hat = torch.randn(b, generator=g)
    _one_level_vs_scalar(y, y_hat, 0.7)


@gpu
@needs_gpu
@pytest.mark.parametrize("b", [256, 1024, 8192])
def test_one_level_equals_scalar_ops_exact(b):
    y, y_hat = _exact(b, 1)
    _one_level_vs_scalar(y, y_hat[:, 0].contiguous(), 0.625)


def _one_level_vs_scalar(y, y_hat, tau):
    yd = _poison(y)
    s_in = _poison(y_hat).requires_grad_(True)
    m_in = _poison(y_hat.unsqueeze(1)).requires_grad_(True)
    ls = F.quantile_loss(yd, s_in, tau)
    lm, sums = F.quantile_loss_parts(yd, m_in, (tau,))
    assert torch.equal(_bits(ls), _bits(lm))
    (ls * 3).backward()
    (lm * 3).backward()
    assert torch.equal(_bits(s_in.grad), _bits(m_in.grad[:, 0]))
    mae, mape, qs = F.eval_metrics(yd, s_in.detach(), tau)
    mm = F.eval_metrics(yd, m_in.detach(), (tau,))
    assert mm.shape == (5,)
    assert torch.equal(_bits(torch.stack([mae, mape, qs])),
                       _bits(mm[[0, 1, 3]]))
    assert float(mm[2]) == 0.0  # one column never crosses


@gpu
@needs_gpu
def test_kernels_random_normal():
    b, q = 3001, 5
    taus = (0.05, 0.3, 0.5, 0.9, 0.99)
    t32 = tuple(float(np.float32(t)) for t in taus)
    g = _gen(11)
    y = torch.randn(b, generator=g).abs() + 0.5
    y_hat = torch.randn(b, q, generator=g)
    yd, yhd = _poison(y), _poison(y_hat).requires_grad_(True)
    y64, yh64 = y.double(), y_hat.double()
    tau = torch.tensor(t32, dtype=torch.float64)
    e = y64.unsqueeze(1) - yh64
    terms = torch.maximum(tau * e, (tau - 1) * e)

    loss, sums = F.quantile_loss_parts(yd, yhd, taus)
    bound = (b + 4 + _blocks(b) + 1) * U32 * terms.sum(dim=0)
    assert bool(((sums.cpu().double() - terms.sum(dim=0)).abs() <= bound).all())
    want_loss = terms.sum() / b
    assert abs(float(loss.detach()) - float(want_loss)) <= \
        (b * q + 4 + _blocks(b)) * U32 * float(want_loss)

    loss.backward()
    want_grad = _grad_rule(y, y_hat, t32)
    # 1 - tau and the product gs * d round once each in fp32
    assert bool(((yhd.grad.cpu().double() - want_grad).abs()
                 <= 2 * U32 * want_grad.abs()).all())

    m = F.eval_metrics(yd, yhd.detach(), taus).cpu().double()
    want = ref.eval_metrics_multi(y64, yh64, t32)
    point = ref.point_level(taus)
    abs_err = (yh64[:, point] - y64).abs()
    mag = torch.cat([torch.stack([abs_err.sum(), (abs_err / y64).sum(),
                                  torch.tensor(0.0, dtype=torch.float64)]),
                     terms.sum(dim=0), torch.zeros(q, dtype=torch.float64)])
    assert bool(((m - want).abs() <= (b + 4) * U32 * mag).all()), (m, want)

    srt = F.quantile_rearrange(yhd.detach())
    assert torch.equal(_bits(srt), _bits(torch.sort(y_hat, dim=1).values))


@gpu
@needs_gpu
def test_non_contiguous_predictions_are_handled():
    """the ops accept a transposed view and compute what its contiguous
    copy gives"""
    y, y_hat = _exact(257, 3)
    taus = _levels(3)
    yd = y.to(DEV)
    nc = y_hat.t().contiguous().to(DEV).t()
    assert not nc.is_contiguous()
    c = nc.contiguous()
    assert torch.equal(F.quantile_loss(yd, nc, taus), F.quantile_loss(yd, c, taus))
    assert torch.equal(F.eval_metrics(yd, nc, taus), F.eval_metrics(yd, c, taus))
    assert torch.equal(F.quantile_rearrange(nc), F.quantile_rearrange(c))
    nc.requires_grad_(True)
    F.quantile_loss(yd, nc, taus).backward()
    assert torch.equal(_bits(nc.grad), _bits(_grad_rule(y, y_hat, taus).float()))


# the decoder GEMMs at n = Q outputs through ops.linear: forward, dgrad and
# wgrad on exact operands (integers in [-8, 8], bias in eighths; every
# product and partial sum is an exact fp32 number, and exact in bf16
# operands too), bit-equal to fp64
@gpu
@needs_gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("m,k", [(8, 64), (8, 256), (1000, 256), (1024, 64)])
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_head_gemm_exact(n, m, k, prec):
    g = _gen(100 * n + m + k)
    x = torch.randint(-8, 9, (m, k), generator=g).float()
    w = torch.randint(-8, 9, (n, k), generator=g).float()
    bias = torch.randint(-8, 9, (n,), generator=g).float() / 8
    go = torch.randint(-8, 9, (m, n), generator=g).float()
    xd = _poison(x).requires_grad_(True)
    wd = _poison(w).requires_grad_(True)
    bd = _poison(bias).requires_grad_(True)
    with _precision(prec):
        out = F.linear(xd, wd, bd)
        out.backward(_poison(go))
    assert torch.equal(out.detach().cpu().double(),
                       x.double() @ w.double().t() + bias.double())
    assert torch.equal(xd.grad.cpu().double(), go.double() @ w.double())
    assert torch.equal(wd.grad.cpu().double(), go.double().t() @ x.double())
    assert torch.equal(bd.grad.cpu().double(), go.double().sum(dim=0))
