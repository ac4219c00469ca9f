"""Grouped P-table GEMMs: every layer's ``table @ we^T`` (and its backward)
for both embedding tables in one launch each.

Forward: bit-equal to the per-layer ``linear16(table, we)``.  Backward: both
the grouped result and the per-layer path (``linear_dgrad16`` /
``linear_wgrad16``, the table gradients summed as autograd sums them) are
measured against fp64 products of the bf16 ``dP`` and of the operands rounded
to bf16, as the LDS staging rounds them; only the fp32 summation order
differs, so the grouped maximum error may be at most twice the per-layer
one, plus one fp32 ulp of the largest output.  (The gradient of a table of
at most 16 rows keeps the fp32 weights on both paths, so against that
reference both are off by the weights' rounding, 5e-3 to 2e-2 here;
``test_tiny_table_dgrad_keeps_fp32_weights`` measures it against the
unrounded products.)

Measured on MI355X (grouped / per-layer max error): H=256 L=3 V=2048 R=5
d_ifc_table 1.37e-06 / 1.30e-06, dW_ifc 3.06e-05 / 3.78e-05, dW_rpc 4.77e-07
/ 4.77e-07; the full table is in profiles/16_ptable_grouped.md.

Run as a script (``python tests/test_ptable_grouped.py det``) this file is
the child process of ``test_deterministic_child``.
"""
import functools
import math
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

import pytest
import torch

from pertgnn.ops import functional as F

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None
needs_gpu = pytest.mark.skipif(not HAS_GPU, reason="no GPU available")

# V = 130: row tail of 64- and 128-row tiles; R = 1 / 5: the tiny-M groups
TABLES = [(130, 5), (64, 1), (2048, 5)]
CASES = [(h, layers, v, r) for h in (64, 256) for layers in (1, 3)
         for (v, r) in TABLES]


def _ext():
    import pertgnn._C as C
    return C


@functools.lru_cache(maxsize=None)
def _operands(h, layers, v, r):
    """(ifc_table, rpc_table, [we_ifc], [we_rpc], [dP] in the op's output
    order) on the GPU; built once per shape and never written to."""
    g = torch.Generator().manual_seed(1000 * h + 10 * layers + v + r)
    ifc = torch.randn(v, h, generator=g)
    rpc = torch.randn(r, h, generator=g)
    we_ifc = [torch.randn(h, h, generator=g) / math.sqrt(h) for _ in range(layers)]
    we_rpc = [torch.randn(h, h, generator=g) / math.sqrt(h) for _ in range(layers)]
    dps = [torch.randn(rows, h, generator=g).to(torch.bfloat16)
           for rows in [v] * layers + [r] * layers]
    dev = lambda t: t.to(DEV)
    return (dev(ifc), dev(rpc), [dev(w) for w in we_ifc],
            [dev(w) for w in we_rpc], [dev(d) for d in dps])


def _bf16_64(t):
    return t.to(torch.bfloat16).double()


def _ulp32(x):
    """One fp32 unit in the last place at magnitude x."""
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


def _fp64_reference(ifc, rpc, we_ifc, we_rpc, dps):
    """-> (d_ifc, d_rpc, [dW_g]); a missing dP contributes nothing."""
    layers = len(we_ifc)
    out = []
    for t, (table, ws) in enumerate(((ifc, we_ifc), (rpc, we_rpc))):
        dt = torch.zeros(table.shape, dtype=torch.float64, device=table.device)
        for l in range(layers):
            d = dps[t * layers + l]
            if d is not None:
                dt += d.double() @ _bf16_64(ws[l])
        out.append(dt)
    dws = []
    for g, d in enumerate(dps):
        table = ifc if g < layers else rpc
        dws.append(None if d is None else d.double().t() @ _bf16_64(table))
    return out[0], out[1], dws


def _per_layer_backward(ifc, rpc, we_ifc, we_rpc, dps):
    """The path the grouped op replaces: one dgrad and one wgrad per (table,
    layer); autograd adds the table gradients in backward order, last layer
    first."""
    C = _ext()
    layers = len(we_ifc)
    dts, dws = [], []
    for t, (table, ws) in enumerate(((ifc, we_ifc), (rpc, we_rpc))):
        dt = None
        for l in reversed(range(layers)):
            d = dps[t * layers + l]
            if d is None:
                continue
            g = C.linear_dgrad16(d, ws[l])
            dt = g if dt is None else dt + g
        dts.append(torch.zeros_like(table) if dt is None else dt)
    for g, d in enumerate(dps):
        table = ifc if g < layers else rpc
        dws.append(None if d is None else C.linear_wgrad16(d, table, False)[0])
    return dts[0], dts[1], dws


def _grouped_backward(ifc, rpc, we_ifc, we_rpc, dps, splits=1):
    none = torch.empty(0, dtype=torch.bfloat16, device=ifc.device)
    d_ifc, d_rpc, dw = _ext().ptables_bwd(
        [none if d is None else d for d in dps], ifc, rpc, we_ifc, we_rpc,
        splits)
    return d_ifc, d_rpc, [None if d is None else dw[g]
                          for g, d in enumerate(dps)]


def _max_err(got, want):
    """Largest |got - want| over a list of tensors (None entries skipped)."""
    return max([float((a.double() - w).abs().max())
                for a, w in zip(got, want) if w is not None and w.numel()],
               default=0.0)


def _check_backward(tag, ops, dps, splits=1):
    """The bound of this file: grouped error <= 2 x per-layer error + 1 ulp
    of the largest output, for the two table gradients and for the weight
    gradients of either table."""
    ifc, rpc, we_ifc, we_rpc = ops
    layers = len(we_ifc)
    ref = _fp64_reference(ifc, rpc, we_ifc, we_rpc, dps)
    old = _per_layer_backward(ifc, rpc, we_ifc, we_rpc, dps)
    new = _grouped_backward(ifc, rpc, we_ifc, we_rpc, dps, splits)
    torch.cuda.synchronize()
    parts = {
        "d_ifc_table": ([new[0]], [old[0]], [ref[0]]),
        "d_rpc_table": ([new[1]], [old[1]], [ref[1]]),
        "dW_ifc": (new[2][:layers], old[2][:layers], ref[2][:layers]),
        "dW_rpc": (new[2][layers:], old[2][layers:], ref[2][layers:]),
    }
    for name, (n, o, r) in parts.items():
        e_new, e_old = _max_err(n, r), _max_err(o, r)
        big = max([float(w.abs().max()) for w in r if w is not None and w.numel()],
                  default=0.0)
        bound = 2.0 * e_old + _ulp32(big)
        print(f"{tag} {name}: grouped {e_new:.3e} per-layer {e_old:.3e} "
              f"bound {bound:.3e} (max |out| {big:.3f})")
        assert e_new <= bound, (tag, name, e_new, e_old, bound)
    return new


# ---------------------------------------------------------------------------
# CPU: the plumbing's gates
# ---------------------------------------------------------------------------

def test_group_switch_is_read_per_call(monkeypatch):
    monkeypatch.delenv("PERTGNN_NO_PTABLE_GROUP", raising=False)
    assert F.ptable_group_enabled()
    monkeypatch.setenv("PERTGNN_NO_PTABLE_GROUP", "1")
    assert not F.ptable_group_enabled()


def test_cpu_model_never_groups(monkeypatch, synthetic_workspace):
    """A CPU forward takes the reference path; the grouped op is not called
    and forward_fused keeps its old signature as a prefix."""
    import inspect

    from pertgnn.data.collate import collate
    from pertgnn.data.dataset import build_data_list
    from pertgnn.models import SAGEDeterministic
    from pertgnn.models.pert_gnn import TransformerConv

    params = list(inspect.signature(TransformerConv.forward_fused).parameters)
    assert params[:7] == ["self", "x", "edge_attr", "ifc_weight", "rpc_weight",
                          "csr", "out16"]
    assert params[7:] == ["pifc", "prpc"]

    def boom(*a, **k):
        raise AssertionError("grouped P tables on the CPU path")

    monkeypatch.setattr(F, "ptables_grouped", boom)
    _, (tr2data, entry2runtimes, _, runtime2pert, resource_df) = synthetic_workspace
    data_list = build_data_list(tr2data, entry2runtimes, runtime2pert,
                                resource_df, limit=8)
    b = collate(data_list[:4])
    torch.manual_seed(0)
    model = SAGEDeterministic(
        9, [max(int(s.cat_X.max()) for s in data_list) + 1],
        max(int(s.entry_id) for s in data_list),
        max(int(s.edge_attr[:, 0].max()) for s in data_list),
        max(int(s.edge_attr[:, 1].max()) for s in data_list), 32, 3, 0.0)
    gp, lp = model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                   b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                   num_graphs=b.num_graphs)
    assert torch.isfinite(gp).all() and torch.isfinite(lp).all()


# ---------------------------------------------------------------------------
# GPU: the op
# ---------------------------------------------------------------------------

@gpu
@needs_gpu
@pytest.mark.parametrize("h,layers,v,r", CASES)
def test_forward_bit_equal(h, layers, v, r):
    ifc, rpc, we_ifc, we_rpc, _ = _operands(h, layers, v, r)
    pifc, prpc = F.ptables_grouped(ifc, rpc, we_ifc, we_rpc)
    assert len(pifc) == layers and len(prpc) == layers
    for l in range(layers):
        for got, table, w in ((pifc[l], ifc, we_ifc[l]),
                              (prpc[l], rpc, we_rpc[l])):
            want = F.linear16(table, w)
            assert got.dtype == torch.bfloat16 and got.shape == want.shape
            assert torch.equal(got, want), (l, tuple(table.shape))


@gpu
@needs_gpu
@pytest.mark.parametrize("h,layers,v,r", CASES)
def test_backward_against_fp64(h, layers, v, r):
    *ops, dps = _operands(h, layers, v, r)
    _check_backward(f"H={h} L={layers} V={v} R={r}", ops, dps)


@gpu
@needs_gpu
def test_backward_missing_dp():
    """One interface dP and one rpc dP missing: they add nothing to the
    table gradients and their weight gradients read as zero."""
    *ops, dps = _operands(64, 3, 130, 5)
    dps = list(dps)
    dps[1] = None
    dps[3] = None
    new = _check_backward("missing dP", ops, dps)
    none = torch.empty(0, dtype=torch.bfloat16, device=DEV)
    dw = _ext().ptables_bwd([none if d is None else d for d in dps], *ops, 1)[2]
    assert not dw[1].any() and not dw[3].any()
    assert new[2][1] is None and new[2][3] is None


@gpu
@needs_gpu
@pytest.mark.parametrize("h,layers,v,r", [(256, 3, 130, 5), (64, 1, 64, 1)])
def test_tiny_table_dgrad_keeps_fp32_weights(h, layers, v, r):
    """The per-layer dgrad of a table of at most 16 rows is the skinny fp32
    kernel, which reads the weights unrounded; the grouped kernel carries
    them as a bf16 pair (hi + lo).  Against fp64 products with the UNROUNDED
    weights its error is at most twice the skinny path's plus what the lo
    half's own rounding can add: bf16 rounds to nearest with 8 significant
    bits, so |W - hi| <= 2^-8 |W| and |(W - hi) - lo| <= 2^-16 |W|, that is
    2^-16 |dP| |W| per term, summed (a bf16-rounded W alone is 2^-8)."""
    ifc, rpc, we_ifc, we_rpc, dps = _operands(h, layers, v, r)
    rdps = dps[layers:]
    want = sum(d.double() @ w.double() for d, w in zip(rdps, we_rpc))
    lo_bound = float(sum(d.double().abs() @ w.double().abs()
                         for d, w in zip(rdps, we_rpc)).max()) * 2.0 ** -16
    old = _per_layer_backward(ifc, rpc, we_ifc, we_rpc, dps)[1]
    new = _grouped_backward(ifc, rpc, we_ifc, we_rpc, dps)[1]
    e_new = float((new.double() - want).abs().max())
    e_old = float((old.double() - want).abs().max())
    rounded = float((_fp64_reference(ifc, rpc, we_ifc, we_rpc, dps)[1]
                     - want).abs().max())
    print(f"H={h} L={layers} R={r}: grouped {e_new:.3e} skinny {e_old:.3e} "
          f"lo bound {lo_bound:.3e}; bf16-rounded W would be off by {rounded:.3e}")
    assert e_new <= 2.0 * e_old + lo_bound, (e_new, e_old, lo_bound)


@gpu
@needs_gpu
def test_backward_layer_split():
    """The dgrad's atomic split over layers meets the same bound."""
    *ops, dps = _operands(256, 3, 130, 5)
    _check_backward("splits=3", ops, dps, splits=3)


@gpu
@needs_gpu
def test_autograd_function_matches_op(monkeypatch):
    """F.ptables_grouped's backward hands each input its gradient: tables
    summed over layers, weights per layer, None where no dP arrived
    (deterministic mode, so the op called directly gives the same bits)."""
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    ifc, rpc, we_ifc, we_rpc, dps = _operands(64, 3, 130, 5)
    leaves = [t.clone().requires_grad_(True)
              for t in [ifc, rpc, *we_ifc, *we_rpc]]
    pifc, prpc = F.ptables_grouped(leaves[0], leaves[1], leaves[2:5], leaves[5:8])
    outs = pifc + prpc
    keep = [0, 2, 3, 5]   # layer 1 of either table gets no gradient
    torch.autograd.backward([outs[i] for i in keep], [dps[i] for i in keep])
    want = _grouped_backward(ifc, rpc, we_ifc, we_rpc,
                             [d if i in keep else None
                              for i, d in enumerate(dps)])
    assert torch.equal(leaves[0].grad, want[0])
    assert torch.equal(leaves[1].grad, want[1])
    for g in range(6):
        if g in keep:
            assert torch.equal(leaves[2 + g].grad, want[2][g]), g
        else:
            assert leaves[2 + g].grad is None, g


@gpu
@needs_gpu
def test_group_cap_split():
    """One (table, layer) pair more than a descriptor holds (2L is even, so
    the smallest excess over the cap is two groups): the launchers split, and
    the results are those of the un-capped references."""
    cap = _ext().ptables_max_groups()
    layers = cap // 2 + 1
    ifc, rpc, we_ifc, we_rpc, dps = _operands(64, layers, 64, 1)
    assert 2 * layers > cap
    pifc, prpc = F.ptables_grouped(ifc, rpc, we_ifc, we_rpc)
    for l in range(layers):
        assert torch.equal(pifc[l], F.linear16(ifc, we_ifc[l])), l
        assert torch.equal(prpc[l], F.linear16(rpc, we_rpc[l])), l
    _check_backward(f"cap L={layers}", (ifc, rpc, we_ifc, we_rpc), dps)
    _check_backward(f"cap L={layers} split", (ifc, rpc, we_ifc, we_rpc), dps,
                    splits=4)


@gpu
@needs_gpu
def test_shape_errors_raise():
    C = _ext()
    ifc, rpc, we_ifc, we_rpc, dps = _operands(64, 3, 130, 5)
    with pytest.raises(RuntimeError, match="per layer"):
        C.ptables_fwd(ifc, rpc, we_ifc, we_rpc[:2])
    with pytest.raises(RuntimeError, match="contiguous"):
        C.ptables_fwd(ifc, rpc, [we_ifc[0].t(), *we_ifc[1:]], we_rpc)
    with pytest.raises(RuntimeError, match="float32"):
        C.ptables_fwd(ifc, rpc, [we_ifc[0].half(), *we_ifc[1:]], we_rpc)
    with pytest.raises(RuntimeError, match="dP entries"):
        C.ptables_bwd(dps[:5], ifc, rpc, we_ifc, we_rpc, 1)
    with pytest.raises(RuntimeError, match="bfloat16"):
        C.ptables_bwd([dps[0].float(), *dps[1:]], ifc, rpc, we_ifc, we_rpc, 1)
    with pytest.raises(RuntimeError, match="must be \\["):
        C.ptables_bwd([dps[3], *dps[1:]], ifc, rpc, we_ifc, we_rpc, 1)
    torch.cuda.synchronize()
    # and the supported call still runs afterwards
    assert torch.equal(C.ptables_fwd(ifc, rpc, we_ifc, we_rpc)[0],
                       F.linear16(ifc, we_ifc[0]))


def _child_det():
    """Two backward calls on the same inputs, PERTGNN_DETERMINISTIC=1."""
    assert os.environ["PERTGNN_DETERMINISTIC"] == "1"
    for shape in ((256, 3, 2048, 5), (64, 3, 130, 5)):
        *ops, dps = _operands(*shape)
        a = _grouped_backward(*ops, dps, splits=3)   # the split is ignored
        b = _grouped_backward(*ops, dps, splits=3)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), shape
        for x, y in zip(a[2], b[2]):
            assert torch.equal(x, y), shape
    print("child OK det")


@gpu
@needs_gpu
def test_deterministic_child():
    env = dict(os.environ, PERTGNN_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "det"],
                       capture_output=True, text=True, timeout=300, env=env,
                       cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "child OK det" in r.stdout


# ---------------------------------------------------------------------------
# GPU: model level (3 layers, H = 256, bf16), built as tests/test_multihead.py
# builds its model
# ---------------------------------------------------------------------------

def _gpu_model(seed=1):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(seed)
    batches, stats = bench_mod.build_synthetic_batches(1, 16, seed=2, device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0).to(DEV)
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
def test_model_grouped_vs_per_layer(monkeypatch):
    """Same model, same batch, grouped path against PERTGNN_NO_PTABLE_GROUP=1
    under PERTGNN_DETERMINISTIC=1 (so every other kernel repeats itself bit
    for bit): loss and both predictions are bit-equal, every gradient the
    change does not touch is bit-equal, and the table / edge-weight gradients
    meet this file's bound against fp64 products of the dP that reached the
    grouped op."""
    from pertgnn.train.optim import FusedAdam

    model, batches = _gpu_model()
    model.train()
    b = batches[0]
    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    seen = {}
    real = F.ptables_grouped

    def spy(ifc, rpc, we_ifc, we_rpc):
        pifc, prpc = real(ifc, rpc, we_ifc, we_rpc)
        for i, p in enumerate(pifc + prpc):
            p.register_hook(lambda g, i=i: seen.__setitem__(i, g.detach().clone()))
        return pifc, prpc

    try:
        F.set_gemm_precision("bf16")
        monkeypatch.setattr(F, "ptables_grouped", spy)
        monkeypatch.delenv("PERTGNN_NO_PTABLE_GROUP", raising=False)
        loss_g, gp_g, lp_g, grads_g = _model_step(model, b)
        assert len(seen) == 6, "the grouped path did not run"
        keys_g = list(model.state_dict().keys())
        seen_grouped = dict(seen)
        seen.clear()
        monkeypatch.setenv("PERTGNN_NO_PTABLE_GROUP", "1")
        loss_p, gp_p, lp_p, grads_p = _model_step(model, b)
        assert not seen, "PERTGNN_NO_PTABLE_GROUP=1 still grouped"
        keys_p = list(model.state_dict().keys())
    finally:
        F.set_gemm_precision("fp32")
    assert torch.equal(loss_g, loss_p)
    assert torch.equal(gp_g, gp_p) and torch.equal(lp_g, lp_p)
    assert keys_g == keys_p
    assert grads_g.keys() == grads_p.keys()

    changed = {"interface_embeds.weight", "rpctype_embeds.weight"}
    changed |= {f"convs.{l}.we_{t}" for l in range(3) for t in ("ifc", "rpc")}
    for n in grads_g:
        if n not in changed:
            assert torch.equal(grads_g[n], grads_p[n]), n

    ifc, rpc = model.interface_embeds.weight.detach(), model.rpctype_embeds.weight.detach()
    we_ifc = [c.we_ifc.detach() for c in model.convs]
    we_rpc = [c.we_rpc.detach() for c in model.convs]
    dps = [seen_grouped[i] for i in range(6)]
    ref = _fp64_reference(ifc, rpc, we_ifc, we_rpc, dps)
    names = (["interface_embeds.weight", "rpctype_embeds.weight"]
             + [f"convs.{l}.we_ifc" for l in range(3)]
             + [f"convs.{l}.we_rpc" for l in range(3)])
    for n, want in zip(names, [ref[0], ref[1], *ref[2]]):
        e_new = float((grads_g[n].double() - want).abs().max())
        e_old = float((grads_p[n].double() - want).abs().max())
        bound = 2.0 * e_old + _ulp32(float(want.abs().max()))
        print(f"model {n}: grouped {e_new:.3e} per-layer {e_old:.3e} "
              f"bound {bound:.3e}")
        assert e_new <= bound, (n, e_new, e_old, bound)

    # flat_param layout: the parameters in registration order, back to back,
    # with every layer's we_ifc / we_rpc still its own [H, H] parameter
    before = [(n, p.detach().clone()) for n, p in model.named_parameters()
              if not isinstance(p, torch.nn.parameter.UninitializedParameter)]
    opt = FusedAdam(model.parameters(), lr=1e-3)
    assert opt.flat_param.numel() == sum(p.numel() for _, p in before)
    assert torch.equal(opt.flat_param,
                       torch.cat([p.reshape(-1) for _, p in before]))
    for l in range(3):
        assert tuple(dict(before)[f"convs.{l}.we_ifc"].shape) == (256, 256)


@gpu
@needs_gpu
def test_captured_steps_match_eager(monkeypatch):
    """Three GraphStepper replays with the grouped path against three eager
    steps from the same state, at the tolerance of
    test_captured_training_steps_heads4_bf16 in tests/test_multihead.py."""
    from pertgnn.train.capture import GraphStepper
    from pertgnn.train.optim import FusedAdam

    monkeypatch.delenv("PERTGNN_NO_PTABLE_GROUP", raising=False)
    model, batches = _gpu_model()
    model.train()
    calls = []
    real = F.ptables_grouped
    monkeypatch.setattr(F, "ptables_grouped",
                        lambda *a: (calls.append(1), real(*a))[1])
    try:
        F.set_gemm_precision("bf16")
        opt = FusedAdam(model.parameters(), lr=1e-3)
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
        assert calls, "the grouped path did not run"
        losses = []
        for _ in range(3):
            total, _, n = stepper.run_epoch_sums()
            losses.append(total / n)
        g_graph = opt.flat_grad.detach().clone()
        p_graph = opt.flat_param.detach().clone()
    finally:
        F.set_gemm_precision("fp32")
    print("captured", losses, "eager", eager_losses)
    for a, e in zip(losses, eager_losses):
        assert math.isfinite(a) and abs(a - e) <= 1e-2 * abs(e), (a, e)
    assert bool(g_eager.abs().max() > 0)
    assert torch.allclose(g_graph, g_eager, atol=1e-2, rtol=1e-2), \
        (g_graph - g_eager).abs().max()
    assert torch.allclose(p_graph, p_eager, atol=1e-2, rtol=1e-2), \
        (p_graph - p_eager).abs().max()


if __name__ == "__main__":
    assert sys.argv[1:] == ["det"], sys.argv
    assert HAS_GPU, "child needs a GPU"
    _child_det()
