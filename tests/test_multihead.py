"""Multi-head attention in ``TransformerConv``: oracle, kernels, model,
``Predictor``, checkpoint and CLI.

The independent reference of every check is the PER-HEAD COMPOSITION: the
single-head oracle (``ref.edge_attention`` without ``heads``) applied to each
head's channel slice of q/k/v/e/skip — its ``sqrt`` then sees C = H/heads —
and the results concatenated column-wise.

CPU tests run everywhere; GPU tests (``-m gpu``) compare the HIP kernels with
that composition computed on the CPU.  Run as a script (``python
tests/test_multihead.py lpr``) this file is the child process of
``test_fused_bf16_lpr``: PERTGNN_ATTN_LPR is read once per process.
"""
import copy
import functools
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

import pytest
import torch

from pertgnn.infer import Predictor
from pertgnn.ops import functional as F
from pertgnn.ops import reference as ref

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None

FP32_TOL = dict(atol=2e-4, rtol=1e-4)   # tests/test_infer.py
BF16_TOL = dict(atol=1e-2, rtol=1e-2)   # tests/test_infer.py
# gradients of the heads=1 attention op (test_edge_attention_parity in
# tests/test_gpu_ops.py): same kernels, same rounding
FP32_GRAD_TOL = dict(atol=5e-4, rtol=1e-3)


# ---------------------------------------------------------------------------
# the independent reference
# ---------------------------------------------------------------------------

def _per_head(q, k, v, e, edge_index, n, skip, heads):
    """Column-wise concatenation of the single-head oracle over the heads'
    channel slices; alpha stacked to [E, heads]."""
    c = q.shape[1] // heads
    outs, alphas = [], []
    for t in range(heads):
        sl = slice(t * c, (t + 1) * c)
        o, a = ref.edge_attention(q[:, sl], k[:, sl], v[:, sl], e[:, sl],
                                  edge_index, n, skip[:, sl],
                                  return_alpha=True)
        outs.append(o)
        alphas.append(a)
    return torch.cat(outs, dim=1), torch.stack(alphas, dim=1)


def _fused_per_head(qkvs, pifc, prpc, ea, row_ptr, csr_src, heads):
    """The fused op's operands fed to the per-head composition (fp32,
    differentiable)."""
    n = qkvs.shape[0]
    h = qkvs.shape[1] // 4
    q, k, v, skip = qkvs.split(h, dim=1)
    e = pifc.index_select(0, ea[:, 0]) + prpc.index_select(0, ea[:, 1])
    deg = (row_ptr[1:] - row_ptr[:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n), deg)
    edge_index = torch.stack([csr_src.long(), dst])
    return _per_head(q, k, v, e, edge_index, n, skip, heads)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [2, 4])
def test_oracle_equals_per_head_composition(heads):
    g = torch.Generator().manual_seed(heads)
    n, e_cnt, h = 23, 90, 32
    q, k, v, skip = (torch.randn(n, h, generator=g) for _ in range(4))
    e = torch.randn(e_cnt, h, generator=g)
    ei = torch.stack([torch.randint(0, n, (e_cnt,), generator=g),
                      torch.randint(0, n - 3, (e_cnt,), generator=g)])
    out, alpha = ref.edge_attention(q, k, v, e, ei, n, skip,
                                    return_alpha=True, heads=heads)
    want, want_alpha = _per_head(q, k, v, e, ei, n, skip, heads)
    assert alpha.shape == (e_cnt, heads)
    assert torch.allclose(out, want, atol=1e-5), (out - want).abs().max()
    assert torch.allclose(alpha, want_alpha, atol=1e-5)
    # rows without in-edges are the skip term, whatever the head count
    assert torch.equal(out[n - 3:], skip[n - 3:])
    # heads=1 through the new argument is the old oracle
    assert torch.equal(ref.edge_attention(q, k, v, e, ei, n, skip, heads=1),
                       ref.edge_attention(q, k, v, e, ei, n, skip))


def test_conv_state_dict_heads4():
    from pertgnn.models.pert_gnn import TransformerConv

    torch.manual_seed(0)
    conv = TransformerConv(40, 32, heads=4, edge_dim=64)
    assert conv.heads == 4
    sd = conv.state_dict()
    for name in ("lin_query", "lin_key", "lin_value", "lin_skip"):
        assert sd[name + ".weight"].shape == (32, 40), name
    assert sd["lin_edge.weight"].shape == (32, 64)
    assert {k for k in sd if k.endswith(".weight")} == {
        "lin_query.weight", "lin_key.weight", "lin_value.weight",
        "lin_skip.weight", "lin_edge.weight"}

    g = torch.Generator().manual_seed(1)
    n, e_cnt = 19, 60
    x = torch.randn(n, 40, generator=g)
    ee = torch.randn(e_cnt, 64, generator=g)
    ei = torch.stack([torch.randint(0, n, (e_cnt,), generator=g),
                      torch.randint(0, n, (e_cnt,), generator=g)])
    out = conv(x, ei, ee)
    conv2 = TransformerConv(40, 32, heads=4, edge_dim=64)
    assert not torch.allclose(conv2(x, ei, ee), out)
    conv2.load_state_dict(sd)
    assert torch.equal(conv2(x, ei, ee), out)
    # and the forward is the per-head composition, not the single-head op
    q = torch.nn.functional.linear(x, conv.lin_query.weight, conv.lin_query.bias)
    k = torch.nn.functional.linear(x, conv.lin_key.weight, conv.lin_key.bias)
    v = torch.nn.functional.linear(x, conv.lin_value.weight, conv.lin_value.bias)
    s = torch.nn.functional.linear(x, conv.lin_skip.weight, conv.lin_skip.bias)
    e = torch.nn.functional.linear(ee, conv.lin_edge.weight)
    want, _ = _per_head(q, k, v, e, ei, n, s, 4)
    assert torch.allclose(out, want, atol=1e-5), (out - want).abs().max()
    one = TransformerConv(40, 32, heads=1, edge_dim=64)
    one.load_state_dict(sd)
    assert not torch.allclose(one(x, ei, ee), out, atol=1e-3)


def test_conv_rejects_heads_that_do_not_divide():
    from pertgnn.models import SAGEDeterministic
    from pertgnn.models.pert_gnn import TransformerConv

    with pytest.raises(ValueError, match="heads"):
        TransformerConv(40, 32, heads=3, edge_dim=64)
    with pytest.raises(ValueError, match="heads"):
        TransformerConv(40, 32, heads=0, edge_dim=64)
    with pytest.raises(ValueError, match="heads"):
        SAGEDeterministic(9, [7], 3, 8, 3, 32, 2, 0.0, heads=3)


@pytest.fixture(scope="module")
def cpu_case(synthetic_workspace):
    from pertgnn.data.collate import collate
    from pertgnn.data.dataset import build_data_list
    from pertgnn.models import SAGEDeterministic

    root, (tr2data, entry2runtimes, _, runtime2pert, resource_df) = synthetic_workspace
    data_list = build_data_list(tr2data, entry2runtimes, runtime2pert,
                                resource_df, limit=24)
    b = collate(data_list[:12])
    cat_max = max(int(s.cat_X.max()) for s in data_list)
    entry_max = max(int(s.entry_id) for s in data_list)
    ifc_max = max(int(s.edge_attr[:, 0].max()) for s in data_list)
    rpc_max = max(int(s.edge_attr[:, 1].max()) for s in data_list)

    def make(heads):
        torch.manual_seed(4)
        return SAGEDeterministic(9, [cat_max + 1], entry_max, ifc_max, rpc_max,
                                 hidden_channels=32, num_layers=3, dropout=0.0,
                                 heads=heads)

    return make, b


def _model_forward(model, b):
    return model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                 b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                 num_graphs=b.num_graphs)


def test_model_gradients_match_per_head_autograd(cpu_case, monkeypatch):
    """SAGEDeterministic(heads=2) forward+backward against autograd through
    the per-head composition: the model's attention op is swapped for the
    composition in a second run of the same weights."""
    make, b = cpu_case
    model = make(2)
    assert model.heads == 2 and all(c.heads == 2 for c in model.convs)
    model.train()

    def run():
        model.zero_grad()
        gp, lp = _model_forward(model, b)
        (F.quantile_loss(b.y, gp.flatten(), 0.5) + lp.mean()).backward()
        return gp.detach().clone(), {
            n: p.grad.clone() for n, p in model.named_parameters()
            if p.grad is not None}

    bn_state = copy.deepcopy([bn.state_dict() for bn in model.bns])
    gp, grads = run()
    for bn, sd in zip(model.bns, bn_state):
        bn.load_state_dict(sd)

    seen = []

    def composed(q, k, v, e, skip, edge_index, num_nodes, csr=None, heads=1):
        seen.append(heads)
        return _per_head(q, k, v, e, edge_index, num_nodes, skip, heads)[0]

    monkeypatch.setattr(F, "edge_attention", composed)
    gp_want, grads_want = run()
    assert seen == [2, 2, 2]
    assert torch.allclose(gp, gp_want, atol=1e-5), (gp - gp_want).abs().max()
    assert set(grads) == set(grads_want) and len(grads) > 10
    for n in grads:
        assert torch.allclose(grads[n], grads_want[n], atol=1e-5), \
            (n, (grads[n] - grads_want[n]).abs().max())
    # the heads really change the function
    one = make(1)
    one.load_state_dict(model.state_dict())
    one.train()
    gp1, _ = _model_forward(one, b)
    assert not torch.allclose(gp1.detach(), gp, atol=1e-4)


def test_predictor_heads2_matches_model_eval_cpu(cpu_case):
    make, b = cpu_case
    model = make(2)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for bn in model.bns:  # non-identity eval-mode BN
            bn.running_mean.copy_(torch.randn(32, generator=g))
            bn.running_var.copy_(torch.rand(32, generator=g) * 1.5 + 0.5)
            bn.weight.copy_(torch.rand(32, generator=g) * 1.5 + 0.5)
            bn.bias.copy_(torch.randn(32, generator=g))
    p = Predictor(model)
    with torch.no_grad():
        gp, lp = _model_forward(model, b)
    pred, local = p.predict_batch(b, return_local=True)
    assert torch.allclose(pred, gp.flatten(), atol=1e-5), \
        (pred - gp.flatten()).abs().max()
    assert torch.allclose(local, lp, atol=1e-5), (local - lp).abs().max()


def test_checkpoint_records_heads(tmp_path):
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train import load_checkpoint, save_checkpoint

    def make(heads):
        return SAGEDeterministic(9, [7], 3, 8, 3, 32, 2, 0.0, heads=heads)

    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, make(4), None, epoch=2)
    state = torch.load(path, weights_only=False)
    assert state["heads"] == 4
    assert load_checkpoint(path, make(4))[0] == 2
    with pytest.raises(ValueError, match=r"heads=4.*heads=1"):
        load_checkpoint(path, make(1))
    # a checkpoint from before the field existed means heads=1
    del state["heads"]
    torch.save(state, path)
    assert load_checkpoint(path, make(1))[0] == 2
    with pytest.raises(ValueError, match=r"heads=1.*heads=2"):
        load_checkpoint(path, make(2))


def _run_cli_cpu(argv):
    # the CLI's main() in a fresh interpreter that reports no device
    cmd = [sys.executable, "-c",
           "import sys, torch; torch.cuda.is_available = lambda: False; "
           "import pert_gnn; pert_gnn.main(sys.argv[1:])", *argv]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                          cwd=str(ROOT))


def test_cli_heads_and_resume_mismatch(tmp_path):
    common = ["--synthetic", "--graph_type", "pert", "--num_layers", "2",
              "--hidden_channels", "16", "--batch_size", "32", "--seed", "3",
              "--epochs", "1", "--processed_dir", str(tmp_path / "processed")]
    ck = tmp_path / "ck.pt"
    r = _run_cli_cpu(common + ["--heads", "2", "--checkpoint", str(ck)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len([l for l in r.stdout.splitlines() if l.startswith("Epoch:")]) == 1
    assert torch.load(ck, weights_only=False)["heads"] == 2
    r = _run_cli_cpu(common + ["--heads", "1", "--checkpoint", str(ck)])
    assert r.returncode != 0
    assert "heads=2" in r.stderr and "heads=1" in r.stderr, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("Epoch:")]


# ---------------------------------------------------------------------------
# the hand-built graph of every kernel case
# ---------------------------------------------------------------------------

N_NODES, VI, VR, HUB, ISOLATED = 71, 5, 3, 9, 4


@functools.lru_cache(maxsize=None)
def _hand_graph():
    """n=71: odd, so the last wave has an empty sub-row at 2 and at 4 rows
    per wave, and no multiple of the 4/8/16 rows per block.  Node 4 has no
    in-edges; node 9 has 40 (more than any lanes-per-row but 64, and more
    than every lanes-per-head, so the strided finalize loops wrap), from
    only 6 sources, so (src,dst) pairs repeat; nodes 20..29 have exactly
    one; (1,0) appears three times more.  Returns the CSR/CSC arrays of
    ``build_csr`` and edge_attr [E,4] in CSR order."""
    from pertgnn.data.collate import build_csr

    g = torch.Generator().manual_seed(17)
    n = N_NODES
    src, dst = [], []
    for i in range(n):
        if i == ISOLATED:
            continue
        if i == HUB:
            deg = 40
        elif 20 <= i < 30:
            deg = 1
        else:
            deg = 2 + i % 3
        s = (torch.randint(0, 6, (deg,), generator=g) if i == HUB
             else torch.randint(0, n, (deg,), generator=g))
        src += s.tolist()
        dst += [i] * deg
    src += [1, 1, 1]
    dst += [0, 0, 0]
    ei = torch.tensor([src, dst])
    perm, row_ptr, csr_src, col_ptr, csc_dst, csc_eid = build_csr(ei, n)
    e = ei.shape[1]
    ea = torch.stack([torch.randint(0, VI, (e,), generator=g),
                      torch.randint(0, VR, (e,), generator=g),
                      torch.ones(e, dtype=torch.long),
                      torch.zeros(e, dtype=torch.long)], dim=1)
    deg = (row_ptr[1:] - row_ptr[:-1]).tolist()
    assert deg[ISOLATED] == 0 and deg[HUB] == 40 and deg[20:30] == [1] * 10
    return (row_ptr, csr_src, col_ptr, csc_dst, csc_eid), ea, n


@functools.lru_cache(maxsize=None)
def _inputs(h, b16):
    """CPU operands and the upstream gradient; the 16-bit ones are rounded
    here so kernel and reference see the same values."""
    g = torch.Generator().manual_seed(200 + h)
    qkvs = torch.randn(N_NODES, 4 * h, generator=g)
    pifc = torch.randn(VI, h, generator=g)
    prpc = torch.randn(VR, h, generator=g)
    gout = torch.randn(N_NODES, h, generator=g)
    scale = torch.rand(h, generator=g) * 1.5 + 0.5
    shift = torch.randn(h, generator=g)
    if b16:
        qkvs, pifc, prpc, gout = (t.to(torch.bfloat16)
                                  for t in (qkvs, pifc, prpc, gout))
    return qkvs, pifc, prpc, gout, scale, shift


@functools.lru_cache(maxsize=None)
def _reference(h, heads, b16):
    """Per-head composition on the CPU in fp32 (on the rounded operands for
    a 16-bit case), with its autograd gradients; computed once per case.
    ``de_abs`` [V] sums |d e_edge| per vocabulary row (for the bf16 bound
    of the table gradients)."""
    csr, ea, _ = _hand_graph()
    qkvs, pifc, prpc, gout, _, _ = (t.float().clone()
                                    for t in _inputs(h, b16))
    qkvs.requires_grad_(True)
    pifc.requires_grad_(True)
    prpc.requires_grad_(True)
    e = (pifc.index_select(0, ea[:, 0])
         + prpc.index_select(0, ea[:, 1])).detach().requires_grad_(True)
    n = qkvs.shape[0]
    q, k, v, skip = qkvs.split(h, dim=1)
    deg = (csr[0][1:] - csr[0][:-1]).long()
    dst = torch.repeat_interleave(torch.arange(n), deg)
    out_e, _ = _per_head(q.detach(), k.detach(), v.detach(), e,
                         torch.stack([csr[1].long(), dst]), n, skip.detach(),
                         heads)
    (de,) = torch.autograd.grad((out_e * gout).sum(), e)
    out, alpha = _fused_per_head(qkvs, pifc, prpc, ea, csr[0], csr[1], heads)
    (out * gout).sum().backward()
    de_abs = de.abs()
    abs_ifc = torch.zeros(VI, h).index_add_(0, ea[:, 0], de_abs)
    abs_rpc = torch.zeros(VR, h).index_add_(0, ea[:, 1], de_abs)
    return dict(out=out.detach(), alpha=alpha.detach(), dqkvs=qkvs.grad,
                dpifc=pifc.grad, dprpc=prpc.grad, abs_ifc=abs_ifc,
                abs_rpc=abs_rpc)


def _close(name, got, want, tol, extra_atol=None):
    got = got.detach().float().cpu()
    err = float((got - want).abs().max())
    print(f"  {name}: max abs err {err:.3e} (max |ref| {float(want.abs().max()):.3e})")
    bound = tol["atol"] + tol["rtol"] * want.abs()
    if extra_atol is not None:
        bound = bound + extra_atol
    bad = (got - want).abs() > bound
    assert not bool(bad.any()), (name, err, int(bad.sum()))


def _run_fused(h, heads, b16):
    """Training forward + backward of the fused op on the device."""
    import pertgnn._C as C

    csr, ea, n = _hand_graph()
    qkvs, pifc, prpc, gout, _, _ = (t.clone().to(DEV)
                                    for t in _inputs(h, b16))
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    _, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea_d, csr_d[0],
                                     csr_d[1], b16, heads)
    for t in (qkvs, pifc, prpc):
        t.requires_grad_(True)
    out = F.edge_attention_fused(qkvs, pifc, prpc, ea_d, csr_d, out16=b16,
                                 heads=heads)
    out.backward(gout)
    torch.cuda.synchronize()
    return out, alpha, qkvs.grad, pifc.grad, prpc.grad


def _check_fused(h, heads, b16):
    print(f"h={h} heads={heads} bf16={b16}")
    want = _reference(h, heads, b16)
    out, alpha, dqkvs, dpifc, dprpc = _run_fused(h, heads, b16)
    e_cnt = _hand_graph()[1].shape[0]
    assert alpha.shape == (e_cnt, heads) and alpha.dtype == torch.float32
    assert out.dtype == (torch.bfloat16 if b16 else torch.float32)
    assert dqkvs.dtype == out.dtype and dpifc.dtype == out.dtype
    if not b16:
        _close("out", out, want["out"], FP32_TOL)
        _close("alpha", alpha, want["alpha"], FP32_TOL)
        _close("dqkvs", dqkvs, want["dqkvs"], FP32_GRAD_TOL)
        _close("dP_ifc", dpifc, want["dpifc"], FP32_GRAD_TOL)
        _close("dP_rpc", dprpc, want["dprpc"], FP32_GRAD_TOL)
        return
    _close("out", out, want["out"], BF16_TOL)
    _close("alpha", alpha, want["alpha"], BF16_TOL)
    _close("dqkvs", dqkvs, want["dqkvs"], BF16_TOL)
    # dP[v] sums the per-edge gradients de AFTER each was stored as bf16
    # (round to nearest: relative error <= 2^-9 per term, and the errors of
    # one vocabulary row add up), so on top of BF16_TOL for the final bf16
    # value the bound carries 2^-9 * sum_e |de_e| of that row
    _close("dP_ifc", dpifc, want["dpifc"], BF16_TOL, want["abs_ifc"] * 2.0 ** -9)
    _close("dP_rpc", dprpc, want["dprpc"], BF16_TOL, want["abs_rpc"] * 2.0 ** -9)


# ---------------------------------------------------------------------------
# kernels (GPU)
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h,heads", [
    (256, 2), (256, 8), (256, 32),      # VEC: 32, 8 and 2 lanes per head
    (32, 4), (96, 3), (128, 2),         # per-column heads: C = 8, 32, 64
])
def test_fused_fp32_fwd_bwd(h, heads):
    _check_fused(h, heads, b16=False)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h,heads", [(256, 4), (512, 4)])
def test_fused_bf16_fwd_bwd(h, heads):
    """bf16 qkvs, bf16 P tables, bf16 out and upstream gradient."""
    _check_fused(h, heads, b16=True)


def _expect_shape_error(fn):
    try:
        res = fn()
    except RuntimeError as exc:
        assert "unsupported shape" in str(exc), exc
        return
    raise AssertionError(f"no shape error, got {type(res)}")


def _child_lpr():
    lpr = os.environ["PERTGNN_ATTN_LPR"]
    _check_fused(256, 4, b16=True)
    if lpr == "32":
        # 64 heads of 4 channels: a lane's 8 contiguous columns would
        # straddle two heads at 32 lanes per row
        import pertgnn._C as C

        csr, ea, _ = _hand_graph()
        qkvs, pifc, prpc, gout, scale, shift = (
            t.to(DEV) for t in _inputs(256, True))
        csr_d = tuple(t.to(DEV) for t in csr)
        ea_d = ea.to(DEV)
        _expect_shape_error(lambda: C.edge_attn_fused_fwd(
            qkvs, pifc, prpc, ea_d, csr_d[0], csr_d[1], True, 64))
        _expect_shape_error(lambda: F.edge_attention_fused_infer(
            qkvs, pifc, prpc, ea_d, csr_d, scale, shift, relu=True,
            out16=True, heads=64))
        alpha = torch.zeros(ea.shape[0], 64, device=DEV)
        _expect_shape_error(lambda: C.edge_attn_fused_bwd(
            gout, qkvs, pifc, prpc, ea_d, alpha, *csr_d, 64))
    torch.cuda.synchronize()
    print("child OK lpr=" + lpr)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("lpr", ["16", "32", "64"])
def test_fused_bf16_lpr(lpr):
    """(256,4) bf16 per lanes-per-row variant (4, 8 and 16 lanes per head);
    the knob is read once per process, so each value runs in a fresh child.
    The 32 child also checks that (256,64) is the shape error there."""
    env = dict(os.environ, PERTGNN_ATTN_LPR=lpr)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "lpr"],
                       capture_output=True, text=True, timeout=300, env=env,
                       cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"child OK lpr={lpr}" in r.stdout


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h,heads,b16", [(32, 4, False), (256, 8, False),
                                         (256, 4, True)])
def test_infer_kernel_heads(h, heads, b16):
    """Forward-only kernel with the affine+ReLU epilogue: equals the
    training forward followed by the folded BN and the ReLU, and the
    per-head composition put through the same epilogue."""
    import pertgnn._C as C

    csr, ea, n = _hand_graph()
    qkvs, pifc, prpc, _, scale, shift = (t.to(DEV) for t in _inputs(h, b16))
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    tol = BF16_TOL if b16 else FP32_TOL
    got = F.edge_attention_fused_infer(qkvs, pifc, prpc, ea_d, csr_d, scale,
                                       shift, relu=True, out16=b16,
                                       heads=heads)
    assert got.shape == (n, h)
    assert got.dtype == (torch.bfloat16 if b16 else torch.float32)
    out_t, _ = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea_d, csr_d[0],
                                     csr_d[1], False, heads)
    want_t = torch.relu(out_t * scale + shift)
    _close("vs training forward + folded BN", got, want_t.cpu(), tol)
    want = torch.relu(_reference(h, heads, b16)["out"] * scale.cpu()
                      + shift.cpu())
    _close("vs per-head composition", got, want, tol)
    frac = float((want == 0).float().mean())
    assert 0.2 < frac < 0.8, frac  # the ReLU really clips
    # no epilogue: the plain aggregate
    plain = F.edge_attention_fused_infer(qkvs, pifc, prpc, ea_d, csr_d,
                                         heads=heads)
    _close("no epilogue", plain, _reference(h, heads, b16)["out"], tol)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h,b16", [(256, False), (64, False), (256, True)])
def test_heads1_is_bitwise_the_call_without_the_argument(h, b16, monkeypatch):
    """``heads=1`` selects the very kernels of a call without the argument:
    out, alpha and all gradients are bitwise equal.  The table gradients
    take the deterministic grouped scatter here so that a bitwise
    comparison of two runs means something."""
    import pertgnn._C as C

    monkeypatch.setenv("PERTGNN_DETERMINISTIC", "1")
    csr, ea, _ = _hand_graph()
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)

    def run(**kw):
        qkvs, pifc, prpc, gout, _, _ = (t.clone().to(DEV)
                                        for t in _inputs(h, b16))
        extra = tuple(kw.values())
        _, alpha = C.edge_attn_fused_fwd(qkvs, pifc, prpc, ea_d, csr_d[0],
                                         csr_d[1], b16, *extra)
        for t in (qkvs, pifc, prpc):
            t.requires_grad_(True)
        out = F.edge_attention_fused(qkvs, pifc, prpc, ea_d, csr_d,
                                     out16=b16, **kw)
        out.backward(gout)
        return out.detach(), alpha, qkvs.grad, pifc.grad, prpc.grad

    a = run()
    c = run(heads=1)
    assert a[1].shape == (ea.shape[0],)
    for name, x, y in zip(("out", "alpha", "dqkvs", "dP_ifc", "dP_rpc"), a, c):
        assert x.shape == y.shape and torch.equal(x, y), name


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_unsupported_head_mapping_is_an_error():
    """(96,2): 48 channels per head do not divide the 64 lanes.  The call
    raises the shape error, returns no tensor, and the process goes on."""
    import pertgnn._C as C

    csr, ea, n = _hand_graph()
    qkvs, pifc, prpc, gout, scale, shift = (
        t.to(DEV) for t in _inputs(96, False))
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    _expect_shape_error(lambda: F.edge_attention_fused(
        qkvs, pifc, prpc, ea_d, csr_d, heads=2))
    _expect_shape_error(lambda: F.edge_attention_fused_infer(
        qkvs, pifc, prpc, ea_d, csr_d, scale, shift, relu=True, heads=2))
    alpha = torch.zeros(ea.shape[0], 2, device=DEV)
    _expect_shape_error(lambda: C.edge_attn_fused_bwd(
        gout, qkvs, pifc, prpc, ea_d, alpha, *csr_d, 2))
    with pytest.raises(RuntimeError, match="heads must divide"):
        F.edge_attention_fused(qkvs, pifc, prpc, ea_d, csr_d, heads=5)
    torch.cuda.synchronize()
    # the supported neighbour still runs afterwards
    out = F.edge_attention_fused(qkvs, pifc, prpc, ea_d, csr_d, heads=3)
    _close("(96,3) after the errors", out, _reference(96, 3, False)["out"],
           FP32_TOL)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_reference_layout_op_runs_per_head():
    """``ops.edge_attention`` on device tensors: the single-head kernel once
    per head on channel slices, forward and gradients."""
    csr, ea, n = _hand_graph()
    h, heads = 64, 4
    g = torch.Generator().manual_seed(3)
    cpu = [torch.randn(n, h, generator=g) for _ in range(3)]
    cpu.append(torch.randn(ea.shape[0], h, generator=g))
    cpu.append(torch.randn(n, h, generator=g))
    gout = torch.randn(n, h, generator=g)
    deg = (csr[0][1:] - csr[0][:-1]).long()
    ei = torch.stack([csr[1].long(),
                      torch.repeat_interleave(torch.arange(n), deg)])
    ref_in = [t.clone().requires_grad_(True) for t in cpu]
    want, _ = _per_head(ref_in[0], ref_in[1], ref_in[2], ref_in[3], ei, n,
                        ref_in[4], heads)
    want.backward(gout)
    dev_in = [t.to(DEV).requires_grad_(True) for t in cpu]
    out = F.edge_attention(dev_in[0], dev_in[1], dev_in[2], dev_in[3],
                           dev_in[4], ei.to(DEV), n,
                           csr=tuple(t.to(DEV) for t in csr), heads=heads)
    out.backward(gout.to(DEV))
    _close("out", out, want.detach(), FP32_TOL)
    for name, a, c in zip("qkves", dev_in, ref_in):
        _close("d" + name, a.grad, c.grad, FP32_GRAD_TOL)


# ---------------------------------------------------------------------------
# model level (GPU): heads=4, H=256, bf16
# ---------------------------------------------------------------------------

def _gpu_model(n_batches, heads=4):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(n_batches, 16, seed=2,
                                                       device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0, heads=heads).to(DEV)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for bn in model.bns:
            bn.weight.copy_((torch.rand(256, generator=g) * 1.5 + 0.5).to(DEV))
            bn.bias.copy_(torch.randn(256, generator=g).to(DEV))
            bn.running_mean.copy_(torch.randn(256, generator=g).to(DEV))
            bn.running_var.copy_((torch.rand(256, generator=g) * 1.5 + 0.5).to(DEV))
    return model, batches


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_predictor_heads4_bf16_gpu():
    """Predictor against model.eval() at the tolerance of
    test_predictor_matches_model_gpu (bf16 vs the fp32 forward: 5% of the
    largest prediction), against the per-head CPU model, and capture +
    replay against eager."""
    model, batches = _gpu_model(2)
    model.eval()
    try:
        F.set_gemm_precision("fp32")
        with torch.no_grad():
            gp32 = [_model_forward(model, b)[0].flatten() for b in batches]
        cpu_model = copy.deepcopy(model).cpu()
        with torch.no_grad():
            gp_cpu = _model_forward(cpu_model, batches[0].to("cpu"))[0].flatten()
        assert torch.allclose(gp32[0].cpu(), gp_cpu, atol=2e-3, rtol=1e-3), \
            (gp32[0].cpu() - gp_cpu).abs().max()
        p = Predictor(model, precision="bf16")
        assert all(t.dtype == torch.bfloat16 for pair in p.p_tables for t in pair)
        eager = [p.predict_batch(b).clone() for b in batches]
        for e, w in zip(eager, gp32):
            rel = (e - w).abs().max() / w.abs().max().clamp_min(1e-6)
            print(f"bf16 heads=4: relative max error {float(rel):.4f}")
            assert rel < 0.05, rel
        # the heads are really in the prediction
        one = copy.deepcopy(model)
        one.heads = 1
        for c in one.convs:
            c.heads = 1
        p1 = Predictor(one, precision="bf16")
        assert not torch.allclose(p1.predict_batch(batches[0]), eager[0],
                                  atol=1e-3)
        assert p.capture(batches) == "graph"
        for _ in range(2):
            for i in range(2):
                assert torch.equal(p.replay(i), eager[i]), i
    finally:
        F.set_gemm_precision("fp32")


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_captured_training_steps_heads4_bf16():
    """Three captured training steps on one resident batch: finite,
    non-increasing loss, and the first replay's gradients are the eager
    step's.  Table and weight gradients use atomics and split-K sums, so two
    runs of the same step differ in summation order: the comparison uses the
    bound test_deterministic_mode_bitwise puts on exactly that difference."""
    from pertgnn.train.capture import GraphStepper
    from pertgnn.train.optim import FusedAdam

    model, batches = _gpu_model(1)
    model.train()
    try:
        F.set_gemm_precision("bf16")
        opt = FusedAdam(model.parameters(), lr=1e-3)
        stepper = GraphStepper(model, opt, None, None, 0.5, DEV, batches)
        snap = stepper._snapshot()
        stepper._full_step(0)
        torch.cuda.synchronize()
        g_eager = opt.flat_grad.detach().clone()
        loss_eager = float(stepper.acc[0]) / batches[0].num_graphs
        stepper._restore(snap)
        assert stepper.capture() == "full"
        losses = []
        for step in range(3):
            total, _, n = stepper.run_epoch_sums()
            losses.append(total / n)
            if step == 0:
                g_graph = opt.flat_grad.detach().clone()
        print("captured losses", losses, "eager first loss", loss_eager)
        assert all(torch.isfinite(torch.tensor(losses)))
        assert losses[1] <= losses[0] and losses[2] <= losses[1], losses
        assert abs(losses[0] - loss_eager) <= 1e-2 * abs(loss_eager)
        assert bool(g_eager.abs().max() > 0)
        assert torch.allclose(g_graph, g_eager, atol=1e-2, rtol=1e-2), \
            (g_graph - g_eager).abs().max()
    finally:
        F.set_gemm_precision("fp32")


if __name__ == "__main__":
    assert sys.argv[1:] == ["lpr"], sys.argv
    assert HAS_GPU, "child needs a GPU"
    _child_lpr()
