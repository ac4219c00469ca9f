"""Inference path: forward-only fused attention with the folded BN+ReLU
epilogue, ``pertgnn.infer.Predictor``, ``evaluate(predictor=...)`` and the
``--predict`` CLI mode.

CPU tests run everywhere; GPU tests (``-m gpu``) check the HIP kernel against
the fp32 reference op run on CPU.  Run as a script (``python
tests/test_infer.py bf16-256``) this file is the child process of
``test_infer_kernel_bf16_lpr``: PERTGNN_ATTN_LPR is read once per process.
"""
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

from pertgnn.infer import Predictor, fold_bn
from pertgnn.ops import functional as F
from pertgnn.ops import reference as ref

gpu = pytest.mark.gpu
HAS_GPU = torch.cuda.is_available()
DEV = torch.device("cuda:0") if HAS_GPU else None

FP32_TOL = dict(atol=2e-4, rtol=1e-4)   # test_edge_attention_parity
BF16_TOL = dict(atol=1e-2, rtol=1e-2)   # test_gemm_bf16_parity


def _randomize_bn(model, seed=0):
    """Non-identity eval-mode BN: random buffers and affine."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for bn in model.bns:
            h = bn.weight.shape[0]
            dev = bn.weight.device
            bn.weight.copy_((torch.rand(h, generator=g) * 1.5 + 0.5).to(dev))
            bn.bias.copy_(torch.randn(h, generator=g).to(dev))
            bn.running_mean.copy_(torch.randn(h, generator=g).to(dev))
            bn.running_var.copy_((torch.rand(h, generator=g) * 1.5 + 0.5).to(dev))


def _model_forward(model, b):
    return model(b.x, b.cat_X, b.edge_index, b.edge_attr, b.pattern_num_nodes,
                 b.rt_probs, b.entry_id, b.batch, csr=b.csr,
                 num_graphs=b.num_graphs)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_fold_bn_matches_eval_batchnorm():
    g = torch.Generator().manual_seed(0)
    h, n = 32, 50
    bn = torch.nn.BatchNorm1d(h)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(h, generator=g))
        bn.bias.copy_(torch.randn(h, generator=g))
        bn.running_mean.copy_(torch.randn(h, generator=g))
        bn.running_var.copy_(torch.rand(h, generator=g) * 1.5 + 0.5)
    x = torch.randn(n, h, generator=g)
    want = torch.nn.functional.batch_norm(
        x, bn.running_mean, bn.running_var, bn.weight, bn.bias, False,
        bn.momentum, bn.eps)
    scale, shift = fold_bn(bn)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32
    assert scale.shape == (h,) and shift.shape == (h,)
    assert torch.allclose(x * scale + shift, want.detach(), atol=1e-5)


@pytest.fixture(scope="module")
def cpu_case(synthetic_workspace):
    from pertgnn.data.collate import collate
    from pertgnn.data.dataset import build_data_list
    from pertgnn.models import SAGEDeterministic

    root, (tr2data, entry2runtimes, _, runtime2pert, resource_df) = synthetic_workspace
    data_list = build_data_list(tr2data, entry2runtimes, runtime2pert,
                                resource_df, limit=24)
    b = collate(data_list[:12])
    torch.manual_seed(4)
    cat_max = max(int(s.cat_X.max()) for s in data_list)
    entry_max = max(int(s.entry_id) for s in data_list)
    ifc_max = max(int(s.edge_attr[:, 0].max()) for s in data_list)
    rpc_max = max(int(s.edge_attr[:, 1].max()) for s in data_list)

    def make():
        torch.manual_seed(4)
        m = SAGEDeterministic(9, [cat_max + 1], entry_max, ifc_max, rpc_max,
                              hidden_channels=32, num_layers=3, dropout=0.0)
        _randomize_bn(m, seed=1)
        return m

    return make, b


def test_predictor_matches_model_eval_cpu(cpu_case):
    make, b = cpu_case
    model = make()
    p = Predictor(model)
    assert not model.training
    with torch.no_grad():
        gp, lp = _model_forward(model, b)
    pred, local = p.predict_batch(b, return_local=True)
    assert pred.shape == (b.num_graphs,) and pred.dtype == torch.float32
    assert not pred.requires_grad
    assert torch.allclose(pred, gp.flatten(), atol=1e-5), \
        (pred - gp.flatten()).abs().max()
    assert torch.allclose(local, lp, atol=1e-5), (local - lp).abs().max()
    assert torch.equal(p.predict_batch(b), pred)
    # predict(): batches concatenated in order on the CPU
    both = p.predict([b, b])
    assert both.device.type == "cpu" and torch.equal(both, torch.cat([pred, pred]))
    # capture() on CPU keeps stepping eagerly
    assert p.capture([b]) == "eager" and p.mode == "eager"
    assert torch.equal(p.replay(0), pred)


def test_predictor_refresh_contract_cpu(cpu_case):
    make, b = cpu_case
    model = make()
    p = Predictor(model)
    ptrs = [t.data_ptr() for pair in p.bn_affine + p.p_tables for t in pair]
    with torch.no_grad():
        model.bns[0].weight.mul_(1.7).add_(0.3)
        model.interface_embeds.weight.add_(0.5)
        gp, _ = _model_forward(model, b)
    stale = p.predict_batch(b)
    assert not torch.allclose(stale, gp.flatten(), atol=1e-5)
    p.refresh()
    assert ptrs == [t.data_ptr() for pair in p.bn_affine + p.p_tables for t in pair]
    fresh = p.predict_batch(b)
    assert torch.allclose(fresh, gp.flatten(), atol=1e-5), \
        (fresh - gp.flatten()).abs().max()


def test_evaluate_with_predictor_cpu(cpu_case):
    """evaluate(predictor=p): same metrics as the default path, both for
    plain batches and for the resident batches of a (CPU: eager) capture."""
    from pertgnn.train import evaluate

    make, b = cpu_case
    model = make()
    base = evaluate(model, [b, b], 0.5, None)
    p = Predictor(model)
    plain = evaluate(model, [b, b], 0.5, None, predictor=p)
    resident = [b, b.to("cpu")]
    p.capture(resident)
    assert p.resident_index(resident[1]) == 1 and p.resident_index(b) == 0
    held = evaluate(model, resident, 0.5, None, predictor=p)
    for a, c, d in zip(base, plain, held):
        assert abs(c - a) <= 1e-5 * abs(a) and abs(d - a) <= 1e-5 * abs(a)


def test_infer_op_is_not_differentiable():
    csr, ea, n = _hand_graph()
    h = 8
    g = torch.Generator().manual_seed(0)
    qkvs = torch.randn(n, 4 * h, generator=g)
    pifc = torch.randn(5, h, generator=g)
    prpc = torch.randn(3, h, generator=g)
    scale = torch.ones(h)
    shift = torch.zeros(h)
    out = F.edge_attention_fused_infer(qkvs, pifc, prpc, ea, csr, scale, shift,
                                       relu=True)
    assert out.shape == (n, h) and not out.requires_grad
    for bad in ("qkvs", "pifc", "bn_scale"):
        args = dict(qkvs=qkvs, pifc=pifc, bn_scale=scale)
        args[bad] = args[bad].clone().requires_grad_(True)
        with pytest.raises(RuntimeError):
            F.edge_attention_fused_infer(args["qkvs"], args["pifc"], prpc, ea,
                                         csr, args["bn_scale"], shift)
        with torch.no_grad():  # fine once grad mode is off
            F.edge_attention_fused_infer(args["qkvs"], args["pifc"], prpc, ea,
                                         csr, args["bn_scale"], shift)


def _run_cli_cpu(argv):
    # the CLI's main() in a fresh interpreter that reports no device, so the
    # numbers are comparable with an in-process CPU evaluate()
    cmd = [sys.executable, "-c",
           "import sys, torch; torch.cuda.is_available = lambda: False; "
           "import pert_gnn; pert_gnn.main(sys.argv[1:])", *argv]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                          cwd=str(ROOT))


def test_cli_predict_round_trip(tmp_path):
    import re

    import numpy as np

    common = ["--synthetic", "--graph_type", "pert", "--num_layers", "2",
              "--hidden_channels", "16", "--batch_size", "32", "--seed", "3",
              "--processed_dir", str(tmp_path / "processed")]
    ck = tmp_path / "ck.pt"
    out = tmp_path / "pred.npy"

    # no checkpoint given / checkpoint missing: clear error, nothing written
    r = _run_cli_cpu(common + ["--predict", str(out)])
    assert r.returncode != 0 and "--checkpoint" in r.stderr, r.stderr[-2000:]
    r = _run_cli_cpu(common + ["--predict", str(out), "--checkpoint", str(ck)])
    assert r.returncode != 0 and "--checkpoint" in r.stderr, r.stderr[-2000:]
    assert not out.exists()

    r = _run_cli_cpu(common + ["--epochs", "1", "--checkpoint", str(ck)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert ck.exists()
    r = _run_cli_cpu(common + ["--checkpoint", str(ck), "--predict", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("Epoch:")]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Predict: ")]
    assert len(lines) == 1, r.stdout[-2000:]
    mt = re.match(r"Predict: n=(\d+), mae=([^,]+), mape=([^,]+), q loss=(\S+)$",
                  lines[0])
    assert mt, lines[0]

    # the same split through evaluate() on the checkpointed model
    import pert_gnn
    from pertgnn.data.collate import BatchLoader
    from pertgnn.data.dataset import split_60_20_20
    from pertgnn.data.pyg_compat import load_data_list_any
    from pertgnn.models import SAGEDeterministic
    from pertgnn.train import evaluate

    args = pert_gnn.build_parser().parse_args(common)
    _, _, runtime2graph, resource_df = pert_gnn.load_artifacts(args)
    data_list = load_data_list_any(
        os.path.join(args.processed_dir, "full_pert_data_list.pt"))
    _, _, test_list = split_60_20_20(data_list)
    model = SAGEDeterministic(
        resource_df.shape[1] - 2 + 1,
        [max(int(g["ms_id"].max()) for g in runtime2graph.values()) + 1],
        max(int(s.entry_id) for s in data_list),
        max(int(s.edge_attr[:, 0].max()) for s in data_list),
        max(int(s.edge_attr[:, 1].max()) for s in data_list),
        args.hidden_channels, args.num_layers, args.dropout)
    state = torch.load(ck, map_location="cpu", weights_only=False)
    model.load_state_dict(state["model"])
    mae, mape, qloss = evaluate(
        model, BatchLoader(test_list, args.batch_size, shuffle=False), 0.5, None)

    preds = np.load(out)
    assert preds.dtype == np.float32 and preds.shape == (len(test_list),)
    assert int(mt.group(1)) == len(test_list)
    assert abs(float(mt.group(2)) - mae) <= 1e-5 * abs(mae), (mt.group(2), mae)
    # split order: the file's MAE against the targets in order is the same
    y = np.array([float(s.y) for s in test_list], dtype=np.float64)
    assert abs(np.abs(preds - y).mean() - mae) <= 1e-4 * abs(mae)


# ---------------------------------------------------------------------------
# the hand-built graph of every kernel case
# ---------------------------------------------------------------------------

N_NODES, VI, VR, HUB = 37, 5, 3, 5


@functools.lru_cache(maxsize=None)
def _hand_graph():
    """n=37 (no multiple of the 8 rows/block at LPR 32 nor the 4 at LPR 64);
    rows 0-4 have no in-edges, row 5 has 70 (more than any LPR, sources
    repeat), the others 1-3.  Edges are destination-sorted (CSR order);
    edge_attr has the PERT layout [E,4] (stride 4, ids in columns 0/1)."""
    g = torch.Generator().manual_seed(11)
    n = N_NODES
    deg = [0] * 5 + [70] + [1 + (i % 3) for i in range(n - 6)]
    row_ptr = torch.zeros(n + 1, dtype=torch.int32)
    row_ptr[1:] = torch.tensor(deg).cumsum(0).to(torch.int32)
    e = int(row_ptr[-1])
    src = torch.randint(0, n, (e,), generator=g)
    src[row_ptr[HUB]:row_ptr[HUB] + 70] = torch.randint(0, 9, (70,), generator=g)
    ea = torch.stack([torch.randint(0, VI, (e,), generator=g),
                      torch.randint(0, VR, (e,), generator=g),
                      torch.ones(e, dtype=torch.long),
                      torch.zeros(e, dtype=torch.long)], dim=1)
    assert deg[HUB] == 70 and max(deg[6:]) == 3 and min(deg[6:]) == 1
    return (row_ptr, src.to(torch.int32)), ea, n


@functools.lru_cache(maxsize=None)
def _inputs(h, q16, p16):
    """CPU inputs; 16-bit ones are rounded here so kernel and oracle see the
    same values.  bn_scale in [0.5, 2], bn_shift of mixed sign."""
    g = torch.Generator().manual_seed(100 + h)
    qkvs = torch.randn(N_NODES, 4 * h, generator=g)
    pifc = torch.randn(VI, h, generator=g)
    prpc = torch.randn(VR, h, generator=g)
    scale = torch.rand(h, generator=g) * 1.5 + 0.5
    shift = torch.randn(h, generator=g)
    if q16:
        qkvs = qkvs.to(torch.bfloat16)
    if p16:
        pifc, prpc = pifc.to(torch.bfloat16), prpc.to(torch.bfloat16)
    return qkvs, pifc, prpc, scale, shift


@functools.lru_cache(maxsize=None)
def _oracle(h, q16, p16, affine, relu):
    """fp32 reference op on CPU, fed the (rounded) inputs widened to fp32;
    computed once per case."""
    csr, ea, _ = _hand_graph()
    qkvs, pifc, prpc, scale, shift = _inputs(h, q16, p16)
    return ref.edge_attention_fused_infer(
        qkvs.float(), pifc.float(), prpc.float(), ea, csr,
        scale if affine else None, shift if affine else None, relu)


def _check_case(h, q16, p16, out16):
    csr, ea, n = _hand_graph()
    qkvs, pifc, prpc, scale, shift = _inputs(h, q16, p16)
    d = [t.to(DEV) for t in (qkvs, pifc, prpc, scale, shift)]
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    worst = {}
    for affine in (False, True):
        for relu in (False, True):
            want = _oracle(h, q16, p16, affine, relu)
            got = F.edge_attention_fused_infer(
                d[0], d[1], d[2], ea_d, csr_d, d[3] if affine else None,
                d[4] if affine else None, relu=relu, out16=out16)
            assert got.shape == (n, h)
            assert got.dtype == (torch.bfloat16 if out16 else torch.float32)
            got = got.float().cpu()
            err = float((got - want).abs().max())
            worst[(affine, relu)] = err
            print(f"h={h} q16={q16} p16={p16} out16={out16} affine={affine} "
                  f"relu={relu}: max abs err {err:.3e}")
            tol = BF16_TOL if out16 else FP32_TOL
            assert torch.allclose(got, want, **tol), (h, q16, p16, out16,
                                                      affine, relu, err)
            if affine and relu:  # the ReLU really clips about half
                frac = float((want == 0).float().mean())
                assert 0.2 < frac < 0.8, frac
    return worst


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h", [32, 96, 256])  # guarded VPT1 / VPT2 / VEC
def test_infer_kernel_fp32(h):
    _check_case(h, q16=False, p16=False, out16=False)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_infer_kernel_bf16_512():
    _check_case(512, q16=True, p16=True, out16=True)


def _child_bf16_256():
    for p16 in (False, True):
        for out16 in (False, True):
            _check_case(256, q16=True, p16=p16, out16=out16)
    torch.cuda.synchronize()
    print("child OK lpr=" + os.environ.get("PERTGNN_ATTN_LPR", ""))


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("lpr", ["16", "32", "64"])
def test_infer_kernel_bf16_lpr(lpr):
    """bf16 qkvs at h=256, p16 x out16, per lanes-per-row variant: the knob
    is read once per process, so each value runs in a fresh child."""
    env = dict(os.environ, PERTGNN_ATTN_LPR=lpr)
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "bf16-256"],
                       capture_output=True, text=True, timeout=300, env=env,
                       cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"child OK lpr={lpr}" in r.stdout


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("h,q16", [(32, False), (96, False), (256, False),
                                   (256, True)])
def test_infer_no_epilogue_matches_training_forward(h, q16):
    import pertgnn._C as C

    csr, ea, n = _hand_graph()
    qkvs, pifc, prpc, _, _ = _inputs(h, q16, False)
    d = [t.to(DEV) for t in (qkvs, pifc, prpc)]
    csr_d = tuple(t.to(DEV) for t in csr)
    out_t, _alpha = C.edge_attn_fused_fwd(d[0], d[1], d[2], ea.to(DEV),
                                          csr_d[0], csr_d[1], False)
    out_i = F.edge_attention_fused_infer(d[0], d[1], d[2], ea.to(DEV), csr_d)
    assert torch.allclose(out_i, out_t, **FP32_TOL), (out_i - out_t).abs().max()


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_infer_empty_graph():
    n, h = 40, 256
    g = torch.Generator().manual_seed(5)
    qkvs = torch.randn(n, 4 * h, generator=g).to(DEV)
    pifc = torch.randn(VI, h, generator=g).to(DEV)
    prpc = torch.randn(VR, h, generator=g).to(DEV)
    scale = (torch.rand(h, generator=g) * 1.5 + 0.5).to(DEV)
    shift = torch.randn(h, generator=g).to(DEV)
    ea = torch.zeros(0, 2, dtype=torch.long, device=DEV)
    csr = (torch.zeros(n + 1, dtype=torch.int32, device=DEV),
           torch.zeros(0, dtype=torch.int32, device=DEV))
    out = F.edge_attention_fused_infer(qkvs, pifc, prpc, ea, csr, scale, shift,
                                       relu=True)
    want = torch.relu(qkvs[:, 3 * h:] * scale + shift)
    assert torch.allclose(out, want, atol=1e-6), (out - want).abs().max()
    # n == 0: empty result, nothing launched
    csr0 = (torch.zeros(1, dtype=torch.int32, device=DEV), csr[1])
    out0 = F.edge_attention_fused_infer(qkvs[:0], pifc, prpc, ea, csr0, scale,
                                        shift, relu=True)
    torch.cuda.synchronize()
    assert out0.shape == (0, h)


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_infer_bad_arguments():
    csr, ea, n = _hand_graph()
    h = 256
    qkvs, pifc, prpc, scale, shift = (t.to(DEV) for t in _inputs(h, False, False))
    csr_d = tuple(t.to(DEV) for t in csr)
    ea_d = ea.to(DEV)
    with pytest.raises(RuntimeError):  # wrong length
        F.edge_attention_fused_infer(qkvs, pifc, prpc, ea_d, csr_d,
                                     scale[: h - 1].contiguous(), shift)
    with pytest.raises(RuntimeError):  # wrong dtype
        F.edge_attention_fused_infer(qkvs, pifc, prpc, ea_d, csr_d,
                                     scale.half(), shift.half())
    with pytest.raises(RuntimeError):  # P tables of another width
        F.edge_attention_fused_infer(qkvs, pifc[:, :128].contiguous(),
                                     prpc[:, :128].contiguous(), ea_d, csr_d)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# model level (GPU)
# ---------------------------------------------------------------------------

def _gpu_model(n_batches):
    import bench as bench_mod
    from pertgnn.models import SAGEDeterministic

    torch.manual_seed(1)
    batches, stats = bench_mod.build_synthetic_batches(n_batches, 16, seed=2,
                                                       device=DEV)
    model = SAGEDeterministic(9, [stats["cat_max"] + 1], stats["entry_max"],
                              stats["ifc_max"], stats["rpc_max"], 256, 3,
                              0.0).to(DEV)
    _randomize_bn(model, seed=3)
    model.eval()
    return model, batches


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_predictor_matches_model_gpu(prec):
    model, batches = _gpu_model(1)
    b = batches[0]
    try:
        F.set_gemm_precision("fp32")
        with torch.no_grad():
            gp32, lp32 = _model_forward(model, b)
        gp32 = gp32.flatten()
        p = Predictor(model, precision=prec)
        assert F.gemm_precision() == prec
        # bf16 tables exactly when the training forward would use them
        want16 = prec != "fp32" and F.act16_enabled() and F.p16_enabled()
        assert all(t.dtype == (torch.bfloat16 if want16 else torch.float32)
                   for pair in p.p_tables for t in pair)
        pred, local = p.predict_batch(b, return_local=True)
    finally:
        F.set_gemm_precision("fp32")
    assert pred.dtype == torch.float32 and pred.shape == (b.num_graphs,)
    if prec == "fp32":
        assert torch.allclose(pred, gp32, atol=2e-3, rtol=1e-3), \
            (pred - gp32).abs().max()
        assert torch.allclose(local, lp32, atol=2e-3, rtol=1e-3)
    else:
        rel = (pred - gp32).abs().max() / gp32.abs().max().clamp_min(1e-6)
        print(f"{prec}: relative max error {float(rel):.4f}")
        assert rel < 0.05, rel


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_predictor_capture_replay(prec):
    model, batches = _gpu_model(2)
    try:
        p = Predictor(model, precision=prec)
        eager = [p.predict_batch(b).clone() for b in batches]
        assert p.capture(batches) == "graph" and p.mode == "graph"
        graphs = list(p._graphs)
        for _ in range(2):  # no atomics, no RNG: replays are bitwise stable
            for i in range(2):
                assert torch.equal(p.replay(i), eager[i]), i
        with torch.no_grad():
            model.bns[0].weight.mul_(1.5)
            model.rpctype_embeds.weight.add_(0.25)
            model.convs[1].w4.mul_(0.9)
        p.refresh()
        for i, b in enumerate(batches):
            new = p.predict_batch(b)
            assert not torch.equal(new, eager[i])
            assert torch.equal(p.replay(i), new), i
        assert all(a is c for a, c in zip(graphs, p._graphs))  # not re-captured
        assert torch.equal(p.predict(batches),
                           torch.cat([p.predict_batch(b) for b in batches]).cpu())
    finally:
        F.set_gemm_precision("fp32")


@gpu
@pytest.mark.skipif(not HAS_GPU, reason="no GPU available")
def test_evaluate_with_predictor():
    from pertgnn.train import evaluate

    model, batches = _gpu_model(2)
    F.set_gemm_precision("fp32")
    base = evaluate(model, batches, 0.5, DEV)
    p = Predictor(model)
    eager = evaluate(model, batches, 0.5, DEV, predictor=p)
    assert p.capture(batches) == "graph"
    replayed = evaluate(model, batches, 0.5, DEV, predictor=p)
    for name, a, c, d in zip(("mae", "mape", "qloss"), base, eager, replayed):
        print(f"{name}: model {a!r} predictor {c!r} captured {d!r}")
        assert abs(c - a) <= 1e-3 * abs(a), (name, a, c)
        assert abs(d - a) <= 1e-3 * abs(a), (name, a, d)


if __name__ == "__main__":
    assert sys.argv[1:] == ["bf16-256"], sys.argv
    assert HAS_GPU, "child needs a GPU"
    _child_bf16_256()
