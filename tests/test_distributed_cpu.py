"""Multi-process CPU tests of the DDP engine (gloo backend, world_size 2).

Validates the SURVEY.md §4.5 requirement: bucketing/overlap logic on a fake
(CPU) process group, and 2x(bs=b) DDP == 1x(bs=2b) single-process gradient
equivalence.
"""
import os

import pytest
import torch
import torch.multiprocessing as mp

from pertgnn.models import SAGEDeterministic


def _make_inputs(seed, n=16, e=30, b=2, h=8):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 9, generator=g)
    cat_X = torch.randint(0, 5, (n, 1), generator=g)
    edge_index = torch.stack([
        torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)
    ])
    edge_attr = torch.stack([
        torch.randint(0, 4, (e,), generator=g), torch.randint(0, 3, (e,), generator=g)
    ], dim=1)
    pnn = torch.randint(1, 4, (n, 1), generator=g).float()
    probs = torch.rand(n, 1, generator=g)
    entry_id = torch.randint(0, 4, (b,), generator=g)
    batch = torch.sort(torch.randint(0, b, (n,), generator=g)).values
    y = torch.rand(b, generator=g) * 5
    return x, cat_X, edge_index, edge_attr, pnn, probs, entry_id, batch, y


def _build_model():
    torch.manual_seed(42)
    return SAGEDeterministic(9, [5], 3, 3, 2, hidden_channels=8, num_layers=1, dropout=0.0)


def _loss_on(model, seed):
    from pertgnn.ops import functional as F
    x, cat_X, ei, ea, pnn, probs, entry, batch, y = _make_inputs(seed)
    b = int(batch.max()) + 1
    gp, _ = model(x, cat_X, ei, ea, pnn, probs, entry[:b], batch)
    return F.quantile_loss(y[:b], gp.flatten(), 0.5)


def _worker(rank, world_size, port, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    from pertgnn.parallel import Comm, GradBucketAllReduce

    comm = Comm(backend="gloo")
    model = _build_model()
    comm.broadcast_module_(model)
    engine = GradBucketAllReduce(model, comm, bucket_cap_mb=0.001)  # force several buckets
    model.train()
    engine.reset()
    loss = _loss_on(model, seed=100 + rank)
    loss.backward()
    engine.finalize()
    # pass by value (numpy) — mp.Queue tensor fd-sharing breaks once the child exits
    grads = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters() if p.grad is not None}
    # metric all-reduce check
    s = comm.all_reduce_scalar(float(rank + 1))
    result_queue.put((rank, grads, s))
    comm.barrier()
    comm.finalize()


@pytest.mark.timeout(120)
def test_ddp_grads_match_average_of_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29511
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    results.sort(key=lambda t: t[0])
    (_, g0, s0), (_, g1, s1) = results
    assert s0 == s1 == 3.0  # 1 + 2

    # single-process reference: average of the two per-rank gradients
    model = _build_model()
    expected = {}
    for seed in (100, 101):
        m = _build_model()
        loss = _loss_on(m, seed)
        loss.backward()
        for n, p in m.named_parameters():
            if p.grad is not None:
                expected[n] = expected.get(n, 0) + p.grad / 2

    for n in expected:
        assert torch.allclose(torch.from_numpy(g0[n]), expected[n], atol=1e-6), n
        assert torch.allclose(torch.from_numpy(g0[n]), torch.from_numpy(g1[n]), atol=1e-6), n


def _worker_flat(rank, world_size, port, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    from pertgnn.parallel import Comm
    from pertgnn.train.optim import FlatGradAllReduce, FusedAdam

    comm = Comm(backend="gloo")
    model = _build_model()
    comm.broadcast_module_(model)
    opt = FusedAdam(model.parameters(), lr=1e-2)
    engine = FlatGradAllReduce(opt, comm, bucket_cap_mb=0.0005)  # many buckets
    model.train()
    for step in range(2):
        opt.zero_grad()
        engine.reset()
        loss = _loss_on(model, seed=200 + rank)
        loss.backward()
        engine.finalize()
        opt.step()
    grads = opt.flat_grad.numpy().copy()
    params = opt.flat_param.numpy().copy()
    result_queue.put((rank, grads, params))
    comm.barrier()
    comm.finalize()


@pytest.mark.timeout(120)
def test_flat_engine_ranks_stay_in_sync():
    """FusedAdam + FlatGradAllReduce: after identical averaged grads, both
    ranks' flat parameters must be bitwise identical."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_flat, args=(r, world, 29513, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    results.sort(key=lambda t: t[0])
    (_, g0, p0), (_, g1, p1) = results
    import numpy as np
    assert np.array_equal(g0, g1), "averaged grads must match bitwise"
    assert np.array_equal(p0, p1), "params must stay in sync"
    assert np.abs(g0).sum() > 0


def _worker_syncbn(rank, world_size, port, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    from pertgnn.ops.functional import batchnorm_relu
    from pertgnn.parallel import Comm

    comm = Comm(backend="gloo")
    torch.manual_seed(7)
    full = torch.randn(8, 6) * 2 + 1   # global batch of 8 rows
    x = full[rank * 4:(rank + 1) * 4].clone().requires_grad_(True)
    gamma = torch.rand(6).add_(0.5).requires_grad_(True)
    beta = torch.randn(6).requires_grad_(True)
    rm = torch.zeros(6)
    rv = torch.ones(6)
    y = batchnorm_relu(x, gamma, beta, rm, rv, 0.1, 1e-5, True, fuse_relu=True, comm=comm)
    # local-mean loss (reference loop semantics per rank)
    loss = y.pow(2).mean()
    loss.backward()
    result_queue.put((rank, x.grad.numpy().copy(), gamma.grad.numpy().copy(),
                      beta.grad.numpy().copy(), rm.numpy().copy(), rv.numpy().copy(),
                      y.detach().numpy().copy()))
    comm.barrier()
    comm.finalize()


@pytest.mark.timeout(120)
def test_sync_bn_matches_single_process():
    """2-rank sync-BN == single-process BN over the concatenated batch:
    forward outputs, running stats, and (after the DDP 1/W averaging) every
    gradient."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_syncbn, args=(r, world, 29514, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=100) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    results.sort(key=lambda t: t[0])

    # single-process reference over the concatenated batch
    torch.manual_seed(7)
    full = torch.randn(8, 6) * 2 + 1
    x = full.clone().requires_grad_(True)
    gamma = torch.rand(6).add_(0.5).requires_grad_(True)
    beta = torch.randn(6).requires_grad_(True)
    rm = torch.zeros(6)
    rv = torch.ones(6)
    y = torch.nn.functional.relu(torch.nn.functional.batch_norm(
        x, rm, rv, gamma, beta, True, 0.1, 1e-5))
    # average of per-rank local-mean losses == mean over global batch
    loss = (y[:4].pow(2).mean() + y[4:].pow(2).mean()) / 2
    loss.backward()

    (_, dx0, dg0, db0, rm0, rv0, y0), (_, dx1, dg1, db1, rm1, rv1, y1) = results
    import numpy as np
    assert np.allclose(np.concatenate([y0, y1]), y.detach().numpy(), atol=1e-5)
    assert np.allclose(rm0, rm.numpy(), atol=1e-6) and np.allclose(rm1, rm.numpy(), atol=1e-6)
    assert np.allclose(rv0, rv.numpy(), atol=1e-5)
    # DDP engine averages grads across ranks: (g0+g1)/2 == single-process
    assert np.allclose((dg0 + dg1) / 2, gamma.grad.numpy(), atol=1e-5)
    assert np.allclose((db0 + db1) / 2, beta.grad.numpy(), atol=1e-5)
    # dx: per-rank dx must equal W * single-process dx rows (engine divides
    # weight grads, and dx feeds W-averaged weight grads upstream)
    assert np.allclose(dx0, 2 * x.grad.numpy()[:4], atol=1e-5), np.abs(dx0 - 2*x.grad.numpy()[:4]).max()
    assert np.allclose(dx1, 2 * x.grad.numpy()[4:], atol=1e-5)


def _worker_train_equiv(rank, world_size, port, result_queue):
    """2-rank DDP training with sync-BN on half-batches."""
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    from pertgnn.ops import functional as F
    from pertgnn.parallel import Comm
    from pertgnn.train.optim import FlatGradAllReduce, FusedAdam

    comm = Comm(backend="gloo")
    model = _build_model()
    comm.broadcast_module_(model)
    model.enable_sync_bn(comm)
    opt = FusedAdam(model.parameters(), lr=1e-2)
    engine = FlatGradAllReduce(opt, comm)
    model.train()
    losses = []
    for step in range(4):
        x, cat_X, ei, ea, pnn, probs, entry_id, batch, y = _make_inputs(
            seed=300 + step, n=24, e=50, b=4)
        inp = dict(x=x, cat_X=cat_X, edge_index=ei, edge_attr=ea,
                   pattern_num_nodes=pnn, pattern_probs=probs,
                   entry_id=entry_id, batch=batch)
        # shard: rank r takes graphs [2r, 2r+2) — emulate per-rank half batch
        sel = (inp["batch"] >= rank * 2) & (inp["batch"] < rank * 2 + 2)
        nidx = sel.nonzero().flatten()
        remap = -torch.ones(24, dtype=torch.long)
        remap[nidx] = torch.arange(nidx.numel())
        emask = sel[inp["edge_index"][0]] & sel[inp["edge_index"][1]]
        local = dict(
            x=inp["x"][nidx],
            cat_X=inp["cat_X"][nidx],
            edge_index=remap[inp["edge_index"][:, emask]],
            edge_attr=inp["edge_attr"][emask],
            pattern_num_nodes=inp["pattern_num_nodes"][nidx],
            pattern_probs=inp["pattern_probs"][nidx],
            entry_id=inp["entry_id"][rank * 2: rank * 2 + 2],
            batch=inp["batch"][nidx] - rank * 2,
        )
        opt.zero_grad()
        engine.reset()
        gp, _ = model(**local, num_graphs=2)
        loss = F.quantile_loss(y[rank * 2: rank * 2 + 2], gp.flatten(), 0.5)
        loss.backward()
        engine.finalize()
        opt.step()
        losses.append(float(loss.detach()))
    params = opt.flat_param.numpy().copy()
    result_queue.put((rank, losses, params))
    comm.barrier()
    comm.finalize()


@pytest.mark.timeout(180)
def test_ddp_training_equals_single_process_big_batch():
    """loss-curve equivalence 2x(bs=b) DDP+syncBN vs
    1x(bs=2b) single process — same parameter trajectory."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_train_equiv, args=(r, world, 29515, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=150) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
    results.sort(key=lambda t: t[0])
    (_, losses0, params0), (_, losses1, params1) = results

    # single-process reference: full batch of 4 graphs per step
    from pertgnn.ops import functional as F
    from pertgnn.train.optim import FusedAdam

    model = _build_model()
    opt = FusedAdam(model.parameters(), lr=1e-2)
    model.train()
    ref_losses = []
    for step in range(4):
        x, cat_X, ei, ea, pnn, probs, entry_id, batch, y = _make_inputs(
            seed=300 + step, n=24, e=50, b=4)
        # drop cross-shard edges exactly like the DDP shard split does
        sel0 = batch < 2
        emask = (sel0[ei[0]] == sel0[ei[1]])
        inp = dict(x=x, cat_X=cat_X, edge_index=ei[:, emask], edge_attr=ea[emask],
                   pattern_num_nodes=pnn, pattern_probs=probs,
                   entry_id=entry_id, batch=batch)
        opt.zero_grad()
        gp, _ = model(**inp, num_graphs=4)
        loss = F.quantile_loss(y, gp.flatten(), 0.5)
        loss.backward()
        opt.step()
        ref_losses.append(float(loss.detach()))

    import numpy as np
    # per-rank losses average to the global loss
    for s in range(4):
        assert abs((losses0[s] + losses1[s]) / 2 - ref_losses[s]) < 1e-4, s
    # both ranks identical params; close to the single-process trajectory
    assert np.array_equal(params0, params1)
    # params: Adam's ~zero-denominator early steps chaotically amplify 1-ulp
    # fp32 ordering differences (see test_optim), so the trajectory check is
    # the per-step losses above (1e-4); params stay in the same neighborhood.
    ref_flat = opt.flat_param.numpy()
    assert np.allclose(params0, ref_flat, atol=2e-2), np.abs(params0 - ref_flat).max()


def _worker_bcast(rank, world_size, port, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    from pertgnn.parallel import Comm

    comm = Comm(backend="gloo")
    torch.manual_seed(1000 + rank)  # DIFFERENT init per rank on purpose
    model = _build_model()
    comm.broadcast_module_(model)
    params = {n: p.detach().numpy().copy() for n, p in model.named_parameters()
              if not isinstance(p, torch.nn.parameter.UninitializedParameter)
              and p.numel() > 0}
    bufs = {n: b.detach().numpy().copy() for n, b in model.named_buffers()
            if torch.is_tensor(b) and b.numel() > 0}
    result_queue.put((rank, params, bufs))
    comm.barrier()
    comm.finalize()


@pytest.mark.timeout(120)
def test_broadcast_module_syncs_divergent_init():
    """Regression: broadcast_module_ must write the REAL parameter storage
    (the conv's fused w4/b4 are exported in state_dict as remapped clones —
    broadcasting those would silently leave ranks desynchronized)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_bcast, args=(r, world, 29516, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(world):
        rank, params, bufs = q.get(timeout=110)
        results[rank] = (params, bufs)
    for p in procs:
        p.join(timeout=110)
        assert p.exitcode == 0
    p0, b0 = results[0]
    p1, b1 = results[1]
    assert set(p0) == set(p1)
    import numpy as np
    for n in p0:
        assert np.array_equal(p0[n], p1[n]), f"param {n} not synced"
    for n in b0:
        assert np.array_equal(b0[n], b1[n]), f"buffer {n} not synced"


def _worker_bench(rank, world_size, port, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    import io
    import sys as _sys
    import contextlib

    # gloo on CPU also where a GPU is present: two ranks cannot share one
    # device under RCCL
    torch.cuda.is_available = lambda: False
    argv = ["bench.py", "--steps", "2", "--warmup", "1", "--batch-size", "6",
            "--n-batches", "1", "--layers", "2", "--hidden", "32"]
    out = io.StringIO()
    old = _sys.argv
    _sys.argv = argv
    try:
        import bench as bench_mod
        with contextlib.redirect_stdout(out):
            bench_mod.main()
    finally:
        _sys.argv = old
    result_queue.put((rank, out.getvalue()))


@pytest.mark.timeout(180)
def test_bench_main_world2_gloo():
    """The driver's scaling run executes bench.py with WORLD_SIZE>1 — run the
    EXACT same main() at world_size=2 over gloo on CPU: vocab-stat sync,
    weight broadcast, flat-grad engine, barriers, max-over-ranks timing and
    the rank-0 JSON contract."""
    import json
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_bench, args=(r, world, 29517, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = {}
    for _ in range(world):
        rank, text = q.get(timeout=170)
        outs[rank] = text
    for p in procs:
        p.join(timeout=170)
        assert p.exitcode == 0
    # rank 0 prints exactly one JSON line; rank 1 prints nothing
    line = outs[0].strip().splitlines()[-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 12
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert outs[1].strip() == ""


def _worker_cli_hipgraph(rank, world_size, port, workdir, result_queue):
    os.environ.update(
        RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank),
        MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
    )
    import contextlib
    import io
    import sys as _sys

    argv = ["--synthetic", "--graph_type", "pert", "--epochs", "2",
            "--num_layers", "1", "--hidden_channels", "16", "--batch_size",
            "32", "--seed", "3", "--hipgraph", "--sync_bn",
            "--processed_dir", os.path.join(workdir, "processed")]
    out = io.StringIO()
    # gloo on CPU also where a GPU is present (see _worker_bench)
    torch.cuda.is_available = lambda: False
    import pert_gnn

    with contextlib.redirect_stdout(out):
        pert_gnn.main(argv)
    result_queue.put((rank, out.getvalue()))


@pytest.mark.timeout(300)
def test_cli_hipgraph_world2_gloo(tmp_path):
    """pert_gnn.py --hipgraph under DDP (2 gloo ranks): resident-batch
    sharding, GraphStepper's cross-rank metric reduction and the sync-BN
    interaction — the schedule an 8-GPU --hipgraph run uses, minus RCCL."""
    # pre-generate the dataset in the parent: two ranks would otherwise
    # race to write the same processed/ dir
    from pertgnn.data.ingest import run_ingest
    from pertgnn.data.synthetic import SyntheticConfig, write_dataset

    write_dataset(str(tmp_path), SyntheticConfig())
    run_ingest(data_root=str(tmp_path / "data"),
               processed_dir=str(tmp_path / "processed"), verbose=False)

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_cli_hipgraph,
                         args=(r, world, 29519, str(tmp_path), q))
             for r in range(world)]
    for p in procs:
        p.start()
    outs = {}
    for _ in range(world):
        rank, text = q.get(timeout=280)
        outs[rank] = text
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    lines = [l for l in outs[0].splitlines() if l.startswith("Epoch:")]
    assert len(lines) == 2, outs[0][-2000:]
    assert any("hipgraph stepping mode: eager" in l
               for l in outs[0].splitlines())  # CPU degrades to eager
