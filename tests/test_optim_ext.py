"""FusedAdam's extended step on the CPU: global-norm clipping, decoupled
weight decay and the learning-rate table (eager path), the table builder,
the decay filter, the unchanged default path, the CLI flags and resume."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from pertgnn.data.collate import BatchLoader
from pertgnn.data.dataset import build_data_list
from pertgnn.models import SAGEDeterministic
from pertgnn.train import load_checkpoint, save_checkpoint, train_epoch
from pertgnn.train import optim as optim_mod
from pertgnn.train.optim import FusedAdam, decay_params_of, make_lr_table

ROOT = Path(__file__).resolve().parents[1]


def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(),
                               torch.nn.Linear(16, 4))


def test_eager_matches_adamw_clip_and_lambda_lr():
    """6 steps against torch.optim.AdamW + clip_grad_norm_ + LambdaLR; the
    default decay filter (dim >= 2) is reproduced with two param groups."""
    base, wd, max_norm, steps = 1e-2, 0.1, 0.05, 6
    table = make_lr_table(base, steps, "cosine", warmup_steps=2, min_lr=1e-4)
    a, b = _mlp(0), _mlp(0)
    ours = FusedAdam(a.parameters(), lr=base, weight_decay=wd,
                     max_grad_norm=max_norm, lr_schedule=table)
    theirs = torch.optim.AdamW(
        [{"params": [p for p in b.parameters() if p.dim() >= 2],
          "weight_decay": wd},
         {"params": [p for p in b.parameters() if p.dim() < 2],
          "weight_decay": 0.0}], lr=base)
    sched = torch.optim.lr_scheduler.LambdaLR(
        theirs, lambda k: float(table[min(k, steps - 1)].double()) / base)
    x = torch.randn(32, 8, generator=torch.Generator().manual_seed(1))
    clipped = 0
    for k in range(steps):
        ours.zero_grad()
        a(x).pow(2).mean().backward()
        ours.step()
        theirs.zero_grad()
        b(x).pow(2).mean().backward()
        norm = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
        clipped += int(float(norm) > max_norm)
        theirs.step()
        sched.step()
        assert float(ours.hstate[0]) == float(table[k])
        assert float(ours.hstate[2]) == pytest.approx(float(norm), rel=1e-6)
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.allclose(pa, pb, rtol=0.0, atol=1e-6), k
    assert clipped > 0, "the case must clip"
    stats = ours.grad_stats()
    assert stats["steps"] == steps
    assert stats["clipped_frac"] == clipped / steps
    assert stats["lr"] == float(table[-1])
    assert ours.grad_stats()["steps"] == 0  # the first read reset them


def test_eager_static_scale_is_undone_before_the_norm():
    a, b = _mlp(2), _mlp(2)
    one = FusedAdam(a.parameters(), lr=1e-2, max_grad_norm=0.05)
    scaled = FusedAdam(b.parameters(), lr=1e-2, max_grad_norm=0.05,
                       grad_scale=1024.0)
    x = torch.randn(32, 8, generator=torch.Generator().manual_seed(3))
    for opt, net in ((one, a), (scaled, b)):
        opt.zero_grad()
        opt.scale_loss(net(x).pow(2).mean()).backward()
        opt.step()
    assert float(one.hstate[2]) == pytest.approx(float(scaled.hstate[2]),
                                                 rel=1e-6)
    assert torch.allclose(one.flat_param, scaled.flat_param, atol=1e-6)


@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_make_lr_table(kind):
    base, T, W, low = 3e-3, 40, 7, 1e-5
    t = make_lr_table(base, T, kind, warmup_steps=W, min_lr=low)
    assert t.dtype == torch.float32 and t.shape == (T,)
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).float())
    assert float(t[W - 1]) == f32(base)
    for k in range(1, W + 1):                  # linear up to W
        assert float(t[k - 1]) == f32(base * k / W)
    after = t[W - 1:].double()
    assert bool((after[1:] <= after[:-1]).all())   # non-increasing after W
    if kind == "constant":
        assert bool((t[W - 1:] == t[W - 1]).all())
    else:
        assert float(t[T - 1]) == f32(low)
        assert float(t[W]) < float(t[W - 1])
    if kind == "linear":
        assert float(t[W + 10]) == f32(base + (low - base) * 11 / (T - W))
    if kind == "cosine":
        s = 11 / (T - W)
        assert float(t[W + 10]) == f32(
            low + (base - low) * 0.5 * (1 + math.cos(math.pi * s)))


def test_make_lr_table_edges():
    assert make_lr_table(1e-3, 5, "cosine").shape == (5,)       # no warm-up
    assert float(make_lr_table(1e-3, 1, "linear")[0]) == float(
        torch.tensor(0.0))                                       # s = 1 at T
    flat = make_lr_table(1e-3, 3, "constant", warmup_steps=3)
    assert float(flat[2]) == float(torch.tensor(1e-3))
    with pytest.raises(ValueError):
        make_lr_table(1e-3, 5, "step")
    with pytest.raises(ValueError):
        make_lr_table(1e-3, 5, "linear", warmup_steps=6)


def test_decay_params_of_model():
    model = SAGEDeterministic(9, [64], 8, 50, 8, hidden_channels=16,
                              num_layers=2, dropout=0.0)
    keep = decay_params_of(model)
    named = {n: p for n, p in model.named_parameters() if not isinstance(
        p, torch.nn.parameter.UninitializedParameter)}
    chosen = {n for n, p in named.items() if keep(p)}
    for n, p in named.items():
        if n.endswith("bias") or n.endswith("b4") or p.dim() < 2:
            assert n not in chosen, n
    for mod_name, mod in model.named_modules():
        if isinstance(mod, (torch.nn.Embedding, torch.nn.BatchNorm1d)):
            for pn, _ in mod.named_parameters(recurse=False):
                assert f"{mod_name}.{pn}" not in chosen
    tables = [n for n in named if "embed" in n]
    assert len(tables) >= 4 and not chosen & set(tables)
    for i in range(2):
        for w in ("w4", "we_ifc", "we_rpc"):
            assert f"convs.{i}.{w}" in chosen
    for head in ("local_linear", "global_linear1", "global_linear2"):
        assert f"{head}.weight" in chosen
    # and the mask FusedAdam builds from it covers exactly those elements
    opt = FusedAdam(model.parameters(), weight_decay=0.01, decay_filter=keep)
    want = sum(named[n].numel() for n in chosen)
    assert int(opt.decay_mask.sum()) == want
    assert opt.decay_mask.dtype == torch.uint8
    assert opt.decay_mask.numel() == opt.flat_param.numel()


def test_default_flags_stay_on_the_plain_step(monkeypatch):
    net = _mlp(4)
    opt = FusedAdam(net.parameters(), lr=1e-2)
    assert not opt.extended and opt.slab is None
    assert opt.decay_mask is None and opt.lr_table is None

    def boom(*a, **k):
        raise AssertionError("the extended step ran with every feature off")

    monkeypatch.setattr(FusedAdam, "_eager_step_ex", boom)
    x = torch.randn(4, 8)
    net(x).pow(2).mean().backward()
    opt.step()
    today = {"step", "dev_state", "exp_avg", "exp_avg_sq", "lr", "betas", "eps"}
    assert today <= set(opt.state_dict())
    assert {"weight_decay", "max_grad_norm", "hstate"} <= set(opt.state_dict())
    # each feature alone switches the extended step on
    for kw in ({"weight_decay": 0.1}, {"max_grad_norm": 1.0},
               {"lr_schedule": [1e-3, 5e-4]}):
        assert FusedAdam(_mlp(4).parameters(), **kw).extended, kw


class _FakeExt:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append(name)


@pytest.mark.parametrize("dynamic", [False, True])
def test_default_flags_never_call_adam_step_ex(monkeypatch, dynamic):
    """The GPU branch of step() through a stand-in extension: the plain
    bindings with every feature off, adam_step_ex with one on."""

    class _OnGpu:
        is_cuda = True

    fake = _FakeExt()
    monkeypatch.setattr(optim_mod, "ext", lambda: fake)
    monkeypatch.setattr(optim_mod, "has_hip", lambda: True)
    for kw, want in (({}, "adam_step_dynamic" if dynamic else "adam_step"),
                     ({"max_grad_norm": 1.0}, "adam_step_ex")):
        opt = FusedAdam(_mlp(5).parameters(), dynamic_scale=dynamic, **kw)
        opt.flat_param = _OnGpu()
        fake.calls.clear()
        opt.step()
        assert fake.calls == [want]


def test_state_dict_round_trip_keeps_constructor_hyperparameters():
    net = _mlp(6)
    opt = FusedAdam(net.parameters(), lr=1e-2, weight_decay=0.1,
                    max_grad_norm=0.05, lr_schedule=[1e-2, 5e-3, 1e-3])
    x = torch.randn(4, 8)
    for _ in range(2):
        opt.zero_grad()
        net(x).pow(2).mean().backward()
        opt.step()
    sd = opt.state_dict()
    assert sd["weight_decay"] == 0.1 and sd["max_grad_norm"] == 0.05
    other = FusedAdam(_mlp(6).parameters(), lr=1e-2, weight_decay=0.0,
                      max_grad_norm=None, lr_schedule=[1e-2, 5e-3, 1e-3])
    other.load_state_dict(sd)
    assert torch.equal(other.hstate, opt.hstate)
    assert other.weight_decay == 0.0 and other.max_grad_norm is None
    assert other.step_count == 2
    # a checkpoint from before the field existed still loads
    del sd["hstate"]
    other.load_state_dict(sd)


def _run_cli_cpu(argv):
    # the CLI's main() in a fresh interpreter that reports no device
    cmd = [sys.executable, "-c",
           "import sys, torch; torch.cuda.is_available = lambda: False; "
           "import pert_gnn; pert_gnn.main(sys.argv[1:])", *argv]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                          cwd=str(ROOT))


NEW_KEYS = {"lr", "grad_norm_mean", "grad_norm_max", "clipped_frac"}


def test_cli_flags_on_and_off(tmp_path):
    common = ["--synthetic", "--graph_type", "pert", "--epochs", "2",
              "--num_layers", "1", "--hidden_channels", "16",
              "--batch_size", "32", "--seed", "3",
              "--processed_dir", str(tmp_path / "processed")]
    on, off = tmp_path / "on.jsonl", tmp_path / "off.jsonl"
    r = _run_cli_cpu(common + [
        "--weight_decay", "0.01", "--clip_grad_norm", "1.0", "--lr_schedule",
        "cosine", "--warmup_steps", "2", "--metrics_jsonl", str(on)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    extra = [i for i, l in enumerate(lines) if l.startswith("  lr=")]
    assert len(extra) == 2, r.stdout[-2000:]
    for i in extra:
        assert lines[i - 1].startswith("Epoch:")
        assert ", grad norm mean=" in lines[i] and ", max=" in lines[i]
        assert lines[i].endswith("%") and ", clipped=" in lines[i]
    recs = [json.loads(l) for l in on.read_text().splitlines()]
    assert len(recs) == 2 and all(NEW_KEYS <= set(r_) for r_ in recs)
    assert recs[0]["lr"] > recs[1]["lr"] >= 0.0       # cosine, past warm-up
    assert recs[1]["lr"] == 0.0                       # the last entry: min_lr
    assert all(r_["grad_norm_max"] >= r_["grad_norm_mean"] > 0 for r_ in recs)

    r = _run_cli_cpu(common + ["--metrics_jsonl", str(off)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("  lr=")]
    first = r.stdout.splitlines()[0]
    assert first.startswith("Namespace(")
    for flag in ("weight_decay", "clip_grad_norm", "lr_schedule",
                 "warmup_steps", "min_lr", "optim_ext"):
        assert flag not in first
    recs = [json.loads(l) for l in off.read_text().splitlines()]
    assert len(recs) == 2 and not any(NEW_KEYS & set(r_) for r_ in recs)


def test_resume_walks_the_same_schedule(synthetic_workspace, tmp_path):
    """2 epochs straight through against 1 epoch, checkpoint, resume into a
    fresh model and optimizer, 1 more epoch: the same rate per epoch and, as
    test_pipeline's resume test requires, the same bits in the parameters."""
    _, (tr2data, e2r, _, runtime2pert, resource_df) = synthetic_workspace
    data = build_data_list(tr2data, e2r, runtime2pert, resource_df, limit=30)
    loader = BatchLoader(data, batch_size=8, shuffle=False)
    table = make_lr_table(3e-3, 2 * len(loader), "cosine", warmup_steps=2)

    def make():
        torch.manual_seed(0)
        model = SAGEDeterministic(9, [64], 8, 50, 8, hidden_channels=16,
                                  num_layers=1, dropout=0.0)
        opt = FusedAdam(model.parameters(), lr=3e-3, weight_decay=0.01,
                        decay_filter=decay_params_of(model),
                        max_grad_norm=1.0, lr_schedule=table)
        return model, opt

    def epoch(model, opt):
        out = {}
        train_epoch(model, loader, opt, 0.5, None, stats_out=out)
        return out["grad_stats"]

    model, opt = make()
    straight = [epoch(model, opt), epoch(model, opt)]
    assert straight[0]["steps"] == straight[1]["steps"] == len(loader)
    assert straight[0]["lr"] == float(table[len(loader) - 1])
    assert straight[1]["lr"] == float(table[-1])

    model1, opt1 = make()
    first = epoch(model1, opt1)
    ck = str(tmp_path / "ck.pt")
    save_checkpoint(ck, model1, opt1, epoch=1)
    model2, opt2 = make()
    assert load_checkpoint(ck, model2, opt2)[0] == 1
    second = epoch(model2, opt2)
    assert [first["lr"], second["lr"]] == [s["lr"] for s in straight]
    assert second["steps"] == len(loader)
    for (n, p), q in zip(model.named_parameters(), model2.parameters()):
        if isinstance(p, torch.nn.parameter.UninitializedParameter):
            continue
        assert torch.equal(p.detach(), q.detach()), n
    assert torch.equal(opt.exp_avg, opt2.exp_avg)
