"""Checkpoint / resume (reference has none — SURVEY.md §5).

Checkpoint = model state_dict (keyed identically to the reference
SAGEDeterministic, including the dead ``edge_linear`` lazy module, quirk 4)
+ optimizer state + RNG states + epoch counter + the attention head count
+ the quantile levels the model is trained for.
Rank 0 writes; all ranks barrier; every rank loads.

A state_dict has the same keys and shapes at every head count, so loading a
heads=4 checkpoint into a heads=1 model would succeed and silently compute
something else.  The checkpoint therefore records ``heads`` and
``load_checkpoint`` refuses a mismatch; a checkpoint without the field was
written before the field existed and means ``heads=1``.

Likewise nothing in the weights says which quantile level an output column
was trained for, so the checkpoint records ``taus`` (a list; ``[tau]`` for a
one-level run) and loading under other levels is refused.  A checkpoint
without the field means "unknown": no check is done.
"""
from __future__ import annotations

import os

import torch


def model_heads(model) -> int:
    """Attention head count of a model (1 when it has no such notion)."""
    return int(getattr(model, "heads", 1))


def check_heads(state: dict, model, path: str = "checkpoint"):
    """Raise when the head count recorded in ``state`` differs from the
    model's (missing field = 1)."""
    saved = int(state.get("heads", 1))
    have = model_heads(model)
    if saved != have:
        raise ValueError(
            f"{path} was written by a model with heads={saved}, but the "
            f"model to load it into has heads={have}; the weights have the "
            "same shapes at any head count and would load silently — build "
            f"the model with heads={saved}")


def _as_levels(taus):
    """A scalar level or a sequence of levels as a list of floats; None
    stays None (unknown)."""
    if taus is None:
        return None
    if hasattr(taus, "__iter__"):
        return [float(t) for t in taus]
    return [float(taus)]


def check_taus(state: dict, taus, path: str = "checkpoint"):
    """Raise when the quantile levels recorded in ``state`` differ from the
    requested ``taus``.  No check when either side is unknown (None / a
    checkpoint written before the field existed).  Returns the recorded
    levels (or None)."""
    saved = _as_levels(state.get("taus"))
    want = _as_levels(taus)
    if saved is not None and want is not None and saved != want:
        raise ValueError(
            f"{path} was written by a model trained for quantile levels "
            f"taus={saved}, but levels taus={want} are requested; the output "
            "columns would be read as levels they were not trained for — "
            f"run with the levels {saved}")
    return saved


def save_checkpoint(path: str, model, optimizer, epoch: int, comm=None, extra: dict | None = None,
                    taus=None):
    """``taus``: the level(s) the model is trained for (default: the
    model's ``taus`` attribute; None = unknown, not recorded)."""
    if taus is None:
        taus = getattr(model, "taus", None)
    if comm is None or comm.rank == 0:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        state = {
            "model": model.state_dict(),
            "optimizer": optimizer.state_dict() if optimizer is not None else None,
            "epoch": epoch,
            "heads": model_heads(model),
            "taus": _as_levels(taus),
            "rng": {
                "torch": torch.get_rng_state(),
                "cuda": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else None,
            },
            "extra": extra or {},
        }
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)
    if comm is not None:
        comm.barrier()


def load_checkpoint(path: str, model, optimizer=None, map_location="cpu", taus=None):
    """``taus``: the level(s) the caller is about to use; a checkpoint that
    records other levels is refused.  The recorded levels (or, when the
    checkpoint has none, ``taus``) are left on ``model.taus``."""
    state = torch.load(path, map_location=map_location, weights_only=False)
    check_heads(state, model, path)
    saved = check_taus(state, taus, path)
    model.load_state_dict(state["model"])
    levels = saved if saved is not None else _as_levels(taus)
    if levels is not None:
        model.taus = tuple(levels)
    if optimizer is not None and state.get("optimizer") is not None:
        optimizer.load_state_dict(state["optimizer"])
    rng = state.get("rng", {})
    if rng.get("torch") is not None:
        torch.set_rng_state(rng["torch"].cpu() if torch.is_tensor(rng["torch"]) else rng["torch"])
    if rng.get("cuda") is not None and torch.cuda.is_available():
        try:
            torch.cuda.set_rng_state_all([s.cpu() for s in rng["cuda"]])
        except RuntimeError:
            pass  # different device count than at save time
    return state.get("epoch", 0), state.get("extra", {})
