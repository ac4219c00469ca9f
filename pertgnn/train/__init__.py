from .checkpoint import load_checkpoint, save_checkpoint
from .loop import QuantileReport, evaluate, train_epoch

__all__ = ["train_epoch", "evaluate", "QuantileReport", "save_checkpoint", "load_checkpoint"]
