"""`from src.utils.train import TrainRunner` (reference: src/utils/train.py) -> sessionrec-pytorch_amd.train"""
import src.models  # noqa: F401  (puts the repo root on sys.path)
from importlib import import_module as _im

_m = _im('sessionrec-pytorch_amd.train')
TrainRunner, evaluate, fix_weight_decay, prepare_batch = _m.TrainRunner, _m.evaluate, _m.fix_weight_decay, _m.prepare_batch
metrics_from_ranks = _m.metrics_from_ranks
evaluate_served, metrics_from_served_ranks = _m.evaluate_served, _m.metrics_from_served_ranks
evaluate_rest, item_ranks_from_scores, metrics_from_item_ranks = _m.evaluate_rest, _m.item_ranks_from_scores, _m.metrics_from_item_ranks
