"""float64 restatement of the per-item bias contract (include/srec.h: the bias of srec_served in srec_score_select and srec_score_items),
shared by tests/test_item_bias_cpu.py, tests/test_item_bias_gpu.py and tests/item_bias_gpu_worker.py.  It builds on
select_oracle and items_oracle: the biased score is scores64(...) + bias[group], and bias == -inf goes to select64 / items64
as `drop`.  Everything is materialised: this is the yardstick, not the product."""
import torch

from items_oracle import items64
from select_oracle import scores64, select64  # noqa: F401  (re-exported: the score half of the contract)

NINF = float('-inf')


def bias_rows(bias, group, B, id_lo=0, n=None):
    """float64 [B, n]: the bias of every (session, table row) - bias [V] or [G, V] over global ids, group [B] row ids (None:
    row 0), columns [id_lo, id_lo + n) of it (default: all)"""
    b = bias.detach().double().cpu()
    if b.dim() == 1:
        b = b[None, :]
    g = torch.zeros(B, dtype=torch.long) if group is None else group.detach().long().cpu().reshape(B)
    n = b.shape[1] - id_lo if n is None else n
    return b[g][:, id_lo:id_lo + n]


def _with_drop(rows, drop):
    off = rows == NINF
    return off if drop is None else off | drop.cpu()


def select_biased64(s64, k, bias, group=None, drop=None, id_lo=0):
    """select64 of the biased scores s64 [B, n] + bias[group]: an item whose bias is -inf is ineligible (never returned, also
    when fewer than k are eligible), order and values are those of the sum"""
    rows = bias_rows(bias, group, s64.shape[0], id_lo, s64.shape[1])
    return select64(s64.double().cpu() + rows, k, _with_drop(rows, drop), id_lo)


def items_biased64(s64, items, bias, group=None, id_lo=0, drop=None):
    """items64 of the biased scores: the owner adds the bias, -inf stays -inf; padding -inf, foreign ids 0 (no bias)"""
    rows = bias_rows(bias, group, s64.shape[0], id_lo, s64.shape[1])
    return items64(s64.double().cpu() + rows, items, id_lo, _with_drop(rows, drop))


def exact_bias(V, G=None, seed=0, off_share=0.3, off_ranges=((128, 256),)):
    """fp32 [V] (G None) or [G, V]: multiples of 1/8 in [-2, 2] - every sum with the scores of select_oracle.exact_case stays
    representable - about off_share of the entries -inf, and -inf on the whole of every row range of off_ranges"""
    g = torch.Generator().manual_seed(1000 + V + 7 * (G or 0) + seed)
    shape = (V,) if G is None else (G, V)
    b = torch.randint(-16, 17, shape, generator=g).float() / 8
    b[torch.rand(shape, generator=g) < off_share] = NINF
    for lo, hi in off_ranges:
        b[..., lo:min(hi, V)] = NINF
    return b
