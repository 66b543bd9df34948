"""float64 restatement of the log-normaliser contract of csrc/score_norm.hip (include/srec.h: srec_score_norm), shared by
tests/test_norm_cpu.py, tests/test_norm_gpu.py and tests/norm_gpu_worker.py.  It builds on select_oracle / item_bias_oracle:
Z[b] = logsumexp over the ELIGIBLE columns of scores64(...) + bias_rows(...); a column is ineligible when its bias is -inf
or when `drop` names it.  Everything is materialised: this is the yardstick, not the product."""
import torch

from item_bias_oracle import NINF, bias_rows
from select_oracle import scores64  # noqa: F401  (re-exported: the score half of the contract)


def eligible(B, n, bias=None, group=None, drop=None, id_lo=0):
    """bool [B, n]: columns [id_lo, id_lo + n) of the catalogue that contribute for every session"""
    ok = torch.ones(B, n, dtype=torch.bool)
    if bias is not None:
        ok &= bias_rows(bias, group, B, id_lo, n) != NINF
    if drop is not None:
        ok &= ~drop.cpu()
    return ok


def norm64(s64, bias=None, group=None, drop=None, id_lo=0):
    """float64 [B]: logsumexp over the eligible columns of s64 [B, n] (the scores of rows id_lo ...) + bias[group] (bias [V]
    or [G, V] over GLOBAL ids); drop: bool [B, n], columns that never contribute; -inf for a session without an eligible
    column (never NaN)"""
    s = s64.double().cpu().clone()
    B, n = s.shape
    if bias is not None:
        rows = bias_rows(bias, group, B, id_lo, n)
        s = s + torch.where(rows == NINF, torch.zeros_like(rows), rows)
    s[~eligible(B, n, bias, group, drop, id_lo)] = NINF
    m = s.max(dim=1).values if n > 0 else torch.full((B,), NINF, dtype=torch.float64)
    ms = torch.where(m == NINF, torch.zeros_like(m), m)
    return torch.where(m == NINF, m, ms + torch.log(torch.exp(s - ms[:, None]).sum(1)))


def lse_pair64(a, b):
    """float64 log(exp(a) + exp(b)) elementwise, -inf-safe: how the normalisers of two disjoint row ranges combine"""
    a, b = a.double().cpu(), b.double().cpu()
    m = torch.maximum(a, b)
    ms = torch.where(m == NINF, torch.zeros_like(m), m)
    return torch.where(m == NINF, m, ms + torch.log(torch.exp(a - ms) + torch.exp(b - ms)))
