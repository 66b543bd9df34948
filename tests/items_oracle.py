"""float64 restatement of the per-slot contract of csrc/score_items.hip (include/srec.h: srec_score_items), shared by
tests/test_items_cpu.py, tests/test_items_gpu.py and tests/items_gpu_worker.py.  Scores come from rank_oracle.scores64;
everything is materialised: this is the yardstick, not the product."""
import torch

from rank_oracle import scores64  # noqa: F401  (re-exported: the score half of the contract)
from select_oracle import drop_mask, exact_case  # noqa: F401  (the same dropped sets, the same exact inputs)


def items64(s64, items, id_lo=0, drop=None):
    """float64 [B, M]: the columns of s64 [B, n] (column v = global id id_lo + v) at the global ids items [B, M] or [M]
    (shared by all sessions): -inf for an id of -1, 0 for an id outside [id_lo, id_lo + n) (another shard's), -inf where
    drop [B, n] (bool, by column) is set"""
    s = s64.double().cpu()
    B, n = s.shape
    it = items.detach().long().cpu()
    if it.dim() == 1:
        it = it[None, :].expand(B, -1)
    loc = it - id_lo
    own = (it >= 0) & (loc >= 0) & (loc < n)
    safe = torch.where(own, loc, torch.zeros_like(loc))
    out = torch.where(own, s.gather(1, safe), torch.zeros(B, it.shape[1], dtype=torch.float64))
    if drop is not None:
        out = torch.where(own & drop.cpu().gather(1, safe), torch.full_like(out, float('-inf')), out)
    return torch.where(it < 0, torch.full_like(out, float('-inf')), out)


def order64(val, items, k=None):
    """(values float64 [B, n], ids int64 [B, n]) of model.rerank's contract: the slots of val [B, M] at ids items ([B, M]
    or [M]) by (value descending, id ascending); -inf slots last with id -1; cut to k when given.  Python sort per session."""
    val = val.detach().double().cpu()
    it = items.detach().long().cpu()
    if it.dim() == 1:
        it = it[None, :].expand(val.shape[0], -1)
    out_v, out_i = [], []
    for vs, ids in zip(val.tolist(), it.tolist()):
        pairs = sorted(((v, i) for v, i in zip(vs, ids) if v != float('-inf')), key=lambda p: (-p[0], p[1]))
        pairs += [(float('-inf'), -1)] * (len(vs) - len(pairs))
        pairs = pairs if k is None else pairs[:k]
        out_v.append([p[0] for p in pairs])
        out_i.append([p[1] for p in pairs])
    return torch.tensor(out_v, dtype=torch.float64).reshape(len(out_v), -1), torch.tensor(out_i, dtype=torch.int64).reshape(len(out_i), -1)
