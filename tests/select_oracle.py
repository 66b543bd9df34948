"""float64 restatement of the selection contract of csrc/recommend.hip (include/srec.h: srec_score_select), shared by
tests/test_select_cpu.py, tests/test_select_gpu.py and tests/select_gpu_worker.py.  Scores come from
rank_oracle.scores64; everything is materialised: this is the yardstick, not the product."""
import torch

from rank_oracle import scores64  # noqa: F401  (re-exported: the score half of the contract)


def drop_mask(listed, n, id_lo=0):
    """bool [B, n]: row v of the table (global id id_lo + v) is among listed[b, :] (global ids, -1 = empty slot)"""
    lst = listed.detach().long().cpu()
    loc = lst - id_lo
    loc = torch.where((lst >= 0) & (loc >= 0) & (loc < n), loc, torch.full_like(loc, n))
    return torch.zeros(lst.shape[0], n + 1, dtype=torch.bool).scatter_(1, loc, True)[:, :n]


def select64(s, k, drop=None, id_lo=0):
    """(values float64 [B, k], ids int64 [B, k]): the k best eligible columns of s [B, n] by (value descending, id
    ascending); ids are id_lo + column; a session with fewer than k eligible columns ends in (-inf, -1) slots"""
    s = s.double().cpu()
    B, n = s.shape
    elig = torch.ones(B, n, dtype=torch.bool) if drop is None else ~drop.cpu()
    o = torch.argsort(s, dim=1, descending=True, stable=True)              # equal values keep the lower column first
    o = o.gather(1, torch.argsort(elig.gather(1, o).int(), dim=1, descending=True, stable=True))   # eligible ones first
    o = o[:, :k]
    val, ok = s.gather(1, o), elig.gather(1, o)
    val = torch.where(ok, val, torch.full_like(val, float('-inf')))
    idx = torch.where(ok, o + id_lo, torch.full_like(o, -1))
    if n < k:
        val = torch.cat([val, val.new_full((B, k - n), float('-inf'))], 1)
        idx = torch.cat([idx, idx.new_full((B, k - n), -1)], 1)
    return val, idx


def merge_lists(vals, idxs, k):
    """the k best of several (values [B, *], ids [B, *]) lists by (value descending, id ascending), unfilled slots (id -1) last"""
    val, idx = torch.cat([v.double().cpu() for v in vals], 1), torch.cat([i.long().cpu() for i in idxs], 1)
    key = torch.where(idx < 0, torch.full_like(idx, 2 ** 62), idx)
    o = torch.argsort(key, dim=1, stable=True)
    val, idx = val.gather(1, o), idx.gather(1, o)
    o = torch.argsort(val, dim=1, descending=True, stable=True)[:, :k]
    return val.gather(1, o), idx.gather(1, o)


def exact_case(B, V, d):
    """inputs whose every product and sum is representable in fp32: entries are multiples of 1/8 in [-1, 1], column scales in
    {0.5, 1, 2}, and some table rows are duplicated (equal scores: the tie rule decides)"""
    g = torch.Generator().manual_seed(B * 7 + V)
    sr = torch.randint(-8, 9, (B, d), generator=g).float() / 8
    E = torch.randint(-8, 9, (V, d), generator=g).float() / 8
    cs = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (V,), generator=g)]
    for a, b in [(3, 17)] + ([(100, 101)] if V > 101 else []):
        E[b], cs[b] = E[a], cs[a]
    return sr, E, cs


def window_count(s64, k, tol, drop=None):
    """int64 [B]: eligible columns whose score lies within 2 tol of the session's k-th best eligible score (that one
    included) - how many columns round-off may move across the end of the list"""
    s = s64.double().cpu().clone()
    if drop is not None:
        s[drop.cpu()] = float('-inf')
    kth = s.topk(k, dim=1).values[:, k - 1:k]
    return ((s - kth).abs() <= 2 * tol).sum(1)


def assert_list_consistent(val, idx, s64, tol, drop=None, what=''):
    """what every returned list must satisfy against scores known to +-tol, per session: ids distinct, in range and not
    dropped; |value - s64[id]| < tol; values non-increasing and equal values in ascending id order; every eligible column
    with s64 > min(s64 over the returned ids) + 2 tol is in the list"""
    val, idx, s64 = val.detach().double().cpu(), idx.detach().long().cpu(), s64.double().cpu()
    B, n = s64.shape
    assert val.shape == idx.shape and val.shape[0] == B, (what, val.shape, idx.shape, s64.shape)
    for b in range(B):
        ids, v = idx[b], val[b]
        assert int(ids.min()) >= 0 and int(ids.max()) < n, (what, b, ids.tolist())
        assert ids.unique().numel() == ids.numel(), (what, b, 'repeated ids', ids.tolist())
        if drop is not None:
            assert not bool(drop[b, ids].any()), (what, b, 'dropped id returned', ids[drop[b, ids]].tolist())
        err = float((v - s64[b, ids]).abs().max())
        assert err < tol, (what, b, 'value off by', err)
        assert bool((v[1:] <= v[:-1]).all()), (what, b, 'values rise', v.tolist())
        tie = v[1:] == v[:-1]
        assert bool((ids[1:][tie] > ids[:-1][tie]).all()), (what, b, 'tie order', ids.tolist())
        must = s64[b] > float(s64[b, ids].min()) + 2 * tol
        if drop is not None:
            must &= ~drop[b]
        must[ids] = False
        assert not bool(must.any()), (what, b, 'missing', must.nonzero().flatten().tolist()[:8])
