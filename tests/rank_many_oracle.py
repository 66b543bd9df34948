"""float64 restatement of the many-targets served-rank contract (include/srec.h: srec_score_ahead_many; model.rank_items),
shared by tests/test_rank_many_cpu.py, tests/test_rank_many_gpu.py and tests/rank_many_gpu_worker.py.  Built on
rank_served_oracle (served64, kernel_case, variant, variants, median_floor, TOL, MAX_WIDTH):
  ahead[b,j] = N[b,j] + A[b,j];  N counts the eligible rows that are NOT targets of the session (left out by id) and stand ahead
  of (items[b,j], target[b,j]);  A orders the session's targets among themselves by their GIVEN values.
N is known to the round-off of the scores (an interval), A exactly.  Everything is materialised: the yardstick, not the product."""
import torch

from rank_served_oracle import MAX_WIDTH, TOL, ahead_exact, ahead_interval, _floor

NINF = float('-inf')


def target_rows(items, n, id_lo=0):
    """bool [B, n]: local row v is one of the session's targets"""
    it = items.detach().long().cpu() - id_lo
    B = it.shape[0]
    m = torch.zeros(B, n + 1, dtype=torch.bool)
    m.scatter_(1, torch.where((it < 0) | (it >= n) | (items.detach().long().cpu() < 0), torch.full_like(it, n), it), True)
    return m[:, :n]


def among_exact(items, target, floor=None):
    """int64 [B, M]: A by the letter of the contract, one pair at a time (given values: no tolerance)"""
    B, M = items.shape
    it = items.detach().long().cpu().tolist()
    t = target.detach().float().cpu().tolist()                       # (Python floats hold every fp32 value exactly)
    f = _floor(floor, B)[:, 0].float().tolist()
    out = [[0] * M for _ in range(B)]
    for b in range(B):
        for j in range(M):
            if it[b][j] < 0:
                continue
            for i in range(M):
                if i == j or it[b][i] < 0 or it[b][i] == it[b][j] or not (t[b][i] > NINF) or t[b][i] < f[b]:
                    continue
                if t[b][i] > t[b][j] or (t[b][i] == t[b][j] and it[b][i] < it[b][j]):
                    out[b][j] += 1
    return torch.tensor(out, dtype=torch.int64).reshape(B, M)


def ahead_many_exact(s, elig, items, target, floor=None, id_lo=0, among_targets=True):
    """int64 [B, M]: srec_score_ahead_many on scores taken as exact"""
    it = items.detach().long().cpu()
    keep = elig.cpu() & ~target_rows(it, s.shape[1], id_lo)
    cols = [ahead_exact(s, keep, it[:, j], target[:, j], floor, id_lo) for j in range(it.shape[1])]
    n = torch.stack(cols, 1)
    return n + among_exact(it, target, floor) if among_targets else n


def ahead_many_interval(s, elig, items, target, tol=TOL, floor=None, id_lo=0, among_targets=True):
    """([lo, hi] int64 [B, M]): N within +-tol over the non-target rows, A exact from the given values"""
    it = items.detach().long().cpu()
    keep = elig.cpu() & ~target_rows(it, s.shape[1], id_lo)
    los, his = zip(*[ahead_interval(s, keep, it[:, j], target[:, j], tol, floor, id_lo) for j in range(it.shape[1])])
    lo, hi = torch.stack(los, 1), torch.stack(his, 1)
    if among_targets:
        a = among_exact(it, target, floor)
        lo, hi = lo + a, hi + a
    return lo, hi


def assert_many_in_interval(ahead, s, elig, items, target, tol=TOL, floor=None, id_lo=0, among_targets=True, what='',
                            max_width=MAX_WIDTH):
    lo, hi = ahead_many_interval(s, elig, items, target, tol, floor, id_lo, among_targets)
    a = ahead.detach().long().cpu()
    bad = (a < lo) | (a > hi)
    assert not bool(bad.any()), '%s: count outside [lo, hi] at %s: got %s lo %s hi %s' % (
        what, bad.nonzero().tolist()[:8], a[bad].tolist()[:8], lo[bad].tolist()[:8], hi[bad].tolist()[:8])
    if max_width is not None:
        assert int((hi - lo).max()) < max_width, '%s: interval width %d makes the check vacuous' % (what, int((hi - lo).max()))
    return lo, hi


def targets(case, B, V, d, C, M):
    """int64 [B, M]: row b = the first M entries of a random permutation of the catalogue; column 0 is the case's label and
    that id is removed elsewhere in the row.  With kernel_case's labels this plants two -1 in column 0, a label whose bias is
    -inf, and a label listed by its own session in every third row"""
    g = torch.Generator().manual_seed(77 + M + V + d + C)
    items = torch.stack([torch.randperm(V, generator=g)[:M] for _ in range(B)])
    labels = case['labels'].long()
    items[:, 1:] = torch.where(items[:, 1:] == labels[:, None], torch.full_like(items[:, 1:], -1), items[:, 1:])
    items[:, 0] = labels
    return items


def close_targets(items, t64, tol=TOL):
    """bool [B, M]: a live finite slot that has another live target of its session within 2 tol of its value (float64) - where
    the order among the targets is decided by round-off"""
    it = items.detach().long().cpu()
    live = (it >= 0) & (t64 > NINF)
    near = (t64[:, :, None] - t64[:, None, :]).abs() <= 2 * tol
    near &= live[:, :, None] & live[:, None, :] & ~torch.eye(it.shape[1], dtype=torch.bool)[None]
    return near.any(2)


def targets_at_the_floor_ahead(items, t64, floor, tol=TOL):
    """int64 [B, M]: for every slot, the number of OTHER live targets of its session that lie within 2 tol of the session's
    floor (float64) and could stand ahead of the slot (the slot's value <= that target's + 2 tol) - whether such a target
    counts at all is decided by round-off, so a count that includes it is known only up to this number.  No floor: zeros"""
    it = items.detach().long().cpu()
    if floor is None:
        return torch.zeros(it.shape, dtype=torch.int64)
    f = floor.detach().double().cpu().reshape(-1, 1)
    edge = (it >= 0) & (t64 > NINF) & ((t64 - f).abs() <= 2 * tol)                       # [B, i]
    could = edge[:, :, None] & (t64[:, None, :] <= t64[:, :, None] + 2 * tol) & ~torch.eye(it.shape[1], dtype=torch.bool)[None]
    return could.sum(1)


def target_values64(s, elig, items):
    """float64 [B, M]: the targets' served values from materialised scores (-inf: not eligible or an empty slot)"""
    it = items.detach().long().cpu()
    t = torch.where(elig, s, torch.full_like(s, NINF)).gather(1, it.clamp(min=0))
    return torch.where(it >= 0, t, torch.full_like(t, NINF))


__all__ = ['TOL', 'MAX_WIDTH', 'NINF', 'target_rows', 'among_exact', 'ahead_many_exact', 'ahead_many_interval',
           'assert_many_in_interval', 'targets', 'close_targets', 'targets_at_the_floor_ahead', 'target_values64']
