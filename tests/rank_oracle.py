"""float64 restatement of the score / rank contract of csrc/rank.hip (include/srec.h: srec_score_rank), shared by
tests/test_rank_cpu.py and tests/test_rank_gpu.py.  Everything is materialised: this is the yardstick, not the product."""
import torch


def scores64(srs, table, cs=None, off_ex=None, off_in=None, listed=None, id_lo=0):
    """(B, n) float64 scores of the rows of `table` (global ids id_lo ...): logsumexp_c(cs[v] <sr_c[b], E_v> + off[c, b]),
    off_in for the items of listed[b, :] (global ids, -1 = empty), off_ex elsewhere; one component: z + off, no exp / log"""
    if isinstance(srs, (list, tuple)):
        srs = torch.stack(list(srs), 0)
    if srs.dim() == 2:
        srs = srs.unsqueeze(0)
    srs, E = srs.detach().double().cpu(), table.detach().double().cpu()
    C, B, _ = srs.shape
    n = E.shape[0]
    z = torch.einsum('cbd,vd->cbv', srs, E)
    if cs is not None:
        z = z * cs.detach().double().cpu()[None, None, :]
    zero = torch.zeros(C, B, dtype=torch.float64)
    oe = zero if off_ex is None else off_ex.detach().double().cpu().reshape(C, B)
    oi = zero if off_in is None else off_in.detach().double().cpu().reshape(C, B)
    inside = torch.zeros(B, n + 1, dtype=torch.bool)
    if listed is not None:
        loc = listed.detach().long().cpu() - id_lo
        loc = torch.where((listed.detach().long().cpu() >= 0) & (loc >= 0) & (loc < n), loc, torch.full_like(loc, n))
        inside.scatter_(1, loc, True)
    inside = inside[:, :n]
    z = z + torch.where(inside[None], oi[:, :, None], oe[:, :, None])
    return z[0] if C == 1 else torch.logsumexp(z, dim=0)


def ranks_exact(s, labels, target=None, id_lo=0):
    """number of columns ahead of the label: higher score, or the same score and a lower id; the label's own column never
    counts; label < 0 -> -1.  target: the labels' scores when the label's column may belong to another shard."""
    s = s.double().cpu()
    lab = labels.detach().long().cpu()
    n = s.shape[1]
    ids = torch.arange(n)[None, :] + id_lo
    if target is None:
        target = s.gather(1, (lab - id_lo).clamp(0, n - 1)[:, None])[:, 0]
    t = target.double().cpu()[:, None]
    ahead = ((s > t) | ((s == t) & (ids < lab[:, None]))) & (ids != lab[:, None])
    return torch.where(lab >= 0, ahead.sum(1), torch.full_like(lab, -1))


def rank_interval(s64, labels, tol):
    """[lo, hi] every rank consistent with scores known to +-tol must fall in: lo = #(s > t + tol), hi = #(s >= t - tol) - 1"""
    s64 = s64.double().cpu()
    lab = labels.detach().long().cpu()
    t = s64.gather(1, lab.clamp(min=0)[:, None])
    return (s64 > t + tol).sum(1), (s64 >= t - tol).sum(1) - 1


def assert_in_interval(rank, s64, labels, tol, what='', max_width=None):
    lo, hi = rank_interval(s64, labels, tol)
    r = rank.detach().long().cpu()
    live = labels.detach().long().cpu() >= 0
    bad = live & ((r < lo) | (r > hi))
    assert not bool(bad.any()), '%s: rank outside [lo, hi] for sessions %s: rank %s lo %s hi %s' % (
        what, bad.nonzero().flatten().tolist()[:8], r[bad].tolist()[:8], lo[bad].tolist()[:8], hi[bad].tolist()[:8])
    assert bool((r[~live] == -1).all()), what
    if max_width is not None:
        w = (hi - lo)[live]
        assert int(w.max()) < max_width, '%s: interval width %d makes the check vacuous' % (what, int(w.max()))
    return lo, hi
