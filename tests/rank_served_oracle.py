"""float64 restatement of the served-rank contract (include/srec.h: srec_score_ahead; model.served_rank), shared by
tests/test_rank_served_cpu.py, tests/test_rank_served_gpu.py and tests/rank_served_gpu_worker.py.  Built on rank_oracle
(scores64, ranks_exact, rank_interval): the biased score is scores64(...) + bias[group]; a row that is dropped, whose bias is
-inf or that lies below the floor is taken out of the count by giving it NaN, which is ahead of nothing.  Everything is
materialised: this is the yardstick, not the product.  The kernel cases of the GPU file live here too, so that the CPU file can
check at the very same shapes that the interval test is not vacuous."""
import torch

from item_bias_oracle import NINF, bias_rows
from rank_oracle import rank_interval, ranks_exact, scores64
from select_oracle import drop_mask

TOL = 1e-4                   # the project's fp32 round-off bound at these magnitudes (tests/test_rank_gpu.py)
MAX_WIDTH = 16               # ... and its cap on the interval width


def served64(srs, table, cs=None, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None):
    """(s' float64 [B, n], eligible bool [B, n]) of the rows of `table` (global ids id_lo ...): the biased served score and the
    eligibility rule - not listed under drop_listed, bias > -inf.  bias: [V] or [G, V] over GLOBAL ids"""
    n = table.shape[0]
    if drop_listed:
        s = scores64(srs, table, cs, off_ex, None, None, id_lo)
        elig = ~drop_mask(listed, n, id_lo) if listed is not None else torch.ones_like(s, dtype=torch.bool)
    else:
        s = scores64(srs, table, cs, off_ex, off_in, listed, id_lo)
        elig = torch.ones_like(s, dtype=torch.bool)
    if bias is not None:
        rows = bias_rows(bias, group, s.shape[0], id_lo, n)
        s = s + rows
        elig = elig & (rows != NINF)
    return s, elig


def _floor(floor, B):
    return torch.full((B, 1), NINF, dtype=torch.float64) if floor is None else floor.detach().double().cpu().reshape(B, 1)


def ahead_exact(s, elig, labels, target, floor=None, id_lo=0):
    """int64 [B]: srec_score_ahead on scores taken as exact - ranks_exact over the rows that are eligible and not below the
    floor (the others are NaN: ahead of nothing); a label < 0 counts nothing"""
    s = s.double().cpu()
    keep = elig.cpu() & ~(s < _floor(floor, s.shape[0]))
    r = ranks_exact(torch.where(keep, s, torch.full_like(s, float('nan'))), labels, target, id_lo)
    return r.clamp(min=0)


def ahead_interval(s, elig, labels, target, tol, floor=None, id_lo=0):
    """[lo, hi] every count consistent with scores known to +-tol (target and floor are the call's own inputs, known exactly)
    must fall in: lo counts the rows that are surely ahead and surely not below the floor, hi those that may be"""
    s = s.double().cpu()
    B, n = s.shape
    lab = labels.detach().long().cpu()
    t = target.detach().double().cpu().reshape(B, 1)
    f = _floor(floor, B)
    other = elig.cpu() & ((torch.arange(n)[None, :] + id_lo) != lab[:, None]) & (lab >= 0)[:, None]
    lo = (other & (s > t + tol) & (s >= f + tol)).sum(1)
    hi = (other & (s >= t - tol) & (s >= f - tol)).sum(1)
    return lo, hi


def assert_ahead_in_interval(ahead, s, elig, labels, target, tol=TOL, floor=None, id_lo=0, what='', max_width=MAX_WIDTH):
    lo, hi = ahead_interval(s, elig, labels, target, tol, floor, id_lo)
    a = ahead.detach().long().cpu()
    bad = (a < lo) | (a > hi)
    assert not bool(bad.any()), '%s: count outside [lo, hi] for sessions %s: got %s lo %s hi %s' % (
        what, bad.nonzero().flatten().tolist()[:8], a[bad].tolist()[:8], lo[bad].tolist()[:8], hi[bad].tolist()[:8])
    if max_width is not None:
        assert int((hi - lo).max()) < max_width, '%s: interval width %d makes the check vacuous' % (what, int((hi - lo).max()))
    return lo, hi


def served_ranks64(s, elig, labels, floor=None):
    """model.served_rank from materialised scores taken as exact: -1 without a label, -2 where the label is not eligible,
    scores -inf or lies below the floor, else ahead_exact with the label's own score as the target"""
    s = s.double().cpu()
    lab = labels.detach().long().cpu()
    safe = lab.clamp(min=0)[:, None]
    t = s.gather(1, safe)[:, 0]
    shown = elig.cpu().gather(1, safe)[:, 0] & (t > NINF) & ~(t < _floor(floor, s.shape[0])[:, 0])
    r = torch.where(shown, ahead_exact(s, elig, lab, t, floor), torch.full_like(lab, -2))
    return torch.where(lab >= 0, r, torch.full_like(lab, -1))


# ------------------------------------------------------------------------------------------- the kernel cases of the GPU file
# (B, V, d, C): two session tiles with a partial one; a partial last chunk (V 300) and several ranges (V 5000); d a multiple
# of the 32-column group and not; one and three components; C 4 x d 320 does not fit LDS (4 * 32 * 324 * 4 B > 160 KB): the
# instances that read the session tiles through the cache
SHAPES = [(33, 300, 32, 1), (33, 300, 36, 3), (33, 5000, 36, 1), (33, 5000, 32, 3), (33, 300, 320, 4)]
LISTS = ('none', 'score', 'drop')
BIASES = ('none', 'vec', 'grouped')
LIST_L, GROUPS = 5, 3


def kernel_case(B, V, d, C):
    """random operands of one shape, every optional one present (a variant leaves some out): session vectors, table, column
    scale, offsets, a list of LIST_L ids per session (empty slots; every third session's list holds its label), a [V] bias
    with -inf entries (one on a label) and a [GROUPS, V] bias with group ids, labels with two -1"""
    g = torch.Generator().manual_seed(1000 * C + V + d)
    srs = torch.randn(C, B, d, generator=g) * 0.3
    E = torch.randn(V, d, generator=g) * 0.2
    cs = torch.rand(V, generator=g) + 0.5
    labels = torch.randint(0, V, (B,), generator=g)
    off_ex = -2.0 * torch.rand(C, B, generator=g)
    off_in = off_ex + torch.rand(C, B, generator=g) * 3 - 1.0
    listed = torch.stack([torch.randperm(V, generator=g)[:LIST_L] for _ in range(B)])
    listed[torch.rand(B, LIST_L, generator=g) < 0.25] = -1
    third = torch.arange(B) % 3 == 0
    for j in range(LIST_L):
        if j != 2:
            listed[:, j] = torch.where(listed[:, j] == labels, torch.full_like(labels, -1), listed[:, j])
    listed[third, 2] = labels[third]
    bias_vec = torch.randn(V, generator=g) * 0.5
    bias_vec[torch.rand(V, generator=g) < 0.2] = NINF
    bias_vec[labels[1]] = NINF
    bias_grp = torch.randn(GROUPS, V, generator=g) * 0.5
    bias_grp[torch.rand(GROUPS, V, generator=g) < 0.2] = NINF
    group = torch.arange(B) % GROUPS
    labels[5], labels[B - 1] = -1, -1
    return dict(srs=srs, E=E, cs=cs, labels=labels, off_ex=off_ex, off_in=off_in, listed=listed, bias_vec=bias_vec,
                bias_grp=bias_grp, group=group)


def variant(case, lists, bias, with_cs):
    """the operands of one variant as keywords of served64 (and, moved to the device, of ops.score_ahead / score_select)"""
    kw = dict(cs=case['cs'] if with_cs else None, off_ex=case['off_ex'], off_in=None, listed=None, drop_listed=False,
              bias=None, group=None)
    if lists != 'none':
        kw.update(listed=case['listed'], drop_listed=lists == 'drop', off_in=None if lists == 'drop' else case['off_in'])
    if bias == 'vec':
        kw.update(bias=case['bias_vec'])
    elif bias == 'grouped':
        kw.update(bias=case['bias_grp'], group=case['group'])
    return kw


def variants():
    """(lists, bias, floored, with_cs): every list mode with every bias form, each with and without a floor, the column scale
    given and left out in turn"""
    out = []
    for i, lists in enumerate(LISTS):
        for j, bias in enumerate(BIASES):
            for floored in (False, True):
                out.append((lists, bias, floored, (i + j + int(floored)) % 2 == 0))
    return out


def median_floor(s, elig):
    """fp32 [B]: the median eligible score of every session - about half of the labels lie below it"""
    x = torch.where(elig, s, torch.full_like(s, float('nan')))
    return torch.nanmedian(x, dim=1).values.float()


__all__ = ['TOL', 'MAX_WIDTH', 'served64', 'ahead_exact', 'ahead_interval', 'assert_ahead_in_interval', 'served_ranks64',
           'SHAPES', 'kernel_case', 'variant', 'variants', 'median_floor', 'rank_interval']
