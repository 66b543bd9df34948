"""float64 oracle of the diversified top-N (csrc/diversify.hip, include/srec.h srec_diversify): the greedy MMR re-rank of a
pool of M slots per session and the intra-list diversity of its picks, in plain torch.

  sim(i, j) = <X_i, X_j> / (max(|X_i|, 1e-12) max(|X_j|, 1e-12))                       (a zero row: 0 to everything)
  for t = 0 .. K-1:  m_t(i) = s[i] - theta * pen_t(i) over the filled slots not yet picked, pen_0 = 0, pen_t(i) = the RAW
  maximum of sim(i, j) over the slots j picked so far; the pick is argmax m_t, ties to the lower slot; theta == 0: m_t = s.
  pick -1 / val -inf / mmr -inf once the filled slots run out; ild = 1 - mean_{a<b} sim(pick_a, pick_b), 0 below two picks.

margin_case(): inputs on which every decision has a margin about a thousand fp32 roundings wide, so a kernel's picks must be
EQUAL to these.  assert_greedy_consistent(): random inputs, each pick judged GIVEN the picks before it."""
import torch

NINF = float('-inf')


def sims64(rows):
    """[B, M, M] float64 cosines of rows [B, M, d] (any dtype), norms clamped at 1e-12"""
    x = rows.double()
    n = x.norm(dim=-1).clamp(min=1e-12)
    return torch.einsum('bid,bjd->bij', x, x) / (n[:, :, None] * n[:, None, :])


def _first_best(m, avail):
    """(slot [B] of the largest m among avail, lower slot on ties; -1: nothing available, best [B], margin [B] to the second
    best available slot - inf with fewer than two)"""
    key = torch.where(avail, m, torch.full_like(m, NINF))
    best = key.max(1).values
    cand = avail & (key == best[:, None])
    p = cand.int().argmax(1)                                     # the first maximal index
    none = ~avail.any(1)
    rest = key.clone()
    rest[torch.arange(m.shape[0]), p] = NINF
    second = rest.max(1).values
    margin = torch.where((avail.sum(1) < 2) | (second == NINF), torch.full_like(best, float('inf')), best - second)
    return torch.where(none, torch.full_like(p, -1), p), best, margin


def _scores(s, pen, theta, t):
    return s.clone() if (theta == 0 or t == 0) else s - theta * pen


def greedy64(rows, s, theta, K, filled=None):
    """dict(pick long [B,K], val [B,K], mmr [B,K], ild [B], margin [B,K]) in float64.  rows [B, M, d], s [B, M];
    filled bool [B, M] (None: every slot).  margin: best minus second best m_t among the slots available at step t."""
    s = s.double()
    B, M = s.shape
    sim = sims64(rows)
    avail = torch.ones(B, M, dtype=torch.bool) if filled is None else filled.clone()
    pen = torch.zeros(B, M, dtype=torch.float64)
    ar = torch.arange(B)
    pick = torch.full((B, K), -1, dtype=torch.long)
    val = torch.full((B, K), NINF, dtype=torch.float64)
    mmr = torch.full((B, K), NINF, dtype=torch.float64)
    margin = torch.full((B, K), float('inf'), dtype=torch.float64)
    for t in range(K):
        p, best, mg = _first_best(_scores(s, pen, theta, t), avail)
        ok = p >= 0
        pc = p.clamp(min=0)
        pick[:, t] = p
        val[:, t] = torch.where(ok, s[ar, pc], val[:, t])
        mmr[:, t] = torch.where(ok, best, mmr[:, t])
        margin[:, t] = torch.where(ok, mg, margin[:, t])
        to = sim[ar, :, pc]
        pen = torch.where(ok[:, None], to if t == 0 else torch.maximum(pen, to), pen)
        avail[ar[ok], p[ok]] = False
    return dict(pick=pick, val=val, mmr=mmr, ild=ild64(rows, pick, sim), margin=margin)


def ild64(rows, pick, sim=None):
    """[B] float64: 1 - the mean cosine over the pairs of filled picks (slot numbers, -1 = none), 0 with fewer than two"""
    sim = sims64(rows) if sim is None else sim
    out = torch.zeros(pick.shape[0], dtype=torch.float64)
    for b in range(pick.shape[0]):
        p = pick[b][pick[b] >= 0].long()
        n = p.numel()
        if n >= 2:
            sub = sim[b][p][:, p]
            out[b] = 1.0 - torch.triu(sub, 1).sum() / (n * (n - 1) / 2)
    return out


DIRECTIONS = 12          # margin_case: distinct unit directions a pool draws from (duplicates are frequent)


def margin_case(B, M, d, seed):
    """(rows fp32 [B, M, d], s fp32 [B, M]) for theta = 1/2: every row is one of DIRECTIONS unit directions with four entries
    of +-1/2 within the first 16 coordinates (every cosine a multiple of 1/4, exact in fp32 in any summation order), and
    s[i] = (16 - i // 8) / 8 - i 2^-10.  Two distinct slots then differ in m_t by a multiple of 1/8 minus (i - j) 2^-10 with
    |i - j| < 128: at least 2^-10 at every step"""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.zeros(B, DIRECTIONS, d)
    for b in range(B):
        for k in range(DIRECTIONS):
            where = torch.randperm(16, generator=g)[:4]
            dirs[b, k, where] = (torch.randint(0, 2, (4,), generator=g).float() - 0.5)
    which = torch.randint(0, DIRECTIONS, (B, M), generator=g)
    rows = dirs[torch.arange(B)[:, None], which]
    i = torch.arange(M)
    s = ((16 - i // 8).float() / 8 - i.float() * 2.0 ** -10)[None, :].expand(B, M).contiguous()
    return rows.contiguous(), s


def assert_greedy_consistent(pick, rows, s, theta, tol, filled=None, max_near=4, what=''):
    """pick [B, K] slot numbers (a kernel's): GIVEN its own earlier picks, the pick of step t is an available slot with
    m64_t(pick_t) >= max m64_t - 2 tol (tol: the round-off of theta * sim in fp32; s is an input and carries none), and -1
    exactly when nothing is available.  Also asserts that at most max_near available slots lie within 2 tol of the maximum
    at any step of any session - else the draw cannot tell a right pick from a wrong one.  Returns the largest count."""
    pick = pick.cpu().long()
    s = s.double().cpu()
    B, M = s.shape
    sim = sims64(rows.cpu())
    avail = torch.ones(B, M, dtype=torch.bool) if filled is None else filled.clone().cpu()
    pen = torch.zeros(B, M, dtype=torch.float64)
    ar = torch.arange(B)
    worst = 0
    for t in range(pick.shape[1]):
        m = torch.where(avail, _scores(s, pen, theta, t), torch.full_like(s, NINF))
        p = pick[:, t]
        some = avail.any(1)
        assert bool(((p >= 0) == some).all()), '%s: step %d: sessions %s pick / leave out of step with the filled slots' % (
            what, t, ((p >= 0) != some).nonzero().flatten().tolist()[:8])
        assert bool((p < M).all())
        pc = p.clamp(min=0)
        assert bool(avail[ar, pc][some].all()), '%s: step %d: a slot that is unfilled or already picked was picked' % (what, t)
        best = m.max(1).values
        finite = some & (best > NINF)
        short = finite & (m[ar, pc] < best - 2 * tol)
        assert not bool(short.any()), '%s: step %d: sessions %s picked a slot %.3e below the best' % (
            what, t, short.nonzero().flatten().tolist()[:8], float((best - m[ar, pc])[short].max()))
        near = (avail & (m >= best[:, None] - 2 * tol) & finite[:, None]).sum(1)
        worst = max(worst, int(near.max()))
        to = sim[ar, :, pc]
        pen = torch.where(some[:, None], to if t == 0 else torch.maximum(pen, to), pen)
        avail[ar[some], p[some]] = False
    assert worst <= max_near, '%s: %d slots within round-off of the best at some step: the check is vacuous' % (what, worst)
    return worst
