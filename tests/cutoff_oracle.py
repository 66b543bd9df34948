"""float64 restatement of the cutoff contract of csrc/score_cutoff.hip (include/srec.h: srec_score_cutoff), shared by
tests/test_cutoff_cpu.py, tests/test_cutoff_gpu.py and tests/cutoff_gpu_worker.py.  Scores and eligibility come from the
existing oracles (select_oracle.scores64, sample_oracle.biased64: s' float64 [B, V] and the mask of INELIGIBLE pairs).
Everything is materialised, sorted and summed: this is the yardstick, not the product."""
import math

import numpy as np
import torch

from sample_oracle import biased64, stat_case  # noqa: F401  (re-exported: the score half of the contract)
from select_oracle import exact_case, scores64  # noqa: F401

NINF = float('-inf')
TOL_S = 1e-4                # the project's fp32 score bound (tests/test_rank_gpu.py)
# exact scores: the fp32 argument (s' - m) / T with |arg| <~ 20 gives about 1.2e-6 relative error in a weight, expf adds about
# 1e-7, the fixed-point quantum at most 1e-6 - about a 4x margin
TOL_MASS_EXACT = 1e-5
EXACT_SHAPES = [(33, 5000, 96), (37, 1300, 64), (40, 3429, 64)]
EXACT_TS = (1.0, 0.5, 2.0)
EXACT_PS = (0.5, 0.9)
EXACT_MIN_PS = (1.0, 0.5, 1e-3)
RANDOM_SHAPES = [(33, 5000, 96), (40, 3429, 64)]


def tol_m(T):
    """the mass a score error of TOL_S can move, per unit of mass, plus the weights' own error"""
    return 1e-4 * max(1.0, 1.0 / T) + 1e-5


def exact_inputs(B, V, d):
    """select_oracle.exact_case with the session vectors scaled by 1/8: every score is exact in fp32, and the soft-max is no
    longer concentrated on a handful of items"""
    sr, E, cs = exact_case(B, V, d)
    return sr / 8, E, cs


def random_inputs(scale=1.0):
    """the generator of test_sample_gpu's reproducibility case (B 37, V 1300, d 64); scale multiplies the session vectors"""
    B, V, d = 37, 1300, 64
    g = torch.Generator().manual_seed(21)
    sr = torch.randn(B, d, generator=g) * 0.3 * scale
    E = torch.randn(V, d, generator=g) * 0.2
    cs = torch.rand(V, generator=g) + 0.5
    return sr, E, cs


def _prep(s64, dm):
    """(s with the ineligible pairs at -inf, eligible bool [B, V]); -0.0 canonicalised"""
    s = s64.double().cpu().clone() + 0.0
    elig = torch.ones_like(s, dtype=torch.bool) if dm is None else ~dm.cpu()
    s[~elig] = NINF
    return s, elig


def weights64(s64, dm, T):
    """(w float64 [B, V]: exp((s' - m) / T) over the eligible pairs, 0 elsewhere and wherever s' = -inf; m float64 [B])"""
    s, elig = _prep(s64, dm)
    m = s.max(1).values if s.shape[1] else torch.full((s.shape[0],), NINF, dtype=torch.float64)
    ms = torch.where(m == NINF, torch.zeros_like(m), m)
    w = torch.exp((s - ms[:, None]) / T)
    w[s == NINF] = 0.0
    return w, m


def tau_k64(s64, dm, k):
    """the k-th largest eligible s', counting multiplicity; -inf with fewer than k eligible rows"""
    s, elig = _prep(s64, dm)
    B, V = s.shape
    if k > V:
        return torch.full((B,), NINF, dtype=torch.float64)
    kth = s.sort(1, descending=True).values[:, k - 1]
    return torch.where(elig.sum(1) >= k, kth, torch.full_like(kth, NINF))


def tau_p64(s64, dm, T, p):
    """the largest eligible score VALUE t with mass{s' >= t} >= p W (ties with t are inside); -inf where W = 0"""
    s, _ = _prep(s64, dm)
    w, _ = weights64(s64, dm, T)
    v, o = s.sort(dim=1, descending=True, stable=True)
    cum = w.gather(1, o).cumsum(1)
    W = cum[:, -1]
    last = torch.ones_like(v, dtype=torch.bool)
    last[:, :-1] = v[:, :-1] != v[:, 1:]
    # mass at or above the value of position i: the running sum at the END of its tie group (cum is non-decreasing)
    ge = torch.where(last, cum, torch.full_like(cum, float('inf'))).flip(1).cummin(1).values.flip(1)
    hit = ge >= (p * W)[:, None]
    first = hit.int().argmax(1)
    t = v.gather(1, first[:, None])[:, 0]
    return torch.where((W > 0) & hit.any(1), t, torch.full_like(t, NINF))


def gap32(T, q):
    """the scalar the host passes for min_p = q: -T ln q in double, rounded once to fp32"""
    return float(np.float32(abs(-T * math.log(q))))


def tau_q32(m, T, q):
    """fp32(m - gap) as the kernel forms it (m exact in fp32); -inf stays -inf"""
    m32 = m.to(torch.float32)
    return torch.where(m32 == NINF, m32, m32 - torch.tensor(gap32(T, q), dtype=torch.float32)).double()


def floor64(s64, dm, T=1.0, top_k=None, top_p=None, min_p=None):
    """float64 [B]: the largest of the criteria given, -inf with none"""
    B = s64.shape[0]
    f = torch.full((B,), NINF, dtype=torch.float64)
    if top_k is not None:
        f = torch.maximum(f, tau_k64(s64, dm, top_k))
    if top_p is not None and top_p < 1.0:
        f = torch.maximum(f, tau_p64(s64, dm, T, top_p))
    if min_p is not None:
        f = torch.maximum(f, tau_q32(weights64(s64, dm, T)[1], T, min_p))
    return f + 0.0


def count64(s64, dm, floor):
    """int64 [B]: eligible rows with s' >= floor (an eligible row scoring -inf counts under floor = -inf only)"""
    s, elig = _prep(s64, dm)
    return (elig & (s >= floor.double()[:, None])).sum(1)


def mass_ge64(s64, dm, T, t, strict=False):
    """float64 [B]: the share of W held by the eligible rows with s' >= t (strict: > t); 0 where W = 0"""
    s, _ = _prep(s64, dm)
    w, _ = weights64(s64, dm, T)
    t = torch.as_tensor(t, dtype=torch.float64).reshape(-1, 1)
    keep = (s > t) if strict else (s >= t)
    W = w.sum(1)
    return torch.where(W > 0, (w * keep).sum(1) / torch.where(W > 0, W, torch.ones_like(W)), torch.zeros_like(W))


def kept64(s64, dm, T, floor):
    """float64 [B]: log(mass{s' >= floor} / W); -inf with nothing eligible, 0 when every eligible row scores -inf"""
    s, elig = _prep(s64, dm)
    w, _ = weights64(s64, dm, T)
    W = w.sum(1)
    n = count64(s64, dm, floor)
    share = mass_ge64(s64, dm, T, floor)
    out = torch.log(torch.where(share > 0, share, torch.ones_like(share)))
    out = torch.where((W > 0) & (share == 0), torch.full_like(out, NINF), out)
    return torch.where(n == 0, torch.full_like(out, NINF), out)


def decided(s64, dm, T, p, tol=TOL_MASS_EXACT):
    """bool [B]: the nucleus boundary is further than tol (in mass) from p on both sides - round-off cannot move it"""
    t = tau_p64(s64, dm, T, p)
    margin = torch.minimum(mass_ge64(s64, dm, T, t) - p, p - mass_ge64(s64, dm, T, t, strict=True))
    return margin > tol


def neighbours(s64, dm, t):
    """(the next distinct eligible score value above t, the next below) per session (+inf / -inf where there is none)"""
    s, elig = _prep(s64, dm)
    t = t.double()[:, None]
    up = torch.where(elig & (s > t), s, torch.full_like(s, float('inf'))).min(1).values
    dn = torch.where(elig & (s < t), s, torch.full_like(s, NINF)).max(1).values
    return up, dn


def near(s64, dm, t, width):
    """int64 [B]: eligible rows within `width` of the value t"""
    s, elig = _prep(s64, dm)
    return (elig & ((s - t.double()[:, None]).abs() <= width)).sum(1)


def top_p_interval(s64, dm, T, p):
    """(n_lo, n_hi) int64 [B]: the counts a floor consistent with scores known to TOL_S and masses known to tol_m(T) may have:
    n_lo = count64(p - tol_m) - w_lo, n_hi = count64(p + tol_m) + w_hi, w_* the eligible rows within 2 TOL_S of that boundary"""
    tm = tol_m(T)
    lo_t = tau_p64(s64, dm, T, max(p - tm, 1e-12))
    hi_t = tau_p64(s64, dm, T, min(p + tm, 1.0))
    n_lo = count64(s64, dm, lo_t) - near(s64, dm, lo_t, 2 * TOL_S)
    n_hi = count64(s64, dm, hi_t) + near(s64, dm, hi_t, 2 * TOL_S)
    return n_lo, n_hi


def assert_top_p_consistent(floor, count, s64, dm, T, p, what=''):
    """check (b) of the issue: the floor's mass brackets p within the tolerances, and the count lies in top_p_interval"""
    f = floor.detach().double().cpu()
    tm = tol_m(T)
    live = weights64(s64, dm, T)[0].sum(1) > 0
    ge = mass_ge64(s64, dm, T, f - TOL_S)
    gt = mass_ge64(s64, dm, T, f + TOL_S, strict=True)
    assert bool((ge[live] >= p - tm).all()), (what, 'too little mass at or above the floor', float(ge[live].min()))
    assert bool((gt[live] < p + tm).all()), (what, 'too much mass above the floor', float(gt[live].max()))
    n_lo, n_hi = top_p_interval(s64, dm, T, p)
    c = count.detach().long().cpu()
    ok = (c >= n_lo) & (c <= n_hi)
    assert bool(ok[live].all()), (what, 'count outside the interval', c[live][~ok[live]].tolist()[:4])
    return n_hi - n_lo


def brute(scores, elig, T, top_k=None, top_p=None, min_p=None):
    """one session, plain python: (floor, count, log_kept, top) by sorting the eligible scores - the check of the oracle"""
    e = sorted((float(s) + 0.0 for s, ok in zip(scores, elig) if ok), reverse=True)
    if not e:
        return NINF, 0, NINF, NINF
    m = e[0]
    w = [0.0 if (s == NINF or m == NINF) else math.exp((s - m) / T) for s in e]
    W = sum(w)
    f = NINF
    if top_k is not None and len(e) >= top_k:
        f = max(f, e[top_k - 1])
    if top_p is not None and top_p < 1.0 and W > 0:
        i, acc = 0, 0.0
        while i < len(e):
            j = i
            while j < len(e) and e[j] == e[i]:
                acc += w[j]
                j += 1
            if acc >= top_p * W:
                f = max(f, e[i])
                break
            i = j
    if min_p is not None and m != NINF:
        f = max(f, float(np.float32(np.float32(m) - np.float32(gap32(T, min_p)))))
    kept = [x for s, x in zip(e, w) if s >= f]
    n = len(kept)
    lk = 0.0 if W == 0 else math.log(sum(kept) / W)
    return f + 0.0, n, lk, m
