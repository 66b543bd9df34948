"""The calibrated greedy re-rank in float64: what csrc/calibrate.hip (ops.calibrate, model.recommend_calibrated) must pick.

Per session: a pool of M slots (ids, val), the category of an item (category[id], < 0: none), a target of T pairs (category
id, weight; a category < 0 or a weight <= 0 is an empty pair, duplicates add up).  P_c the summed weights of category c,
S = {c: P_c > 0}, p_c = P_c / sum_S P_c; without any such category the session has no target and its term is 0.  After some
picks n_c counts the picks of category c and N the picks with any category >= 0;
    KL(n, N) = sum_{c in S} p_c log(p_c / ((1 - a) n_c / max(N, 1) + a p_c))
and step t picks the available slot with the largest m = (1 - w) val - w KL(state with the slot added), ties to the lower slot
(w == 0: m = val; val == -inf: m = -inf).  w and a are the fp32-rounded scalars the kernel receives.  The term is evaluated ONCE
PER CATEGORY: adding a slot changes the state in one of 2 + |S| ways (uncategorised, a category outside S, category c of S).

The kernel forms the same sums in double in another order: the two differ by double round-off only - at most 256 terms of
magnitude at most about 25, a few ulp of a log each, about 1e-12 in all - so TOL = 1e-9 separates "the same candidate" from
"another one" with three orders of magnitude to spare, and the kernel's picks are compared with == wherever the oracle's best
two candidates are at least TOL apart (`margin`)."""
import numpy as np
import torch

NINF = float('-inf')
TOL = 1e-9
F32 = 2.0 ** -23                 # the kernel's obj / kl are fp32 roundings of double values


class Session:
    """one session's target, slots and state"""

    def __init__(self, ids, val, category, weight, tcat, tw, alpha):
        n_items = len(category)
        self.w, self.a = float(np.float32(weight)), float(np.float32(alpha))
        self.val = np.asarray(val, dtype=np.float32).astype(np.float64)
        ids = np.asarray(ids, dtype=np.int64)
        self.filled = (ids >= 0) & (ids < n_items)
        cat = np.where(self.filled, np.asarray(category, dtype=np.int64)[np.where(self.filled, ids, 0)], -1)
        P = {}
        if tcat is not None:
            for c, x in zip(np.asarray(tcat, dtype=np.int64).tolist(), np.asarray(tw, dtype=np.float32).astype(np.float64).tolist()):
                if c >= 0 and x > 0:
                    P[c] = P.get(c, 0.0) + x
        self.S = sorted(P)
        W = sum(P[c] for c in self.S)
        self.target = W > 0
        self.p = np.array([P[c] / W for c in self.S]) if self.target else np.zeros(0)
        where = {c: j for j, c in enumerate(self.S)}
        # kind of a slot: -1 uncategorised, -2 a category outside S, j >= 0: category S[j]
        self.kind = np.array([-1 if c < 0 else where.get(c, -2) if self.target else -2 for c in cat.tolist()], dtype=np.int64)
        self.n = np.zeros(len(self.S))
        self.N = 0
        self.avail = self.filled.copy()

    def _kl(self, n, N):
        """KL for rows of counts n [..., |S|] over N categorised picks"""
        if not self.target:
            return np.zeros(n.shape[:-1])
        return (self.p * np.log(self.p / ((1.0 - self.a) * n / max(N, 1) + self.a * self.p))).sum(-1)

    def kl(self):
        return float(self._kl(self.n, self.N))

    def objective(self):
        """m [M] float64 of every slot under the state so far (meaningful where avail)"""
        if self.w == 0.0:
            m = self.val.copy()
        else:
            kl_none = self._kl(self.n, self.N)                                  # once per way of changing the state
            kl_out = self._kl(self.n, self.N + 1)
            kl_in = self._kl(self.n[None, :] + np.eye(len(self.S)), self.N + 1) if self.S else np.zeros(0)
            kl = np.where(self.kind == -1, kl_none, kl_out)
            inside = self.kind >= 0
            kl[inside] = kl_in[self.kind[inside]]
            with np.errstate(invalid='ignore'):
                m = (1.0 - self.w) * self.val - self.w * kl
        m[self.val == NINF] = NINF
        return m

    def take(self, i):
        self.avail[i] = False
        if self.kind[i] != -1:
            self.N += 1
            if self.kind[i] >= 0:
                self.n[self.kind[i]] += 1


def _rows(x, B):
    return [None] * B if x is None else [r for r in np.asarray(x)]


def greedy64(ids, val, category, k, weight, tcat=None, tw=None, alpha=0.01):
    """dict(pick int64 [B,k] (-1: the filled slots ran out), val fp32 [B,k] = val[pick] (-inf in the tail), obj float64 [B,k]
    the winning m (-inf in the tail), kl float64 [B] of the final picks, margin float64 [B,k]: best minus second best of the
    step (inf with one candidate or none, 0 for two at -inf))"""
    ids, val = np.asarray(ids), np.asarray(val, dtype=np.float32)
    B, M = ids.shape
    pick = np.full((B, k), -1, dtype=np.int64)
    obj = np.full((B, k), NINF)
    margin = np.full((B, k), np.inf)
    kl = np.zeros(B)
    category = np.asarray(category)
    for b, (tc, x) in enumerate(zip(_rows(tcat, B), _rows(tw, B))):
        s = Session(ids[b], val[b], category, weight, tc, x, alpha)
        for t in range(k):
            if not s.avail.any():
                break
            m = np.where(s.avail, s.objective(), NINF)
            cand = np.flatnonzero(s.avail)
            i = int(cand[np.argmax(m[cand])])                                   # (argmax: the first of equals, the lower slot)
            if len(cand) > 1:
                second = np.max(np.delete(m[cand], np.argmax(m[cand])))
                margin[b, t] = 0.0 if second == m[i] else m[i] - second
            pick[b, t], obj[b, t] = i, m[i]
            s.take(i)
        kl[b] = s.kl()
    got = pick >= 0
    out_val = np.where(got, np.take_along_axis(val, np.maximum(pick, 0), 1), np.float32(NINF)).astype(np.float32)
    return dict(pick=torch.from_numpy(pick), val=torch.from_numpy(out_val), obj=torch.from_numpy(obj), kl=torch.from_numpy(kl),
                margin=torch.from_numpy(margin))


def assert_greedy_consistent(pick, ids, val, category, weight, tcat=None, tw=None, alpha=0.01, obj=None, kl=None):
    """pick [B,k] is A greedy solution: replaying the caller's OWN prefix, the pick of every step is an available slot whose
    float64 objective is within TOL * max(1, |best|) of the best one's, and -1 exactly when nothing is available.  obj / kl
    (the kernel's fp32 outputs), when given, are compared at 2^-23 max(1, |value|) with the float64 values of that prefix.
    Returns (ties, worst |obj - f64|, worst |kl - f64|): ties = the steps with another candidate within TOL of the pick."""
    ids, val, pick = np.asarray(ids), np.asarray(val, dtype=np.float32), np.asarray(pick)
    B, k = pick.shape
    category = np.asarray(category)
    ties, worst_obj, worst_kl = 0, 0.0, 0.0
    for b, (tc, x) in enumerate(zip(_rows(tcat, B), _rows(tw, B))):
        s = Session(ids[b], val[b], category, weight, tc, x, alpha)
        for t in range(k):
            i = int(pick[b, t])
            if not s.avail.any():
                assert i == -1, 'session %d step %d: pick %d with nothing available' % (b, t, i)
                if obj is not None:
                    assert float(obj[b, t]) == NINF, (b, t)
                continue
            assert 0 <= i < len(s.avail) and s.avail[i], 'session %d step %d: slot %d is not available' % (b, t, i)
            m = np.where(s.avail, s.objective(), NINF)
            best = float(m.max())
            assert m[i] >= best - TOL * max(1.0, abs(best)), 'session %d step %d: slot %d has %r, the best %r' % (b, t, i, m[i], best)
            ties += int(((m >= m[i] - TOL * max(1.0, abs(best))) & s.avail).sum() > 1)
            if obj is not None:
                got = float(obj[b, t])
                if m[i] == NINF:
                    assert got == NINF, (b, t, got)
                else:
                    assert abs(got - m[i]) <= F32 * max(1.0, abs(m[i])), 'session %d step %d: obj %r, float64 %r' % (b, t, got, m[i])
                    worst_obj = max(worst_obj, abs(got - m[i]))
            s.take(i)
        if kl is not None:
            want = s.kl()
            assert abs(float(kl[b]) - want) <= F32 * max(1.0, abs(want)), 'session %d: kl %r, float64 %r' % (b, float(kl[b]), want)
            worst_kl = max(worst_kl, abs(float(kl[b]) - want))
    return ties, worst_obj, worst_kl


def random_case(B, M, T, G, seed=0, n_items=None, target_cats=None):
    """(ids int64 [B,M], val fp32 [B,M] descending around -8 +- 2, category int32 [n_items] in [-1, G), tcat int64 [B,T] in
    [-1, target_cats) (default min(G, 10)), tw fp32 [B,T] > 0)"""
    g = torch.Generator().manual_seed(7919 * seed + 31 * B + 7 * M + 3 * T + G)
    n_items = max(2 * M, 64) if n_items is None else n_items
    category = torch.randint(-1, G, (n_items,), generator=g).to(torch.int32)
    ids = torch.stack([torch.randperm(n_items, generator=g)[:M] for _ in range(B)])
    val = torch.sort(-8.0 + 2.0 * torch.randn(B, M, generator=g), 1, descending=True).values
    tcat = torch.randint(-1, min(G, 10) if target_cats is None else target_cats, (B, T), generator=g)
    tw = torch.rand(B, T, generator=g) + 0.05
    return ids, val, category, tcat, tw


def lists(val, ids, r):
    """(values fp32 [B,k], item ids int32 [B,k]) of greedy64's result r over the pool (val, ids): the pool's own numbers at the
    picks, (-inf, -1) in the tail - what model.recommend_calibrated returns for that pool"""
    pick = r['pick']
    got = pick >= 0
    i = torch.where(got, ids.long().gather(1, pick.clamp(min=0)), torch.full((), -1, dtype=torch.long))
    return r['val'], i.to(torch.int32)
