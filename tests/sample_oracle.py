"""float64 restatement of the sampling contract of csrc/recommend.hip (include/srec.h: srec_score_sample), shared by
tests/test_sample_cpu.py, tests/test_sample_gpu.py and tests/sample_gpu_worker.py: the counter-based noise in numpy (uint32
arithmetic, np.float32 for w, the two logarithms in float64), the sampled key  key64 = s64 / T + g64,  and the statistics a
draw is judged by.  Scores, selection and the list check come from the existing oracles.  Everything is materialised: this
is the yardstick, not the product."""
import numpy as np
import torch

from item_bias_oracle import NINF, bias_rows
from select_oracle import scores64

U32 = np.uint32
TOL_NOISE = 1e-5            # fp32 logf / log1pf within 2 ulp: < 2e-7 on log E, < 2e-6 after the rounding at |g| <= 22.9; margin over that
CHI2_5 = 25.74              # 1 - 1e-4 quantile of chi-square, 5 degrees of freedom (first draw among 6 items)
CHI2_19 = 50.80             # ... 19 degrees of freedom (ordered pairs among 5 items)
LN2 = 0.6931471805599453


def tol_key(T):
    """the project's fp32 score bound (1e-4, tests/test_rank_gpu.py), scaled by 1 / T, plus the noise's"""
    return 1e-4 * max(1.0, 1.0 / T) + TOL_NOISE


def h32(x):
    """"lowbias32" on uint32 arrays"""
    x = x.astype(U32)
    x = x ^ (x >> U32(16))
    x = x * U32(0x7feb352d)
    x = x ^ (x >> U32(15))
    x = x * U32(0x846ca68b)
    return x ^ (x >> U32(16))


def _u32(a):
    """integers (any sign, a tensor or a sequence) as their 32-bit pattern"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return (a.astype(np.int64) & 0xffffffff).astype(U32).reshape(-1)


def w_of(h):
    """fminf(fmaf((float)h, 2^-32, 2^-33), 1 - 2^-24): product and sum are exact in float64, one rounding to fp32"""
    w = (h.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32)
    return np.minimum(w, np.float32(1.0 - 2.0 ** -24))


def hash_hw(seed, keys, ids):
    """(h uint32 [nb, nv], w float32 [nb, nv]) for session keys and GLOBAL item ids"""
    lo, hi = U32(seed & 0xffffffff), U32(seed >> 32)
    with np.errstate(over='ignore'):
        skey = h32(lo ^ h32(_u32(keys) * U32(0x9E3779B9) + hi * U32(0x85EBCA6B) + U32(0x165667B1)))
        h = h32(skey[:, None] ^ (_u32(ids) * U32(0x9E3779B1) + U32(0x7F4A7C15))[None, :])
    return h, w_of(h)


def log64(x):
    """natural log in float64 from +, -, *, / and frexp alone - the lines of score._log64, so that the two agree to the bit
    on every host (numpy's, torch's and libm's logs differ in the last place); test_sample_cpu holds it against np.log"""
    m, e = np.frexp(x)
    small = m < 0.7071067811865476
    m = np.where(small, m * 2.0, m)
    e = e.astype(np.float64) - small.astype(np.float64)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = np.full_like(t, 1.0 / 27.0)
    for n in range(25, 0, -2):
        p = p * t2 + 1.0 / n
    return e * LN2 + 2.0 * t * p


def gumbel_of_w(w):
    """float64 -log(-log1p(-w)); log1p by Kahan's identity on the rounded u = 1 - w"""
    w = w.astype(np.float64)
    u = 1.0 - w
    one = u == 1.0
    l1 = np.where(one, -w, log64(u) * (-w) / np.where(one, -1.0, u - 1.0))
    return -log64(-l1)


def gumbel64(seed, keys, ids):
    """float64 tensor [nb, nv]: g(seed, q, id)"""
    return torch.from_numpy(gumbel_of_w(hash_hw(seed, keys, ids)[1]))


def key64(s64, T, seed, keys=None, id_lo=0):
    """float64 [B, n]: s64 / T + g for the columns id_lo .. id_lo + n; keys None = the row index"""
    B, n = s64.shape
    keys = np.arange(B) if keys is None else keys
    return s64.double().cpu() / T + gumbel64(seed, keys, np.arange(id_lo, id_lo + n))


def biased64(srs, E, cs, off_ex, off_in, listed, drop, bias, group):
    """(s' float64 [B, V], ineligible bool [B, V] or None): scores64 plus the bias rows; listed items dropped (drop) or scored"""
    from select_oracle import drop_mask
    V = E.shape[0]
    if drop:
        s, dm = scores64(srs, E, cs, off_ex), drop_mask(listed, V)
    else:
        s, dm = scores64(srs, E, cs, off_ex, off_in, listed), None
    if bias is not None:
        rows = bias_rows(bias, group, s.shape[0])
        s = s + rows
        dm = (rows == NINF) if dm is None else dm | (rows == NINF)
    return s, dm


def min_gap(k64, k, drop=None):
    """the smallest difference between neighbours among the k + 1 best eligible keys of any session: above the round-off, the
    ids of the list are decided"""
    s = k64.clone()
    if drop is not None:
        s[drop] = NINF
    top = s.topk(min(k + 1, s.shape[1]), dim=1).values
    d = top[:, :-1] - top[:, 1:]
    return float(d[torch.isfinite(d)].min())


# ------------------------------------------------------------------------------------------- the distribution
STAT_B, STAT_D, STAT_SEED = 4096, 32, 2024


def stat_case(V):
    """(sr [B, d] - B copies of one session vector, E [V, d], bias [V] or None): entries are multiples of 1/8, so the fp32
    score is exact.  V = 8: a bias that takes two items out of the catalogue and moves the others (first draw); V = 5: no bias
    (ordered pairs)"""
    g = torch.Generator().manual_seed(100 + V)
    sr = (torch.randint(-4, 5, (1, STAT_D), generator=g).float() / 8).expand(STAT_B, STAT_D).contiguous()
    E = torch.randint(-3, 4, (V, STAT_D), generator=g).float() / 8
    bias = None
    if V == 8:
        bias = torch.randint(-4, 5, (V,), generator=g).float() / 8
        bias[[2, 5]] = NINF
    return sr, E, bias


def stat_probs(V, T):
    """float64 [V]: softmax(s' / T) over the eligible items (0 for the others)"""
    sr, E, bias = stat_case(V)
    s = scores64(sr[:1], E)[0]
    if bias is not None:
        s = s + bias.double()
    return torch.softmax(s / T, 0)


def chi2_first(ids, p):
    """chi-square of the first-draw counts of ids [B] against probabilities p [V] (the items with p > 0)"""
    ids = ids.long().cpu().reshape(-1)
    cnt = torch.bincount(ids, minlength=p.numel()).double()
    live = p > 0
    assert float(cnt[~live].sum()) == 0, 'an ineligible item was drawn'
    exp = p[live] * ids.numel()
    return float(((cnt[live] - exp) ** 2 / exp).sum())


def chi2_pairs(ids, p):
    """chi-square of the ordered-pair counts of ids [B, 2] against Plackett-Luce p_i p_j / (1 - p_i), i != j"""
    ids = ids.long().cpu()
    V = p.numel()
    cnt = torch.bincount(ids[:, 0] * V + ids[:, 1], minlength=V * V).double().reshape(V, V)
    exp = p[:, None] * p[None, :] / (1.0 - p[:, None]) * ids.shape[0]
    off = ~torch.eye(V, dtype=torch.bool)
    assert float(cnt[~off].sum()) == 0, 'an item was drawn twice'
    return float(((cnt[off] - exp[off]) ** 2 / exp[off]).sum())


def oracle_draw(V, k, T, seed=STAT_SEED):
    """int64 [B, k]: the draw of the oracle itself for stat_case(V) with keys arange(B)"""
    sr, E, bias = stat_case(V)
    s, dm = biased64(sr, E, None, None, None, None, False, bias, None)
    k64 = key64(s, T, seed)
    if dm is not None:
        k64[dm] = NINF
    return k64.topk(k, dim=1).indices


# ------------------------------------------------------------------------------------------- the cases both test files share
NOISE_SHAPE, NOISE_SEED = (37, 1300, 32, 128), 225       # (B, V, d, K): sr = 0, the keys are the noise; the seed: min_gap > 2 TOL_NOISE
LIST_SHAPES = [(33, 5000, 96), (40, 3429, 64)]
LIST_KINDS = ['single', 'mix3', 'listed-score', 'listed-drop']
LIST_TS = (1.0, 0.5, 2.0)
LIST_K, LIST_SEED = 50, 1


def list_case(B, V, d, kind, mode):
    """the random case of tests/test_select_gpu._random_case with a bias: mode 'row' - fp32 [V], a third of it -inf; 'groups' -
    [3, V] with group = b % 3.  -> (srs, E, cs, off_ex, off_in, listed, drop, bias, group)"""
    from item_bias_oracle import exact_bias
    from test_select_gpu import _random_case
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    if mode == 'row':
        bias, group = exact_bias(V, None, off_share=1.0 / 3, off_ranges=()), None
    else:
        bias, group = exact_bias(V, 3, off_ranges=()), torch.arange(B) % 3
    return srs, E, cs, off_ex, off_in, listed, kind == 'listed-drop', bias, group
