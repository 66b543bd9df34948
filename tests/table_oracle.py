"""float64 oracle of the item-table optimizer pass (csrc/adam.hip: srec_adam_rows / srec_adam_rows_proj) and of the row
kernels around it (csrc/rowops.hip), the fp32 restatement that sets the tolerances, and the shared case table.

The oracle is plain torch float64 written from what the operations MEAN (torch.optim.Adam with coupled L2,
torch.embedding_renorm_, F.normalize / NISER's norm + eps, the chain rule of E / |E|), not from the kernel's expression order;
tests/test_table_step_oracle.py pins every piece to torch itself on the CPU.  Nothing here imports the product.

Tolerance rule (the same for every compared quantity): the same formula is evaluated in fp32 torch on the same inputs
(`table_step32`, the straightforward restatement), its error against the oracle is measured with `rel_err`, and the kernel is
allowed `bound(e32) = max(4 e32, 2 ulp)`: 4x for the reduction order of a 64-lane sum and the contraction of multiply-adds,
which differ from torch's, and never below 2 ulp (2 * 2^-23) because a restatement that happens to round exactly says nothing
about another expression order.  `rel_err` is max |x - ref| / (|ref| + floor) over ALL elements, floor = the fp32 ulp of the
row's largest reference magnitude; no element is excluded.  Every comparison is made a second time, under the same rule, in
`row_err` (the differences over the row's largest magnitude), because rel_err is decided by the elements that cancel to ~0.
"""
import collections
import math

import numpy as np
import torch

F64 = torch.float64
ULP = 2.0 ** -23
CS_SCALE = 12.0                 # NISER / MSGIFSR cosine scale
CS_EPS = 2.0 ** -40             # ~9.1e-13, exact in fp32 and fp64: the zero row's cs = CS_SCALE / CS_EPS is exact in both
INV_SCALE = float(np.float32(1.0 / CS_SCALE))
ADAM = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)


def _d(x):
    return torch.as_tensor(x).detach().to('cpu', F64)


# ----------------------------------------------------------------------------------------------------------- the oracle
def adam_step64(p, g, m, v, lr, b1, b2, eps, wd, t):
    """torch.optim.Adam (coupled L2 decay, bias correction), step number t >= 1 -> (p, m, v)"""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    m_hat = m / (1.0 - b1 ** t)
    v_hat = v / (1.0 - b2 ** t)
    return p - lr * m_hat / (v_hat.sqrt() + eps), m, v


def renorm64(W, max_norm):
    """torch.embedding_renorm_ of every row (max_norm <= 0: none)"""
    W = _d(W)
    if max_norm <= 0:
        return W
    n = W.pow(2).sum(1, keepdim=True).sqrt()
    return torch.where(n > max_norm, W * (max_norm / (n + 1e-7)), W)


def cs64(W, scale, eps_mode, eps):
    """scale / max(|W_v|, eps) (eps_mode 0, F.normalize) or scale / (|W_v| + eps) (eps_mode 1, NISER)"""
    n = _d(W).pow(2).sum(1).sqrt()
    return scale / n.clamp(min=eps) if eps_mode == 0 else scale / (n + eps)


def project64(W, cs, inv_scale, dE):
    """chain rule of the row normalisation applied to the gradient dE w.r.t. the UNnormalised direction:
    dE - W <W, dE> (cs inv_scale)^2"""
    W, dE = _d(W), _d(dE)
    iv = (_d(cs) * inv_scale).unsqueeze(1)
    return dE - W * ((W * dE).sum(1, keepdim=True) * iv * iv)


def lookup_sum64(rows, items, ptr, pos, n, d, dtype=F64):
    """l [n, d]: l[items[u]] = sum of rows[pos[ptr[u]:ptr[u+1]]] (the lookup gradient added after the scoring gradient);
    dtype float32: the fp32 restatement of the same sums"""
    l = torch.zeros(n, d, dtype=dtype)
    rows = rows.detach().to('cpu', dtype)
    for u, it in enumerate(items.tolist()):
        l[it] = rows[pos[ptr[u]:ptr[u + 1]].long()].sum(0)
    return l


def table_step64(W, M, V, dE, l, hp, t, use_wd, max_norm, renorm_write, cs_scale=None, eps_mode=0, cs_eps=CS_EPS,
                 proj_cs=None, proj_inv_scale=INV_SCALE):
    """srec_adam_rows (proj_cs None) / srec_adam_rows_proj as include/srec.h describes them: the projection applies to dE only
    (the part of the gradient buffer not covered by `radial`), l is added after it; Adam; W is the renormed row when
    renorm_write else the plain Adam result; cs (cs_scale given) is that of the renormed row either way."""
    g = _d(dE) if proj_cs is None else project64(W, proj_cs, proj_inv_scale, dE)
    if l is not None:
        g = g + _d(l)
    p, m, v = adam_step64(W, g, M, V, hp['lr'], hp['b1'], hp['b2'], hp['eps'], hp['wd'] if use_wd else 0.0, t)
    pr = renorm64(p, max_norm)
    out = dict(W=pr if renorm_write else p, M=m, V=v)
    if cs_scale is not None:
        out['cs'] = cs64(pr, cs_scale, eps_mode, cs_eps)
    return out


def bf16_copy(W32, Dp):
    """the operand copy the scoring kernels read: round-to-nearest-even of the fp32 rows as written, zeros in d .. Dp"""
    n, d = W32.shape
    out = torch.zeros(n, Dp, dtype=torch.bfloat16, device=W32.device)
    out[:, :d] = W32.bfloat16()
    return out


# ---------------------------------------------------------------------------------------- fp32 restatement (the yardstick)
def hyper_host(lr, b1, b2, eps, wd, t):
    """the 8 step scalars in Python double, as include/srec.h lists them"""
    return [lr / (1.0 - b1 ** t), b1, b2, eps, wd, 1.0 - b1, 1.0 - b2, math.sqrt(1.0 - b2 ** t)]


def hyper32(hp, t):
    return torch.tensor(hyper_host(hp['lr'], hp['b1'], hp['b2'], hp['eps'], hp['wd'], t), dtype=torch.float32)


def adam_step32(p, g, m, v, h32, use_wd):
    """fp32 torch, the fp32 step scalars the kernels read (torch's own single-tensor order)"""
    h = [float(x) for x in h32]
    if use_wd:
        g = g + h[4] * p
    m = h[1] * m + h[5] * g
    v = h[2] * v + h[6] * g * g
    return p - h[0] * (m / (v.sqrt() / h[7] + h[3])), m, v


def renorm32(W, max_norm):
    if max_norm <= 0:
        return W
    n = W.norm(dim=1, keepdim=True)
    return torch.where(n > max_norm, W * (max_norm / (n + 1e-7)), W)


def cs32(W, scale, eps_mode, eps):
    n = W.norm(dim=1)
    return scale / n.clamp(min=eps) if eps_mode == 0 else scale / (n + eps)


def project32(W, cs, inv_scale, G, radial=None):
    """the deferred form on the summed buffer: G - W (<W, G> - radial) iv^2 (radial None: G is the scoring gradient alone)"""
    iv = (cs * inv_scale).unsqueeze(1)
    dot = (W * G).sum(1, keepdim=True)
    if radial is not None:
        dot = dot - radial.unsqueeze(1)
    return G - W * (dot * iv * iv)


def table_step32(W, M, V, dE, l, h32, use_wd, max_norm, renorm_write, cs_scale=None, eps_mode=0, cs_eps=CS_EPS,
                 proj_cs=None, proj_inv_scale=INV_SCALE):
    """fp32 restatement of table_step64, on the gradient buffer as production builds it: G = dE + l, radial = <W, l>, the
    projection taken off the sum (so the <W, G> - radial cancellation is part of the yardstick)"""
    G = dE if l is None else dE + l
    if proj_cs is not None:
        G = project32(W, proj_cs, proj_inv_scale, G, None if l is None else (W * l).sum(1))
    p, m, v = adam_step32(W, G, M, V, h32, use_wd)
    pr = renorm32(p, max_norm)
    out = dict(W=pr if renorm_write else p, M=m, V=v)
    if cs_scale is not None:
        out['cs'] = cs32(pr, cs_scale, eps_mode, cs_eps)
    return out


def ulp32(x):
    x32 = _d(x).abs().float()
    u = (torch.nextafter(x32, torch.full_like(x32, float('inf'))) - x32).double()
    return u.clamp(min=float(torch.finfo(torch.float32).tiny))


def rel_err(x, ref):
    """max over ALL elements of |x - ref| / (|ref| + ulp32(row max |ref|)) -> (error, row, column)"""
    x, ref = _d(x), _d(ref)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if x.dim() == 1:
        x, ref = x.unsqueeze(1), ref.unsqueeze(1)
    e = (x - ref).abs() / (ref.abs() + ulp32(ref.abs().amax(1, keepdim=True)))
    assert not torch.isnan(e).any(), 'NaN'
    k = int(e.argmax())
    return float(e.flatten()[k]), k // e.shape[1], k % e.shape[1]


def row_err(x, ref):
    """max over ALL elements of |x - ref| / (row max |ref|) -> (error, row, column): the same differences on the scale of the
    row's summands.  rel_err alone is decided by the few elements that cancel to ~0 (there a fraction of an ulp of the row's
    magnitude already reads as 0.1 .. 1) and would let every ordinary element be wrong by as much; this one would not."""
    x, ref = _d(x), _d(ref)
    if x.dim() == 1:
        x, ref = x.unsqueeze(1), ref.unsqueeze(1)
    e = (x - ref).abs() / ref.abs().amax(1, keepdim=True).clamp(min=float(torch.finfo(torch.float32).tiny))
    k = int(e.argmax())
    return float(e.flatten()[k]), k // e.shape[1], k % e.shape[1]


def errs(x, ref):
    return rel_err(x, ref)[0], row_err(x, ref)[0]


def bound(e32):
    return max(4.0 * e32, 2.0 * ULP)


def check(name, got, ref, e32, what=''):
    """the per-row assertion in both measures (e32 = errs(restatement, ref)): names the worst row and column.

    rel measure, element by element: |x - ref| <= max(bound(e32) (|ref| + floor), 2 floor), floor = ulp32 of the row's largest
    reference magnitude.  The second term is the "never below 2 ulp" of the rule in the unit the measure itself uses for its
    floor: the summands of every compared quantity (b1 m and (1 - b1) g; p and its update; the addends of a lookup sum) are of
    the row's magnitude, so an expression order other than the restatement's may round them differently by ulps of THAT
    magnitude wherever they cancel - which 4 x the restatement's own luck at its own worst element does not cover when the
    sample is small (a 3-element tensor, a 1-row table: measured on the MI355X without this term, four misses of this kind,
    e.g. m = 1.64731e-05 for 1.64730e-05 after three steps of +-1e-3 summands, 0.4 ulp of a summand, against a restatement
    that happened to round to 3.6e-08).  Ordinary elements stay bound by row_err below."""
    g2, r2 = _d(got).reshape(len(got), -1), _d(ref).reshape(len(ref), -1)
    floor = ulp32(r2.abs().amax(1, keepdim=True))
    diff = (g2 - r2).abs()
    assert not torch.isnan(diff).any(), '%s %s: NaN' % (what, name)
    allowed = torch.maximum(bound(e32[0]) * (r2.abs() + floor), 2.0 * floor)
    ratio = diff / allowed
    k = int(ratio.argmax())
    r, c = k // g2.shape[1], k % g2.shape[1]
    e = rel_err(got, ref)[0]
    print('%s %s rel: kernel %.3e  fp32 restatement %.3e  bound %.3e  (worst element at %.2f of its allowance)' % (
        what, name, e, e32[0], bound(e32[0]), float(ratio.flatten()[k])))
    assert float(ratio.flatten()[k]) <= 1.0, '%s %s: |err| %.3e > allowed %.3e (rel bound %.3e from restatement %.3e), worst at ' \
        'row %d col %d: got %r want %r' % (what, name, float(diff[r, c]), float(allowed[r, c]), bound(e32[0]), e32[0], r, c,
                                           float(g2[r, c]), float(r2[r, c]))
    er, r, c = row_err(got, ref)
    b = bound(e32[1])
    print('%s %s row-scaled: kernel %.3e  fp32 restatement %.3e  bound %.3e' % (what, name, er, e32[1], b))
    assert er <= b, '%s %s: row-scaled err %.3e > bound %.3e (restatement %.3e), worst at row %d col %d: got %r want %r' % (
        what, name, er, b, e32[1], r, c, float(g2[r, c]), float(r2[r, c]))
    return e, er


# --------------------------------------------------------------------------------------------------------- the case table
# d, n, ld - d, use_wd, max_norm, renorm_write, cs (None = no cs_out, else eps_mode), Dp ('d', '128' = next multiple of 128,
# None = no dst16), t
Case = collections.namedtuple('Case', 'd n pad wd mn rw cs dp t')
ROWS_CASES = [Case(*c) for c in [
    (4, 1, 0, 0, 0.0, 0, None, None, 1),
    (4, 2, 4, 1, 1.0, 1, 0, '128', 2),
    (4, 3, 0, 1, 1.0, 0, 1, 'd', 1000),
    (4, 5, 4, 0, 0.0, 0, 0, '128', 1),
    (4, 777, 0, 1, 1.0, 1, None, 'd', 2),
    (32, 1, 4, 1, 1.0, 1, 1, '128', 1000),
    (32, 3, 0, 0, 1.0, 0, None, 'd', 1),
    (32, 5, 4, 1, 0.0, 1, 0, None, 2),
    (32, 777, 0, 0, 1.0, 1, 0, 'd', 1000),
    (96, 2, 0, 1, 1.0, 0, 0, '128', 1),
    (96, 5, 4, 0, 1.0, 1, 1, 'd', 2),
    (96, 777, 4, 1, 0.0, 0, None, '128', 1000),
    (100, 1, 0, 0, 1.0, 1, 0, '128', 2),
    (100, 3, 4, 1, 1.0, 0, 0, 'd', 1),
    (100, 5, 0, 1, 0.0, 0, 1, '128', 1000),
    (100, 777, 4, 0, 1.0, 1, 1, '128', 1),
    (256, 1, 0, 1, 0.0, 0, 0, 'd', 2),
    (256, 2, 4, 0, 1.0, 1, None, 'd', 1000),
    (256, 3, 0, 1, 1.0, 1, 1, None, 1),
    (256, 5, 0, 0, 1.0, 0, 1, 'd', 2),
    (256, 777, 0, 1, 1.0, 1, 0, 'd', 1000),
    (256, 777, 4, 0, 1.0, 0, 0, None, 1),
    (516, 1, 4, 1, 1.0, 1, 0, '128', 1),
    (516, 3, 0, 0, 0.0, 0, 1, 'd', 2),
    (516, 5, 4, 1, 1.0, 0, None, '128', 1000),
    (516, 777, 0, 0, 1.0, 1, 1, '128', 2),
    (1024, 2, 0, 0, 1.0, 1, 0, 'd', 1),
    (1024, 3, 4, 1, 0.0, 0, None, None, 2),
    (1024, 5, 0, 1, 1.0, 0, 0, 'd', 1000),
    (1024, 777, 4, 0, 1.0, 1, 1, 'd', 1),
    (1028, 1, 0, 1, 1.0, 1, 0, None, 2),
    (1028, 2, 4, 0, 0.0, 0, None, None, 1),
    (1028, 3, 0, 1, 1.0, 0, 1, None, 1000),
    (1028, 5, 4, 0, 1.0, 1, None, None, 2),
    (1028, 777, 0, 1, 1.0, 1, 1, None, 1),
    (1280, 1, 4, 0, 1.0, 0, 0, None, 1000),
    (1280, 2, 0, 1, 0.0, 1, 1, None, 1),
    (1280, 3, 0, 1, 0.0, 0, 0, None, 2),
    (1280, 5, 0, 0, 1.0, 1, 0, None, 1),
    (1280, 777, 4, 1, 1.0, 1, 0, None, 1000),
    (1280, 777, 0, 0, 1.0, 0, 1, None, 2),
]]
PROJ_CASES = [i for i, c in enumerate(ROWS_CASES) if c.cs is not None]


def case_id(c):
    return 'd%d-n%d-ld+%d-wd%d-mn%g-rw%d-cs%s-Dp%s-t%d' % c


def case_Dp(c):
    return None if c.dp is None else c.d if c.dp == 'd' else (c.d + 127) // 128 * 128


def special_rows(n):
    """(all-zero row with zero gradient, row with zero gradient but live moments) - None where n is too small to hold them
    next to an ordinary first and last row"""
    return (1 if n >= 3 else None), (n - 2 if n >= 5 else 1 if n == 2 else None)


def make_rows_inputs(c, seed=0):
    """fp32 CPU inputs of one case: row norms scattered over 0.3 .. 3 (both sides of max_norm = 1, a good part above 2)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * c.d + c.n + 13 * c.t)
    W = torch.randn(c.n, c.d, generator=g) * ((0.3 + 2.7 * torch.rand(c.n, 1, generator=g)) / c.d ** 0.5)
    G = torch.randn(c.n, c.d, generator=g) * 1e-2
    M = torch.randn(c.n, c.d, generator=g) * 3e-3
    V = (torch.randn(c.n, c.d, generator=g) * 1e-2).pow(2) * (0.2 + torch.rand(c.n, c.d, generator=g))
    zrow, grow = special_rows(c.n)
    if zrow is not None:
        W[zrow], G[zrow], M[zrow], V[zrow] = 0.0, 0.0, 0.0, 0.0
    if grow is not None:
        G[grow] = 0.0
    return dict(W=W, G=G, M=M, V=V)


def make_proj_inputs(c, seed=0, lookups=True):
    """+ the production shape of the gradient: G is the scoring gradient dE, the lookup rows (sorted distinct items with
    their position lists) are added afterwards; cs0 is this step's forward column scale (fp32)"""
    x = make_rows_inputs(c, seed)
    g = torch.Generator().manual_seed(5000 + 1000 * seed + 3 * c.d + c.n)
    x['dE'] = x.pop('G')
    x['cs0'] = cs64(x['W'], CS_SCALE, c.cs, CS_EPS).float()
    zrow, grow = special_rows(c.n)
    keep = torch.ones(c.n, dtype=torch.bool)
    for r in (zrow, grow):
        if r is not None:
            keep[r] = False
    pick = keep & (torch.rand(c.n, generator=g) < 0.5)
    pick[0] = pick[c.n - 1] = True                       # first and last row always take lookup gradients
    pick &= keep
    if not lookups or not bool(pick.any()):
        x.update(rows=None, items=None, ptr=None, pos=None, l=None, l32=None)
        return x
    items = torch.nonzero(pick).flatten().int()
    cnt = torch.randint(1, 4, (items.numel(),), generator=g)
    cnt[0] = 21                                          # one hot item: the 16-deep and the 4-deep loop of the adder
    ptr = torch.zeros(items.numel() + 1, dtype=torch.int32)
    ptr[1:] = cnt.cumsum(0).int()
    P = int(ptr[-1])
    x['rows'] = torch.randn(P, c.d, generator=g) * 5e-3
    x['items'], x['ptr'], x['pos'] = items, ptr, torch.randperm(P, generator=g).int()
    x['l'] = lookup_sum64(x['rows'], items, ptr, x['pos'], c.n, c.d)
    x['l32'] = lookup_sum64(x['rows'], items, ptr, x['pos'], c.n, c.d, torch.float32)
    return x


def rows_case_errors(c, proj=False, seed=0, lookups=True):
    """({name: oracle}, {name: fp32 restatement error}, inputs) of one case of (a) (proj False) or (b)"""
    x = make_proj_inputs(c, seed, lookups) if proj else make_rows_inputs(c, seed)
    kw = dict(use_wd=c.wd, max_norm=c.mn, renorm_write=c.rw, cs_scale=None if c.cs is None else CS_SCALE,
              eps_mode=c.cs or 0)
    if proj:
        kw.update(proj_cs=x['cs0'])
        ref = table_step64(x['W'], x['M'], x['V'], x['dE'], x['l'], ADAM, c.t, **kw)
        r32 = table_step32(x['W'], x['M'], x['V'], x['dE'], x['l32'], hyper32(ADAM, c.t), **kw)
    else:
        ref = table_step64(x['W'], x['M'], x['V'], x['G'], None, ADAM, c.t, **kw)
        r32 = table_step32(x['W'], x['M'], x['V'], x['G'], None, hyper32(ADAM, c.t), **kw)
    return ref, {k: errs(r32[k], ref[k]) for k in ref}, x
