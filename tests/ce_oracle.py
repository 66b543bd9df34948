"""float64 oracle of the fused full-catalog scoring + soft-max CE ("flash-CE": csrc/score_ce_bf16.hip, csrc/score_ce.hip),
an emulation of the bf16 kernel's rounding, the element-wise error bound, and the shared case table.

Plain torch on the CPU; nothing here imports the product.  tests/test_ce_oracle_cpu.py shows that the bound is met by the
emulation and missed by seeded wrong variants of it, tests/test_score_ce_gpu.py holds the HIP kernels to it.

What the bf16 kernels promise: the operands are rounded ONCE to bf16 (RNE), the logits, the soft-max statistics, exp and
the one-hot subtraction are fp32, P is rounded once to bf16 AFTER the one-hot subtraction, and both gradient products
accumulate in fp32.  So `exact` works in float64 on the bf16-ROUNDED operands

    z[b, v] = cs[v] <sr16_b, E16_v>        lse_b = log sum_v exp z[b, v]        loss = mean_{b < live} (lse_b - z[b, label_b])
    P[b, v] = (ga_b softmax_b[v] - gc_b [v == label_b]) cs[v]        dE = P^T sr16        dsr = P E16

(dE is d / dE_v at fixed cs: the kernels' output before the row-normalisation projection), rows b >= live contribute
nothing and get dsr = 0, a label of -1 has no one-hot and leaves the label logit as the caller set it.  Plain CE is
ga = gc = gscale / live (`plain_coef`).

Gradient bound, element-wise: the only rounding beyond fp32 is the one RNE rounding of P, unit roundoff U = 2^-8, so

    |got - exact| <= FACTOR U bound + FLOOR max|exact|,      bound_dE = |P|^T |sr16|,  bound_dsr = |P| |E16|

FACTOR = 1.25 covers the fp32 logit / exp / lse errors that can flip a rounding of P and the fp32 accumulation.
Forward: lse and the label logit to rtol 1e-5 / atol 1e-4, the loss to 1e-5 relative - the project's fp32 tolerances,
because the forward has no rounding after the operands."""
import collections
import functools
import math
import zlib

import torch

F64 = torch.float64
U = 2.0 ** -8                   # unit roundoff of bf16 (8 significant bits, round to nearest even)
FACTOR = 1.25
FLOOR = 1e-9
LSE_RTOL, LSE_ATOL, LOSS_RTOL = 1e-5, 1e-4, 1e-5
CH = 32                         # streamed rows per chunk of the bf16 kernels (what the seeded faults are phrased in)

Result = collections.namedtuple('Result', 'lse lab loss dE dsr bound_dE bound_dsr')


def bf16r(x):
    """x rounded to bf16 (RNE), as float64"""
    return torch.as_tensor(x).detach().to('cpu', torch.float32).bfloat16().to(F64)


def _d(x):
    return torch.as_tensor(x).detach().to('cpu', F64)


def plain_coef(B, live, gscale=1.0, denom=None):
    """ga = gc of plain mean CE scaled by the upstream gscale"""
    return torch.full((B,), float(gscale) / float(max(live if denom is None else denom, 1)), dtype=F64)


def exact(sr, E, cs, labels, ga, gc, live, lab_init=0.0, rounded=True, block=1024, grads=True):
    """float64 on the bf16-rounded operands (rounded=False: on the operands as given - the fp32 kernels' reference);
    walks `block` sessions at a time so that the largest case stays a few hundred MB; grads=False: forward only"""
    sr16, E16 = (bf16r(sr), bf16r(E)) if rounded else (_d(sr), _d(E))
    B, d = sr16.shape
    V = E16.shape[0]
    csd = torch.ones(V, dtype=F64) if cs is None else _d(cs)
    labels = torch.as_tensor(labels).detach().cpu().long()
    ga, gc = _d(ga), _d(gc)
    lse = torch.zeros(B, dtype=F64)
    lab = torch.full((B,), float(lab_init), dtype=F64)
    dE, bdE = torch.zeros(V, d, dtype=F64), torch.zeros(V, d, dtype=F64)
    dsr, bdsr = torch.zeros(B, d, dtype=F64), torch.zeros(B, d, dtype=F64)
    aE = E16.abs()
    for b0 in range(0, live, block):
        b1 = min(live, b0 + block)
        s = sr16[b0:b1]
        z = (s @ E16.t()) * csd
        l = torch.logsumexp(z, 1)
        lse[b0:b1] = l
        lb = labels[b0:b1]
        rows = torch.nonzero(lb >= 0)[:, 0]
        lab[b0 + rows] = z[rows, lb[rows]]
        if not grads:
            continue
        P = torch.exp(z - l[:, None]) * ga[b0:b1, None]
        P[rows, lb[rows]] -= gc[b0:b1][rows]
        P *= csd
        dE += P.t() @ s
        dsr[b0:b1] = P @ E16
        P.abs_()
        bdE += P.t() @ s.abs()
        bdsr[b0:b1] = P @ aE
    loss = float((lse[:live] - lab[:live]).sum()) / max(live, 1)
    return Result(lse, lab, loss, dE, dsr, bdE, bdsr)


FAULTS = ('item_tail_dropped', 'session_tail_dropped', 'session_zeroed', 'onehot_missing', 'onehot_at_label_plus_1',
          'ga_gc_exchanged', 'mean_over_B', 'dead_session_contributes', 'rows_exchanged_in_chunk', 'accumulate_overwrites')


def emulate(sr, E, cs, labels, ga, gc, live, lab_init=0.0, dE_prev=None, fault=None):
    """`exact` with the bf16 kernel's rounding: fp32 logits and lse, P rounded once to bf16 after the one-hot subtraction,
    fp32 products.  dE_prev: the accumulating launch (parts & 4), dE = dE_prev + this head's.  fault: one of FAULTS, a
    seeded wrong variant (the bound must catch each of them somewhere)."""
    assert fault is None or fault in FAULTS, fault
    f32 = torch.float32
    sr16, E16 = bf16r(sr).to(f32), bf16r(E).to(f32)
    B, d = sr16.shape
    V = E16.shape[0]
    csf = torch.ones(V, dtype=f32) if cs is None else torch.as_tensor(cs).detach().cpu().to(f32)
    labels = torch.as_tensor(labels).detach().cpu().long().clone()
    ga, gc = _d(ga).to(f32), _d(gc).to(f32)
    nlive = live
    if fault == 'ga_gc_exchanged':
        ga, gc = gc, ga
    if fault == 'mean_over_B':
        assert live < B
        ga, gc = ga * (live / B), gc * (live / B)
    if fault == 'dead_session_contributes':
        assert live < B
        nlive = live + 1
    s = sr16.clone()
    s[nlive:] = 0
    z = (s @ E16.t()) * csf
    lse = torch.logsumexp(z, 1)
    P = torch.exp(z - lse[:, None]) * (ga[:, None] * csf)
    lab = torch.full((B,), float(lab_init), dtype=f32)
    rows = torch.nonzero(labels[:nlive] >= 0)[:, 0]
    lab[rows] = z[rows, labels[rows]]
    hot = labels.clone()
    if fault == 'onehot_at_label_plus_1':
        hot[rows] = (hot[rows] + 1) % V
    if fault == 'onehot_missing':
        rows = rows[rows != rows[len(rows) // 2]]
    P[rows, hot[rows]] -= gc[rows] * csf[hot[rows]]
    P[nlive:] = 0
    lse[nlive:] = 0
    if fault == 'session_zeroed':
        P[nlive // 2] = 0
    if fault == 'session_tail_dropped':
        assert nlive % CH
        P[nlive // CH * CH:] = 0
    if fault == 'item_tail_dropped':
        assert V % CH
        P[:, V // CH * CH:] = 0
    P = P.bfloat16().to(f32)
    PE, PS = P, P
    if fault == 'rows_exchanged_in_chunk':           # a wrong k-order of the second product: streamed rows 5 and 9 of chunk 0
        i, j = min(5, V - 1), min(9, V - 2)
        PS = P.clone()
        PS[:, [i, j]] = P[:, [j, i]]
        i, j = min(5, nlive - 1), min(9, nlive - 2)
        PE = P.clone()
        PE[[i, j]] = P[[j, i]]
    dE = PE.t() @ s
    dsr = PS @ E16
    if dE_prev is not None and fault != 'accumulate_overwrites':
        dE = torch.as_tensor(dE_prev).detach().cpu().to(f32) + dE
    loss = float((lse[:live] - lab[:live]).double().sum()) / max(live, 1)
    return Result(lse, lab, loss, dE, dsr, None, None)


def grad_error(got, want, bound):
    """(largest |got - want| / (U bound) over the elements above the floor, number of elements outside the bound)"""
    got, want = _d(got), _d(want)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    err = (got - want).abs()
    floor = FLOOR * float(want.abs().max()) if want.numel() else 0.0
    bad = ~(err <= FACTOR * U * bound + floor)       # (a NaN in got is bad)
    over = err > floor
    ratio = float((err[over] / (U * bound[over]).clamp(min=1e-300)).max()) if bool(over.any()) else 0.0
    return ratio, int(bad.sum())


def check_grad(got, want, bound, what):
    ratio, nbad = grad_error(got, want, bound)
    assert nbad == 0, '%s: %d elements outside %.2f u bound, largest error / (u bound) = %.3g' % (what, nbad, FACTOR, ratio)
    return ratio


def check_forward(got_lse, got_lab, got_loss, ex, live, what):
    """lse and label logit of the live sessions at rtol 1e-5 / atol 1e-4, loss (None: not produced) at 1e-5 relative"""
    for name, got, want in (('lse', got_lse, ex.lse), ('label logit', got_lab, ex.lab)):
        g, w = _d(got)[:live], want[:live]
        err = (g - w).abs()
        assert bool((err <= LSE_ATOL + LSE_RTOL * w.abs()).all()), '%s %s: max abs err %.3e' % (what, name, float(err.max()))
    if got_loss is not None:
        assert math.isfinite(float(got_loss)) and abs(float(got_loss) - ex.loss) <= LOSS_RTOL * abs(ex.loss), (what, float(got_loss), ex.loss)


# ---------------------------------------------------------------------------------------------------------- the cases
Case = collections.namedtuple('Case', 'name B V d cosine labels live coef gscale logits')


def _case(name, B, V, d, cosine=False, labels='rand', live=None, coef='plain', gscale=1.0, logits=None):
    return Case(name, B, V, d, cosine, labels, live, coef, gscale, logits)


def _cases():
    cs = []
    # every template (d_pad 32 / 64 / 96 / 128 / 256), d == d_pad (vector epilogue) and d != d_pad (scalar epilogue)
    for d in (32, 64, 96, 128, 256, 4, 36, 100, 132):
        cs.append(_case('template-d%d' % d, 37, 700, d, cosine=d in (64, 128, 4, 100)))
    # tails of the streamed and of the owned side, B = 513: past the item-tile role's 512-session side block
    # (V = 1 with per-session coefficients, ga != gc: under plain CE its soft-max IS the one-hot, the exact gradient and
    #  with it the bound are identically 0, and the check would ask fp32 exp(z - lse) to be 1 to the last bit - not what the
    #  bound is about.  With ga != gc, P = (ga - gc) cs is an ordinary number and the one-item tail is checked like any other)
    for V in (1, 31, 33, 127, 129):
        cs.append(_case('tail-V%d' % V, 129, V, 32, cosine=V in (33, 129), coef='g' if V == 1 else 'plain'))
    for B in (1, 31, 33, 127, 129, 513):
        cs.append(_case('tail-B%d' % B, B, 257, 64, cosine=B in (31, 513)))
    # more than 512 items per range: the side block of the session-tile role (backward) is refilled
    cs.append(_case('refill', 4096, 4500, 32, cosine=True))
    for lab in ('edges', 'same', 'neg'):
        cs.append(_case('labels-' + lab, 129, 257, 32, labels=lab, cosine=lab == 'edges'))
    for live in (0, 1, 77, 300 - 129, 300):
        cs.append(_case('dyn-live%d' % live, 300, 257, 64, live=live))
    for d in (64, 36):
        cs.append(_case('coef-gscale-d%d' % d, 37, 700, d, gscale=3.0))
        cs.append(_case('coef-g-d%d' % d, 37, 700, d, coef='g', cosine=True))
        cs.append(_case('coef-g-gscale-d%d' % d, 37, 700, d, coef='g', gscale=3.0))
    cs.append(_case('split2', 1024, 200, 32, cosine=True))
    cs.append(_case('split2-ragged', 1100, 200, 64))
    cs.append(_case('split2-ragged-live600', 1100, 200, 64, live=600))
    cs.append(_case('split2-ragged-live500', 1100, 200, 64, live=500, coef='g'))
    # online soft-max: session 0's logits ascend / descend with the item id (every chunk of a range rescales the running
    # sum); 'dead-range': its leading items lie 160 below its maximum (exp underflows: that range's partial sum is 0)
    for lg in ('ascending', 'descending', 'dead-range'):
        cs.append(_case('online-' + lg, 4096, 2100, 32, cosine=True, logits=lg))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ONLINE_SCALE = 16.0
DEAD_RANGE_NORM = 5.0     # |sr_0| of the dead-range case: cosine logits at scale 16 span 32, a gap of 150 needs |sr| >= 4.7

Data = collections.namedtuple('Data', 'case sr E cs labels ga gc live gscale')


def make(case, seed_extra=0):
    """the inputs of a case (fp32 tensors on the CPU; labels int64, -1 = no label; ga / gc: float64 [B], what the oracle is
    given - for coef == 'plain' they are gscale / live, for 'g' signed random with exact zeros and ga != gc, NOT yet
    multiplied by gscale: the oracle gets ga * gscale)"""
    c = BY_NAME[case] if isinstance(case, str) else case
    g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + seed_extra)
    B, V, d = c.B, c.V, c.d
    sr = torch.randn(B, d, generator=g) * 0.3
    E = torch.randn(V, d, generator=g) * 0.3
    scale = ONLINE_SCALE if c.logits else 12.0
    if c.cosine:
        sr = torch.nn.functional.normalize(sr, dim=1)
    if c.logits:
        # E_v = |E_v| (cos t_v sr_0 + sin t_v w), w orthogonal to sr_0: session 0's logit of item v is scale cos t_v
        w = torch.randn(d, generator=g)
        w = torch.nn.functional.normalize(w - (w @ sr[0]) * sr[0], dim=0)
        if c.logits == 'dead-range':
            cos = torch.cat([torch.full((V // 2,), -1.0), torch.linspace(-1.0, 1.0, V - V // 2)])
            sr[0] *= DEAD_RANGE_NORM
        else:
            cos = torch.linspace(-1.0, 1.0, V)
            if c.logits == 'descending':
                cos = cos.flip(0)
        E = E.norm(dim=1, keepdim=True) * (cos[:, None] * torch.nn.functional.normalize(sr[0], dim=0) + (1 - cos * cos).clamp(min=0).sqrt()[:, None] * w)
    cs = (scale / E.norm(dim=1)).contiguous() if c.cosine else None
    labels = torch.randint(0, V, (B,), generator=g)
    if c.labels == 'edges':
        edge = torch.tensor([0, V - 1, 31, 32, 127, 128])
        labels = edge[torch.arange(B) % 6]
    elif c.labels == 'same':
        labels[:] = min(77, V - 1)
    elif c.labels == 'neg':
        labels[::3] = -1
    if c.logits:
        labels[0] = V // 3         # not the item that carries session 0's whole soft-max
    live = B if c.live is None else c.live
    if c.coef == 'plain':
        ga = gc = plain_coef(B, live, 1.0)
    else:
        ga = torch.randn(B, generator=g).to(F64) / 16
        gc = torch.randn(B, generator=g).to(F64) / 16
        ga[3 % B], gc[5 % B] = 0.0, 0.0
        ga[7 % B], gc[7 % B] = 0.0, 0.0
        ga, gc = ga.float().to(F64), gc.float().to(F64)      # what the kernel is handed: fp32 values
    return Data(c, sr, E, cs, labels, ga, gc, live, c.gscale)


@functools.lru_cache(maxsize=None)
def reference(name, seed_extra=0, rounded=True):
    """(inputs, exact result) of a case, computed once per process and shared (read-only) by the tests that need it"""
    D = make(name, seed_extra)
    return D, exact(D.sr, D.E, D.cs, D.labels, D.ga * D.gscale, D.gc * D.gscale, D.live, rounded=rounded)
