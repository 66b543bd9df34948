"""GPU: the fused scoring / CE kernels element-wise against the float64 oracle of tests/ce_oracle.py.

bf16 kernels (csrc/score_ce_bf16.hip, always with ops.TableBF16(E).refresh(E)): lse, label logit and loss at the project's
fp32 tolerances, dE and dsr element-wise inside 1.25 u bound (u = 2^-8: the one rounding of P) - on every template, both
epilogues, both workgroup roles' tails and side-block refills, the session-split slab path with ragged / empty pieces, the
three ways of passing the coefficients, accumulation into an existing dE, dynB, labels of -1, strided dE and single parts.
Where the launch plan decides the path, the plan is asserted (split value, chunks per range, epilogue).
fp32 kernels (csrc/score_ce.hip): the same rows for ga / gc, gscale with ga / gc, accumulation, labels of -1 and strided dE
against a float64 run of the unrounded operands, row-wise 1e-4."""
import ctypes
import importlib

import pytest
import torch

import ce_oracle as O

pytestmark = pytest.mark.gpu


def _ops():
    return importlib.import_module('sessionrec-pytorch_amd.ops')


# ------------------------------------------------------------------ the launch plan, restated (csrc/score_ce_bf16.hip)
OWN, CH, SB = 128, 32, 512                  # owner rows per workgroup, streamed rows per chunk, rows per side block
XCDS, XCD_SLOTS, FWD_SLOTS, FWD_RMAX, BWD_RMAX = 8, 64, 512, 1024, 64


def _cdiv(a, b):
    return (a + b - 1) // b


def _dpad(d):
    return 32 if d <= 32 else 64 if d <= 64 else 96 if d <= 96 else 128 if d <= 128 else 256


def _plan_fwd(B, V):
    """(ranges, chunks per range) of the forward"""
    T, chunks = _cdiv(B, OWN), _cdiv(V, CH)
    R = max(1, min(FWD_SLOTS // T, FWD_RMAX, chunks))
    cpr = _cdiv(chunks, R)
    return _cdiv(chunks, cpr), cpr


def _plan_bwd(B, V, with_de, split=1):
    """(ranges, chunks per range) of the backward's session-tile role"""
    T, chunks, de_tiles = _cdiv(B, OWN), _cdiv(V, CH), _cdiv(V, OWN) * split
    rx = []
    for x in range(XCDS):
        free = XCD_SLOTS
        if with_de:
            cnt = (de_tiles - x + XCDS - 1) // XCDS if x < de_tiles else 0
            if cnt % XCD_SLOTS:
                free = XCD_SLOTS - cnt % XCD_SLOTS
        rx.append(free // T)
    if sum(rx) == 0:
        rx = [1] * XCDS
    total = min(sum(rx), BWD_RMAX, chunks)
    cpr = _cdiv(chunks, total)
    return _cdiv(chunks, cpr), cpr


def _de_split(B, V, d):
    sp = ctypes.c_int(0)
    _ops().lib.srec_ce_de_split(B, V, d, ctypes.addressof(sp))
    return sp.value


def _plan_checked(B, V, d):
    """the restated plan agrees with what the library reports for this shape -> (fwd, bwd with dE at the split taken)"""
    nt, nr, dp = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _ops().lib.srec_ce_plan_bf16(B, V, d, ctypes.addressof(nt), ctypes.addressof(nr), ctypes.addressof(dp))
    split = _de_split(B, V, d)
    fwd, bwd = _plan_fwd(B, V), _plan_bwd(B, V, True, split)
    assert dp.value == _dpad(d) and nt.value == fwd[0], (nt.value, fwd, dp.value)
    assert nr.value == max(_plan_bwd(B, V, True)[0], _plan_bwd(B, V, False)[0], bwd[0]), (nr.value, bwd)
    return fwd, bwd


def _epilogue(d, ld, t):
    """which epilogue of the bf16 backward stores into a [rows, d] view of leading dimension ld"""
    return 'vector' if d == _dpad(d) and ld % 4 == 0 and t.data_ptr() % 16 == 0 else 'scalar'


# ------------------------------------------------------------------------------------------------------- the runners
class Run:
    pass


def _setup(dev, D, bf16, E=None, ws=None):
    ops = _ops()
    r = Run()
    r.D, r.B, r.V, r.d = D, D.case.B, D.case.V, D.case.d
    r.sr = D.sr.to(dev)
    r.E = D.E.to(dev) if E is None else E
    r.cs = None if D.cs is None else D.cs.to(dev)
    r.labels = D.labels.to(dev).int()
    r.dyn = None if D.case.live is None else torch.tensor([D.live], dtype=torch.int32, device=dev)
    r.ws = ops.CEWorkspace(r.B, r.V, r.d, dev) if ws is None else ws
    r.tb = ops.TableBF16(r.E).refresh(r.E) if bf16 else None
    if bf16:
        assert r.tb.E16.shape[1] == _dpad(r.d) and r.ws.sr16.shape == (r.ws.Bp, _dpad(r.d))
    r.ga = (D.ga * 1.0).float().to(dev)
    r.gc = (D.gc * 1.0).float().to(dev)
    return r


def _run_ce(dev, D, bf16=True):
    """plain mean CE through ops.ScoreCE; the upstream gradient of the loss is D.gscale"""
    ops = _ops()
    r = _setup(dev, D, bf16)
    r.tg = ops.TableGrad(r.E)
    r.tg.buf.fill_(7.0)                                   # (must be overwritten)
    srg = r.sr.clone().requires_grad_()
    r.loss, r.lse = ops.ScoreCE.apply(srg, r.E, r.cs, r.labels, r.ws, r.tg, r.dyn, 0.0, r.tb)
    (r.loss * D.gscale).backward()
    r.lab, r.dE, r.dsr, r.loss = r.ws.lab_logit.clone(), r.tg.buf, srg.grad, r.loss.item()
    return r


def _run_stats(dev, D, bf16=True, tg=None, E=None, ws=None):
    """per-session coefficients through ops.ScoreStats: objective sum_b ga_b lse_b - gc_b z[b, label_b]"""
    ops = _ops()
    assert D.gscale == 1.0
    r = _setup(dev, D, bf16, E, ws)
    r.tg = ops.TableGrad(r.E) if tg is None else tg
    if tg is None:
        r.tg.buf.fill_(7.0)
    srg = r.sr.clone().requires_grad_()
    lse, lab = ops.ScoreStats.apply(srg, r.E, r.cs, r.labels, r.ws, r.tg, r.dyn, 0.0, r.tb)
    ((r.ga * lse).sum() - (r.gc * lab).sum()).backward()
    r.lse, r.lab, r.loss, r.dE, r.dsr = lse.detach(), lab.detach(), None, r.tg.buf, srg.grad
    return r


def _run_direct(dev, D, bf16=True, parts=3, dE=None, dsr=None, lab_init=0.0, coef=None):
    """ops._ce_fwd / ops._ce_bwd with caller-owned buffers: gscale by pointer, with or without ga / gc"""
    ops = _ops()
    r = _setup(dev, D, bf16)
    B, V, d = r.B, r.V, r.d
    r.lse = torch.empty(B, device=dev)
    lossvec, loss = torch.empty(B, device=dev), torch.empty((), device=dev)
    r.lab = torch.full((B,), lab_init, device=dev)
    ops._ce_fwd(r.sr, r.E, r.cs, r.labels, r.ws, r.dyn, r.tb, r.lab, r.lse, lossvec, loss)
    coef = D.case.coef if coef is None else coef
    gl = torch.tensor([D.gscale], device=dev) if (coef == 'plain' or D.gscale != 1.0) else None
    r.dE = torch.full((V, d), 7.0, device=dev) if dE is None else dE
    r.dsr = torch.full((B, d), 7.0, device=dev) if dsr is None else dsr
    if parts:
        ops._ce_bwd(r.sr, r.E, r.cs, r.labels, r.lse, gl, r.ga if coef == 'g' else None, r.gc if coef == 'g' else None,
                    r.ws, r.dyn, r.tb, r.dE, r.dsr, parts)
    r.loss = loss.item()
    return r


def _check_rows32(got, want, what):
    """the fp32 kernels: 1e-4 relative per row plus close()'s floor (2e-6 of the tensor's largest magnitude)"""
    got, want = got.detach().double().cpu(), want
    err, ref = (got - want).abs().amax(1), want.abs().amax(1)
    floor = 2e-6 * float(want.abs().max())
    bad = ~(err <= 1e-4 * ref + floor)
    assert not bool(bad.any()), '%s: %d rows out, worst row error %.3e (row max %.3e)' % (
        what, int(bad.sum()), float(err[bad].max()), float(ref[bad][err[bad].argmax()]))


def _check(r, ex, what, bf16=True, dE_want=None, dE_bound=None, outputs=('dE', 'dsr')):
    D = r.D
    O.check_forward(r.lse, r.lab, r.loss, ex, D.live, what)
    assert bool(torch.isfinite(r.dE).all()) and bool(torch.isfinite(r.dsr).all()), what
    dE_want = ex.dE if dE_want is None else dE_want
    dE_bound = ex.bound_dE if dE_bound is None else dE_bound
    ratios = {}
    if bf16:
        if 'dE' in outputs:
            ratios['dE'] = O.check_grad(r.dE, dE_want, dE_bound, what + ' dE')
        if 'dsr' in outputs:
            ratios['dsr'] = O.check_grad(r.dsr, ex.dsr, ex.bound_dsr, what + ' dsr')
        print('RATIO %s: error / (u bound) %s' % (what, ' '.join('%s %.3f' % kv for kv in ratios.items())))
    else:
        if 'dE' in outputs:
            _check_rows32(r.dE, dE_want, what + ' dE (fp32)')
        if 'dsr' in outputs:
            _check_rows32(r.dsr, ex.dsr, what + ' dsr (fp32)')
    if 'dsr' in outputs:
        assert not bool(r.dsr[D.live:].any()), what + ': dsr of a session beyond the live count'
    return ratios


def _run_case(dev, D, bf16=True):
    if D.case.coef == 'plain':
        return _run_ce(dev, D, bf16)
    if D.gscale == 1.0:
        return _run_stats(dev, D, bf16)
    return _run_direct(dev, D, bf16)


# --------------------------------------------------------------------------------------------------------- the tests
SCALAR_NT = {4: 1, 36: 2, 100: 4, 132: 8}


@pytest.mark.parametrize('name', [c.name for c in O.CASES])
def test_bf16_case_against_the_oracle(dev, name):
    D, ex = O.reference(name)
    c = D.case
    B, V, d = c.B, c.V, c.d
    r = _run_case(dev, D)
    fwd, bwd = _plan_checked(B, V, d)
    split = _de_split(B, V, d)
    # the path this case is here for was taken
    if name.startswith('template'):
        assert _epilogue(d, r.dE.stride(0), r.dE) == ('scalar' if d in SCALAR_NT else 'vector')
        assert d not in SCALAR_NT or _dpad(d) // 32 == SCALAR_NT[d]
    if name.startswith('coef'):
        assert _epilogue(d, r.dE.stride(0), r.dE) == ('scalar' if d == 36 else 'vector')
    if name == 'refill':
        assert bwd[1] * CH > SB and split > 1, (bwd, split)
    if name == 'tail-B513':
        assert B > SB and split == 1
    if name.startswith('split2'):
        assert split == 2 and _epilogue(d, r.dE.stride(0), r.dE) == 'vector'
        (sp, slabs), = r.ws._de.values()
        assert sp == 2 and slabs.numel() == 2 * V * d
        de_per = _cdiv(_cdiv(B, 2), CH) * CH
        if 'ragged' in name:
            assert de_per * 2 != B and 500 < de_per < 600
    elif c.coef == 'plain' or c.gscale == 1.0:
        assert split == 1 or all(sp == split for sp, _ in r.ws._de.values())
    if c.logits:
        assert fwd[1] >= 2, fwd                           # several chunks per forward range: the running sum rescales
        z0 = (O.bf16r(D.E) @ O.bf16r(D.sr)[0]) * D.cs.double()
        cm = z0[:V // CH * CH].reshape(-1, CH).amax(1)
        if c.logits == 'ascending':
            assert bool((cm[1:] > cm[:-1]).all())
        elif c.logits == 'descending':
            assert bool((cm[1:] < cm[:-1]).all())
        else:
            assert float(z0[:fwd[1] * CH].max()) < float(z0.max()) - 150.0
    _check(r, ex, name)
    if c.labels == 'neg':
        assert bool((r.lab[D.labels.to(dev) < 0] == 0).all())
    if D.live == 0:
        assert not bool(r.dE.any()) and not bool(r.dsr.any())


def test_forward_side_block_refill(dev):
    """more than 512 items per forward range (the forward's side block of column scales is refilled): the smallest V at
    B = 4096 for which the plan says so; forward only"""
    B, d = 4096, 32
    V = next(v for v in range(4500, 20000) if _plan_fwd(B, v)[1] * CH > SB)
    fwd, _ = _plan_checked(B, V, d)
    assert fwd[1] * CH > SB and _plan_fwd(B, V - 1)[1] * CH <= SB
    D = O.make(O.Case('fwd-refill', B, V, d, True, 'rand', None, 'plain', 1.0, None))
    ex = O.exact(D.sr, D.E, D.cs, D.labels, D.ga, D.gc, D.live, grads=False)
    r = _run_direct(dev, D, parts=0)
    O.check_forward(r.lse, r.lab, r.loss, ex, D.live, 'fwd-refill V=%d' % V)


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
def test_label_minus_one_leaves_the_label_logit_alone(dev, bf16):
    D = O.make('labels-neg')
    ex = O.exact(D.sr, D.E, D.cs, D.labels, D.ga, D.gc, D.live, lab_init=-7.5, rounded=bf16)
    r = _run_direct(dev, D, bf16, lab_init=-7.5)
    none = D.labels.to(dev) < 0
    assert int(none.sum()) > 40 and bool((r.lab[none] == -7.5).all())
    _check(r, ex, 'labels-neg, preset label logit', bf16)


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('name', ['coef-g-d64', 'coef-g-d36', 'split2', 'split2-ragged-live600', 'split2-ragged-live500'])
def test_two_heads_accumulate_into_one_table_gradient(dev, name, bf16):
    """two ops.ScoreStats heads on one TableGrad: the first backward overwrites what the buffer held, the second adds
    (parts | 4) - vector epilogue, scalar epilogue, and the session-split path (de_reduce_kernel with acc = 1)"""
    ops = _ops()
    D1 = O.make(name)._replace(gscale=1.0)
    D2 = O.make(name, seed_extra=1)._replace(E=D1.E, cs=D1.cs, gscale=1.0)
    e1, e2 = (O.exact(D.sr, D.E, D.cs, D.labels, D.ga, D.gc, D.live, rounded=bf16) for D in (D1, D2))
    c = D1.case
    want_split = 2 if name.startswith('split2') and bf16 else 1
    if bf16:
        assert _de_split(c.B, c.V, c.d) == want_split
    r1 = _run_stats(dev, D1, bf16)
    assert not bool((r1.dE == 7.0).any())
    _check(r1, e1, name + ' head 1', bf16)
    assert r1.tg.fresh
    r2 = _run_stats(dev, D2, bf16, tg=r1.tg, E=r1.E, ws=r1.ws)
    _check(r2, e2, name + ' head 1 + 2', bf16, dE_want=e1.dE + e2.dE, dE_bound=e1.bound_dE + e2.bound_dE)
    if bf16:
        assert [sp for sp, _ in r1.ws._de.values()] == [want_split]
        assert _epilogue(c.d, r2.dE.stride(0), r2.dE) == ('scalar' if c.d == 36 else 'vector')


@pytest.mark.parametrize('bf16', [True, False], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('name,pad', [('split2', 4), ('split2', 1), ('coef-g-gscale-d36', 4), ('coef-g-d64', 1)])
def test_strided_dE(dev, name, pad, bf16):
    """dE as a column-slice view [V, d] of a [V, d + pad] buffer through ops._ce_bwd: pad 4 keeps the vector epilogue
    (where d is its own padding), pad 1 takes the scalar one, a split shape falls back to one piece; the columns outside
    the view stay as they were.  Once overwriting, once accumulating."""
    D, _ = O.reference(name)
    ex = O.exact(D.sr, D.E, D.cs, D.labels, D.ga * D.gscale, D.gc * D.gscale, D.live, rounded=bf16)
    c = D.case
    buf = torch.full((c.V, c.d + pad), 9.0, device=dev)
    view = buf[:, :c.d]
    assert _epilogue(c.d, view.stride(0), view) == ('vector' if pad == 4 and c.d == _dpad(c.d) else 'scalar')
    r = _run_direct(dev, D, bf16, dE=view)
    assert not r.ws._de                                   # (no slab workspace: the split path was not taken)
    assert bool((buf[:, c.d:] == 9.0).all())
    _check(r, ex, '%s ld_de = d + %d' % (name, pad), bf16)
    r = _run_direct(dev, D, bf16, dE=view, parts=3 | 4)
    assert bool((buf[:, c.d:] == 9.0).all())
    _check(r, ex, '%s ld_de = d + %d, accumulated' % (name, pad), bf16, dE_want=2 * ex.dE, dE_bound=2 * ex.bound_dE)


@pytest.mark.parametrize('name', ['template-d36', 'split2', 'coef-g-d64'])
@pytest.mark.parametrize('parts', [1, 2])
def test_single_parts_leave_the_other_output_alone(dev, name, parts):
    D, ex = O.reference(name)
    r = _run_direct(dev, D, parts=parts)
    if parts == 1:
        assert bool((r.dsr == 7.0).all())
        r.dsr.zero_()
        _check(r, ex, name + ' parts = 1', outputs=('dE',))
        if name == 'split2':
            assert [sp for sp, _ in r.ws._de.values()] == [2]
    else:
        assert bool((r.dE == 7.0).all()) and not r.ws._de
        r.dE.zero_()
        _check(r, ex, name + ' parts = 2', outputs=('dsr',))


@pytest.mark.parametrize('name', ['coef-g-d64', 'coef-g-d36', 'coef-g-gscale-d64', 'coef-g-gscale-d36', 'coef-gscale-d36',
                                  'labels-neg', 'dyn-live77'])
def test_fp32_kernels_row_wise(dev, name):
    """csrc/score_ce.hip (tb = None, unrounded operands) against a float64 run: ga / gc, gscale with ga / gc, labels of -1"""
    D, ex = O.reference(name, rounded=False)
    _check(_run_case(dev, D, bf16=False), ex, name + ' fp32', bf16=False)
