"""GPU: the item-table optimizer pass (csrc/adam.hip: adam_rows_kernel) and the kernels around it, row-wise against the
float64 oracle of tests/table_oracle.py (pinned to torch on the CPU by tests/test_table_step_oracle.py).

Every comparison covers every element and names the worst row and column; every output buffer is larger than its live extent
and sentinel-filled, and what lies past n - or past d inside a padded row stride - must keep its bits (dst16: the kernel
clears the columns d .. Dp of the live rows).  Bit-exact assertions (bf16 copy, sentinels, radial == 0, the skip identity) take
no tolerance.

Tolerances are never constants: each case evaluates the same formula in fp32 torch on the same inputs (table_oracle.
table_step32 and friends), measures that restatement against the oracle, and allows the kernel max(4 x that, 2 ulp) - in
`rel_err` (|x - ref| / (|ref| + ulp of the row's largest)) and again in `row_err` (|x - ref| / the row's largest).  Measured
fp32-restatement errors, worst over the cases (CPU, tests/test_table_step_oracle.py -s), and the bounds that follow:

    quantity   rel_err (a)  -> bound    row_err (a)  -> bound    rel_err (b)  -> bound    row_err (b)  -> bound
    W          4.8e-02       1.9e-01    1.1e-06       4.5e-06    5.3e-03       2.1e-02    6.9e-06       2.7e-05
    M          7.8e-02       3.1e-01    2.3e-07       9.2e-07    2.7e-02       1.1e-01    1.5e-07       5.9e-07
    V          1.4e-06       5.7e-06    2.3e-07       9.2e-07    2.8e-06       1.1e-05    1.2e-07       4.9e-07
    cs         4.4e-07       1.8e-06    4.4e-07       1.8e-06    3.1e-07       1.3e-06    3.1e-07       1.3e-06

(the bound applied is the case's own, these are the worst).  rel_err of W and M is large because among 777 x d elements some
cancel to ~0 (b1 m against (1 - b1) g; p against its update), where half an ulp of the row's magnitude is already 0.1 .. 0.5 in
that measure: the term is the rounding of the larger summand, the yardstick is the restatement of that same sum.  row_err is the
measure that binds ordinary elements.  In (b) W's row_err grows with the <W, G> - radial cancellation times 1 / sqrt(v) of
the smallest second moments (t = 1000 cases); again the restatement performs the same subtraction.

Branches of adam_rows_kernel and which cases of table_oracle.ROWS_CASES reach them:
    HOLD (d <= 1024) register tiles: one lane live (d 4), part of a tile (32, 96, 100), one full tile (256), tile 2 with lane 0
        only (516), all four tiles (1024); streaming path adam_rows_kernel<false> (d 1028: second trip with lane 0 only; 1280:
        five full trips), dst16 NULL as the launcher passes it
    the last n % 4 rows of the 4-rows-per-workgroup grid: n 1, 2, 3, 5 and 777 at every width (777 = 4 * 194 + 1)
    ld == d + 4 (a column slice): cases 1 3 5 7 11 13 15 17 21 22 24 27 29 31 33 35 39
    no row epilogue at all (max_norm 0, cs NULL: HOLD skips the wave sum, streaming returns early): 0 11 27 / 31
    cs without renorm (max_norm 0): 3 7 14 16 23 / 36 37;   renorm_write without max_norm (no-op): 7 / 36
    max_norm 1, renorm_write 0 - W plain, cs of the renormed row: 2 9 13 19 21 28 / 32 35 40; with cs NULL (nothing but the plain
        Adam row may show): 6 24
    max_norm 1, renorm_write 1: 1 5 8 10 12 15 18 20 22 25 26 29 / 30 34 38 39; with cs NULL: 4 17 / 33
    eps_mode 0 / 1, use_wd 0 / 1, t 1 / 2 / 1000: spread over both paths (asserted by test_case_table_covers_what_the_issue_lists)
    dst16 with Dp == d, Dp = next multiple of 128 (> d for d 4, 32, 96, 100, 516), NULL

Skip identity under renorm (test_skip_scalars_make_every_adam_kernel_the_identity): with the skip scalars {0, 1, 1, eps, 0, 0,
0, 1} the Adam arithmetic keeps every bit, but the row pass then RE-RAN its renorm epilogue: a row that the previous
renorm_write = 1 step had scaled to max_norm / (norm + 1e-7) recomputes, in fp32, to a norm an ulp above max_norm about as often
as not (always possible once norm >= 2, where norm + 1e-7 == norm) and was scaled again - parameters changed bits under
skip, against include/srec.h.  Measured on an MI355X with the kernel as it was: "W changed bits in 9 rows, first row 211" of
777 at renorm_write 1.  The kernel now leaves the renorm write out when the scalars are the identity's, and the test passes.

The rel measure's absolute minimum (table_oracle.check: 2 ulp of the row's largest magnitude per element) - figures of the run
without it, 85 of 89 tests passing in 4.2 s, the four misses all at elements that cancel to ~1e-6 .. 1e-5 of their summands:
    rows d1280 n5:   W 2.07e-05 against 4 x 4.91e-06;   proj d1028 n1: M 2.40e-04 against 4 x 5.53e-05
    proj d1280 n3:   G 2.44e-04 against 4 x 3.06e-05;   adam_multi tensor of 3 elements: m 3.23e-06 against the 2.38e-07 floor
every one of them an absolute error below one ulp of the row's largest magnitude, and all inside the row-scaled bound.
"""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import table_oracle as O

pytestmark = pytest.mark.gpu

SENT = 77.25
F32 = torch.float32


def _L():
    return importlib.import_module('sessionrec-pytorch_amd._lib')


def _padded(live, ld, dev, extra=3, fill=SENT):
    """[n + extra, ld] sentinel-filled device buffer with `live` in [:n, :d]"""
    n, d = live.shape
    buf = torch.full((n + extra, ld), fill, dtype=live.dtype, device=dev)
    buf[:n, :d] = live.to(dev)
    return buf


def _vec(live, dev, extra=3, fill=SENT):
    buf = torch.full((live.numel() + extra,), fill, dtype=live.dtype, device=dev)
    buf[:live.numel()] = live.to(dev)
    return buf


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _outside_kept(after, before, n, d, what):
    """everything outside [:n, :d] keeps its bits"""
    mask = torch.ones(after.shape, dtype=torch.bool, device=after.device)
    if after.dim() == 2:
        mask[:n, :d] = False
    else:
        mask[:n] = False
    assert torch.equal(_bits(after)[mask], _bits(before)[mask]), what + ': written outside the live extent'


def _run_rows_case(dev, c, proj, mode='alias', seed=0):
    L = _L()
    lookups = mode != 'noradial'
    ref, e32, x = O.rows_case_errors(c, proj, seed, lookups)
    n, d, ld = c.n, c.d, c.d + c.pad
    Dp = O.case_Dp(c)
    W, M, V = (_padded(x[k], ld, dev) for k in 'WMV')
    G = _padded(x['dE'] if proj else x['G'], ld, dev)
    h = O.hyper32(O.ADAM, c.t).to(dev)
    cs_buf = None
    if c.cs is not None:
        cs_buf = _vec(x['cs0'], dev) if (proj and mode != 'distinct') else torch.full((n + 3,), SENT, device=dev)
    dst16 = torch.full((n + 3, Dp), 7.0, dtype=torch.bfloat16, device=dev) if Dp is not None else None
    before = {k: t.clone() for k, t in (('W', W), ('M', M), ('V', V), ('cs', cs_buf), ('dst16', dst16)) if t is not None}
    common = (L.ptr(W), L.ptr(G), L.ptr(M), L.ptr(V), n, d, ld, L.ptr(h), c.wd, c.mn, c.rw, L.ptr(cs_buf), O.CS_SCALE,
              c.cs or 0, O.CS_EPS)
    what = ('proj ' if proj else 'rows ') + mode + ' ' + O.case_id(c)
    if proj:
        radial = None
        if lookups:
            radial = torch.full((n + 5,), 3.5, device=dev)
            radial[:n] = 0.0
            if x['rows'] is not None:
                rows, items, ptr_, pos = (x[k].to(dev) for k in ('rows', 'items', 'ptr', 'pos'))
                L.lib.srec_scatter_add_sorted_ex(L.ptr(rows), d, L.ptr(items), L.ptr(ptr_), L.ptr(pos), L.ptr(G), ld,
                                                 items.numel(), None, d, 1, 0.0, 0, None, 0, L.ptr(W), ld, L.ptr(radial),
                                                 L.stream())
                # the producer of `radial`: the summed buffer and the side sums against the oracle's
                G64 = x['dE'].double() + x['l']
                l32 = x['l32']
                O.check('G', G[:n, :d], G64, O.errs(x['dE'] + l32, G64), what)
                r64 = (x['W'].double() * x['l']).sum(1)
                e_r = (x['W'] * l32).sum(1)
                scale = (x['W'].double().abs() * x['l'].abs()).sum(1).clamp(min=1e-30)      # the summands' size
                got_r = radial[:n].double().cpu()
                lim = max(4.0 * float(((e_r.double() - r64).abs() / scale).max()), 2 * O.ULP)
                bad = ((got_r - r64).abs() / scale)
                assert float(bad.max()) <= lim, '%s radial: row %d off by %.3e of its summands (bound %.3e)' % (
                    what, int(bad.argmax()), float(bad.max()), lim)
                assert bool((radial[n:] == 3.5).all())
        proj_cs = cs_buf if mode != 'distinct' else _vec(x['cs0'], dev)
        proj_before = proj_cs.clone()
        L.lib.srec_adam_rows_proj(*common, L.ptr(proj_cs), O.INV_SCALE, L.ptr(radial), L.ptr(dst16), Dp or 0, L.stream())
        if radial is not None:
            assert bool((radial[:n] == 0).all()) and not bool(torch.signbit(radial[:n]).any()), what + ': radial not cleared'
            assert bool((radial[n:] == 3.5).all()), what + ': radial written past n'
        if mode == 'distinct':
            assert torch.equal(_bits(proj_cs), _bits(proj_before)), what + ': proj_cs is an input'
    else:
        L.lib.srec_adam_rows(*common, L.ptr(dst16), Dp or 0, L.stream())
    torch.cuda.synchronize()
    for k, buf in (('W', W), ('M', M), ('V', V)):
        O.check(k, buf[:n, :d], ref[k], e32[k], what)
        _outside_kept(buf, before[k], n, d, what + ' ' + k)
    if c.cs is not None:
        O.check('cs', cs_buf[:n], ref['cs'], e32['cs'], what)
        _outside_kept(cs_buf, before['cs'], n, 1, what + ' cs')
    zrow, grow = O.special_rows(n)
    if zrow is not None:
        assert float(W[zrow, :d].abs().max()) == 0.0 and float(M[zrow, :d].abs().max()) == 0.0 \
            and float(V[zrow, :d].abs().max()) == 0.0, what + ': the all-zero row moved'
        if c.cs is not None:
            assert float(cs_buf[zrow]) == O.CS_SCALE / O.CS_EPS, (what, float(cs_buf[zrow]))
    if dst16 is not None:
        assert torch.equal(_bits(dst16[:n]), _bits(O.bf16_copy(W[:n, :d].contiguous(), Dp))), \
            what + ': dst16 is not the RNE rounding of W as written (zeros in d .. Dp)'
        _outside_kept(dst16, before['dst16'], n, Dp, what + ' dst16')


@pytest.mark.parametrize('i', range(len(O.ROWS_CASES)), ids=[O.case_id(c) for c in O.ROWS_CASES])
def test_adam_rows_single_step(dev, i):
    """(a) srec_adam_rows, one step from the kernel's own fp32 inputs (branch list: module docstring)"""
    _run_rows_case(dev, O.ROWS_CASES[i], proj=False)


PROJ_PARAMS = [(i, 'alias') for i in O.PROJ_CASES] + [(20, 'distinct'), (34, 'distinct'), (20, 'noradial'), (39, 'noradial')]


@pytest.mark.parametrize('i,mode', PROJ_PARAMS, ids=['%s-%s' % (O.case_id(O.ROWS_CASES[i]), m) for i, m in PROJ_PARAMS])
def test_adam_rows_proj_single_step(dev, i, mode):
    """(b) srec_adam_rows_proj: G = scoring gradient + lookup rows added by srec_scatter_add_sorted_ex (projW = W, so the
    kernel under test produces radial); oracle adam(project64(dE) + l).  alias: proj_cs and cs_out are ONE array, as the
    optimizer passes them (a kernel that read proj_cs after writing cs_out would project with the next step's scale: cs changes
    by the renorm and by the step, the error is of first order); distinct: two arrays, proj_cs untouched; noradial: radial NULL."""
    _run_rows_case(dev, O.ROWS_CASES[i], proj=True, mode=mode)


@pytest.mark.parametrize('d', [32, 100, 256, 1028])
def test_row_kernels_against_the_oracle(dev, d):
    """(c) srec_rownorm_project, srec_rownorm_project_radial, srec_row_invnorm, srec_renorm_rows (idx list + device-side count)"""
    L = _L()
    n = 777
    c = O.Case(d, n, 4, 0, 1.0, 0, 0, None, 1)
    x = O.make_proj_inputs(c, seed=3)
    Wc, dE, cs0 = x['W'], x['dE'], x['cs0']
    ld_w, ld_g = d + 4, d + 8
    W = _padded(Wc, ld_w, dev)
    Wb = W.clone()
    cs = _vec(cs0, dev)
    # plain projection
    G = _padded(dE, ld_g, dev)
    Gb = G.clone()
    L.lib.srec_rownorm_project(L.ptr(W), ld_w, L.ptr(cs), O.INV_SCALE, L.ptr(G), ld_g, n, d, L.stream())
    ref = O.project64(Wc, cs0, O.INV_SCALE, dE)
    O.check('G', G[:n, :d], ref, O.errs(O.project32(Wc, cs0, O.INV_SCALE, dE), ref), 'rownorm_project d%d' % d)
    _outside_kept(G, Gb, n, d, 'rownorm_project G')
    assert torch.equal(_bits(W), _bits(Wb))
    # deferred form: the oracle is fed the buffer and the side sums the kernel reads
    l32 = x['l32']
    Gs = dE + l32
    rad = ((Wc.double() * x['l']).sum(1)).float()
    G = _padded(Gs, ld_g, dev)
    Gb = G.clone()
    radial = torch.full((n + 5,), 3.5, device=dev)
    radial[:n] = rad.to(dev)
    L.lib.srec_rownorm_project_radial(L.ptr(W), ld_w, L.ptr(cs), O.INV_SCALE, L.ptr(G), ld_g, n, d, L.ptr(radial), L.stream())
    iv = (cs0.double() * O.INV_SCALE).unsqueeze(1)
    ref = Gs.double() - Wc.double() * (((Wc.double() * Gs.double()).sum(1) - rad.double()).unsqueeze(1) * iv * iv)
    O.check('G', G[:n, :d], ref, O.errs(O.project32(Wc, cs0, O.INV_SCALE, Gs, rad), ref), 'rownorm_project_radial d%d' % d)
    _outside_kept(G, Gb, n, d, 'rownorm_project_radial G')
    assert bool((radial[:n] == 0).all()) and bool((radial[n:] == 3.5).all())
    # 1 / norm
    for eps_mode in (0, 1):
        out = torch.full((n + 3,), SENT, device=dev)
        L.lib.srec_row_invnorm(L.ptr(W), ld_w, n, d, eps_mode, O.CS_EPS, O.CS_SCALE, L.ptr(out), L.stream())
        ref = O.cs64(Wc, O.CS_SCALE, eps_mode, O.CS_EPS)
        O.check('cs', out[:n], ref, O.errs(O.cs32(Wc, O.CS_SCALE, eps_mode, O.CS_EPS), ref), 'row_invnorm d%d mode %d' % (d, eps_mode))
        assert bool((out[n:] == SENT).all())
        zrow, _ = O.special_rows(n)
        assert float(out[zrow]) == O.CS_SCALE / O.CS_EPS
    # renorm of listed rows only, *dyn < n_cap
    g = torch.Generator().manual_seed(d)
    mid = 1 + torch.randperm(n - 2, generator=g)[:298].int()       # distinct, as include/srec.h requires: a row listed twice
    idx = torch.cat([torch.tensor([n - 1, 0], dtype=torch.int32), mid])      # would be rescaled twice, or not, by a race
    assert idx.unique().numel() == 300
    live = 211
    dyn = torch.tensor([live], dtype=torch.int32, device=dev)
    L.lib.srec_renorm_rows(L.ptr(W), ld_w, L.ptr(idx.to(dev)), 300, L.ptr(dyn), d, 1.0, L.stream())
    sel = idx[:live].long()
    assert float(Wc[sel].norm(dim=1).max()) > 1.0 > float(Wc[sel].norm(dim=1).min())
    ref = O.renorm64(Wc[sel], 1.0)
    O.check('W', W[:n, :d][sel.to(dev)], ref, O.errs(O.renorm32(Wc[sel], 1.0), ref), 'renorm_rows d%d' % d)
    rest = torch.ones(n + 3, dtype=torch.bool)
    rest[sel] = False
    assert torch.equal(_bits(W[rest.to(dev)]), _bits(Wb[rest.to(dev)])), 'rows not listed, or listed past *dyn, keep their bits'
    _outside_kept(W, Wb, n, d, 'renorm_rows W')
    assert float(W[:n, :d].norm(dim=1)[sel.to(dev)].max()) <= 1.0 + 4 * O.ULP


def test_adam_rows_proj_trajectory(dev):
    """(d) 20 consecutive steps of (b) at d 256, n 777: fresh gradients drawn directly each step, lr dropped after step 10,
    max_norm 1, renorm_write 1, cs aliased, step scalars from srec_adam_hyper - against table_step64 iterated in float64 from the
    same start; the bound is 4 x the error of the fp32 restatement iterated the same way (the only place error accumulates)."""
    L = _L()
    n, d, Dp, steps = 777, 256, 256, 20
    c = O.Case(d, n, 0, 1, 1.0, 1, 0, 'd', 1)
    x0 = O.make_proj_inputs(c, seed=9)
    hp = dict(O.ADAM, wd=1e-2)
    W, M, V = (_padded(t, d, dev) for t in (x0['W'], torch.zeros(n, d), torch.zeros(n, d)))
    cs = _vec(x0['cs0'], dev)
    dst16 = torch.full((n + 3, Dp), 7.0, dtype=torch.bfloat16, device=dev)
    radial = torch.full((n + 5,), 3.5, device=dev)
    radial[:n] = 0.0
    before = dict(W=W.clone(), M=M.clone(), V=V.clone(), cs=cs.clone(), dst16=dst16.clone())
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    cfg = torch.zeros(5, dtype=torch.float64, device=dev)
    hyper = torch.zeros(8, device=dev)
    s64 = dict(W=x0['W'].double(), M=torch.zeros(n, d, dtype=O.F64), V=torch.zeros(n, d, dtype=O.F64), cs=x0['cs0'].double())
    s32 = dict(W=x0['W'].clone(), M=torch.zeros(n, d), V=torch.zeros(n, d), cs=x0['cs0'].clone())
    kw = dict(use_wd=1, max_norm=1.0, renorm_write=1, cs_scale=O.CS_SCALE, eps_mode=0)
    for t in range(1, steps + 1):
        hp['lr'] = 3e-3 if t <= 10 else 3e-4
        cfg.copy_(torch.tensor([hp['lr'], hp['b1'], hp['b2'], hp['eps'], hp['wd']], dtype=torch.float64))
        y = O.make_proj_inputs(c, seed=100 + t)                    # only its gradient parts are used
        G = _padded(y['dE'], d, dev)
        rows, items, ptr_, pos = (y[k].to(dev) for k in ('rows', 'items', 'ptr', 'pos'))
        L.lib.srec_adam_hyper(L.ptr(counter), L.ptr(cfg), L.ptr(hyper), L.stream())
        L.lib.srec_scatter_add_sorted_ex(L.ptr(rows), d, L.ptr(items), L.ptr(ptr_), L.ptr(pos), L.ptr(G), d, items.numel(), None,
                                         d, 1, 0.0, 0, None, 0, L.ptr(W), d, L.ptr(radial), L.stream())
        L.lib.srec_adam_rows_proj(L.ptr(W), L.ptr(G), L.ptr(M), L.ptr(V), n, d, d, L.ptr(hyper), 1, 1.0, 1, L.ptr(cs), O.CS_SCALE,
                                  0, O.CS_EPS, L.ptr(cs), O.INV_SCALE, L.ptr(radial), L.ptr(dst16), Dp, L.stream())
        s64 = O.table_step64(s64['W'], s64['M'], s64['V'], y['dE'], y['l'], hp, t, proj_cs=s64['cs'], **kw)
        s32 = O.table_step32(s32['W'], s32['M'], s32['V'], y['dE'], y['l32'], O.hyper32(hp, t), proj_cs=s32['cs'], **kw)
    torch.cuda.synchronize()
    assert int(counter) == steps
    for k, buf in (('W', W[:n]), ('M', M[:n]), ('V', V[:n]), ('cs', cs[:n])):
        O.check(k, buf, s64[k], O.errs(s32[k], s64[k]), 'trajectory')
    assert torch.equal(_bits(dst16[:n]), _bits(O.bf16_copy(W[:n].contiguous(), Dp)))
    assert bool((radial[:n] == 0).all()) and bool((radial[n:] == 3.5).all())
    for k, buf in (('W', W), ('M', M), ('V', V), ('cs', cs), ('dst16', dst16)):
        _outside_kept(buf, before[k], n, buf.shape[1] if buf.dim() == 2 else 1, 'trajectory ' + k)
    assert float(W[:n].norm(dim=1).max()) <= 1.0 + 4 * O.ULP


# ------------------------------------------------------------------------------------------------------- (e) step scalars
def _f32(x):
    return float(np.float32(x))


def _assert_hyper(got, cfg, t, what):
    """hyper[0..7] = the float32 rounding of the Python-double values; 1 ulp allowed on the two entries that go through the
    device's double pow(), which is not correctly rounded (the others are conversions and one subtraction: exact)"""
    want = O.hyper_host(*cfg, t)
    got = [float(v) for v in got.cpu()]
    for k in range(8):
        w = np.float32(want[k])
        tol = float(np.spacing(np.abs(w))) if k in (0, 7) else 0.0
        assert abs(got[k] - float(w)) <= tol, '%s: hyper[%d] = %r, want %r (t = %d)' % (what, k, got[k], float(w), t)


@pytest.mark.parametrize('start', [0, 1, 999, 10 ** 6])
def test_adam_hyper_scalars(dev, start):
    L = _L()
    cfgv = (3e-3, 0.9, 0.999, 1e-8, 1e-4)
    counter = torch.full((3,), 55, dtype=torch.int32, device=dev)
    counter[0] = start
    cfg = torch.tensor(cfgv, dtype=torch.float64, device=dev)
    hyper = torch.full((10,), SENT, device=dev)
    for k in range(1, 4):
        L.lib.srec_adam_hyper(L.ptr(counter), L.ptr(cfg), L.ptr(hyper), L.stream())
        assert counter.tolist() == [start + k, 55, 55]
        _assert_hyper(hyper[:8], cfgv, start + k, 'adam_hyper')
        assert hyper[8:].tolist() == [SENT, SENT]
    if start == 10 ** 6:
        assert float(hyper[7]) == 1.0 and float(hyper[0]) == _f32(3e-3)      # b2^t underflows, b1^t is gone


def _slots(dev, n, starts):
    cfgs = [(1e-3 * (k + 1), 0.9 - 0.01 * k, 0.999 - 0.0005 * k, 1e-8 * (k + 1), 1e-4 * k) for k in range(n)]
    counters = [torch.tensor([s], dtype=torch.int32, device=dev) for s in starts]
    cfg = [torch.tensor(cf, dtype=torch.float64, device=dev) for cf in cfgs]
    hyper = [torch.full((8,), SENT, device=dev) for _ in range(n)]
    arr = ctypes.c_void_p * n
    host = tuple(arr(*[t.data_ptr() for t in ts]) for ts in (counters, cfg, hyper))
    return cfgs, counters, cfg, hyper, host


def test_adam_hyper_multi_slots_tap_and_skip(dev):
    """16 slots with different cfg and counters in ONE launch, each checked on its own; the loss tap owned by slot 5 (not slot 0
    of the call) writes a ring of 5 over 12 calls; then skip: counters advance, the tapped slot reads NaN, the scalars are the
    identity's"""
    L = _L()
    n, own, ring_n = 16, 5, 5
    starts = [0, 1, 999, 10 ** 6, 7, 3] + [11 * k for k in range(6, 16)]
    cfgs, counters, cfg, hyper, host = _slots(dev, n, starts)
    src = torch.zeros(1, device=dev)
    ring = torch.full((ring_n + 2,), SENT, device=dev)
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    shadow = [SENT] * (ring_n + 2)
    addr = [ctypes.addressof(h) for h in host]
    for call in range(1, 13):
        src.fill_(call + 0.5)
        L.lib.srec_adam_hyper_multi(n, addr[0], addr[1], addr[2], L.ptr(counters[own]), L.ptr(src), L.ptr(ring), ring_n,
                                    L.ptr(skip), L.stream())
        for k in range(n):
            assert int(counters[k]) == starts[k] + call, (k, call)
            _assert_hyper(hyper[k], cfgs[k], starts[k] + call, 'slot %d call %d' % (k, call))
        t = starts[own] + call
        shadow[(t - 1) % ring_n] = call + 0.5
        assert ring.tolist() == shadow, (call, ring.tolist(), shadow)
    skip.fill_(1)
    src.fill_(99.0)
    L.lib.srec_adam_hyper_multi(n, addr[0], addr[1], addr[2], L.ptr(counters[own]), L.ptr(src), L.ptr(ring), ring_n, L.ptr(skip),
                                L.stream())
    t = starts[own] + 13
    got = ring.tolist()
    assert math.isnan(got[(t - 1) % ring_n])
    assert [v for k, v in enumerate(got) if k != (t - 1) % ring_n] == [v for k, v in enumerate(shadow) if k != (t - 1) % ring_n]
    for k in range(n):
        assert int(counters[k]) == starts[k] + 13
        assert hyper[k].tolist() == [0.0, 1.0, 1.0, _f32(cfgs[k][3]), 0.0, 0.0, 0.0, 1.0], (k, hyper[k].tolist())
    # no tap: nothing but counters and scalars is written
    skip.fill_(0)
    L.lib.srec_adam_hyper_multi(n, addr[0], addr[1], addr[2], None, None, None, 0, None, L.stream())
    assert [math.isnan(v) or v for v in ring.tolist()] == [math.isnan(v) or v for v in got]
    _assert_hyper(hyper[2], cfgs[2], starts[2] + 14, 'after skip')


def _multi_desc(tensors, use_wd):
    optim = importlib.import_module('sessionrec-pytorch_amd.optim')
    nt = len(tensors)
    arr = ctypes.c_void_p * nt
    keep = [(ctypes.c_int * nt)(*use_wd), (ctypes.c_long * nt)(*[t[0].numel() for t in tensors])]
    keep += [arr(*[t[k].data_ptr() for t in tensors]) for k in range(4)]
    desc = optim._AdamMultiDesc(nt, *[ctypes.addressof(a) for a in keep])
    return desc, keep


def test_skip_scalars_make_every_adam_kernel_the_identity(dev):
    """include/srec.h: with the skip scalars 'parameters and moments keep their bits' - srec_adam_flat, srec_adam_multi, and
    srec_adam_rows with both renorm_write values on a table that a previous, non-skipped renorm_write = 1 step has just written
    (rows whose fp32 norm recomputes an ulp above max_norm are the suspects), rows with v == 0 included"""
    L = _L()
    n, d = 777, 256
    c = O.Case(d, n, 4, 0, 1.0, 1, 0, 'd', 1)
    x = O.make_rows_inputs(c, seed=5)
    still = [3, 400, n - 1]                                        # rows no step has moved: zero gradient, zero moments
    for r in still:
        x['G'][r], x['M'][r], x['V'][r] = 0.0, 0.0, 0.0
    x['W'][400] *= 2.5 / x['W'][400].norm()                        # one of them far above max_norm
    ld = d + c.pad
    W, G, M, V = (_padded(x[k], ld, dev) for k in 'WGMV')
    cs = torch.full((n + 3,), SENT, device=dev)
    dst16 = torch.full((n + 3, d), 7.0, dtype=torch.bfloat16, device=dev)
    cfgs, counters, cfg, hyper, host = _slots(dev, 2, [4, 9])
    addr = [ctypes.addressof(h) for h in host]
    skip = torch.zeros(1, dtype=torch.int32, device=dev)

    def scalars():
        L.lib.srec_adam_hyper_multi(2, addr[0], addr[1], addr[2], None, None, None, 0, L.ptr(skip), L.stream())

    def rows(renorm_write):
        L.lib.srec_adam_rows(L.ptr(W), L.ptr(G), L.ptr(M), L.ptr(V), n, d, ld, L.ptr(hyper[0]), 0, 1.0, renorm_write, L.ptr(cs),
                             O.CS_SCALE, 0, O.CS_EPS, L.ptr(dst16), d, L.stream())

    scalars()
    rows(1)                                                        # the live step: every row above 1 is renormed and written
    assert float(V[still, :d].abs().max()) == 0.0 and float(W[:n, :d].norm(dim=1).max()) <= 1.0 + 4 * O.ULP
    assert int((x['W'].norm(dim=1) >= 2.0).sum()) > 50
    skip.fill_(1)
    scalars()
    assert hyper[0].tolist() == [0.0, 1.0, 1.0, _f32(cfgs[0][3]), 0.0, 0.0, 0.0, 1.0]
    G[:n, :d] = torch.randn(n, d, generator=torch.Generator().manual_seed(1)).to(dev)      # a stale batch's gradient
    for renorm_write in (1, 0):
        kept = [t.clone() for t in (W, M, V)]
        c16 = dst16.clone()
        rows(renorm_write)
        for name, a, b in zip('WMV', (W, M, V), kept):
            diff = (_bits(a) != _bits(b)).any(1)
            assert not bool(diff.any()), 'srec_adam_rows renorm_write %d under skip: %s changed bits in %d rows, first row %d' % (
                renorm_write, name, int(diff.sum()), int(diff.nonzero()[0]))
        assert torch.equal(_bits(dst16), _bits(c16)), 'the operand copy of an unchanged table is unchanged'
    # flat and multi-tensor kernels with the same scalars
    gen = torch.Generator().manual_seed(2)
    sizes = [5, 4096, 4097, 70001]
    ts = []
    for k, sz in enumerate(sizes):
        p, g, m = (torch.randn(sz, generator=gen).to(dev) for _ in range(3))
        v = torch.rand(sz, generator=gen).to(dev) * 1e-4
        v[::7], m[::7] = 0.0, 0.0
        ts.append((p, g, m, v))
    kept = [[t.clone() for t in tup] for tup in ts]
    desc, keep = _multi_desc(ts, [1, 0, 1, 1])
    L.lib.srec_adam_multi(ctypes.addressof(desc), L.ptr(hyper[1]), L.stream())
    big = tuple(torch.cat([t[k] for t in ts] + [ts[0][k][:3]]).clone() for k in range(4))      # 16-byte aligned, n % 4 == 2
    kept_big = [t.clone() for t in big]
    L.lib.srec_adam_flat(L.ptr(big[0]), L.ptr(big[1]), L.ptr(big[2]), L.ptr(big[3]), big[0].numel(), L.ptr(hyper[1]), 1, L.stream())
    torch.cuda.synchronize()
    for tup, kp in zip(ts + [big], kept + [kept_big]):
        for name, a, b in zip('pgmv', tup, kp):
            assert torch.equal(_bits(a), _bits(b)), 'skip: %s of a tensor of %d changed bits' % (name, a.numel())


def test_adam_multi_across_launches(dev):
    """(f) 200 tensors = three launches of MT = 88: sizes mixing 1, 3, 4095, 4096, 4097 and a few of ~70 000, use_wd without a
    period and differing across 63/64 (the words of wd_mask), 87/88 and 175/176 (the launches), one tensor per launch with
    4-byte-only alignment; 3 steps against adam_step64 per tensor.  weight_decay 0.1: a tensor decayed against its flag has m off
    by wd p / |g|, up to 40 % (p itself from the second step on; the first Adam step is sign(g) lr whatever the decay).

    Inputs: |p| <= 0.02 and gradients drawn directly with |g| in 0.005 .. 0.015 and a random sign, so that g + wd p (|wd p| <=
    0.003 over the three steps) never cancels.  With Gaussian p ~ 0.1 and g ~ 0.01 about one of the 600 000 elements has g + wd p
    cancel to ~1e-7, near the size of eps: there the first step lr g / (|g| + eps) turns on the last bits of the product wd p, two
    fp32 evaluation orders differ by 1e-6 of the row's magnitude, and a restatement that rounds the other way measures nothing
    of it (MI355X, those inputs: tensor 69, where g + wd p = 6e-8 at step 1, p row-scaled 3.295e-07 against 4 x 8.185e-08) - the
    comparison then tests the inputs' conditioning, not the kernel."""
    L = _L()
    nt = 200
    gen = torch.Generator().manual_seed(11)
    small = [1, 3, 4095, 4096, 4097]
    sizes = [small[k % 5] for k in range(nt)]
    for k, s in ((5, 70001), (90, 69999), (180, 70000), (199, 65537)):
        sizes[k] = s
    use_wd = torch.randint(0, 2, (nt,), generator=gen).tolist()
    for a in (63, 87, 175):
        use_wd[a + 1] = 1 - use_wd[a]
    assert len({tuple(use_wd[k:k + 24]) for k in (0, 64, 88, 128, 176)}) == 5      # no shift by a word or a launch maps it to itself
    unaligned = (10, 100, 190)
    hp = dict(O.ADAM)
    ts, cpu = [], []
    for k, sz in enumerate(sizes):
        p = (2.0 * torch.rand(sz, generator=gen) - 1.0) * 0.02
        if k in unaligned:
            base = [torch.full((sz + 1,), SENT, device=dev) for _ in range(3)]
            tup = tuple(b[1:] for b in base)
            assert all(t.data_ptr() % 16 == 4 for t in tup)
        else:
            tup = tuple(torch.empty(sz, device=dev) for _ in range(3))
        tup[0].copy_(p)
        tup[1].zero_()
        tup[2].zero_()
        ts.append(tup)
        cpu.append(dict(p64=p.double(), m64=torch.zeros(sz, dtype=O.F64), v64=torch.zeros(sz, dtype=O.F64),
                        p32=p.clone(), m32=torch.zeros(sz), v32=torch.zeros(sz)))
    grads = [torch.empty(sz, device=dev) for sz in sizes]
    full = [(ts[k][0], grads[k], ts[k][1], ts[k][2]) for k in range(nt)]
    desc, keep = _multi_desc(full, use_wd)
    for t in range(1, 4):
        hp['lr'] = 3e-3 if t < 3 else 1e-3
        h32 = O.hyper32(hp, t)
        h = h32.to(dev)
        for k in range(nt):
            g = (0.5 + torch.rand(sizes[k], generator=gen)) * 1e-2 * (2 * torch.randint(0, 2, (sizes[k],), generator=gen) - 1)
            grads[k].copy_(g)
            s = cpu[k]
            s['p64'], s['m64'], s['v64'] = O.adam_step64(s['p64'], g, s['m64'], s['v64'], hp['lr'], hp['b1'], hp['b2'], hp['eps'],
                                                         hp['wd'] if use_wd[k] else 0.0, t)
            s['p32'], s['m32'], s['v32'] = O.adam_step32(s['p32'], g, s['m32'], s['v32'], h32, use_wd[k])
        L.lib.srec_adam_multi(ctypes.addressof(desc), L.ptr(h), L.stream())
        torch.cuda.synchronize()
    for k in range(nt):
        s = cpu[k]
        for name, got, a64, a32 in (('p', ts[k][0], s['p64'], s['p32']), ('m', ts[k][1], s['m64'], s['m32']),
                                    ('v', ts[k][2], s['v64'], s['v32'])):
            O.check(name, got.unsqueeze(0), a64.unsqueeze(0), O.errs(a32.unsqueeze(0), a64.unsqueeze(0)),
                    'adam_multi tensor %d (n %d, wd %d)' % (k, sizes[k], use_wd[k]))
        if k in unaligned:
            assert all(float(t._base[0]) == SENT for t in ts[k])
