"""GPU: the tail of the training step - the second level of the lookup gradient summed by the optimizer's row pass
(srec_scatter_add_sorted_stamp + srec_adam_rows_lookup instead of srec_scatter_add_sorted_ex + srec_adam_rows_proj) and the
row pass and the multi-tensor Adam launch as ONE launch (srec_adam_rows_multi).

Both are re-arrangements of launches, not of arithmetic: every comparison against the two-launch sequence is BIT-exact (no
tolerance anywhere in this file except the one oracle comparison, which takes table_oracle's rule).  The float64 oracle
comparison is there because bit-equality with a wrong parent would prove nothing.

Shapes of the kernel-level fold test, the smallest at which each branch can go wrong: 301 table rows (the last workgroup of 4
rows is partial); d 64 (one float4 per lane, idle lanes), 96 (ragged last float4 group, with a padded row stride), 256 (the
benchmark's), 1028 (the streaming body); 37 touched items including rows 0 and 300 with piece counts 1 3 4 5 16 17 40 (the
issue's: every tail of a 16 / 4 / 1 loop) and 8 9 13 (the row pass keeps 8 loads in flight, not 16: its own tails); a slot list
of capacity 48 with 38 live entries, one of them items[u] = -1, and padded entries that name a valid row which must not be
stamped.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import table_oracle as O
from util import pkg, reseed

pytestmark = pytest.mark.gpu

F32 = torch.float32
NROWS = 301
COUNTS = [1, 3, 4, 5, 16, 17, 40, 8, 9, 13]


def _L():
    return importlib.import_module('sessionrec-pytorch_amd._lib')


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b, what):
    diff = _bits(a) != _bits(b)
    assert not bool(diff.any()), '%s: %d elements differ in their bits, first at flat index %d' % (
        what, int(diff.sum()), int(diff.flatten().nonzero()[0]))


_LOOKUP = {}


def _lookup_case(d):
    """(items [48], cptr [49], dyn_u, positions rows g [P, d], chunk_ptr [C + 1], pos [P]) on the CPU, built once per width"""
    if d in _LOOKUP:
        return _LOOKUP[d]
    gen = torch.Generator().manual_seed(40 + d)
    cand = torch.tensor([r for r in range(1, NROWS - 1) if r != 5])
    touched = torch.cat([torch.tensor([0, NROWS - 1]), cand[torch.randperm(cand.numel(), generator=gen)[:35]]]).sort().values
    assert touched.numel() == 37 and int(touched[0]) == 0 and int(touched[-1]) == NROWS - 1 and 5 not in touched.tolist()
    u_cap, live = 48, 38
    items = torch.full((u_cap,), 5, dtype=torch.int32)           # padded entries name a valid row: it must not be stamped
    items[:10] = touched[:10].int()
    items[10] = -1                                               # a row owned by another shard
    items[11:live] = touched[10:].int()
    counts = [COUNTS[k % len(COUNTS)] for k in range(live)]
    counts[0], counts[live - 1] = 40, 17                         # rows 0 and 300: the deep loop and its tails
    cptr = torch.zeros(u_cap + 1, dtype=torch.int32)
    cptr[1:live + 1] = torch.tensor(counts).cumsum(0).int()
    cptr[live + 1:] = cptr[live]                                 # padded slots: empty segments
    C = int(cptr[live]) + 3                                      # a few padded chunks behind the live ones
    sizes = torch.randint(1, 17, (C,), generator=gen)
    sizes[int(cptr[live]):] = 0
    chunk_ptr = torch.zeros(C + 1, dtype=torch.int32)
    chunk_ptr[1:] = sizes.cumsum(0).int()
    P = int(chunk_ptr[-1])
    g = torch.randn(P, d, generator=gen) * 2e-3
    pos = torch.randperm(P, generator=gen).int()
    _LOOKUP[d] = dict(items=items, cptr=cptr, live=live, u_cap=u_cap, C=C, chunk_ptr=chunk_ptr, g=g, pos=pos, touched=touched)
    return _LOOKUP[d]


def _stamped_part(dev, d, slot):
    """first level through both entry points: the same `part`, and the stamps"""
    L = _L()
    k = _lookup_case(d)
    g, pos, chunk_ptr, items = (k[n].to(dev) for n in ('g', 'pos', 'chunk_ptr', 'items'))
    C = k['C']
    ar = torch.arange(C + 1, dtype=torch.int32, device=dev)
    dyn_u = torch.tensor([k['live']], dtype=torch.int32, device=dev)
    part_a = torch.full((C, d), 9.0, device=dev)
    part_b = torch.full((C, d), 9.0, device=dev)
    L.lib.srec_scatter_add_sorted(L.ptr(g), d, L.ptr(ar), L.ptr(chunk_ptr), L.ptr(pos), L.ptr(part_a), d, C, None, d, 0, L.stream())
    L.lib.srec_scatter_add_sorted_stamp(L.ptr(g), d, L.ptr(ar), L.ptr(chunk_ptr), L.ptr(pos), L.ptr(part_b), d, C, None, d, 0,
                                        0.0, 0, None, 0, L.ptr(items), k['u_cap'], L.ptr(dyn_u), L.ptr(slot), L.stream())
    _same(part_a, part_b, 'first level d%d' % d)
    want = torch.zeros(slot.numel(), dtype=torch.int32)
    for u in range(k['live']):
        if int(k['items'][u]) >= 0:
            want[int(k['items'][u])] = u + 1
    assert torch.equal(slot.cpu(), want), 'stamps d%d' % d
    assert int(want[5]) == 0 and int((want != 0).sum()) == 37
    return part_b, items, k['cptr'].to(dev), ar, dyn_u


def _fold_case(dev, d, proj, mn, oracle=False):
    L = _L()
    pad = 4 if d == 96 else 0
    ld = d + pad
    c = O.Case(d, NROWS, pad, 1, mn, 1 if mn > 0 else 0, 0, '128' if d <= 1024 else None, 2)
    x = O.make_rows_inputs(c, seed=21)
    cs0 = O.cs64(x['W'], O.CS_SCALE, 0, O.CS_EPS).float()
    Dp = O.case_Dp(c)
    h = O.hyper32(O.ADAM, c.t).to(dev)
    k = _lookup_case(d)
    slot = torch.zeros(NROWS + 3, dtype=torch.int32, device=dev)
    part, items, cptr, ar, dyn_u = _stamped_part(dev, d, slot[:NROWS])
    runs = {}
    for name in ('two', 'one'):
        W, G, M, V = (torch.full((NROWS + 3, ld), 77.25, device=dev) for _ in range(4))
        for buf, key in ((W, 'W'), (G, 'G'), (M, 'M'), (V, 'V')):
            buf[:NROWS, :d] = x[key].to(dev)
        cs = torch.full((NROWS + 3,), 77.25, device=dev)
        cs[:NROWS] = cs0.to(dev)
        radial = None
        if proj:
            radial = torch.full((NROWS + 5,), 3.5, device=dev)
            radial[:NROWS] = 0.0
        dst16 = torch.full((NROWS + 3, Dp), 7.0, dtype=torch.bfloat16, device=dev) if Dp is not None else None
        common = (L.ptr(W), L.ptr(G), L.ptr(M), L.ptr(V), NROWS, d, ld, L.ptr(h), c.wd, c.mn, c.rw, L.ptr(cs), O.CS_SCALE, 0,
                  O.CS_EPS)
        if name == 'two':
            L.lib.srec_scatter_add_sorted_ex(L.ptr(part), d, L.ptr(items), L.ptr(cptr), L.ptr(ar), L.ptr(G), ld, k['u_cap'],
                                             L.ptr(dyn_u), d, 1, 0.0, 0, None, 0, L.ptr(W) if proj else None, ld, L.ptr(radial),
                                             L.stream())
            if proj:
                L.lib.srec_adam_rows_proj(*common, L.ptr(cs), O.INV_SCALE, L.ptr(radial), L.ptr(dst16), Dp or 0, L.stream())
            else:
                L.lib.srec_adam_rows(*common, L.ptr(dst16), Dp or 0, L.stream())
        else:
            G0 = G.clone()
            L.lib.srec_adam_rows_lookup(*common, L.ptr(cs) if proj else None, O.INV_SCALE, L.ptr(radial), L.ptr(dst16), Dp or 0,
                                        L.ptr(slot), L.ptr(part), L.ptr(cptr), k['u_cap'], k['C'], L.stream())
            _same(G, G0, 'the folded pass leaves the gradient buffer as it was')
            assert int(slot.abs().max()) == 0, 'stamps not cleared'
        runs[name] = dict(W=W, M=M, V=V, cs=cs, radial=radial, dst16=dst16)
    torch.cuda.synchronize()
    what = 'fold d%d proj%d mn%g' % (d, proj, mn)
    for key in ('W', 'M', 'V', 'cs', 'radial', 'dst16'):
        if runs['two'][key] is not None:
            _same(runs['one'][key], runs['two'][key], what + ' ' + key)
    if proj:
        assert bool((runs['one']['radial'][:NROWS] == 0).all()) and bool((runs['one']['radial'][NROWS:] == 3.5).all())
    # the touched rows did take their lookup sums (a fold that summed nothing would still equal a parent given no pieces)
    if oracle:
        l64 = torch.zeros(NROWS, d, dtype=O.F64)
        l32 = torch.zeros(NROWS, d)
        pc = part.cpu()
        for u in range(k['live']):
            it = int(k['items'][u])
            if it >= 0:
                seg = pc[int(k['cptr'][u]):int(k['cptr'][u + 1])]
                l64[it] = seg.double().sum(0)
                l32[it] = seg.sum(0)
        kw = dict(use_wd=c.wd, max_norm=c.mn, renorm_write=c.rw, cs_scale=O.CS_SCALE, eps_mode=0, proj_cs=cs0 if proj else None)
        ref = O.table_step64(x['W'], x['M'], x['V'], x['G'], l64, O.ADAM, c.t, **kw)
        r32 = O.table_step32(x['W'], x['M'], x['V'], x['G'], l32, O.hyper32(O.ADAM, c.t), **kw)
        for key in ('W', 'M', 'V', 'cs'):
            got = runs['one'][key]
            got = got[:NROWS, :d] if got.dim() == 2 else got[:NROWS]
            O.check(key, got, ref[key], O.errs(r32[key], ref[key]), what)


@pytest.mark.parametrize('mn', [0.0, 1.0])
@pytest.mark.parametrize('proj', [1, 0])
@pytest.mark.parametrize('d', [64, 96, 256, 1028])
def test_row_pass_sums_the_lookup_pieces_bit_identically(dev, d, proj, mn):
    """1. srec_scatter_add_sorted_ex (second level) + srec_adam_rows_proj / srec_adam_rows against srec_adam_rows_lookup on the
    same inputs: W, M, V, cs, radial, the bf16 copy bit-identical, slot all zero afterwards, sentinels behind the live extent
    included in the comparison (whole buffers are compared)"""
    _fold_case(dev, d, bool(proj), mn)


def test_folded_row_pass_against_the_float64_oracle(dev):
    _fold_case(dev, 256, True, 1.0, oracle=True)


# ----------------------------------------------------------------------------------------------------- 2. one optimizer launch
def _multi_desc(tensors, use_wd):
    optim = pkg('optim')
    nt = len(tensors)
    arr = ctypes.c_void_p * nt
    keep = [(ctypes.c_int * nt)(*use_wd), (ctypes.c_long * nt)(*[t[0].numel() for t in tensors])]
    keep += [arr(*[t[k].data_ptr() for t in tensors]) for k in range(4)]
    desc = optim._AdamMultiDesc(nt, *[ctypes.addressof(a) for a in keep])
    return desc, keep


@pytest.mark.parametrize('d', [256, 1028])
@pytest.mark.parametrize('lookup', [0, 1])
def test_rows_and_multi_in_one_launch_equal_two_launches(dev, d, lookup):
    """2. srec_adam_rows_multi (ROWS + MULTI workgroup ranges of one launch) against srec_adam_rows_proj / _lookup followed by
    srec_adam_multi: tensors of 1, 3 (4-byte aligned only: the scalar path), 4096, 4097 and 10 000 elements, decayed and
    undecayed ones mixed (the two merged groups), a hyper block per role - every buffer bit-identical"""
    L = _L()
    c = O.Case(d, NROWS, 0, 1, 1.0, 1, 0, '128' if d <= 1024 else None, 3)
    x = O.make_rows_inputs(c, seed=22)
    cs0 = O.cs64(x['W'], O.CS_SCALE, 0, O.CS_EPS).float()
    Dp = O.case_Dp(c)
    h_rows = O.hyper32(O.ADAM, 3).to(dev)
    h_multi = O.hyper32(dict(O.ADAM, lr=1e-2, wd=0.05, b1=0.8), 7).to(dev)
    k = _lookup_case(d)
    gen = torch.Generator().manual_seed(77)
    sizes, use_wd = [1, 3, 4096, 4097, 10000, 4096], [1, 0, 1, 0, 1, 0]
    init = [tuple(torch.randn(sz, generator=gen) * s for s in (0.1, 0.01, 3e-3)) + (torch.rand(sz, generator=gen) * 1e-4,) for sz in sizes]
    runs = {}
    for name in ('two', 'one'):
        slot = torch.zeros(NROWS, dtype=torch.int32, device=dev)
        part, items, cptr, ar, dyn_u = _stamped_part(dev, d, slot)
        W, G, M, V = (x[key].to(dev).clone() for key in 'WGMV')
        cs = cs0.to(dev).clone()
        radial = torch.zeros(NROWS, device=dev)
        dst16 = torch.full((NROWS, Dp), 7.0, dtype=torch.bfloat16, device=dev) if Dp is not None else None
        ts = []
        for j, tup in enumerate(init):
            if sizes[j] == 3:                                     # 4-byte aligned only
                base = [torch.zeros(4, device=dev) for _ in range(4)]
                dt = tuple(b[1:] for b in base)
                assert all(t.data_ptr() % 16 == 4 for t in dt)
            else:
                dt = tuple(torch.empty(sizes[j], device=dev) for _ in range(4))
            for a, b in zip(dt, tup):
                a.copy_(b)
            ts.append(dt)
        desc, keep = _multi_desc(ts, use_wd)
        rows_args = (L.ptr(W), L.ptr(G), L.ptr(M), L.ptr(V), NROWS, d, d, L.ptr(h_rows), 1, 1.0, 1, L.ptr(cs), O.CS_SCALE, 0,
                     O.CS_EPS, L.ptr(cs), O.INV_SCALE, L.ptr(radial), L.ptr(dst16), Dp or 0)
        lk = (L.ptr(slot), L.ptr(part), L.ptr(cptr), k['u_cap'], k['C']) if lookup else (None, None, None, 0, 0)
        if not lookup:                                            # the second level as a launch in both runs
            L.lib.srec_scatter_add_sorted_ex(L.ptr(part), d, L.ptr(items), L.ptr(cptr), L.ptr(ar), L.ptr(G), d, k['u_cap'],
                                             L.ptr(dyn_u), d, 1, 0.0, 0, None, 0, L.ptr(W), d, L.ptr(radial), L.stream())
        if name == 'two':
            if lookup:
                L.lib.srec_adam_rows_lookup(*rows_args, *lk, L.stream())
            else:
                L.lib.srec_adam_rows_proj(*rows_args, L.stream())
            L.lib.srec_adam_multi(ctypes.addressof(desc), L.ptr(h_multi), L.stream())
        else:
            L.lib.srec_adam_rows_multi(*rows_args, *lk, ctypes.addressof(desc), L.ptr(h_multi), L.stream())
        torch.cuda.synchronize()
        runs[name] = dict(W=W, M=M, V=V, cs=cs, radial=radial, dst16=dst16, slot=slot if lookup else None, ts=ts)
    what = 'one launch d%d lookup%d' % (d, lookup)
    for key in ('W', 'M', 'V', 'cs', 'radial', 'dst16', 'slot'):
        if runs['two'][key] is not None:
            _same(runs['one'][key], runs['two'][key], what + ' ' + key)
    for j, (a, b) in enumerate(zip(runs['one']['ts'], runs['two']['ts'])):
        for nm, u, v in zip('pgmv', a, b):
            _same(u, v, '%s tensor %d (%d elements) %s' % (what, j, sizes[j], nm))
        assert not torch.equal(a[0].cpu(), init[j][0]), 'tensor %d did not step' % j
    assert not torch.equal(runs['one']['W'].cpu(), x['W'])


# ------------------------------------------------------------------------------------------------------------ 3. step level
def _samples(rng, n, V, max_len=12):
    out = []
    for _ in range(n):
        Ls = int(rng.integers(1, max_len))
        seq = rng.integers(0, V, size=Ls).tolist()
        if Ls > 1 and rng.random() < 0.3:
            seq[1] = seq[0]
        out.append((seq, int(rng.integers(0, V))))
    return out


def _model(dev, V, d, dropout):
    sp, c = pkg(), pkg('collate')
    torch.manual_seed(1)
    model = sp.MSGIFSR(V, 'x', d, 1, dropout=dropout, order=2, extra=False, fusion=False).to(dev)
    return model, (lambda caps: c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), 2, caps=caps))


SWITCHES = [('0', '0'), ('1', '0'), ('0', '1'), ('1', '1')]


@pytest.mark.parametrize('pdrop', [0.0, 0.1])
def test_captured_step_is_bit_identical_under_both_switches(dev, pdrop, monkeypatch):
    """3. MSGIFSR (d 64, order 2, B 32, V 300) captured, six replays, under the four combinations of SREC_LOOKUP_IN_ROWPASS
    and SREC_ADAM_ONE_LAUNCH: parameters, moments, losses and step counters bit-identical; with both on the captured step has
    two kernel nodes less"""
    c, train, optim, G = pkg('collate'), pkg('train'), pkg('optim'), pkg('graph')
    V = 300
    caps = c.default_caps(32, 12)
    runs = {}
    for sw in SWITCHES:
        monkeypatch.setenv('SREC_LOOKUP_IN_ROWPASS', sw[0])
        monkeypatch.setenv('SREC_ADAM_ONE_LAUNCH', sw[1])
        rng = np.random.default_rng(9)
        model, mk = _model(dev, V, 64, pdrop)
        reseed(5)
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model, fuse_projection=True)
        model.train()
        padded = [mk(caps)(_samples(rng, n, V)) for n in (32, 32, 20, 32, 27, 32)]
        x0, l0 = padded[0]
        step = G.GraphedTrainStep(model, opt, [x.to(dev) for x in x0], l0.to(dev))
        losses = [step([x.to(dev) for x in xs], lab.to(dev)).item() for xs, lab in padded]
        step.check()
        nodes = step.node_counts()
        tg = model._state(1)['tgrad']
        assert tg.slot is not None and int(tg.slot.abs().max()) == 0 and tg.lookup is None and not tg.slot_dirty
        runs[sw] = (losses, {k: p.detach().clone() for k, p in model.named_parameters()},
                    {k: (opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone()) for k, p in model.named_parameters()
                     if 'exp_avg' in opt.state[p]},
                    int(opt._hyper[(0, 0)]['counter'].item()), nodes['kernel'] if nodes else None)
    base = runs[('0', '0')]
    assert base[3] == 6
    for sw in SWITCHES[1:]:
        r = runs[sw]
        assert r[0] == base[0] and r[3] == base[3], sw
        for k in base[1]:
            _same(r[1][k], base[1][k], '%s parameter %s' % (sw, k))
        for k in base[2]:
            _same(r[2][k][0], base[2][k][0], '%s exp_avg %s' % (sw, k))
            _same(r[2][k][1], base[2][k][1], '%s exp_avg_sq %s' % (sw, k))
    n = {sw: runs[sw][4] for sw in SWITCHES}
    print('kernel nodes of the captured step by (lookup in row pass, one launch):', n)
    if n[('0', '0')] is not None:
        assert n[('1', '0')] == n[('0', '0')] - 1 and n[('0', '1')] == n[('0', '0')] - 1, n
        assert n[('1', '1')] == n[('0', '0')] - 2, n


# -------------------------------------------------------------------------------------------------------------- 4. contract
def _eager(dev, monkeypatch, switch, script):
    c, train, optim = pkg('collate'), pkg('train'), pkg('optim')
    monkeypatch.setenv('SREC_LOOKUP_IN_ROWPASS', switch)
    V = 300
    rng = np.random.default_rng(4)
    model, mk = _model(dev, V, 64, 0.0)
    reseed(6)
    opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model, fuse_projection=True)
    model.train()
    batches = [mk(None)(_samples(rng, 32, V)) for _ in range(3)]

    def backward(i):
        (mg,), lab = batches[i]
        loss = model.fused_loss(mg.to(dev), lab.to(dev))
        loss.backward()
        return loss
    tg = lambda: model._state(1)['tgrad']
    out = script(model, opt, backward, tg)
    torch.cuda.synchronize()
    t = tg()
    assert int(t.slot.abs().max()) == 0 and t.lookup is None and not t.slot_dirty, 'stamps left behind'
    return out, {k: p.detach().clone() for k, p in model.named_parameters()}


def test_backward_then_materialize_gives_the_parent_gradient(dev, monkeypatch):
    """4a. a reader other than the row pass: the recorded lookup goes through the second-level launch after all"""
    def script(model, opt, backward, tg):
        opt.zero_grad()
        backward(0)
        handed = tg().lookup is not None
        return handed, model.table_grad.buf.clone()
    (h1, g1), _ = _eager(dev, monkeypatch, '1', script)
    (h0, g0), _ = _eager(dev, monkeypatch, '0', script)
    assert h1 and not h0
    _same(g1, g0, 'materialised table gradient')
    assert float(g1.abs().max()) > 0


def test_two_backwards_and_a_reset_before_the_step(dev, monkeypatch):
    """4b. two backwards before one step (the second scoring backward overwrites the buffer: the first lookup is dropped with the
    contents it belonged to), and a reset() between a backward and the step (the step then has no table gradient): stamps all
    zero, parameters those of the two-launch path"""
    def two(model, opt, backward, tg):
        opt.zero_grad()
        backward(0)
        backward(1)
        opt.step()
        opt.zero_grad()
        backward(2)
        opt.step()

    def reset(model, opt, backward, tg):
        opt.zero_grad()
        backward(0)
        opt.step()
        opt.zero_grad()
        backward(1)
        tg().reset()
        assert int(tg().slot.abs().max()) == 0
        opt.step()
        opt.zero_grad()
        backward(2)
        opt.step()
    for script in (two, reset):
        _, p1 = _eager(dev, monkeypatch, '1', script)
        _, p0 = _eager(dev, monkeypatch, '0', script)
        for k in p0:
            _same(p1[k], p0[k], '%s: parameter %s' % (script.__name__, k))
