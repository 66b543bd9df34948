"""The three host descriptors of the k-gram GRU expander (gru.gru_fused_desc / gru_fused_bwd_desc / gru_step_desc ->
srec_gru_fused_desc, srec_gru_fused_bwd_desc, srec_gru_step_desc of include/srec_hg.h), its path predicate and what ops.py
re-exports of gru.py.  CPU only: `ptr` is pointed at Tensor.data_ptr and nothing is launched."""
import itertools

import pytest
import torch

from util import pkg

D = 64                       # 1024 // D = 16 nodes per block of the step kernel
RB = max(8, 1024 // D)


@pytest.fixture
def gru(monkeypatch):
    pkg('ops')               # (ops.py first: gru.py imports it and is imported at its end)
    g = pkg('gru')
    monkeypatch.setattr(g, 'ptr', lambda t: None if t is None else t.data_ptr())
    return g


def _table(q):
    """every per-problem field of a descriptor as a list over ALL slots (NULL -> 0)"""
    return {name: [v or 0 for v in getattr(q, name)] for name, _ in q._fields_ if name not in ('np', 'd')}


def _expect(q, maxp, **fields):
    """q's problem table is exactly `fields` (lists over the used slots of tensors / ints); everything else is zero"""
    want = {name: [0] * maxp for name in _table(q)}
    assert set(fields) <= set(want), set(fields) - set(want)
    for name, vals in fields.items():
        for i, v in enumerate(vals):
            want[name][i] = (v.data_ptr() if torch.is_tensor(v) else v) or 0
    assert _table(q) == want


class Orders:
    """P orders k = 2, 3, ... with distinct node counts and one distinct tensor for every descriptor field"""

    def __init__(self, gru, ks, ns):
        self.ks, self.ns, self.P = ks, ns, len(ks)
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt)
        per = lambda f: [f(k, n) for k, n in zip(ks, ns)]
        self.dyn_n, self.dyn_rows = per(lambda k, n: z(1, dt=torch.int32)), per(lambda k, n: z(1, dt=torch.int32))
        self.Wih, self.Whh = per(lambda k, n: z(3 * D, D)), per(lambda k, n: z(3 * D, D))
        self.bih, self.bhh = per(lambda k, n: z(3 * D)), per(lambda k, n: z(3 * D))
        self.orders = [gru.GruOrder(k, n, dn, dr, wi, bi, wh, bh) for k, n, dn, dr, wi, bi, wh, bh in
                       zip(ks, ns, self.dyn_n, self.dyn_rows, self.Wih, self.bih, self.Whh, self.bhh)]
        self.X, self.X16 = per(lambda k, n: z(n * k, D)), per(lambda k, n: z(n * k, D, dt=torch.bfloat16))
        self.H, self.H16 = per(lambda k, n: z(k, n, D)), per(lambda k, n: z(k - 1, n, D, dt=torch.bfloat16))
        self.gates, self.out = per(lambda k, n: z(k, n, 4 * D)), per(lambda k, n: z(n, D))
        self.GI, self.GH = per(lambda k, n: z(n * k, 3 * D)), per(lambda k, n: z(n, 3 * D))
        self.wf = per(lambda k, n: (z(3 * D * D, dt=torch.bfloat16), z(3 * D * D, dt=torch.bfloat16)))
        self.wt = per(lambda k, n: (z(3 * D * D, dt=torch.bfloat16), z(3 * D * D, dt=torch.bfloat16)))
        self.dout, self.dX = per(lambda k, n: z(n, D)), per(lambda k, n: z(n * k, D))
        self.dGI16 = per(lambda k, n: z(n * k, 3 * D, dt=torch.bfloat16))
        self.dGH16 = per(lambda k, n: z(k - 1, n, 3 * D, dt=torch.bfloat16))
        self.part = per(lambda k, n: z(k * -(-n // RB), 6 * D))
        self.dH, self.dHp = per(lambda k, n: z(n, D)), per(lambda k, n: z(n, D))


@pytest.mark.parametrize('P', [4, 2])
def test_fused_descs_fill_every_slot_with_its_own_order(gru, P):
    o = Orders(gru, [2, 3, 4, 5][:P], [33, 24, 17, 9][:P])
    maxp = gru.GRU_MAXP
    q = gru.gru_fused_desc(o.orders, D, o.X, o.X16, o.wf, o.H, o.H16, o.gates, o.out)
    assert (q.np, q.d) == (P, D)
    _expect(q, maxp, n=o.ns, k=o.ks, dyn=o.dyn_n, X=o.X, X16=o.X16, Wih_f=[w[0] for w in o.wf], Whh_f=[w[1] for w in o.wf],
            bih=o.bih, bhh=o.bhh, H=o.H, H16=o.H16, gates=o.gates, out=o.out)
    b = gru.gru_fused_bwd_desc(o.orders, D, o.gates, o.H, o.dout, o.wt, o.dGI16, o.dGH16, o.dX, o.part)
    assert (b.np, b.d) == (P, D)
    _expect(b, maxp, n=o.ns, k=o.ks, dyn=o.dyn_n, gates=o.gates, H=o.H, dout=o.dout, Wih_f=[w[0] for w in o.wt],
            Whh_f=[w[1] for w in o.wt], dGI16=o.dGI16, dGH16=o.dGH16, dX=o.dX, bias_part=o.part, part_row0=[0] * P)
    for t in (_table(q), _table(b)):           # distinct tensors everywhere: a pointer in a wrong slot cannot pass by coincidence
        ptrs = [v for name, vals in t.items() if name not in ('n', 'k', 'part_row0') for v in vals[:P]]
        assert len(set(ptrs)) == len(ptrs) and 0 not in ptrs
        assert all(v == 0 for vals in t.values() for v in vals[P:])        # unused slots stay zero


def test_step_desc_forward(gru):
    o = Orders(gru, [2, 3], [33, 24])
    bufs = [gru.StepFwd(o.GI[p], o.GH[p], o.H[p], o.H16[p], o.gates[p], o.X[p], o.out[p]) for p in range(2)]
    for t in range(3):
        act = [p for p in range(2) if t < o.ks[p]]
        q = gru.gru_step_desc([(o.orders[p], bufs[p]) for p in act], t, D)
        assert (q.np, q.d) == (len(act), D)
        last = [t == o.ks[p] - 1 for p in act]
        _expect(q, gru.GRU_MAXP, n=[o.ns[p] for p in act], k=[o.ks[p] for p in act], t=[t] * len(act), dyn=[o.dyn_n[p] for p in act],
                GI=[o.GI[p] for p in act], bih=[o.bih[p] for p in act], bhh=[o.bhh[p] for p in act],
                GH=[o.GH[p] if t > 0 else 0 for p in act], Hp=[o.H[p][t - 1] if t > 0 else 0 for p in act],
                Hn=[o.H[p][t] for p in act], gates=[o.gates[p][t] for p in act],
                Hn16=[0 if l else o.H16[p][t] for p, l in zip(act, last)],
                X=[o.X[p] if l else 0 for p, l in zip(act, last)], out=[o.out[p] if l else 0 for p, l in zip(act, last)])
        if t == 0:
            assert q.np == 2 and not q.GH[0] and not q.GH[1] and not q.Hp[0] and not q.Hp[1] and q.Hn16[0] and q.Hn16[1]
        if t == 1:
            assert q.np == 2 and q.X[0] == o.X[0].data_ptr() and not q.Hn16[0] and not q.X[1] and q.Hn16[1] == o.H16[1][1].data_ptr()
        if t == 2:                                 # only the k = 3 order is left, in slot 0
            assert q.np == 1 and (q.n[0], q.k[0]) == (24, 3) and q.X[0] == o.X[1].data_ptr() and q.out[0] == o.out[1].data_ptr()


def test_step_desc_backward(gru):
    o = Orders(gru, [2, 3], [33, 24])
    nblk = [-(-n // RB) for n in o.ns]
    assert nblk == [3, 2]
    for t in (2, 1, 0):
        act = [p for p in range(2) if t < o.ks[p]]
        bufs = [gru.StepBwd(o.gates[p], o.H[p], o.dout[p], o.dX[p], o.dGI16[p], o.dGH16[p], o.part[p],
                            None if t == o.ks[p] - 1 else o.dH[p], o.dHp[p] if t > 0 else None) for p in act]
        q = gru.gru_step_desc(list(zip([o.orders[p] for p in act], bufs)), t, D, backward=True)
        assert (q.np, q.d) == (len(act), D)
        last = [t == o.ks[p] - 1 for p in act]
        _expect(q, gru.GRU_MAXP, n=[o.ns[p] for p in act], k=[o.ks[p] for p in act], t=[t] * len(act), dyn=[o.dyn_n[p] for p in act],
                gates=[o.gates[p][t] for p in act], dGI16=[o.dGI16[p] for p in act],
                dout=[o.dout[p] if l else 0 for p, l in zip(act, last)], dX=[o.dX[p] if l else 0 for p, l in zip(act, last)],
                dH=[0 if l else o.dH[p] for p, l in zip(act, last)],
                Hp=[o.H[p][t - 1] if t > 0 else 0 for p in act], dGH16=[o.dGH16[p][t - 1] if t > 0 else 0 for p in act],
                dHp=[o.dHp[p] if t > 0 else 0 for p in act],
                bias_part=[o.part[p] for p in act], part_row0=[t * nblk[p] for p in act])
    assert gru.gru_step_blocks(33, D) == 3 and gru.gru_step_blocks(32, D) == 2 and gru.gru_step_blocks(9, 256) == 2


@pytest.mark.parametrize('P', [0, 5])
def test_too_many_or_no_orders_assert(gru, P):
    o = Orders(gru, list(range(2, 2 + P)), list(range(9, 9 + P)))
    with pytest.raises(AssertionError):
        gru.gru_fused_desc(o.orders, D, o.X, o.X16, o.wf, o.H, o.H16, o.gates, o.out)
    with pytest.raises(AssertionError):
        gru.gru_fused_bwd_desc(o.orders, D, o.gates, o.H, o.dout, o.wt, o.dGI16, o.dGH16, o.dX, o.part)
    fwd = [(o.orders[p], gru.StepFwd(o.GI[p], o.GH[p], o.H[p], o.H16[p], o.gates[p], o.X[p], o.out[p])) for p in range(P)]
    with pytest.raises(AssertionError):
        gru.gru_step_desc(fwd, 0, D)
    with pytest.raises(AssertionError):
        gru.gru_step_desc(fwd, 0, D, backward=True)


@pytest.mark.parametrize('prec,fused', list(itertools.product(['fp32', 'bf16'], [True, False])))
def test_expand_path_is_the_three_old_conditions(gru, monkeypatch, prec, fused):
    ops = pkg('ops')
    monkeypatch.setitem(ops.PRECISION, 'matmul', prec)
    monkeypatch.setattr(ops, 'FUSED_GRU', fused)
    seen = set()
    for d, reducer, K in itertools.product([64, 96, 128, 256, 1024, 2048], ['mean', 'max', 'concat'], [1, 2, 5, 6]):
        fast_ok = prec == 'bf16' and reducer == 'mean' and d % 64 == 0 and d <= 1024 and 256 % (d // 4) == 0
        fused_ok = d in (128, 256) and K - 1 <= 4 and fused
        assert bool(ops.gru_expand_fast_ok(d, reducer)) == fast_ok and bool(ops.gru_fused_ok(d, K - 1)) == fused_ok
        bf16 = ops.PRECISION['matmul'] == 'bf16'
        prologue = bool(bf16 and 1 < K <= 5 and ops.gru_expand_fast_ok(d, reducer) and ops.gru_fused_ok(d, K - 1))   # _step_prologue
        all_orders = bool(K > 1 and K <= 5 and ops.gru_expand_fast_ok(d, reducer))                                    # _session_repr
        node_fused = bool(ops.gru_fused_ok(d, K - 1))                                                                 # GRUExpandAll.forward
        path = gru.expand_path(d, reducer, K)
        assert path in (None, 'step', 'fused')
        assert (path == 'fused') == prologue and (path is not None) == all_orders
        if all_orders:
            assert (path == 'fused') == node_fused
        seen.add(path)
    assert seen == ({None} if prec == 'fp32' else {None, 'step', 'fused'} if fused else {None, 'step'})


def test_wfrag_args_and_pieces(gru):
    ws = [torch.zeros(3 * D, D) for _ in range(4)]
    of, ob, args = gru._gru_wfrag_args(ws)
    assert [list(a) for a in args] == [[t.data_ptr() for t in ts] for ts in (ws, of, ob)]
    assert all(t.dtype == torch.bfloat16 and t.numel() == 3 * D * D for t in of + ob)
    of, ob, args = gru._gru_wfrag_args(ws, backward=False)
    assert ob is None and [list(a) for a in args] == [[t.data_ptr() for t in ts] for ts in (ws, of)]
    buf = torch.arange(12.0).reshape(6, 2)
    a, b, c = gru.pieces(buf, [1, 3, 2])
    assert (a.shape[0], b.shape[0], c.shape[0]) == (1, 3, 2)
    assert b.data_ptr() == buf[1:].data_ptr() and c.data_ptr() == buf[4:].data_ptr() and torch.equal(c, buf[4:])


REEXPORTED = ['GRUPointwise', 'GramCombine', 'GRUExpand', 'GRUExpandAll', 'gru_step', 'gram_combine', 'gru_expand', 'gru_expand_all',
              'gru_wfrag', 'gru_wfrag_both', 'gru_fused_ok', 'gru_expand_fast_ok', 'expand_path', 'GruOrder', 'gru_step_desc',
              'gru_fused_desc', 'gru_fused_bwd_desc', '_gru_wfrag_args']


def test_ops_reexports_gru_and_the_dead_names_are_gone(gru):
    ops = pkg('ops')
    for name in REEXPORTED:
        assert getattr(ops, name) is getattr(gru, name), name
    for name in ('unbind_mid', 'UnbindMid', 'gru_wfrag_t'):
        assert not hasattr(ops, name) and not hasattr(gru, name), name
    assert ops.FUSED_GRU is True and not hasattr(gru, 'FUSED_GRU') and not hasattr(gru, 'PRECISION')     # the switches live in ops.py
    assert all(hasattr(ops, n) for n in ('GRUSeq', 'gru_seq'))                                             # LESSR's GRU stays in ops.py
