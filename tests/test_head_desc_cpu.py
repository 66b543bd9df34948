"""The host side of the attention read-out head (head.py): the two descriptors of the fused head (head.head_fwd_desc /
head_bwd_desc -> srec_head_desc, srec_head_bwd_desc of include/srec_hg.h), the problem lists and launch chunks of the two
backward tails, the path predicate, the fragment-copy cache and what ops.py re-exports of head.py.  CPU only: `ptr` is pointed
at Tensor.data_ptr, the library is a stub that launches nothing, and gemm_f32_group records its calls."""
import itertools

import pytest
import torch

from util import pkg

D, B, NT = 8, 5, 11


class _NoLib:
    """every srec_* entry point: accepted, not run"""

    def __getattr__(self, name):
        return lambda *args: 0


@pytest.fixture
def head(monkeypatch):
    ops = pkg('ops')         # (ops.py first: head.py imports it and is imported at its end)
    h = pkg('head')
    monkeypatch.setattr(h, 'ptr', lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(h, 'stream', lambda: None)
    monkeypatch.setattr(h, 'lib', _NoLib())
    ops.weights_changed()
    yield h
    ops.weights_changed()        # (no fragment copy of a CPU tensor outlives its test)


@pytest.fixture
def launches(head, monkeypatch):
    """[(problems, split3, defer)] of every gemm_f32_group call head.py makes"""
    seen = []
    monkeypatch.setattr(head, 'gemm_f32_group', lambda probs, split3=False, defer=None: seen.append((list(probs), split3, defer)))
    return seen


def _table(q):
    """every per-head field of a descriptor as a list over ALL slots (NULL -> 0)"""
    return {name: [v or 0 for v in getattr(q, name)] for name, _ in q._fields_ if hasattr(getattr(q, name), '__len__')}


def _expect(q, maxh, **fields):
    """q's per-head table is exactly `fields` (lists over the used slots of tensors); everything else is zero"""
    want = {name: [0] * maxh for name in _table(q)}
    assert set(fields) == set(want), set(fields) ^ set(want)
    for name, vals in fields.items():
        for i, v in enumerate(vals):
            want[name][i] = (v.data_ptr() if torch.is_tensor(v) else v) or 0
    assert _table(q) == want
    return want


@pytest.mark.parametrize('n', [1, 4])
def test_descs_fill_every_slot_with_its_own_order(head, n):
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt)
    per = lambda f: [f() for _ in range(n)]
    allf, seg, dB = z(NT, D), z(B + 1, dt=torch.int32), z(1, dt=torch.int32)
    orders = per(lambda: head.HeadOrder(z(B, 2 * D)[:, :D], z(D, D), z(D), z(D, D), z(D), z(D, 2 * D)))
    wf = per(lambda: [z(2 * D * D, dt=torch.bfloat16), z(2 * D * D, dt=torch.bfloat16), z(4 * D * D, dt=torch.bfloat16)])
    fb = per(lambda: head.HeadFwdBufs(z(B, 2 * D), z(NT), z(NT, D), z(B, D), z(B, D), z(B)))
    sr16 = z(B + 3, D + 8, dt=torch.bfloat16)
    q = head.head_fwd_desc(allf, seg, dB, 1, orders, wf, fb, sr16)
    assert (q.nh, q.d, q.B, q.NT, q.ld_x, q.ld16, q.eps_mode) == (n, D, B, NT, D, D + 8, 1) and abs(q.eps - 1e-12) < 1e-18
    assert (q.X, q.seg, q.dynB) == (allf.data_ptr(), seg.data_ptr(), dB.data_ptr())
    tf = _expect(q, head.HEAD_MAXH, cat=[b.cat for b in fb], Wu_f=[w[0] for w in wf], Wv_f=[w[1] for w in wf], Wsr_f=[w[2] for w in wf],
                 bu=[o.bu for o in orders], we=[o.we for o in orders], alpha=[b.alpha for b in fb], U=[b.U for b in fb],
                 Vq=[b.Vq for b in fb], y=[b.y for b in fb], inv=[b.inv for b in fb], y16=[sr16])
    q0 = head.head_fwd_desc(allf, seg, None, 0, [o._replace(bu=None) for o in orders], wf, fb)       # no bias, no operand copy, no dyn
    assert (q0.ld16, q0.eps_mode, q0.dynB) == (0, 0, None)
    assert _table(q0)['bu'] == [0] * head.HEAD_MAXH and _table(q0)['y16'] == [0] * head.HEAD_MAXH

    saved = [head.HeadSavedFused(o.v, o.Wu, o.Wv, o.we, o.Wsr, b.U, b.Vq, b.alpha, b.cat, b.y, b.inv) for o, b in zip(orders, fb)]
    wft = per(lambda: z(4 * D * D, dt=torch.bfloat16))
    bb = per(lambda: head.HeadBwdBufs(z(B, D + 4)[:, :D], z(B, D), z(B, 2 * D), z(NT, D), z(NT, D), z(B, D), z(B, D)))
    r = head.head_bwd_desc(allf, seg, dB, saved, wft, bb)
    assert (r.nh, r.d, r.B, r.NT, r.ld_x, r.ld_gy) == (n, D, B, NT, D, D + 4)
    assert (r.X, r.seg, r.dynB) == (allf.data_ptr(), seg.data_ptr(), dB.data_ptr())
    tb = _expect(r, head.HEAD_MAXH, gy=[b.gy for b in bb], y=[s.y for s in saved], inv=[s.inv for s in saved], WsrT_f=wft,
                 alpha=[s.alpha for s in saved], U=[s.U for s in saved], Vq=[s.Vq for s in saved], we=[s.we for s in saved],
                 gs=[b.gs for b in bb], gcat=[b.gcat for b in bb], dX=[b.dX for b in bb], dU=[b.dU for b in bb],
                 dVq=[b.dVq for b in bb], dwp=[b.dwp for b in bb])
    for t in (tf, tb):          # distinct tensors everywhere: a pointer in a wrong slot cannot pass by coincidence
        ptrs = [v for name, vals in t.items() if name != 'y16' for v in vals[:n]]
        assert len(set(ptrs)) == len(ptrs) and 0 not in ptrs
    if n > 1:
        with pytest.raises(AssertionError):    # a gradient with another row stride than the first
            head.head_bwd_desc(allf, seg, dB, saved, wft, bb[:-1] + [bb[-1]._replace(gy=z(B, D))])


@pytest.mark.parametrize('n', [0, 5])
def test_too_many_or_no_heads_assert(head, n):
    z = torch.zeros
    allf, seg = z(NT, D), z(B + 1, dtype=torch.int32)
    orders = [head.HeadOrder(z(B, D), z(D, D), None, z(D, D), z(D), z(D, 2 * D)) for _ in range(n)]
    fb = [head.HeadFwdBufs(z(B, 2 * D), z(NT), z(NT, D), z(B, D), z(B, D), z(B)) for _ in range(n)]
    with pytest.raises(AssertionError):
        head.head_fwd_desc(allf, seg, None, 0, orders, [[z(1)] * 3] * n, fb)
    saved = [head.HeadSavedFused(o.v, o.Wu, o.Wv, o.we, o.Wsr, b.U, b.Vq, b.alpha, b.cat, b.y, b.inv) for o, b in zip(orders, fb)]
    bb = [head.HeadBwdBufs(z(B, D), z(B, D), z(B, 2 * D), z(NT, D), z(NT, D), z(B, D), z(B, D)) for _ in range(n)]
    with pytest.raises(AssertionError):
        head.head_bwd_desc(allf, seg, None, saved, [z(1)] * n, bb)


class Head:
    """n live orders with distinct leaf tensors; bias[i] False: order i has no fc_u bias"""

    def __init__(self, bias):
        r = lambda *shape: torch.randn(*shape).requires_grad_()
        self.allf, self.seg = r(NT, D), torch.zeros(B + 1, dtype=torch.int32)
        self.dT, self.dB = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
        self.bufs, self.per = [], []
        for has in bias:
            buf = r(B, 2 * D)
            v = buf[:, :D]
            v._srec_cat_left = True
            self.bufs.append(buf)
            self.per.append([v, r(D, D), r(D) if has else None, r(D, D), r(1, D), r(D, 2 * D)])

    def backward(self, outs):
        leaves = [self.allf] + [t for po in self.per for t in po[1:] if t is not None] + self.bufs
        return torch.autograd.grad([o.sum() for o in outs], leaves, allow_unused=True)


def _same(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _check_tail(h, bias, probs, fused):
    """the problem list of one backward tail, in order, against the products the parent's two backward functions listed"""
    it = iter(probs)
    for o, has in zip(h.per, bias):
        v, Wu, bu, Wv, we, Wsr = o
        kind, dU, b, dX, pb, dyn, beta = next(it)
        assert (kind, beta, pb) == ('nn', 1.0, None) and _same(b, Wu) and dyn is h.dT and dU.shape == (NT, D) and dX.shape == (NT, D)
        kind, a, b, out, pb, dyn, beta = next(it)
        assert (kind, beta, pb) == ('tn', 0.0, None) and a is dU and _same(b, h.allf) and dyn is h.dT and out.shape == Wu.shape
        kind, dVq, b, gv, pb, dyn, beta = next(it)
        assert (kind, beta, pb) == ('nn', 1.0, None) and _same(b, Wv) and dyn is h.dB and dVq.shape == (B, D)
        assert gv.shape == (B, D) and gv.stride() == (2 * D, 1)                      # the left half of d cat
        kind, a, b, out, pb, dyn, beta = next(it)
        assert (kind, beta, pb) == ('tn', 0.0, None) and a is dVq and _same(b, v) and dyn is h.dB and out.shape == Wv.shape
        if fused:
            kind, gs, cat, out, pb, dyn, beta = next(it)
            assert (kind, beta, pb) == ('tn', 0.0, None) and gs.shape == (B, D) and dyn is h.dB and out.shape == Wsr.shape
            assert cat.data_ptr() == v.data_ptr() and cat.shape == (B, 2 * D)
        if has:                 # the grouped head sums dU over the node rows, the fused head dVq over the sessions
            kind, ones, b, s_bu, pb, dyn, beta = next(it)
            assert (kind, beta, pb) == ('tn', 0.0, None) and s_bu.shape == (4, D)
            assert (b is dVq and dyn is h.dB and ones.shape == (B, 4)) if fused else (b is dU and dyn is h.dT and ones.shape == (NT, 4))
            assert bool((ones == 1).all())
        kind, ones, dwp, s_we, pb, dyn, beta = next(it)
        assert (kind, beta, pb) == ('tn', 0.0, None) and ones.shape == (B, 4) and dwp.shape == (B, D) and dyn is h.dB
        assert s_we.shape == (4, D) and dwp is not dVq and bool((ones == 1).all())
        if has:
            assert s_we.data_ptr() == s_bu.data_ptr() + 4 * D * 4                       # the two blocks of one [8, D] buffer
    assert next(it, None) is None


PATTERNS = [p for n in range(1, 5) for p in itertools.product([True, False], repeat=n)]
# (bias pattern) -> problems per launch, from the parent's `12 if len(probs) > 16 else 16` and
# `GEMM32_MAXP if len(probs) <= GEMM32_MAXP else GEMM32_MAXP // 7 * 7`
NAMED_GROUPED = {(True, True, True): [12, 6], (True, False, True, False): [12, 10], (True,): [6], (True, True): [12],
                 (False, False, False): [15], (True, True, True, True): [12, 12], (False, False, False, False): [12, 8]}
NAMED_FUSED = {(True, True, True): [14, 7], (True, False, True, False): [14, 12], (False, True, False): [14, 5], (True,): [7],
               (True, True): [14], (False, False): [12], (True, True, True, True): [14, 14], (False, False, False, False): [14, 10]}


def _chunks(total, step):
    return [min(step, total - c) for c in range(0, total, step)]


@pytest.mark.parametrize('prec', ['fp32', 'bf16'])
@pytest.mark.parametrize('bias', PATTERNS)
def test_grouped_backward_problem_list(head, launches, monkeypatch, bias, prec):
    ops = pkg('ops')
    monkeypatch.setitem(ops.PRECISION, 'matmul', prec)
    h, n = Head(bias), len(bias)
    outs = head.readout_head(h.allf, h.seg, h.dT, h.dB, h.per)
    assert [len(p) for p, _, _ in launches] == [2 * n, n]                      # forward: all U / Vq, then all s
    for o, (kind, a, b, out, pb, dyn, beta) in zip(h.per, launches[0][0][::2]):
        assert kind == 'nt' and _same(b, o[1]) and (pb is None if o[2] is None else _same(pb, o[2])) and dyn is h.dT      # the bias (or None) rides on the U product
    del launches[:]
    grads = h.backward(outs)
    assert all(g is not None for g in grads)
    first, tail = launches[0], launches[1:]
    assert [p[0] for p in first[0]] == ['nn', 'tn'] * n                         # d cat, d Wsr of every order
    total = 5 * n + sum(bias)
    want = _chunks(total, 12 if total > 16 else 16)
    assert [len(p) for p, _, _ in tail] == want == NAMED_GROUPED.get(bias, want)
    assert all(s3 == (prec == 'bf16') and defer is None for _, s3, defer in launches)
    _check_tail(h, bias, [p for ps, _, _ in tail for p in ps], fused=False)


@pytest.mark.parametrize('bias', PATTERNS)
def test_fused_backward_problem_list(head, launches, bias):
    h, n = Head(bias), len(bias)
    ys = head.readout_head_fused(h.allf, h.seg, h.dT, h.dB, h.per)
    assert launches == [] and len(head._WF) == 4 * n                            # one launch forward; fc_u, fc_v, fc_sr, fc_sr^T copies
    grads = h.backward(ys)
    assert all(g is not None for g in grads)
    total = 6 * n + sum(bias)
    want = _chunks(total, 16 if total <= 16 else 14)
    assert [len(p) for p, _, _ in launches] == want == NAMED_FUSED.get(bias, want)
    assert all(s3 is True and defer is None for _, s3, defer in launches)      # (no step is deferring here)
    _check_tail(h, bias, [p for ps, _, _ in launches for p in ps], fused=True)


def test_fused_backward_defer_list(head, launches, monkeypatch):
    """inside a deferring step: every weight gradient in order of the heads, then the sum blocks"""
    monkeypatch.setattr(head, 'defer_scope', lambda: True)
    bias = (True, False, True)
    h = Head(bias)
    h.backward(head.readout_head_fused(h.allf, h.seg, h.dT, h.dB, h.per))
    assert len(launches) == 2 and launches[0][2] is launches[1][2]
    probs, later = [p for ps, _, _ in launches for p in ps], launches[0][2]
    tn = [p[3] for p in probs if p[0] == 'tn']
    gw = [t for t in tn if t.shape != (4, D)]
    blocks = [t for t in tn if t.shape == (4, D)]
    assert len(gw) == 9 and len(blocks) == 5 and len(later) == 14
    assert all(a is b for a, b in zip(later, gw + blocks))                        # the SAME objects: gemm_f32_group matches by identity


def test_head_path_table(head, monkeypatch):
    ops = pkg('ops')
    seen = set()
    for prec, norm, d, b, n in itertools.product(['fp32', 'bf16'], [True, False], [64, 128, 256], [1, 2, 8192, 8193], [1, 4, 5]):
        monkeypatch.setitem(ops.PRECISION, 'matmul', prec)
        fused = prec == 'bf16' and norm and n <= 4 and d in (128, 256) and 1 < b <= 8192        # msgifsr.py's old condition
        assert head.head_path(d, n, b, norm) == ('fused' if fused else 'grouped'), (prec, norm, d, b, n)
        seen.add(fused)
    assert seen == {True, False} and head.HEAD_FUSED_MAX_B == 8192 and head.HEAD_MAXH == 4
    assert head.head_path(128, 0, 64, True) == 'grouped'


def test_fragment_cache_has_one_key(head):
    ops = pkg('ops')
    w, u = torch.zeros(D, 2 * D), torch.zeros(D, D)
    entries = [(w, 0), (w, 1), (u, False)]
    assert head.wfrag_missing(entries) == [(w, 0), (w, 1), (u, 0)]
    made = head.head_wfrag([w, u], [1, 0])
    assert [m.numel() for m in made] == [4 * D * D, 2 * D * D] and all(m.dtype == torch.bfloat16 for m in made)
    assert head.wfrag_missing(entries) == [(w, 0)] and head.wfrag_get(w, True) is made[0]
    again = head.head_wfrag([u, w, w], [0, 0, 1])
    assert again[0] is made[1] and again[2] is made[0] and head.wfrag_missing(entries) == []
    assert len(head.wfrag_missing([(torch.zeros(D, D), 0) for _ in range(20)])) == head.HEAD_MAXW == 16
    assert ops._HEAD_WF is head._WF and len(head._WF) == 3
    ops.weights_changed()
    assert not head._WF and head.wfrag_missing(entries) == [(w, 0), (w, 1), (u, 0)]


REEXPORTED = ['SegAttn', 'seg_attn', 'ReadoutHead', 'ReadoutHeadFused', '_head_wfrag_args', 'head_wfrag', 'HEAD_FUSED_MAX_B',
              'readout_head_fused_ok', 'readout_head_fused', 'readout_head', 'head_path', 'head_fwd_desc', 'head_bwd_desc', 'HeadOrder']


def test_ops_reexports_head_and_the_dead_names_are_gone(head):
    ops = pkg('ops')
    for name in REEXPORTED:
        assert getattr(ops, name) is getattr(head, name), name
    for name in ('_HEAD_WF_CACHE', '_readout_head_backward'):
        assert not hasattr(ops, name) and not hasattr(head, name), name
    assert [n for n in vars(ops) if n.startswith('FUSED_')] == ['FUSED_GRU']                 # the one switch tests flip
    assert not hasattr(head, 'PRECISION')                                                    # the switch lives in ops.py
    assert all(hasattr(ops, n) and not hasattr(head, n) for n in ('step_prologue', '_GROUP_DEBUG'))
