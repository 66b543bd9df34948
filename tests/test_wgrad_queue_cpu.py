"""Waiting tn products of stepq.StepQueue on the CPU: a product that waits is issued before any slab sum and before the backward
pass ends, whoever sends it off; its keepalive lives exactly until then.  The three launch callables are recorders that log
into ONE list, so the order between product launches and sum launches is what the assertions read - no kernel runs."""
import gc
import weakref

import pytest
import torch

from util import pkg


class Rec:
    def __init__(self):
        self.log = []                                  # ('sum', [out ptrs]) / ('tn', family A or None, family B or None)
        self.q = pkg('stepq').StepQueue(
            lambda tasks, rider=None: self.log.append(('sum', [t[1].data_ptr() for t in tasks])),
            lambda *entry: self.log.append(('intake',) + entry),
            lambda a, b=None: self.log.append(('tn', None if a is None else list(a), None if b is None else list(b))))


class Keep:
    """a keepalive one can watch die"""


def _node(x, backward):
    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            backward()
            return g
    return Node.apply(x)


def _chain(x, *backwards):
    """backwards run in the order given (the first is the node nearest the loss)"""
    for b in reversed(backwards):
        x = _node(x, b)
    return x


def _sum(tag):
    return torch.full((2, 3), float(tag)), torch.zeros(3)


def _x():
    return torch.ones(3, requires_grad=True)


def test_taker_carries_the_waiting_list_as_family_a():
    r = Rec()
    q = r.q
    p1, o1 = _sum(1)
    seen = []

    def giver():
        q.defer_product(['g0', 'g1', 'g2'], 'keep')
        q.defer_slab_sum(p1, o1, True)                 # (the sum over the slabs the product writes)
        seen.append((q.products_waiting(), list(r.log)))
    _chain(_x(), giver, lambda: q.leave_with(['r0', 'r1'], 16)).sum().backward()
    assert seen == [(1, [])]                           # nothing left before the taker
    assert r.log == [('tn', ['g0', 'g1', 'g2'], ['r0', 'r1']), ('sum', [o1.data_ptr()])]
    assert q.products_waiting() == 0 and q.waiting() == 0


def test_what_does_not_fit_leaves_in_front_in_waiting_order():
    r = Rec()
    q = r.q
    big1, small, big2 = ['a%d' % i for i in range(12)], ['b0', 'b1'], ['c%d' % i for i in range(12)]
    own = ['r0', 'r1', 'r2', 'r3']
    _chain(_x(), lambda: q.defer_product(big1), lambda: q.defer_product(big2), lambda: q.defer_product(small),
           lambda: q.leave_with(own, 16)).sum().backward()
    # 12 fit beside 4; the second list of 12 does not and leaves on its own in front; 2 more would not fit either
    assert r.log == [('tn', big2, None), ('tn', small, None), ('tn', big1, own)]
    assert q.products_waiting() == 0
    # whole lists only, several when they fit
    r = Rec()
    q = r.q
    _chain(_x(), lambda: q.defer_product(['a0', 'a1']), lambda: q.defer_product(['b0']),
           lambda: q.leave_with(own, 16)).sum().backward()
    assert r.log == [('tn', ['a0', 'a1', 'b0'], own)]


def test_taker_with_nothing_waiting_launches_its_own():
    r = Rec()
    _chain(_x(), lambda: r.q.leave_with(['r0'], 16)).sum().backward()
    r.q.leave_with(['r1'], 16)                         # ... also outside a backward pass
    assert r.log == [('tn', None, ['r0']), ('tn', None, ['r1'])]


def test_finish_issues_products_first_when_nobody_takes_them():
    r = Rec()
    q = r.q
    p1, o1 = _sum(1)

    def giver():
        q.defer_slab_sum(p1, o1, True)                 # (registered first: the order of issue must not follow it)
        q.defer_product(['g0'])
    q.offer_rider(('args',), [(0, 0)], None)
    _chain(_x(), giver).sum().backward()               # order 1: no GRU node follows the layer
    assert r.log == [('tn', ['g0'], None), ('sum', [o1.data_ptr()])]
    assert q.rider_result() == frozenset([(0, 0)])
    # a product alone still gets the end-of-backward callback
    r = Rec()
    _chain(_x(), lambda: r.q.defer_product(['g0'])).sum().backward()
    assert r.log == [('tn', ['g0'], None)] and r.q.products_waiting() == 0


def test_mid_backward_flush_issues_products_then_sums():
    r = Rec()
    q = r.q
    (p1, o1), (p2, o2) = _sum(1), _sum(2)

    def giver():
        q.defer_slab_sum(p1, o1, True)
        q.defer_product(['g0'])
    _chain(_x(), giver, q.flush, lambda: q.defer_slab_sum(p2, o2, True),
           lambda: q.leave_with(['r0'], 16)).sum().backward()
    assert r.log == [('tn', ['g0'], None), ('sum', [o1.data_ptr()]), ('tn', None, ['r0']), ('sum', [o2.data_ptr()])]


def test_immediate_sum_issues_products_first():
    r = Rec()
    q = r.q
    p1, o1 = _sum(1)
    _chain(_x(), lambda: q.defer_product(['g0']), lambda: q.defer_slab_sum(p1, o1, False),
           lambda: q.leave_with(['r0'], 16)).sum().backward()
    assert r.log == [('tn', ['g0'], None), ('sum', [o1.data_ptr()]), ('tn', None, ['r0'])]


def test_outside_a_backward_or_not_ok_nothing_waits():
    r = Rec()
    q = r.q
    q.defer_product(['g0'], 'keep')                    # no backward pass is running
    assert r.log == [('tn', ['g0'], None)] and q.products_waiting() == 0
    _chain(_x(), lambda: q.defer_product(['g1'], 'keep', ok=False),
           lambda: r.log.append(('after', q.products_waiting()))).sum().backward()
    assert r.log[1:] == [('tn', ['g1'], None), ('after', 0)]


@pytest.mark.parametrize('how', ['abort', 'drop_stale', 'deferring'])
def test_abort_and_drop_stale_forget_products_and_keepalives(how):
    r = Rec()
    q = r.q
    keep = Keep()
    alive = weakref.ref(keep)

    def boom():
        q.defer_product(['g0'], keep)
        raise RuntimeError('boom')
    with pytest.raises(RuntimeError, match='boom'):
        _chain(_x(), boom).sum().backward()
    del keep, boom
    gc.collect()
    assert q.products_waiting() == 1 and alive() is not None
    if how == 'deferring':                             # the next outermost permission scope forgets a dead pass's leftovers
        with q.deferring(True):
            assert q.products_waiting() == 0
    else:
        getattr(q, how)()
    gc.collect()
    assert q.products_waiting() == 0 and alive() is None
    q.finish()
    q.flush()
    assert r.log == []


@pytest.mark.parametrize('sender', ['take', 'finish', 'flush', 'sum'])
def test_keepalive_lives_until_the_launch_is_issued(sender):
    r = Rec()
    q = r.q
    p1, o1 = _sum(1)
    state = {}
    launch = q._launch_products

    def launch_and_look(a, b=None):
        if a is not None:
            state['at_launch'] = state['ref']() is not None
        launch(a, b)
    q._launch_products = launch_and_look

    def giver():
        keep = Keep()
        state['ref'] = weakref.ref(keep)
        q.defer_product(['g0'], keep)

    def look():
        gc.collect()
        state['before'] = state['ref']() is not None
    send = {'take': lambda: q.leave_with(['r0'], 16), 'finish': lambda: None, 'flush': q.flush,
            'sum': lambda: q.defer_slab_sum(p1, o1, False)}[sender]

    def after():
        gc.collect()
        state['after'] = state['ref']() is not None
    _chain(_x(), giver, look, send, after).sum().backward()
    gc.collect()
    assert state['before'] and state['at_launch'] and state['ref']() is None
    assert state['after'] == (sender == 'finish')      # (finish runs after the last node)
    assert [e for e in r.log if e[0] == 'tn'][0][1] == ['g0']
