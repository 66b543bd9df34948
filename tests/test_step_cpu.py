"""The protocol of stepq.StepQueue (ops.STEP) on the CPU: which waiting launch leaves with which, driven by toy autograd nodes on
a fresh queue whose two launch callables are recorders - no kernel runs."""
import pytest
import torch

from util import pkg


class Rec:
    def __init__(self):
        self.sums, self.intakes = [], []             # [(tasks, rider)], [entry[:6]]
        self.q = pkg('stepq').StepQueue(lambda tasks, rider=None: self.sums.append((list(tasks), rider)),
                                        lambda *entry: self.intakes.append(entry))


def _node(x, backward):
    """identity whose backward calls backward() first"""
    class Node(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 1.0

        @staticmethod
        def backward(ctx, g):
            backward()
            return g
    return Node.apply(x)


def _sum(tag):
    return torch.full((2, 3), float(tag)), torch.zeros(3)


def _outs(tasks):
    return [t[1].data_ptr() for t in tasks]


def test_mid_backward_flush_keeps_the_rider():
    r = Rec()
    q = r.q
    (p1, o1), (p2, o2) = _sum(1), _sum(2)
    x = torch.ones(3, requires_grad=True)
    y = _node(x, lambda: q.defer_slab_sum(p2, o2, True))          # (runs last)
    y = _node(y, q.flush)                                          # dist.VocabParallel.bucket_ready
    y = _node(y, lambda: q.defer_slab_sum(p1, o1, True))          # (runs first)
    q.offer_rider(('args',), [(0, 0), (1, 0)], 'keep')
    y.sum().backward()
    assert len(r.sums) == 2
    (t1, r1), (t2, r2) = r.sums
    assert _outs(t1) == [o1.data_ptr()] and r1 is None
    assert _outs(t2) == [o2.data_ptr()] and r2 == ('args',)
    assert t1[0][0] is p1 and t2[0][0] is p2 and q.waiting() == 0
    assert q.rider_result() == frozenset([(0, 0), (1, 0)])
    assert q.rider_result() is None


def test_rider_with_nothing_to_ride_in():
    r = Rec()
    q = r.q
    x = torch.ones(3, requires_grad=True)
    q.offer_rider(('stale',), [(0, 0)], None)
    _node(x, lambda: None).sum().backward()
    q.finish()                                                     # FusedAdam._work
    assert r.sums == [] and q.rider_result() is None
    p, o = _sum(1)
    _node(x, lambda: q.defer_slab_sum(p, o, True)).sum().backward()
    assert len(r.sums) == 1 and r.sums[0][1] is None               # no stale rider
    assert q.rider_result() is None


def test_aborted_backward_and_nested_permission():
    r = Rec()
    q = r.q
    (p1, o1), (p2, o2) = _sum(1), _sum(2)
    x = torch.ones(3, requires_grad=True)

    def boom():
        q.defer_slab_sum(p1, o1, True)
        raise RuntimeError('boom')
    with pytest.raises(RuntimeError, match='boom'):
        _node(x, boom).sum().backward()
    assert q.waiting() == 1 and not q.may_defer
    with q.deferring(True):
        assert q.waiting() == 0 and r.sums == [] and q.may_defer
        y = _node(x, lambda: q.defer_slab_sum(p2, o2, True))
    assert not q.may_defer
    y.sum().backward()
    assert [_outs(t) for t, _ in r.sums] == [[o2.data_ptr()]] and q.waiting() == 0
    # nested: drops nothing, restores the outer value - also when the body raises
    def stale():
        with pytest.raises(RuntimeError, match='boom'):
            _node(x, boom).sum().backward()
    for outer in (True, False):
        stale()
        with q.deferring(outer):
            assert q.waiting() == 0
            stale()
            with q.deferring(not outer):
                assert q.may_defer == (not outer) and q.waiting() == 1
            assert q.may_defer == outer
            with pytest.raises(KeyError):
                with q.deferring(not outer):
                    raise KeyError('x')
            assert q.may_defer == outer and q.waiting() == 1
        assert not q.may_defer
    assert len(r.sums) == 1


def test_not_ok_or_outside_a_backward_launches_on_the_spot():
    r = Rec()
    p, o = _sum(1)
    r.q.defer_slab_sum(p, o, True)                                 # no backward pass is running
    r.q.defer_slab_sum(p, o, False)
    assert [(len(t), rd) for t, rd in r.sums] == [(1, None), (1, None)] and r.q.waiting() == 0


def test_intake_rides_or_leaves_in_order():
    r = Rec()
    q = r.q
    ents = [(i, 64, 100 + i, 200 + i, 300 + i, 400 + i, 'keepalive') for i in range(3)]
    q.offer_intake(ents)
    assert q.intake_pending()
    assert q.take_intake() == ents[2]
    assert r.intakes == [ents[0][:6], ents[1][:6]] and not q.intake_pending()
    assert q.take_intake() is None
    del r.intakes[:]
    q.offer_intake(ents)
    q.flush_intake()
    assert r.intakes == [e[:6] for e in ents] and not q.intake_pending()


def test_abort_forgets_everything():
    r = Rec()
    q = r.q
    p, o = _sum(1)
    x = torch.ones(3, requires_grad=True)

    def boom():
        q.defer_slab_sum(p, o, True)
        raise RuntimeError('boom')
    with pytest.raises(RuntimeError, match='boom'):
        _node(x, boom).sum().backward()
    q.offer_rider(('args',), [(0, 0)], None)
    q.offer_intake([(0, 64, 1, 2, 3, 4)])
    assert q.waiting() == 1 and q.intake_pending()
    q.abort()
    assert q.waiting() == 0 and q.rider_result() is None and not q.intake_pending()
    q.finish()
    assert r.sums == [] and r.intakes == []


class _Shard:
    aborted = 0

    def abort_step(self):
        self.aborted += 1


class _Opt:
    def __init__(self):
        self._frozen, self.grad_join = ['work'], (lambda: None)


def _stub_step(made):
    graph = pkg('graph')
    gs = graph.GraphedTrainStep.__new__(graph.GraphedTrainStep)      # (a capture that "succeeded": no constructor, no GPU)
    gs.model, gs.opt = torch.nn.Linear(2, 2), _Opt()
    gs.model.shard = _Shard()
    made.append(gs)
    return gs


def test_capture_agreed_cleans_up_a_step_another_rank_refused():
    graph, ops = pkg('graph'), pkg('ops')
    try:
        made = []
        ops.STEP.offer_rider(('args',), [(0, 0)], None)
        ops.STEP.offer_intake([(0, 64, 1, 2, 3, 4)])
        gs, attempts, err = graph.capture_agreed(lambda: _stub_step(made), agree_min=lambda ok: 0.0, retries=1)
        assert gs is None and attempts == 2 and err is None and len(made) == 2
        for s in made:
            assert s.opt._frozen is None and s.opt.grad_join is None and s.model.shard.aborted == 1
        assert ops.STEP.waiting() == 0 and not ops.STEP.intake_pending() and ops.STEP.rider_result() is None
        # all ranks agree: nothing is touched
        made = []
        ops.STEP.offer_intake([(0, 64, 1, 2, 3, 4)])
        gs, attempts, err = graph.capture_agreed(lambda: _stub_step(made), agree_min=lambda ok: ok, retries=1)
        assert gs is made[0] and attempts == 1 and err is None and len(made) == 1
        assert gs.opt._frozen == ['work'] and gs.opt.grad_join is not None and gs.model.shard.aborted == 0
        assert ops.STEP.intake_pending()
    finally:
        ops.STEP.abort()
