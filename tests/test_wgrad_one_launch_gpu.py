"""ops.WGRAD_ONE_LAUNCH: the MSHGNN layers' weight-gradient products wait for the k-gram GRU's and leave in its launch
(stepq.StepQueue, "Waiting tn products").  Every output tile is computed by the same code from the same operands whichever launch
carries it, so a training step with the switch on equals the step with it off byte for byte: losses, every parameter gradient, the
parameters after the steps.  Each case also pins WHICH launches left, so that no comparison is switch-off against switch-off."""
import numpy as np
import pytest
import torch

from util import pkg, reseed

V = 400


def _samples(rng, n=8, max_len=6):
    """n sessions of at most max_len clicks, some with a repeated item"""
    out = []
    for _ in range(n):
        L = int(rng.integers(1, max_len + 1))
        seq = rng.integers(0, V, size=L).tolist()
        if L > 1 and rng.random() < 0.3:
            seq[1] = seq[0]
        out.append((seq, int(rng.integers(0, V))))
    return out


def _model(dev, order, d, dropout, layers=1):
    torch.manual_seed(order * 1000 + d)
    return pkg().MSGIFSR(V, 'x', d, layers, dropout=dropout, order=order, extra=False, fusion=False).to(dev).train()


def _batches(order, n_batches=4):
    c = pkg('collate')
    rng = np.random.default_rng(17)
    mk = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), order, caps=c.default_caps(8, 6))
    return [mk(_samples(rng)) for _ in range(n_batches)]


class Spy:
    """the (family A, family B) problem counts of every tn product launch the queue issues"""

    def __init__(self, monkeypatch, ops):
        self.calls = []
        launch = ops.STEP._launch_products

        def spy(a, b=None):
            self.calls.append((len(a) if a else 0, len(b) if b else 0))
            launch(a, b)
        monkeypatch.setattr(ops.STEP, '_launch_products', spy)


def _eager(dev, ops, sw, order, d, dropout, layers=1, steps=2, twice=False):
    """-> (losses, gradients after the last backward, parameters after the steps)"""
    train, optim = pkg('train'), pkg('optim')
    ops.WGRAD_ONE_LAUNCH = sw
    model = _model(dev, order, d, dropout, layers)
    reseed(5)
    opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model)
    losses = []
    for (mg,), lab in _batches(order)[:steps]:
        opt.zero_grad()
        for _ in range(2 if twice else 1):             # twice: the second backward finds p.grad set
            loss = model.fused_loss(mg.to(dev), lab.to(dev))
            loss.backward()
            losses.append(loss.item())
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
    torch.cuda.synchronize()
    assert ops.STEP.products_waiting() == 0
    return losses, grads, {k: p.detach().clone() for k, p in model.named_parameters()}


def _same(a, b):
    (l0, g0, p0), (l1, g1, p1) = a, b
    assert l0 == l1, (l0, l1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), ('gradient', k)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), ('parameter', k)


@pytest.fixture
def bf16(monkeypatch):
    ops = pkg('ops')
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    monkeypatch.setattr(ops, 'WGRAD_ONE_LAUNCH', False)
    ops.weights_changed()
    yield ops
    ops.STEP.abort()


@pytest.mark.gpu
@pytest.mark.parametrize('family_order', ['a', 'b'])
@pytest.mark.parametrize('dropout', [0.0, 0.1], ids=['nodrop', 'drop0.1'])
@pytest.mark.parametrize('d', [64, 256])
@pytest.mark.parametrize('order', [2, 3])
def test_eager_steps_are_byte_equal(dev, bf16, monkeypatch, order, d, dropout, family_order):
    ops = bf16
    monkeypatch.setattr(ops, 'WGRAD_FAMILY_ORDER', family_order)
    spy = Spy(monkeypatch, ops)
    off = _eager(dev, ops, False, order, d, dropout)
    assert spy.calls == []                             # switch off: nobody goes through the queue
    on = _eager(dev, ops, True, order, d, dropout)
    # one launch per step: the layer's problems (one per module and node type it projects) as family A, the GRUs' 2 per order as B
    assert len(spy.calls) == 2 and spy.calls[0] == spy.calls[1], spy.calls
    nA, nB = spy.calls[0]
    assert nB == 2 * (order - 1) and nA >= 2 * (order + 1) and nA + nB <= ops.G16_MAXP, spy.calls
    assert len(off[1]) > 8                             # (the gradients are there to be compared)
    _same(off, on)


@pytest.mark.gpu
@pytest.mark.parametrize('dropout', [0.0, 0.1], ids=['nodrop', 'drop0.1'])
@pytest.mark.parametrize('d', [64, 256])
@pytest.mark.parametrize('order', [2, 3])
def test_captured_steps_are_byte_equal(dev, bf16, monkeypatch, order, d, dropout):
    """first step + three replays; the captured step has one kernel node fewer"""
    train, optim, G = pkg('train'), pkg('optim'), pkg('graph')
    ops = bf16
    runs = {}
    for sw in (False, True):
        monkeypatch.setattr(ops, 'WGRAD_ONE_LAUNCH', sw)
        model = _model(dev, order, d, dropout)
        reseed(5)
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model)
        data = _batches(order)
        (mg0,), l0 = data[0]
        step = G.GraphedTrainStep(model, opt, [mg0.to(dev)], l0.to(dev))
        losses = [step([mg.to(dev)], lab.to(dev)).item() for (mg,), lab in data]
        step.check()
        nodes = step.node_counts()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        runs[sw] = ((losses, grads, {k: p.detach().clone() for k, p in model.named_parameters()}), nodes['kernel'] if nodes else None)
        assert ops.STEP.products_waiting() == 0
    _same(runs[False][0], runs[True][0])
    if runs[False][1] is not None:
        assert runs[True][1] == runs[False][1] - 1, (runs[False][1], runs[True][1])


@pytest.mark.gpu
def test_order_1_has_no_taker_and_finish_launches(dev, bf16, monkeypatch):
    ops = bf16
    spy = Spy(monkeypatch, ops)
    off = _eager(dev, ops, False, 1, 64, 0.1)
    on = _eager(dev, ops, True, 1, 64, 0.1)
    assert len(spy.calls) == 2 and all(nA > 0 and nB == 0 for nA, nB in spy.calls), spy.calls
    _same(off, on)


@pytest.mark.gpu
def test_two_layers_wait_and_one_fits(dev, bf16, monkeypatch):
    """order 3, two layers: two lists wait, one fits beside the GRUs' 4; the other leaves on its own in front"""
    ops = bf16
    spy = Spy(monkeypatch, ops)
    off = _eager(dev, ops, False, 3, 64, 0.1, layers=2, steps=1)
    on = _eager(dev, ops, True, 3, 64, 0.1, layers=2, steps=1)
    (n1, b1), (n2, b2) = spy.calls
    assert b1 == 0 and b2 == 4 and n1 == n2 and 2 * n1 + 4 > ops.G16_MAXP >= n1 + 4, spy.calls
    _same(off, on)


@pytest.mark.gpu
def test_second_backward_before_the_step_waits_for_nothing(dev, bf16, monkeypatch):
    """p.grad is set: AccumulateGrad would ADD an unwritten buffer, so the layer launches on the spot (ops.can_defer)"""
    ops = bf16
    seen = []
    defer = ops.STEP.defer_product
    monkeypatch.setattr(ops.STEP, 'defer_product', lambda probs, keep=None, ok=True: (seen.append(len(probs)), defer(probs, keep, ok))[1])
    spy = Spy(monkeypatch, ops)
    off = _eager(dev, ops, False, 3, 64, 0.0, steps=1, twice=True)
    on = _eager(dev, ops, True, 3, 64, 0.0, steps=1, twice=True)
    # first backward: the layer waits and rides; second backward: it never asks, the GRUs launch alone
    assert len(seen) == 1 and spy.calls == [(seen[0], 4), (0, 4)], (seen, spy.calls)
    _same(off, on)
