"""CPU: the harness of tests/test_score_ce_gpu.py has teeth.  The emulation of the bf16 scoring kernels' rounding
(tests/ce_oracle.py: bf16 operands, fp32 logits and lse, P rounded once to bf16, fp32 products) stays inside the element-wise
bound on every case of the shared table, and each seeded wrong variant of it leaves the bound somewhere; the float64 oracle
itself is pinned to torch's autograd."""
import pytest
import torch

import ce_oracle as O

F64 = torch.float64


def _emulate(D, **kw):
    return O.emulate(D.sr, D.E, D.cs, D.labels, D.ga * D.gscale, D.gc * D.gscale, D.live, **kw)


def test_exact_is_the_autograd_gradient_of_torch_cross_entropy():
    """plain CE and a function of (lse, label logit) with per-session coefficients, float64 autograd on the rounded operands"""
    for name in ('template-d36', 'coef-g-gscale-d64', 'dyn-live77', 'labels-neg'):
        D, ex = O.reference(name)
        live = D.live
        sr = O.bf16r(D.sr)[:live].requires_grad_()
        E = O.bf16r(D.E).requires_grad_()
        cs = torch.ones(D.E.shape[0], dtype=F64) if D.cs is None else D.cs.to(F64)
        z = (sr @ E.t()) * cs
        lse = torch.logsumexp(z, 1)
        has = D.labels[:live] >= 0
        lab = torch.where(has, z.gather(1, D.labels[:live].clamp(min=0)[:, None])[:, 0], torch.zeros((), dtype=F64))
        obj = D.gscale * ((D.ga[:live] * lse).sum() - (D.gc[:live] * lab).sum())
        dsr, dE = torch.autograd.grad(obj, [sr, E])
        assert torch.allclose(ex.lse[:live], lse.detach(), rtol=1e-13, atol=1e-13)
        assert torch.allclose(ex.lab[:live], lab.detach(), rtol=1e-13, atol=1e-13)
        assert abs(ex.loss - float((lse - lab).detach().mean())) <= 1e-12 * abs(ex.loss)
        assert torch.allclose(ex.dsr[:live], dsr, rtol=1e-11, atol=1e-15), name
        assert torch.allclose(ex.dE, dE, rtol=1e-11, atol=1e-15), name
        assert not ex.dsr[live:].any()
        assert bool((ex.bound_dE >= ex.dE.abs() * (1 - 1e-12)).all()) and bool((ex.bound_dsr >= ex.dsr.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize('name', [c.name for c in O.CASES])
def test_emulation_within_bound(name):
    D, ex = O.reference(name)
    em = _emulate(D)
    O.check_forward(em.lse, em.lab, em.loss, ex, D.live, name)
    r1 = O.check_grad(em.dE, ex.dE, ex.bound_dE, name + ' dE')
    r2 = O.check_grad(em.dsr, ex.dsr, ex.bound_dsr, name + ' dsr')
    print('%s: error / (u bound): dE %.3f dsr %.3f' % (name, r1, r2))


def test_emulated_accumulation_within_summed_bound():
    D1, e1 = O.reference('coef-g-d36')
    D2 = O.make('coef-g-d36', seed_extra=1)
    D2 = D2._replace(E=D1.E, cs=D1.cs)
    e2 = O.exact(D2.sr, D2.E, D2.cs, D2.labels, D2.ga, D2.gc, D2.live)
    h1 = _emulate(D1)
    h2 = _emulate(D2, dE_prev=h1.dE)
    O.check_grad(h2.dE, e1.dE + e2.dE, e1.bound_dE + e2.bound_dE, 'two heads')


# which case shows which fault (a fault that needs live < B, a ragged tail or ga != gc runs where there is one)
FAULT_CASES = {
    'item_tail_dropped': ('template-d32', 'tail-V33', 'split2'),
    'session_tail_dropped': ('template-d64', 'tail-B33', 'dyn-live77'),
    'session_zeroed': ('template-d256', 'split2', 'coef-g-d64'),
    'onehot_missing': ('template-d32', 'split2', 'coef-g-gscale-d36'),
    'onehot_at_label_plus_1': ('template-d100', 'labels-edges'),
    'ga_gc_exchanged': ('coef-g-d64', 'coef-g-gscale-d36', 'split2-ragged-live500'),
    'mean_over_B': ('dyn-live77', 'split2-ragged-live600'),
    'dead_session_contributes': ('dyn-live77', 'dyn-live0', 'split2-ragged-live600'),
    'rows_exchanged_in_chunk': ('template-d32', 'tail-B33'),
    'accumulate_overwrites': ('coef-g-d36', 'split2'),
}
assert set(FAULT_CASES) == set(O.FAULTS)


@pytest.mark.parametrize('fault,name', [(f, n) for f in O.FAULTS for n in FAULT_CASES[f]])
def test_seeded_fault_exceeds_bound(fault, name):
    D, ex = O.reference(name)
    want, bound, prev = ex.dE, ex.bound_dE, None
    if fault == 'accumulate_overwrites':
        D0 = O.make(name, seed_extra=1)
        e0 = O.exact(D0.sr, D.E, D.cs, D0.labels, D0.ga * D0.gscale, D0.gc * D0.gscale, D0.live)
        prev = O.emulate(D0.sr, D.E, D.cs, D0.labels, D0.ga * D0.gscale, D0.gc * D0.gscale, D0.live).dE
        want, bound = want + e0.dE, bound + e0.bound_dE
        O.check_grad(_emulate(D, dE_prev=prev).dE, want, bound, 'clean accumulation')
    em = _emulate(D, dE_prev=prev, fault=fault)
    rE, badE = O.grad_error(em.dE, want, bound)
    rS, badS = O.grad_error(em.dsr, ex.dsr, ex.bound_dsr)
    print('%s at %s: error / (u bound): dE %.3g (%d elements out) dsr %.3g (%d)' % (fault, name, rE, badE, rS, badS))
    assert badE + badS > 0 and max(rE, rS) > O.FACTOR
