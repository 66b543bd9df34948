"""CPU: the float64 oracle of the item-table optimizer pass (tests/table_oracle.py) pinned to torch itself, so that
tests/test_table_step_gpu.py compares the HIP kernels with what torch means and not with a second hand-written guess; and
the fp32 restatement that sets the GPU tolerances checked on every chosen case."""
import pytest
import torch

import table_oracle as O

F64 = torch.float64


def test_adam_step64_is_torch_adam():
    """5 steps of torch.optim.Adam (coupled L2) in float64, lr changed after the second"""
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(37, 20, generator=g, dtype=F64)
    for wd in (0.0, 0.1):
        q = p0.clone().requires_grad_()
        opt = torch.optim.Adam([q], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for t in range(1, 6):
            lr = 3e-3 if t <= 2 else 7e-4
            opt.param_groups[0]['lr'] = lr
            gr = torch.randn(37, 20, generator=g, dtype=F64) * 1e-2
            q.grad = gr.clone()
            opt.step()
            p, m, v = O.adam_step64(p, gr, m, v, lr, 0.9, 0.999, 1e-8, wd, t)
            st = opt.state[q]
            for name, a, b in (('p', p, q.detach()), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
                # (atol: float64 rounding of summands of 1e-2 where b1 m and (1 - b1) g cancel)
                assert torch.allclose(a, b, rtol=1e-13, atol=1e-17), (wd, t, name, float((a - b).abs().max()))


def test_renorm64_is_embedding_renorm():
    g = torch.Generator().manual_seed(1)
    W = torch.randn(50, 24, generator=g, dtype=F64) * ((0.3 + 2.7 * torch.rand(50, 1, generator=g, dtype=F64)) / 24 ** 0.5)
    W[7] = 0.0
    nrm = W.norm(dim=1)
    assert bool((nrm > 1).any()) and bool((nrm < 1).any())
    for mn in (1.0, 0.5):
        ref = W.clone()
        torch.embedding_renorm_(ref, torch.arange(50), mn, 2.0)
        assert torch.allclose(O.renorm64(W, mn), ref, rtol=1e-14, atol=0.0)
    assert torch.equal(O.renorm64(W, 0.0), W)


@pytest.mark.parametrize('eps_mode', [0, 1])
def test_project64_is_the_autograd_gradient_of_the_row_normalisation(eps_mode):
    """y = scale E / |E| (eps_mode 0: max(|E|, eps), 1: |E| + eps); the scoring backward hands the optimizer dE = cs * dL/dy.
    With eps_mode 1 the exact derivative has 1 / (|E| (|E| + eps)^2) where the projection has 1 / (|E| + eps)^3: a relative
    eps / |E| <= 1e-10 of the radial term at these norms, inside the 1e-9 asked below."""
    g = torch.Generator().manual_seed(2 + eps_mode)
    E = (torch.randn(40, 16, generator=g, dtype=F64) * 0.3).requires_grad_()
    gy = torch.randn(40, 16, generator=g, dtype=F64)
    n = E.norm(dim=1, keepdim=True)
    y = O.CS_SCALE * E / (n.clamp(min=O.CS_EPS) if eps_mode == 0 else n + O.CS_EPS)
    want, = torch.autograd.grad(y, E, gy)
    cs = O.cs64(E, O.CS_SCALE, eps_mode, O.CS_EPS)
    assert torch.allclose(cs, O.CS_SCALE / E.detach().norm(dim=1), rtol=1e-10)
    got = O.project64(E, cs, 1.0 / O.CS_SCALE, cs.unsqueeze(1) * gy)
    assert torch.allclose(got, want, rtol=1e-9, atol=1e-12), float((got - want).abs().max())


def test_projection_plus_lookup_is_autograd_of_scoring_plus_lookup():
    """loss = scoring(scale E / |E|) + lookup(E): the table gradient is proj(dE) + l, the order table_step64 composes"""
    g = torch.Generator().manual_seed(4)
    n, d, B = 30, 12, 9
    E = (torch.randn(n, d, generator=g, dtype=F64) * 0.4).requires_grad_()
    sr = torch.randn(B, d, generator=g, dtype=F64)
    labels = torch.randint(0, n, (B,), generator=g)
    idx = torch.randint(0, n, (25,), generator=g)
    wl = torch.randn(25, d, generator=g, dtype=F64)
    y = O.CS_SCALE * torch.nn.functional.normalize(E, dim=1, eps=O.CS_EPS)
    y.retain_grad()
    loss = torch.nn.functional.cross_entropy(sr @ y.t(), labels) + (E[idx] * wl).sum()
    loss.backward()
    cs = O.cs64(E, O.CS_SCALE, 0, O.CS_EPS)
    dE = cs.unsqueeze(1) * y.grad                               # the unprojected scoring gradient
    items, inv = torch.unique(idx, return_inverse=True)
    order = torch.argsort(inv, stable=True)
    ptr = torch.zeros(items.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.bincount(inv, minlength=items.numel()).cumsum(0)
    l = O.lookup_sum64(wl, items, ptr, order, n, d)
    got = O.project64(E, cs, 1.0 / O.CS_SCALE, dE) + l
    assert torch.allclose(got, E.grad, rtol=1e-10, atol=1e-13), float((got - E.grad).abs().max())
    # and table_step64 feeds exactly that sum to Adam
    z = torch.zeros(n, d, dtype=F64)
    out = O.table_step64(E, z, z, dE, l, O.ADAM, 1, 0, 1.0, 1, O.CS_SCALE, 0, O.CS_EPS, proj_cs=cs, proj_inv_scale=1.0 / O.CS_SCALE)
    p, m, v = O.adam_step64(E, E.grad, z, z, O.ADAM['lr'], O.ADAM['b1'], O.ADAM['b2'], O.ADAM['eps'], 0.0, 1)
    assert torch.allclose(out['M'], m, rtol=1e-9, atol=1e-15)
    assert torch.allclose(out['W'], O.renorm64(p, 1.0), rtol=1e-9)
    assert torch.allclose(out['cs'], O.cs64(O.renorm64(p, 1.0), O.CS_SCALE, 0, O.CS_EPS), rtol=1e-9)


def test_table_step64_renorm_write_and_bf16_copy():
    c = O.ROWS_CASES[20]
    x = O.make_rows_inputs(c)
    a = O.table_step64(x['W'], x['M'], x['V'], x['G'], None, O.ADAM, 3, 1, 1.0, 0, O.CS_SCALE, 0)
    b = O.table_step64(x['W'], x['M'], x['V'], x['G'], None, O.ADAM, 3, 1, 1.0, 1, O.CS_SCALE, 0)
    p, _, _ = O.adam_step64(x['W'], x['G'], x['M'], x['V'], t=3, **O.ADAM)
    assert torch.equal(a['W'], p) and torch.equal(b['W'], O.renorm64(p, 1.0)) and torch.equal(a['cs'], b['cs'])
    assert float(b['W'].norm(dim=1).max()) <= 1.0 and float(a['W'].norm(dim=1).max()) > 1.5
    zrow, _ = O.special_rows(c.n)
    assert float(a['W'][zrow].abs().max()) == 0.0 and float(a['cs'][zrow]) == O.CS_SCALE / O.CS_EPS
    c16 = O.bf16_copy(x['W'], 384)
    assert c16.shape == (c.n, 384) and torch.equal(c16[:, :256], x['W'].bfloat16()) and float(c16[:, 256:].abs().max()) == 0.0


def test_case_table_covers_what_the_issue_lists():
    cs = O.ROWS_CASES
    assert 38 <= len(cs) <= 45
    assert {c.d for c in cs} == {4, 32, 96, 100, 256, 516, 1024, 1028, 1280}
    for d in {c.d for c in cs}:
        assert 777 in {c.n for c in cs if c.d == d}
    assert {c.n for c in cs} == {1, 2, 3, 5, 777} and {c.t for c in cs} == {1, 2, 1000}
    for path in (lambda c: c.d <= 1024, lambda c: c.d > 1024):
        sub = [c for c in cs if path(c)]
        assert {(c.mn, c.rw) for c in sub} == {(0.0, 0), (0.0, 1), (1.0, 0), (1.0, 1)}
        assert {c.cs for c in sub} == {None, 0, 1} and {c.wd for c in sub} == {0, 1} and {c.pad for c in sub} == {0, 4}
        assert any(c.mn == 0 and c.cs is None for c in sub) and any(c.mn > 0 and c.rw and c.cs is None for c in sub)
    assert all(c.dp is None for c in cs if c.d > 1024)
    assert {c.dp for c in cs if c.d <= 1024} == {None, 'd', '128'}
    assert any(O.case_Dp(c) > c.d for c in cs if c.dp)


@pytest.mark.parametrize('proj', [False, True], ids=['rows', 'proj'])
def test_fp32_restatement_stays_inside_its_own_bound(proj, capsys):
    """every chosen case of (a) and (b): the fp32 restatement is finite, inside bound() of itself, and - the sanity of the
    yardstick - on the scale of its row no element of the restatement is off by 64 ulp, and no element that cancelled to ~0 by
    a whole ulp of its row's largest.  Prints the table that the GPU module's docstring quotes (pytest -s)."""
    worst = {}
    for i in (O.PROJ_CASES if proj else range(len(O.ROWS_CASES))):
        c = O.ROWS_CASES[i]
        ref, e32, x = O.rows_case_errors(c, proj)
        nrm = x['W'].double().norm(dim=1)
        if c.n >= 5 and c.mn > 0:
            assert bool((nrm > c.mn).any()) and bool((nrm < c.mn).any()), 'norms on both sides of max_norm'
        for k, (e, er) in e32.items():
            assert e == e and e <= O.bound(e) and er == er and er <= O.bound(er), (O.case_id(c), k, e, er)
            worst[k] = (max(worst.get(k, (0.0, 0.0))[0], e), max(worst.get(k, (0.0, 0.0))[1], er))
        print('%2d %-44s %s' % (i, O.case_id(c), '  '.join('%s %.1e/%.1e' % (k, e[0], e[1]) for k, e in sorted(e32.items()))))
    print('worst', {k: 'rel %.2e -> bound %.2e, row-scaled %.2e -> bound %.2e' % (e[0], O.bound(e[0]), e[1], O.bound(e[1]))
                    for k, e in worst.items()})
    for k, (e, er) in worst.items():
        assert e < 1.0 and er < 64 * O.ULP, (k, e, er)
