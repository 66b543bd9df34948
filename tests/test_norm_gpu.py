"""Renormalisation of the served scores on the GPU: csrc/score_norm.hip through ops.score_norm, dist.VocabParallel.norm,
model.log_mass and the `renormalize=` keyword of model.recommend / score_items / rerank, and the launchers' --renormalize,
against a float64 logsumexp over the eligible columns of the materialised scores (tests/norm_oracle.py).

The bounds: counting inputs 1e-5 (one missed or doubled item of at most 3001 moves Z by at least 1 / 3001 = 3e-4; fp32
round-off at |Z| < 9 is below 2e-6); exact inputs 2e-5 (half an ulp of |Z| < 128 for the final add, 3.8e-6, plus a relative
error of l below 60 * 2^-24 = 3.6e-6 - chains of at most ceil(V / 128) + 12 adds, expf within 2 ulp - plus logf, doubled);
random inputs the project's TOL = 1e-4; the models 2e-4, the difference of two quantities each held to 1e-4.

On the exact inputs one item usually holds most of a session's mass, so the bias moves Z by about the bias of that item: on
every case more than three quarters of the sessions move by more than 0.05 (asserted from the oracle), not every session -
the smallest movement over all cases is 5e-4 - so a kernel that dropped the bias fails the 2e-5 bound on most sessions."""
import math
import os
import subprocess
import sys

import pytest
import torch

from item_bias_oracle import NINF, bias_rows, exact_bias
from norm_oracle import eligible, lse_pair64, norm64
from select_oracle import drop_mask, exact_case, scores64
from test_item_bias_gpu import _groups, _mixture_case, _random_bias, _seen
from test_select_gpu import _random_case
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ops():
    return pkg('ops')


def _t(dev):
    return lambda x: None if x is None else x.to(dev)


def _close(z, ref, tol, what):
    """|z - ref| < tol on the finite entries, the -inf entries equal, no NaN anywhere; -> the largest error"""
    assert z.dtype == torch.float32 and z.shape == ref.shape, (what, z.dtype, z.shape, ref.shape)
    z = z.cpu().double()
    assert not bool(torch.isnan(z).any()), (what, 'NaN', z.tolist()[:8])
    fin = torch.isfinite(ref)
    assert torch.equal(z[~fin], ref[~fin]), (what, 'the infinite entries differ', z[~fin].tolist()[:8], ref[~fin].tolist()[:8])
    err = float((z[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(what, 'max |Z - oracle| %.2e over %d finite sessions, %d at -inf' % (err, int(fin.sum()), int((~fin).sum())))
    assert err < tol, (what, err, tol)
    return err


# ------------------------------------------------------------------------------------------- 1) counting
def _counting_case(B, V, d=32):
    sr = torch.zeros(B, d)
    sr[:, 0] = 1.0
    E = torch.zeros(V, d)
    E[:, 0], E[:, 1] = 0.5, 1.0                          # every score is 0.5 (column 1 is orthogonal to the sessions)
    return sr, E


def _counting_bias(V, G=None, seed=0):
    """0 / -inf: -inf on a random third of the ids, on the whole chunk 128 .. 255 and - at V = 3000, where a workgroup owns
    256 rows - on the whole workgroup range 512 .. 767"""
    g = torch.Generator().manual_seed(V + seed)
    shape = (V,) if G is None else (G, V)
    b = torch.zeros(shape)
    b[torch.rand(shape, generator=g) < 1 / 3] = NINF
    b[..., 128:256] = NINF
    if V == 3000:
        b[..., 512:768] = NINF
    return b


@pytest.mark.parametrize('B', [5, 33])
@pytest.mark.parametrize('V', [1, 20, 127, 129, 3000])
def test_counting_every_eligible_item_once(dev, B, V):
    ops, t = _ops(), _t(dev)
    sr, E = _counting_case(B, V)
    g = torch.Generator().manual_seed(B + V)
    L = min(6, V)
    listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])
    listed[:, L - 1] = -1
    for G in (None, 3):
        bias = _counting_bias(V, G)
        group = None if G is None else _groups(B, G)
        for lst in (None, listed):
            dm = None if lst is None else drop_mask(lst, V)
            n = eligible(B, V, bias, group, dm).sum(1).double()
            want = torch.where(n > 0, 0.5 + torch.log(n.clamp(min=1)), torch.full_like(n, NINF))
            z = ops.score_norm(sr.to(dev), E.to(dev), None, listed=t(lst), drop_listed=lst is not None, bias=bias.to(dev),
                               group=t(group))
            _close(z, want, 1e-5, 'counting B %d V %d G %s %s: %s eligible' % (B, V, G, 'drop' if lst is not None else 'plain',
                                                                              sorted(set(n.long().tolist()))[:4]))
    # no bias at all: every item counts
    z = ops.score_norm(sr.to(dev), E.to(dev), None)
    _close(z, torch.full((B,), 0.5 + math.log(V), dtype=torch.float64), 1e-5, 'counting B %d V %d no bias' % (B, V))


# ------------------------------------------------------------------------------------------- 2) dominance and emptiness
def test_one_dominant_item_gives_its_score_exactly(dev):
    ops = _ops()
    B, V, d = 33, 3000, 32
    sr, E = _counting_case(B, V, d)
    E[:, 0] = -200.0 - (torch.arange(V) % 5).float()      # expf(-90) and below is exactly 0 beside 1 in fp32
    E[777, 0], E[1500, 0] = 0.0, -110.0
    z = ops.score_norm(sr.to(dev), E.to(dev), None)
    assert z.dtype == torch.float32 and bool((z == 0.0).all()), z.tolist()[:8]
    # the dominant item leaves the catalogue, the next one (score -110, boosted by 0.5) takes over
    bias = torch.zeros(V)
    bias[777], bias[1500] = NINF, 0.5
    z = ops.score_norm(sr.to(dev), E.to(dev), None, bias=bias.to(dev))
    assert bool((z == -109.5).all()), z.tolist()[:8]
    # ... or is dropped for the sessions that list it
    listed = torch.full((B, 3), -1)
    listed[::2, 1] = 777
    z = ops.score_norm(sr.to(dev), E.to(dev), None, listed=listed.to(dev), drop_listed=True).cpu()
    assert bool((z[::2] == -110.0).all()) and bool((z[1::2] == 0.0).all()), z.tolist()[:8]
    # ... or scores through off_in there: 0 + 300
    off_in = torch.full((1, B), 300.0)
    z = ops.score_norm(sr.to(dev), E.to(dev), None, None, off_in.to(dev), listed.to(dev)).cpu()
    assert bool((z[::2] == 300.0).all()) and bool((z[1::2] == 0.0).all()), z.tolist()[:8]


def test_sessions_without_an_eligible_item_give_minus_infinity(dev):
    ops = _ops()
    B, V, d = 5, 20, 32
    sr, E, cs = exact_case(B, V, d)
    sr, E, cs = sr.to(dev), E.to(dev), cs.to(dev)
    none = torch.full((V,), NINF)
    z = ops.score_norm(sr, E, cs, bias=none.to(dev)).cpu()
    assert z.tolist() == [NINF] * B
    # one of three groups empty
    bias3 = torch.stack([torch.zeros(V), none, exact_bias(V, off_ranges=())])
    group = torch.tensor([0, 1, 2, 1, 0])
    z = ops.score_norm(sr, E, cs, bias=bias3.to(dev), group=group.to(dev))
    ref = norm64(scores64(sr, E, cs), bias3, group)
    assert ref[1] == NINF and ref[3] == NINF and bool(torch.isfinite(ref[[0, 2, 4]]).all())
    _close(z, ref, 2e-5, 'group 1 empty')
    # V < 128 and everything dropped
    listed = torch.arange(V)[None].expand(B, V).contiguous()
    z = ops.score_norm(sr, E, cs, listed=listed.to(dev), drop_listed=True).cpu()
    assert z.tolist() == [NINF] * B
    # a large catalogue (several ranges) with nothing in it, and with one item in the last chunk
    Bb, Vb = 33, 3000
    srb, Eb = _counting_case(Bb, Vb)
    allout = torch.full((Vb,), NINF)
    z = ops.score_norm(srb.to(dev), Eb.to(dev), None, bias=allout.to(dev)).cpu()
    assert bool((z == NINF).all())
    allout[Vb - 1] = 0.25
    z = ops.score_norm(srb.to(dev), Eb.to(dev), None, bias=allout.to(dev)).cpu()
    assert bool((z == 0.75).all()), z.tolist()[:8]


# ------------------------------------------------------------------------------------------- 3) exact inputs on every path
def _moves(z64, z0, what):
    """the bias matters: see the module docstring"""
    share = float(((z64 - z0).abs() > 0.05).double().mean())
    print(what, 'sessions with |Z - Z_unbiased| > 0.05: %.2f, smallest movement %.1e' % (share, float((z64 - z0).abs().min())))
    assert share > 0.75, (what, share)


@pytest.mark.parametrize('G', [None, 3])
@pytest.mark.parametrize('B,V,d', [(5, 300, 32), (33, 5000, 96), (40, 3429, 64)])
def test_exact_inputs_within_the_summation_bound(dev, B, V, d, G):
    ops, t = _ops(), _t(dev)
    sr, E, cs = exact_case(B, V, d)
    bias = exact_bias(V, G, off_ranges=((128, 256), (512, 1024)) if V == 5000 else ((128, 256),))
    group = None if G is None else _groups(B, G)
    for scale in (cs, None):
        s64 = scores64(sr, E, scale)
        ref = norm64(s64, bias, group)
        assert float(ref.abs().max()) < 128
        z = ops.score_norm(sr.to(dev), E.to(dev), t(scale), bias=bias.to(dev), group=t(group))
        what = 'exact %s G %s %s' % ((B, V, d), G, 'cs' if scale is not None else 'no cs')
        _close(z, ref, 2e-5, what)
        _moves(ref, norm64(s64), what)
        _close(ops.score_norm(sr.to(dev), E.to(dev), t(scale)), norm64(s64), 2e-5, what + ', no bias')


@pytest.mark.parametrize('B,V,d,C,L', [(37, 700, 100, 2, 5), (33, 700, 256, 3, 64), (33, 500, 1024, 1, 5), (40, 600, 512, 4, 5),
                                       (33, 500, 1024, 2, 5)])
def test_exact_mixtures_on_every_kernel_path(dev, B, V, d, C, L):
    """session tiles in LDS (the first three: C = 1 at d = 1024 still fits) and through the cache (the last two), C = 1 .. 4,
    one bias row and G = 2 - without a list, with a scored and with a dropped one"""
    ops, t = _ops(), _t(dev)
    srs, E, cs, off, off_in, listed = _mixture_case(B, V, d, C, L)
    for G in (None, 2):
        bias = exact_bias(V, G, seed=C)
        group = None if G is None else _groups(B, G)
        for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
            z = ops.score_norm(srs.to(dev), E.to(dev), cs.to(dev), off.to(dev), t(oi), t(lst), drop_listed=drop,
                               bias=bias.to(dev), group=t(group))
            if drop:
                s64, dm = scores64(srs, E, cs, off), drop_mask(listed, V)
            else:
                s64, dm = scores64(srs, E, cs, off, oi, lst), None
            ref = norm64(s64, bias, group, dm)
            assert float(ref.abs().max()) < 128
            name = 'mixture %s G %s %s' % ((B, V, d, C, L), G, what)
            _close(z, ref, 2e-5, name)
            _moves(ref, norm64(s64, None, None, dm), name)


# ------------------------------------------------------------------------------------------- 4) random inputs
@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed-score', 'listed-drop'])
@pytest.mark.parametrize('B,V,d', [(33, 5000, 96), (40, 3429, 64)])
def test_random_inputs_within_tol(dev, B, V, d, kind):
    ops, t = _ops(), _t(dev)
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    G = None if kind == 'single' else 4
    bias, group = _random_bias(V, G, B + V), (None if G is None else _groups(B, G))
    drop = kind == 'listed-drop'
    z = ops.score_norm([s.to(dev) for s in srs], t(E), t(cs), t(off_ex), t(off_in), t(listed), drop_listed=drop,
                       bias=bias.to(dev), group=t(group))
    if drop:
        s64, dm = scores64(srs, E, cs, off_ex), drop_mask(listed, V)
    else:
        s64, dm = scores64(srs, E, cs, off_ex, off_in, listed), None
    ref = norm64(s64, bias, group, dm)
    _close(z, ref, TOL, 'random %s %s' % (kind, (B, V, d)))
    # the bias, and the listed items' treatment, matter far beyond TOL
    assert float((ref - norm64(s64, None, None, dm)).abs().min()) > 100 * TOL
    if listed is not None:
        other = norm64(scores64(srs, E, cs, off_ex), bias, group)
        assert float((ref - other).abs().max()) > 10 * TOL


# ------------------------------------------------------------------------------------------- 5) views and shards
def test_bias_views_two_row_ranges_and_repeated_calls(dev):
    ops = _ops()
    B, V, d, G = 33, 5000, 96, 3
    sr, E, cs = exact_case(B, V, d)
    bias = exact_bias(V, G, seed=7, off_ranges=((128, 256), (2400, 2600)))
    group = _groups(B, G)
    g = torch.Generator().manual_seed(7)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    s64 = scores64(sr, E, cs)
    sr, E, cs, listed_d, group_d = sr.to(dev), E.to(dev), cs.to(dev), listed.to(dev), group.to(dev)
    wide = torch.full((G, 2 * V), 99.0, device=dev)
    wide[:, V:] = bias.to(dev)
    view = wide[:, V:]                                    # a column slice of a [G, 2V] tensor: row stride 2V
    assert view.stride() == (2 * V, 1) and not view.is_contiguous()
    for kw in (dict(), dict(listed=listed_d, drop_listed=True)):
        dm = drop_mask(listed, V) if kw else None
        whole = ops.score_norm(sr, E, cs, bias=view, group=group_d, **kw)
        assert torch.equal(whole, ops.score_norm(sr, E, cs, bias=view.contiguous(), group=group_d, **kw))
        assert torch.equal(whole, ops.score_norm(sr, E, cs, bias=view, group=group_d, **kw))       # a repeated call: equal bits
        _close(whole, norm64(s64, bias, group, dm), 2e-5, 'whole table, bias view')
        # two row ranges: each takes its columns of the bias (again a view) and its id_lo
        lo = ops.score_norm(sr, E[:2500], cs[:2500], id_lo=0, bias=view[:, :2500], group=group_d, **kw)
        hi = ops.score_norm(sr, E[2500:], cs[2500:], id_lo=2500, bias=view[:, 2500:], group=group_d, **kw)
        _close(lo, norm64(s64[:, :2500], bias, group, None if dm is None else dm[:, :2500], 0), 2e-5, 'rows [0, 2500)')
        _close(hi, norm64(s64[:, 2500:], bias, group, None if dm is None else dm[:, 2500:], 2500), 2e-5, 'rows [2500, 5000)')
        both = lse_pair64(lo, hi)
        err = float((both - whole.cpu().double()).abs().max())
        print('two row ranges against the whole table: %.2e' % err)
        assert err < 2e-5
    # the dropped list matters for the shard that owns the ids
    assert not torch.equal(whole, ops.score_norm(sr, E, cs, bias=view, group=group_d))


def test_norm_scratch_stays_out_of_the_evaluation_kernels_cache(dev):
    """score_norm at shape A, shape B, then A again repeats A's bits, and its partials live in their own cache: the one
    score_topk / score_rank / score_select share (tests/test_select_gpu.py pins its kinds) gains no entry"""
    ops, score = _ops(), pkg('score')
    g = torch.Generator().manual_seed(11)
    a = (torch.randn(3, 32, generator=g).to(dev), torch.randn(300, 32, generator=g).to(dev))
    b = (torch.randn(130, 64, generator=g).to(dev), torch.randn(1000, 64, generator=g).to(dev))
    before = set(score._BYTE_WS)
    first = ops.score_norm(*a, None)
    ops.score_norm(*b, None)
    assert torch.equal(ops.score_norm(*a, None), first)
    assert set(score._BYTE_WS) == before and {k[0] for k in score._NORM_WS} == {'norm'}
    assert len({k for k in score._NORM_WS if k[1] == dev.index}) >= 2


# ------------------------------------------------------------------------------------------- 6) sharded, W = 2 on one GPU
def test_sharded_norm_and_renormalized_recommend_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from item_bias_gpu_worker import sharded_bias
    from norm_gpu_worker import identity_model, run_rank
    from select_gpu_worker import K, sharded_case
    from test_dist_gpu import _free_port
    world = 2
    ctx = mp.get_context('spawn')
    port = _free_port()
    procs = [ctx.Process(target=run_rank, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for p in procs:                  # each rank under its own time limit; stop at the first one that did not end well
            p.join(timeout=240)
            assert p.exitcode == 0, 'rank process ended with %r' % (p.exitcode,)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    ops = _ops()
    sr, E, cs, listed = sharded_case()
    bias, group = sharded_bias()
    V = E.shape[0]
    s64 = scores64(sr, E, cs)
    model = identity_model(E).to(dev)
    sr, E, cs, listed_d, bias_d, group_d = [x.to(dev) for x in (sr, E, cs, listed, bias, group)]
    want = dict(norm=ops.score_norm(sr, E, cs, bias=bias_d, group=group_d).cpu(),
                norm_plain=ops.score_norm(sr, E, cs).cpu(),
                norm_drop=ops.score_norm(sr, E, cs, listed=listed_d, drop_listed=True, bias=bias_d, group=group_d).cpu())
    want['norm_routed'] = want['norm']
    _close(want['norm_drop'], norm64(s64, bias, group, drop_mask(listed, V)), 2e-5, 'single device, dropped list')
    _close(want['norm'], norm64(s64, bias, group), 2e-5, 'single device')
    rv, ri = [x.cpu() for x in model.recommend(sr, k=K, item_bias=bias_d, item_group=group_d, renormalize=True)]
    lm = model.log_mass(sr, item_bias=bias_d, item_group=group_d).cpu()
    n = sr.shape[0] // world
    res = [torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r)) for r in range(world)]
    for r in range(world):
        assert res[r]['hi'] - res[r]['lo'] == res[r]['n_live'] and (r == 0 or res[r]['n_live'] < res[r]['rows'])
        for key, w in want.items():                       # every rank feeds the same sessions: the full answer on every rank
            z = res[r][key]
            assert z.dtype == torch.float32 and torch.equal(z, res[0][key]), (r, key, 'the ranks hold different bits')
            err = float((z.double() - w.double()).abs().max())
            print('rank', r, key, 'against the single device: %.2e' % err)
            assert err < 2e-5, (r, key, err)
        # every rank feeds its own slice, with its own list width and its own group ids: its own sessions' results
        mine = slice(r * n, (r + 1) * n)
        assert float((res[r]['norm_dp'].double() - want['norm'][mine].double()).abs().max()) < 2e-5, r
        assert torch.equal(res[r]['norm_dp'], res[r]['norm'][mine]), r        # the same fold of the same gathered values
        w = ops.score_norm(sr[mine], E, cs, listed=listed_d[mine, :4 + r], drop_listed=True, bias=bias_d, group=group_d[mine]).cpu()
        assert float((res[r]['norm_dp_drop'].double() - w.double()).abs().max()) < 2e-5, r
        # the model over the sharded table: the ids of one device, values within 2e-4
        sv, si = res[r]['recommend']
        assert si.dtype == torch.int32 and torch.equal(si, ri), r
        assert float((sv.double() - rv.double()).abs().max()) < 2e-4, r
        assert float((res[r]['log_mass'].double() - lm.double()).abs().max()) < 2e-4, r
    assert torch.equal(res[0]['recommend'][0], res[1]['recommend'][0])
    # renormalised: over the eligible catalogue the returned head is a part of a distribution
    assert bool((rv.double().exp().sum(1) <= 1 + 1e-3).all()) and bool((ri >= 0).all())


# ------------------------------------------------------------------------------------------- 7) models
@pytest.mark.parametrize('name', ['srgnn_s32', 'niser_s32', 'lessr_L3_s32', 'msgifsr_K3_ext_fus_s32'])
def test_models_renormalize_and_log_mass_against_forward(dev, name, monkeypatch):
    from test_items_gpu import _model_candidates
    from test_rank_gpu import _fixture_model
    from util import load_golden
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()             # forward()'s log-probabilities, materialised
    B, V = s64.shape
    seen = _seen(samples, V)
    items = _model_candidates(samples, labels, V, len(name))
    every = torch.arange(V)
    lib = pkg('_lib').lib

    def never(*a, **k):
        raise AssertionError('a pass ran that this call must not launch')

    # nothing to renormalise: the call of renormalize=False, bit for bit, and no norm pass
    plain = model.recommend(*inputs, k=20)
    plain_items = model.score_items(*inputs, items=items.to(dev))
    with monkeypatch.context() as mp:
        mp.setitem(lib.__dict__, 'srec_score_norm', never)
        v, i = model.recommend(*inputs, k=20, renormalize=True)
        assert torch.equal(v, plain[0]) and torch.equal(i, plain[1])
        assert torch.equal(model.score_items(*inputs, items=items.to(dev), renormalize=True), plain_items)
        rv, ri = model.rerank(*inputs, items=items.to(dev), k=30, renormalize=True)
        wv, wi = model.rerank(*inputs, items=items.to(dev), k=30)
        assert torch.equal(rv, wv) and torch.equal(ri, wi)
    z0 = model.log_mass(*inputs).cpu().double()
    assert float(z0.abs().max()) < TOL, ('the whole catalogue holds all the mass', z0.tolist()[:6])

    model.train()
    for G in (None, 2):
        bias = _random_bias(V, G, len(name))
        group = None if G is None else _groups(B, G)
        rows = bias_rows(bias, group, B)
        kw = dict(item_bias=bias.to(dev), item_group=None if group is None else group.to(dev))
        for ex in (False, True):
            dm = seen if ex else None
            what = '%s G %s exclude_seen %s' % (name, G, ex)
            Z64 = norm64(s64, bias, group, dm)
            lm = model.log_mass(*inputs, exclude_seen=ex, **kw)
            assert model.training                       # restored
            _close(lm, Z64, TOL, what + ' log_mass')
            want = s64 + torch.where(rows == NINF, torch.zeros_like(rows), rows) - Z64[:, None]
            want[~eligible(B, V, bias, group, dm)] = NINF
            # recommend: the ids of renormalize=False, the values minus Z
            v0, i0 = model.recommend(*inputs, k=20, exclude_seen=ex, **kw)
            v1, i1 = model.recommend(*inputs, k=20, exclude_seen=ex, renormalize=True, **kw)
            assert v1.dtype == torch.float32 and i1.dtype == torch.int32 and torch.equal(i1, i0) and model.training, what
            got, ref = v1.cpu().double(), want.gather(1, i1.cpu().long().clamp(min=0))
            assert bool((i1 >= 0).all()) and bool(torch.isfinite(ref).all()), what
            err = float((got - ref).abs().max())
            print(what, 'recommend: max |value - (forward + bias - Z64)| %.2e' % err)
            assert err < 2e-4, (what, err)
            # score_items / rerank: normalised over the eligible CATALOGUE, -inf slots stay -inf
            o0 = model.score_items(*inputs, items=items.to(dev), exclude_seen=ex, **kw).cpu()
            o1 = model.score_items(*inputs, items=items.to(dev), exclude_seen=ex, renormalize=True, **kw).cpu()
            ref = torch.where(items >= 0, want.gather(1, items.clamp(min=0)), torch.full(items.shape, NINF, dtype=torch.float64))
            assert torch.equal(o1 == NINF, o0 == NINF) and torch.equal(o1 == NINF, ref == NINF), what
            fin = ref != NINF
            err = float((o1.double()[fin] - ref[fin]).abs().max())
            print(what, 'score_items: %.2e over %d slots, %d at -inf' % (err, int(fin.sum()), int((~fin).sum())))
            assert err < 2e-4 and int((~fin).sum()) > B, (what, err)
            r0 = model.rerank(*inputs, items=items.to(dev), k=30, exclude_seen=ex, **kw)
            r1 = model.rerank(*inputs, items=items.to(dev), k=30, exclude_seen=ex, renormalize=True, **kw)
            assert torch.equal(r1[1], r0[1]), what
            ref = torch.where(r1[1].cpu() >= 0, want.gather(1, r1[1].cpu().long().clamp(min=0)), torch.full(r1[1].shape, NINF, dtype=torch.float64))
            fin = ref != NINF
            assert torch.equal(r1[0].cpu() == NINF, ~fin) and float((r1[0].cpu().double()[fin] - ref[fin]).abs().max()) < 2e-4, what
            # a distribution over what can be shown
            allv = model.score_items(*inputs, items=every.to(dev), exclude_seen=ex, renormalize=True, **kw).cpu().double()
            assert torch.equal(allv == NINF, ~eligible(B, V, bias, group, dm)), what
            tot = allv.exp().sum(1)
            print(what, 'sum of exp over the eligible catalogue: %.6f .. %.6f' % (float(tot.min()), float(tot.max())))
            assert float((tot - 1).abs().max()) < 1e-3, what
    model.eval()
    if name == 'srgnn_s32':             # a single soft-max: the full-catalogue statistics pass is skipped
        with monkeypatch.context() as mp:
            mp.setattr(model, '_lse', never)
            v2, i2 = model.recommend(*inputs, k=20, exclude_seen=True, renormalize=True, **kw)
            assert torch.equal(i2, i1) and torch.equal(v2, v1)
            model.score_items(*inputs, items=items.to(dev), renormalize=True, **kw)
            with pytest.raises(AssertionError, match='must not launch'):
                model.recommend(*inputs, k=20, **kw)
    assert not model.training


def test_models_refuse_a_bad_item_bias_before_anything_runs_log_mass_included(dev, monkeypatch):
    sp = pkg()
    V = 50
    model = sp.SRGNN(V, 32, 1).to(dev).train()

    def never(*a, **k):
        raise AssertionError('something ran although the item bias is refused')
    monkeypatch.setattr(model, 'session_repr', never)
    for fn in ('score_select', 'score_items', 'score_norm'):
        monkeypatch.setattr(_ops(), fn, never)
    lib = pkg('_lib').lib
    for fn in ('srec_score_rank', 'srec_score_select', 'srec_score_sample', 'srec_score_items', 'srec_score_norm',
               'srec_score_cutoff_hist', 'srec_score_cutoff_tail', 'srec_score_cutoff'):
        monkeypatch.setitem(lib.__dict__, fn, never)
    ok = torch.zeros(V, device=dev)
    nan, pinf = ok.clone(), ok.clone()
    nan[7], pinf[9] = float('nan'), float('inf')
    grp = torch.tensor([0, 1], device=dev)
    cases = ((dict(item_bias=torch.zeros(V + 1, device=dev)), r'item_bias must be a floating tensor \[50\] or \[G, 50\]'),
             (dict(item_bias=nan), 'item_bias holds NaN or \\+inf'),
             (dict(item_bias=torch.stack([ok, pinf]), item_group=grp), 'item_bias holds NaN or \\+inf'),
             (dict(item_bias=torch.stack([ok, ok]), item_group=torch.tensor([0, 2], device=dev)), r'row id outside \[0, 2\)'),
             (dict(item_bias=torch.stack([ok, ok])), 'G > 1 needs it'),
             (dict(item_group=grp), 'item_group is given without an item_bias'))
    items = torch.tensor([[1, 2], [3, 4]], device=dev)
    for kw, msg in cases:
        with pytest.raises(ValueError, match='recommend: .*' + msg):
            model.recommend(None, k=5, renormalize=True, **kw)
        with pytest.raises(ValueError, match='score_items: .*' + msg):
            model.score_items(None, items=items, renormalize=True, **kw)
        with pytest.raises(ValueError, match='score_items: .*' + msg):
            model.rerank(None, items=items, k=2, renormalize=True, **kw)
        with pytest.raises(ValueError, match='log_mass: .*' + msg):
            model.log_mass(None, **kw)
    assert model.training                               # nothing ran, nothing was switched
    good = ok.clone()
    good[3], good[4] = NINF, -2.5
    with pytest.raises(AssertionError, match='something ran'):
        model.log_mass(None, item_bias=good)
    assert model.training                               # ... and restored after a failure inside


# ------------------------------------------------------------------------------------------- 8) launchers
def test_launchers_with_renormalize_equal_the_in_process_calls(dev, tmp_path):
    sp, col, ops = pkg(), pkg('collate'), _ops()
    sys.path.insert(0, os.path.join(ROOT, 'src', 'scripts'))
    try:
        import recommend as rec
        import rerank as rr
    finally:
        sys.path.pop(0)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    sessions = rec.read_session_file(os.path.join(GOLDEN, 'sample_test.txt'))[:40]
    g = torch.Generator().manual_seed(10)
    deny = torch.randperm(V, generator=g)[:V // 3].tolist()
    cands = [torch.randint(0, V, (150,), generator=g).tolist() + s[:2] for s in sessions]
    (tmp_path / 'sessions.txt').write_text(rec.format_sessions(sessions))
    (tmp_path / 'cands.txt').write_text(rec.format_sessions(cands))
    (tmp_path / 'deny.txt').write_text(''.join('%d\n' % i for i in deny))
    common = ['--model', 'SRGNN', '--dataset-dir', data, '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt),
              '--sessions', str(tmp_path / 'sessions.txt'), '--renormalize', '--deny', str(tmp_path / 'deny.txt')]
    top, ranked = tmp_path / 'top.txt', tmp_path / 'ranked.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py')] + common +
                       ['--top', '50', '--exclude-seen', '--output', str(top)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'rerank.py')] + common +
                       ['--candidates', str(tmp_path / 'cands.txt'), '--output', str(ranked)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    inputs = [x.to(dev) for x in inputs]
    bias = ops.catalog_bias(V, deny=deny, device=dev)
    val, idx = model.recommend(*inputs, k=50, exclude_seen=True, item_bias=bias, renormalize=True)
    raw = model.recommend(*inputs, k=50, exclude_seen=True, item_bias=bias)[0]
    assert bool(torch.isfinite(raw).all()) and float((val - raw).min()) > 0.05      # a third of the catalogue is gone: every value rises
    lines = top.read_text().splitlines()
    assert len(lines) == len(sessions)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == idx[b].tolist() and not set(ids) & set(deny) and not set(ids) & set(sessions[b]), b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
    val, idx = model.rerank(*inputs, items=torch.tensor(rr.pad_candidates(cands)).to(dev), item_bias=bias, renormalize=True)
    lines = ranked.read_text().splitlines()
    assert len(lines) == len(sessions)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        n = len(ids)
        assert n == sum(c not in set(deny) for c in cands[b]) and 0 < n < len(cands[b]), b
        assert ids == idx[b, :n].tolist() and bool((idx[b, n:] == -1).all()), b
        assert max(abs(a - c) for a, c in zip(vals, val[b, :n].tolist())) <= 1e-6, b
