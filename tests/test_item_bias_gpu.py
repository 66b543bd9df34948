"""Per-item bias and catalogue filters of the serving calls on the GPU: the biased instances of csrc/recommend.hip and
csrc/score_items.hip through ops.score_select / ops.score_items (bias=, group=), dist.VocabParallel, model.recommend /
score_items / rerank (item_bias=, item_group=) and the launchers' --allow / --deny / --item-bias, against materialised float64
scores plus the bias (tests/item_bias_oracle.py).

Exact inputs (select_oracle.exact_case; bias values multiples of 1/8 in [-2, 2], so every sum stays representable) must give
EQUAL lists and values - an item of bias -inf that enters a list, a bias row of the wrong group, a chunk or a whole workgroup
range without an eligible item and the tail rule show there.  Random inputs and the models are held to 1e-4, the fp32 bound
tests/test_select_gpu.py and tests/test_items_gpu.py use for this score, with no session left out."""
import os
import subprocess
import sys

import pytest
import torch

from item_bias_oracle import NINF, bias_rows, exact_bias, items_biased64, select_biased64
from items_oracle import items64, order64
from select_oracle import assert_list_consistent, drop_mask, exact_case, merge_lists, scores64, select64, window_count
from test_select_gpu import _random_case
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ops():
    return pkg('ops')


def _t(dev):
    return lambda x: None if x is None else x.to(dev)


def _equal_lists(val, idx, ref, what):
    rv, ri = ref
    val, idx = val.cpu(), idx.cpu()
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == rv.shape == idx.shape, what
    bad = (idx.long() != ri).any(1) | (val.double() != rv).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. ids %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], idx[bad][0].tolist()[:12], ri[bad][0].tolist()[:12])


def _equal_values(out, ref, what):
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, out.shape, ref.shape)
    bad = out.double() != ref
    assert not bool(bad.any()), '%s: %d slots differ, first at %s: got %s, expected %s' % (
        what, int(bad.sum()), bad.nonzero()[0].tolist(), out[bad][:6].tolist(), ref[bad][:6].tolist())


def _close(out, ref, what):
    """|out - ref| < TOL on the finite slots; the +-inf slots equal"""
    out = out.cpu().double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(out[~fin], ref[~fin]), (what, 'the infinite slots differ')
    err = float((out[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(what, 'max |out - oracle| %.2e over %d finite slots, %d infinite' % (err, int(fin.sum()), int((~fin).sum())))
    assert err < TOL, (what, err)


def _groups(B, G, seed=0):
    g = torch.randint(0, G, (B,), generator=torch.Generator().manual_seed(B + G + seed))
    g[:G] = torch.arange(G)[:B]                         # every row is used
    return g


# ------------------------------------------------------------------------------------------- 1) select, exact inputs
@pytest.mark.parametrize('G', [None, 3])
@pytest.mark.parametrize('B,V,d,K', [(5, 300, 32, 1), (5, 300, 32, 32), (33, 5000, 96, 128)])
def test_select_exact_inputs_give_equal_lists(dev, B, V, d, K, G):
    """about 30 % of the entries -inf, a whole 128-item chunk (rows 128 .. 255) and - at V = 5000, where a workgroup owns 512
    rows - a whole workgroup range (rows 512 .. 1023) without an eligible item"""
    ops, t = _ops(), _t(dev)
    sr, E, cs = exact_case(B, V, d)
    bias = exact_bias(V, G, off_ranges=((128, 256), (512, 1024)) if V == 5000 else ((128, 256),))
    group = None if G is None else _groups(B, G)
    rows = bias_rows(bias, group, B)
    assert 0.25 < float((rows == NINF).float().mean()) < 0.7 and bool((rows[:, 128:256] == NINF).all())
    for scale in (cs, None):
        val, idx = ops.score_select(sr.to(dev), E.to(dev), t(scale), K, bias=bias.to(dev), group=t(group))
        ref = select_biased64(scores64(sr, E, scale), K, bias, group)
        print('exact', (B, V, d, K, G), 'cs' if scale is not None else 'no cs', idx[0].tolist()[:8], ref[1][0].tolist()[:8])
        _equal_lists(val, idx, ref, 'exact %s' % ((B, V, d, K, G),))
        assert bool((rows.gather(1, idx.cpu().long().clamp(min=0)) != NINF).all())
        assert not torch.equal(ref[1], select64(scores64(sr, E, scale), K)[1])      # the bias matters: the unbiased list differs


# ------------------------------------------------------------------------------------------- 2) fewer eligible than K
def test_select_fewer_eligible_items_than_k(dev):
    ops, t = _ops(), _t(dev)
    B, V, d, K = 5, 20, 32, 20
    sr, E, cs = exact_case(B, V, d)
    s64 = scores64(sr, E, cs)
    sr, E, cs = sr.to(dev), E.to(dev), cs.to(dev)
    g = torch.Generator().manual_seed(4)
    allowed = torch.randperm(V, generator=g)[:12]
    bias = ops.catalog_bias(V, allow=allowed, boost=(allowed[:3], [0.5, -1.0, 2.0]))
    val, idx = ops.score_select(sr, E, cs, K, bias=bias.to(dev))
    _equal_lists(val, idx, select_biased64(s64, K, bias), '12 of 20 allowed')
    assert bool((idx[:, 12:] == -1).all()) and bool((val[:, 12:] == NINF).all()) and bool((idx[:, :12] >= 0).all())
    assert all(set(r[:12]) == set(allowed.tolist()) for r in idx.cpu().tolist())
    # nothing allowed: every slot is (-inf, -1) - an ineligible item does not beat an unfilled slot
    none = torch.full((V,), NINF)
    val, idx = ops.score_select(sr, E, cs, K, bias=none.to(dev))
    assert bool((idx == -1).all()) and bool((val == NINF).all())
    # one of three groups without any item
    bias3 = torch.stack([bias, none, torch.zeros(V)])
    group = torch.tensor([0, 1, 2, 1, 0])
    val, idx = ops.score_select(sr, E, cs, K, bias=bias3.to(dev), group=group.to(dev))
    _equal_lists(val, idx, select_biased64(s64, K, bias3, group), 'group 1 empty')
    assert bool((idx[group == 1] == -1).all()) and bool((idx[2] >= 0).all()) and int((idx[0] >= 0).sum()) == 12
    # together with a dropped list: both take items away
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    val, idx = ops.score_select(sr, E, cs, K, listed=listed.to(dev), drop_listed=True, bias=bias3.to(dev), group=group.to(dev))
    ref = select_biased64(s64, K, bias3, group, drop_mask(listed, V))
    _equal_lists(val, idx, ref, 'bias and drop_listed')
    assert int((idx[2] >= 0).sum()) == 15 and 7 <= int((idx[0] >= 0).sum()) <= 12


# ------------------------------------------------------------------------------------------- 3) order
@pytest.mark.parametrize('K', [1, 31, 128])
def test_select_order_is_that_of_the_biased_score(dev, K):
    ops = _ops()
    B, V, d = 33, 3000, 32
    sr = torch.zeros(B, d)
    sr[:, 0] = 1.0
    v = torch.arange(V).float()
    E = torch.zeros(V, d)
    E[:, 1] = 1.0                                         # (orthogonal to the sessions: no part of the score)
    j = torch.arange(K)
    # all tied, the first K ids out of the catalogue: ids K .. 2K - 1
    E[:, 0] = 0.5
    bias = torch.zeros(V)
    bias[:K] = NINF
    val, idx = ops.score_select(sr.to(dev), E.to(dev), None, K, bias=bias.to(dev))
    _equal_lists(val, idx, (torch.full((B, K), 0.5, dtype=torch.float64), (K + j)[None].expand(B, K)), 'tied K=%d' % K)
    # rising scores, a bias that reverses them: v / 8 - v / 4 falls with the id
    E[:, 0] = v / 8
    val, idx = ops.score_select(sr.to(dev), E.to(dev), None, K, bias=(-v / 4).to(dev))
    _equal_lists(val, idx, ((-j.double() / 8)[None].expand(B, K), j[None].expand(B, K)), 'reversed K=%d' % K)
    # falling scores, a finite boost on one far-away item: it leads the list, the rest is as before
    E[:, 0] = (V - 1 - v) / 8
    bias = torch.zeros(V)
    bias[2777] = 1024.0
    val, idx = ops.score_select(sr.to(dev), E.to(dev), None, K, bias=bias.to(dev))
    ids = torch.cat([torch.tensor([2777]), j[:K - 1]])
    vals = torch.cat([torch.tensor([(V - 1 - 2777) / 8 + 1024.0], dtype=torch.float64), (V - 1 - j[:K - 1]).double() / 8])
    _equal_lists(val, idx, (vals[None].expand(B, K), ids[None].expand(B, K)), 'boosted K=%d' % K)


# ------------------------------------------------------------------------------------------- 4) every kernel path, mixtures
def _mixture_case(B, V, d, C, L=5):
    """the construction of tests/test_select_gpu.py: session b's component b % C carries an offset that is a multiple of 1/8
    and the others -1e5 (exp() of them is exactly 0 in fp32 and in float64), so the mixture is exact"""
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(d + C)
    srs = torch.randint(-8, 9, (C, B, d), generator=g).float() / 8
    srs[0] = sr
    off = torch.full((C, B), -1.0e5)
    off[torch.arange(B) % C, torch.arange(B)] = -torch.randint(0, 9, (B,), generator=g).float() / 8
    listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])
    listed[:, L - 1] = -1
    off_in = off.clone()
    off_in[torch.arange(B) % C, torch.arange(B)] += 2.0
    return srs, E, cs, off, off_in, listed


@pytest.mark.parametrize('B,V,d,C,K,L', [(37, 700, 100, 2, 40, 5), (40, 600, 512, 4, 40, 5), (33, 500, 1024, 2, 40, 5),
                                         (33, 700, 256, 3, 128, 64)])
def test_select_exact_mixtures_on_every_kernel_path(dev, B, V, d, C, K, L):
    """session tiles in LDS and through the cache, C = 2, 3 and 4, one bias row and G = 2 - without a list, with a scored and
    with a dropped one.  The last case (C 3, d 256, K 128, L 64) sits at the LDS limit of the tile placement: whichever side
    an instance falls on, the lists are the oracle's."""
    ops, t = _ops(), _t(dev)
    srs, E, cs, off, off_in, listed = _mixture_case(B, V, d, C, L)
    for G in (None, 2):
        bias = exact_bias(V, G, seed=C)
        group = None if G is None else _groups(B, G)
        for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
            val, idx = ops.score_select(srs.to(dev), E.to(dev), cs.to(dev), K, off.to(dev), t(oi), t(lst), drop_listed=drop,
                                        bias=bias.to(dev), group=t(group))
            if drop:
                ref = select_biased64(scores64(srs, E, cs, off), K, bias, group, drop_mask(listed, V))
            else:
                ref = select_biased64(scores64(srs, E, cs, off, oi, lst), K, bias, group)
            print('exact mix', (B, V, d, C, K, L), G, what, idx[0].tolist()[:8], ref[1][0].tolist()[:8])
            _equal_lists(val, idx, ref, 'mixture %s G %s %s' % ((B, V, d, C, K, L), G, what))


# ------------------------------------------------------------------------------------------- 5) random inputs
def _random_bias(V, G, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (V,) if G is None else (G, V)
    b = torch.randn(shape, generator=g)
    b[torch.rand(shape, generator=g) < 0.3] = NINF
    return b


@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed-drop'])
@pytest.mark.parametrize('B,V,d', [(33, 5000, 96), (40, 3429, 64)])
def test_select_random_inputs_lists_consistent_with_roundoff(dev, B, V, d, kind):
    ops, t = _ops(), _t(dev)
    K = 50
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    G = None if kind == 'single' else 4
    bias, group = _random_bias(V, G, B + V), (None if G is None else _groups(B, G))
    drop = kind == 'listed-drop'
    val, idx = ops.score_select([s.to(dev) for s in srs], t(E), t(cs), K, t(off_ex), t(off_in), t(listed), drop_listed=drop,
                                bias=bias.to(dev), group=t(group))
    rows = bias_rows(bias, group, B)
    s64 = scores64(srs, E, cs, off_ex) + rows
    dm = (rows == NINF) | drop_mask(listed, V) if drop else rows == NINF          # eligibility: ~(dropped | bias == -inf)
    near = window_count(s64, K, TOL, dm)
    print(kind, (B, V, d), 'items within 2 TOL of the K-th best: max %d, mean %.2f' % (int(near.max()), float(near.float().mean())))
    assert int(near.max()) <= 4, 'the round-off window holds %d items: the check is vacuous for this draw' % int(near.max())
    assert_list_consistent(val, idx, s64, TOL, dm, what='%s %s' % (kind, (B, V, d)))
    with pytest.raises(AssertionError):                   # the bias matters: against the unbiased scores some list is inconsistent
        assert_list_consistent(val, idx, scores64(srs, E, cs, off_ex), TOL, dm, what='no bias')


# ------------------------------------------------------------------------------------------- 6) zero bias
@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed-score', 'listed-drop'])
def test_zero_bias_returns_the_unbiased_ids_and_values(dev, kind):
    ops, t = _ops(), _t(dev)
    B, V, d, K, M = 40, 3429, 64, 50, 300
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    drop = kind == 'listed-drop'
    items = torch.randint(-1, V, (B, M), generator=torch.Generator().manual_seed(3))
    args = ([s.to(dev) for s in srs], t(E), t(cs))
    kw = dict(off_ex=t(off_ex), off_in=t(off_in), listed=t(listed), drop_listed=drop)
    v0, i0 = ops.score_select(*args, K, **kw)
    o0 = ops.score_items(*args, items.to(dev), **kw)
    for bias, group in ((torch.zeros(V), None), (torch.zeros(3, V), _groups(B, 3)), (-torch.zeros(V), None)):
        v1, i1 = ops.score_select(*args, K, bias=bias.to(dev), group=t(group), **kw)
        assert torch.equal(i1, i0) and bool((v1 == v0).all()), (kind, tuple(bias.shape))
        o1 = ops.score_items(*args, items.to(dev), bias=bias.to(dev), group=t(group), **kw)
        assert bool((o1 == o0).all()), (kind, tuple(bias.shape))
    assert int((o0 == NINF).sum()) >= int((items < 0).sum()) > 0


# ------------------------------------------------------------------------------------------- 7) views and shards
def test_bias_views_and_two_row_ranges(dev):
    ops = _ops()
    B, V, d, K, M, G = 33, 5000, 96, 50, 150, 3
    sr, E, cs = exact_case(B, V, d)
    bias = exact_bias(V, G, seed=7, off_ranges=((128, 256), (2400, 2600)))
    group = _groups(B, G)
    g = torch.Generator().manual_seed(7)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    items = torch.randint(0, V, (B, M), generator=g)
    items[:, 0], items[:, 1], items[:, 2], items[:, 3] = 0, V - 1, -1, items[:, 4]
    items[:, 10:16] = listed
    items[:, 20], items[:, 21] = 2499, 2500
    s64 = scores64(sr, E, cs)
    sr, E, cs, listed_d, items_d, group_d = sr.to(dev), E.to(dev), cs.to(dev), listed.to(dev), items.to(dev), group.to(dev)
    wide = torch.full((G, 2 * V), 99.0, device=dev)
    wide[:, V:] = bias.to(dev)
    view = wide[:, V:]                                    # a column slice of a [G, 2V] tensor: row stride 2V
    assert view.stride() == (2 * V, 1) and not view.is_contiguous()
    for kw in (dict(), dict(listed=listed_d, drop_listed=True)):
        dm = drop_mask(listed, V) if kw else None
        whole = ops.score_select(sr, E, cs, K, bias=view, group=group_d, **kw)
        same = ops.score_select(sr, E, cs, K, bias=view.contiguous(), group=group_d, **kw)
        assert torch.equal(whole[0], same[0]) and torch.equal(whole[1], same[1])
        _equal_lists(whole[0], whole[1], select_biased64(s64, K, bias, group, dm), 'whole table, bias view')
        # two row ranges: each takes its columns of the bias (again a view) and its id_lo
        lo = ops.score_select(sr, E[:2500], cs[:2500], K, id_lo=0, bias=view[:, :2500], group=group_d, **kw)
        hi = ops.score_select(sr, E[2500:], cs[2500:], K, id_lo=2500, bias=view[:, 2500:], group=group_d, **kw)
        assert int(hi[1][hi[1] >= 0].min()) >= 2500 and int(lo[1].max()) < 2500
        mv, mi = merge_lists([lo[0], hi[0]], [lo[1], hi[1]], K)
        assert torch.equal(mi, whole[1].cpu().long()) and torch.equal(mv, whole[0].cpu().double())
        # items: the two shards' outputs summed are the single call's bits; a foreign id reads no bias (0.0, not -inf)
        one = ops.score_items(sr, E, cs, items_d, bias=view, group=group_d, **kw)
        lo = ops.score_items(sr, E[:2500], cs[:2500], items_d, id_lo=0, bias=view[:, :2500], group=group_d, **kw)
        hi = ops.score_items(sr, E[2500:], cs[2500:], items_d, id_lo=2500, bias=view[:, 2500:], group=group_d, **kw)
        assert bool((lo.cpu()[items >= 2500] == 0).all()) and bool((hi.cpu()[(items >= 0) & (items < 2500)] == 0).all())
        assert torch.equal(lo + hi, one)
        _equal_values(one, items_biased64(s64, items, bias, group, 0, dm), 'items, whole table')


# ------------------------------------------------------------------------------------------- 8) score_items, exact inputs
@pytest.mark.parametrize('M', [1, 257])
def test_score_items_exact_inputs_give_equal_values(dev, M):
    """M = 257 crosses the 256-slot chunk; per-session and shared lists, one bias row and groups; padding slots, foreign ids
    (the table is the row range [1000, 4000) of the catalogue), duplicates, ids out of the catalogue and dropped listed ids"""
    ops, t = _ops(), _t(dev)
    B, V, d, G = 33, 5000, 96, 3
    lo, hi = 1000, 4000
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(M)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    items = torch.randint(lo, hi, (B, M), generator=g)
    if M > 1:
        items[:, 0], items[:, 1], items[:, 2], items[:, 3] = -1, 7, V - 1, items[:, 4]      # padding, two foreign ids, a duplicate
        items[:, 5], items[:, 6] = lo, hi - 1
        items[:, 10:16] = listed
        items[:, 256] = 2000
        items[:, 100:130] = torch.arange(1128, 1158)      # the chunk without an eligible item (catalogue rows 1128 .. 1255)
    s64 = scores64(sr, E[lo:hi], cs[lo:hi], id_lo=lo)
    for Gn in (None, G):
        full = exact_bias(V, Gn, seed=M, off_ranges=((1128, 1256),))
        group = None if Gn is None else _groups(B, G)
        bias = full[..., lo:hi].to(dev)                   # the shard's columns of the global bias
        for kw, dm in ((dict(), None), (dict(listed=listed.to(dev), drop_listed=True), drop_mask(listed, hi - lo, lo))):
            for its in (items, items[B - 1]):
                out = ops.score_items(sr.to(dev), E[lo:hi].to(dev), cs[lo:hi].to(dev), its.to(dev), id_lo=lo, bias=bias,
                                      group=t(group), **kw)
                ref = items_biased64(s64, its, full, group, lo, dm)
                _equal_values(out, ref, 'items M %d G %s %s %s' % (M, Gn, 'drop' if kw else 'plain', tuple(its.shape)))
                if M > 1 and its.dim() == 2:
                    assert bool((ref[:, 0] == NINF).all()) and bool((ref[:, 1:3] == 0).all()) and bool((ref[:, 100:130] == NINF).all())
                    assert torch.equal(ref[:, 3], ref[:, 4]) and (not kw or bool((ref[:, 10:16][(listed >= lo) & (listed < hi)] == NINF).all()))
    if M > 1:                                             # the bias matters
        assert not torch.equal(ref, items64(s64, items[B - 1], lo, dm))


# ------------------------------------------------------------------------------------------- 9) sharded, W = 2 on one GPU
def test_sharded_select_and_score_items_with_bias_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from item_bias_gpu_worker import run_rank, sharded_bias
    from items_gpu_worker import candidates
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
    items = candidates()
    V = E.shape[0]
    s64 = scores64(sr, E, cs)
    sr, E, cs, listed_d, bias_d, group_d, items_d = [x.to(dev) for x in (sr, E, cs, listed, bias, group, items)]
    cpu = lambda r: [x.cpu() for x in r] if isinstance(r, (tuple, list)) else r.cpu()
    want = dict(select=cpu(ops.score_select(sr, E, cs, K, bias=bias_d, group=group_d)),
                select_shared=cpu(ops.score_select(sr, E, cs, K, bias=bias_d[1])),
                select_drop=cpu(ops.score_select(sr, E, cs, K, listed=listed_d, drop_listed=True, bias=bias_d, group=group_d)),
                items=cpu(ops.score_items(sr, E, cs, items_d, bias=bias_d, group=group_d)),
                items_shared=cpu(ops.score_items(sr, E, cs, items_d[0], bias=bias_d[1])),
                items_drop=cpu(ops.score_items(sr, E, cs, items_d, listed=listed_d, drop_listed=True, bias=bias_d, group=group_d)))
    want['select_routed'], want['items_routed'] = want['select'], want['items']
    _equal_lists(*want['select_drop'], select_biased64(s64, K, bias, group, drop_mask(listed, V)), 'single device select')
    _equal_values(want['items_drop'], items_biased64(s64, items, bias, group, 0, drop_mask(listed, V)), 'single device items')
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        for key, w in want.items():                       # every rank feeds the same sessions: the full answer on every rank
            if key.startswith('select'):
                assert res[key][1].dtype == torch.int32 and torch.equal(res[key][0], w[0]) and torch.equal(res[key][1], w[1]), (r, key)
            else:
                assert res[key].dtype == torch.float32 and torch.equal(res[key], w), (r, key)
        # every rank feeds its own slice, with its own list width and its own group ids: its own sessions' results
        mine = slice(r * n, (r + 1) * n)
        kw = dict(listed=listed_d[mine, :4 + r], drop_listed=True, bias=bias_d, group=group_d[mine])
        w = cpu(ops.score_select(sr[mine], E, cs, K, **kw))
        assert torch.equal(res['select_dp_drop'][0], w[0]) and torch.equal(res['select_dp_drop'][1], w[1]), r
        assert torch.equal(res['items_dp_drop'], ops.score_items(sr[mine], E, cs, items_d[mine], **kw).cpu()), r


# ------------------------------------------------------------------------------------------- 10) models against forward() + bias
def _seen(samples, V):
    m = torch.zeros(len(samples), V, dtype=torch.bool)
    for b, (seq, _) in enumerate(samples):
        m[b, torch.tensor(seq)] = True
    return m


@pytest.mark.parametrize('name', ['srgnn_s32', 'niser_s32', 'lessr_L3_s32', 'msgifsr_K3_ext_fus_s32'])
def test_models_with_item_bias_against_forward_plus_bias(dev, name):
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
    for G in (None, 2):
        bias = _random_bias(V, G, len(name))
        group = None if G is None else _groups(B, G)
        rows = bias_rows(bias, group, B)
        kw = dict(item_bias=bias.to(dev), item_group=None if group is None else group.to(dev))
        for ex in (False, True):
            dm = (rows == NINF) | seen if ex else rows == NINF
            val, idx = model.recommend(*inputs, k=20, exclude_seen=ex, **kw)
            assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (B, 20) and not model.training
            assert_list_consistent(val, idx, s64 + rows, TOL, dm, what='%s recommend G %s exclude_seen %s' % (name, G, ex))
            out = model.score_items(*inputs, items=items.to(dev), exclude_seen=ex, **kw)
            _close(out, items_biased64(s64, items, bias, group, 0, seen if ex else None), '%s score_items G %s exclude_seen %s' % (name, G, ex))
            for k in (None, 30):
                rv, ri = model.rerank(*inputs, items=items.to(dev), k=k, exclude_seen=ex, **kw)
                wv, wi = order64(out, items, k)
                assert rv.dtype == torch.float32 and ri.dtype == torch.int32 and rv.shape == ri.shape == wi.shape, (name, G, ex, k)
                assert torch.equal(ri.cpu().long(), wi) and torch.equal(rv.cpu().double(), wv), (name, G, ex, k)
        # the bias matters, and an item out of the catalogue is never named
        plain = model.recommend(*inputs, k=20)
        assert not torch.equal(plain[1], idx)
        assert bool((rows.gather(1, idx.cpu().long()) != NINF).all())
    assert not model.training


def test_models_refuse_a_bad_item_bias_before_anything_runs(dev, monkeypatch):
    sp = pkg()
    V = 50
    model = sp.SRGNN(V, 32, 1).to(dev).train()

    def never(*a, **k):
        raise AssertionError('something ran although the item bias is refused')
    monkeypatch.setattr(model, 'session_repr', never)
    for fn in ('score_select', 'score_items'):
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
             (dict(item_bias=torch.zeros(2, V - 1, device=dev), item_group=grp), r'item_bias must be a floating tensor \[50\]'),
             (dict(item_bias=torch.zeros(V, dtype=torch.int64, device=dev)), 'item_bias must be a floating tensor'),
             (dict(item_bias=torch.zeros(1, 2, V, device=dev)), 'item_bias must be a floating tensor'),
             (dict(item_bias=nan), 'item_bias holds NaN or \\+inf'),
             (dict(item_bias=pinf), 'item_bias holds NaN or \\+inf'),
             (dict(item_bias=torch.stack([ok, pinf]), item_group=grp), 'item_bias holds NaN or \\+inf'),
             (dict(item_bias=torch.stack([ok, ok]), item_group=torch.tensor([0, 2], device=dev)), r'row id outside \[0, 2\)'),
             (dict(item_bias=torch.stack([ok, ok]), item_group=torch.tensor([-1, 0])), r'row id outside \[0, 2\)'),
             (dict(item_bias=torch.stack([ok, ok])), 'G > 1 needs it'),
             (dict(item_bias=ok, item_group=grp), 'item_group .* goes with an item_bias \\[G, 50\\]'),
             (dict(item_group=grp), 'item_group is given without an item_bias'),
             (dict(item_bias=torch.stack([ok, ok]), item_group=torch.tensor([0.0, 1.0])), 'item_group must be an integer tensor'))
    items = torch.tensor([[1, 2], [3, 4]], device=dev)
    for kw, msg in cases:
        with pytest.raises(ValueError, match='recommend: .*' + msg):
            model.recommend(None, k=5, **kw)
        with pytest.raises(ValueError, match='score_items: .*' + msg):
            model.score_items(None, items=items, **kw)
        with pytest.raises(ValueError, match='score_items: .*' + msg):
            model.rerank(None, items=items, k=2, **kw)
    assert model.training                               # nothing ran, nothing was switched
    # a bias of -inf and finite values passes the check (and then reaches the encoder)
    good = ok.clone()
    good[3], good[4] = NINF, -2.5
    with pytest.raises(AssertionError, match='something ran'):
        model.recommend(None, k=5, item_bias=good)


# ------------------------------------------------------------------------------------------- 11) launchers
def test_launchers_with_catalogue_flags_equal_the_in_process_calls(dev, tmp_path):
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
    boost_ids = torch.randperm(V, generator=g)[:200].tolist()
    boost_vals = (torch.randint(-16, 17, (200,), generator=g).float() / 4).tolist()
    allow = torch.randperm(V, generator=g)[:V // 2].tolist()
    cands = [torch.randint(0, V, (150,), generator=g).tolist() + s[:2] for s in sessions]
    (tmp_path / 'sessions.txt').write_text(rec.format_sessions(sessions))
    (tmp_path / 'cands.txt').write_text(rec.format_sessions(cands))
    (tmp_path / 'deny.txt').write_text(''.join('%d\n' % i for i in deny))
    (tmp_path / 'allow.txt').write_text(''.join('%d\n' % i for i in allow))
    (tmp_path / 'bias.txt').write_text(''.join(('%d:%r\n' if n % 2 else '%d\t%r\n') % (i, v) for n, (i, v) in enumerate(zip(boost_ids, boost_vals))))
    common = ['--model', 'SRGNN', '--dataset-dir', data, '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt),
              '--sessions', str(tmp_path / 'sessions.txt')]
    top, ranked = tmp_path / 'top.txt', tmp_path / 'ranked.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py')] + common +
                       ['--top', '50', '--deny', str(tmp_path / 'deny.txt'), '--item-bias', str(tmp_path / 'bias.txt'), '--output', str(top)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'rerank.py')] + common +
                       ['--candidates', str(tmp_path / 'cands.txt'), '--allow', str(tmp_path / 'allow.txt'), '--output', str(ranked)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    inputs = [x.to(dev) for x in inputs]
    val, idx = model.recommend(*inputs, k=50, item_bias=ops.catalog_bias(V, deny=deny, boost=(boost_ids, boost_vals), device=dev))
    lines = top.read_text().splitlines()
    assert len(lines) == len(sessions)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == idx[b].tolist() and not set(ids) & set(deny), b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
    assert any(set(r) & set(boost_ids) for r in idx.cpu().tolist())
    val, idx = model.rerank(*inputs, items=torch.tensor(rr.pad_candidates(cands)).to(dev), item_bias=ops.catalog_bias(V, allow=allow, device=dev))
    lines = ranked.read_text().splitlines()
    assert len(lines) == len(sessions)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        n = len(ids)
        assert n == sum(c in set(allow) for c in cands[b]) and 0 < n < len(cands[b]), b
        assert ids == idx[b, :n].tolist() and bool((idx[b, n:] == -1).all()), b
        assert max(abs(a - c) for a, c in zip(vals, val[b, :n].tolist())) <= 1e-6, b
