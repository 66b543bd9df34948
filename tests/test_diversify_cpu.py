"""CPU side of the diversified top-N: the float64 oracle (tests/diversify_oracle.py) against a brute force by hand, the
margin property the GPU test's EQUAL-picks cases rest on, and the argument checks of ops.diversify, model.recommend_diverse /
list_diversity and the launcher, which must raise before anything is loaded or launched."""
import os
import sys

import pytest
import torch

import diversify_oracle as do
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
MARGIN_SHAPES = [(5, 128, 256, 20), (33, 37, 100, 37), (3, 128, 1024, 64), (4, 64, 32, 10)]       # (B, M, d, K)


def margin_inputs(B, M, d):
    return do.margin_case(B, M, d, seed=B + M)


# ------------------------------------------------------------------------------------------- the oracle by hand
def _four_slots():
    """two clusters: slots 0, 1 along e0 (slot 1 slightly turned), slots 2, 3 along e1; values descending"""
    rows = torch.tensor([[[1.0, 0.0, 0.0, 0.0], [3.0, 0.0, 4.0, 0.0], [0.0, 2.0, 0.0, 0.0], [0.0, 3.0, 0.0, 4.0]]])
    s = torch.tensor([[4.0, 3.5, 3.0, 2.0]])
    return rows, s


def test_oracle_against_a_brute_force_by_hand():
    rows, s = _four_slots()
    # cosines by hand: (0,1) 3/5, (0,2) 0, (0,3) 0, (1,2) 0, (1,3) 0, (2,3) 3/5
    sim = do.sims64(rows)[0]
    want = torch.tensor([[1, .6, 0, 0], [.6, 1, 0, 0], [0, 0, 1, .6], [0, 0, .6, 1]], dtype=torch.float64)
    assert torch.allclose(sim, want, rtol=0, atol=1e-15)
    # theta = 1, K = 4, by hand:
    #   t0: m = s                          -> slot 0 (4)
    #   t1: pen = (., .6, 0, 0): 2.9, 3, 2 -> slot 2 (3)
    #   t2: pen = (., .6, ., .6): 2.9, 1.4 -> slot 1 (2.9)
    #   t3: pen(3) = .6                    -> slot 3 (1.4)
    r = do.greedy64(rows, s, 1.0, 4)
    assert r['pick'].tolist() == [[0, 2, 1, 3]]
    assert r['val'].tolist() == [[4.0, 3.0, 3.5, 2.0]]
    assert torch.allclose(r['mmr'], torch.tensor([[4.0, 3.0, 2.9, 1.4]], dtype=torch.float64), rtol=0, atol=1e-15)
    assert torch.allclose(r['margin'][0, :3], torch.tensor([0.5, 0.1, 1.5], dtype=torch.float64), rtol=0, atol=1e-15)
    assert abs(float(r['ild'][0]) - (1 - (0.6 + 0.6) / 6)) < 1e-15
    # K = 2: one item per cluster, and its diversity is 1
    r2 = do.greedy64(rows, s, 1.0, 2)
    assert r2['pick'].tolist() == [[0, 2]] and float(r2['ild'][0]) == 1.0
    assert float(do.ild64(rows, torch.tensor([[0, 1]]))[0]) == pytest.approx(0.4, abs=1e-15)


def test_oracle_large_theta_picks_one_item_per_cluster_and_zero_is_slot_order():
    g = torch.Generator().manual_seed(2)
    centres = torch.eye(8)[:5] * 3
    which = torch.arange(40) % 5
    rows = (centres[which] + 0.01 * torch.randn(40, 8, generator=g))[None]
    s = torch.linspace(2, 1, 40)[None]
    r = do.greedy64(rows, s, 50.0, 5)
    assert sorted(which[r['pick'][0]].tolist()) == [0, 1, 2, 3, 4]
    assert float(r['ild'][0]) > 0.99
    # theta = 0: slot order whatever the rows are - tied values, values descending, and unfilled slots skipped
    tied = torch.full((1, 40), 0.25)
    assert do.greedy64(rows, tied, 0.0, 7)['pick'].tolist() == [list(range(7))]
    assert do.greedy64(rows, s, 0.0, 7)['pick'].tolist() == [list(range(7))]
    filled = torch.ones(1, 40, dtype=torch.bool)
    filled[0, [1, 2, 5]] = False
    r = do.greedy64(rows, tied, 0.0, 40, filled)
    assert r['pick'][0, :37].tolist() == [i for i in range(40) if i not in (1, 2, 5)]
    assert r['pick'][0, 37:].tolist() == [-1] * 3 and bool((r['val'][0, 37:] == do.NINF).all())
    # a negative cosine RAISES m (the raw maximum, not clamped at 0): the opposite row beats an orthogonal one of equal value
    rows = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0]]])
    assert do.greedy64(rows, torch.tensor([[1.0, 0.5, 0.5]]), 1.0, 2)['pick'].tolist() == [[0, 2]]
    # a zero row: similarity 0 to everything, no NaN
    rows = torch.tensor([[[1.0, 0.0], [0.0, 0.0], [1.0, 0.0]]])
    r = do.greedy64(rows, torch.tensor([[1.0, 0.9, 0.95]]), 1.0, 3)
    assert r['pick'].tolist() == [[0, 1, 2]] and not bool(torch.isnan(r['mmr']).any()) and float(r['ild'][0]) == pytest.approx(2 / 3)


def test_assert_greedy_consistent_accepts_the_oracle_and_refuses_a_swap():
    g = torch.Generator().manual_seed(5)
    rows, s = torch.randn(6, 20, 16, generator=g), torch.randn(6, 20, generator=g)
    pick = do.greedy64(rows, s, 1.0, 8)['pick']
    do.assert_greedy_consistent(pick, rows, s, 1.0, 1e-4)
    bad = pick.clone()
    bad[:, [2, 3]] = pick[:, [3, 2]]
    with pytest.raises(AssertionError):
        do.assert_greedy_consistent(bad, rows, s, 1.0, 1e-4)
    with pytest.raises(AssertionError):                       # a repeated slot
        rep = pick.clone()
        rep[:, 4] = pick[:, 0]
        do.assert_greedy_consistent(rep, rows, s, 1.0, 1e-4)


# ------------------------------------------------------------------------------------------- the margin cases
@pytest.mark.parametrize('B,M,d,K', MARGIN_SHAPES)
def test_margin_case_has_a_wide_margin_at_every_step(B, M, d, K):
    rows, s = margin_inputs(B, M, d)
    assert rows.dtype == s.dtype == torch.float32 and rows.shape == (B, M, d) and s.shape == (B, M)
    sim = do.sims64(rows)
    assert bool((sim * 4 == (sim * 4).round()).all()), 'a cosine that is no multiple of 1/4'
    assert bool((rows.double().norm(dim=-1) == 1.0).all())
    r = do.greedy64(rows, s, 0.5, K)
    assert float(r['margin'].min()) == 2.0 ** -10, float(r['margin'].min())
    slot_order = torch.arange(K)[None].expand(B, K)
    assert bool((r['pick'] != slot_order).any(1).all()), 'a session that the penalty does not reorder'
    assert bool((r['pick'] >= 0).all())
    if K < M:       # the diversified list is strictly more diverse than the first K slots, in the mean over the sessions
        rise = float(r['ild'].mean() - do.ild64(rows, slot_order).mean())
        print((B, M, d, K), 'mean ild rise %.4f' % rise)
        if (B, M, d, K) != (3, 128, 1024, 64):      # (K = 64 of 12 directions: both lists are the first 64 slots as SETS)
            assert rise > 0.01


# ------------------------------------------------------------------------------------------- argument checks
def test_ops_diversify_refuses_bad_arguments_before_any_launch():
    ops = pkg('ops')
    X, row, val = torch.zeros(50, 32), torch.zeros(3, 10, dtype=torch.int64), torch.zeros(3, 10)
    bad = [
        dict(k=0), dict(k=11), dict(k=129), dict(diversity=-0.5), dict(diversity=float('nan')), dict(diversity=float('inf')),
        dict(diversity='much'), dict(X=torch.zeros(50, 30)), dict(X=torch.zeros(50, 1028)), dict(X=torch.zeros(50, 32).double()),
        dict(X=torch.zeros(2, 50, 32)), dict(row=torch.zeros(3, 10)), dict(row=torch.zeros(30, dtype=torch.int64)),
        dict(row=torch.zeros(3, 10, dtype=torch.bool)), dict(val=torch.zeros(3, 9)), dict(val=torch.zeros(3, 10).double()),
        dict(row=torch.full((3, 10), 50)),                                   # a row past the end of X (checked=False)
        dict(row=torch.zeros(3, 129, dtype=torch.int64), val=torch.zeros(3, 129), k=5),
    ]
    for kw in bad:
        a = dict(X=X, row=row, val=val, k=5, diversity=0.5)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.diversify(a['X'], a['row'], a['val'], a['k'], a['diversity'])
    # the scalars on their own
    assert ops.diversify_scalars('t', 20, 0) == (20, 0.0) and ops.diversify_scalars('t', 128, 2, 128) == (128, 2.0)
    for k, th, M in ((0, 0.5, None), (129, 0.5, None), (5, 0.5, 4), (5, -1e-9, None), (5, 0.5, 129), (5, 0.5, 0)):
        with pytest.raises(ValueError):
            ops.diversify_scalars('t', k, th, M)
    # good arguments on CPU tensors get as far as the launch, which has no fallback
    with pytest.raises(RuntimeError, match='GPU|libsrec'):
        ops.diversify(X, row, val, 5, 0.5)


def _cpu_model(V=30, d=8):
    class TableOnly(pkg('srgnn')._ScoringMixin, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = torch.nn.Embedding(V, d)

        def session_repr(self, *a, **k):
            raise AssertionError('the model ran before its arguments were checked')
    return TableOnly()


def test_recommend_diverse_and_list_diversity_check_their_arguments_before_the_model_runs():
    m = _cpu_model()
    for kw in (dict(k=0), dict(k=129), dict(k=10, pool=9), dict(k=10, pool=129), dict(diversity=-1), dict(diversity=float('nan')),
               dict(diversity=float('inf')), dict(item_bias=torch.zeros(7)), dict(item_group=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            m.recommend_diverse(None, **kw)
    assert m._diverse_args('t', 20, 0.5, None) == (20, 0.5, 80)
    assert m._diverse_args('t', 50, 0, None) == (50, 0.0, 128)
    assert m._diverse_args('t', 128, 1, None) == (128, 1.0, 128)
    assert m._diverse_args('t', 3, 1, 3) == (3, 1.0, 3)
    for ids in (torch.zeros(2, 5), torch.zeros(5, dtype=torch.int64), torch.zeros(2, 129, dtype=torch.int64),
                torch.full((2, 5), 30), torch.full((2, 5), -2), torch.zeros(2, 0, dtype=torch.int64)):
        with pytest.raises(ValueError):
            m.list_diversity(ids)
    assert m._ROUTES['diversify'] == ('diversify', {'checked': True})


def test_launcher_takes_diversity_and_pool_and_refuses_them_with_sample():
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
    finally:
        sys.path.remove(SCRIPTS)
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt']
    a = rec.parse(base)
    assert a.diversity is None and a.pool is None
    a = rec.parse(base + ['--diversity', '0.5', '--pool', '40', '--top', '10', '--exclude-seen'])
    assert a.diversity == 0.5 and a.pool == 40 and a.top == 10 and a.exclude_seen and not a.sample
    assert rec.parse(base + ['--diversity', '0']).diversity == 0.0
    for bad in (['--diversity', '0.5', '--sample'], ['--diversity', '-1'], ['--diversity', 'nan'], ['--diversity', 'inf'],
                ['--pool', '40'], ['--diversity', '0.5', '--pool', '129'], ['--diversity', '0.5', '--pool', '5', '--top', '10']):
        with pytest.raises(SystemExit):
            rec.parse(base + bad)
    helptext = rec.parser('SRGNN').format_help()
    assert '--diversity' in helptext and '--pool' in helptext


# ------------------------------------------------------------------------------------------- the sharded route over gloo
def _div_case(V):
    g = torch.Generator().manual_seed(17 + V)
    table = torch.randint(-8, 9, (V, 16), generator=g).float() / 8
    ids = torch.stack([torch.randperm(V, generator=g)[:12] for _ in range(8)]).to(torch.int32)
    ids[:, 5] = -1
    ids[3, 9:] = -1
    val = torch.sort(torch.randn(8, 12, generator=g), 1, descending=True).values
    return table, ids, val


def _oracle_local():
    from test_dist_cpu import TorchLocal

    class DiverseLocal(TorchLocal):
        """TorchLocal + the diversify entry of dist.HipLocal, from the float64 oracle"""

        def diversify(self, X, row, val, k, diversity):
            r = do.greedy64(X[row.clamp(min=0).long()], val, diversity, k, row >= 0)
            return r['val'].float(), r['pick'].to(torch.int32), r['mmr'].float(), r['ild'].float()
    return DiverseLocal()


def _div_worker(rank, world, port, V, q):
    import torch.distributed as dist
    from test_dist_cpu import FakeModel
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, ids, val = _div_case(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=_oracle_local())
        shard = model._table().detach()
        n = ids.shape[0] // world
        sl = slice(rank * n, (rank + 1) * n)
        with torch.no_grad():
            rep = vp.diversify(shard, ids, val, 6, 0.75)
            dp = vp.diversify(shard, ids[sl], val[sl], 6, 0.75, data_parallel=True)
        q.put((rank, vp.n_live, [t.tolist() for t in rep], [t.tolist() for t in dp]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('V', [150, 40])
def test_sharded_diversify_two_ranks_equal_unsharded(V):
    """every rank contributes the rows it owns and one sum-all-reduce completes the pool's rows: the result is the unsharded
    one bit for bit, replicated and data-parallel, also where rank 1 has no live rows (V = 40: the neutral branch)"""
    import torch.multiprocessing as mp
    from test_dist_cpu import _free_port
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_div_worker, args=(r, world, port, V, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    table, ids, val = _div_case(V)
    ref = [t.tolist() for t in _oracle_local().diversify(table, ids, val, 6, 0.75)]
    assert ref[1] != [list(range(6))] * 8 and -1 not in ref[1][0] and ref[1][3][-1] >= 0
    n = ids.shape[0] // world
    for rank, n_live, rep, dp in res:
        assert n_live == {150: (128, 22), 40: (40, 0)}[V][rank]
        assert rep == ref, (V, rank)
        assert dp == [x[rank * n:(rank + 1) * n] for x in ref], (V, rank)
