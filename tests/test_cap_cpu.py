"""CPU side of the per-category caps: the properties of the oracle (tests/cap_oracle.py) the GPU test compares with, the
argument checks of ops.cap_rule / ops.cap_select, model.recommend_capped and the launcher - which must raise before anything
is loaded or launched - and the sharded route over two gloo ranks with an oracle-backed local."""
import os
import sys

import pytest
import torch

import cap_oracle as co
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
POOLS = [(1, 1, 1, 1), (33, 128, 20, 7), (5, 300, 128, 50), (2, 600, 100, 3)]          # (B, P, k, G)


# ------------------------------------------------------------------------------------------- the oracle
def test_oracle_by_hand():
    category = [0, 0, 0, 1, 1, -1, 2, 7]                     # (7 >= G: no category)
    caps = [1, 2, 0]
    #       id:  0  1   3  9  4  3  6   5  7  2  -1
    # category:  0  0   1  .  1  1  2  -1  .  0
    #   accept:  y  n   y  u  y  n  n   y  y  n   u
    ids = [[0, 1, 3, 9, 4, 3, 6, 5, 7, 2, -1]]
    assert co.capped(ids, category, caps, 5) == ([[0, 2, 4, 7, 8]], [5], [9])
    assert co.capped(ids, category, caps, 4) == ([[0, 2, 4, 7]], [4], [8])
    assert co.capped(ids, category, caps, 7) == ([[0, 2, 4, 7, 8, -1, -1]], [5], [11])
    assert co.capped(ids, category, caps, 1) == ([[0]], [1], [1])
    val = torch.arange(11, 0, -1).float()[None]
    v, i = co.capped_lists(val, torch.tensor(ids), category, caps, 7)
    assert i.tolist() == [[0, 3, 4, 5, 7, -1, -1]] and v.tolist() == [[11.0, 9.0, 7.0, 4.0, 3.0, co.NINF, co.NINF]]


@pytest.mark.parametrize('B,P,k,G', POOLS)
def test_oracle_properties(B, P, k, G):
    ids, _, category, caps = co.random_pool(B, P, G, garbage=True)
    n = category.numel()
    pick, kept, scanned = co.capped(ids, category, caps, k)
    cat, cap, rows = category.tolist(), caps.tolist(), ids.tolist()
    bound = 0
    for b in range(B):
        got = [p for p in pick[b] if p >= 0]
        assert got == sorted(set(got)) and len(got) == kept[b] and pick[b][kept[b]:] == [-1] * (k - kept[b])
        assert scanned[b] == (got[-1] + 1 if kept[b] == k else P)
        count = {}
        for p in got:                                        # every pick is a filled slot; no category exceeds its cap
            assert 0 <= rows[b][p] < n
            c = cat[rows[b][p]]
            if c >= 0:
                count[c] = count.get(c, 0) + 1
        assert all(m <= cap[c] for c, m in count.items()), (b, count)
        for i in range(scanned[b]):                          # every skipped filled slot before `scanned` belongs to a full category
            if i not in got and 0 <= rows[b][i] < n:
                c = cat[rows[b][i]]
                assert c >= 0 and sum(1 for p in got if p < i and cat[rows[b][p]] == c) == cap[c], (b, i)
                bound += 1
    assert bound > 0 or P == 1, 'no cap binds: the case shows nothing'
    # caps >= P: the first k filled slots
    free, kept_f, _ = co.capped(ids, category, [P] * G, k)
    for b in range(B):
        filled = [i for i, v in enumerate(rows[b]) if 0 <= v < n]
        assert free[b][:kept_f[b]] == filled[:k] and kept_f[b] == min(k, len(filled))


# ------------------------------------------------------------------------------------------- argument checks
def test_cap_rule_builds_the_record_and_refuses_bad_arguments():
    ops = pkg('ops')
    r = ops.cap_rule(5, [0, 2, -1, 2, 1], 2)
    assert isinstance(r, ops.CapRule) and r.G == 3 and r.category.dtype == r.caps.dtype == torch.int32
    assert r.category.tolist() == [0, 2, -1, 2, 1] and r.caps.tolist() == [2, 2, 2]
    r = ops.cap_rule(5, torch.tensor([0, 2, -1, 2, 1], dtype=torch.int16), torch.tensor([1, 0, 3, 9]))
    assert r.G == 4 and r.caps.tolist() == [1, 0, 3, 9]
    assert ops.cap_rule(3, [-1, -1, -1], 0).G == 1                       # no category at all: one unused counter
    gmax = ops.CONST['SREC_CAP_MAXG']
    assert gmax == 16384 and ops.CONST['SREC_CAP_MAXP'] == 4096 == ops.CONST['SREC_SELECT_MANY_MAXK']
    assert ops.cap_rule(2, [0, gmax - 1], 1).G == gmax
    for cat, cap in (([0, 1, 2, 3], 2),                                  # a wrong length
                     ([0.0, 1.0, 2.0, 0.0, 1.0], 2), ([True] * 5, 2),    # a non-integer dtype
                     ([[0, 1, 2, 0, 1]], 2),
                     ([0, -2, 1, 0, 0], 2),                              # a category < -1
                     ([0, 1, 2, 0, 1], [1, 1]),                          # ... and >= G
                     ([0, 1, 2, 0, 1], -1), ([0, 1, 2, 0, 1], [1, -1, 1]),            # a negative cap
                     ([0, 1, 2, 0, 1], 1.5), ([0, 1, 2, 0, 1], [1.0, 1.0, 1.0]), ([0, 1, 2, 0, 1], True),
                     ([0, 1, 2, 0, 1], []), ([0, 1, 2, 0, gmax], 1), ([0, 1, 2, 0, 1], [1] * (gmax + 1))):
        with pytest.raises(ValueError):
            ops.cap_rule(5, cat, cap)


def test_ops_cap_select_refuses_bad_arguments_before_any_launch():
    ops = pkg('ops')
    rule = ops.cap_rule(50, torch.arange(50) % 5, 2)
    ids, val = torch.zeros(3, 10, dtype=torch.int64), torch.zeros(3, 10)
    bad = [
        dict(k=0), dict(k=11), dict(k=4097), dict(ids=torch.zeros(3, 10)), dict(ids=torch.zeros(30, dtype=torch.int64)),
        dict(ids=torch.zeros(3, 10, dtype=torch.bool)), dict(val=torch.zeros(3, 9)), dict(val=torch.zeros(3, 10).double()),
        dict(ids=torch.full((3, 10), 50)),                                   # an id past the rule's items (checked=False)
        dict(ids=torch.zeros(3, 4097, dtype=torch.int64), val=torch.zeros(3, 4097), k=5),
        dict(ids=ids.to('meta')), dict(val=val.to('meta')),                  # not on the rule's device: refused, not moved
        dict(rule=ops.CapRule(rule.category, rule.caps.to('meta'), rule.G)),
        dict(rule=(rule.category, rule.caps, rule.G)), dict(rule=None),
        dict(rule=ops.CapRule(rule.category.long(), rule.caps, rule.G)), dict(rule=ops.CapRule(rule.category, rule.caps, 4)),
        dict(rule=ops.CapRule(rule.category, torch.zeros(20000, dtype=torch.int32), 20000)),
    ]
    for kw in bad:
        a = dict(ids=ids, val=val, rule=rule, k=5)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.cap_select(a['ids'], a['val'], a['rule'], a['k'])
    assert ops.cap_k('t', 4096) == 4096 and ops.cap_k('t', 7, 7) == 7
    for k, P in ((0, None), (4097, None), (5, 4), (5, 4097), (1, 0)):
        with pytest.raises(ValueError):
            ops.cap_k('t', k, P)
    # good arguments on CPU tensors get as far as the launch, which has no fallback
    with pytest.raises(RuntimeError, match='GPU|libsrec'):
        ops.cap_select(ids, val, rule, 5)


def _cpu_model(V=30, d=8):
    class TableOnly(pkg('srgnn')._ScoringMixin, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = torch.nn.Embedding(V, d)

        def session_repr(self, *a, **k):
            raise AssertionError('the model ran before its arguments were checked')
    return TableOnly()


def test_recommend_capped_checks_its_arguments_before_the_model_runs():
    m, ops = _cpu_model(), pkg('ops')
    cat = torch.arange(30) % 4
    good = dict(item_category=cat, max_per_category=2)
    rule = ops.cap_rule(30, cat, 2)
    for kw in (dict(k=0, **good), dict(k=4097, **good), dict(k=10, pool=9, **good), dict(k=10, pool=4097, **good),
               dict(), dict(item_category=cat), dict(max_per_category=2), dict(rule=rule, **good), dict(rule=rule, max_per_category=2),
               dict(rule=(rule.category, rule.caps, rule.G)), dict(rule=ops.cap_rule(29, cat[:29], 2)),
               dict(item_category=cat[:29], max_per_category=2), dict(item_category=cat.float(), max_per_category=2),
               dict(item_category=cat - 2, max_per_category=2), dict(item_category=cat, max_per_category=-1),
               dict(item_category=cat, max_per_category=[1, 1]), dict(item_bias=torch.zeros(7), **good),
               dict(item_group=torch.zeros(2, dtype=torch.int64), **good)):
        with pytest.raises(ValueError):
            m.recommend_capped(None, **kw)
    # good arguments reach the model
    for kw in (good, dict(rule=rule), dict(rule=rule, k=200), dict(rule=rule, k=5, pool=4096)):
        with pytest.raises(AssertionError, match='the model ran'):
            m.recommend_capped(None, **kw)
    assert m._ROUTES['cap'] == ('cap_select', {'checked': True})
    assert 'recommend_capped' in pkg('serving').__doc__


def test_launcher_takes_the_cap_flags_and_refuses_the_combinations(tmp_path):
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
    finally:
        sys.path.remove(SCRIPTS)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    cats = tmp_path / 'cats.txt'
    cats.write_text(''.join('%d:%d\n' % (i, i % 5) for i in range(0, V, 2)) + '\n')
    capsf = tmp_path / 'caps.txt'
    capsf.write_text('1:0\n6:3\n')
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--dataset-dir', data]
    a = rec.parse(base)
    assert a.categories is None and a.caps is None and a.max_per_category is None
    a = rec.parse(base + ['--categories', str(cats), '--max-per-category', '2', '--top', '10', '--exclude-seen'])
    assert a.caps['item_category'] == [i % 5 if i % 2 == 0 else -1 for i in range(V)] and a.caps['max_per_category'] == [2] * 5
    assert a.pool is None and not a.sample and a.diversity is None
    a = rec.parse(base + ['--categories', str(cats), '--max-per-category', '2', '--category-caps', str(capsf), '--pool', '3000'])
    assert a.caps['max_per_category'] == [2, 0, 2, 2, 2, 2, 3] and a.pool == 3000
    a = rec.parse(base + ['--categories', str(cats), '--category-caps', str(capsf)])
    assert a.caps['max_per_category'] == [2 ** 31 - 1, 0] + [2 ** 31 - 1] * 4 + [3]
    rule = pkg('ops').cap_rule(V, **a.caps)
    assert rule.G == 7 and rule.caps.tolist() == a.caps['max_per_category']
    on = ['--categories', str(cats), '--max-per-category', '2']
    (tmp_path / 'bad_item.txt').write_text('0:1\n%d:1\n' % V)
    (tmp_path / 'twice.txt').write_text('3:1\n3:2\n')
    (tmp_path / 'bad_cat.txt').write_text('3:-1\n')
    (tmp_path / 'big_cat.txt').write_text('3:16384\n')
    (tmp_path / 'words.txt').write_text('3:shoes\n')
    (tmp_path / 'neg_cap.txt').write_text('1:-1\n')
    (tmp_path / 'tabs.txt').write_text('3\t1\n')                           # (`id:category` is the format; a tab is none)
    for bad in (['--max-per-category', '2'], ['--category-caps', str(capsf)], ['--categories', str(cats)],
                on + ['--sample'], on + ['--diversity', '0.5'], on + ['--pool', '5', '--top', '10'], on + ['--pool', '4097'],
                ['--categories', str(cats), '--max-per-category', '-1'], ['--categories', str(tmp_path / 'none.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'bad_item.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'twice.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'bad_cat.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'big_cat.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'words.txt'), '--max-per-category', '2'],
                ['--categories', str(tmp_path / 'tabs.txt'), '--max-per-category', '2'],
                on + ['--category-caps', str(tmp_path / 'neg_cap.txt')], ['--pool', '40']):
        with pytest.raises(SystemExit):
            rec.parse(base + bad)
    helptext = rec.parser('SRGNN').format_help()
    assert '--categories' in helptext and '--max-per-category' in helptext and '--category-caps' in helptext


# ------------------------------------------------------------------------------------------- the sharded route over gloo
def _cap_case():
    ids, val, category, caps = co.random_pool(8, 40, 6, n_items=150, seed=3)
    return ids, val, pkg('ops').CapRule(category, caps, 6)


def _oracle_local():
    from test_dist_cpu import TorchLocal

    class CapLocal(TorchLocal):
        """TorchLocal + the cap_select entry of dist.HipLocal, from the oracle"""

        def cap_select(self, ids, val, rule, k):
            pick, kept, scanned = co.capped(ids, rule.category, rule.caps, k)
            pick = torch.tensor(pick, dtype=torch.long).view(ids.shape[0], k)
            v = torch.where(pick >= 0, val.gather(1, pick.clamp(min=0)), torch.full((), co.NINF))
            return v, pick.to(torch.int32), torch.tensor(kept, dtype=torch.int32), torch.tensor(scanned, dtype=torch.int32)
    return CapLocal()


def _cap_worker(rank, world, port, q):
    import torch.distributed as dist
    from test_dist_cpu import FakeModel
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        ids, val, rule = _cap_case()
        g = torch.Generator().manual_seed(1)
        model = FakeModel(torch.randn(150, 16, generator=g))
        vp = pkg('dist').VocabParallel(model, local=_oracle_local())
        n = ids.shape[0] // world
        sl = slice(rank * n, (rank + 1) * n)
        with torch.no_grad():
            rep = vp.cap_select(ids, val, rule, 9)
            dp = vp.cap(ids[sl], val[sl], rule, 9, data_parallel=True)
        # a flag only rank 1 holds: data-parallel ranks agree on it, replicated ranks hold the same flags already
        own = torch.tensor([False, rank == 1])
        assert vp.any_session(own, data_parallel=True) is True
        assert vp.any_session(torch.tensor([False, False]), data_parallel=True) is False
        assert vp.any_session(torch.tensor([False, True])) is True and vp.any_session(torch.tensor([False])) is False
        q.put((rank, vp.n_live, [t.tolist() for t in rep], [t.tolist() for t in dp]))
    finally:
        dist.destroy_process_group()


SPLIT_K = 5


def _split_case():
    """(session vectors [8, d], table, category, caps, full order [8, V]) of tests/test_serving_model_cpu.py's exact-input
    case with a rule that binds for ONE rank's sessions only: the 128 best items of session 4 (rank 1 under two data-parallel
    ranks) share category 0 with cap 2, the other 22 have none.  Session 4 keeps 2 of its 128-item pool; the sessions of
    rank 0 find their SPLIT_K in theirs"""
    from select_oracle import select64
    from test_serving_model_cpu import CASE, V
    sr, table = CASE['srs'][0], CASE['table']
    s = (sr.double() @ table.double().t()).float()                       # exact: multiples of 1/64
    order = select64(s, V, torch.zeros_like(s, dtype=torch.bool), 0)[1].long()
    category = torch.full((V,), -1)
    category[order[4, :128]] = 0
    return sr, table, category, torch.tensor([2]), order


def _split_worker(rank, world, port, q):
    import torch.distributed as dist
    from test_serving_model_cpu import AllLocal, V, _models
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        D, ops = pkg('dist'), pkg('ops')

        class CapAllLocal(AllLocal, type(_oracle_local())):
            """every served route from the oracles, cap_select included"""
        sr, _, category, caps, _ = _split_case()
        model = _models()[0]().eval()
        vp = D.VocabParallel(model, local=CapAllLocal(V))
        vp.eval_data_parallel = True
        rule = ops.cap_rule(V, category, caps)
        n = sr.shape[0] // world
        mine = sr[rank * n:(rank + 1) * n]
        before = D.STATS['count']
        val, ids, complete = model.recommend_capped(mine, k=SPLIT_K, rule=rule, return_complete=True)
        used = D.STATS['count'] - before
        before = D.STATS['count']
        model.recommend_capped(mine, k=SPLIT_K, rule=rule, pool=128)
        one_stage = D.STATS['count'] - before
        dist.barrier()                                   # (a rank that left early would leave the other one alone in here)
        q.put((rank, ids.tolist(), complete.tolist(), used, one_stage))
    finally:
        dist.destroy_process_group()


def test_data_parallel_ranks_take_the_fallback_together_when_one_ranks_sessions_need_it():
    """recommend_capped over a row-sharded table fed data-parallel: the 4096-item pool is a chain of collectives, so the
    decision to take it must be the same on every rank although only rank 1 holds an incomplete session - rank 0 follows
    (one more all-reduce), nobody waits alone, and every session gets the list of the larger pool"""
    import torch.multiprocessing as mp
    from test_dist_cpu import _free_port
    sr, _, category, caps, order = _split_case()
    stage1 = torch.tensor(co.capped(order[:, :128], category, caps, SPLIT_K)[1]) == SPLIT_K
    assert stage1[:4].all() and not stage1[4], 'the rule must bind for the sessions of rank 1 only: %s' % stage1.tolist()
    want = co.capped_lists(torch.zeros(order.shape), order, category, caps, SPLIT_K)[1]
    assert bool((want >= 0).all())
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_split_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=120) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    n = sr.shape[0] // world
    for rank, ids, complete, used, one_stage in res:
        assert ids == want[rank * n:(rank + 1) * n].tolist(), rank
        assert complete == [True] * n, rank                              # (V = 150: the 4096-item pool ends unfilled)
    assert res[0][3] == res[1][3] and res[0][4] == res[1][4], 'the ranks issued different numbers of collectives'
    assert res[0][3] > res[0][4] + 1, 'rank 0 did not follow into the larger pool'


def test_sharded_cap_select_two_ranks_equal_unsharded():
    """the pool holds global ids and the rule is replicated: every rank runs its local kernel and no collective follows - the
    unsharded oracle, replicated and data-parallel"""
    import torch.multiprocessing as mp
    from test_dist_cpu import _free_port
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_cap_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ids, val, rule = _cap_case()
    ref = [t.tolist() for t in _oracle_local().cap_select(ids, val, rule, 9)]
    assert ref[1] != [list(range(9))] * 8 and any(-1 in row for row in ref[1]) is False
    assert (ids >= 128).any() and (ids < 128).any()                      # the pools span both shards
    n = ids.shape[0] // world
    for rank, n_live, rep, dp in res:
        assert n_live == (128, 22)[rank]
        assert rep == ref, rank
        assert dp == [x[rank * n:(rank + 1) * n] for x in ref], rank
