"""CPU side of the many-targets served rank: the C ABI of srec_score_ahead_many (prototype and refusals, fake pointers never
followed), the argument checks of model.rank_items and ops.score_ahead_many, ops.ahead_among_targets against a brute-force
loop, the rest-of-session metric arithmetic (train.metrics_from_item_ranks), train.item_ranks_from_scores against the oracle,
dataset.rest_items, the sharded route dist.VocabParallel.ahead_many over gloo (plain-torch stand-in for the kernel),
scripts/evaluate.py's new flags, and the oracle's own interval widths at the shapes of the GPU file."""
import ctypes
import json
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_many_oracle as mo
import rank_served_oracle as ro
import served_abi
from test_dist_cpu import FakeModel, _free_port
from test_rank_served_cpu import AheadLocal, B_, _case, _launcher
from test_served_args_cpu import GOOD
from util import ROOT, pkg

NINF = float('-inf')
REST = dict(items=0x3000, target=0x4000, ld_items=5, M=5, floor=None, among_targets=1, ahead=0x5000, ws=None)


# ------------------------------------------------------------------------------------------- C ABI
def _call(args, **kw):
    L = pkg('_lib')
    rest = [n for _, n in L.lib.protos['srec_score_ahead_many'][1:]]
    assert set(rest) == set(REST) | {'stream'}
    return served_abi.call(L.lib.load().srec_score_ahead_many, rest, args, **kw)


def test_prototypes_as_declared():
    assert served_abi.proto('srec_score_ahead_many') == [
        ('const void*', 'served'), ('const int*', 'items'), ('const float*', 'target'), ('long', 'ld_items'), ('int', 'M'),
        ('const float*', 'floor'), ('int', 'among_targets'), ('int*', 'ahead'), ('void*', 'ws'), ('void*', 'stream')]
    assert served_abi.proto('srec_score_ahead_many_ws') == [('int', 'B'), ('int', 'V'), ('int', 'd'), ('int', 'C'), ('int', 'L'),
                                                            ('int', 'M'), ('long*', 'bytes')]
    assert pkg('_lib').CONST['SREC_AHEAD_MAXT'] == 64
    # the single-label entry point beside it is what it was
    assert served_abi.proto('srec_score_ahead') == [('const void*', 'served'), ('const int*', 'labels'), ('const float*', 'target'),
                                                    ('const float*', 'floor'), ('int*', 'ahead'), ('void*', 'ws'), ('void*', 'stream')]


def test_refusals_ahead_of_any_launch():
    L = pkg('_lib')
    good = {**GOOD, **REST, 'stream': None}
    assert _call(good, null=True) == 1001
    nothing = {n: (None if v is None or v >= 0x1000 else 0) for n, v in good.items()}
    assert _call(nothing, null=True) == 1001                                # also with nothing else valid
    for change in (dict(d=30), dict(C=5), dict(L=65), dict(sr=0x1004), dict(E=0x2008), dict(ld_e=30), dict(id_lo=-1),
                   dict(listed_mode=2), dict(G=0), dict(G=2), dict(group=0x7001), dict(bias=0x6002),
                   dict(M=0), dict(M=65, ld_items=65), dict(M=-1), dict(ld_items=4), dict(items=None), dict(target=None),
                   dict(ahead=None), dict(floor=0x5002), dict(target=0x4001), dict(items=0x3002), dict(ahead=0x5001)):
        assert _call({**good, **change}) == 1001, change
    assert _call({**good, 'B': 0, 'd': 30, 'G': 0, 'M': 0}) == 0             # no sessions: nothing to do, ahead of the checks
    # a bias, a grouped bias, SREC_LISTED_DROP, a floor, ids beyond int32, M at both ends and a wider row stride pass the
    # checks.  With fake pointers the call must not launch, so it is made with B = 0; that the real call accepts them is
    # tests/test_rank_many_gpu.py's
    for change in (dict(bias=0x6000), dict(bias=0x6000, ld_bias=10, group=0x7000, G=3),
                   dict(listed_mode=L.CONST['SREC_LISTED_DROP'], listed=0x9000, L=5), dict(floor=0x5000), dict(id_lo=2 ** 31 - 5),
                   dict(M=1), dict(M=64, ld_items=64), dict(ld_items=100), dict(among_targets=0)):
        assert _call({**good, **change, 'B': 0}) == 0, change
    # the workspace size is a token, and the shape contract is checked there too
    n = ctypes.c_long(-1)
    ws = L.lib.load().srec_score_ahead_many_ws
    assert ws(2, 10, 32, 1, 0, 64, ctypes.addressof(n)) == 0 and 0 < n.value <= 64
    for bad in ((2, 10, 30, 1, 0, 5), (2, 10, 32, 5, 0, 5), (2, 10, 32, 1, 0, 0), (2, 10, 32, 1, 0, 65)):
        assert ws(*bad, ctypes.addressof(n)) == 1001, bad
    assert ws(2, 10, 32, 1, 0, 5, None) == 1001


# ------------------------------------------------------------------------------------------- model.rank_items: checks
def test_rank_items_refuses_bad_arguments_before_anything_runs(monkeypatch):
    sp = pkg()
    V = 50
    model = sp.SRGNN(V, 32, 1).train()

    def never(*a, **k):
        raise AssertionError('something ran although the arguments are refused')
    monkeypatch.setattr(model, 'session_repr', never)
    for fn in ('score_ahead', 'score_ahead_many', 'score_items', 'score_cutoff'):
        monkeypatch.setattr(pkg('ops'), fn, never)
    ok = torch.zeros(V)
    nan = ok.clone()
    nan[7] = float('nan')
    it = torch.tensor([[1, 2, -1], [4, 3, 9]])
    cases = ((dict(items=it, item_bias=torch.zeros(V + 1)), r'rank_items: item_bias must be a floating tensor \[50\] or \[G, 50\]'),
             (dict(items=it, item_bias=nan), r'rank_items: item_bias holds NaN or \+inf'),
             (dict(items=it, item_group=torch.tensor([0, 1])), 'rank_items: item_group is given without an item_bias'),
             (dict(items=torch.tensor([[1, V]])), r'rank_items: item id 50; ids are in \[0, 50\)'),
             (dict(items=torch.tensor([[1, -2]])), r'rank_items: item id -2; ids are in \[0, 50\)'),
             (dict(items=torch.tensor([[1.0, 2.0]])), 'rank_items: items must be an integer tensor'),
             (dict(items=torch.zeros(2, 2, 2, dtype=torch.long)), 'rank_items: items must be an integer tensor'),
             (dict(items=torch.tensor([[1, 2, 3], [4, 9, 4]])), 'rank_items: an item id appears twice in a row'),
             (dict(items=torch.tensor([3, 5, 3])), 'rank_items: an item id appears twice in a row'),
             (dict(items=torch.arange(65)[None, :] % V), 'rank_items: 65 items per session; between 1 and 64'),
             (dict(items=torch.zeros(2, 0, dtype=torch.long)), 'rank_items: 0 items per session'),
             (dict(items=it, top_k=0), 'rank_items: top_k = 0'),
             (dict(items=it, top_p=0.0), 'rank_items: top_p = 0.0'),
             (dict(items=it, min_p=1.5), 'rank_items: min_p = 1.5'),
             (dict(items=it, temperature=0.0), 'rank_items: temperature = 0.0'))
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            model.rank_items(None, **kw)
    assert model.training                               # nothing ran, nothing was switched
    good = ok.clone()
    good[3], good[4] = NINF, -2.5
    # a fine call reaches the encoder: two -1 in a row are padding, not a repeated id
    for items in (torch.tensor([[1, -1, -1], [4, 3, 9]]), torch.tensor([7, 8], dtype=torch.int32)):
        with pytest.raises(AssertionError, match='something ran'):
            model.rank_items(None, items=items, item_bias=good, top_k=5)
    assert model.training
    assert pkg('srgnn')._ScoringMixin._ROUTES['ahead_many'] == ('score_ahead_many', {})
    assert pkg('srgnn')._ScoringMixin._ROUTES['ahead'] == ('score_ahead', {})


def test_score_ahead_many_checks_its_operands_on_cpu_tensors():
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(10, 8)
    it, t = torch.tensor([[1, 2], [3, -1], [4, 5]]), torch.zeros(3, 2)
    with pytest.raises(ValueError, match=r'score_ahead_many: items must hold \[3, M\] integer item ids'):
        ops.score_ahead_many(sr, E, None, it[:2], t)
    with pytest.raises(ValueError, match=r'score_ahead_many: items must hold \[3, M\] integer item ids'):
        ops.score_ahead_many(sr, E, None, it.float(), t)
    with pytest.raises(ValueError, match=r'score_ahead_many: target must hold \[3, 2\] floating numbers'):
        ops.score_ahead_many(sr, E, None, it, it)
    with pytest.raises(ValueError, match=r'score_ahead_many: target must hold \[3, 2\] floating numbers'):
        ops.score_ahead_many(sr, E, None, it, t[:, :1])
    with pytest.raises(ValueError, match='score_ahead_many: 65 items per session'):
        ops.score_ahead_many(sr, E, None, torch.zeros(3, 65, dtype=torch.long), torch.zeros(3, 65))
    with pytest.raises(ValueError, match='score_ahead_many: 0 items per session'):
        ops.score_ahead_many(sr, E, None, it[:, :0], t[:, :0])
    with pytest.raises(ValueError, match='score_ahead_many: floor must hold 3 floating numbers'):
        ops.score_ahead_many(sr, E, None, it, t, floor=torch.zeros(2))
    with pytest.raises(ValueError, match=r'score_ahead_many: 65 listed items per session; csrc/rank_served_many\.hip'):
        ops.score_ahead_many(sr, E, None, it, t, listed=torch.zeros(3, 65, dtype=torch.int64))
    with pytest.raises(ValueError, match='score_ahead_many: bias has 9 columns for 10 table rows'):
        ops.score_ahead_many(sr, E, None, it, t, bias=torch.zeros(9))
    with pytest.raises(RuntimeError, match='need GPU'):                     # no fallback
        ops.score_ahead_many(sr, E, None, it, t)
    assert ops.score_ahead_many(sr[:0], E, None, it[:0], t[:0]).shape == (0, 2)          # nothing to do
    # a shard without rows: the targets among themselves (equal values: the lower id first), or nothing
    assert ops.score_ahead_many(sr, E[:0], None, it, t).tolist() == [[0, 1], [0, 0], [0, 1]]
    assert ops.score_ahead_many(sr, E[:0], None, it, t, among_targets=False).tolist() == [[0, 0]] * 3
    score = pkg('score')
    assert ops.score_ahead_many is score.score_ahead_many and ops.ahead_among_targets is score.ahead_among_targets


def test_ahead_among_targets_against_a_brute_force_loop():
    ops = pkg('ops')
    g = torch.Generator().manual_seed(21)
    B, M = 17, 9
    items = torch.stack([torch.randperm(40, generator=g)[:M] for _ in range(B)])
    items[torch.rand(B, M, generator=g) < 0.2] = -1
    target = torch.randint(-3, 4, (B, M), generator=g).float() / 2           # half-integers: ties everywhere
    target[torch.rand(B, M, generator=g) < 0.15] = NINF
    floor = torch.randint(-3, 3, (B,), generator=g).float() / 2
    for fl in (None, floor):
        got = ops.ahead_among_targets(items, target, fl)
        ref = mo.among_exact(items, target, fl)
        assert got.dtype == torch.int32 and torch.equal(got.long(), ref), (fl, got, ref)
        assert int(ref.max()) > 2 and bool((got[items < 0] == 0).all())
        # the targets that count get pairwise distinct positions among themselves
        cnt = (items >= 0) & (target > NINF) & (~(target < fl[:, None]) if fl is not None else True)
        for b in range(B):
            pos = sorted(got[b][cnt[b]].tolist())
            assert pos == list(range(len(pos))), (b, pos)
    assert int((mo.among_exact(items, target, floor) != mo.among_exact(items, target)).sum()) > 0     # the floor matters
    assert ops.ahead_among_targets(items[:, :1], target[:, :1]).abs().sum() == 0                     # one target: nothing


# ------------------------------------------------------------------------------------------- metrics
def test_metrics_from_item_ranks_hand_values():
    train = pkg('train')
    m = train.metrics_from_item_ranks(torch.tensor([[0, 3, -2]]), (5,))
    exp = {'hit@5': 1.0, 'recall@5': 2 / 3, 'precision@5': 2 / 5, 'mrr@5': 1.0, 'map@5': (1 + 2 / 4) / 3,
           'ndcg@5': (1 + 1 / math.log2(5)) / (1 + 1 / math.log2(3) + 1 / 2), 'shown': 2 / 3}
    assert set(m) == set(exp)
    for k, v in exp.items():
        assert abs(m[k] - v) < 1e-12, (k, m[k], v)
    assert abs(m['ndcg@5'] - 0.67139) < 1e-5 and m['map@5'] == 0.5
    # two cases, an all-empty row between them is no case; cutoff 2 is below the second case's number of targets
    r = torch.tensor([[0, 3, -2, -1], [-1, -1, -1, -1], [1, 0, 5, 2]])
    m = train.metrics_from_item_ranks(r, (2, 5))
    ideal2 = 1 + 1 / math.log2(3)
    exp = {'hit@2': 1.0, 'recall@2': (1 / 3 + 2 / 4) / 2, 'precision@2': (1 / 2 + 2 / 2) / 2, 'mrr@2': 1.0,
           'map@2': ((1 / 1) / 2 + (1 / 1 + 2 / 2) / 2) / 2, 'ndcg@2': (1 / ideal2 + 1.0) / 2,
           'hit@5': 1.0, 'recall@5': (2 / 3 + 3 / 4) / 2, 'precision@5': (2 / 5 + 3 / 5) / 2, 'mrr@5': 1.0,
           'map@5': (0.5 + (1 + 1 + 1) / 4) / 2,
           'ndcg@5': ((1 + 1 / math.log2(5)) / (1 + 1 / math.log2(3) + 1 / 2)
                      + (1 + 1 / math.log2(3) + 1 / 2) / (1 + 1 / math.log2(3) + 1 / 2 + 1 / math.log2(5))) / 2,
           'shown': 6 / 7}
    assert set(m) == set(exp)
    for k, v in exp.items():
        assert abs(m[k] - v) < 1e-12, (k, m[k], v)
    # one target per case: hit = recall, and hit / mrr / ndcg / shown are metrics_from_served_ranks'
    one = torch.tensor([0, 4, 5, -1, -2, -2, 19, 20])
    mi, ms = train.metrics_from_item_ranks(one[:, None], (5, 20)), train.metrics_from_served_ranks(one, (5, 20))
    for k in (5, 20):
        assert mi['hit@%d' % k] == mi['recall@%d' % k]
        assert abs(mi['map@%d' % k] - mi['mrr@%d' % k]) < 1e-12
    for k, v in ms.items():
        assert abs(mi[k] - v) < 1e-12, (k, mi[k], v)
    # nothing to average: no division by zero
    none = train.metrics_from_item_ranks(torch.tensor([[-1, -1], [-1, -1]]), (10,))
    assert none == {'hit@10': 0.0, 'recall@10': 0.0, 'precision@10': 0.0, 'mrr@10': 0.0, 'map@10': 0.0, 'ndcg@10': 0.0, 'shown': 0.0}
    assert train.metrics_from_item_ranks(torch.zeros(0, 3, dtype=torch.long), (10,)) == none
    gone = train.metrics_from_item_ranks(torch.tensor([[-2, -1]]), (10,))
    assert gone['shown'] == 0.0 and gone['recall@10'] == 0.0 and gone['ndcg@10'] == 0.0
    import src.utils.train as st
    assert st.evaluate_rest is train.evaluate_rest and st.metrics_from_item_ranks is train.metrics_from_item_ranks
    assert st.item_ranks_from_scores is train.item_ranks_from_scores


def test_item_ranks_from_scores_against_the_oracle():
    train = pkg('train')
    g = torch.Generator().manual_seed(3)
    B, V, M = 9, 40, 6
    s = torch.randint(-6, 7, (B, V), generator=g).double() / 2              # ties everywhere
    bias = torch.randint(-2, 3, (2, V), generator=g).double() / 2
    bias[torch.rand(2, V, generator=g) < 0.3] = NINF
    group = torch.arange(B) % 2
    seen = torch.randint(-1, V, (B, 3), generator=g)
    items = torch.stack([torch.randperm(V, generator=g)[:M] for _ in range(B)])
    items[2, 1], items[4, :] = -1, -1
    seen[3, 1] = items[3, 0]
    rows = bias[group]
    drop = torch.zeros(B, V + 1, dtype=torch.bool).scatter_(1, torch.where(seen < 0, torch.full_like(seen, V), seen), True)[:, :V]
    elig = (rows != NINF) & ~drop
    k = 7
    floor = torch.where(elig, s + rows, torch.full_like(s, NINF)).sort(1, descending=True).values[:, k - 1]
    for kw, fl in ((dict(), None), (dict(top_k=k), floor)):
        got = train.item_ranks_from_scores(s, items, item_bias=bias, item_group=group, seen=seen, **kw)
        t64 = mo.target_values64(s + rows, elig, items)
        ahead = mo.ahead_many_exact(s + rows, elig, items, t64.float(), fl)
        shown = (t64 > NINF) & (~(t64 < fl[:, None]) if fl is not None else True)
        ref = torch.where(items < 0, torch.full_like(ahead, -1), torch.where(shown, ahead, torch.full_like(ahead, -2)))
        assert got.dtype == torch.int64 and torch.equal(got, ref), (kw, got, ref)
        assert got[2, 1] == -1 and bool((got[4] == -1).all()) and got[3, 0] == -2 and int((got >= 0).sum()) > B
        # column 0 alone is served_ranks_from_scores for those labels, up to the other targets ahead of it
        one = train.served_ranks_from_scores(s, items[:, 0], item_bias=bias, item_group=group, seen=seen, **kw)
        assert torch.equal(train.item_ranks_from_scores(s, items[:, :1], item_bias=bias, item_group=group, seen=seen, **kw)[:, 0], one)
    # a 1-D list is shared by all sessions
    shared = train.item_ranks_from_scores(s, items[0])
    assert torch.equal(shared, train.item_ranks_from_scores(s, items[0].expand(B, M)))


# ------------------------------------------------------------------------------------------- dataset.rest_items
def test_rest_items_on_hand_written_sessions():
    ds = pkg('dataset')
    sessions = [[5, 7, 5, 9, 7], [3, 4], [8], [1, 2, 3, 4, 5, 6]]
    data = ds.AugmentedDataset(sessions)
    assert len(data) == 4 + 1 + 0 + 5
    items, cut = data.rest_items(range(len(data)))
    assert items.dtype.name == 'int32' and cut == 0 and items.shape == (10, 5)
    want = [[7, 5, 9], [5, 9, 7], [9, 7], [7], [4], [2, 3, 4, 5, 6], [3, 4, 5, 6], [4, 5, 6], [5, 6], [6]]
    for i, row in enumerate(want):
        assert items[i].tolist() == row + [-1] * (5 - len(row)), i
        assert items[i, 0] == data[i][1]                                     # column 0 is the next-item label
    # M is the longest row of the call
    assert data.rest_items([3, 4])[0].tolist() == [[7], [4]]
    # more than max_targets distinct remaining items: the first ones are kept, and counted
    items, cut = data.rest_items(range(len(data)), max_targets=2)
    assert cut == 5 and items.shape == (10, 2)
    assert items.tolist() == [[7, 5], [5, 9], [9, 7], [7, -1], [4, -1], [2, 3], [3, 4], [4, 5], [5, 6], [6, -1]]
    assert data.rest_items([], 4)[0].shape == (0, 1)
    # the sample split (datasets/sample/test.txt): the figures the issue quotes
    test = ds.AugmentedDataset(ds.read_sessions(os.path.join(ROOT, 'datasets', 'sample', 'test.txt')))
    items, cut = test.rest_items(range(len(test)))
    assert cut == 0 and items.shape[1] <= 64 and bool((items[:, 0] >= 0).all())
    for row in items[:200]:
        live = row[row >= 0].tolist()
        assert len(set(live)) == len(live)


# ------------------------------------------------------------------------------------------- sharded route (gloo)
M_ = 5


class ManyLocal(AheadLocal):
    """AheadLocal + the ahead_many entry of dist.HipLocal, from the float64 oracle (N only: the caller adds A); the scores are
    rounded to fp32 first, so that a shard and the whole table compare the same numbers"""

    def ahead_many(self, srs, table, cs, items, target, off_ex, off_in, listed, drop_listed, id_lo, floor=None, **bias):
        s, elig = ro.served64(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo)
        if bias.get('bias') is not None:                                    # (this shard's columns: local ids)
            from item_bias_oracle import bias_rows
            rows = bias_rows(bias['bias'], bias.get('group'), s.shape[0], 0, table.shape[0])
            s, elig = s + rows, elig & (rows != NINF)
        return mo.ahead_many_exact(s.float(), elig, items, target, floor, id_lo, among_targets=False).to(torch.int32)


def _items(V):
    g = torch.Generator().manual_seed(5 + V)
    labels = _case(V)[-1]
    items = torch.stack([torch.randperm(V, generator=g)[:M_] for _ in range(B_)])
    items[:, 1:] = torch.where(items[:, 1:] == labels[:, None], torch.full_like(items[:, 1:], -1), items[:, 1:])
    items[:, 0] = labels                                                    # (one -1, one label its own session lists)
    items[2, 3] = -1
    return items


def _whole(V, drop):
    """(counts, target, floor) on the whole table"""
    table, srs, off_ex, off_in, listed, bias, group, _ = _case(V)
    items = _items(V)
    s, elig = ro.served64(srs, table, None, off_ex, off_in, listed, drop, 0, bias, group)
    s = s.float()
    target = mo.target_values64(s, elig, items).float()
    floor = ro.median_floor(s.double(), elig)
    return mo.ahead_many_exact(s, elig, items, target, floor), target, floor


def _worker(rank, world, port, V, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, srs, off_ex, off_in, listed, bias, group, _ = _case(V)
        items = _items(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=ManyLocal())
        shard = model._table().detach()
        n = B_ // world
        sl = slice(rank * n, (rank + 1) * n)
        out = {}
        with torch.no_grad():
            for drop in (False, True):
                _, target, floor = _whole(V, drop)
                out[drop, False] = vp.ahead_many(list(srs), shard, None, items, target, off_ex, off_in, listed, drop, bias=bias,
                                                 group=group, floor=floor).tolist()
                out[drop, True] = vp.ahead_many(list(srs[:, sl]), shard, None, items[sl], target[sl], off_ex[:, sl], off_in[:, sl],
                                                listed[sl], drop, data_parallel=True, bias=bias, group=group[sl],
                                                floor=floor[sl]).tolist()
        q.put((rank, vp.n_live, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world,V', [(2, 150), (2, 40), (3, 150), (3, 40)])
def test_sharded_ahead_many_equals_the_whole_table_oracle(world, V):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, V, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    live = {(2, 150): (128, 22), (2, 40): (40, 0), (3, 150): (64, 64, 22), (3, 40): (40, 0, 0)}[world, V]
    n = B_ // world
    for drop in (False, True):
        ref = _whole(V, drop)[0].tolist()
        assert max(max(r) for r in ref) > 0 and ref[4][0] == 0 and ref[2][3] == 0
        for rank, n_live, out in res:
            assert n_live == live[rank]
            assert out[drop, False] == ref, (world, V, rank, drop, 'replicated')
            assert out[drop, True] == ref[rank * n:(rank + 1) * n], (world, V, rank, drop, 'data_parallel')


# ------------------------------------------------------------------------------------------- scripts/evaluate.py
def test_launcher_protocol_flags_and_report_keys(capsys):
    ev = _launcher()
    base = ['--checkpoint', 'c.pt', '--dataset-dir', os.path.join(ROOT, 'datasets', 'sample')]
    args = ev.parse(base)
    assert args.protocol == 'next' and args.max_targets == 64
    line = json.loads(ev.report({'hit@1': 0.5, 'shown': 1.0}, 7, args))
    assert set(line) == {'metrics', 'sessions', 'flags'} and 'protocol' not in line['flags'] and 'max_targets' not in line['flags']
    args = ev.parse(base + ['--protocol', 'rest', '--max-targets', '8', '--cutoffs', '1,50', '--exclude-seen'])
    assert args.protocol == 'rest' and args.max_targets == 8
    line = json.loads(ev.report({'recall@1': 0.25, 'shown': 1.0, 'truncated': 3}, 7, args))
    assert set(line) == {'metrics', 'sessions', 'truncated', 'flags'}
    assert line['metrics'] == {'recall@1': 0.25, 'shown': 1.0} and line['truncated'] == 3 and line['sessions'] == 7
    assert line['flags']['protocol'] == 'rest' and line['flags']['max_targets'] == 8 and line['flags']['exclude_seen'] is True
    for extra in (['--protocol', 'all'], ['--max-targets', '0'], ['--max-targets', '65']):
        with pytest.raises(SystemExit):
            ev.parse(base + extra)
    capsys.readouterr()


def test_evaluate_rest_on_a_cpu_model():
    from test_rank_cpu import _evaluate_fixture
    train, ds = pkg('train'), pkg('dataset')
    _, model, batches = _evaluate_fixture(4)
    cpu = torch.device('cpu')

    class Pairs:
        """the fixture's batches as a dataset of one sample per batch row, its targets given directly"""

        def __init__(self, width):
            self.width = width

        def __len__(self):
            return len(batches)

        def __getitem__(self, i):
            return i

        def rest_items(self, idx, max_targets):
            labels = torch.cat([batches[i][1] for i in idx])
            extra = (labels[:, None] + 1 + torch.arange(self.width - 1)[None, :]) % 3429
            return torch.cat([labels[:, None], extra], 1)[:, :max_targets].int().numpy(), 0

    def collate(samples):
        assert len(samples) == 1
        return batches[samples[0]]
    # one target per case: the next-item protocol's numbers
    want = train.evaluate_served(model, batches, cpu, (5, 10, 20))
    got = train.evaluate_rest(model, Pairs(1), collate, cpu, 1, (5, 10, 20))
    assert got.pop('truncated') == 0
    for k, v in want.items():
        assert abs(got[k] - v) < 1e-12, (k, got[k], v)
    # three targets per case: recall cannot exceed hit, precision is hits / k
    got = train.evaluate_rest(model, Pairs(3), collate, cpu, 1, (5, 20), max_targets=3)
    assert set(got) == {m + '@%d' % k for m in ('hit', 'recall', 'precision', 'mrr', 'map', 'ndcg') for k in (5, 20)} | {'shown', 'truncated'}
    assert got['shown'] == 1.0 and got['recall@20'] <= got['hit@20'] and got['recall@5'] <= got['recall@20']
    with pytest.raises(ValueError, match='exclude_seen on the materialised route'):
        train.evaluate_rest(model, Pairs(2), collate, cpu, 1, (5,), exclude_seen=True)
    assert hasattr(ds.AugmentedDataset, 'rest_items')


# ------------------------------------------------------------------------------------------- the oracle at the GPU shapes
@pytest.mark.parametrize('B,V,d,C', ro.SHAPES)
def test_oracle_intervals_at_the_gpu_shapes_are_not_vacuous(B, V, d, C):
    """at TOL = 1e-4 the [lo, hi] interval of every (session, slot) stays narrower than 16, the exact count lies inside it, at
    most 5 % of the live finite slots have another target of their session within 2 TOL, and the targets hold what they are
    meant to hold"""
    case = ro.kernel_case(B, V, d, C)
    labels = case['labels']
    widest, closest = 0, 0.0
    for M in (5, 64):
        items = mo.targets(case, B, V, d, C, M)
        assert torch.equal(items[:, 0], labels) and int((items[:, 0] < 0).sum()) == 2
        for b in range(B):
            live = items[b][items[b] >= 0].tolist()
            assert len(set(live)) == len(live)
        assert case['bias_vec'][items[1, 0]] == NINF and bool((case['listed'][::3, 2] == items[::3, 0]).all())
        for lists, bias, floored, with_cs in [ro.variants()[i] for i in (3, 10, 13)]:      # three operand variants per shape
            s, elig = ro.served64(case['srs'], case['E'], id_lo=0, **ro.variant(case, lists, bias, with_cs))
            t64 = mo.target_values64(s, elig, items)
            target = t64.float()
            floor = ro.median_floor(s, elig) if floored else None
            lo, hi = mo.ahead_many_interval(s, elig, items, target, ro.TOL, floor)
            exact = mo.ahead_many_exact(s, elig, items, target, floor)
            assert bool(((lo <= exact) & (exact <= hi)).all()), (M, lists, bias, floored)
            assert int((hi - lo).max()) < ro.MAX_WIDTH, (M, lists, bias, floored, int((hi - lo).max()))
            widest = max(widest, int((hi - lo).max()))
            assert bool((exact[items < 0] == 0).all()) and int(exact.max()) > V // 20
            fin = (items >= 0) & (t64 > NINF)
            share = float(mo.close_targets(items, t64)[fin].float().mean())
            assert share <= 0.05, (M, lists, bias, floored, share)
            closest = max(closest, share)
    print('shape', (B, V, d, C), 'widest interval', widest, 'largest share of close targets', closest)
