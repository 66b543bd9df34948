"""CPU side of the served-rank evaluation: the C ABI of srec_score_ahead (prototype and refusals, fake pointers never followed),
the argument checks of model.served_rank, the metric arithmetic (train.metrics_from_served_ranks), the sharded route
dist.VocabParallel.ahead over gloo (plain-torch stand-in for the kernel), scripts/evaluate.py's flags,
train.evaluate_served on a materialising model, and the oracle's own interval widths at the shapes of the GPU file."""
import importlib
import json
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import rank_served_oracle as ro
import served_abi
from test_dist_cpu import FakeModel, TorchLocal, _free_port
from test_served_args_cpu import GOOD
from util import GOLDEN, ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
NINF = float('-inf')
REST = dict(labels=0x3000, target=0x4000, floor=None, ahead=0x5000, ws=None)


# ------------------------------------------------------------------------------------------- C ABI
def _call(args, **kw):
    L = pkg('_lib')
    rest = [n for _, n in L.lib.protos['srec_score_ahead'][1:]]
    assert set(rest) == set(REST) | {'stream'}
    return served_abi.call(L.lib.load().srec_score_ahead, rest, args, **kw)


def test_prototype_as_declared():
    assert served_abi.proto('srec_score_ahead') == [('const void*', 'served'), ('const int*', 'labels'), ('const float*', 'target'),
                                                    ('const float*', 'floor'), ('int*', 'ahead'), ('void*', 'ws'), ('void*', 'stream')]
    assert served_abi.proto('srec_score_ahead_ws') == [('int', 'B'), ('int', 'V'), ('int', 'd'), ('int', 'C'), ('int', 'L'), ('long*', 'bytes')]
    # the rank entry point beside it is what it was
    assert served_abi.proto('srec_score_rank') == [('const void*', 'served'), ('const int*', 'labels'), ('float*', 'target'),
                                                   ('int', 'target_given'), ('int*', 'rank'), ('void*', 'ws'), ('void*', 'stream')]


def test_refusals_ahead_of_any_launch():
    L = pkg('_lib')
    good = {**GOOD, **REST}
    assert _call(good, null=True) == 1001
    nothing = {n: (None if v is None or v >= 0x1000 else 0) for n, v in good.items()}
    assert _call(nothing, null=True) == 1001                                # also with nothing else valid
    for change in (dict(d=30), dict(C=5), dict(L=65), dict(sr=0x1004), dict(E=0x2008), dict(ld_e=30), dict(id_lo=-1),
                   dict(listed_mode=2), dict(G=0), dict(G=2), dict(group=0x7001), dict(bias=0x6002),
                   dict(labels=None), dict(target=None), dict(ahead=None), dict(floor=0x5002), dict(target=0x4001),
                   dict(labels=0x3002)):
        assert _call({**good, **change}) == 1001, change
    assert _call({**good, 'B': 0, 'd': 30, 'G': 0}) == 0                     # no sessions: nothing to do, ahead of the checks
    # what srec_score_rank refuses is this entry point's purpose: a bias, a grouped bias, SREC_LISTED_DROP, a floor and ids
    # beyond int32 pass the checks.  With fake pointers the call must not launch, so it is made with B = 0; that the real
    # call accepts them is tests/test_rank_served_gpu.py's
    for change in (dict(bias=0x6000), dict(bias=0x6000, ld_bias=10, group=0x7000, G=3),
                   dict(listed_mode=L.CONST['SREC_LISTED_DROP'], listed=0x9000, L=5), dict(floor=0x5000), dict(id_lo=2 ** 31 - 5)):
        assert _call({**good, **change, 'B': 0}) == 0, change
    # the workspace size is a token, and the shape contract is checked there too
    import ctypes
    n = ctypes.c_long(-1)
    ws = L.lib.load().srec_score_ahead_ws
    assert ws(2, 10, 32, 1, 0, ctypes.addressof(n)) == 0 and 0 < n.value <= 64
    assert ws(2, 10, 30, 1, 0, ctypes.addressof(n)) == 1001 and ws(2, 10, 32, 5, 0, ctypes.addressof(n)) == 1001
    assert ws(2, 10, 32, 1, 0, None) == 1001


# ------------------------------------------------------------------------------------------- model.served_rank: checks
def test_served_rank_refuses_bad_arguments_before_anything_runs(monkeypatch):
    sp = pkg()
    V = 50
    model = sp.SRGNN(V, 32, 1).train()

    def never(*a, **k):
        raise AssertionError('something ran although the arguments are refused')
    monkeypatch.setattr(model, 'session_repr', never)
    for fn in ('score_ahead', 'score_items', 'score_cutoff'):
        monkeypatch.setattr(pkg('ops'), fn, never)
    ok = torch.zeros(V)
    nan = ok.clone()
    nan[7] = float('nan')
    lab = torch.tensor([1, 2])
    cases = ((dict(labels=lab, item_bias=torch.zeros(V + 1)), r'served_rank: item_bias must be a floating tensor \[50\] or \[G, 50\]'),
             (dict(labels=lab, item_bias=nan), r'served_rank: item_bias holds NaN or \+inf'),
             (dict(labels=lab, item_group=torch.tensor([0, 1])), 'served_rank: item_group is given without an item_bias'),
             (dict(labels=lab, item_bias=torch.stack([ok, ok]), item_group=torch.tensor([0, 2])), r'served_rank: .*row id outside \[0, 2\)'),
             (dict(labels=torch.tensor([1, V])), r'served_rank: label 50; item ids are in \[0, 50\)'),
             (dict(labels=torch.tensor([1.0, 2.0])), 'served_rank: labels must be an integer tensor'),
             (dict(labels=lab, top_k=0), 'served_rank: top_k = 0'),
             (dict(labels=lab, top_p=0.0), 'served_rank: top_p = 0.0'),
             (dict(labels=lab, min_p=1.5), 'served_rank: min_p = 1.5'),
             (dict(labels=lab, temperature=0.0), 'served_rank: temperature = 0.0'),
             (dict(labels=lab, top_k=3, temperature=float('inf')), 'served_rank: temperature = inf'))
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg):
            model.served_rank(None, **kw)
    assert model.training                               # nothing ran, nothing was switched
    good = ok.clone()
    good[3], good[4] = NINF, -2.5
    with pytest.raises(AssertionError, match='something ran'):       # a fine call reaches the encoder
        model.served_rank(None, labels=torch.tensor([1, -1]), item_bias=good, top_k=5)
    assert model.training


def test_score_ahead_checks_its_operands_on_cpu_tensors():
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(10, 8)
    lab, t = torch.tensor([1, 2, -1]), torch.zeros(3)
    with pytest.raises(ValueError, match='score_ahead: labels must hold 3 integer item ids'):
        ops.score_ahead(sr, E, None, lab[:2], t)
    with pytest.raises(ValueError, match='score_ahead: target must hold 3 floating numbers'):
        ops.score_ahead(sr, E, None, lab, lab)
    with pytest.raises(ValueError, match='score_ahead: floor must hold 3 floating numbers'):
        ops.score_ahead(sr, E, None, lab, t, floor=torch.zeros(2))
    with pytest.raises(ValueError, match=r'score_ahead: 65 listed items per session; csrc/rank_served\.hip'):
        ops.score_ahead(sr, E, None, lab, t, listed=torch.zeros(3, 65, dtype=torch.int64))
    with pytest.raises(ValueError, match='score_ahead: bias has 9 columns for 10 table rows'):
        ops.score_ahead(sr, E, None, lab, t, bias=torch.zeros(9))
    with pytest.raises(RuntimeError, match='need GPU'):                     # no fallback
        ops.score_ahead(sr, E, None, lab, t)
    assert ops.score_ahead(sr[:0], E, None, lab[:0], t[:0]).shape == (0,)   # nothing to do
    assert ops.score_ahead(sr, E[:0], None, lab, t).tolist() == [0, 0, 0]   # a shard without rows counts nothing
    assert pkg('srgnn')._ScoringMixin._ROUTES['ahead'] == ('score_ahead', {})


# ------------------------------------------------------------------------------------------- metrics
def test_metrics_from_served_ranks_hand_values():
    train = pkg('train')
    # best item, last inside @5, first outside @5, no label, filtered out (twice), last inside @20, first outside @20
    m = train.metrics_from_served_ranks(torch.tensor([0, 4, 5, -1, -2, -2, 19, 20]), (5, 20))
    n = 7.0
    exp = {
        'hit@5': 2 / n, 'mrr@5': (1 + 1 / 5) / n, 'ndcg@5': (1 + 1 / math.log2(6)) / n,
        'hit@20': 4 / n, 'mrr@20': (1 + 1 / 5 + 1 / 6 + 1 / 20) / n,
        'ndcg@20': (1 + 1 / math.log2(6) + 1 / math.log2(7) + 1 / math.log2(21)) / n,
        'shown': 5 / n,
    }
    assert set(m) == set(exp)
    for k, v in exp.items():
        assert abs(m[k] - v) < 1e-12, (k, m[k], v)
    # without a -2 the metrics are metrics_from_ranks' and everything is shown
    r = torch.tensor([0, 4, 5, -1, 19, 20])
    ms, mr = train.metrics_from_served_ranks(r, (5, 20)), train.metrics_from_ranks(r, (5, 20))
    assert ms.pop('shown') == 1.0 and ms == mr
    # nothing to average: no division by zero
    assert train.metrics_from_served_ranks(torch.tensor([-1, -1]), (10,)) == {'hit@10': 0.0, 'mrr@10': 0.0, 'ndcg@10': 0.0, 'shown': 0.0}
    assert train.metrics_from_served_ranks(torch.tensor([-2, -1]), (10,))['shown'] == 0.0


def test_served_ranks_from_scores_against_the_oracle():
    train = pkg('train')
    g = torch.Generator().manual_seed(3)
    B, V = 9, 40
    s = torch.randint(-6, 7, (B, V), generator=g).double() / 2              # ties everywhere
    bias = torch.randint(-2, 3, (2, V), generator=g).double() / 2
    bias[torch.rand(2, V, generator=g) < 0.3] = NINF
    group = torch.arange(B) % 2
    seen = torch.randint(-1, V, (B, 3), generator=g)
    labels = torch.randint(0, V, (B,), generator=g)
    labels[2], seen[3, 1] = -1, labels[3]
    rows = bias[group]
    drop = torch.zeros(B, V + 1, dtype=torch.bool).scatter_(1, torch.where(seen < 0, torch.full_like(seen, V), seen), True)[:, :V]
    elig = (rows != NINF) & ~drop
    got = train.served_ranks_from_scores(s, labels, item_bias=bias, item_group=group, seen=seen)
    ref = ro.served_ranks64(s + rows, elig, labels)
    assert torch.equal(got, ref) and got[2] == -1 and got[3] == -2 and int((got >= 0).sum()) > 0, (got, ref)
    # a top_k floor: the k-th best eligible score, ties with it kept
    k = 4
    se = torch.where(elig, s + rows, torch.full_like(s, NINF))
    floor = se.sort(1, descending=True).values[:, k - 1]
    got = train.served_ranks_from_scores(s, labels, item_bias=bias, item_group=group, seen=seen, top_k=k)
    assert torch.equal(got, ro.served_ranks64(s + rows, elig, labels, floor))
    assert bool(((got >= 0) | (got < 0)).all()) and int(got.max()) < V
    # no keywords: the ranks of ranks_from_scores
    assert torch.equal(train.served_ranks_from_scores(s, labels), train.ranks_from_scores(s, labels))


# ------------------------------------------------------------------------------------------- sharded route (gloo)
D_, B_, C_, L_ = 16, 12, 2, 4


class AheadLocal(TorchLocal):
    """TorchLocal + the ahead entry of dist.HipLocal, from the float64 oracle; the scores are rounded to fp32 first, so that
    a shard and the whole table compare the same numbers"""

    def ahead(self, srs, table, cs, labels, target, off_ex, off_in, listed, drop_listed, id_lo, floor=None, **bias):
        s, elig = ro.served64(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo)
        if bias.get('bias') is not None:                                    # (this shard's columns: local ids)
            from item_bias_oracle import bias_rows
            rows = bias_rows(bias['bias'], bias.get('group'), s.shape[0], 0, table.shape[0])
            s, elig = s + rows, elig & (rows != NINF)
        return ro.ahead_exact(s.float(), elig, labels, target, floor, id_lo).to(torch.int32)


def _case(V):
    g = torch.Generator().manual_seed(77 + V)
    eighth = lambda *shape: torch.randint(-8, 9, shape, generator=g).float() / 8      # exact products and sums
    table, srs = eighth(V, D_), eighth(C_, B_, D_)
    off_ex = -eighth(C_, B_).abs()
    off_in = off_ex + 0.5
    listed = torch.randint(0, V, (B_, L_), generator=g)
    listed[:, 3] = -1
    bias = eighth(2, V) * 2
    bias[0, ::5] = NINF
    bias[1, 1::3] = NINF
    group = torch.arange(B_) % 2
    labels = torch.randint(0, V, (B_,), generator=g)
    labels[4] = -1
    labels[7] = listed[7, 0]                                                # a label its own session lists
    return table, srs, off_ex, off_in, listed, bias, group, labels


def _whole(V, drop):
    """(count, target, floor) on the whole table"""
    table, srs, off_ex, off_in, listed, bias, group, labels = _case(V)
    s, elig = ro.served64(srs, table, None, off_ex, off_in, listed, drop, 0, bias, group)
    s = s.float()
    target = torch.where(elig, s, torch.full_like(s, NINF)).gather(1, labels.clamp(min=0)[:, None])[:, 0]
    floor = ro.median_floor(s.double(), elig)
    return ro.ahead_exact(s, elig, labels, target, floor), target, floor


def _worker(rank, world, port, V, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, srs, off_ex, off_in, listed, bias, group, labels = _case(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=AheadLocal())
        shard = model._table().detach()
        n = B_ // world
        sl = slice(rank * n, (rank + 1) * n)
        out = {}
        with torch.no_grad():
            for drop in (False, True):
                _, target, floor = _whole(V, drop)
                out[drop, False] = vp.ahead(list(srs), shard, None, labels, target, off_ex, off_in, listed, drop, bias=bias,
                                            group=group, floor=floor).tolist()
                out[drop, True] = vp.ahead(list(srs[:, sl]), shard, None, labels[sl], target[sl], off_ex[:, sl], off_in[:, sl],
                                           listed[sl], drop, data_parallel=True, bias=bias, group=group[sl], floor=floor[sl]).tolist()
        q.put((rank, vp.n_live, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world,V', [(2, 150), (2, 40), (3, 150), (3, 40)])
def test_sharded_ahead_equals_the_whole_table_oracle(world, V):
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
        assert max(ref) > 0 and ref[4] == 0
        for rank, n_live, out in res:
            assert n_live == live[rank]
            assert out[drop, False] == ref, (world, V, rank, drop, 'replicated')
            assert out[drop, True] == ref[rank * n:(rank + 1) * n], (world, V, rank, drop, 'data_parallel')


# ------------------------------------------------------------------------------------------- scripts/evaluate.py
def _launcher():
    sys.path.insert(0, SCRIPTS)
    try:
        return importlib.import_module('evaluate')
    finally:
        sys.path.remove(SCRIPTS)


def test_launcher_flags_and_argument_errors(tmp_path, capsys):
    ev = _launcher()
    base = ['--checkpoint', 'c.pt', '--dataset-dir', os.path.join(ROOT, 'datasets', 'sample')]
    args = ev.parse(base)
    assert args.model == 'SRGNN' and args.cutoffs == (5, 10, 20) and not args.exclude_seen and args.catalog is None
    assert args.temperature == 1.0 and args.sample_top_k is None and args.precision == 'fp32'
    deny = tmp_path / 'deny.txt'
    deny.write_text('3\n7\n')
    args = ev.parse(base + ['--model', 'MSGIFSR', '--extra', '--fusion', '--cutoffs', '1,50', '--exclude-seen', '--deny', str(deny),
                            '--sample-top-k', '100', '--sample-top-p', '0.9', '--sample-min-p', '0.01', '--temperature', '0.5'])
    assert args.cutoffs == (1, 50) and args.catalog == {'deny': [3, 7]} and args.extra and args.embedding_dim == 256
    kw = ev.served_keywords(args, 'BIAS')
    assert kw == dict(exclude_seen=True, item_bias='BIAS', top_k=100, top_p=0.9, min_p=0.01, temperature=0.5)
    line = json.loads(ev.report({'hit@1': 0.5, 'shown': 1.0}, 7, args))
    assert line['metrics'] == {'hit@1': 0.5, 'shown': 1.0} and line['sessions'] == 7
    assert line['flags']['cutoffs'] == [1, 50] and line['flags']['deny'] == str(deny) and line['flags']['exclude_seen'] is True
    bad = tmp_path / 'bad.txt'
    bad.write_text('99999999\n')
    for extra in (['--cutoffs', '0,5'], ['--cutoffs', ''], ['--sample-top-k', '0'], ['--sample-top-p', '1.0'], ['--sample-min-p', '0'],
                  ['--temperature', '0'], ['--batch-size', '0'], ['--deny', str(bad)], ['--allow', str(tmp_path / 'missing.txt')]):
        with pytest.raises(SystemExit):
            ev.parse(base + extra)
    with pytest.raises(SystemExit):
        ev.parse(['--dataset-dir', 'x'])                # --checkpoint is required
    capsys.readouterr()


def test_evaluate_served_without_keywords_equals_the_rank_evaluation_on_a_cpu_model():
    from test_rank_cpu import _evaluate_fixture
    train = pkg('train')
    _, model, batches = _evaluate_fixture(4)
    cpu = torch.device('cpu')
    want = train.evaluate(model, batches, cpu, method='rank', cutoffs=(5, 10, 20))
    got = train.evaluate_served(model, batches, cpu, (5, 10, 20))
    assert got.pop('shown') == 1.0 and got == want
    # a deny-list on the first batch's labels: those sessions are misses at every cutoff and stay in the denominator
    deny = torch.zeros(3429)
    deny[batches[0][1]] = NINF
    m = train.evaluate_served(model, batches, cpu, (5, 10, 20), item_bias=deny)
    assert 0.0 < m['shown'] <= 0.75 and m['hit@5'] <= m['hit@20'] <= m['shown']
    with pytest.raises(ValueError, match='exclude_seen on the materialised route'):
        train.evaluate_served(model, batches, cpu, (5,), exclude_seen=True)
    import src.utils.train as st
    assert st.evaluate_served is train.evaluate_served and st.metrics_from_served_ranks is train.metrics_from_served_ranks


# ------------------------------------------------------------------------------------------- the oracle at the GPU shapes
@pytest.mark.parametrize('B,V,d,C', ro.SHAPES)
def test_oracle_intervals_at_the_gpu_shapes_are_not_vacuous(B, V, d, C):
    """at TOL = 1e-4 the [lo, hi] interval of every kernel case stays narrower than 16 (the cap of tests/test_rank_gpu.py),
    the exact count lies inside it, and the cases hold what they are meant to hold"""
    case = ro.kernel_case(B, V, d, C)
    labels = case['labels']
    assert int((labels < 0).sum()) == 2 and case['bias_vec'][labels[1]] == NINF
    assert bool((case['listed'][::3, 2] == labels[::3]).all())
    widest = 0
    for lists, bias, floored, with_cs in ro.variants():
        s, elig = ro.served64(case['srs'], case['E'], id_lo=0, **ro.variant(case, lists, bias, with_cs))
        target = torch.where(elig, s, torch.full_like(s, NINF)).gather(1, labels.clamp(min=0)[:, None])[:, 0].float()
        floor = ro.median_floor(s, elig) if floored else None
        lo, hi = ro.ahead_interval(s, elig, labels, target, ro.TOL, floor)
        exact = ro.ahead_exact(s, elig, labels, target.double(), floor)
        assert bool(((lo <= exact) & (exact <= hi)).all()), (lists, bias, floored)
        assert int((hi - lo).max()) < ro.MAX_WIDTH, (lists, bias, floored, int((hi - lo).max()))
        widest = max(widest, int((hi - lo).max()))
        assert int(exact.max()) > V // 20 and exact[5] == 0
        if floored:
            live = labels >= 0
            below = (target < floor)[live & (target > NINF)]
            assert 0 < int(below.sum()) < int(below.numel())                # some labels below the floor, some not
        if lists == 'drop':
            assert bool((target[::3][labels[::3] >= 0] == NINF).all())      # a dropped label scores -inf
    print('shape', (B, V, d, C), 'widest interval', widest)
