"""CPU side of the per-session hide / boost lists: the oracle (tests/personal_oracle.py) against the top-k of the adjusted dense
row and the completeness rule, the argument checks of ops.personal_lists / ops.personal_merge / model.recommend_personal, the
export and what srec_personal_merge refuses ahead of any launch (fake pointers, never followed), and the launcher's flags."""
import os
import sys

import pytest
import torch

import personal_oracle as po
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
NINF = float('-inf')


# ------------------------------------------------------------------------------------------- the oracle
def test_oracle_by_hand():
    pool_ids = torch.tensor([[5, 2, -1, 9, 7, -1]])
    pool_val = torch.tensor([[3.0, 2.0, 7.0, 2.0, 1.0, 7.0]])
    items = torch.tensor([[9, -1, 4, 5, 9, 8]])                       # 9 twice: the first slot wins
    base = torch.tensor([[2.0, 0.0, -1.0, 3.0, 2.0, NINF]])
    bias = torch.tensor([[-0.5, 9.0, 3.0, NINF, 5.0, 4.0]])
    val, ids, src, hit, kept = po.merge(pool_ids, pool_val, items, base, bias, 6)
    # survivors 2 (2.0, slot 1) and 7 (1.0, slot 4); candidates 9 (1.5, list slot 0) and 4 (2.0, list slot 2); 5 hidden, 8 -inf
    assert ids.tolist() == [[2, 4, 9, 7, -1, -1]] and val.tolist() == [[2.0, 2.0, 1.5, 1.0, NINF, NINF]]
    assert src.tolist() == [[1, 6 + 2, 6 + 0, 4, -1, -1]] and hit.tolist() == [2] and kept.tolist() == [4]
    val, ids, src, hit, kept = po.merge(pool_ids, pool_val, items, base, None, 2)
    assert ids.tolist() == [[2, 7]] and src.tolist() == [[1, 4]] and hit.tolist() == [2] and kept.tolist() == [2]
    assert po.complete(hit, pool_ids, 2).tolist() == [True] and po.complete(hit, pool_ids[:, :5], 4).tolist() == [False]


@pytest.mark.parametrize('V', [5, 40, 300])
def test_oracle_equals_the_top_k_of_the_adjusted_dense_row_wherever_the_rule_says_complete(V):
    g = torch.Generator().manual_seed(V)
    n_complete = n_incomplete = n_differ = n_sum = 0
    for case in range(120):
        B = 4
        dense = (torch.randn(B, V, generator=g) * 2).round() / 2 if case % 2 else torch.randn(B, V, generator=g)
        dense[torch.rand(B, V, generator=g) < 0.1] = NINF
        M = int(torch.randint(1, min(V, 12) + 1, (1,), generator=g))
        k = int(torch.randint(1, min(V, 10) + 1, (1,), generator=g))
        whole = case % 3 == 0
        P = k + M if whole else int(torch.randint(1, k + M + 1, (1,), generator=g))
        n_sum += whole
        pool_ids = torch.full((B, P), -1, dtype=torch.int64)
        pool_val = torch.full((B, P), 7.0)
        items = torch.full((B, M), -1, dtype=torch.int64)
        for b in range(B):
            top, vals = po.dense_top(dense[b], P)
            pool_ids[b, :len(top)] = torch.tensor(top, dtype=torch.int64)
            pool_val[b, :len(top)] = torch.tensor(vals)
            m = int(torch.randint(0, M + 1, (1,), generator=g))
            head = torch.tensor((top + list(range(V)))[:max(2 * M, 1)]).unique()       # mostly the pool's head
            chosen = head[torch.randperm(head.numel(), generator=g)][:m]
            items[b, torch.randperm(M, generator=g)[:chosen.numel()]] = chosen
        base = torch.where(items >= 0, dense.gather(1, items.clamp(min=0)), torch.full((B, M), NINF))
        bias = torch.tensor(po.BIASES)[torch.randint(0, len(po.BIASES), (B, M), generator=g)] if case % 4 else None
        val, ids, src, hit, kept = po.merge(pool_ids, pool_val, items, base, bias, k)
        adjusted = dense.clone()
        t = po.new_values(base, bias)
        for b in range(B):
            for j in range(M):
                if items[b, j] >= 0:
                    adjusted[b, items[b, j]] = t[b, j]
        done = po.complete(hit, pool_ids, k)
        for b in range(B):
            top, vals = po.dense_top(adjusted[b], k)
            same = ids[b, :len(top)].tolist() == top and bool((ids[b, len(top):] == -1).all()) and \
                val[b, :len(top)].tolist() == vals and int(kept[b]) == len(top)
            if done[b]:
                n_complete += 1
                assert same, (case, b, ids[b].tolist(), top)
            else:
                assert not whole, 'a pool of k + M slots is always complete'
                n_incomplete += 1
                n_differ += not same
    assert n_sum > 0 and n_complete > 100
    if V > 5:                                      # (V = 5: every pool reaches the end of the catalogue)
        assert n_incomplete > 0 and n_differ > 0, 'no incomplete case differs: the flag shows nothing'


def test_random_cases_hit_the_pool_and_let_candidates_in():
    for B, P, M, K in ((1, 1, 1, 1), (33, 40, 20, 20), (5, 300, 172, 128)):
        pool_ids, pool_val, items, base, bias = po.random_case(B, P, M, seed=1)
        val, ids, src, hit, kept = po.merge(pool_ids, pool_val, items, base, bias, K)
        assert int(hit.sum()) > 0, (B, P, M, K)
        if P > 1:
            assert bool((src >= P).any()) and bool(((src >= 0) & (src < P)).any()), (B, P, M, K)
        filled = ids >= 0
        assert torch.equal(filled.sum(1).to(torch.int32), kept) and bool((val[~filled] == NINF).all())
        for b in range(B):                          # ordered by (value descending, id ascending), ids distinct
            pairs = [(-v + 0.0, i) for v, i in zip(val[b].tolist(), ids[b].tolist()) if i >= 0]
            assert pairs == sorted(pairs) and len(set(i for _, i in pairs)) == len(pairs), b
        none = po.merge(pool_ids, pool_val, items, base, None, K)
        assert not bool((none[2] >= P).any()) and torch.equal(none[3], hit)


# ------------------------------------------------------------------------------------------- ops
def test_personal_lists_pads_checks_and_refuses():
    ops = pkg('ops')
    rec = ops.personal_lists('t', [[3, 4, 5], [], [7]], None, 3, 10, 'cpu')
    assert isinstance(rec, ops.PersonalLists) and rec.M == 3 and rec.bias is None and rec.items.dtype == torch.int32
    assert rec.items.tolist() == [[3, 4, 5], [-1, -1, -1], [7, -1, -1]]
    rec = ops.personal_lists('t', [[3, 4], [5]], [[0.5, NINF], [1.0]], 2, 10, 'cpu')
    assert rec.bias.dtype == torch.float32 and rec.bias.tolist() == [[0.5, NINF], [1.0, 0.0]] and rec.M == 2
    rec = ops.personal_lists('t', torch.tensor([1, 2, -1]), torch.tensor([1.0, 2.0, float('nan')]).double(), 4, 10, 'cpu')
    assert rec.items.shape == (4, 3) and rec.items.is_contiguous() and rec.bias.shape == (4, 3)     # (a padding slot's bias is not looked at)
    rec = ops.personal_lists('t', torch.tensor([1, 2, -1]), None, None, 10, 'cpu')
    assert rec.items.shape == (1, 3)
    rec = ops.personal_lists('t', torch.tensor([[1, 2], [2, 1]], dtype=torch.int16), None, 2, 10, 'cpu')
    assert rec.items.tolist() == [[1, 2], [2, 1]]
    good = dict(items=torch.tensor([[1, 2], [3, 4]]), bias=torch.zeros(2, 2), B=2)
    for kw in (dict(items=torch.tensor([[1, 10], [3, 4]])), dict(items=torch.tensor([[1, -2], [3, 4]])),
               dict(items=torch.tensor([[1, 1], [3, 4]])), dict(items=torch.tensor([[1.0, 2.0], [3.0, 4.0]])),
               dict(items=torch.zeros(2, 2, dtype=torch.bool)), dict(items=torch.zeros(2, 2, 2, dtype=torch.int64)),
               dict(items=torch.zeros(2, 0, dtype=torch.int64), bias=None), dict(items=torch.arange(1025)[None] % 10, bias=None),
               dict(items=[[1, 2], [3, 'x']]), dict(items=None),
               dict(bias=torch.zeros(2, 2, dtype=torch.int64)), dict(bias=torch.zeros(2, 3)), dict(bias=torch.zeros(3, 2)),
               dict(bias=torch.tensor([[0.0, float('nan')], [0.0, 0.0]])), dict(bias=torch.tensor([[0.0, float('inf')], [0.0, 0.0]])),
               dict(B=3), dict(bias=[[0.0, 0.0], [0.0]])):
        a = dict(good, **kw)
        with pytest.raises(ValueError, match='^t: '):
            ops.personal_lists('t', a['items'], a['bias'], a['B'], 10, 'cpu')
    assert ops.personal_k('t', 20, 1024) == 20 and ops.personal_k('t', 3072, 1024) == 3072
    for k, M in ((0, 5), (3073, 1024), (4096, 1)):
        with pytest.raises(ValueError):
            ops.personal_k('t', k, M)


def test_ops_personal_merge_refuses_bad_arguments_before_any_launch():
    ops = pkg('ops')
    good = dict(pool_ids=torch.zeros(3, 10, dtype=torch.int64), pool_val=torch.zeros(3, 10),
                items=torch.arange(4).repeat(3, 1), base=torch.zeros(3, 4), bias=torch.zeros(3, 4), k=5)
    bad = [
        dict(k=0), dict(k=4097), dict(pool_ids=torch.zeros(3, 10)), dict(pool_ids=torch.zeros(30, dtype=torch.int64)),
        dict(pool_ids=torch.zeros(3, 10, dtype=torch.bool)), dict(pool_val=torch.zeros(3, 9)), dict(pool_val=torch.zeros(3, 10).double()),
        dict(items=torch.zeros(3, 4)), dict(items=torch.zeros(12, dtype=torch.int64)), dict(items=torch.arange(4).repeat(2, 1)),
        dict(base=torch.zeros(3, 5)), dict(base=torch.zeros(3, 4).double()), dict(bias=torch.zeros(3, 5)),
        dict(bias=torch.zeros(3, 4, dtype=torch.int64)),
        dict(pool_ids=torch.zeros(3, 4097, dtype=torch.int64), pool_val=torch.zeros(3, 4097)),
        dict(items=torch.arange(1025).repeat(3, 1), base=torch.zeros(3, 1025), bias=None),
        dict(items=torch.zeros(3, 0, dtype=torch.int64), base=torch.zeros(3, 0), bias=None),
        dict(items=torch.tensor([[0, 1, 2, 1]]).repeat(3, 1)),                 # an id twice in a row (checked=False)
        dict(pool_ids=good['pool_ids'].to('meta')), dict(pool_val=good['pool_val'].to('meta')), dict(items=good['items'].to('meta')),
        dict(base=good['base'].to('meta')), dict(bias=good['bias'].to('meta')),
    ]
    for kw in bad:
        a = dict(good, **kw)
        with pytest.raises(ValueError, match='^personal_merge: '):
            ops.personal_merge(a['pool_ids'], a['pool_val'], a['items'], a['base'], a['bias'], a['k'])
    # good arguments on CPU tensors get as far as the launch, which has no fallback
    for bias in (good['bias'], None):
        with pytest.raises(RuntimeError, match='GPU|libsrec'):
            ops.personal_merge(good['pool_ids'], good['pool_val'], good['items'], good['base'], bias, 5)
    with pytest.raises(RuntimeError, match='GPU|libsrec'):                      # a repeated id under checked=True is the kernel's
        ops.personal_merge(good['pool_ids'], good['pool_val'], torch.zeros(3, 4, dtype=torch.int64), good['base'], None, 5, checked=True)
    out = ops.personal_merge(torch.zeros(0, 10, dtype=torch.int64), torch.zeros(0, 10), torch.zeros(0, 4, dtype=torch.int32),
                             torch.zeros(0, 4), None, 5)
    assert [tuple(t.shape) for t in out] == [(0, 5), (0, 5), (0, 5), (0,), (0,)]
    assert [t.dtype for t in out] == [torch.float32] + [torch.int32] * 4


def _cpu_model(V=30, d=8):
    class TableOnly(pkg('srgnn')._ScoringMixin, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = torch.nn.Embedding(V, d)

        def session_repr(self, *a, **k):
            raise AssertionError('the model ran before its arguments were checked')
    return TableOnly()


def test_recommend_personal_checks_its_arguments_before_the_model_runs():
    m = _cpu_model()
    items = torch.tensor([[3, 4, -1], [5, 6, 7]])
    for kw in (dict(k=0, personal_items=items), dict(k=4094, personal_items=items), dict(k=10, pool=9, personal_items=items),
               dict(k=10, pool=4097, personal_items=items), dict(personal_items=torch.tensor([[3, 30]])),
               dict(personal_items=torch.tensor([[3, -2]])), dict(personal_items=torch.tensor([[3, 3]])),
               dict(personal_items=items.float()), dict(personal_items=torch.arange(1025) % 30),
               dict(personal_items=items, personal_bias=torch.zeros(2, 2)), dict(personal_items=items, personal_bias=items),
               dict(personal_items=items, personal_bias=torch.full((2, 3), float('inf'))),
               dict(personal_items=items, personal_bias=torch.full((2, 3), float('nan'))),
               dict(personal_items=items, item_bias=torch.zeros(7)),
               dict(personal_items=items, item_group=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError, match='^recommend_personal: '):
            m.recommend_personal(None, **kw)
    with pytest.raises(TypeError):
        m.recommend_personal(None, k=5)                                       # the list is the point of the call
    with pytest.raises(TypeError):
        m.recommend_personal(None, personal_items=items, renormalize=True)    # out of scope: no such keyword
    # good arguments reach the model
    for kw in (dict(personal_items=items), dict(personal_items=[[3], [], [4, 5]], personal_bias=[[0.5], [], [NINF, 1.0]]),
               dict(personal_items=items, k=4093), dict(personal_items=items, k=5, pool=4096, return_complete=True),
               dict(personal_items=torch.tensor([1, 2]), personal_bias=torch.tensor([0.5, -0.5]), exclude_seen=True)):
        with pytest.raises(AssertionError, match='the model ran'):
            m.recommend_personal(None, **kw)
    assert m._ROUTES['personal'] == ('personal_merge', {'checked': True})
    assert 'recommend_personal' in pkg('serving').__doc__
    D = pkg('dist')
    assert D.VocabParallel.personal is D.VocabParallel.personal_merge and hasattr(D.HipLocal, 'personal_merge')


# ------------------------------------------------------------------------------------------- the export
def test_the_export_its_prototype_and_every_bad_argument_without_a_launch():
    L = pkg('_lib')
    assert L.CONST['SREC_PERSONAL_MAXM'] == 1024 and L.CONST['SREC_CAP_MAXP'] == 4096
    proto = L.lib.protos['srec_personal_merge']
    assert [n for _, n in proto] == ['pool_ids', 'pool_s', 'B', 'P', 'items', 'base', 'bias', 'M', 'K', 'ids_out', 'val_out', 'src',
                                     'hit', 'kept', 'stream'] and len(proto) == 15
    assert all(t in L._CT for t, _ in proto)
    dll = L.lib.load()
    good = dict(pool_ids=0x1000, pool_s=0x2000, B=2, P=8, items=0x3000, base=0x4000, bias=0x5000, M=4, K=3, ids_out=0x6000,
                val_out=0x7000, src=0x8000, hit=0x9000, kept=0xa000, stream=None)
    call = lambda **kw: dll.srec_personal_merge(*[{**good, **kw}[n] for _, n in proto])
    for change in (dict(P=0), dict(P=4097), dict(M=0), dict(M=1025), dict(K=0), dict(K=4097), dict(pool_ids=None), dict(pool_s=None),
                   dict(items=None), dict(base=None), dict(ids_out=None), dict(val_out=None), dict(hit=None), dict(kept=None),
                   dict(pool_ids=0x1002), dict(pool_s=0x2001), dict(items=0x3002), dict(base=0x4003), dict(bias=0x5002),
                   dict(ids_out=0x6001), dict(val_out=0x7002), dict(src=0x8002), dict(hit=0x9001), dict(kept=0xa002)):
        assert call(**change) == 1001, change
    assert call(B=0) == 0 and call(B=-3, K=0, pool_ids=None) == 0            # no sessions: nothing to do, ahead of the checks
    with pytest.raises(TypeError):
        dll.srec_personal_merge(*[good[n] for _, n in proto][:-1])           # one short
    with pytest.raises(TypeError, match='takes exactly 15 arguments'):
        dll.srec_personal_merge(*[good[n] for _, n in proto], None)


# ------------------------------------------------------------------------------------------- the launcher
def test_launcher_takes_the_list_flags_and_refuses_the_combinations(tmp_path):
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
    finally:
        sys.path.remove(SCRIPTS)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    (tmp_path / 's.txt').write_text('1,2,3\n\n4,5\n6\n')                      # three sessions (blank lines are not counted)
    base = ['--checkpoint', 'c.pt', '--sessions', str(tmp_path / 's.txt'), '--dataset-dir', data]
    a = rec.parse(base)
    assert a.hide is None and a.session_bias is None and a.personal is None
    # an output line of recommend.py itself is a --hide line: page 2 is --hide page1.txt
    page1 = [rec.format_line([7, 3, 9], [-1.5, -2.25, -3.0]), rec.format_line([-1, -1, -1], [NINF] * 3), rec.format_line([4, -1, -1], [-0.5, NINF, NINF])]
    (tmp_path / 'page1.txt').write_text('\n'.join(page1) + '\n')
    a = rec.parse(base + ['--hide', str(tmp_path / 'page1.txt'), '--top', '3'])
    assert a.personal == dict(personal_items=[[3, 7, 9], [-1], [4]], personal_bias=None) and a.pool is None
    (tmp_path / 'one.txt').write_text('5, 6:x,-1\n')
    a = rec.parse(base + ['--hide', str(tmp_path / 'one.txt'), '--pool', '300', '--exclude-seen'])
    assert a.personal == dict(personal_items=[[5, 6]], personal_bias=None) and a.pool == 300
    (tmp_path / 'bias.txt').write_text('3:0.5,8:-2\n\n4:1e-1\t2:-inf\n')
    a = rec.parse(base + ['--session-bias', str(tmp_path / 'bias.txt')])
    assert a.personal == dict(personal_items=[[3, 8], [-1], [2, 4]], personal_bias=[[0.5, -2.0], [0.0], [NINF, 0.1]])
    a = rec.parse(base + ['--session-bias', str(tmp_path / 'bias.txt'), '--hide', str(tmp_path / 'page1.txt')])
    assert a.personal['personal_items'] == [[3, 7, 8, 9], [-1], [2, 4]]      # an id in both files is hidden
    assert a.personal['personal_bias'] == [[NINF, NINF, -2.0, NINF], [0.0], [NINF, NINF]]
    lists = pkg('ops').personal_lists('t', a.personal['personal_items'], a.personal['personal_bias'], 3, V, 'cpu')
    assert lists.M == 4 and lists.items[1].tolist() == [-1] * 4
    (tmp_path / 'far.txt').write_text('1,%d\n' % V)
    (tmp_path / 'neg.txt').write_text('1,-2\n')
    (tmp_path / 'twice.txt').write_text('1,2,1:0.5\n')
    (tmp_path / 'many.txt').write_text(','.join(str(i) for i in range(1025)) + '\n')
    (tmp_path / 'two.txt').write_text('1\n2\n')
    (tmp_path / 'words.txt').write_text('shoes\n')
    (tmp_path / 'bare.txt').write_text('1,2\n')                               # (--session-bias entries are `id:value`)
    (tmp_path / 'nan.txt').write_text('1:nan\n')
    (tmp_path / 'inf.txt').write_text('1:inf\n')
    (tmp_path / 'cats.txt').write_text('1:0\n')
    on = ['--hide', str(tmp_path / 'one.txt')]
    for bad in (['--hide', str(tmp_path / 'far.txt')], ['--hide', str(tmp_path / 'neg.txt')], ['--hide', str(tmp_path / 'twice.txt')],
                ['--hide', str(tmp_path / 'many.txt')], ['--hide', str(tmp_path / 'two.txt')], ['--hide', str(tmp_path / 'words.txt')],
                ['--hide', str(tmp_path / 'none.txt')], ['--session-bias', str(tmp_path / 'bare.txt')],
                ['--session-bias', str(tmp_path / 'nan.txt')], ['--session-bias', str(tmp_path / 'inf.txt')],
                ['--session-bias', str(tmp_path / 'two.txt')], ['--session-bias', str(tmp_path / 'far.txt')],
                on + ['--sample'], on + ['--diversity', '0.5'], on + ['--renormalize'],
                on + ['--categories', str(tmp_path / 'cats.txt'), '--max-per-category', '2'], on + ['--max-per-category', '2'],
                on + ['--categories', str(tmp_path / 'cats.txt'), '--calibrate', '0.5'], on + ['--pool', '5', '--top', '10'],
                on + ['--pool', '4097'], ['--session-bias', str(tmp_path / 'bias.txt'), '--sample']):
        with pytest.raises(SystemExit):
            rec.parse(base + bad)
    helptext = rec.parser('SRGNN').format_help()
    assert '--hide' in helptext and '--session-bias' in helptext
