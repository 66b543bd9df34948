"""CPU side of the calibrated slates: the float64 oracle (tests/calibrate_oracle.py) against a brute-force enumeration and the
objective's closed forms, the argument checks of ops.calibrate / ops.calibrate_scalars, the export and what srec_calibrate
refuses ahead of any launch (fake pointers, never followed), the launcher's flags, and model.recommend_calibrated /
list_calibration on the CPU stand-in of tests/test_serving_model_cpu.py with the oracle as the 'calibrate' launcher."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import calibrate_oracle as cal
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
NINF = float('-inf')


# ------------------------------------------------------------------------------------------- the oracle
def _brute(ids, val, category, k, weight, tcat, tw, alpha):
    """the definition, slot by slot: for every available slot the state with that slot added is built from scratch and KL summed
    over S with math.log - no classes, no sharing between slots.  One session; -> (picks, objective values, final KL)"""
    w, a = float(np.float32(weight)), float(np.float32(alpha))
    n_items = len(category)
    P = {}
    for c, x in zip(tcat, tw):
        x = float(np.float32(x))
        if c >= 0 and x > 0:
            P[c] = P.get(c, 0.0) + x
    W = sum(P[c] for c in sorted(P))
    p = {c: P[c] / W for c in sorted(P)} if W > 0 else {}

    def kl(chosen):
        cats = [category[ids[i]] for i in chosen]
        N = sum(1 for c in cats if c >= 0)
        return sum(pc * math.log(pc / ((1 - a) * sum(1 for x in cats if x == c) / max(N, 1) + a * pc)) for c, pc in p.items())
    avail = [i for i, v in enumerate(ids) if 0 <= v < n_items]
    picks, objs = [], []
    for _ in range(k):
        if not avail:
            picks.append(-1)
            objs.append(NINF)
            continue
        best, at = None, -1
        for i in avail:
            s = float(np.float32(val[i]))
            m = NINF if s == NINF else s if w == 0 else (1 - w) * s - w * kl(picks + [i])
            if best is None or m > best + 1e-12:                 # (round-off between two summation orders is no new best)
                best, at = m, i
        picks.append(at)
        objs.append(best)
        avail.remove(at)
    return picks, objs, kl([i for i in picks if i >= 0])


@pytest.mark.parametrize('seed', range(6))
def test_oracle_equals_the_brute_force_enumeration_on_tiny_pools(seed):
    g = torch.Generator().manual_seed(seed)
    B, M, T = 12, 1 + seed, 4
    n_items = 12
    category = torch.randint(-1, 4, (n_items,), generator=g)
    ids = torch.stack([torch.randperm(n_items, generator=g)[:M] for _ in range(B)])
    ids[torch.rand(B, M, generator=g) < 0.15] = -1
    ids[0] = torch.arange(M)
    val = torch.sort(-8 + 2 * torch.randn(B, M, generator=g), 1, descending=True).values
    tcat = torch.randint(-1, 5, (B, T), generator=g)              # (4: a category no item has)
    tw = torch.rand(B, T, generator=g) - 0.2                      # some weights <= 0: empty pairs
    tcat[1], tw[2] = -1, 0.0                                      # sessions without a target
    for weight in (0.0, 0.3, 0.9, 1.0):
        r = cal.greedy64(ids, val, category, M, weight, tcat, tw, 0.01)
        for b in range(B):
            if float(r['margin'][b].min()) < 1e-9:
                continue
            picks, objs, kl = _brute(ids[b].tolist(), val[b].tolist(), category.tolist(), M, weight, tcat[b].tolist(),
                                     tw[b].tolist(), 0.01)
            assert r['pick'][b].tolist() == picks, (seed, weight, b)
            for x, y in zip(r['obj'][b].tolist(), objs):
                assert x == y == NINF or abs(x - y) <= 1e-12 * max(1, abs(y)), (seed, weight, b, x, y)
            assert abs(float(r['kl'][b]) - kl) <= 1e-12 * max(1, abs(kl))
        cal.assert_greedy_consistent(r['pick'], ids, val, category, weight, tcat, tw, 0.01, obj=r['obj'].float(), kl=r['kl'].float())
        filled = ((ids >= 0) & (ids < n_items)).sum(1)
        assert torch.equal((r['pick'] >= 0).sum(1), filled)
        assert bool((r['val'][r['pick'] < 0] == NINF).all())


def test_closed_forms_no_target_weight_zero_and_a_single_category():
    a = float(np.float32(0.01))
    category = torch.tensor([0, 0, 1, 1, -1, 2])
    ids = torch.tensor([[0, 2, 4, 1, 3, 5]])
    val = torch.tensor([[-1.0, -2.0, -3.0, -4.0, -5.0, -6.0]])
    # no target (None, T == 0, every pair empty): KL 0, the objective is (1 - w) val, the order the pool's
    for tcat, tw in ((None, None), (torch.zeros(1, 0, dtype=torch.long), torch.zeros(1, 0)),
                     (torch.tensor([[-1, 1]]), torch.tensor([[1.0, 0.0]]))):
        r = cal.greedy64(ids, val, category, 6, 0.25, tcat, tw)
        assert r['pick'].tolist() == [[0, 1, 2, 3, 4, 5]] and float(r['kl'][0]) == 0.0
        assert torch.equal(r['obj'][0], (1.0 - 0.25) * val[0].double())
    # w = 0: the objective is val exactly, whatever the target; kl is still that of the picks
    r = cal.greedy64(ids, val, category, 3, 0.0, torch.tensor([[1]]), torch.tensor([[2.0]]))
    assert r['pick'].tolist() == [[0, 1, 2]] and torch.equal(r['obj'][0], val[0, :3].double())
    # slots 0, 1, 2 hold categories 0, 1, none: N = 2, n_1 = 1
    assert float(r['kl'][0]) == pytest.approx(math.log(1.0 / ((1 - a) * 0.5 + a)), abs=1e-15)
    # a single category, w = 1: p = 1, KL = -log((1 - a) n / N + a).  Slot 1 (category 1: KL 0) first; then slot 4 (category 1)
    # and slot 2 (uncategorised: the state is unchanged) tie at KL 0 and the lower slot goes first; the rest are outside S:
    # KL rises the same for each, slot order
    r = cal.greedy64(ids, val, category, 6, 1.0, torch.tensor([[1, 1]]), torch.tensor([[0.5, 1.5]]))
    assert r['pick'].tolist() == [[1, 2, 4, 0, 3, 5]]
    want = [0.0, 0.0, 0.0] + [math.log(1.0 / ((1 - a) * 2 / N + a)) for N in (3, 4, 5)]
    assert np.allclose(r['obj'][0].numpy(), -np.array(want), rtol=0, atol=1e-15)
    assert float(r['kl'][0]) == pytest.approx(want[-1], abs=1e-15)
    mg = r['margin'][0].tolist()                                  # (exact ties are the rule at w = 1)
    assert mg[0] == mg[1] == mg[3] == 0.0 and mg[2] > 0.5 and mg[5] == float('inf')
    # -inf values at w = 1: never NaN, picked last in slot order
    v = torch.tensor([[NINF, -2.0, NINF, -4.0, -5.0, -6.0]])
    r = cal.greedy64(ids, v, category, 6, 1.0, torch.tensor([[1]]), torch.tensor([[1.0]]))
    assert r['pick'][0, -2:].tolist() == [0, 2] and not bool(torch.isnan(r['obj']).any()) and r['obj'][0, -2:].tolist() == [NINF] * 2


# ------------------------------------------------------------------------------------------- argument checks
def test_calibrate_scalars_and_ops_calibrate_refuse_bad_arguments_before_any_launch():
    ops = pkg('ops')
    k, w, a = ops.calibrate_scalars('t', 5, 0.7, 0.01, 8)
    assert (k, w, a) == (5, float(np.float32(0.7)), float(np.float32(0.01))) and ops.calibrate_scalars('t', 128, 0, 0.5)[0] == 128
    for bad in ((0, 0.5, 0.01, None), (129, 0.5, 0.01, None), (5, 0.5, 0.01, 4), (1, 0.5, 0.01, 0), (1, 0.5, 0.01, 129),
                (5, -0.1, 0.01, None), (5, 1.1, 0.01, None), (5, float('nan'), 0.01, None), (5, 'x', 0.01, None),
                (5, 0.5, 0.0, None), (5, 0.5, 1.0, None), (5, 0.5, float('nan'), None), (5, 0.5, 1e-60, None), (5, 0.5, None, None)):
        with pytest.raises(ValueError):
            ops.calibrate_scalars('t', *bad)
    category = (torch.arange(50) % 5).to(torch.int32)
    ids, val = torch.zeros(3, 10, dtype=torch.int64), torch.zeros(3, 10)
    tc, tw = torch.zeros(3, 4, dtype=torch.int64), torch.ones(3, 4)
    bad = [
        dict(k=0), dict(k=11), dict(weight=2.0), dict(alpha=0.0), dict(ids=torch.zeros(3, 10)),
        dict(ids=torch.zeros(30, dtype=torch.int64)), dict(ids=torch.zeros(3, 10, dtype=torch.bool)), dict(val=torch.zeros(3, 9)),
        dict(val=torch.zeros(3, 10).double()), dict(ids=torch.full((3, 10), 50)),        # an id past category (checked=False)
        dict(ids=torch.zeros(3, 129, dtype=torch.int64), val=torch.zeros(3, 129), k=5),
        dict(category=category.long()), dict(category=category[None]), dict(category=category.tolist()),
        dict(target_cat=None), dict(target_w=None), dict(target_cat=tc.float()), dict(target_w=tw.long()),
        dict(target_cat=tc[:2], target_w=tw[:2]), dict(target_w=tw[:, :3]), dict(target_cat=tc[0], target_w=tw[0]),
        dict(target_cat=torch.zeros(3, 129, dtype=torch.int64), target_w=torch.ones(3, 129)),
        dict(target_w=tw * float('nan')), dict(target_w=tw * float('inf')), dict(target_w=-tw),
        dict(ids=ids.to('meta')), dict(val=val.to('meta')), dict(target_cat=tc.to('meta')),      # refused, not moved
    ]
    for kw in bad:
        a = dict(ids=ids, val=val, category=category, k=5, weight=0.5, target_cat=tc, target_w=tw, alpha=0.01)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.calibrate(**a)
    # good arguments on CPU tensors get as far as the launch, which has no fallback
    for kw in (dict(target_cat=tc, target_w=tw), dict(), dict(target_cat=tc, target_w=tw, checked=True)):
        with pytest.raises(RuntimeError, match='GPU|libsrec'):
            ops.calibrate(ids, val, category, 5, 0.5, **kw)
    assert ops.calibrate(ids[:0], val[:0], category, 5, 0.5)[1].shape == (0, 5)            # no sessions: no launch


def test_the_export_its_prototype_and_every_bad_argument_without_a_launch():
    L = pkg('_lib')
    assert L.CONST['SREC_CALIB_MAXT'] == 128 and L.CONST['SREC_SELECT_MAXK'] == 128
    proto = L.lib.protos['srec_calibrate']
    assert [n for _, n in proto] == ['ids', 's', 'B', 'M', 'K', 'category', 'n_items', 'tcat', 'tw', 'T', 'weight', 'smooth', 'pick',
                                     'val', 'obj', 'kl', 'stream'] and len(proto) == 17
    assert all(t in L._CT for t, _ in proto) and [t for t, _ in proto].count('float') == 2
    dll = L.lib.load()
    good = dict(ids=0x1000, s=0x2000, B=2, M=8, K=3, category=0x3000, n_items=10, tcat=0x4000, tw=0x5000, T=4, weight=0.5,
                smooth=0.01, pick=0x6000, val=0x7000, obj=0x8000, kl=0x9000, stream=None)
    call = lambda **kw: dll.srec_calibrate(*[{**good, **kw}[n] for _, n in proto])
    nan = float('nan')
    for change in (dict(K=0), dict(K=9), dict(M=0), dict(M=129, K=129), dict(M=129), dict(T=-1), dict(T=129), dict(n_items=-1),
                   dict(weight=-0.1), dict(weight=1.5), dict(weight=nan), dict(smooth=0.0), dict(smooth=1.0), dict(smooth=-0.5),
                   dict(smooth=nan), dict(ids=None), dict(s=None), dict(category=None), dict(pick=None), dict(val=None),
                   dict(tcat=None), dict(tw=None), dict(ids=0x1002), dict(s=0x2001), dict(category=0x3002), dict(tcat=0x4002),
                   dict(tw=0x5001), dict(pick=0x6002), dict(val=0x7003), dict(obj=0x8002), dict(kl=0x9001),
                   dict(T=0, tcat=0x4002), dict(T=0, tw=0x5002)):
        assert call(**change) == 1001, change
    assert call(B=0) == 0 and call(B=-3, K=0, ids=None) == 0                 # no sessions: nothing to do, ahead of the checks
    with pytest.raises(TypeError):
        dll.srec_calibrate(*[good[n] for _, n in proto][:-1])                # one short
    with pytest.raises(TypeError, match='takes exactly 17 arguments'):
        dll.srec_calibrate(*[good[n] for _, n in proto], None)


# ------------------------------------------------------------------------------------------- the launcher
def test_launcher_takes_the_calibrate_flags_and_refuses_the_combinations(tmp_path, capsys):
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
    finally:
        sys.path.remove(SCRIPTS)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    cats = tmp_path / 'cats.txt'
    cats.write_text(''.join('%d:%d\n' % (i, (i % 5) * 100000) for i in range(0, V, 2)) + '\n')
    capsf = tmp_path / 'caps.txt'
    capsf.write_text('1:0\n')
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--dataset-dir', data]
    a = rec.parse(base)
    assert a.calibrate is None and a.calibration is None and a.caps is None
    on = ['--calibrate', '0.7', '--categories', str(cats)]
    a = rec.parse(base + on + ['--top', '10', '--exclude-seen'])                   # --categories alone is legal here
    assert a.caps is None and a.pool is None and a.calibration['weight'] == 0.7 and a.calibration['alpha'] == 0.01
    assert a.calibration['item_category'] == [(i % 5) * 100000 if i % 2 == 0 else -1 for i in range(V)]
    a = rec.parse(base + on + ['--calibrate-smooth', '0.2', '--pool', '128', '--top', '128'])
    assert a.calibration['alpha'] == 0.2 and a.pool == 128
    assert rec.parse(base + ['--calibrate', '0', '--categories', str(cats)]).calibration['weight'] == 0.0
    (tmp_path / 'bad_item.txt').write_text('0:1\n%d:1\n' % V)
    (tmp_path / 'twice.txt').write_text('3:1\n3:2\n')
    (tmp_path / 'bad_cat.txt').write_text('3:-1\n')
    (tmp_path / 'big_cat.txt').write_text('3:%d\n' % 2 ** 31)
    errors = [
        ('give --categories', ['--calibrate', '0.5']),
        ('--calibrate-smooth smooths', ['--calibrate-smooth', '0.1', '--categories', str(cats), '--max-per-category', '2']),
        ('--sample draws', on + ['--sample']),
        ('two re-ranks', on + ['--diversity', '0.5']),
        ('soft counterpart', on + ['--max-per-category', '2']),
        ('soft counterpart of', on + ['--category-caps', str(capsf)]),
        ('--calibrate must be in', ['--calibrate', '1.5', '--categories', str(cats)]),
        ('--calibrate must be in ', ['--calibrate', '-0.1', '--categories', str(cats)]),
        ('--calibrate must be in [', ['--calibrate', 'nan', '--categories', str(cats)]),
        ('--calibrate-smooth must be in', on + ['--calibrate-smooth', '0']),
        ('--calibrate-smooth must be in ', on + ['--calibrate-smooth', '1']),
        ('--pool must be between --top and 128', on + ['--pool', '129']),
        ('--pool must be between --top and 128', on + ['--pool', '5', '--top', '10']),
        ('No such file', ['--calibrate', '0.5', '--categories', str(tmp_path / 'none.txt')]),
        ('ids are in', ['--calibrate', '0.5', '--categories', str(tmp_path / 'bad_item.txt')]),
        ('named twice', ['--calibrate', '0.5', '--categories', str(tmp_path / 'twice.txt')]),
        ('categories are in [0, 2^31)', ['--calibrate', '0.5', '--categories', str(tmp_path / 'bad_cat.txt')]),
        ('categories are in [0, 2^31)', ['--calibrate', '0.5', '--categories', str(tmp_path / 'big_cat.txt')]),
        # without --calibrate every message stays
        ('--categories goes with --max-per-category N or --category-caps FILE', ['--categories', str(cats)]),
        ('--pool goes with --diversity or --categories', ['--pool', '40']),
        ('--categories caps the most probable items in served order: not together with --sample or --diversity',
            ['--categories', str(cats), '--max-per-category', '2', '--sample']),
        ('--max-per-category / --category-caps cap the categories of --categories: give the file', ['--max-per-category', '2']),
        ('--pool must be between --top and 4096', ['--categories', str(cats), '--max-per-category', '2', '--pool', '4097']),
        ('--diversity re-ranks the most probable items and --sample draws them: give one of the two', ['--diversity', '0.5', '--sample']),
    ]
    for text, bad in errors:
        with pytest.raises(SystemExit):
            rec.parse(base + bad)
        assert text in capsys.readouterr().err, bad
    helptext = rec.parser('SRGNN').format_help()
    assert '--calibrate W' in helptext and '--calibrate-smooth A' in helptext


# ------------------------------------------------------------------------------------------- the model API on the CPU stand-in
def _cal_local(base):
    class CalLocal(base):
        """+ the calibrate entry of dist.HipLocal, from the oracle"""

        def calibrate(self, ids, val, category, k, weight, tcat, tw, alpha):
            r = cal.greedy64(ids, val, category, k, weight, tcat, tw, alpha)
            return r['val'], r['pick'].to(torch.int32), r['obj'].float(), r['kl'].float()
    return CalLocal


@pytest.fixture(scope='module', params=['softmax', 'mixture'])
def served(request):
    import test_serving_model_cpu as sm
    TableOnly, Mixture = sm._models()
    model = (TableOnly if request.param == 'softmax' else Mixture)().train()
    pkg('dist').VocabParallel(model, local=_cal_local(sm.AllLocal)(sm.V))
    return model, (sm.CASE['srs'][0] if request.param == 'softmax' else sm.CASE['srs']), sm


def test_recommend_calibrated_and_list_calibration_on_the_stand_in(served):
    model, x, sm = served
    V, B, K = sm.V, sm.B, sm.K
    category = (torch.arange(V) * 7919 % 6 - 1).to(torch.int32)               # -1 .. 4
    listed = sm.CASE['listed']
    tcat = torch.where(listed < 0, torch.full_like(listed, -1), category[listed.clamp(min=0)].long())
    kw = dict(exclude_seen=True, item_bias=sm.CASE['bias'], item_group=sm.CASE['group'])
    changed = 0
    for pool, weight, extra in ((12, 0.9, {}), (20, 0.5, kw), (K, 1.0, dict(renormalize=True, **kw))):
        pv, pi = model.recommend(x, k=pool, **extra)
        r = cal.greedy64(pi, pv, category, K, weight, tcat, torch.ones(tcat.shape), 0.01)
        want = cal.lists(pv, pi, r)
        val, ids, kl = model.recommend_calibrated(x, k=K, weight=weight, item_category=category, pool=pool, return_kl=True, **extra)
        assert val.dtype == torch.float32 and ids.dtype == torch.int32 and kl.dtype == torch.float32 and kl.shape == (B,)
        assert torch.equal(ids, want[1]) and torch.equal(val.view(torch.int32), want[0].view(torch.int32)), pool
        assert torch.equal(kl, r['kl'].float())
        changed += int((ids != pi[:, :K]).any(1).sum())
        assert torch.equal(model.list_calibration(x, item_ids=ids, item_category=category), kl)
        # weight 0: the first k columns of the pool
        val0, ids0 = model.recommend_calibrated(x, k=K, weight=0, item_category=category.tolist(), pool=pool, **extra)
        assert torch.equal(ids0, pi[:, :K]) and torch.equal(val0.view(torch.int32), pv[:, :K].view(torch.int32))
    assert changed > 0, 'calibration moved nothing: the comparison shows nothing'
    assert bool((ids[6, 4:] == -1).all()) and bool((val[6, 4:] == NINF).all())            # group 1 keeps four items
    assert model.training                                                                 # (_Serving put the flag back)
    # an explicit target; the default pool is min(128, max(4 k, k)) = 20
    tc = torch.tensor([[0, 3, 0, -1]] * B)
    tw = torch.tensor([[1.0, 2.0, 0.5, 9.0]] * B)
    pv, pi = model.recommend(x, k=20)
    r = cal.greedy64(pi, pv, category, K, 0.8, tc, tw, 0.05)
    val, ids = model.recommend_calibrated(x, k=K, weight=0.8, item_category=category.long(), target=(tc, tw), alpha=0.05)
    assert torch.equal(ids, cal.lists(pv, pi, r)[1])
    got = model.list_calibration(item_ids=pi[:, :7], item_category=category, target=(tc.tolist(), tw.tolist()), alpha=0.05)
    want = cal.greedy64(pi[:, :7], torch.zeros(B, 7), category, 7, 0.0, tc, tw, 0.05)['kl'].float()
    assert torch.equal(got, want) and float(got.min()) > 0
    # no pair at all: no target, KL 0, the plain order
    val, ids, kl = model.recommend_calibrated(x, k=K, weight=0.9, item_category=category, target=(tc[:, :0], tw[:, :0]), return_kl=True)
    assert torch.equal(ids, pi[:, :K]) and kl.tolist() == [0.0] * B


def test_recommend_calibrated_checks_its_arguments_before_the_model_runs():
    from test_cap_cpu import _cpu_model
    m = _cpu_model()
    m._session_items = lambda mg: torch.zeros(2, 3, dtype=torch.int32)
    cat = torch.arange(30) % 4
    tc, tw = torch.zeros(2, 3, dtype=torch.int64), torch.ones(2, 3)
    for kw in (dict(k=0), dict(k=129), dict(k=10, pool=9), dict(k=10, pool=129), dict(weight=1.5), dict(weight=-1), dict(alpha=0),
               dict(alpha=1), dict(item_category=None), dict(item_category=cat[:29]), dict(item_category=cat.float()),
               dict(item_category=cat[None]), dict(item_category=cat + 2 ** 31), dict(target=(tc, tw[:, :2])), dict(target=(tc.float(), tw)),
               dict(target=(tc, tw.long())), dict(target=tc), dict(target=(tc[0], tw[0])), dict(target=(tc, -tw)),
               dict(target=(tc, tw * float('nan'))), dict(target=(torch.zeros(2, 129, dtype=torch.int64), torch.ones(2, 129))),
               dict(item_bias=torch.zeros(7)), dict(item_group=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            m.recommend_calibrated(None, **{**dict(item_category=cat), **kw})
    with pytest.raises(ValueError, match='at most 128'):
        m.recommend_calibrated(None, item_category=cat, target=(torch.zeros(2, 129, dtype=torch.int64), torch.ones(2, 129)))
    m._session_items = lambda mg: torch.zeros(2, 129, dtype=torch.int32)
    with pytest.raises(ValueError, match='at most 128'):                                 # a session of 129 distinct items
        m.recommend_calibrated(None, item_category=cat)
    m._session_items = lambda mg: torch.zeros(2, 3, dtype=torch.int32)
    for kw in (dict(), dict(k=128), dict(k=5, pool=128, target=(tc, tw)), dict(weight=0, item_category=cat.to(torch.int32))):
        with pytest.raises(AssertionError, match='the model ran'):
            m.recommend_calibrated(None, **{**dict(item_category=cat), **kw})
    for kw in (dict(item_ids=torch.zeros(2, 129, dtype=torch.int64)), dict(item_ids=torch.zeros(2, 4)), dict(item_ids=torch.zeros(8, dtype=torch.int64)),
               dict(item_ids=torch.full((2, 4), 30)), dict(item_ids=torch.full((2, 4), -2)), dict(alpha=2.0), dict(item_category=cat[:5])):
        with pytest.raises(ValueError):
            m.list_calibration(None, **{**dict(item_ids=torch.zeros(2, 4, dtype=torch.int64), item_category=cat), **kw})
    assert m._ROUTES['calibrate'] == ('calibrate', {'checked': True})
    doc = pkg('serving').__doc__
    assert 'recommend_calibrated' in doc and 'list_calibration' in doc
    assert 'multiplicity' in m.recommend_calibrated.__doc__ or 'how often' in m.recommend_calibrated.__doc__


# ------------------------------------------------------------------------------------------- the sharded route over gloo
def _route_worker(rank, world, port, q):
    import torch.distributed as dist
    from test_dist_cpu import FakeModel, TorchLocal
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        D = pkg('dist')
        ids, val, category, tcat, tw = cal.random_case(8, 40, 6, 9, seed=3, n_items=150)
        model = FakeModel(torch.randn(150, 16, generator=torch.Generator().manual_seed(1)))
        vp = D.VocabParallel(model, local=_cal_local(TorchLocal)())
        n = ids.shape[0] // world
        sl = slice(rank * n, (rank + 1) * n)
        before = D.STATS['count']
        with torch.no_grad():
            rep = vp.calibrate(ids, val, category, 9, 0.7, tcat, tw, 0.01)
            dp = vp.calibrate(ids[sl], val[sl], category, 9, 0.7, tcat[sl], tw[sl], 0.01, data_parallel=True)
        q.put((rank, D.STATS['count'] - before, [t.tolist() for t in rep], [t.tolist() for t in dp]))
    finally:
        dist.destroy_process_group()


def test_sharded_calibrate_two_ranks_equal_unsharded_without_a_collective():
    import torch.multiprocessing as mp
    from test_dist_cpu import TorchLocal, _free_port
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_route_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=120) for _ in range(world)]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    ids, val, category, tcat, tw = cal.random_case(8, 40, 6, 9, seed=3, n_items=150)
    ref = [t.tolist() for t in _cal_local(TorchLocal)().calibrate(ids, val, category, 9, 0.7, tcat, tw, 0.01)]
    assert ref[1] != [list(range(9))] * 8
    n = ids.shape[0] // world
    for rank, sent, rep, dp in res:
        assert sent == 0, 'the calibrated re-rank needs no collective'
        assert rep == ref, rank
        assert dp == [x[rank * n:(rank + 1) * n] for x in ref], rank
