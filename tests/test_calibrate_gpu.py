"""Calibrated slates on the GPU: csrc/calibrate.hip through ops.calibrate, dist.VocabParallel.calibrate,
model.recommend_calibrated / list_calibration and src/scripts/recommend.py, against the float64 greedy of
tests/calibrate_oracle.py.

The kernel forms its objective in double, so its picks are compared with `==` on every session whose two best candidates are
at least 1e-9 apart in the oracle at every step (calibrate_oracle.TOL, derived there), and at most 1 % of the sessions may
fall below that; where exact ties are the rule (weight 1) the kernel's own prefix is replayed instead
(assert_greedy_consistent).  obj and kl are fp32 roundings of double values: compared at 2^-23 max(1, |value|); val with
torch.equal."""
import os
import subprocess
import sys

import pytest
import torch

import calibrate_oracle as cal
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')
WORST = {'obj': 0.0, 'kl': 0.0}              # the largest |obj - f64| and |kl - f64| seen, printed by every check


def _ops():
    return pkg('ops')


def _run(ops, dev, ids, val, category, k, w, tcat=None, tw=None, alpha=0.01, **kw):
    on = lambda t: None if t is None else t.to(dev)
    return [t.cpu() for t in ops.calibrate(on(ids), on(val), on(category), k, w, on(tcat), on(tw), alpha, **kw)]


def _check(out, ids, val, category, k, w, tcat=None, tw=None, alpha=0.01, what='', equal=True):
    """shapes and dtypes; val = val[pick] bit for bit; the kernel's picks are A greedy solution of its own prefix, with obj
    and kl within fp32 rounding of the float64 values; equal: picks == the oracle's where its margins allow, and at most 1 % of
    the sessions may not allow it.  -> (picks, oracle result)"""
    got_val, pick, obj, kl = out
    B = ids.shape[0]
    assert got_val.dtype == obj.dtype == kl.dtype == torch.float32 and pick.dtype == torch.int32, what
    assert pick.shape == got_val.shape == obj.shape == (B, k) and kl.shape == (B,), what
    assert not bool(torch.isnan(obj).any()) and not bool(torch.isnan(kl).any()), what
    want = torch.where(pick < 0, torch.full_like(got_val, NINF), val.gather(1, pick.clamp(min=0).long()))
    assert torch.equal(got_val.view(torch.int32), want.view(torch.int32)), '%s: val is not val[pick] bit for bit' % what
    assert bool((obj[pick < 0] == NINF).all()), what
    ties, e_obj, e_kl = cal.assert_greedy_consistent(pick, ids, val, category, w, tcat, tw, alpha, obj=obj, kl=kl)
    WORST['obj'], WORST['kl'] = max(WORST['obj'], e_obj), max(WORST['kl'], e_kl)
    print('%s: %d tied steps, max |obj - f64| %.3e, max |kl - f64| %.3e (so far %.3e, %.3e)'
          % (what, ties, e_obj, e_kl, WORST['obj'], WORST['kl']))
    r = cal.greedy64(ids, val, category, k, w, tcat, tw, alpha)
    if equal:
        clear = r['margin'].min(1).values >= cal.TOL
        assert int((~clear).sum()) <= B // 100, '%s: %d of %d sessions have a margin below %g' % (what, int((~clear).sum()), B, cal.TOL)
        bad = (pick.long() != r['pick']).any(1) & clear
        assert not bool(bad.any()), '%s: sessions %s differ, e.g. picks %s, expected %s' % (
            what, bad.nonzero().flatten().tolist()[:8], pick[bad][0].tolist()[:16], r['pick'][bad][0].tolist()[:16])
    return pick, r


# ------------------------------------------------------------------------------------------- 1) random pools
@pytest.mark.parametrize('B,M,T,G,K,w', [(64, 128, 12, 40, 20, 0.5), (64, 128, 128, 300, 128, 0.9), (64, 37, 1, 5, 37, 0.3)])
def test_random_pools_picks_equal_the_oracle(dev, B, M, T, G, K, w):
    ops = _ops()
    ids, val, category, tcat, tw = cal.random_case(B, M, T, G, seed=2)
    for dtype in (torch.int64, torch.int32):
        out = _run(ops, dev, ids.to(dtype), val, category, K, w, tcat.to(dtype), tw)
        pick, _ = _check(out, ids, val, category, K, w, tcat, tw, what='random %s %s' % ((B, M, T, G, K, w), dtype))
    plain = _run(ops, dev, ids, val, category, K, 0.0, tcat, tw)
    assert plain[1].tolist() == [list(range(K))] * B and torch.equal(plain[0], val[:, :K]) and torch.equal(plain[2], val[:, :K])
    changed = int((pick != plain[1]).any(1).sum())
    print('calibration changed the picks of %d of %d sessions' % (changed, B))
    assert changed > B // 2, 'calibration moves too little: the comparison does not bite'
    if K == M:                                                                   # the same set of picks: the same counts
        assert torch.equal(out[3], plain[3])
    else:
        assert float(out[3].mean()) < float(plain[3].mean())


# ------------------------------------------------------------------------------------------- 2) weight 1: ties
def test_weight_one_ties_are_broken_towards_the_lower_slot(dev):
    ops = _ops()
    B, M, T, G = 33, 128, 64, 16384
    ids, val, category, tcat, tw = cal.random_case(B, M, T, G, seed=1, n_items=4000, target_cats=G)
    g = torch.Generator().manual_seed(5)
    some = torch.stack([torch.randperm(M, generator=g)[:T // 2] for _ in range(B)])
    tcat[:, :T // 2] = category[ids.gather(1, some)].long()                      # half of the pairs name categories of the pool
    for k in (M, 20):
        out = _run(ops, dev, ids, val, category, k, 1.0, tcat, tw)
        _, r = _check(out, ids, val, category, k, 1.0, tcat, tw, what='weight 1, k %d' % k, equal=False)
        assert k < M or int((r['margin'] == 0).sum()) > 100, 'exact ties are the rule at weight 1'
    # structural ties, by hand: items 0 .. 7 with categories 3, 3, 900, 901, none, none, 3, 5; the target names 3 and 5
    category = torch.tensor([3, 3, 900, 901, -1, -1, 3, 5], dtype=torch.int32)
    tcat, tw = torch.tensor([[3, 5]]), torch.tensor([[3.0, 1.0]])
    cases = [([0, 1], [-2.0, -2.0], 0.6),                  # the same category and the same s
             ([1, 0, 6], [-2.0, -2.0, -2.0], 1.0),
             ([2, 3], [-2.0, -2.0], 0.6),                  # two different categories outside S and the same s
             ([3, 2], [-1.0, -1.0], 1.0),
             ([4, 5], [-2.0, -2.0], 0.6),                  # two uncategorised slots
             ([5, 4], [-3.0, -3.0], 1.0),
             ([7, 0, 1, 2], [-1.0, -1.0, -1.0, -1.0], 0.0),   # w = 0 and equal s: slot order whatever the categories
             ([2, 7, 3, 0, 5, 1], [-1.0, -5.0, -1.0, -5.0, -1.0, -5.0], 1.0)]   # s is irrelevant at w = 1
    for items, s, w in cases:
        ids1, val1 = torch.tensor([items]), torch.tensor([s])
        out = _run(ops, dev, ids1, val1, category, len(items), w, tcat, tw)
        pick, r = _check(out, ids1, val1, category, len(items), w, tcat, tw, what='tie %s w %g' % (items, w), equal=False)
        assert pick.tolist() == r['pick'].tolist(), (items, w, pick.tolist(), r['pick'].tolist())
        if len(items) < 6:
            assert pick[0, :2].tolist() == [0, 1] and float(r['margin'][0, 0]) == 0.0, (items, w)
    # p = (3/4, 1/4): category 3 first (slot 3), then the pair of slots that brings in 5 and 3 ...
    assert pick.tolist()[0][0] == 3


# ------------------------------------------------------------------------------------------- 3) edges
def test_edges(dev):
    ops = _ops()
    ids, val, category, tcat, tw = cal.random_case(8, 40, 6, 9, seed=3, n_items=150)
    n = category.numel()
    # M = 1, K = M
    _check(_run(ops, dev, ids[:, :1], val[:, :1], category, 1, 0.7, tcat, tw), ids[:, :1], val[:, :1], category, 1, 0.7, tcat, tw, what='M 1')
    _check(_run(ops, dev, ids, val, category, 40, 0.7, tcat, tw), ids, val, category, 40, 0.7, tcat, tw, what='K = M')
    # T = 0 with NULL target pointers, and a [B, 0] target: no target, the plain order, KL 0
    for target in ((None, None), (tcat[:, :0], tw[:, :0])):
        out = _run(ops, dev, ids, val, category, 10, 0.7, *target)
        _check(out, ids, val, category, 10, 0.7, *target, what='T 0')
        assert out[1].tolist() == [list(range(10))] * 8 and out[3].tolist() == [0.0] * 8
    # a session whose pairs are all empty beside sessions with targets
    tc2, tw2 = tcat.clone(), tw.clone()
    tc2[2], tw2[5] = -1, 0.0
    out = _run(ops, dev, ids, val, category, 10, 0.7, tc2, tw2)
    pick, _ = _check(out, ids, val, category, 10, 0.7, tc2, tw2, what='empty targets')
    assert pick[2].tolist() == pick[5].tolist() == list(range(10)) and out[3][2] == out[3][5] == 0
    assert any(pick[b].tolist() != list(range(10)) for b in (0, 1, 3, 4, 6, 7))
    # unfilled slots in the middle and at the end: -1, and garbage under checked=True; K above the filled count
    holes = ids.clone()
    holes[:, 3], holes[:, 17], holes[:, 30:] = -1, -1, -1
    out = _run(ops, dev, holes, val, category, 40, 0.7, tcat, tw)
    pick, _ = _check(out, holes, val, category, 40, 0.7, tcat, tw, what='holes')
    assert bool((pick[:, :28] >= 0).all()) and bool((pick[:, 28:] == -1).all()) and bool((out[0][:, 28:] == NINF).all())
    assert not bool(((pick == 3) | (pick == 17) | (pick >= 30)).any())
    junk = holes.clone()
    junk[:, 3], junk[:, 17], junk[:, 30:35], junk[:, 35:] = n, 2 ** 31 - 1, -2 ** 31, -7
    with pytest.raises(ValueError):
        ops.calibrate(junk.to(dev), val.to(dev), category.to(dev), 40, 0.7, tcat.to(dev), tw.to(dev))
    for dtype in (torch.int64, torch.int32):
        again = _run(ops, dev, junk.to(dtype), val, category, 40, 0.7, tcat, tw, checked=True)
        for x, y in zip(out, again):
            assert torch.equal(x, y), dtype
    # -inf values at weight 1: no NaN anywhere, and they are picked last, in slot order
    v = val.clone()
    v[:, [0, 5, 9]] = NINF
    for w in (1.0, 0.5):
        out = _run(ops, dev, ids, v, category, 40, w, tcat, tw)
        pick, _ = _check(out, ids, v, category, 40, w, tcat, tw, what='-inf values, w %g' % w, equal=False)
        assert pick[:, -3:].tolist() == [[0, 5, 9]] * 8 and bool((out[2][:, -3:] == NINF).all()) and bool(torch.isfinite(out[2][:, :-3]).all())
    # duplicate target pairs add up: (c, 1), (c, 2) is (c, 3)
    dup_c, dup_w = torch.tensor([[4, 1, 4, 2]] * 8), torch.tensor([[1.0, 2.0, 2.0, 0.5]] * 8)
    one_c, one_w = torch.tensor([[4, 1, 2]] * 8), torch.tensor([[3.0, 2.0, 0.5]] * 8)
    a, b = _run(ops, dev, ids, val, category, 12, 0.8, dup_c, dup_w), _run(ops, dev, ids, val, category, 12, 0.8, one_c, one_w)
    _check(a, ids, val, category, 12, 0.8, dup_c, dup_w, what='duplicates')
    assert torch.equal(a[1], b[1]) and torch.allclose(a[3], b[3], rtol=0, atol=1e-6)
    # ids as int64 beyond int32: an unfilled slot, not the item it would wrap to; a category id beyond int32: an empty pair
    far = ids.clone()
    far[:, 0] = 2 ** 32 + far[:, 1]
    _check(_run(ops, dev, far, val, category, 12, 0.8, tcat, tw, checked=True), far, val, category, 12, 0.8, tcat, tw, what='beyond int32')
    far_c = tcat.clone()
    far_c[:, 0] = 2 ** 32 + 3
    gone = tcat.clone()
    gone[:, 0] = -1
    for x, y in zip(_run(ops, dev, ids, val, category, 12, 0.8, far_c, tw), _run(ops, dev, ids, val, category, 12, 0.8, gone, tw)):
        assert torch.equal(x, y)
    # large category ids are only compared
    big = (category.long() * 7919 * 271 % (2 ** 31 - 1)).to(torch.int32)
    big[category < 0] = -1
    big_t = torch.where(tcat < 0, tcat, tcat * 7919 * 271 % (2 ** 31 - 1))
    assert int(big.max()) > 10 ** 6
    out = _run(ops, dev, ids, val, big, 12, 0.8, big_t, tw)
    for x, y in zip(out, _run(ops, dev, ids, val, category, 12, 0.8, tcat, tw)):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------- 4) bits
def test_views_and_batch_independence_bit_for_bit(dev):
    ops = _ops()
    B, M, T, K = 64, 128, 12, 20
    ids, val, category, tcat, tw = cal.random_case(B, M, T, 40, seed=4)
    category = category.to(dev)
    base = ops.calibrate(ids.to(dev), val.to(dev), category, K, 0.5, tcat.to(dev), tw.to(dev))
    alone = ops.calibrate(ids[40:41].to(dev), val[40:41].to(dev), category, K, 0.5, tcat[40:41].to(dev), tw[40:41].to(dev))
    for x, y in zip(base, alone):                                # position 40 of B = 64 is position 0 of B = 1
        assert torch.equal(x[40:41], y)
    wide_i = torch.full((B, M + 40), 7, dtype=torch.int64, device=dev)
    wide_v = torch.full((B, M + 40), 7.0, device=dev)
    wide_i[:, 8:M + 8], wide_v[:, 8:M + 8] = ids.to(dev), val.to(dev)
    vi, vv = wide_i[:, 8:M + 8], wide_v[:, 8:M + 8]
    wide_c = torch.zeros(B, 2 * T, dtype=torch.int64, device=dev)
    wide_w = torch.zeros(B, 2 * T, device=dev)
    wide_c[:, ::2], wide_w[:, ::2] = tcat.to(dev), tw.to(dev)
    assert not vi.is_contiguous() and not wide_c[:, ::2].is_contiguous()
    for x, y in zip(base, ops.calibrate(vi, vv, category, K, 0.5, wide_c[:, ::2], wide_w[:, ::2])):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------- 5) models
_MODELS = {}


def _model(name, dev):
    if name not in _MODELS:
        from test_rank_gpu import _fixture_model
        _MODELS[name] = _fixture_model(name, dev)
    return _MODELS[name]


def _same(got, want, what):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32, what
    assert torch.equal(got[1].cpu(), want[1]), '%s: ids' % what
    assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32)), '%s: values are not the pool\'s bits' % what


@pytest.mark.parametrize('name', ['srgnn_s32', 'niser_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_recommend_calibrated_against_its_own_pool(dev, name):
    from util import load_golden
    z, model, inputs, labels = _model(name, dev)
    B, V = labels.numel(), model._num_items()
    category = (torch.arange(V) * 7919 % 13 - 1).to(torch.int32)               # -1 .. 11
    listed = model._session_items(inputs[0]).cpu().long()
    tcat = torch.where(listed < 0, torch.full_like(listed, -1), category[listed.clamp(min=0)].long())
    tw = torch.ones(tcat.shape)
    K, POOL, W = 20, 80, 0.6
    moved = 0
    bias = torch.zeros(V, device=dev)
    bias[::3] = NINF
    bias[1::3] = 0.5
    for kw in (dict(), dict(exclude_seen=True, item_bias=bias), dict(exclude_seen=True, item_bias=bias, renormalize=True)):
        pv, pi = [t.cpu() for t in model.recommend(*inputs, k=POOL, **kw)]
        r = cal.greedy64(pi, pv, category, K, W, tcat, tw)
        clear = r['margin'].min(1).values >= cal.TOL                             # (a step too close to call judges nothing)
        assert int(clear.sum()) >= B - max(1, B // 10), 'too many sessions with a margin below %g' % cal.TOL
        want = cal.lists(pv, pi, r)
        got = model.recommend_calibrated(*inputs, k=K, weight=W, item_category=category.to(dev), return_kl=True, **kw)
        assert got[0].shape == (B, K) and got[2].shape == (B,)
        _same([t[clear.to(dev)] for t in got[:2]], [t[clear] for t in want], '%s %s' % (name, sorted(kw)))
        got_pool = (got[1].cpu()[:, :, None] == pi[:, None, :]) | (got[1].cpu()[:, :, None] < 0)
        assert bool(got_pool.any(2).all()), 'an item that is not in the pool'
        assert not model.training and got[2].dtype == torch.float32
        diff = (got[2].cpu().double() - r['kl']).abs()[clear]
        WORST['kl'] = max(WORST['kl'], float(diff.max()))
        print('%s %s: max |kl - f64| %.3e (so far %.3e)' % (name, sorted(kw), float(diff.max()), WORST['kl']))
        assert bool((diff <= cal.F32 * r['kl'][clear].abs().clamp(min=1)).all())
        moved += int((got[1].cpu() != pi[:, :K]).any(1).sum())
        # list_calibration of the returned list is return_kl's value; a Python list of categories is the same vector
        assert torch.equal(model.list_calibration(*inputs, item_ids=got[1], item_category=category.tolist()), got[2])
        # weight 0: the first k columns of the pool
        _same(model.recommend_calibrated(*inputs, k=K, weight=0, item_category=category, pool=POOL, **kw), (pv[:, :K], pi[:, :K]),
              name + ' weight 0')
        if kw:
            samples = load_golden(name)[1]
            for b, (seq, _) in enumerate(samples):
                assert not set(got[1][b].tolist()) & set(seq), b
            assert not bool((got[1][got[1] >= 0] % 3 == 0).any())
    assert moved > 0, 'calibration moved no session of %s' % name
    # list_calibration of a plain list is the oracle's KL of it; the calibrated list is no further from the target
    pv, pi = [t.cpu() for t in model.recommend(*inputs, k=K)]
    got = model.list_calibration(*inputs, item_ids=pi.to(dev), item_category=category).cpu()
    want = cal.greedy64(pi, torch.zeros(pi.shape), category, K, 0.0, tcat, tw)['kl']
    assert bool(((got.double() - want).abs() <= cal.F32 * want.abs().clamp(min=1)).all())
    strong = model.recommend_calibrated(*inputs, k=K, weight=0.99, item_category=category, pool=128, return_kl=True)[2].cpu()
    assert float(strong.mean()) < float(got.mean())
    # the default pool is min(128, max(4 k, k)); an explicit target of category ids
    tc = torch.tensor([[0, 5, 5]] * B)
    tx = torch.tensor([[1.0, 0.5, 0.5]] * B)
    pv, pi = [t.cpu() for t in model.recommend(*inputs, k=40)]
    want = cal.lists(pv, pi, cal.greedy64(pi, pv, category, 10, 0.8, tc, tx, 0.05))
    _same(model.recommend_calibrated(*inputs, k=10, weight=0.8, item_category=category, target=(tc, tx), alpha=0.05), want, name + ' target')


# ------------------------------------------------------------------------------------------- 6) sharded, W = 2 on one GPU
def test_sharded_recommend_calibrated_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from calibrate_gpu_worker import K, POOL, WEIGHT, case_target, run_rank
    from norm_gpu_worker import identity_model
    from select_gpu_worker import sharded_case
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
    sr, E, _, _ = sharded_case()
    V = E.shape[0]
    category, tcat, tw = case_target(sr.shape[0], V)
    model = identity_model(E).to(dev)
    one = [t.cpu() for t in model.recommend_calibrated(sr.to(dev), k=K, weight=WEIGHT, item_category=category.to(dev), pool=POOL,
                                                       target=(tcat.to(dev), tw.to(dev)), return_kl=True)]
    assert not torch.equal(one[1], model.recommend(sr.to(dev), k=K)[1].cpu())        # the calibration binds
    assert bool((one[1] < 2560).any()) and bool((one[1] >= 2560).any())              # the lists span both shards
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])
        mine = slice(r * n, (r + 1) * n)
        assert res['collectives_dp'] == res['collectives_pool_dp'], 'the re-rank added a collective'
        for key, want in (('calibrated', one), ('calibrated_dp', [t[mine] for t in one])):
            got = res[key]
            assert torch.equal(got[1], want[1]), (r, key)                             # the list of the single device
            assert torch.equal(got[2], want[2]), (r, key)                             # ... and its KL, bit for bit
            err = float((got[0] - want[0]).abs().max())
            print('rank', r, key, 'values against the single device: %.2e' % err)
            assert err <= 2e-5, (r, key, err)        # (the sharded log-normaliser folds in another order: tests/test_norm_gpu.py)
        # ... the values are the rank's own pool's bits, and the route is the single-device kernel on that pool, bit for bit
        pv, pi = res['pool']
        here = _ops().calibrate(pi.to(dev), pv.to(dev), category.to(dev), K, WEIGHT, tcat.to(dev), tw.to(dev))
        for x, y in zip(res['route'], here):
            assert torch.equal(x, y.cpu()), r
        want = cal.lists(pv, pi, cal.greedy64(pi, pv, category, K, WEIGHT, tcat, tw))
        assert torch.equal(res['calibrated'][1], want[1]) and torch.equal(res['calibrated'][0].view(torch.int32), want[0].view(torch.int32)), r
        assert torch.equal(res['route'][0].view(torch.int32), want[0].view(torch.int32)), r


# ------------------------------------------------------------------------------------------- 7) launcher
def test_recommend_launcher_calibrate_equals_in_process_recommend_calibrated(dev, tmp_path):
    sp, col = pkg(), pkg('collate')
    sys.path.insert(0, os.path.join(ROOT, 'src', 'scripts'))
    try:
        import recommend as rec
    finally:
        sys.path.pop(0)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    sessions = rec.read_session_file(os.path.join(GOLDEN, 'sample_test.txt'))[:40]
    (tmp_path / 'sessions.txt').write_text(rec.format_sessions(sessions))
    category = [i % 7 if i % 10 else -1 for i in range(V)]
    (tmp_path / 'f').write_text(''.join('%d:%d\n' % (i, c) for i, c in enumerate(category) if c >= 0))
    out = tmp_path / 'top.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py'), '--model', 'SRGNN', '--dataset-dir', data,
                        '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--sessions',
                        str(tmp_path / 'sessions.txt'), '--calibrate', '0.7', '--categories', str(tmp_path / 'f'), '--top', '10',
                        '--output', str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.recommend_calibrated(*[x.to(dev) for x in inputs], k=10, weight=0.7, item_category=category)
    plain = model.recommend(*[x.to(dev) for x in inputs], k=10)[1]
    assert not torch.equal(idx, plain)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)                         # the same `id:logprob` format as before
        assert ids == [i for i in idx[b].tolist() if i >= 0] and len(ids) == 10, b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
