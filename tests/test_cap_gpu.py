"""Per-category caps on the GPU: csrc/cap_select.hip through ops.cap_select, dist.VocabParallel.cap_select,
model.recommend_capped and src/scripts/recommend.py, against the Python loop of tests/cap_oracle.py.  Integer logic on an
existing order: everything is compared with `==`.

Random pools, runs of one category across every chunk boundary, the early exit at slot 255 / 256 / 257 with garbage behind
it, a cap of 0, nothing accepted, G = 1 and G = 16384, views and batch independence, the four model families against their
own pools (both stages of the pool policy), two ranks on one GPU, and the launcher."""
import os
import subprocess
import sys

import pytest
import torch

import cap_oracle as co
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')


def _ops():
    return pkg('ops')


def _rule(ops, category, caps, dev):
    category, caps = torch.as_tensor(category), torch.as_tensor(caps)
    return ops.CapRule(category.to(torch.int32).to(dev), caps.to(torch.int32).to(dev), caps.numel())


def _check(out, ids, val, category, caps, k, what):
    """pick / kept / scanned EQUAL to the oracle's, val the pool's own bits at the picks (-inf in the tail)"""
    got_val, pick, kept, scanned = [t.cpu() for t in out]
    B = ids.shape[0]
    assert got_val.dtype == torch.float32 and pick.dtype == kept.dtype == scanned.dtype == torch.int32, what
    assert pick.shape == got_val.shape == (B, k) and kept.shape == scanned.shape == (B,), what
    want_pick, want_kept, want_scanned = co.capped(ids, category, caps, k)
    want_pick = torch.tensor(want_pick, dtype=torch.int32).view(B, k)
    bad = (pick != want_pick).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. picks %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], pick[bad][0].tolist()[:16], want_pick[bad][0].tolist()[:16])
    assert kept.tolist() == want_kept, what
    assert scanned.tolist() == want_scanned, what
    want = torch.where(pick < 0, torch.full_like(got_val, NINF), val.gather(1, pick.clamp(min=0).long()))
    assert torch.equal(got_val.view(torch.int32), want.view(torch.int32)), '%s: val is not val[pick] bit for bit' % what
    return pick, kept, scanned


# ------------------------------------------------------------------------------------------- 1) random pools
@pytest.mark.parametrize('B,P,k,G', [(1, 1, 1, 1), (33, 128, 20, 7), (5, 300, 128, 50), (2, 4096, 100, 3), (3, 4096, 4096, 16384)])
def test_random_pools_equal_the_oracle(dev, B, P, k, G):
    ops = _ops()
    ids, val, category, caps = co.random_pool(B, P, G)
    rule = _rule(ops, category, caps, dev)
    n = category.numel()
    for dtype in (torch.int64, torch.int32):
        out = ops.cap_select(ids.to(dtype).to(dev), val.to(dev), rule, k)
        pick, kept, _ = _check(out, ids, val, category, caps, k, 'random %s %s' % ((B, P, k, G), dtype))
    if P > 1:
        free = co.capped(ids, category, [P] * G, k)[0]
        assert pick.tolist() != free, 'no cap binds: the case shows nothing'
    # ids >= n_items, and < -1, in the unfilled slots: refused by default, unfilled slots under checked=True
    gids, gval, _, _ = co.random_pool(B, P, G, garbage=True)
    if bool((gids >= n).any()):
        with pytest.raises(ValueError):
            ops.cap_select(gids.to(dev), gval.to(dev), rule, k)
    for dtype in (torch.int64, torch.int32):
        out = ops.cap_select(gids.to(dtype).to(dev), gval.to(dev), rule, k, checked=True)
        _check(out, gids, gval, category, caps, k, 'garbage %s %s' % ((B, P, k, G), dtype))
    # an id beyond int32 is an unfilled slot, not the item it would wrap to
    if P > 1:
        far = ids.clone()
        far[:, 0] = 2 ** 32 + far[:, 1].clamp(min=0)
        _check(ops.cap_select(far.to(dev), val.to(dev), rule, k, checked=True), far, val, category, caps, k, 'beyond int32')


# ------------------------------------------------------------------------------------------- 2) chunk boundaries
@pytest.mark.parametrize('c', [1, 63, 64, 65, 255, 256, 257, 1023])
def test_one_category_with_cap_c_keeps_the_first_c_slots(dev, c):
    ops = _ops()
    P = 1024
    ids = torch.stack([torch.arange(P), torch.arange(P).flip(0)])
    val = torch.sort(torch.randn(2, P, generator=torch.Generator().manual_seed(c)), 1, descending=True).values
    category, caps = [0] * P, [c]
    out = ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), P)
    pick, kept, scanned = _check(out, ids, val, category, caps, P, 'one category, cap %d' % c)
    assert pick[:, :c].tolist() == [list(range(c))] * 2 and bool((pick[:, c:] == -1).all())
    assert kept.tolist() == [c, c] and scanned.tolist() == [P, P]
    if c > 1:                                                    # k = c - 1: the walk ends behind slot c - 2
        _, _, scanned = _check(ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), c - 1), ids, val,
                               category, caps, c - 1, 'one category, cap %d, k = cap - 1' % c)
        assert scanned.tolist() == [c - 1] * 2


def test_two_alternating_categories_and_a_capped_item_behind_a_full_category(dev):
    ops = _ops()
    P = 1024
    ids = torch.arange(P)[None]
    val = torch.linspace(0, -5, P)[None]
    category, caps = [i % 2 for i in range(P)], [2, 300]
    out = ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), 400)
    pick, kept, scanned = _check(out, ids, val, category, caps, 400, 'alternating')
    assert pick[0, :302].tolist() == [0, 1, 2] + list(range(3, 600, 2)) and kept.tolist() == [302] and scanned.tolist() == [P]
    for at in (255, 256, 257):                                   # category 0 is full after slot 0; category 1 has one item, at `at`
        category = [0] * P
        category[at] = 1
        for cap1, want in ((1, [0, at]), (0, [0])):
            caps = [1, cap1]
            out = ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), 3)
            pick, kept, _ = _check(out, ids, val, category, caps, 3, 'single item at %d, cap %d' % (at, cap1))
            assert pick[0, :len(want)].tolist() == want and kept.tolist() == [len(want)]


@pytest.mark.parametrize('at', [255, 256, 257])
def test_early_exit_scanned_is_exact_and_slots_behind_it_may_hold_garbage(dev, at):
    """the k-th acceptance falls at slot `at`: scanned = at + 1, and nothing behind it matters - ids far outside the catalogue
    there (checked=True: the caller vouches) change nothing and are not dereferenced"""
    ops = _ops()
    P, k, n = 1024, 100, 2000
    g = torch.Generator().manual_seed(at)
    ids = torch.randperm(n, generator=g)[:P][None].repeat(3, 1)
    val = torch.sort(torch.randn(3, P, generator=g), 1, descending=True).values
    accept = torch.zeros(P, dtype=torch.bool)
    accept[torch.randperm(at, generator=g)[:k - 1]] = True       # k - 1 accepted slots before `at`, the k-th at `at`
    accept[at] = True
    category = torch.zeros(n, dtype=torch.long)                  # category 0 has cap 0; the accepted items have none
    category[ids[0][accept]] = -1
    caps = [0, 5]
    ids[1, at + 1:] = 2 ** 31 - 1
    ids[2, at + 1:] = -2 ** 31
    out = ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), k, checked=True)
    pick, kept, scanned = _check(out, ids, val, category, caps, k, 'early exit at %d' % at)
    assert scanned.tolist() == [at + 1] * 3 and kept.tolist() == [k] * 3 and pick[:, -1].tolist() == [at] * 3
    assert torch.equal(pick[0], pick[1]) and torch.equal(pick[0], pick[2])


# ------------------------------------------------------------------------------------------- 3) caps of 0, nothing, G = 1 / 16384
def test_cap_zero_nothing_accepted_and_the_largest_category_id(dev):
    ops = _ops()
    B, P, n = 4, 300, 1400
    g = torch.Generator().manual_seed(9)
    ids = torch.randperm(n, generator=g)[:B * P].view(B, P)      # (disjoint pools: an item set below belongs to one slot)
    val = torch.sort(torch.randn(B, P, generator=g), 1, descending=True).values
    # a cap-0 category is never shown
    category = torch.randint(0, 3, (n,), generator=g)
    caps = [2, 0, 300]
    pick, _, _ = _check(ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), 50), ids, val, category, caps,
                        50, 'cap 0')
    shown = category[ids.gather(1, pick.clamp(min=0).long())]
    assert not bool((shown == 1).any()) and bool((shown == 2).sum(1).ge(40).all())
    # everything capped away: kept 0, scanned P, a (-1, -inf) list; and nothing filled at all
    out = ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, [0, 0, 0], dev), 50)
    pick, kept, scanned = _check(out, ids, val, category, [0, 0, 0], 50, 'all capped')
    assert bool((pick == -1).all()) and kept.tolist() == [0] * B and scanned.tolist() == [P] * B and bool((out[0] == NINF).all())
    none = torch.full((B, P), -1)
    out = ops.cap_select(none.to(dev), val.to(dev), _rule(ops, category, caps, dev), 50)
    _, kept, scanned = _check(out, none, val, category, caps, 50, 'all unfilled')
    assert kept.tolist() == [0] * B and scanned.tolist() == [P] * B
    # G = 1 and G = 16384 with the category id G - 1 present in every pool; a category >= G in the table is no category
    for G in (1, 16384):
        category = torch.randint(0, G, (n,), generator=g)
        category[category == G - 1] = -1                         # (the last category: the three slots below alone)
        category[ids[:, 3]] = G - 1
        category[ids[:, 5]] = G - 1
        category[ids[:, 9]] = G - 1
        category[ids[0, 20]] = G + 5
        caps = torch.randint(0, 3, (G,), generator=g)
        caps[G - 1] = 2
        pick, _, _ = _check(ops.cap_select(ids.to(dev), val.to(dev), _rule(ops, category, caps, dev), 200), ids, val, category,
                            caps, 200, 'G = %d' % G)
        assert all(3 in row and 5 in row and 9 not in row for row in pick.tolist()) and 20 in pick[0].tolist()


# ------------------------------------------------------------------------------------------- 4) views and batching
def test_views_and_batch_independence_bit_for_bit(dev):
    ops = _ops()
    B, P, k, G = 33, 600, 150, 11
    ids, val, category, caps = co.random_pool(B, P, G, seed=4)
    rule = _rule(ops, category, caps, dev)
    base = ops.cap_select(ids.to(dev), val.to(dev), rule, k)
    _check(base, ids, val, category, caps, k, 'views: base')
    wide_i = torch.full((B, P + 40), 7, dtype=torch.int64, device=dev)
    wide_v = torch.full((B, P + 40), 7.0, device=dev)
    wide_i[:, 8:P + 8], wide_v[:, 8:P + 8] = ids.to(dev), val.to(dev)
    vi, vv = wide_i[:, 8:P + 8], wide_v[:, 8:P + 8]
    assert vi.stride(0) == P + 40 and not vi.is_contiguous()
    for what, got in (('row-strided views', ops.cap_select(vi, vv, rule, k)),
                      ('int16 ids', ops.cap_select(ids.to(torch.int16).to(dev), val.to(dev), rule, k))):
        for a, b in zip(base, got):
            assert torch.equal(a, b), what
    for b in (0, 17, B - 1):                                     # session b alone is row b of the batch of 33
        alone = ops.cap_select(ids[b:b + 1].to(dev), val[b:b + 1].to(dev), rule, k)
        for x, y in zip(base, alone):
            assert torch.equal(x[b:b + 1], y), b


# ------------------------------------------------------------------------------------------- 5) models
_MODELS = {}


def _model(name, dev):
    if name not in _MODELS:
        from test_rank_gpu import _fixture_model
        _MODELS[name] = _fixture_model(name, dev)
    return _MODELS[name]


def _expect(pool, category, caps, k):
    """(values, ids, complete) the oracle gives for the pool (val, ids) of a model"""
    pv, pi = [t.cpu() for t in pool]
    v, i = co.capped_lists(pv, pi.long(), category, caps, k)
    kept = torch.tensor(co.capped(pi.long(), category, caps, k)[1])
    return v, i, (kept == k) | (pi[:, -1] < 0)


def _same(got, want, what):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32, what
    assert torch.equal(got[1].cpu(), want[1]), '%s: ids' % what
    assert torch.equal(got[0].cpu().view(torch.int32), want[0].view(torch.int32)), '%s: values are not the pool\'s bits' % what


@pytest.mark.parametrize('name', ['srgnn_s32', 'niser_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_recommend_capped_against_its_own_pools(dev, name):
    from util import load_golden
    ops = _ops()
    z, model, inputs, labels = _model(name, dev)
    B, V = labels.numel(), model._num_items()
    assert 128 < V <= 4096
    pool128, pool4096 = model.recommend(*inputs, k=128), model.recommend_many(*inputs, k=4096)
    # id % 50, at most 2 of each: 100 items fit, the 128-item pool gives the 20
    cat50 = torch.arange(V) % 50
    want = _expect(pool128, cat50, [2] * 50, 20)
    assert bool(want[2].all()) and int(want[1].min()) >= 0
    got = model.recommend_capped(*inputs, k=20, item_category=cat50.to(dev), max_per_category=2, return_complete=True)
    _same(got, want, name + ' %50')
    assert got[2].dtype == torch.bool and got[2].tolist() == [True] * B and not model.training
    assert not torch.equal(got[1], pool128[1][:, :20]), 'no cap binds in any session'
    rule = ops.cap_rule(V, cat50, 2, device=dev)
    _same(model.recommend_capped(*inputs, k=20, rule=rule), want, name + ' %50 by rule')
    # id % 5, at most 2 of each: 10 items whatever the pool - stage 1 is incomplete, stage 2 runs and its pool ends unfilled
    cat5 = torch.arange(V) % 5
    assert not bool(_expect(pool128, cat5, [2] * 5, 20)[2].any())
    want = _expect(pool4096, cat5, [2] * 5, 20)
    got = model.recommend_capped(*inputs, k=20, item_category=cat5, max_per_category=2, return_complete=True)
    _same(got, want, name + ' %5')
    assert bool((got[1][:, :10] >= 0).all()) and bool((got[1][:, 10:] == -1).all()) and bool((got[0][:, 10:] == NINF).all())
    assert got[2].tolist() == [True] * B
    # explicit pools on both sides of 128; a full pool that runs short is not complete
    for P in (100, 128):
        want = _expect(model.recommend(*inputs, k=P), cat5, [2] * 5, 20)
        got = model.recommend_capped(*inputs, k=20, item_category=cat5, max_per_category=2, pool=P, return_complete=True)
        _same(got, want, name + ' pool %d' % P)
        assert got[2].tolist() == [False] * B
    for P, k in ((129, 20), (1000, 300)):
        want = _expect(model.recommend_many(*inputs, k=P), cat50, [2] * 50, k)
        got = model.recommend_capped(*inputs, k=k, rule=rule, pool=P, return_complete=True)
        _same(got, want, name + ' pool %d' % P)
        assert got[2].cpu().tolist() == want[2].tolist()
    # k > 128 without a pool: the 4096-item pool directly
    _same(model.recommend_capped(*inputs, k=200, rule=rule), _expect(pool4096, cat50, [2] * 50, 200)[:2], name + ' k 200')
    # exclude_seen and an item_bias with -inf entries: the pools of the same keywords
    bias = torch.zeros(V, device=dev)
    bias[::3] = NINF
    bias[1::3] = 0.5
    kw = dict(exclude_seen=True, item_bias=bias)
    want = _expect(model.recommend(*inputs, k=128, **kw), cat50, [2] * 50, 20)
    assert bool(want[2].all())
    got = model.recommend_capped(*inputs, k=20, rule=rule, **kw)
    _same(got, want, name + ' exclude_seen + bias')
    samples = load_golden(name)[1]
    for b, (seq, _) in enumerate(samples):
        assert not set(got[1][b].tolist()) & set(seq), b
    assert not bool((got[1] % 3 == 0).any())
    want = _expect(model.recommend_many(*inputs, k=4096, **kw), cat5, [2] * 5, 20)
    _same(model.recommend_capped(*inputs, k=20, item_category=cat5, max_per_category=2, **kw), want, name + ' %5 exclude_seen + bias')


# ------------------------------------------------------------------------------------------- 6) sharded, W = 2 on one GPU
def test_sharded_recommend_capped_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from cap_gpu_worker import K, case_rule, run_rank, split_rule, tight_rule
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
    category, caps = case_rule(V)
    model = identity_model(E).to(dev)
    rule = _ops().cap_rule(V, category, caps, device=dev)
    one = [t.cpu() for t in model.recommend_capped(sr.to(dev), k=K, rule=rule, exclude_seen=False)]
    many = [t.cpu() for t in model.recommend_capped(sr.to(dev), k=K, rule=rule, pool=300)]
    tight = _ops().cap_rule(V, *tight_rule(V), device=dev)
    fallback = [t.cpu() for t in model.recommend_capped(sr.to(dev), k=20, rule=tight, return_complete=True)]
    assert not torch.equal(one[1], model.recommend(sr.to(dev), k=K)[1].cpu())        # the caps bind
    assert bool((one[1] < 2560).any()) and bool((one[1] >= 2560).any())              # the lists span both shards
    assert bool((fallback[1][:, :10] >= 0).all()) and bool((fallback[1][:, 10:] == -1).all())
    assert fallback[2].tolist() == [False] * sr.shape[0]                              # V > 4096: even that pool was full
    n = sr.shape[0] // world
    # the rule that binds for rank 1's sessions only: stage 1 completes every session of rank 0 and not session 16
    pool_ids = model.recommend(sr.to(dev), k=128)[1].cpu()
    cat_s, caps_s = split_rule(pool_ids, V)
    stage1 = torch.tensor(co.capped(pool_ids.long(), cat_s, caps_s, K)[1]) == K
    assert bool(stage1[:n].all()) and not bool(stage1[n]), stage1.tolist()
    split = [t.cpu() for t in model.recommend_capped(sr.to(dev), k=K, rule=_ops().cap_rule(V, cat_s, caps_s, device=dev),
                                                     pool=4096, return_complete=True)]
    assert split[2].tolist() == [True] * sr.shape[0]
    counts = []
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])
        assert torch.equal(res['pool'][1], pool_ids), r                               # (the worker built the same rule)
        mine = slice(r * n, (r + 1) * n)
        counts.append((res['collectives_dp_split'], res['collectives_dp']))
        assert torch.equal(res['capped_dp_split'][2], split[2][mine]), r
        for key, want in (('capped', one), ('capped_many', many), ('capped_fallback', fallback),
                          ('capped_dp', [t[mine] for t in one]), ('capped_dp_split', [t[mine] for t in split])):
            got = res[key]
            assert torch.equal(got[1], want[1]), (r, key)                             # the list of the single device
            tail = want[1] < 0
            assert bool((got[0][tail] == NINF).all()), (r, key)
            err = float((got[0][~tail] - want[0][~tail]).abs().max())
            print('rank', r, key, 'values against the single device: %.2e' % err)
            assert err <= 2e-5, (r, key, err)        # (the sharded log-normaliser folds in another order: tests/test_norm_gpu.py)
        assert torch.equal(res['capped_fallback'][2], fallback[2]), r
        # ... and its values are its own pool's bits, by the oracle
        pv, pi = res['pool']
        v, i = co.capped_lists(pv, pi.long(), category, caps, K)
        assert torch.equal(res['capped'][1], i) and torch.equal(res['capped'][0].view(torch.int32), v.view(torch.int32)), r
        for got, want in zip(res['route_dp'], res['route']):
            assert torch.equal(got, want[r * n:(r + 1) * n]), r
        assert torch.equal(res['route'][0].view(torch.int32), v.view(torch.int32)), r
    # both ranks issued the same collectives, and more of them than a call that ends after stage 1: rank 0 followed rank 1
    assert counts[0] == counts[1] and counts[0][0] > counts[0][1] + 1, counts


# ------------------------------------------------------------------------------------------- 7) launcher
def test_recommend_launcher_caps_equal_in_process_recommend_capped(dev, tmp_path):
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
    (tmp_path / 'cats.txt').write_text(''.join('%d:%d\n' % (i, c) for i, c in enumerate(category) if c >= 0))
    (tmp_path / 'caps.txt').write_text('3:0\n4:1\n')
    caps = [2, 2, 2, 0, 1, 2, 2]
    out = tmp_path / 'top.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py'), '--model', 'SRGNN', '--dataset-dir', data,
                        '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--sessions',
                        str(tmp_path / 'sessions.txt'), '--top', '10', '--categories', str(tmp_path / 'cats.txt'),
                        '--max-per-category', '2', '--category-caps', str(tmp_path / 'caps.txt'), '--exclude-seen',
                        '--output', str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.recommend_capped(*[x.to(dev) for x in inputs], k=10, item_category=category, max_per_category=caps,
                                      exclude_seen=True)
    plain = model.recommend(*[x.to(dev) for x in inputs], k=10, exclude_seen=True)[1]
    assert not torch.equal(idx, plain)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == [i for i in idx[b].tolist() if i >= 0], b
        assert not set(ids) & set(sessions[b]), b
        count = {}
        for i in ids:
            count[category[i]] = count.get(category[i], 0) + 1
        assert all(c < 0 or m <= caps[c] for c, m in count.items()), (b, count)
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
