"""Drawing from the served distribution on the GPU: csrc/recommend.hip's NOISE instances through ops.score_sample,
dist.VocabParallel.sample, model.sample and src/scripts/recommend.py --sample, against the float64 restatement of the noise and
of the sampled key (tests/sample_oracle.py) and the existing score / selection oracles.

The noise is counter-based, so everything here is deterministic: lists are compared with the oracle's (equal ids where the
oracle's keys are further apart than the round-off, the list-consistency check of tests/select_oracle.py elsewhere), draws
are compared bit for bit across batches, views and shards, and the distribution is tested by chi-square at fixed seeds whose
oracle statistics tests/test_sample_cpu.py asserts."""
import os
import subprocess
import sys

import pytest
import torch

import sample_oracle as so
from select_oracle import assert_list_consistent, drop_mask, exact_case, merge_lists, scores64, select64, window_count
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')


def _ops():
    return pkg('ops')


def _t(x, dev):
    return None if x is None else x.to(dev)


def _typed(key, idx, B, k):
    assert key.dtype == torch.float32 and idx.dtype == torch.int32 and key.shape == idx.shape == (B, k)


# ------------------------------------------------------------------------------------------- a) the noise alone
def test_noise_alone_equals_the_oracle(dev):
    """sr = 0: the keys ARE the noise.  Several item ranges and a tail chunk, the largest K.  The seed is one for which the
    oracle's 129 best keys of every session lie further apart than twice the tolerance, so the ids must be equal"""
    ops = _ops()
    B, V, d, K = so.NOISE_SHAPE
    g64 = so.key64(torch.zeros(B, V, dtype=torch.float64), 1.0, so.NOISE_SEED)
    key, idx = ops.score_sample(torch.zeros(B, d, device=dev), torch.randn(V, d, device=dev), None, K, seed=so.NOISE_SEED)
    _typed(key, idx, B, K)
    rv, ri = select64(g64, K)
    err = float((key.cpu().double() - g64.gather(1, idx.cpu().long())).abs().max())
    print('noise alone %s: max |key - g64| = %.3e (bound %.0e)' % ((B, V, d, K), err, so.TOL_NOISE))
    assert torch.equal(idx.cpu().long(), ri)
    assert err < so.TOL_NOISE
    assert torch.equal(ops.sample_noise(so.NOISE_SEED, torch.arange(B), torch.arange(V)), g64)


# ------------------------------------------------------------------------------------------- b) lists against the oracle
@pytest.mark.parametrize('kind', so.LIST_KINDS)
@pytest.mark.parametrize('B,V,d', so.LIST_SHAPES)
def test_random_inputs_lists_consistent_with_the_sampled_keys(dev, B, V, d, kind):
    ops = _ops()
    K = so.LIST_K
    for mode in ('row', 'groups'):
        srs, E, cs, off_ex, off_in, listed, drop, bias, group = so.list_case(B, V, d, kind, mode)
        s64, dm = so.biased64(srs, E, cs, off_ex, off_in, listed, drop, bias, group)
        for T in so.LIST_TS:
            tol = so.tol_key(T)
            k64 = so.key64(s64, T, so.LIST_SEED)
            near = window_count(k64, K, tol, dm)
            assert int(near.max()) <= 4, 'the round-off window holds %d items: the check is vacuous for this draw' % int(near.max())
            key, idx = ops.score_sample([s.to(dev) for s in srs], _t(E, dev), _t(cs, dev), K, _t(off_ex, dev), _t(off_in, dev),
                                        _t(listed, dev), drop_listed=drop, bias=_t(bias, dev), group=_t(group, dev),
                                        temperature=T, seed=so.LIST_SEED)
            _typed(key, idx, B, K)
            err = float((key.cpu().double() - k64.gather(1, idx.cpu().long())).abs().max())
            print(kind, (B, V, d), mode, 'T %.1f: max |key - key64| %.2e (tol %.2e), window max %d' % (T, err, tol, int(near.max())))
            assert_list_consistent(key, idx, k64, tol, dm, what='%s %s %s T=%s' % (kind, (B, V, d), mode, T))
    # the noise matters: the last list is no top-K of the scores themselves
    assert not torch.equal(idx.cpu().long(), select64(s64, K, dm)[1])


# ------------------------------------------------------------------------------------------- c) every kernel path
@pytest.mark.parametrize('K', [1, 40, 128])
@pytest.mark.parametrize('B,V,d,C', [(37, 700, 100, 2), (40, 600, 512, 4), (33, 500, 1024, 2)])
def test_exact_mixture_inputs_on_every_kernel_path(dev, B, V, d, C, K):
    """the exact mixtures of tests/test_select_gpu.py (a d that is no multiple of 32, C = 2 and 4, session tiles through the
    cache): s is exact in fp32, only the noise carries round-off - without a list, with a scored and with a dropped one"""
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(d + C)
    srs = torch.randint(-8, 9, (C, B, d), generator=g).float() / 8
    srs[0] = sr
    off = torch.full((C, B), -1.0e5)
    off[torch.arange(B) % C, torch.arange(B)] = -torch.randint(0, 9, (B,), generator=g).float() / 8
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    listed[:, 4] = -1
    off_in = off.clone()
    off_in[torch.arange(B) % C, torch.arange(B)] += 2.0
    seed = 7
    for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
        key, idx = ops.score_sample(srs.to(dev), E.to(dev), cs.to(dev), K, off.to(dev), _t(oi, dev), _t(lst, dev), drop_listed=drop,
                                    seed=seed)
        _typed(key, idx, B, K)
        if drop:
            s64, dm = scores64(srs, E, cs, off), drop_mask(listed, V)
        else:
            s64, dm = scores64(srs, E, cs, off, oi, lst), None
        k64 = so.key64(s64, 1.0, seed)
        err = float((key.cpu().double() - k64.gather(1, idx.cpu().long())).abs().max())
        print('exact mix', (B, V, d, C, K), what, 'max |key - key64| %.2e' % err, 'window', int(window_count(k64, K, so.TOL_NOISE, dm).max()))
        assert_list_consistent(key, idx, k64, so.TOL_NOISE, dm, what='mixture %s %s' % ((B, V, d, C, K), what))


# ------------------------------------------------------------------------------------------- d) eligibility
def test_eligibility_fewer_rows_than_k_and_nothing_eligible(dev):
    ops = _ops()
    B, V, d, K = 5, 20, 32, 20
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(4)
    perm = torch.stack([torch.randperm(V, generator=g)[:8] for _ in range(B)])
    listed = perm[:, :5]                                    # 5 listed and dropped
    bias = torch.zeros(B + 1, V)
    bias.scatter_(1, torch.cat([perm[:, 5:], perm[:1, 5:]]), NINF)   # 3 others out of the catalogue, per session (rows 0 .. B - 1)
    bias[B] = NINF                                          # ... and a row without any item
    group = torch.arange(B)
    group[3] = B                                            # session 3: nothing eligible
    key, idx = ops.score_sample(sr.to(dev), E.to(dev), cs.to(dev), K, listed=listed.to(dev), drop_listed=True, bias=bias.to(dev),
                                group=group.to(dev), temperature=0.5, seed=2)
    _typed(key, idx, B, K)
    s64, dm = so.biased64(sr, E, cs, None, None, listed, True, bias, group)
    assert (~dm).sum(1).tolist() == [12, 12, 12, 0, 12]
    key, idx = key.cpu(), idx.cpu()
    for b in range(B):
        n = 0 if b == 3 else 12
        assert bool((idx[b, n:] == -1).all()) and bool((key[b, n:] == NINF).all()), b
        ids = idx[b, :n].long()
        assert ids.unique().numel() == n and not bool(dm[b, ids].any()) and bool(torch.isfinite(key[b, :n]).all()), b
    live = [0, 1, 2, 4]
    assert_list_consistent(key[live, :12], idx[live, :12], so.key64(s64, 0.5, 2)[live], so.tol_key(0.5), dm[live], what='12 eligible')
    # K > V without filters: V entries, then the tail
    key, idx = ops.score_sample(sr.to(dev), E.to(dev), cs.to(dev), 28, seed=2)
    assert bool((idx[:, V:] == -1).all()) and bool((key[:, V:] == NINF).all())
    assert idx[:, :V].long().sort(1).values.cpu().tolist() == [list(range(V))] * B
    assert_list_consistent(key[:, :V], idx[:, :V], so.key64(scores64(sr, E, cs), 1.0, 2), so.TOL_NOISE, what='K = 28 > V = 20')


# ------------------------------------------------------------------------------------------- e) determinism and keys
def test_draws_are_reproducible_and_do_not_depend_on_the_batch(dev):
    ops = _ops()
    B, V, d = 37, 1300, 64
    g = torch.Generator().manual_seed(21)
    sr = (torch.randn(B, d, generator=g) * 0.3).to(dev)
    E = (torch.randn(V, d, generator=g) * 0.2).to(dev)
    cs = (torch.rand(V, generator=g) + 0.5).to(dev)
    q = (torch.randperm(100000, generator=g)[:B] - 50000).to(dev)           # keys that are not the row index, some negative
    kw = dict(temperature=0.8, seed=(7 << 32) | 5)
    k20 = ops.score_sample(sr, E, cs, 20, session_keys=q, **kw)
    again = ops.score_sample(sr, E, cs, 20, session_keys=q, **kw)
    assert torch.equal(k20[0], again[0]) and torch.equal(k20[1], again[1])
    k5 = ops.score_sample(sr, E, cs, 5, session_keys=q, **kw)
    assert torch.equal(k5[0], k20[0][:, :5]) and torch.equal(k5[1], k20[1][:, :5])
    other = ops.score_sample(sr, E, cs, 20, session_keys=q, temperature=0.8, seed=(7 << 32) | 6)
    changed = int((other[1] != k20[1]).any(1).sum())
    print('another seed changes the ids of %d of %d sessions' % (changed, B))
    assert changed > B // 2
    # default keys are the row index
    dflt = ops.score_sample(sr, E, cs, 20, **kw)
    rows = ops.score_sample(sr, E, cs, 20, session_keys=torch.arange(B), **kw)
    assert torch.equal(dflt[0], rows[0]) and torch.equal(dflt[1], rows[1]) and not torch.equal(dflt[1], k20[1])
    # the sessions permuted together with their keys: the permuted result
    perm = torch.randperm(B, generator=g).to(dev)
    pk, pi = ops.score_sample(sr[perm].contiguous(), E, cs, 20, session_keys=q[perm], **kw)
    assert torch.equal(pk, k20[0][perm]) and torch.equal(pi, k20[1][perm])
    # a session alone, with its key: the row it had in the batch
    for b in (0, 17, 36):
        ok, oi = ops.score_sample(sr[b:b + 1], E, cs, 20, session_keys=q[b:b + 1], **kw)
        assert torch.equal(ok[0], k20[0][b]) and torch.equal(oi[0], k20[1][b]), b
    # strided table and session views
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E
    sw = torch.full((B, d + 8), 7.0, device=dev)
    sw[:, :d] = sr
    tv, sv = Ew[:, :d], sw[:, :d]
    assert tv.stride(0) == d + 32 and sv.stride(0) == d + 8 and not tv.is_contiguous()
    vk, vi = ops.score_sample(sv, tv, cs, 20, session_keys=q, **kw)
    assert torch.equal(vk, k20[0]) and torch.equal(vi, k20[1])
    # ... and the draw is the one the documented restatement gives
    k64 = scores64(sr, E, cs) / 0.8 + ops.sample_noise(kw['seed'], q, torch.arange(V))
    assert_list_consistent(k20[0], k20[1], k64, so.tol_key(0.8), what='sample_noise restates the draw')
    assert sorted({k[0] for k in pkg('score')._SAMPLE_WS}) == ['sample']
    assert 'sample' not in {k[0] for k in pkg('score')._BYTE_WS}


# ------------------------------------------------------------------------------------------- f) the distribution
@pytest.fixture(scope='module')
def stat_draws(dev):
    """{(V, T): ids [4096, k]} of the statistical cases, drawn once"""
    ops = _ops()
    out = {}
    for V, k in ((8, 1), (5, 2)):
        sr, E, bias = so.stat_case(V)
        for T in so.LIST_TS:
            key, idx = ops.score_sample(sr.to(dev), E.to(dev), None, k, bias=_t(bias, dev), temperature=T, seed=so.STAT_SEED,
                                        session_keys=torch.arange(so.STAT_B))
            out[(V, T)] = idx.cpu().long()
    return out


@pytest.mark.parametrize('T', so.LIST_TS)
def test_first_draw_follows_the_softmax_over_the_eligible_items(stat_draws, T):
    ids = stat_draws[(8, T)][:, 0]
    p = so.stat_probs(8, T)
    assert int((p > 0).sum()) == 6
    c = so.chi2_first(ids, p)                                  # (asserts that no ineligible item was drawn)
    same = float((ids == so.oracle_draw(8, 1, T)[:, 0]).double().mean())
    print('T %.1f: first-draw chi-square %.2f at 5 dof (< %.2f); %.4f of the draws are the oracle\'s' % (T, c, so.CHI2_5, same))
    assert c < so.CHI2_5
    if T == 0.5:                                               # positive control: the temperature is really applied
        assert so.chi2_first(ids, so.stat_probs(8, 1.0)) > so.CHI2_5


@pytest.mark.parametrize('T', so.LIST_TS)
def test_ordered_pairs_follow_plackett_luce(stat_draws, T):
    ids = stat_draws[(5, T)]
    c = so.chi2_pairs(ids, so.stat_probs(5, T))                # (asserts that no item was drawn twice)
    print('T %.1f: ordered-pair chi-square %.2f at 19 dof (< %.2f)' % (T, c, so.CHI2_19))
    assert c < so.CHI2_19
    if T == 0.5:
        assert so.chi2_pairs(ids, so.stat_probs(5, 1.0)) > so.CHI2_19


# ------------------------------------------------------------------------------------------- g) shards
def test_two_row_ranges_merge_to_the_whole_table_result(dev):
    ops = _ops()
    B, V, d, K = 33, 5000, 96, 50
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(7)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    bias = torch.randn(V, generator=g)
    bias[torch.rand(V, generator=g) < 0.3] = NINF
    sr, E, cs, listed, bias = sr.to(dev), E.to(dev), cs.to(dev), listed.to(dev), bias.to(dev)
    q = torch.arange(B, device=dev) * 3 + 1
    for kw in (dict(), dict(listed=listed, drop_listed=True, session_keys=q, temperature=0.6)):
        whole = ops.score_sample(sr, E, cs, K, seed=5, bias=bias, **kw)
        lo = ops.score_sample(sr, E[:2500], cs[:2500], K, id_lo=0, seed=5, bias=bias[:2500], **kw)
        hi = ops.score_sample(sr, E[2500:], cs[2500:], K, id_lo=2500, seed=5, bias=bias[2500:], **kw)
        assert int(hi[1].min()) >= 2500 and int(lo[1].max()) < 2500
        mv, mi = merge_lists([lo[0], hi[0]], [lo[1], hi[1]], K)
        assert torch.equal(mi, whole[1].cpu().long()) and torch.equal(mv, whole[0].cpu().double())
        assert int((hi[1] >= 2500).sum()) > 0 and int((whole[1] < 2500).sum()) > 0


def test_sharded_sample_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from sample_gpu_worker import K, SEED, T, run_rank, session_keys
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
    ops = _ops()
    sr, E, cs, listed = [t.to(dev) for t in sharded_case()]
    B = sr.shape[0]
    q = session_keys(B).to(dev)
    kw = dict(temperature=T, seed=SEED)
    plain = [t.cpu() for t in ops.score_sample(sr, E, cs, K, **kw)]
    keyed = [t.cpu() for t in ops.score_sample(sr, E, cs, K, listed=listed, drop_listed=True, session_keys=q, **kw)]
    assert not torch.equal(plain[1], keyed[1])
    n = B // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        # every rank feeds the same sessions: the full answer on every rank
        for got, want in ((res['replicated'], plain), (res['replicated_drop_keys'], keyed)):
            assert got[1].dtype == torch.int32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), r
        # every rank feeds its own slice: its own sessions' draws - default keys are the GLOBAL row index
        mine = slice(r * n, (r + 1) * n)
        got = res['data_parallel']
        assert torch.equal(got[0], plain[0][mine]) and torch.equal(got[1], plain[1][mine]), r
        want = [t.cpu() for t in ops.score_sample(sr[mine], E, cs, K, listed=listed[mine, :4 + r], drop_listed=True,
                                                  session_keys=q[mine], **kw)]
        got = res['data_parallel_drop_keys']
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), r


# ------------------------------------------------------------------------------------------- h) models
def _seen(samples, V):
    m = torch.zeros(len(samples), V, dtype=torch.bool)
    for b, (seq, _) in enumerate(samples):
        m[b, torch.tensor(seq)] = True
    return m


def _assert_draw_consistent(ids, k64, tol, drop=None, what=''):
    """the list check of (b) for ids alone (model.sample returns log-probabilities, not keys): distinct, in range, eligible;
    in the order of keys known to +-tol; no eligible item left out whose key is ahead of the last one by more than 2 tol"""
    ids = ids.cpu().long()
    B, V = k64.shape
    for b in range(B):
        i = ids[b]
        assert int(i.min()) >= 0 and int(i.max()) < V and i.unique().numel() == i.numel(), (what, b, i.tolist())
        if drop is not None:
            assert not bool(drop[b, i].any()), (what, b, 'ineligible id returned')
        v = k64[b, i]
        assert bool((v[1:] <= v[:-1] + 2 * tol).all()), (what, b, 'order', v.tolist())
        must = k64[b] > float(v.min()) + 2 * tol
        if drop is not None:
            must &= ~drop[b]
        must[i] = False
        assert not bool(must.any()), (what, b, 'missing', must.nonzero().flatten().tolist()[:8])


@pytest.mark.parametrize('name', ['srgnn_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_sample_against_forward_and_score_items(dev, name):
    from test_rank_gpu import _fixture_model
    from util import load_golden
    ops = _ops()
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    B = labels.numel()
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    V = s64.shape[1]
    seen = _seen(samples, V)
    g64 = ops.sample_noise(3, torch.arange(B), torch.arange(V))
    val, ids = model.sample(*inputs, k=20, seed=3)
    _typed(val, ids, B, 20)
    assert not model.training
    assert torch.equal(val, model.score_items(*inputs, items=ids))
    assert float((val.cpu().double() - s64.gather(1, ids.cpu().long())).abs().max()) < 1e-4
    _assert_draw_consistent(ids, s64 + g64, so.tol_key(1.0), what=name)
    assert not torch.equal(ids, model.recommend(*inputs, k=20)[1])           # a draw, not the arg-max
    # exclude_seen, at another temperature
    val, ids = model.sample(*inputs, k=20, seed=3, temperature=2.0, exclude_seen=True)
    assert not bool(seen.gather(1, ids.cpu().long()).any()), 'an item of the session itself was drawn'
    assert torch.equal(val, model.score_items(*inputs, items=ids, exclude_seen=True))
    _assert_draw_consistent(ids, s64 / 2.0 + g64, so.tol_key(2.0), seen, what=name + ' exclude_seen')
    # a bias that filters, renormalised values, caller's keys
    gb = torch.Generator().manual_seed(V)
    bias = torch.randint(-8, 9, (V,), generator=gb).float() / 8
    bias[torch.rand(V, generator=gb) < 0.3] = NINF
    q = torch.arange(B) * 11 - 40
    kw = dict(item_bias=bias.to(dev), exclude_seen=True, renormalize=True)
    val, ids = model.sample(*inputs, k=20, seed=3, temperature=0.5, session_keys=q, **kw)
    assert torch.equal(val, model.score_items(*inputs, items=ids, **kw))
    off = seen | (bias == NINF)[None]
    k64 = (s64 + bias.double()[None]) / 0.5 + ops.sample_noise(3, q, torch.arange(V))
    _assert_draw_consistent(ids, k64, so.tol_key(0.5), off, what=name + ' bias, renormalize')
    mass = model.log_mass(*inputs, exclude_seen=True, item_bias=bias.to(dev)).cpu().double()
    err = float((val.cpu().double() - (s64 + bias.double()[None] - mass[:, None]).gather(1, ids.cpu().long())).abs().max())
    print(name, 'renormalised values against forward() + bias - log_mass: %.2e' % err)
    assert err < 2e-4
    # fewer eligible items than k: (-inf, -1) slots
    allow = torch.full((V,), NINF)
    allow[:7] = 0.0
    val, ids = model.sample(*inputs, k=10, seed=3, item_bias=allow.to(dev))
    assert bool((ids[:, 7:] == -1).all()) and bool((val[:, 7:] == NINF).all())
    assert ids[:, :7].long().sort(1).values.cpu().tolist() == [list(range(7))] * B and bool(torch.isfinite(val[:, :7]).all())
    # the training flag comes back, and bad arguments raise before the model runs
    model.train()
    model.sample(*inputs, k=2)
    assert model.training
    ran = []
    orig = model.session_repr
    model.session_repr = lambda *a, **k: ran.append(1) or orig(*a, **k)
    try:
        for bad in (dict(item_bias=torch.zeros(V + 1, device=dev)), dict(temperature=0.0), dict(temperature=float('inf'))):
            with pytest.raises(ValueError, match='^sample: '):
                model.sample(*inputs, k=2, **bad)
        assert not ran and model.training
    finally:
        del model.session_repr
        model.eval()


def test_mixture_sample_allocates_no_score_matrix(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, K = 37484, 64, 64, 3
    torch.manual_seed(3)
    model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
    (mg,), _ = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 5))
    mg = mg.to(dev)
    model.sample(mg, k=100, seed=1)                      # workspaces and column scales are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = model.sample(mg, k=100, seed=1)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.2f MB, one (B, V) fp32 matrix %.2f MB' % (rise / 2 ** 20, B * V * 4 / 2 ** 20))
    assert rise < B * V * 4, rise
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    # the route it replaces: forward(), Gumbel noise of the same size, topk - several such matrices: the measure bites
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        s = model(mg)
        (s - torch.log(-torch.log(torch.rand_like(s)))).topk(100)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > B * V * 4
    k64 = s.double().cpu() + _ops().sample_noise(1, torch.arange(B), torch.arange(V))
    _assert_draw_consistent(idx, k64, so.tol_key(1.0), what='V = 37484 mixture')
    assert float((val.cpu().double() - s.double().cpu().gather(1, idx.cpu().long())).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------- i) launcher
def test_recommend_launcher_sample_equals_in_process_sample_for_any_batching(dev, tmp_path):
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
    texts = []
    for bs in (40, 16):
        out = tmp_path / ('draw%d.txt' % bs)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py'), '--model', 'SRGNN', '--dataset-dir', data,
                            '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--sessions',
                            str(tmp_path / 'sessions.txt'), '--sample', '--seed', '5', '--temperature', '0.7', '--top', '10',
                            '--exclude-seen', '--batch-size', str(bs), '--output', str(out)],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        texts.append(out.read_text())
    lines = texts[0].splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.sample(*[x.to(dev) for x in inputs], k=10, temperature=0.7, seed=5, session_keys=torch.arange(len(sessions)),
                            exclude_seen=True)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == idx[b].tolist(), b
        assert not set(ids) & set(sessions[b]), b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
    # the file does not depend on how the lines were batched: the session key is the line number
    assert texts[1] == texts[0]
