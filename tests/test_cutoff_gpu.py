"""Truncated sampling on the GPU: csrc/score_cutoff.hip through ops.score_cutoff / ops.cutoff_passes, the floor operand of
csrc/recommend.hip through ops.score_select / ops.score_sample, model.cutoff and model.sample(top_k / top_p / min_p), against the
float64 restatement of the contract (tests/cutoff_oracle.py) over the existing score oracles.

Where the scores are exact in fp32 the floors and counts must be the oracle's own numbers; elsewhere they must be consistent
with scores known to 1e-4 and masses known to tol_m(T).  Everything is deterministic, so bits are compared across launch
splits, shards, batches and views."""
import pytest
import torch

import cutoff_oracle as co
import sample_oracle as so
from select_oracle import drop_mask, exact_case, scores64, window_count
from util import pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')
CHI2_3 = 21.11              # 1 - 1e-4 quantile of chi-square, 3 degrees of freedom (first draw among 4 kept items)


def _ops():
    return pkg('ops')


def _t(x, dev):
    return None if x is None else x.to(dev)


def _typed(out, B):
    floor, count, log_kept, top = out
    assert floor.dtype == log_kept.dtype == top.dtype == torch.float32 and count.dtype == torch.int32
    assert floor.shape == count.shape == log_kept.shape == top.shape == (B,)
    assert not bool(torch.isnan(floor).any() | torch.isnan(log_kept).any() | torch.isnan(top).any())
    assert bool((log_kept <= 0).all())
    return floor.cpu().double(), count.cpu().long(), log_kept.cpu().double(), top.cpu().double()


def _assert_log_kept(lk, want, what):
    """the kept share within TOL_MASS_EXACT relative (an absolute bound on its log), plus the fp32 rounding of the log"""
    fin = torch.isfinite(want)
    assert torch.equal(lk[~fin], want[~fin]), what
    err = (lk[fin] - want[fin]).abs()
    assert bool((err <= co.TOL_MASS_EXACT + 2.0 ** -23 * want[fin].abs()).all()), (what, float(err.max()))


# ------------------------------------------------------------------------------------------- a) exact cases, every criterion
@pytest.mark.parametrize('B,V,d', co.EXACT_SHAPES)
def test_exact_inputs_every_criterion_equals_the_oracle(dev, B, V, d):
    ops = _ops()
    sr, E, cs = co.exact_inputs(B, V, d)
    s64 = scores64(sr, E, cs)
    assert torch.equal((sr @ (E * cs[:, None]).t()).double(), s64), 'the fp32 scores of the exact case are not exact'
    m64 = s64.max(1).values + 0.0
    dsr, dE, dcs = sr.to(dev), E.to(dev), cs.to(dev)
    for T in co.EXACT_TS:
        for k in (1, 129, 1000, V, V + 5):
            floor, count, lk, top = _typed(ops.score_cutoff(dsr, dE, dcs, top_k=k, temperature=T), B)
            want = co.floor64(s64, None, T, top_k=k)
            assert torch.equal(top, m64) and torch.equal(floor, want), ('top_k', k, T)
            assert torch.equal(count, co.count64(s64, None, want)), ('top_k count', k, T)
            _assert_log_kept(lk, co.kept64(s64, None, T, want), ('top_k', k, T))
        for q in co.EXACT_MIN_PS:
            floor, count, lk, top = _typed(ops.score_cutoff(dsr, dE, dcs, min_p=q, temperature=T), B)
            want = co.tau_q32(m64, T, q)
            assert torch.equal(floor, want) and torch.equal(count, co.count64(s64, None, want)), ('min_p', q, T)
            _assert_log_kept(lk, co.kept64(s64, None, T, want), ('min_p', q, T))
        for p in co.EXACT_PS:
            floor, count, lk, top = _typed(ops.score_cutoff(dsr, dE, dcs, top_p=p, temperature=T), B)
            want = co.tau_p64(s64, None, T, p)
            dec = co.decided(s64, None, T, p)
            print('exact', (B, V, d), 'T %.1f p %.1f: %d of %d sessions decided, counts %d .. %d' %
                  (T, p, int(dec.sum()), B, int(count.min()), int(count.max())))
            assert float(dec.double().mean()) >= 0.85
            assert torch.equal(floor[dec], want[dec]), ('top_p floor', p, T)
            assert torch.equal(count[dec], co.count64(s64, None, want)[dec]), ('top_p count', p, T)
            up, dn = co.neighbours(s64, None, want)
            und = ~dec
            assert bool(((floor[und] == want[und]) | (floor[und] == up[und]) | (floor[und] == dn[und])).all()), ('undecided', p, T)
            _assert_log_kept(lk, co.kept64(s64, None, T, floor), ('top_p', p, T))
            # combinations: the largest of the floors, each as the kernel itself found it
            fk = ops.score_cutoff(dsr, dE, dcs, top_k=129, temperature=T)[0]
            fq = ops.score_cutoff(dsr, dE, dcs, min_p=0.5, temperature=T)[0]
            both = ops.score_cutoff(dsr, dE, dcs, top_k=129, top_p=p, min_p=0.5, temperature=T)
            fb, cb, lb, _ = _typed(both, B)
            assert torch.equal(both[0].cpu(), torch.maximum(torch.maximum(fk.cpu(), fq.cpu()), floor.float()))
            assert torch.equal(cb, co.count64(s64, None, fb))
            _assert_log_kept(lb, co.kept64(s64, None, T, fb), ('all three', p, T))
    none = _typed(ops.score_cutoff(dsr, dE, dcs), B)
    assert bool((none[0] == NINF).all()) and bool((none[1] == V).all()) and bool((none[2] == 0).all())


# ------------------------------------------------------------------------------------------- b) random inputs
@pytest.mark.parametrize('kind', so.LIST_KINDS)
@pytest.mark.parametrize('B,V,d', co.RANDOM_SHAPES)
def test_random_inputs_consistent_with_the_float64_distribution(dev, B, V, d, kind):
    ops = _ops()
    for mode in ('row', 'groups'):
        srs, E, cs, off_ex, off_in, listed, drop, bias, group = so.list_case(B, V, d, kind, mode)
        s64, dm = so.biased64(srs, E, cs, off_ex, off_in, listed, drop, bias, group)
        args = ([s.to(dev) for s in srs], _t(E, dev), _t(cs, dev), _t(off_ex, dev), _t(off_in, dev), _t(listed, dev))
        kw = dict(drop_listed=drop, bias=_t(bias, dev), group=_t(group, dev))
        for T in co.EXACT_TS:
            for p in co.EXACT_PS:
                floor, count, lk, top = _typed(ops.score_cutoff(*args, top_p=p, temperature=T, **kw), B)
                width = co.assert_top_p_consistent(floor, count, s64, dm, T, p, what=(kind, mode, T, p))
                assert float((top - co.weights64(s64, dm, T)[1]).abs().max()) < co.TOL_S
                live = co.weights64(s64, dm, T)[0].sum(1) > 0
                share, tm = torch.exp(lk), co.tol_m(T)
                assert bool((share <= co.mass_ge64(s64, dm, T, floor - co.TOL_S) + tm)[live].all()), (kind, mode, T, p)
                assert bool((share >= co.mass_ge64(s64, dm, T, floor + co.TOL_S, strict=True) - tm)[live].all()), (kind, mode, T, p)
                print(kind, (B, V, d), mode, 'T %.1f p %.1f: counts %d .. %d, interval width max %d' %
                      (T, p, int(count.min()), int(count.max()), int(width.max())))
        for k in (1, 50, 700):
            floor, count, lk, top = _typed(ops.score_cutoff(*args, top_k=k, **kw), B)
            want = co.tau_k64(s64, dm, k)
            win = window_count(s64, k, co.TOL_S, dm)
            assert float((floor - want).abs().max()) < co.TOL_S, (kind, mode, k)
            assert bool(((count - co.count64(s64, dm, want)).abs() <= win).all()), (kind, mode, k)


# ------------------------------------------------------------------------------------------- c) every kernel path
@pytest.mark.parametrize('B,V,d,C', [(37, 700, 100, 2), (40, 600, 512, 4), (33, 500, 1024, 2)])
def test_exact_mixture_inputs_on_every_kernel_path(dev, B, V, d, C):
    """the exact mixtures of tests/test_sample_gpu.py (a d that is no multiple of 32, C = 2 and 4, session tiles through the
    cache): s is exact in fp32 - without a list, with a scored and with a dropped one"""
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(d + C)
    srs = torch.randint(-8, 9, (C, B, d), generator=g).float() / 8
    srs[0] = sr
    srs = srs / 8
    off = torch.full((C, B), -1.0e5)
    off[torch.arange(B) % C, torch.arange(B)] = -torch.randint(0, 9, (B,), generator=g).float() / 8
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    listed[:, 4] = -1
    off_in = off.clone()
    off_in[torch.arange(B) % C, torch.arange(B)] += 2.0
    for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
        if drop:
            s64, dm = scores64(srs, E, cs, off), drop_mask(listed, V)
        else:
            s64, dm = scores64(srs, E, cs, off, oi, lst), None
        args = (srs.to(dev), E.to(dev), cs.to(dev), off.to(dev), _t(oi, dev), _t(lst, dev))
        for k in (1, 129, V - 4, V + 5):
            floor, count, lk, top = _typed(ops.score_cutoff(*args, drop_listed=drop, top_k=k), B)
            want = co.floor64(s64, dm, 1.0, top_k=k)
            assert torch.equal(floor, want) and torch.equal(count, co.count64(s64, dm, want)), (what, k)
            _assert_log_kept(lk, co.kept64(s64, dm, 1.0, want), (what, k))
        floor, count, lk, top = _typed(ops.score_cutoff(*args, drop_listed=drop, top_p=0.9, min_p=1e-3, top_k=V - 4), B)
        want = co.floor64(s64, dm, 1.0, top_k=V - 4, top_p=0.9, min_p=1e-3)
        dec = co.decided(s64, dm, 1.0, 0.9)
        print('exact mix', (B, V, d, C), what, '%d of %d decided, counts %d .. %d' % (int(dec.sum()), B, int(count.min()), int(count.max())))
        assert float(dec.double().mean()) >= 0.85
        assert torch.equal(floor[dec], want[dec]) and torch.equal(count[dec], co.count64(s64, dm, want)[dec]), what
        _assert_log_kept(lk, co.kept64(s64, dm, 1.0, floor), what)


# ------------------------------------------------------------------------------------------- d) eligibility
def test_eligibility_empty_session_fewer_rows_than_k_and_all_minus_inf(dev):
    ops = _ops()
    B, V, d = 5, 20, 32
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(4)
    perm = torch.stack([torch.randperm(V, generator=g)[:8] for _ in range(B)])
    listed = perm[:, :5]                                    # 5 listed and dropped
    bias = torch.zeros(B + 1, V)
    bias.scatter_(1, torch.cat([perm[:, 5:], perm[:1, 5:]]), NINF)   # 3 others out of the catalogue, per session
    bias[B] = NINF                                          # ... and a row without any item
    group = torch.arange(B)
    group[3] = B                                            # session 3: nothing eligible
    off = torch.zeros(1, B)
    off[0, 1] = NINF                                        # session 1: every eligible row scores -inf
    s64, dm = so.biased64(sr, E, cs, off, None, listed, True, bias, group)
    assert (~dm).sum(1).tolist() == [12, 12, 12, 0, 12]
    args = (sr.to(dev), E.to(dev), cs.to(dev), off.to(dev), None, listed.to(dev))
    kw = dict(drop_listed=True, bias=bias.to(dev), group=group.to(dev))
    for crit in (dict(top_k=5), dict(top_p=0.7), dict(min_p=0.3), dict(top_k=13), dict(top_k=5, top_p=0.7, min_p=0.3), dict()):
        floor, count, lk, top = _typed(ops.score_cutoff(*args, temperature=0.5, **crit, **kw), B)
        want = co.floor64(s64, dm, 0.5, **crit)
        assert [floor[3].item(), count[3].item(), lk[3].item(), top[3].item()] == [NINF, 0, NINF, NINF], crit
        assert [floor[1].item(), count[1].item(), lk[1].item(), top[1].item()] == [NINF, 12, 0.0, NINF], crit
        live = [0, 2, 4]
        assert torch.equal(floor[live], want[live]) and torch.equal(count[live], co.count64(s64, dm, want)[live]), crit
        _assert_log_kept(lk[live], co.kept64(s64, dm, 0.5, want)[live], crit)
        if crit == dict(top_k=13) or not crit:
            assert floor.tolist() == [NINF] * B and count.tolist() == [12, 12, 12, 0, 12] and lk[live].tolist() == [0.0] * 3


# ------------------------------------------------------------------------------------------- e) independence
def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _lockstep(parts):
    """drive several ops.cutoff_passes generators together: what they yield is combined (MAX / SUM) and written back INTO
    each part's own tensor, which is what the part then receives - an in-place all-reduce.  -> every part's result"""
    step = [next(p) for p in parts]
    while True:
        kinds = {k for k, _ in step}
        assert len(kinds) == 1
        ts = [t for _, t in step]
        total = torch.stack(ts).amax(0) if kinds == {'max'} else torch.stack(ts).sum(0)
        nxt = []
        for p, t in zip(parts, ts):
            t.copy_(total)
            try:
                nxt.append(p.send(t))
            except StopIteration as end:
                nxt.append(end.value)
        if not isinstance(nxt[0][0], str):
            return nxt
        step = nxt


def test_results_do_not_depend_on_shards_batches_or_views(dev):
    ops = _ops()
    B, V, d = 37, 1300, 64
    sr, E, cs = (t.to(dev) for t in co.random_inputs())
    g = torch.Generator().manual_seed(9)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)]).to(dev)
    bias = torch.randn(V, generator=g)
    bias[torch.rand(V, generator=g) < 0.3] = NINF
    bias = bias.to(dev)
    crit = dict(top_k=300, top_p=0.8, min_p=0.01, temperature=0.7)
    kw = dict(listed=listed, drop_listed=True, bias=bias)
    whole = ops.score_cutoff(sr, E, cs, **crit, **kw)
    assert _equal(whole, ops.score_cutoff(sr, E, cs, **crit, **kw)), 'a repeated call gives other bits'
    # row ranges through the pass-granular calls with a reduce that works IN PLACE, as an all-reduce does: every part gets its
    # own tensor back holding the combination over all parts.  Two ranges split in the middle of a 128-item chunk; then the
    # same with a third, EMPTY range (a shard without rows: it launches nothing and must give a neutral partial in every pass)
    n = 700 + 37
    for cuts in ((0, n, V), (0, n, V, V), (0, 0, n, V)):
        parts = [ops.cutoff_passes(sr, E[lo:hi], cs[lo:hi], id_lo=lo, listed=listed, drop_listed=True, bias=bias[lo:hi], **crit)
                 for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])].count(0) == len(cuts) - 3
        done = _lockstep(parts)
        for got in done:
            assert _equal(got, whole), ('row shards do not combine to the single-device bits', cuts)
    # one criterion at a time over the empty range as well (the searches keep separate state), and none (no search at all)
    for one in (dict(top_k=300), dict(top_p=0.8), dict(min_p=0.01), dict()):
        want = ops.score_cutoff(sr, E, cs, temperature=0.7, **one, **kw)
        parts = [ops.cutoff_passes(sr, E[lo:hi], cs[lo:hi], id_lo=lo, listed=listed, drop_listed=True, bias=bias[lo:hi],
                                   temperature=0.7, **one) for lo, hi in ((0, n), (n, V), (V, V))]
        for got in _lockstep(parts):
            assert _equal(got, want), ('with an empty shard', one)
    # an empty table alone: nothing eligible
    alone = ops.score_cutoff(sr, E[:0], cs[:0], reduce_max=lambda t: t, reduce_sum=lambda t: t, **crit)
    assert bool((alone[0] == NINF).all() & (alone[1] == 0).all() & (alone[2] == NINF).all() & (alone[3] == NINF).all())
    # the reduce callables of score_cutoff, identity: the pass-granular route on one device equals the chained entry
    same = ops.score_cutoff(sr, E, cs, reduce_max=lambda t: t, reduce_sum=lambda t: t, **crit, **kw)
    assert _equal(same, whole)
    # the sessions permuted: the permuted result; a session alone: its row
    perm = torch.randperm(B, generator=g).to(dev)
    got = ops.score_cutoff(sr[perm].contiguous(), E, cs, listed=listed[perm], drop_listed=True, bias=bias, **crit)
    assert _equal(got, [t[perm] for t in whole])
    for b in (0, 17, 36):
        one = ops.score_cutoff(sr[b:b + 1], E, cs, listed=listed[b:b + 1], drop_listed=True, bias=bias, **crit)
        assert _equal(one, [t[b:b + 1] for t in whole]), b
    # strided table and session views
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E
    sw = torch.full((B, d + 8), 7.0, device=dev)
    sw[:, :d] = sr
    assert _equal(ops.score_cutoff(sw[:, :d], Ew[:, :d], cs, **crit, **kw), whole)


# ------------------------------------------------------------------------------------------- f) the floor in select and sample
def test_floor_in_select_and_sample(dev):
    ops = _ops()
    B, V, d = 37, 1300, 64
    sr, E, cs = (t.to(dev) for t in co.exact_inputs(B, V, d))
    s64 = scores64(sr.cpu(), E.cpu(), cs.cpu())
    kw = dict(temperature=0.8, seed=11)
    # no floor, and a floor of -inf: today's calls, bit for bit
    for fl in (None, torch.full((B,), NINF, device=dev)):
        assert _equal(ops.score_select(sr, E, cs, 20, floor=fl), ops.score_select(sr, E, cs, 20))
        assert _equal(ops.score_sample(sr, E, cs, 20, floor=fl, **kw), ops.score_sample(sr, E, cs, 20, **kw))
    floor, count, _, _ = ops.score_cutoff(sr, E, cs, top_k=40, temperature=0.8)
    assert int(count.max()) <= 128 and int(count.min()) >= 40
    keep = s64 >= floor.cpu().double()[:, None]
    assert torch.equal(keep.sum(1), count.cpu().long())
    val, idx = ops.score_select(sr, E, cs, 128, floor=floor)
    key, ids = ops.score_sample(sr, E, cs, 128, floor=floor, **kw)
    want_v, want_i = [], []
    for b in range(B):
        n = int(count[b])
        assert bool((idx[b, n:] == -1).all()) and bool((ids[b, n:] == -1).all()) and bool((val[b, n:] == NINF).all()), b
        kept = keep[b].nonzero().flatten()
        assert torch.equal(ids[b, :n].long().sort().values.cpu(), kept), (b, 'the draw is not the kept set')
        order = torch.argsort(s64[b, kept], descending=True, stable=True)
        assert torch.equal(idx[b, :n].long().cpu(), kept[order]), (b, 'the selection is not the kept set in order')
        assert torch.equal(val[b, :n].cpu().double(), s64[b, kept[order]]), b
    key20, ids20 = ops.score_sample(sr, E, cs, 20, floor=floor, **kw)
    assert torch.equal(ids20, ids[:, :20]) and torch.equal(key20, key[:, :20])
    assert bool((s64.gather(1, ids20.cpu().long()) >= floor.cpu().double()[:, None]).all()), 'a draw below the floor'
    assert not torch.equal(ids20, ops.score_sample(sr, E, cs, 20, **kw)[1])


@pytest.mark.parametrize('crit', [dict(top_k=3), dict(top_p=0.7)])
def test_first_draw_follows_the_softmax_restricted_to_the_kept_items(dev, crit):
    """4096 copies of one session with exact scores (sample_oracle.stat_case(8): 6 eligible items).  The third and the fourth
    best of them TIE (-0.171875 twice), and the kept set is a function of a value alone, so no criterion keeps exactly 3: the
    sets a cutoff can keep hold 1, 2, 4, 5 or 6 items.  top_k = 3 and top_p = 0.7 both keep 4 - the tie at the boundary is
    inside - which leaves 3 degrees of freedom: the threshold is the 1 - 1e-4 quantile of chi-square at 3, 21.11."""
    ops = _ops()
    sr, E, bias = so.stat_case(8)
    T = 1.0
    p_all = so.stat_probs(8, T)
    s64, dm = so.biased64(sr[:1], E, None, None, None, None, False, bias, None)
    f64 = co.floor64(s64, dm, T, **crit)
    assert int(co.count64(s64, dm, f64)) == 4 and int((~dm).sum()) == 6, 'the cutoff of the statistical case does not keep 4 of 6'
    assert sorted({int(co.count64(s64, dm, co.floor64(s64, dm, T, top_k=k))) for k in range(1, 7)}) == [1, 2, 4, 5, 6]
    floor, count, lk, _ = ops.score_cutoff(sr.to(dev), E.to(dev), None, bias=bias.to(dev), temperature=T, **crit)
    assert count.tolist() == [4] * so.STAT_B and torch.equal(floor.cpu().double(), f64.expand(so.STAT_B))
    _, ids = ops.score_sample(sr.to(dev), E.to(dev), None, 1, bias=bias.to(dev), temperature=T, seed=so.STAT_SEED,
                              session_keys=torch.arange(so.STAT_B), floor=floor)
    kept = (s64[0] >= f64) & ~dm[0]
    p_kept = torch.where(kept, p_all, torch.zeros_like(p_all))
    p_kept = p_kept / p_kept.sum()
    assert abs(float(lk[0]) - float(torch.log(p_all[kept].sum()))) < 1e-5
    c = so.chi2_first(ids[:, 0], p_kept)                       # (asserts that nothing outside the kept set was drawn)
    print(crit, 'first-draw chi-square %.2f at 3 dof (< %.2f)' % (c, CHI2_3))
    assert c < CHI2_3
    assert so.chi2_first(ids[:, 0], p_all) > CHI2_3            # positive control: not the unrestricted soft-max


# ------------------------------------------------------------------------------------------- g) shards
def test_sharded_cutoff_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import os
    import torch.multiprocessing as mp
    from cutoff_gpu_worker import CRIT, NARROW, SMALL_CRITS, run_rank, small_case
    from sample_gpu_worker import K, SEED, T, session_keys
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

    def single(srs, crit, **more):
        lists = {k: v for k, v in more.items() if k in ('listed', 'drop_listed')}
        cut = ops.score_cutoff(srs, E, cs, **crit, **lists)
        return [t.cpu() for t in cut] + [t.cpu() for t in ops.score_sample(srs, E, cs, K, floor=cut[0], **kw, **more)]
    plain, narrow = single(sr, CRIT), single(sr, NARROW)
    keyed = single(sr, CRIT, listed=listed, drop_listed=True, session_keys=q)
    assert int(narrow[1].max()) < K and bool((narrow[5][:, -1] == -1).all()) and int(plain[1].min()) > 0
    n = B // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        for name, want in (('replicated', plain), ('replicated_narrow', narrow), ('replicated_drop_keys', keyed)):
            assert _equal(res[name], want), (r, name)
        mine = slice(r * n, (r + 1) * n)
        assert _equal(res['data_parallel'], [t[mine] for t in plain]), r
        want = single(sr[mine], NARROW, listed=listed[mine, :4 + r], drop_listed=True, session_keys=q[mine])
        assert _equal(res['data_parallel_drop_keys'], want), r
    # the table whose rows all live on rank 0: the rank without live rows joins every pass with a neutral partial
    sr2, E2, cs2 = [t.to(dev) for t in small_case()]
    n2 = sr2.shape[0] // world
    for i, crit in enumerate(SMALL_CRITS):
        cut = ops.score_cutoff(sr2, E2, cs2, temperature=T, **crit)
        want = [t.cpu() for t in cut] + [t.cpu() for t in ops.score_sample(sr2, E2, cs2, 20, floor=cut[0], **kw)]
        if crit:
            assert 0 < int(want[1].min()) and int(want[1].max()) < E2.shape[0], 'the criteria of the small case cut nothing'
        for r in range(world):
            res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
            assert res['small_n_live'] == (E2.shape[0], 0)[r]
            assert _equal(res['small', i], want), (r, crit)
            assert _equal(res['small_dp', i], [t[r * n2:(r + 1) * n2] for t in want]), (r, crit, 'data_parallel')


# ------------------------------------------------------------------------------------------- h) models
@pytest.mark.parametrize('name', ['srgnn_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_cutoff_and_truncated_sample_against_forward(dev, name):
    from test_rank_gpu import _fixture_model
    from test_sample_gpu import _seen
    from util import load_golden
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    B = labels.numel()
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    V = s64.shape[1]
    for T, p in ((1.0, 0.9), (0.5, 0.5)):
        floor, count, lk = model.cutoff(*inputs, top_p=p, temperature=T)
        assert floor.dtype == lk.dtype == torch.float32 and count.dtype == torch.int32 and floor.shape == count.shape == lk.shape == (B,)
        width = co.assert_top_p_consistent(floor, count, s64, None, T, p, what=(name, T, p))
        print(name, 'T %.1f p %.1f: nuclei of %d .. %d items, interval width max %d' % (T, p, int(count.min()), int(count.max()), int(width.max())))
    floor, count, lk = model.cutoff(*inputs, top_k=200)
    assert float((floor.cpu().double() - co.tau_k64(s64, None, 200)).abs().max()) < co.TOL_S
    assert bool(((count.cpu().long() - 200).abs() <= window_count(s64, 200, co.TOL_S)).all())
    assert not model.training
    # the truncated draw: values are score_items', and no id lies below the floor
    floor, count, lk = model.cutoff(*inputs, top_p=0.9)
    val, ids = model.sample(*inputs, k=20, seed=3, top_p=0.9)
    assert val.dtype == torch.float32 and ids.dtype == torch.int32 and val.shape == ids.shape == (B, 20)
    assert torch.equal(val, model.score_items(*inputs, items=ids))
    got = ids.cpu().long()
    filled = got >= 0
    assert torch.equal(filled.sum(1), count.cpu().long().clamp(max=20))
    assert bool((s64.gather(1, got.clamp(min=0)) >= floor.cpu().double()[:, None] - co.TOL_S)[filled].all()), 'a draw below the floor'
    assert not torch.equal(ids, model.sample(*inputs, k=20, seed=3)[1])
    # none of the three criteria: today's call, bit for bit
    a, b = model.sample(*inputs, k=20, seed=3, top_k=None, top_p=None, min_p=None), model.sample(*inputs, k=20, seed=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # with exclude_seen, a bias that filters, renormalised values, another temperature: consistent with log_mass
    seen = _seen(samples, V)
    gb = torch.Generator().manual_seed(V)
    bias = torch.randint(-8, 9, (V,), generator=gb).float() / 8
    bias[torch.rand(V, generator=gb) < 0.3] = NINF
    kw = dict(item_bias=bias.to(dev), exclude_seen=True)
    crit = dict(top_p=0.9, min_p=0.01, temperature=0.5)
    f_ren, c_ren, l_ren = model.cutoff(*inputs, renormalize=True, **crit, **kw)
    mass = model.log_mass(*inputs, **kw)
    off = seen | (bias == NINF)[None]
    sb = s64 + bias.double()[None]
    val, ids = model.sample(*inputs, k=20, seed=3, renormalize=True, **crit, **kw)
    assert torch.equal(val, model.score_items(*inputs, items=ids, renormalize=True, **kw))
    got = ids.cpu().long()
    filled = got >= 0
    assert not bool(off.gather(1, got.clamp(min=0))[filled].any()), 'an ineligible item was drawn'
    err = (val.cpu().double() - (sb - mass.cpu().double()[:, None]).gather(1, got.clamp(min=0)))[filled].abs().max()
    assert float(err) < 2e-4
    assert bool((val >= f_ren[:, None] - 1e-4)[filled.to(dev)].all()), 'a renormalised value below the renormalised floor'
    # the nucleus of the filtered distribution against forward() + bias in float64, raw and renormalised (top_p alone)
    f_p, c_p, _ = model.cutoff(*inputs, top_p=0.9, temperature=0.5, **kw)
    co.assert_top_p_consistent(f_p, c_p, sb, off, 0.5, 0.9, what=name + ' filtered')
    f_p, c_p, _ = model.cutoff(*inputs, top_p=0.9, temperature=0.5, renormalize=True, **kw)
    co.assert_top_p_consistent(f_p, c_p, sb - mass.cpu().double()[:, None], off, 0.5, 0.9, what=name + ' filtered, renormalised')
    # the training flag comes back, and bad arguments raise before the model runs
    model.train()
    model.sample(*inputs, k=2, top_k=5)
    model.cutoff(*inputs, top_k=5)
    assert model.training
    ran = []
    orig = model.session_repr
    model.session_repr = lambda *a, **k: ran.append(1) or orig(*a, **k)
    try:
        for bad in (dict(top_p=0.0), dict(top_p=float('nan')), dict(top_k=0), dict(min_p=1.5)):
            with pytest.raises(ValueError, match='^sample: '):
                model.sample(*inputs, k=2, **bad)
            with pytest.raises(ValueError, match='^cutoff: '):
                model.cutoff(*inputs, **bad)
        assert not ran and model.training
    finally:
        del model.session_repr
        model.eval()


# ------------------------------------------------------------------------------------------- i) memory
def test_truncated_mixture_sample_allocates_no_score_matrix(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, K = 37484, 64, 64, 3
    torch.manual_seed(3)
    model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
    (mg,), _ = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 5))
    mg = mg.to(dev)
    model.sample(mg, k=100, seed=1, top_p=0.9)           # workspaces and column scales are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = model.sample(mg, k=100, seed=1, top_p=0.9)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.2f MB, one (B, V) fp32 matrix %.2f MB' % (rise / 2 ** 20, B * V * 4 / 2 ** 20))
    assert rise < B * V * 4, rise
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    # the route it replaces: forward(), sort, cumsum - several such matrices: the measure bites
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        s = model(mg)
        sv, _ = s.sort(dim=1, descending=True)
        nucleus = torch.softmax(sv, 1).cumsum(1) < 0.9
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > B * V * 4
    floor, count, _ = model.cutoff(mg, top_p=0.9)
    co.assert_top_p_consistent(floor, count, s.double().cpu(), None, 1.0, 0.9, what='V = 37484 mixture')
    assert int((count.cpu() - 1 - nucleus.sum(1).cpu()).abs().max()) <= 16
    assert bool((s.gather(1, idx.long()) >= floor[:, None] - 1e-4).all())


# ------------------------------------------------------------------------------------------- j) launcher
def test_recommend_launcher_truncated_sample_equals_in_process_for_any_batching(dev, tmp_path):
    import os
    import subprocess
    import sys
    from util import GOLDEN, ROOT
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
                            '--sample-top-p', '0.9', '--sample-top-k', '50', '--batch-size', str(bs), '--output', str(out)],
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        texts.append(out.read_text())
    lines = texts[0].splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    inputs = [x.to(dev) for x in inputs]
    val, idx = model.sample(*inputs, k=10, temperature=0.7, seed=5, session_keys=torch.arange(len(sessions)), top_p=0.9, top_k=50)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == [i for i in idx[b].tolist() if i >= 0], b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
    assert texts[1] == texts[0]
    assert not torch.equal(idx, model.sample(*inputs, k=10, temperature=0.7, seed=5, session_keys=torch.arange(len(sessions)))[1])
