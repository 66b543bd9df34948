"""Top-N serving on the GPU: csrc/recommend.hip through ops.score_select, dist.VocabParallel.select, model.recommend and
src/scripts/recommend.py, against materialised float64 scores (tests/select_oracle.py).

Exact inputs (every product and sum representable) must give EQUAL lists - lost tail tiles, a candidate list that
overflows, the tie direction and the tail rule show there.  Random inputs and the models are checked by what every list
consistent with scores known to +-1e-4 (the fp32 bound of tests/test_rank_gpu.py) must satisfy."""
import os
import subprocess
import sys

import pytest
import torch

from select_oracle import assert_list_consistent, drop_mask, exact_case, merge_lists, scores64, select64, window_count
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ops():
    return pkg('ops')


def _equal(val, idx, ref, what):
    rv, ri = ref
    val, idx = val.cpu(), idx.cpu()
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == rv.shape == idx.shape, what
    bad = (idx.cpu().long() != ri).any(1) | (val.cpu().double() != rv).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. ids %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], idx[bad][0].tolist()[:12], ri[bad][0].tolist()[:12])


# ------------------------------------------------------------------------------------------- 1) exact inputs
@pytest.mark.parametrize('B,V,d,K', [(3, 20, 32, 20), (5, 300, 32, 1), (5, 300, 32, 32), (33, 5000, 96, 33), (33, 5000, 96, 128),
                                     (64, 37484, 256, 100)])
def test_exact_inputs_give_equal_lists(dev, B, V, d, K):
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    for scale in (cs, None):
        val, idx = ops.score_select(sr.to(dev), E.to(dev), None if scale is None else scale.to(dev), K)
        ref = select64(scores64(sr, E, scale), K)
        print('exact', (B, V, d, K), 'cs' if scale is not None else 'no cs', idx[0].tolist()[:8], ref[1][0].tolist()[:8])
        _equal(val, idx, ref, 'exact %s' % ((B, V, d, K),))


# ------------------------------------------------------------------------------------------- 2) adversarial score orders
@pytest.mark.parametrize('K', [1, 31, 128])
@pytest.mark.parametrize('order', ['rising', 'falling', 'tied'])
def test_adversarial_score_orders(dev, order, K):
    """rising scores: every item of every chunk beats the running K-th best, so every chunk fills its candidate list;
    all-tied: nothing after the first K items may enter."""
    ops = _ops()
    B, V, d = 33, 3000, 32
    sr = torch.zeros(B, d)
    sr[:, 0] = 1.0
    E = torch.zeros(V, d)
    v = torch.arange(V).float()
    E[:, 0] = {'rising': v / 8, 'falling': (V - 1 - v) / 8, 'tied': torch.full((V,), 0.5)}[order]
    E[:, 1] = 1.0                                         # (orthogonal to the sessions: no part of the score)
    val, idx = ops.score_select(sr.to(dev), E.to(dev), None, K)
    j = torch.arange(K)
    ids = (V - 1 - j) if order == 'rising' else j
    vals = torch.full((K,), 0.5, dtype=torch.float64) if order == 'tied' else (V - 1 - j).double() / 8
    _equal(val, idx, (vals[None].expand(B, K), ids[None].expand(B, K)), '%s K=%d' % (order, K))


# ------------------------------------------------------------------------------------------- 3) every kernel path, mixtures
@pytest.mark.parametrize('B,V,d,C', [(37, 700, 100, 2), (40, 600, 512, 4), (33, 500, 1024, 2)])
def test_exact_mixture_inputs_on_every_kernel_path(dev, B, V, d, C):
    """a d that is no multiple of the 32-column group, C = 2 and C = 4, session tiles read through the cache; session b's
    component b % C carries an offset that is a multiple of 1/8 and the others -1e5 (exp() of them is exactly 0 in fp32 and
    in float64), so the mixture is exact and the lists must be EQUAL - without a list, with a scored and with a dropped one"""
    ops = _ops()
    K = 40
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
    t = lambda x: None if x is None else x.to(dev)
    for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
        val, idx = ops.score_select(srs.to(dev), E.to(dev), cs.to(dev), K, off.to(dev), t(oi), t(lst), drop_listed=drop)
        if drop:
            ref = select64(scores64(srs, E, cs, off), K, drop_mask(listed, V))
        else:
            ref = select64(scores64(srs, E, cs, off, oi, lst), K)
        print('exact mix', (B, V, d, C), what, idx[0].tolist()[:8], ref[1][0].tolist()[:8])
        _equal(val, idx, ref, 'mixture %s %s' % ((B, V, d, C), what))
        if what == 'score':      # the listed items' offsets matter: scored as "ex" the lists differ
            assert not torch.equal(select64(scores64(srs, E, cs, off), K)[1], ref[1])


# ------------------------------------------------------------------------------------------- 4) fewer eligible than K
def test_fewer_eligible_rows_than_k(dev):
    ops = _ops()
    B, V, d, K = 5, 20, 32, 20
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(4)
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    val, idx = ops.score_select(sr.to(dev), E.to(dev), cs.to(dev), K, listed=listed.to(dev), drop_listed=True)
    ref = select64(scores64(sr, E, cs), K, drop_mask(listed, V))
    _equal(val, idx, ref, 'V = 20, 5 dropped')
    assert bool((idx[:, 15:] == -1).all()) and bool((val[:, 15:] == float('-inf')).all()) and bool((idx[:, :15] >= 0).all())
    # K > V without a list: V entries, then the tail
    val, idx = ops.score_select(sr.to(dev), E.to(dev), cs.to(dev), 28)
    _equal(val, idx, select64(scores64(sr, E, cs), 28), 'K = 28 > V = 20')


# ------------------------------------------------------------------------------------------- 5) random inputs
def _random_case(B, V, d, kind):
    """drawn as tests/test_rank_gpu._random_case (labels are not needed here)"""
    g = torch.Generator().manual_seed(B + V + len(kind))
    C = 1 if kind == 'single' else 3
    srs = torch.randn(C, B, d, generator=g) * 0.3
    E = torch.randn(V, d, generator=g) * 0.2
    cs = torch.rand(V, generator=g) + 0.5
    off_ex = off_in = listed = None
    if kind != 'single':
        off_ex = -2.0 * torch.rand(C, B, generator=g)
    if kind.startswith('listed'):
        L = 7
        off_in = off_ex + torch.rand(C, B, generator=g) * 3 - 1.0
        listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])       # distinct ids per session
        listed[torch.rand(B, L, generator=g) < 0.25] = -1
    return srs, E, cs, off_ex, off_in, listed


@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed-score', 'listed-drop'])
@pytest.mark.parametrize('B,V,d', [(33, 5000, 96), (40, 3429, 64)])
def test_random_inputs_lists_consistent_with_roundoff(dev, B, V, d, kind):
    ops = _ops()
    K = 50
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    drop = kind == 'listed-drop'
    g = lambda t: None if t is None else t.to(dev)
    val, idx = ops.score_select([s.to(dev) for s in srs], g(E), g(cs), K, g(off_ex), g(off_in), g(listed), drop_listed=drop)
    if drop:
        s64, dm = scores64(srs, E, cs, off_ex), drop_mask(listed, V)
    else:
        s64, dm = scores64(srs, E, cs, off_ex, off_in, listed), None
    near = window_count(s64, K, TOL, dm)
    print(kind, (B, V, d), 'items within 2 TOL of the K-th best: max %d, mean %.2f' % (int(near.max()), float(near.float().mean())))
    assert int(near.max()) <= 4, 'the round-off window holds %d items: the check is vacuous for this draw' % int(near.max())
    assert_list_consistent(val, idx, s64, TOL, dm, what='%s %s' % (kind, (B, V, d)))
    if kind == 'listed-score':   # the listed items' offsets matter: as "ex" scores some list is inconsistent
        with pytest.raises(AssertionError):
            assert_list_consistent(val, idx, scores64(srs, E, cs, off_ex), TOL, None, what='ex only')


# ------------------------------------------------------------------------------------------- 6) views
def test_strided_table_and_session_views(dev):
    ops = _ops()
    B, V, d, K = 33, 1000, 96, 50
    srs, E, cs, _, _, _ = _random_case(B, V, d, 'single')
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E.to(dev)
    sw = torch.full((B, d + 8), 7.0, device=dev)
    sw[:, :d] = srs[0].to(dev)
    tv, sv = Ew[:, :d], sw[:, :d]
    assert tv.stride(0) == d + 32 and sv.stride(0) == d + 8 and not tv.is_contiguous()
    v1, i1 = ops.score_select(sv, tv, cs.to(dev), K)
    v0, i0 = ops.score_select(sv.contiguous(), tv.contiguous(), cs.to(dev), K)
    assert torch.equal(v1, v0) and torch.equal(i1, i0)
    assert_list_consistent(v1, i1, scores64(srs, E, cs), TOL, what='strided')


# ------------------------------------------------------------------------------------------- 7) shard contract, one process
def test_two_row_ranges_merge_to_the_whole_table_result(dev):
    ops = _ops()
    B, V, d, K = 33, 5000, 96, 50
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(7)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    sr, E, cs, listed = sr.to(dev), E.to(dev), cs.to(dev), listed.to(dev)
    for kw in (dict(), dict(listed=listed, drop_listed=True)):
        whole = ops.score_select(sr, E, cs, K, **kw)
        lo = ops.score_select(sr, E[:2500], cs[:2500], K, id_lo=0, **kw)
        hi = ops.score_select(sr, E[2500:], cs[2500:], K, id_lo=2500, **kw)
        assert int(hi[1].min()) >= 2500 and int(lo[1].max()) < 2500
        mv, mi = merge_lists([lo[0], hi[0]], [lo[1], hi[1]], K)
        assert torch.equal(mi, whole[1].cpu().long()) and torch.equal(mv, whole[0].cpu().double())
        ref = select64(scores64(sr, E, cs), K, drop_mask(listed, V) if kw else None)
        _equal(whole[0], whole[1], ref, 'whole table')


# ------------------------------------------------------------------------------------------- 8) sharded, W = 2 on one GPU
def test_sharded_select_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from select_gpu_worker import K, run_rank, sharded_case
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
    V = E.shape[0]
    plain = [t.cpu() for t in ops.score_select(sr, E, cs, K)]
    dropped = [t.cpu() for t in ops.score_select(sr, E, cs, K, listed=listed, drop_listed=True)]
    _equal(dropped[0], dropped[1], select64(scores64(sr, E, cs), K, drop_mask(listed, V)), 'single device')
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        # every rank feeds the same sessions: the full answer on every rank
        for got, want in ((res['replicated'], plain), (res['replicated_drop'], dropped)):
            assert got[1].dtype == torch.int32 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), r
        # every rank feeds its own slice, with its own list width: its own sessions' lists
        mine = slice(r * n, (r + 1) * n)
        want = [t.cpu() for t in ops.score_select(sr[mine], E, cs, K, listed=listed[mine, :4 + r], drop_listed=True)]
        got = res['data_parallel_drop']
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), r


# ------------------------------------------------------------------------------------------- 9) models against fixtures
NAMES = ['srgnn_s32', 'niser_s32', 'lessr_L1_s32', 'lessr_L3_s32', 'msgifsr_K1_s32', 'msgifsr_K3_s32', 'msgifsr_K3_fus_s32',
         'msgifsr_K3_ext_s32', 'msgifsr_K3_ext_fus_s32', 'msgifsr_K1_edge', 'msgifsr_K3_edge', 'msgifsr_K3_fus_edge',
         'msgifsr_K3_ext_edge', 'msgifsr_K3_ext_fus_edge']


def _seen(samples, V):
    """bool [B, V]: the items of every session"""
    m = torch.zeros(len(samples), V, dtype=torch.bool)
    for b, (seq, _) in enumerate(samples):
        m[b, torch.tensor(seq)] = True
    return m


@pytest.mark.parametrize('name', NAMES)
def test_model_recommend_against_fixture(dev, name):
    from test_rank_gpu import _fixture_model
    z, model, inputs, labels = _fixture_model(name, dev)
    head = torch.from_numpy(z['eval_logprobs_head']).double()           # the reference's own log-probabilities
    val, idx = model.recommend(*inputs, k=20)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (labels.numel(), 20)
    assert not model.training
    H = head.shape[0]
    print(name, 'ids', idx[0].tolist()[:8], 'window', window_count(head, 20, TOL).tolist()[:8])
    assert_list_consistent(val[:H], idx[:H], head, TOL, what=name + ' vs reference log-probs')
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    err = float((val.cpu().double() - s64.gather(1, idx.cpu().long())).abs().max())
    print(name, 'max |value - forward()| %.2e' % err)
    assert err < TOL
    assert_list_consistent(val, idx, s64, TOL, what=name + ' vs forward()')


# ------------------------------------------------------------------------------------------- 10) exclude_seen
@pytest.mark.parametrize('name', ['srgnn_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_recommend_exclude_seen(dev, name):
    from test_rank_gpu import _fixture_model
    from util import load_golden
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    head = torch.from_numpy(z['eval_logprobs_head']).double()
    seen = _seen(samples, head.shape[1])
    val, idx = model.recommend(*inputs, k=20, exclude_seen=True)
    assert not bool(seen.gather(1, idx.cpu().long()).any()), 'an item of the session itself was returned'
    H = head.shape[0]
    # no renormalisation: the remaining items keep forward()'s log-probabilities
    assert_list_consistent(val[:H], idx[:H], head, TOL, seen[:H], what=name + ' exclude_seen vs reference log-probs')
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    assert_list_consistent(val, idx, s64, TOL, seen, what=name + ' exclude_seen vs forward()')


# ------------------------------------------------------------------------------------------- 11) no (B, V) allocation
def test_mixture_recommend_allocates_no_score_matrix(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, K = 37484, 64, 64, 3
    torch.manual_seed(3)
    model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
    (mg,), _ = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 5))
    mg = mg.to(dev)
    model.recommend(mg, k=100)                           # workspaces and column scales are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = model.recommend(mg, k=100)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.2f MB, one (B, V) fp32 matrix %.2f MB' % (rise / 2 ** 20, B * V * 4 / 2 ** 20))
    assert rise < B * V * 4, rise
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    # the same answer through forward(): more than one such matrix - the measure bites
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        s = model(mg)
        tv, ti = s.topk(100)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > B * V * 4
    assert_list_consistent(val, idx, s.double().cpu(), TOL, what='V = 37484 mixture')


# ------------------------------------------------------------------------------------------- 12) launcher
def test_recommend_launcher_equals_in_process_recommend(dev, tmp_path):
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
    out = tmp_path / 'top.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'recommend.py'), '--model', 'SRGNN', '--dataset-dir', data,
                        '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--sessions',
                        str(tmp_path / 'sessions.txt'), '--top', '50', '--exclude-seen', '--output', str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.recommend(*[x.to(dev) for x in inputs], k=50, exclude_seen=True)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == idx[b].tolist(), b
        assert not set(ids) & set(sessions[b]), b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b


# ------------------------------------------------------------------------------------------- workspace cache of the three users
def test_topk_rank_select_interleaved_at_two_shapes_keep_their_own_scratch(dev):
    """score_topk, score_rank and score_select draw their byte scratch from one cache keyed (kind, device, size): shape A,
    shape B, then A again must repeat A's results bit for bit, and - random fp32 inputs, no ties - select must name the
    items top-K names"""
    ops = _ops()
    g = torch.Generator().manual_seed(11)

    def case(B, V, d):
        return (torch.randn(B, d, generator=g).to(dev), torch.randn(V, d, generator=g).to(dev),
                torch.randint(0, V, (B,), generator=g).to(dev))

    def run(sr, E, labels):
        tv, ti = ops.score_topk(sr, E, None, 5)
        rank, target = ops.score_rank(sr, E, None, labels)
        sv, si = ops.score_select(sr, E, None, 5)
        assert torch.equal(si, ti), (si[0].tolist(), ti[0].tolist())
        return tv, ti, rank, target, sv, si
    a, b = case(3, 300, 32), case(130, 1000, 64)
    first = run(*a)
    run(*b)
    again = run(*a)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    kinds = sorted({k[0] for k in pkg('score')._BYTE_WS})
    assert kinds == ['rank', 'select', 'topk'], kinds
