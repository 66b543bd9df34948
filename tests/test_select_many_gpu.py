"""Top-N lists beyond 128 items on the GPU: csrc/select_many.hip through ops.score_select_many, model.recommend_many and the
candidates.py launcher, against the float64 restatement of the selection contract (tests/select_oracle.py) over the score
oracles.  Where the scores are exact in fp32 the lists must be the oracle's own; elsewhere they must be consistent with
scores known to TOL.  Everything is deterministic, so bits are compared across calls, shards, views and with the selection
kernel of csrc/recommend.hip where both apply."""
import os
import subprocess
import sys

import pytest
import torch

from sample_oracle import biased64
from select_oracle import assert_list_consistent, drop_mask, exact_case, merge_lists, scores64, select64
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # the project's tolerance for served log-probabilities (tests/test_select_gpu.py)
NINF = float('-inf')
MAXK = 4096


def _ops():
    return pkg('ops')


def _t(x, dev):
    return None if x is None else x.to(dev)


def _equal(val, idx, ref, what):
    rv, ri = ref
    val, idx = val.cpu(), idx.cpu()
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == rv.shape == idx.shape, what
    bad = (idx.long() != ri).any(1) | (val.double() != rv).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. ids %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], idx[bad][0].tolist()[:12], ri[bad][0].tolist()[:12])


def _collected(ops, k, srs, E, cs, **kw):
    """(count of score_cutoff(top_k=k), n of the collect pass under its floor) - the two numbers the route relies on being equal"""
    score = pkg('score')
    floor, count, _, _ = ops.score_cutoff(srs, E, cs, top_k=k, **kw)
    a = score._served_args('test', srs, E, cs, kw.get('off_ex'), kw.get('off_in'), kw.get('listed'), kw.get('drop_listed', False),
                           kw.get('id_lo', 0), kw.get('bias'), kw.get('group'))
    n = score._collect_many(a, floor, int(count.max()))[2].clone()
    return count.cpu(), n.cpu()


# ------------------------------------------------------------------------------------------- 1) exact inputs
@pytest.mark.parametrize('B,V,d', [(3, 20, 32), (5, 300, 32), (33, 5000, 96)])
def test_exact_inputs_give_equal_lists(dev, B, V, d):
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    for scale in (cs, None):
        s64 = scores64(sr, E, scale)
        es = E if scale is None else E * scale[:, None]
        assert torch.equal((sr @ es.t()).double(), s64), 'the fp32 scores of the exact case are not exact'
        for k in sorted({min(k, MAXK) for k in (1, 128, 129, 257, V - 1, V, V + 5)}):
            val, idx = ops.score_select_many(sr.to(dev), E.to(dev), _t(scale, dev), k)
            _equal(val, idx, select64(s64, k), 'exact %s k=%d %s' % ((B, V, d), k, 'cs' if scale is not None else 'no cs'))


# ------------------------------------------------------------------------------------------- 2) a tie that cuts the list
def test_a_tie_at_the_kth_takes_the_lowest_ids(dev):
    ops = _ops()
    B, V, d, k = 5, 600, 32, 200
    g = torch.Generator().manual_seed(2)
    base = torch.randint(-8, 9, (4, d), generator=g).float() / 8
    sr = torch.randint(-8, 9, (B, d), generator=g).float() / 8
    E = base[torch.arange(V) % 4]
    s64 = scores64(sr, E, None)
    levels = [s64[b].unique().numel() for b in range(B)]
    assert min(levels) == 4, 'the four base rows do not score apart for every session: %s' % levels
    val, idx = ops.score_select_many(sr.to(dev), E.to(dev), None, k)
    _equal(val, idx, select64(s64, k), 'tie at the k-th')
    count, n = _collected(ops, k, sr.to(dev), E.to(dev), None)
    assert torch.equal(n, count) and count.tolist() == [300] * B          # two whole levels: the k-th lies inside the second


# ------------------------------------------------------------------------------------------- 3) tie overflow
def test_tie_overflow_orders_with_torch_and_equals_the_order_kernel(dev):
    ops = _ops()
    B, d, k = 2, 8, 500
    sr = torch.full((B, d), 0.5)
    got = {}
    for V in (9000, 8000):          # 9000 pairs per session do not fit the order kernel's 8192; 8000 do
        E = torch.full((V, d), 0.25)
        count, n = _collected(ops, k, sr.to(dev), E.to(dev), None)
        assert n.tolist() == count.tolist() == [V] * B
        val, idx = ops.score_select_many(sr.to(dev), E.to(dev), None, k)
        assert val.dtype == torch.float32 and idx.dtype == torch.int32
        assert torch.equal(idx.cpu().long(), torch.arange(k)[None].expand(B, k)), V
        assert bool((val == 1.0).all()), V
        got[V] = (val.cpu(), idx.cpu())
    assert torch.equal(got[9000][0], got[8000][0]) and torch.equal(got[9000][1], got[8000][1])


# ------------------------------------------------------------------------------------------- 4) / 5) random fp32 inputs
def _random_case(C, mode):
    """B = 70: two full session tiles and a partial one.  The offsets are finite and the bias is either finite or -inf (which
    makes the pair ineligible), so NO eligible pair scores -inf - the corner in which score_select_many follows
    score_cutoff's counting and is not compared with score_select."""
    B, V, d, L = 70, 2500, 256, 20
    g = torch.Generator().manual_seed(70 + C + len(mode))
    srs = torch.randn(C, B, d, generator=g) * 0.3
    E = torch.randn(V, d, generator=g) * 0.2
    cs = torch.rand(V, generator=g) + 0.5
    off_ex = off_in = listed = None
    if C > 1:
        off_ex = -2.0 * torch.rand(C, B, generator=g)
        off_in = off_ex + torch.rand(C, B, generator=g) * 3 - 1.0
        listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])
        listed[torch.rand(B, L, generator=g) < 0.2] = -1
    bias = torch.randn(4, V, generator=g)
    bias[torch.rand(4, V, generator=g) < 0.2] = NINF
    group = torch.randint(0, 4, (B,), generator=g)
    drop = mode == 'drop'
    return srs, E, cs, off_ex, None if drop else off_in, listed, drop, bias, group


RANDOM = [(1, 'plain'), (3, 'score'), (3, 'drop')]


@pytest.mark.parametrize('C,mode', RANDOM)
def test_random_inputs_lists_consistent_with_roundoff(dev, C, mode):
    ops = _ops()
    k = 1000
    srs, E, cs, off_ex, off_in, listed, drop, bias, group = _random_case(C, mode)
    s64, dm = biased64(srs, E, cs, off_ex, off_in, listed, drop, bias, group)
    assert int((~dm).sum(1).min()) > k and not bool(torch.isinf(s64[~dm]).any())
    args = ([s.to(dev) for s in srs], E.to(dev), cs.to(dev), k, _t(off_ex, dev), _t(off_in, dev), _t(listed, dev))
    kw = dict(drop_listed=drop, bias=bias.to(dev), group=group.to(dev))
    val, idx = ops.score_select_many(*args, **kw)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (70, k)
    assert_list_consistent(val, idx, s64, TOL, dm, what='random C=%d %s' % (C, mode))
    again = ops.score_select_many(*args, **kw)
    assert torch.equal(again[0], val) and torch.equal(again[1], idx), 'a repeated call gives other bits'
    count, n = _collected(ops, k, args[0], args[1], args[2], off_ex=args[4], off_in=args[5], listed=args[6], **kw)
    assert torch.equal(n, count) and int(count.min()) >= k


@pytest.mark.parametrize('C,mode', RANDOM)
def test_short_lists_equal_the_selection_kernel(dev, C, mode):
    """no eligible pair of _random_case scores -inf (see there), so the two kernels answer the same question"""
    ops = _ops()
    srs, E, cs, off_ex, off_in, listed, drop, bias, group = _random_case(C, mode)
    args = lambda k: ([s.to(dev) for s in srs], E.to(dev), cs.to(dev), k, _t(off_ex, dev), _t(off_in, dev), _t(listed, dev))
    kw = dict(drop_listed=drop, bias=bias.to(dev), group=group.to(dev))
    for k in (1, 20, 128):
        val, idx = ops.score_select_many(*args(k), **kw)
        v0, i0 = ops.score_select(*args(k), **kw)
        assert torch.equal(val, v0) and torch.equal(idx, i0), (C, mode, k)


# ------------------------------------------------------------------------------------------- 6) fewer eligible than k
def test_fewer_eligible_rows_than_k(dev):
    ops = _ops()
    B, V, d, k = 5, 300, 32, 300
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(6)
    allow = torch.randperm(V, generator=g)[:50]
    bias = ops.catalog_bias(V, allow=allow)
    listed = allow[None, :50].expand(B, 50).clone()
    listed[:4] = -1                                         # session 4: every allowed item is listed and dropped
    s64 = scores64(sr, E, cs) + bias.double()[None]
    dm = (bias == NINF)[None].expand(B, V) | drop_mask(listed, V)
    assert (~dm).sum(1).tolist() == [50, 50, 50, 50, 0]
    val, idx = ops.score_select_many(sr.to(dev), E.to(dev), cs.to(dev), k, listed=listed.to(dev), drop_listed=True, bias=bias.to(dev))
    _equal(val, idx, select64(s64, k, dm), 'an allow-list of 50, k = 300')
    assert bool((idx[:4, :50] >= 0).all()) and bool((idx[:, 50:] == -1).all()) and bool((val[:, 50:] == NINF).all())
    assert bool((idx[4] == -1).all()) and bool((val[4] == NINF).all())
    # nothing eligible in ANY session: no collect pass at all
    val, idx = ops.score_select_many(sr.to(dev), E.to(dev), cs.to(dev), k, bias=torch.full((V,), NINF, device=dev))
    assert bool((idx == -1).all()) and bool((val == NINF).all()) and val.shape == (B, k)


# ------------------------------------------------------------------------------------------- 7) row shards on one device
def test_two_row_ranges_merge_to_the_whole_table_result(dev):
    ops = _ops()
    k = 1000
    srs, E, cs, off_ex, off_in, listed, drop, bias, group = _random_case(3, 'drop')
    V, n = E.shape[0], 1200 + 37                            # the cut lies inside a 128-item chunk
    srs = [s.to(dev) for s in srs]
    E, cs, off_ex, listed, bias, group = (t.to(dev) for t in (E, cs, off_ex, listed, bias, group))
    kw = dict(off_ex=off_ex, listed=listed, drop_listed=True, group=group)
    whole = ops.score_select_many(srs, E, cs, k, bias=bias, **kw)
    floor, count, _, _ = ops.score_cutoff(srs, E, cs, top_k=k, bias=bias, **kw)
    cap = int(count.max())
    parts = [ops.score_select_many(srs, E[lo:hi], cs[lo:hi], k, id_lo=lo, bias=bias[:, lo:hi], floor=floor, cap=cap, **kw)
             for lo, hi in ((0, n), (n, V))]
    assert int(parts[0][1].max()) < n and int(parts[1][1][parts[1][1] >= 0].min()) >= n
    assert any(-1 in row for row in parts[0][1].tolist()), 'no shard list is cut by the floor'
    mv, mi = merge_lists([p[0] for p in parts], [p[1] for p in parts], k)
    assert torch.equal(mi, whole[1].cpu().long()) and torch.equal(mv, whole[0].cpu().double())
    # strided table and session views
    d = E.shape[1]
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E
    sw = [torch.full((s.shape[0], d + 8), 7.0, device=dev) for s in srs]
    for w, s in zip(sw, srs):
        w[:, :d] = s
    tv = Ew[:, :d]
    assert tv.stride(0) == d + 32 and not tv.is_contiguous()
    got = ops.score_select_many([w[:, :d] for w in sw], tv, cs, k, bias=bias, **kw)
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    one = ops.score_select_many(sw[0][:, :d], tv, cs, k)
    ref = ops.score_select_many(srs[0], E, cs, k)
    assert sw[0][:, :d].stride(0) == d + 8 and torch.equal(one[0], ref[0]) and torch.equal(one[1], ref[1])


# ------------------------------------------------------------------------------------------- 8) models
@pytest.mark.parametrize('name', ['srgnn_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_recommend_many_against_forward_and_recommend(dev, name):
    from test_rank_gpu import _fixture_model
    from test_select_gpu import _seen
    from util import load_golden
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    B = labels.numel()
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    V = s64.shape[1]
    gb = torch.Generator().manual_seed(V)
    bias = torch.randint(-8, 9, (V,), generator=gb).float() / 8
    bias[torch.rand(V, generator=gb) < 0.3] = NINF
    off = _seen(samples, V) | (bias == NINF)[None]
    sb = s64 + bias.double()[None]
    kw = dict(exclude_seen=True, item_bias=bias.to(dev))
    mass = model.log_mass(*inputs, **kw).cpu().double()
    for ren in (False, True):
        val, idx = model.recommend_many(*inputs, k=500, renormalize=ren, **kw)
        assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (B, 500)
        assert not model.training
        assert_list_consistent(val, idx, sb - mass[:, None] if ren else sb, TOL, off, what='%s renormalize=%s' % (name, ren))
        v128, i128 = model.recommend(*inputs, k=128, renormalize=ren, **kw)
        assert torch.equal(val[:, :128], v128) and torch.equal(idx[:, :128], i128), (name, ren)
    a, b = model.recommend_many(*inputs, k=64), model.recommend(*inputs, k=64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    model.train()
    model.recommend_many(*inputs, k=200)
    assert model.training
    model.eval()


# ------------------------------------------------------------------------------------------- 9) launchers
def test_candidates_launcher_feeds_rerank(dev, tmp_path):
    sp = pkg()
    scripts = os.path.join(ROOT, 'src', 'scripts')
    sys.path.insert(0, scripts)
    try:
        import recommend as rec
    finally:
        sys.path.remove(scripts)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    sessions = rec.read_session_file(os.path.join(GOLDEN, 'sample_test.txt'))[:40]
    (tmp_path / 'sessions.txt').write_text(rec.format_sessions(sessions))
    common = ['--model', 'SRGNN', '--dataset-dir', data, '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt),
              '--sessions', str(tmp_path / 'sessions.txt'), '--exclude-seen']

    def run(script, *more):
        r = subprocess.run([sys.executable, os.path.join(scripts, script)] + common + list(more), capture_output=True, text=True,
                           timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
    run('candidates.py', '--top', '300', '--output', str(tmp_path / 'pairs.txt'))
    run('candidates.py', '--top', '300', '--ids-only', '--batch-size', '16', '--output', str(tmp_path / 'cands.txt'))
    run('rerank.py', '--candidates', str(tmp_path / 'cands.txt'), '--output', str(tmp_path / 'reranked.txt'))
    pairs = [rec.parse_line(ln) for ln in (tmp_path / 'pairs.txt').read_text().splitlines()]
    cands = rec.read_session_file(str(tmp_path / 'cands.txt'))
    reranked = [rec.parse_line(ln) for ln in (tmp_path / 'reranked.txt').read_text().splitlines()]
    assert len(pairs) == len(cands) == len(reranked) == len(sessions)
    for b, ((ids, vals), c, (rids, rvals)) in enumerate(zip(pairs, cands, reranked)):
        assert len(ids) == 300 and len(set(ids)) == 300 and not set(ids) & set(sessions[b]), b
        assert c == ids and rids == ids, b
        assert max(abs(x - y) for x, y in zip(vals, rvals)) <= TOL, b
