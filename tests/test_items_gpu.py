"""Scoring given items on the GPU: csrc/score_items.hip through ops.score_items, dist.VocabParallel.score_items,
model.score_items / model.rerank and src/scripts/rerank.py, against materialised float64 scores (tests/items_oracle.py).

Exact inputs (every product and sum representable) must give EQUAL values - a lost column group, a slot scored by the wrong
lane group, a chunk boundary and the padding / foreign / dropped slots show there.  Random inputs and the models are held
to 1e-4, the fp32 bound tests/test_rank_gpu.py and tests/test_select_gpu.py use for this score."""
import os
import subprocess
import sys

import pytest
import torch

from items_oracle import drop_mask, exact_case, items64, order64, scores64
from test_select_gpu import NAMES, _random_case
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4
INF = float('inf')


def _ops():
    return pkg('ops')


def _equal(out, ref, what):
    out = out.cpu()
    assert out.dtype == torch.float32 and out.shape == ref.shape, (what, out.dtype, out.shape, ref.shape)
    bad = out.double() != ref
    assert not bool(bad.any()), '%s: %d slots differ, first at %s: got %s, expected %s' % (
        what, int(bad.sum()), bad.nonzero()[0].tolist(), out[bad][:6].tolist(), ref[bad][:6].tolist())


def _close(out, ref, what):
    """|out - ref| < TOL on the finite slots; the +-inf slots equal"""
    out = out.cpu().double()
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(out[~fin], ref[~fin]), (what, 'the infinite slots differ')
    err = float((out[fin] - ref[fin]).abs().max()) if bool(fin.any()) else 0.0
    print(what, 'max |out - oracle| %.2e over %d finite slots, %d infinite' % (err, int(fin.sum()), int((~fin).sum())))
    assert err < TOL, (what, err)


# ------------------------------------------------------------------------------------------- 1) exact inputs
def _lists(B, V, M, seed, every=False):
    g = torch.Generator().manual_seed(seed)
    items = torch.randint(0, V, (B, M), generator=g)
    if every:                           # in EVERY list: ids 0 and V - 1, a repeated id, -1 slots
        items[:, 0], items[:, 1], items[:, 2], items[:, 3] = 0, V - 1, -1, items[:, 4]
        items[:, M - 1] = -1
    return items


@pytest.mark.parametrize('B,V,d,M', [(1, 20, 32, 1), (3, 20, 32, 45), (5, 300, 100, 7), (33, 5000, 96, 257), (2, 37484, 256, 1000)])
def test_exact_inputs_give_equal_values(dev, B, V, d, M):
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    items = _lists(B, V, M, B + M, every=M == 45)
    if M == 45:
        assert all(len(set(r)) < M and {0, V - 1, -1} <= set(r) for r in items.tolist())
    for scale in (cs, None):
        s64 = scores64(sr, E, scale)
        t = lambda x: None if x is None else x.to(dev)
        out = ops.score_items(sr.to(dev), E.to(dev), t(scale), items.to(dev))
        print('exact', (B, V, d, M), 'cs' if scale is not None else 'no cs', out[0, :6].tolist())
        _equal(out, items64(s64, items), 'exact %s' % ((B, V, d, M),))
        if M in (45, 257):              # one list for all sessions, and another integer dtype
            out = ops.score_items(sr.to(dev), E.to(dev), t(scale), items[B - 1].to(torch.int32).to(dev))
            _equal(out, items64(s64, items[B - 1]), 'shared list %s' % ((B, V, d, M),))


# ------------------------------------------------------------------------------------------- 2) every kernel path, mixtures
@pytest.mark.parametrize('B,V,d,C', [(37, 700, 100, 2), (4, 600, 1024, 4), (33, 500, 512, 2)])
def test_exact_mixture_inputs_on_every_kernel_path(dev, B, V, d, C):
    """the construction of tests/test_select_gpu.py: a d that is no power of two of float4 lanes, one, two and four column
    groups per lane, C = 2 and C = 4; session b's component b % C carries an offset that is a multiple of 1/8 and the
    others -1e5 (exp() of them is exactly 0 in fp32 and in float64), so the mixture is exact and the values must be EQUAL -
    without a list, with a scored and with a dropped one"""
    ops = _ops()
    M = 130
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
    items = _lists(B, V, M, d + C, every=True)
    items[:, 10:14] = listed[:, :4]                     # the session's listed ids are among its candidates
    t = lambda x: None if x is None else x.to(dev)
    for what, lst, oi, drop in (('plain', None, None, False), ('score', listed, off_in, False), ('drop', listed, off_in, True)):
        out = ops.score_items(srs.to(dev), E.to(dev), cs.to(dev), items.to(dev), off.to(dev), t(oi), t(lst), drop_listed=drop)
        if drop:
            ref = items64(scores64(srs, E, cs, off), items, 0, drop_mask(listed, V))
            assert bool((ref[:, 10:14] == -INF).all())
        else:
            ref = items64(scores64(srs, E, cs, off, oi, lst), items)
        print('exact mix', (B, V, d, C), what, out[0, 8:14].tolist(), ref[0, 8:14].tolist())
        _equal(out, ref, 'mixture %s %s' % ((B, V, d, C), what))
        if what == 'score':      # the listed items' offsets matter: scored as "ex" the values differ
            assert not torch.equal(items64(scores64(srs, E, cs, off), items), ref)


# ------------------------------------------------------------------------------------------- 3) random inputs
@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed-score', 'listed-drop'])
@pytest.mark.parametrize('B,V,d', [(33, 5000, 96), (40, 3429, 64)])
def test_random_inputs_within_roundoff(dev, B, V, d, kind):
    ops = _ops()
    M = 200
    srs, E, cs, off_ex, off_in, listed = _random_case(B, V, d, kind)
    g = torch.Generator().manual_seed(M + B)
    items = torch.randint(0, V, (B, M), generator=g)
    if listed is not None:              # half of every list from the session's listed ids (-1 among them: padding slots)
        items[:, ::2] = listed.gather(1, torch.randint(0, listed.shape[1], (B, M // 2), generator=g))
    drop = kind == 'listed-drop'
    t = lambda x: None if x is None else x.to(dev)
    out = ops.score_items([s.to(dev) for s in srs], t(E), t(cs), t(items), t(off_ex), t(off_in), t(listed), drop_listed=drop)
    if drop:
        ref = items64(scores64(srs, E, cs, off_ex), items, 0, drop_mask(listed, V))
    else:
        ref = items64(scores64(srs, E, cs, off_ex, off_in, listed), items)
    _close(out, ref, '%s %s' % (kind, (B, V, d)))
    if listed is not None:
        assert int((ref == -INF).sum()) > B             # padding slots (and dropped ones) are there
    if kind == 'listed-score':          # the listed items' offsets matter: the "ex" scores are further off than TOL
        ex = items64(scores64(srs, E, cs, off_ex), items)
        fin = torch.isfinite(ex)
        assert float((out.cpu().double()[fin] - ex[fin]).abs().max()) > 100 * TOL


# ------------------------------------------------------------------------------------------- 4) views
def test_strided_table_and_session_views(dev):
    ops = _ops()
    B, V, d, M = 33, 1000, 96, 77
    srs, E, cs, _, _, _ = _random_case(B, V, d, 'single')
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E.to(dev)
    sw = torch.full((B, d + 8), 7.0, device=dev)
    sw[:, :d] = srs[0].to(dev)
    tv, sv = Ew[:, :d], sw[:, :d]
    assert tv.stride(0) == d + 32 and sv.stride(0) == d + 8 and not tv.is_contiguous()
    items = _lists(B, V, M, 4, every=True).to(dev)
    wide = torch.full((B, M + 3), -5, device=dev, dtype=torch.int64)     # (a view of the ids is copied by the host: -5 never arrives)
    wide[:, :M] = items
    o1 = ops.score_items(sv, tv, cs.to(dev), wide[:, :M])
    o0 = ops.score_items(sv.contiguous(), tv.contiguous(), cs.to(dev), items)
    assert torch.equal(o1, o0)
    _close(o1, items64(scores64(srs, E, cs), items), 'strided')


# ------------------------------------------------------------------------------------------- 5) shard contract, one process
def test_two_row_ranges_sum_to_the_whole_table_result(dev):
    ops = _ops()
    B, V, d, M = 33, 5000, 96, 150
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(7)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    items = _lists(B, V, M, 5, every=True)
    items[:, 10:16] = listed
    items[:, 20], items[:, 21] = 2499, 2500
    s64 = scores64(sr, E, cs)
    sr, E, cs, listed_d, items_d = sr.to(dev), E.to(dev), cs.to(dev), listed.to(dev), items.to(dev)
    for kw in (dict(), dict(listed=listed_d, drop_listed=True)):
        whole = ops.score_items(sr, E, cs, items_d, **kw)
        lo = ops.score_items(sr, E[:2500], cs[:2500], items_d, id_lo=0, **kw)
        hi = ops.score_items(sr, E[2500:], cs[2500:], items_d, id_lo=2500, **kw)
        own_lo = ((items >= 0) & (items < 2500))
        assert bool((lo.cpu()[(items >= 2500)] == 0).all()) and bool((hi.cpu()[own_lo] == 0).all())
        assert bool((lo.cpu()[items < 0] == -INF).all()) and bool((hi.cpu()[items < 0] == -INF).all())
        assert torch.equal(lo + hi, whole)
        _equal(whole, items64(s64, items, 0, drop_mask(listed, V) if kw else None), 'whole table')
        if kw:
            assert bool((whole[:, 10:16] == -INF).all())


# ------------------------------------------------------------------------------------------- 6) sharded, W = 2 on one GPU
def test_sharded_score_items_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from items_gpu_worker import candidates, run_rank
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
    items = candidates().to(dev)
    V = E.shape[0]
    plain = ops.score_items(sr, E, cs, items).cpu()
    shared = ops.score_items(sr, E, cs, items[0]).cpu()
    dropped = ops.score_items(sr, E, cs, items, listed=listed, drop_listed=True).cpu()
    _equal(dropped, items64(scores64(sr, E, cs), items, 0, drop_mask(listed, V)), 'single device')
    assert int((dropped == -INF).sum()) > int((plain == -INF).sum()) >= 2 * sr.shape[0]
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        # every rank feeds the same sessions: the full answer on every rank
        for key, want in (('replicated', plain), ('routed', plain), ('replicated_shared', shared), ('replicated_drop', dropped)):
            assert res[key].dtype == torch.float32 and torch.equal(res[key], want), (r, key)
        # every rank feeds its own slice, with its own list width: its own sessions' scores
        mine = slice(r * n, (r + 1) * n)
        want = ops.score_items(sr[mine], E, cs, items[mine], listed=listed[mine, :4 + r], drop_listed=True).cpu()
        assert torch.equal(res['data_parallel_drop'], want), r


# ------------------------------------------------------------------------------------------- 7) models against fixtures
def _model_candidates(samples, labels, V, seed):
    """int64 [B, M]: 50 random ids, the label, the session's own items, a -1 - rows padded with -1 to one width"""
    g = torch.Generator().manual_seed(seed)
    rows = [torch.randint(0, V, (50,), generator=g).tolist() + [int(lab)] + sorted(set(seq)) + [-1]
            for (seq, _), lab in zip(samples, labels.tolist())]
    M = max(len(r) for r in rows)
    return torch.tensor([r + [-1] * (M - len(r)) for r in rows])


def _seen_slots(samples, items):
    """bool [B, M]: the slot names an item of its session"""
    return torch.tensor([[i in set(seq) for i in row] for (seq, _), row in zip(samples, items.tolist())])


@pytest.mark.parametrize('name', NAMES)
def test_model_score_items_and_rerank_against_fixture(dev, name):
    from test_rank_gpu import _fixture_model
    from util import load_golden
    z, model, inputs, labels = _fixture_model(name, dev)
    samples = load_golden(name)[1]
    head = torch.from_numpy(z['eval_logprobs_head']).double()           # the reference's own log-probabilities
    H, V = head.shape
    items = _model_candidates(samples, labels, V, len(name))
    out = model.score_items(*inputs, items=items.to(dev))
    assert out.dtype == torch.float32 and out.shape == items.shape and not model.training
    _close(out[:H], items64(head, items[:H]), name + ' vs reference log-probs')
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    _close(out, items64(s64, items), name + ' vs forward()')
    assert bool((out.cpu()[items < 0] == -INF).all()) and bool(torch.isfinite(out.cpu()[items >= 0]).all())
    # exclude_seen: -inf exactly at the session's own items, everything else as before (no renormalisation)
    seen = _seen_slots(samples, items)
    assert bool(seen.any(1).all())
    ex = model.score_items(*inputs, items=items.to(dev), exclude_seen=True).cpu()
    assert torch.equal(ex == -INF, seen | (items < 0)), name
    assert torch.equal(ex[~seen], out.cpu()[~seen]), name
    # rerank: the same values in the order (value descending, id ascending), -inf slots last with id -1
    for kw in (dict(), dict(k=20), dict(exclude_seen=True, k=30)):
        val, idx = model.rerank(*inputs, items=items.to(dev), **kw)
        rv, ri = order64(ex if kw.get('exclude_seen') else out, items, kw.get('k'))
        assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == ri.shape, (name, kw)
        assert torch.equal(idx.cpu().long(), ri) and torch.equal(val.cpu().double(), rv), (name, kw)
    assert not model.training


# ------------------------------------------------------------------------------------------- 8) range check
def test_model_score_items_refuses_ids_out_of_range_before_anything_runs(dev, monkeypatch):
    sp = pkg()
    V = 50
    model = sp.SRGNN(V, 32, 1).to(dev).train()

    def never(*a, **k):
        raise AssertionError('the encoder ran although an id is out of range')
    monkeypatch.setattr(model, 'session_repr', never)
    monkeypatch.setattr(_ops(), 'score_items', never)
    for items, shown in ((torch.tensor([[1, V], [2, 3]]), str(V)), (torch.tensor([0, -2]), '-2'), (torch.tensor([[V + 7]], dtype=torch.int32), str(V + 7))):
        with pytest.raises(ValueError, match=r'score_items: item id %s; ids are in \[0, 50\)' % shown):
            model.score_items(None, items=items.to(dev))
        with pytest.raises(ValueError, match='score_items: item id'):
            model.rerank(None, items=items.to(dev), k=3)
    assert model.training                               # nothing ran, nothing was switched


# ------------------------------------------------------------------------------------------- 9) no (B, V) allocation
def test_mixture_score_items_allocates_no_score_matrix(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, K, M = 37484, 64, 64, 3, 500
    torch.manual_seed(3)
    model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
    (mg,), _ = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 5))
    mg = mg.to(dev)
    items = torch.randint(0, V, (B, M), generator=torch.Generator().manual_seed(9)).to(dev)
    model.score_items(mg, items=items)                   # workspaces and column scales are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = model.score_items(mg, items=items)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.2f MB, one (B, V) fp32 matrix %.2f MB' % (rise / 2 ** 20, B * V * 4 / 2 ** 20))
    assert rise < B * V * 4, rise
    # the same answer through forward(): more than one such matrix - the measure bites
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        ref = model(mg).gather(1, items)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > B * V * 4
    _close(out, ref.double().cpu(), 'V = 37484 mixture')


# ------------------------------------------------------------------------------------------- 10) launcher
def test_rerank_launcher_equals_in_process_rerank(dev, tmp_path):
    sp, col = pkg(), pkg('collate')
    sys.path.insert(0, os.path.join(ROOT, 'src', 'scripts'))
    try:
        import recommend as rec
        import rerank as rr
    finally:
        sys.path.pop(0)
    data = os.path.join(ROOT, 'datasets', 'sample')
    V = int(open(os.path.join(data, 'num_items.txt')).readline())
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    sessions = rec.read_session_file(os.path.join(GOLDEN, 'sample_test.txt'))[:40]
    g = torch.Generator().manual_seed(10)
    cands = [torch.randint(0, V, (140 + 13 * (b % 7),), generator=g).tolist() + s[:2] for b, s in enumerate(sessions)]   # ragged
    assert len({len(c) for c in cands}) > 3 and max(len(c) for c in cands) > 128
    (tmp_path / 'sessions.txt').write_text(rec.format_sessions(sessions))
    (tmp_path / 'cands.txt').write_text(rec.format_sessions(cands))
    out = tmp_path / 'ranked.txt'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'rerank.py'), '--model', 'SRGNN', '--dataset-dir', data,
                        '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--sessions',
                        str(tmp_path / 'sessions.txt'), '--candidates', str(tmp_path / 'cands.txt'), '--exclude-seen',
                        '--output', str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.rerank(*[x.to(dev) for x in inputs], items=torch.tensor(rr.pad_candidates(cands)).to(dev), exclude_seen=True)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        n = len(ids)
        assert n == sum(c not in set(sessions[b]) for c in cands[b]) and n > 128, b
        assert ids == idx[b, :n].tolist() and bool((idx[b, n:] == -1).all()), b
        assert not set(ids) & set(sessions[b]), b
        assert max(abs(a - c) for a, c in zip(vals, val[b, :n].tolist())) <= 1e-6, b
