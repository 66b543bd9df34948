"""Diversified top-N on the GPU: csrc/diversify.hip through ops.diversify, dist.VocabParallel.diversify,
model.recommend_diverse / list_diversity and src/scripts/recommend.py, against the float64 greedy of tests/diversify_oracle.py.

Inputs with a wide margin at every step (margin_case: the picks must be EQUAL), theta = 0, unfilled / out-of-range slots and
zero rows, random inputs judged pick by pick given the kernel's own prefix, views and batch independence (bit for bit), the
four model families against their own recommend(), peak memory, two ranks on one GPU, and the launcher."""
import os
import subprocess
import sys

import pytest
import torch

import diversify_oracle as do
from test_diversify_cpu import MARGIN_SHAPES, margin_inputs
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4                  # fp32 bound of a cosine / a score (tests/test_rank_gpu.py, tests/test_select_gpu.py): tol = theta * TOL
NINF = float('-inf')


def _ops():
    return pkg('ops')


def _gathered(ops, rows, s, k, theta, dev, row=None):
    """ops.diversify over rows [B, M, d] laid out as a [B M, d] row source (row = arange unless given)"""
    B, M, d = rows.shape
    row = torch.arange(B * M).view(B, M) if row is None else row
    return ops.diversify(rows.reshape(B * M, d).to(dev), row.to(dev), s.to(dev), k, theta)


def _check_outputs(out, ref, s, what):
    """picks EQUAL, val the pool's own bits at the picks (-inf in the tail), mmr and ild within 1e-5 of float64"""
    val, pick, mmr, ild = [t.cpu() for t in out]
    assert val.dtype == mmr.dtype == ild.dtype == torch.float32 and pick.dtype == torch.int32, what
    assert pick.shape == val.shape == mmr.shape == ref['pick'].shape and ild.shape == (pick.shape[0],), what
    bad = (pick.long() != ref['pick']).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. picks %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], pick[bad][0].tolist()[:16], ref['pick'][bad][0].tolist()[:16])
    want = torch.where(pick < 0, torch.full_like(val, NINF), s.gather(1, pick.clamp(min=0).long()))
    assert torch.equal(val, want), '%s: val is not s[pick] bit for bit' % what
    tail = pick < 0
    assert bool((mmr[tail] == NINF).all()), what
    err_m = float((mmr.double() - ref['mmr'])[~tail].abs().max()) if bool((~tail).any()) else 0.0
    err_i = float((ild.double() - ref['ild']).abs().max())
    print(what, 'max |mmr - f64| %.2e, max |ild - f64| %.2e' % (err_m, err_i))
    assert err_m <= 1e-5 and err_i <= 1e-5, (what, err_m, err_i)


# ------------------------------------------------------------------------------------------- 1) margin cases: EQUAL picks
@pytest.mark.parametrize('B,M,d,K', MARGIN_SHAPES)
def test_margin_cases_give_equal_picks(dev, B, M, d, K):
    """rows in LDS (128 x 256, 37 x 100, 64 x 32), rows through the cache (128 x 1024), d no multiple of 32, M no multiple
    of the wavefront, K = M.  The three facts that make the comparison bite are asserted here as well."""
    rows, s = margin_inputs(B, M, d)
    ref = do.greedy64(rows, s, 0.5, K)
    sim = do.sims64(rows)
    assert float(ref['margin'].min()) == 2.0 ** -10
    assert bool((ref['pick'] != torch.arange(K)[None]).any(1).all())
    assert bool((sim * 4 == (sim * 4).round()).all())
    out = _gathered(_ops(), rows, s, K, 0.5, dev)
    _check_outputs(out, ref, s, 'margin %s' % ((B, M, d, K),))
    if K < M and d <= 256:        # a strict rise of the diversity over the first K slots
        plain = _gathered(_ops(), rows[:, :K].contiguous(), s[:, :K].contiguous(), K, 0.0, dev)[3]
        assert float(out[3].mean()) > float(plain.mean()) + 0.01


# ------------------------------------------------------------------------------------------- 2) theta = 0
def test_theta_zero_is_slot_order_whatever_the_rows_are(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    B, M, d, K = 9, 70, 64, 33
    rows = torch.randn(B, M, d, generator=g)
    rows[0, 3] = float('inf')                          # (the rows are not looked at for the order)
    s = torch.full((B, M), -1.25)
    row = torch.arange(B * M).view(B, M)
    row[:, [0, 4, 5, 40]] = -1
    val, pick, mmr, ild = [t.cpu() for t in _gathered(ops, rows, s, K, 0.0, dev, row)]
    want = torch.tensor([i for i in range(M) if i not in (0, 4, 5, 40)][:K])
    assert torch.equal(pick.long(), want[None].expand(B, K))
    assert torch.equal(val, torch.full((B, K), -1.25)) and torch.equal(mmr, val)
    # descending values (a pool of recommend()): the first K filled slots again, val bit-equal
    s2 = torch.sort(torch.randn(B, M, generator=g), 1, descending=True).values
    val, pick, _, _ = [t.cpu() for t in _gathered(ops, rows, s2, K, 0.0, dev, row)]
    assert torch.equal(pick.long(), want[None].expand(B, K)) and torch.equal(val, s2[:, want])


# ------------------------------------------------------------------------------------------- 3) unfilled / out-of-range / zero rows
@pytest.mark.parametrize('B', [1, 33])
def test_unfilled_and_out_of_range_slots_and_zero_rows(dev, B):
    """unfilled slots in the middle and at the end, K above the filled count: a (-1, -inf) tail.  Row indices >= n_rows
    (checked=True: the caller vouches, the kernel's own contract) are unfilled slots too - the buffer is valid, nothing is
    read out of bounds.  A zero row has similarity 0 and no NaN.  Margin inputs: the picks must be EQUAL."""
    ops = _ops()
    M, d, K = 48, 32, 44
    rows, s = do.margin_case(B, M, d, seed=70 + B)
    rows[:, 6] = 0.0
    rows[:, 20] = 0.0
    n = B * M
    row = torch.arange(n).view(B, M).clone()
    filled = torch.ones(B, M, dtype=torch.bool)
    for sl, r in ((3, -1), (17, -7), (18, n), (19, 2 ** 31 - 1), (45, -1), (46, n + 5), (47, -1)):
        row[:, sl] = r
        filled[:, sl] = False
    ref = do.greedy64(rows, s, 0.5, K, filled)
    assert float(ref['margin'].min()) >= 2.0 ** -10 and bool((ref['pick'][:, 41:] == -1).all()) and bool((ref['pick'][:, :41] >= 0).all())
    X = rows.reshape(n, d).to(dev)
    with pytest.raises(ValueError):
        ops.diversify(X, row.to(dev), s.to(dev), K, 0.5)                    # the default looks at the rows first
    out = ops.diversify(X, row.to(dev), s.to(dev), K, 0.5, checked=True)
    _check_outputs(out, ref, s, 'unfilled B=%d' % B)
    assert not bool(torch.isnan(out[2]).any()) and not bool(torch.isnan(out[3]).any())
    # nothing filled at all: every slot (-1, -inf), diversity 0; one filled slot: diversity 0
    none = torch.full((B, M), -1)
    val, pick, mmr, ild = [t.cpu() for t in ops.diversify(X, none.to(dev), s.to(dev), 5, 0.5)]
    assert bool((pick == -1).all()) and bool((val == NINF).all()) and bool((mmr == NINF).all()) and bool((ild == 0).all())
    none[:, 9] = 9
    val, pick, _, ild = [t.cpu() for t in ops.diversify(X, none.to(dev), s.to(dev), 5, 0.5)]
    assert pick[:, 0].tolist() == [9] * B and bool((pick[:, 1:] == -1).all()) and bool((ild == 0).all())
    assert torch.equal(val[:, 0], s[:, 9])


# ------------------------------------------------------------------------------------------- 4) random inputs
def _random_case(B, M, d):
    """rows around a few directions per session (cosines from -0.3 to 0.95), values like log-probabilities"""
    g = torch.Generator().manual_seed(B + M + d)
    centres = torch.randn(B, 9, d, generator=g)
    rows = centres[torch.arange(B)[:, None], torch.randint(0, 9, (B, M), generator=g)] + 0.6 * torch.randn(B, M, d, generator=g)
    rows = rows * (0.1 + torch.rand(B, M, 1, generator=g))               # norms differ: the similarity must not care
    s = -3.0 * torch.rand(B, M, generator=g) - 2.0
    return rows, s


@pytest.mark.parametrize('theta', [0.3, 2.0])
@pytest.mark.parametrize('B,M,d', [(33, 128, 96), (40, 50, 64)])
def test_random_inputs_every_pick_is_greedy_given_its_prefix(dev, B, M, d, theta):
    rows, s = _random_case(B, M, d)
    K = 40
    val, pick, mmr, ild = [t.cpu() for t in _gathered(_ops(), rows, s, K, theta, dev)]
    near = do.assert_greedy_consistent(pick, rows, s, theta, theta * TOL, what='random %s theta %.1f' % ((B, M, d), theta))
    print('random', (B, M, d), theta, 'slots within 2 tol of the best: at most %d' % near, 'ild', ild[:4].tolist())
    assert torch.equal(val, s.gather(1, pick.long()))
    assert float((ild.double() - do.ild64(rows, pick)).abs().max()) <= 1e-5
    # the penalty matters: the same picks are NOT greedy for another theta
    with pytest.raises(AssertionError):
        do.assert_greedy_consistent(pick, rows, s, 3 * theta + 1, theta * TOL, max_near=M)


# ------------------------------------------------------------------------------------------- 5) views and batching
def test_views_table_mode_and_batch_independence_bit_for_bit(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(8)
    for V, d, B, M, K in ((700, 96, 33, 128, 30), (300, 1024, 3, 128, 20)):       # rows in LDS; rows through the cache
        E = (torch.randn(40, d, generator=g)[torch.randint(0, 40, (V,), generator=g)] + 0.5 * torch.randn(V, d, generator=g)).to(dev)
        row = torch.stack([torch.randperm(V, generator=g)[:M] for _ in range(B)])
        row[:, 7] = -1
        s = torch.sort(torch.randn(B, M, generator=g), 1, descending=True).values.to(dev)
        base = ops.diversify(E, row.to(dev), s, K, 0.8)
        # a strided table view
        Ew = torch.full((V, d + 32), 7.0, device=dev)
        Ew[:, :d] = E
        view = Ew[:, :d]
        assert view.stride(0) == d + 32 and not view.is_contiguous()
        # gathered rows with row = arange; any integer dtype for row
        gathered = E[row.clamp(min=0).to(dev)].reshape(B * M, d)
        arange = torch.where(row < 0, torch.full_like(row, -1), torch.arange(B * M).view(B, M))
        for what, got in (('strided view', ops.diversify(view, row.to(dev), s, K, 0.8)),
                          ('gathered rows', ops.diversify(gathered, arange.to(dev), s, K, 0.8)),
                          ('int32 rows', ops.diversify(E, row.to(torch.int32).to(dev), s, K, 0.8)),
                          ('int16 rows', ops.diversify(E, row.to(torch.int16).to(dev), s, K, 0.8))):
            for a, b in zip(base, got):
                assert torch.equal(a, b), (what, V, d)
        # session b alone is row b of the batch
        for b in (0, B - 1):
            alone = ops.diversify(E, row[b:b + 1].to(dev), s[b:b + 1], K, 0.8)
            for x, y in zip(base, alone):
                assert torch.equal(x[b:b + 1], y), (b, V, d)
        assert bool((base[1] != torch.arange(K, device=dev)[None]).any())     # (something was re-ranked)


# ------------------------------------------------------------------------------------------- 6) models
_MODELS = {}


def _model(name, dev):
    if name not in _MODELS:
        from test_rank_gpu import _fixture_model
        _MODELS[name] = _fixture_model(name, dev)
    return _MODELS[name]


def _slots_of(ids, pool_ids):
    """slot in the pool of every returned id (ids are distinct within a pool), -1 for an unfilled slot"""
    hit = ids[:, :, None] == pool_ids[:, None, :]
    assert bool((hit.sum(2) == (ids >= 0).long()).all())
    return torch.where(ids >= 0, hit.int().argmax(2), torch.full_like(ids, -1, dtype=torch.long))


@pytest.mark.parametrize('name', ['srgnn_s32', 'niser_s32', 'lessr_L1_s32', 'msgifsr_K3_ext_fus_s32'])
def test_model_recommend_diverse_against_its_own_pool(dev, name):
    from util import load_golden
    z, model, inputs, labels = _model(name, dev)
    B = labels.numel()
    pv, pi = model.recommend(*inputs, k=40)
    # diversity 0: the first 10 columns of the pool, bit for bit
    v0, i0 = model.recommend_diverse(*inputs, k=10, pool=40, diversity=0)
    assert v0.dtype == torch.float32 and i0.dtype == torch.int32 and v0.shape == i0.shape == (B, 10) and not model.training
    assert torch.equal(v0, pv[:, :10]) and torch.equal(i0, pi[:, :10])
    # diversity 1: greedy given its prefix against the pool's own values and the table rows in float64; the pool's values
    v1, i1 = model.recommend_diverse(*inputs, k=10, pool=40, diversity=1.0)
    pool_ids = pi.cpu().long()
    table = model._table().detach().double().cpu()
    rows = table[pool_ids.clamp(min=0)]
    slots = _slots_of(i1.cpu().long(), pool_ids)
    near = do.assert_greedy_consistent(slots, rows, pv.cpu(), 1.0, TOL, filled=pool_ids >= 0, what=name)
    assert torch.equal(v1.cpu(), pv.cpu().gather(1, slots.clamp(min=0)))
    # exclude_seen never returns a session item
    samples = load_golden(name)[1]
    vs, isn = model.recommend_diverse(*inputs, k=10, pool=40, diversity=1.0, exclude_seen=True)
    for b, (seq, _) in enumerate(samples):
        assert not set(isn[b].tolist()) & set(seq), b
    ps = model.recommend(*inputs, k=40, exclude_seen=True)
    assert torch.equal(model.recommend_diverse(*inputs, k=10, pool=40, diversity=0, exclude_seen=True)[1], ps[1][:, :10])
    # list_diversity against float64, and the diversified list is no less diverse than the plain top 10
    ld1, ld0 = model.list_diversity(i1), model.list_diversity(pi[:, :10])
    assert ld1.dtype == torch.float32 and ld1.shape == (B,)
    for ids, ld in ((i1, ld1), (pi[:, :10], ld0)):
        idc = ids.cpu().long()
        want = do.ild64(table[idc.clamp(min=0)], torch.where(idc >= 0, torch.arange(10)[None].expand_as(idc), torch.full_like(idc, -1)))
        assert float((ld.cpu().double() - want).abs().max()) <= 1e-5
    print(name, 'near-ties at most %d; mean diversity plain %.4f, diversified %.4f' % (near, float(ld0.mean()), float(ld1.mean())))
    assert float(ld1.mean()) >= float(ld0.mean()) - 1e-5


# ------------------------------------------------------------------------------------------- 7) no big intermediate
def test_recommend_diverse_allocates_no_gathered_rows(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, M = 37484, 64, 64, 128
    torch.manual_seed(3)
    model = sp.SRGNN(V, d, 1).to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)(synth_samples(B, V, 5))
    inputs = [x.to(dev) for x in inputs]
    model.recommend_diverse(*inputs, k=20, pool=M)           # workspaces are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = model.recommend_diverse(*inputs, k=20, pool=M)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.3f MB, one [B, M, d] fp32 tensor %.3f MB' % (rise / 2 ** 20, B * M * d * 4 / 2 ** 20))
    assert rise < B * M * d * 4, rise
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    # the composition in PyTorch on the same pool: more than one such tensor - the measure bites
    pv, pi = model.recommend(*inputs, k=M)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        x = torch.nn.functional.normalize(model._table()[pi.long()], dim=-1)
        sim = torch.bmm(x, x.transpose(1, 2))
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > B * M * d * 4
    assert sim.shape == (B, M, M)
    slots = _slots_of(idx.cpu().long(), pi.cpu().long())                    # every returned id is one of the pool's
    assert torch.equal(val.cpu(), pv.cpu().gather(1, slots))


# ------------------------------------------------------------------------------------------- 8) sharded, W = 2 on one GPU
def test_sharded_diversify_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from diversify_gpu_worker import K, POOL, THETA, run_rank, sharded_case
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
    sr, E = [t.to(dev) for t in sharded_case()]
    pv, pi = ops.score_select(sr, E, None, POOL)
    want = [t.cpu() for t in ops.diversify(E, pi, pv, K, THETA)]
    assert bool((want[1] != torch.arange(K)[None]).any(1).float().mean() > 0.5)      # most sessions are re-ranked
    ids = pi.cpu().long()
    assert bool((ids < 2560).any()) and bool((ids >= 2560).any())                    # the pools span both shards
    ld = ops.diversify(E, pi[:, :K].contiguous(), torch.zeros_like(pv[:, :K]), K, 0.0)[3].cpu()
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        assert torch.equal(res['pool'][0], pv.cpu()) and torch.equal(res['pool'][1], pi.cpu())
        for got, w in zip(res['replicated'], want):
            assert got.dtype == w.dtype and torch.equal(got, w), r
        for got, w in zip(res['data_parallel'], want):
            assert torch.equal(got, w[r * n:(r + 1) * n]), r
        assert torch.equal(res['list_diversity'], ld), r


# ------------------------------------------------------------------------------------------- 9) launcher
def test_recommend_launcher_diversity_equals_in_process_recommend_diverse(dev, tmp_path):
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
                        str(tmp_path / 'sessions.txt'), '--top', '10', '--diversity', '0.5', '--pool', '40', '--exclude-seen',
                        '--output', str(out)],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    assert len(lines) == len(sessions)
    model = model.to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)([(s, 0) for s in sessions])
    val, idx = model.recommend_diverse(*[x.to(dev) for x in inputs], k=10, diversity=0.5, pool=40, exclude_seen=True)
    for b, line in enumerate(lines):
        ids, vals = rec.parse_line(line)
        assert ids == idx[b].tolist(), b
        assert not set(ids) & set(sessions[b]), b
        assert max(abs(a - c) for a, c in zip(vals, val[b].tolist())) <= 1e-6, b
