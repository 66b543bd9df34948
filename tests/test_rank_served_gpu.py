"""Served-rank evaluation on the GPU (csrc/rank_served.hip through ops.score_ahead, model.served_rank,
dist.VocabParallel.ahead) against the float64 oracle of tests/rank_served_oracle.py and against the product's own serving
routes.

Random inputs are checked by the interval every count consistent with scores known to +-1e-4 must fall in (the bound and the
width cap of tests/test_rank_gpu.py; tests/test_rank_served_cpu.py checks at these very shapes that the intervals stay narrow).
The checks without a tolerance: shard additivity, position j of the selection kernel's own list counts j rows ahead (the two
kernels form the same fp32 score for every pair), a zero bias is no bias, and a call does not depend on what ran before it."""
import os

import pytest
import torch

import rank_served_oracle as ro
from rank_oracle import assert_in_interval
from util import ROOT, pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')


def _ops():
    return pkg('ops')


def _dev(kw, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _target(ops, srs, E, labels, kw):
    """the labels' served scores by the route model.served_rank takes: score_items at labels[:, None]"""
    cs = kw['cs']
    rest = {k: v for k, v in kw.items() if k != 'cs'}
    return ops.score_items(srs, E, cs, labels[:, None].clamp(min=-1), **rest)[:, 0]


def _ahead(ops, srs, E, labels, target, kw, floor=None, id_lo=0):
    cs = kw['cs']
    rest = {k: v for k, v in kw.items() if k != 'cs'}
    return ops.score_ahead(srs, E, cs, labels, target, id_lo=id_lo, floor=floor, **rest)


# ------------------------------------------------------------------------------------------- 1) kernel cases, interval check
@pytest.mark.parametrize('B,V,d,C', ro.SHAPES)
def test_counts_inside_the_roundoff_interval_for_every_operand_variant(dev, B, V, d, C):
    ops = _ops()
    case = ro.kernel_case(B, V, d, C)
    srs, E, labels = case['srs'].to(dev), case['E'].to(dev), case['labels'].to(dev)
    for lists, bias, floored, with_cs in ro.variants():
        kw = ro.variant(case, lists, bias, with_cs)
        s64, elig = ro.served64(case['srs'], case['E'], id_lo=0, **kw)
        kwd = _dev(kw, dev)
        target = _target(ops, srs, E, labels, kwd)
        t64 = torch.where(elig, s64, torch.full_like(s64, NINF)).gather(1, case['labels'].clamp(min=0)[:, None])[:, 0]
        live = case['labels'] >= 0
        tc = target.cpu().double()
        assert torch.equal(tc[live] == NINF, t64[live] == NINF), (lists, bias)
        fin = live & (t64 > NINF)
        assert float((tc[fin] - t64[fin]).abs().max()) < ro.TOL
        floor = ro.median_floor(s64, elig) if floored else None
        got = _ahead(ops, srs, E, labels, target, kwd, None if floor is None else floor.to(dev))
        assert got.dtype == torch.int32 and got.shape == (B,)
        what = '%s lists %s bias %s floor %s cs %s' % ((B, V, d, C), lists, bias, floored, with_cs)
        lo, hi = ro.assert_ahead_in_interval(got, s64, elig, case['labels'], target.cpu(), ro.TOL, floor, what=what)
        assert bool((got.cpu()[~live] == 0).all()), what
        print(what, 'got', got.tolist()[:8], 'lo', lo.tolist()[:8], 'hi', hi.tolist()[:8])
        if lists == 'score' and bias == 'none' and not floored:
            # the list matters: scored with off_ex everywhere the counts leave the interval
            s_ex, _ = ro.served64(case['srs'], case['E'], id_lo=0, **{**kw, 'listed': None, 'off_in': None})
            wrong = ro.ahead_exact(s_ex, elig, case['labels'], target.cpu())
            assert int(((wrong < lo) | (wrong > hi)).sum()) > 0


# ------------------------------------------------------------------------------------------- 2) exact, tolerance-free checks
def test_counts_of_two_row_shards_add_up_to_the_whole_table(dev):
    ops = _ops()
    B, V, d, C = 33, 5000, 32, 3
    case = ro.kernel_case(B, V, d, C)
    srs, E, labels = case['srs'].to(dev), case['E'].to(dev), case['labels'].to(dev)
    cut = 2500
    for lists, bias, floored, with_cs in ro.variants():
        kw = _dev(ro.variant(case, lists, bias, with_cs), dev)
        target = _target(ops, srs, E, labels, kw)
        floor = None
        if floored:
            s64, elig = ro.served64(case['srs'], case['E'], id_lo=0, **ro.variant(case, lists, bias, with_cs))
            floor = ro.median_floor(s64, elig).to(dev)
        whole = _ahead(ops, srs, E, labels, target, kw, floor)
        parts = []
        for lo, hi in ((0, cut), (cut, V)):
            sub = dict(kw)
            if sub['cs'] is not None:
                sub['cs'] = sub['cs'][lo:hi]
            if sub['bias'] is not None:
                sub['bias'] = sub['bias'][..., lo:hi]                        # a column slice: the row stride stays V
            parts.append(_ahead(ops, srs, E[lo:hi], labels, target, sub, floor, id_lo=lo))
        assert torch.equal(parts[0] + parts[1], whole), (lists, bias, floored, (parts[0] + parts[1] - whole).tolist())
        assert int(parts[0].max()) > 0 and int(parts[1].max()) > 0


@pytest.mark.parametrize('B,V,d,C', [(33, 300, 32, 1), (33, 5000, 36, 1), (33, 5000, 32, 3), (33, 300, 320, 4)])
def test_position_j_of_the_selection_has_j_rows_ahead(dev, B, V, d, C):
    """label := ids[b, j], target := values[b, j] of ops.score_select(k = 20) over the same operands: the count is j for every
    filled slot - the two kernels form the same fp32 score for every (session, row) pair and break ties the same way"""
    ops = _ops()
    K = 20
    case = ro.kernel_case(B, V, d, C)
    srs, E = case['srs'].to(dev), case['E'].to(dev)
    for lists, bias, floored, with_cs in ro.variants():
        kw = _dev(ro.variant(case, lists, bias, with_cs), dev)
        cs = kw['cs']
        rest = {k: v for k, v in kw.items() if k != 'cs'}
        floor = None
        if floored:                                         # a floor that cuts into the list: the session's 10th best value
            floor = ops.score_select(srs, E, cs, K, **rest)[0][:, 9].contiguous()
        val, idx = ops.score_select(srs, E, cs, K, floor=floor, **rest)
        filled = idx >= 0
        assert bool(filled[:, 0].all()) and (not floored or not bool(filled[:, 12].any()) or V < 100)
        for j in range(K):
            got = ops.score_ahead(srs, E, cs, idx[:, j], val[:, j].contiguous(), floor=floor, **rest)
            ok = filled[:, j]
            assert torch.equal(got[ok], torch.full_like(got[ok], j)), (lists, bias, floored, j, got.tolist(), idx[:, j].tolist())
            assert bool((got[~ok] == 0).all())              # an unfilled slot is a label < 0


def test_a_zero_bias_is_no_bias_and_null_operands_are_the_plain_call(dev):
    ops = _ops()
    for B, V, d, C in ro.SHAPES[1:4]:
        case = ro.kernel_case(B, V, d, C)
        srs, E, labels = case['srs'].to(dev), case['E'].to(dev), case['labels'].to(dev)
        for lists in ro.LISTS:
            kw = _dev(ro.variant(case, lists, 'none', True), dev)
            target = _target(ops, srs, E, labels, kw)
            plain = _ahead(ops, srs, E, labels, target, kw)
            zero = _ahead(ops, srs, E, labels, target, {**kw, 'bias': torch.zeros(V, device=dev)})
            zero3 = _ahead(ops, srs, E, labels, target, {**kw, 'bias': torch.zeros(3, V, device=dev), 'group': case['group'].to(dev)})
            low = _ahead(ops, srs, E, labels, target, kw, torch.full((B,), NINF, device=dev))
            assert torch.equal(zero, plain) and torch.equal(zero3, plain) and torch.equal(low, plain), (B, V, d, C, lists)
        # without a list, a bias or a floor the count is score_rank's for the same target
        kw = _dev(ro.variant(case, 'none', 'none', True), dev)
        target = _target(ops, srs, E, labels, kw)
        rank, _ = ops.score_rank(srs, E, kw['cs'], labels, kw['off_ex'], target=target)
        assert torch.equal(_ahead(ops, srs, E, labels, target, kw), rank.clamp(min=0))


def test_a_call_repeats_its_bits_whatever_ran_in_between(dev):
    ops = _ops()
    outs = []
    for shape in (ro.SHAPES[3], ro.SHAPES[4], ro.SHAPES[3]):
        case = ro.kernel_case(*shape)
        srs, E, labels = case['srs'].to(dev), case['E'].to(dev), case['labels'].to(dev)
        kw = _dev(ro.variant(case, 'score', 'grouped', True), dev)
        target = _target(ops, srs, E, labels, kw)
        outs.append(_ahead(ops, srs, E, labels, target, kw).cpu())
    assert torch.equal(outs[0], outs[2]) and int(outs[0].max()) > 0 and outs[0].shape == outs[1].shape


def test_the_call_adds_no_entry_to_the_shared_scratch_caches(dev):
    score = pkg('score')
    before = (set(score._BYTE_WS), set(score._NORM_WS), set(score._SAMPLE_WS))
    case = ro.kernel_case(*ro.SHAPES[0])
    srs, E, labels = case['srs'].to(dev), case['E'].to(dev), case['labels'].to(dev)
    kw = _dev(ro.variant(case, 'drop', 'vec', True), dev)
    _ahead(_ops(), srs, E, labels, torch.zeros(labels.numel(), device=dev), kw)
    assert (set(score._BYTE_WS), set(score._NORM_WS), set(score._SAMPLE_WS)) == before


# ------------------------------------------------------------------------------------------- 3) models
def _model_case(name, dev):
    """a small random model and one batch of the sample sessions"""
    from test_models_gpu import _collate
    sp, ds = pkg(), pkg('dataset')
    V, d = 3429, 32
    torch.manual_seed(11 + len(name))
    if name == 'srgnn':
        model = sp.SRGNN(V, d, 1)
    elif name == 'niser':
        model = sp.NISER(V, d, 1)
    elif name.startswith('lessr'):
        model = sp.LESSR(V, d, 2)
    else:
        model = sp.MSGIFSR(V, 'sample', d, 1, order=2, extra=True, fusion=True)
    data = ds.AugmentedDataset(ds.read_sessions(os.path.join(ROOT, 'tests', 'golden', 'sample_test.txt')))
    samples = [data[i] for i in range(40, 72)]
    samples = [([int(x) for x in seq], int(lab)) for seq, lab in samples]
    inputs, labels = _collate(name, samples)
    return model.to(dev).eval(), [x.to(dev) for x in inputs], labels.to(dev), samples, V


@pytest.mark.parametrize('name', ['srgnn', 'niser', 'lessr_L2', 'msgifsr_K2_ext_fus'])
def test_model_served_rank_is_the_position_in_recommend(dev, name):
    ops = _ops()
    model, inputs, data_labels, samples, V = _model_case(name, dev)
    B = len(samples)
    ids0 = model.recommend(*inputs, k=128)[1].long()
    labels = data_labels.clone().long()
    even = torch.arange(B, device=dev) % 2 == 0
    labels[even] = ids0[torch.arange(B, device=dev), (7 * torch.arange(B, device=dev)) % 128][even]   # labels recommend() returns
    labels[3] = samples[3][0][-1]                        # a label the session has seen
    labels[5] = -1
    g = torch.Generator().manual_seed(5)
    deny_ids = torch.randperm(V, generator=g)[:300].tolist() + [int(labels[4]), int(labels[9])]
    deny = ops.catalog_bias(V, deny=deny_ids, device=dev)
    seen = torch.zeros(B, V, dtype=torch.bool)
    for b, (seq, _) in enumerate(samples):
        seen[b, torch.tensor(seq)] = True
    lab_c = labels.cpu()
    safe = lab_c.clamp(min=0)
    is_seen = seen[torch.arange(B), safe] & (lab_c >= 0)
    is_denied = (deny.cpu()[safe] == NINF) & (lab_c >= 0)
    assert bool(is_seen[3]) and bool(is_denied[4]) and bool(is_denied[9])
    for kw in (dict(exclude_seen=True), dict(item_bias=deny), dict(exclude_seen=True, item_bias=deny)):
        ids = model.recommend(*inputs, k=128, **kw)[1].cpu().long()
        r = model.served_rank(*inputs, labels=labels, **kw)
        assert r.dtype == torch.int32 and r.shape == (B,) and not model.training
        r = r.cpu().long()
        gone = (is_seen if kw.get('exclude_seen') else torch.zeros(B, dtype=torch.bool)) | \
               (is_denied if 'item_bias' in kw else torch.zeros(B, dtype=torch.bool))
        found = 0
        for b in range(B):
            pos = (ids[b] == lab_c[b]).nonzero().flatten().tolist() if lab_c[b] >= 0 else []
            if lab_c[b] < 0:
                assert r[b] == -1, (name, kw.keys(), b)
            elif gone[b]:
                assert r[b] == -2 and not pos, (name, kw.keys(), b, int(r[b]))
            else:
                assert r[b] >= 0, (name, kw.keys(), b, int(r[b]))
                if pos:
                    found += 1
                    assert r[b] == pos[0], (name, kw.keys(), b, int(r[b]), pos)
                if r[b] < 128:
                    assert ids[b, r[b]] == lab_c[b], (name, kw.keys(), b, int(r[b]))
        print(name, sorted(kw), 'labels inside the 128 best:', found, 'ranks', r.tolist()[:12])
        assert found >= B // 4
    # no keywords: inside the round-off interval of forward()'s log-probabilities, and target_rank's own answer
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    r0 = model.served_rank(*inputs, labels=labels)
    lo, hi = assert_in_interval(r0, s64, lab_c, ro.TOL, what=name + ' vs forward()')
    print(name, 'no keywords: rank', r0.tolist()[:10], 'lo', lo.tolist()[:10], 'hi', hi.tolist()[:10])
    # a top_k truncation: labels well inside keep their rank, labels well outside could not have been shown
    rk = model.served_rank(*inputs, labels=labels, top_k=50).cpu().long()
    r0 = r0.cpu().long()
    inside, outside = (r0 >= 0) & (r0 < 49), r0 > 50
    assert torch.equal(rk[inside], r0[inside]) and bool((rk[outside] == -2).all()) and rk[5] == -1, (name, rk.tolist(), r0.tolist())
    assert int(inside.sum()) > 0 and int(outside.sum()) > 0


# ------------------------------------------------------------------------------------------- 4) launcher
def test_evaluate_launcher_prints_the_metrics_of_the_in_process_call(dev, tmp_path):
    import json
    import subprocess
    import sys
    from torch.utils.data import DataLoader
    sp, col, ds, train, ops = pkg(), pkg('collate'), pkg('dataset'), pkg('train'), _ops()
    V = int(open(os.path.join(ROOT, 'datasets', 'sample', 'num_items.txt')).readline())
    data = tmp_path / 'data'
    data.mkdir()
    (data / 'num_items.txt').write_text('%d\n' % V)
    lines = open(os.path.join(ROOT, 'tests', 'golden', 'sample_test.txt')).read().splitlines()[:40]
    (data / 'test.txt').write_text('\n'.join(lines) + '\n')
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    g = torch.Generator().manual_seed(10)
    deny = torch.randperm(V, generator=g)[:V // 3].tolist()
    (tmp_path / 'deny.txt').write_text(''.join('%d\n' % i for i in deny))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'src', 'scripts', 'evaluate.py'), '--model', 'SRGNN', '--dataset-dir', str(data),
                        '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--cutoffs', '5,50,500',
                        '--exclude-seen', '--deny', str(tmp_path / 'deny.txt'), '--sample-top-k', '1000', '--batch-size', '64'],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    test_set = ds.AugmentedDataset(ds.read_sessions(str(data / 'test.txt')))
    loader = DataLoader(test_set, batch_size=64, shuffle=False, collate_fn=col.collate_fn_factory(col.seq_to_session_graph))
    want = train.evaluate_served(model.to(dev).eval(), loader, dev, (5, 50, 500), exclude_seen=True,
                                 item_bias=ops.catalog_bias(V, deny=deny, device=dev), top_k=1000)
    assert out['sessions'] == len(test_set) > 64 and out['flags']['cutoffs'] == [5, 50, 500] and out['flags']['exclude_seen'] is True
    assert set(out['metrics']) == set(want) == {'hit@5', 'mrr@5', 'ndcg@5', 'hit@50', 'mrr@50', 'ndcg@50', 'hit@500', 'mrr@500',
                                                'ndcg@500', 'shown'}
    for k, v in want.items():
        assert abs(out['metrics'][k] - v) < 1e-12, (k, out['metrics'][k], v)
    # a third of the catalogue is denied, seen items are gone and only the 1000 best are shown: many labels are not
    assert 0.0 < want['shown'] < 0.6 and want['hit@5'] <= want['hit@50'] <= want['hit@500'] <= want['shown']
    print('evaluate.py:', r.stdout.strip().splitlines()[-1][:300])


# ------------------------------------------------------------------------------------------- 5) sharded, W = 2 on one GPU
def test_sharded_ahead_and_served_rank_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from item_bias_gpu_worker import sharded_bias
    from rank_served_gpu_worker import TOP_K, run_rank, seen_model, sharded_labels
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
    sr, E, cs, listed = sharded_case()
    bias, group = sharded_bias()
    labels = sharded_labels()
    model = seen_model(E, listed).to(dev)
    sr, E, cs, listed_d, bias_d, group_d, labels_d = [x.to(dev) for x in (sr, E, cs, listed, bias, group, labels)]
    kw = dict(listed=listed_d, drop_listed=True, bias=bias_d, group=group_d)
    target = ops.score_items(sr, E, cs, labels_d[:, None], **kw)[:, 0]
    floor = ops.score_cutoff(sr, E, cs, top_k=TOP_K, **kw)[0]
    want = dict(target=target.cpu(), floor=floor.cpu(), ahead=ops.score_ahead(sr, E, cs, labels_d, target, **kw).cpu(),
                ahead_floor=ops.score_ahead(sr, E, cs, labels_d, target, floor=floor, **kw).cpu())
    want['ahead_routed'] = want['ahead']
    want['served'] = model.served_rank(sr, labels=labels_d, exclude_seen=True, item_bias=bias_d, item_group=group_d).cpu()
    want['served_top_k'] = model.served_rank(sr, labels=labels_d, exclude_seen=True, item_bias=bias_d, item_group=group_d,
                                             top_k=TOP_K).cpu()
    # the single-device counts against the oracle (exact inputs: equal)
    s64, elig = ro.served64(sr.cpu(), E.cpu(), cs.cpu(), None, None, listed, True, 0, bias, group)
    assert torch.equal(want['ahead'].long(), ro.ahead_exact(s64, elig, labels, target.cpu()))
    assert want['served'][0] == -1 and want['served'][1] == -2 and int((want['served'] >= 0).sum()) > 8
    assert int((want['served_top_k'] == -2).sum()) > int((want['served'] == -2).sum())
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        for key, w in want.items():                       # every rank feeds the same sessions: the full answer on every rank
            assert res[key].dtype == w.dtype and torch.equal(res[key], w), (r, key, res[key].tolist(), w.tolist())
        mine = slice(r * n, (r + 1) * n)
        w = ops.score_ahead(sr[mine], E, cs, labels_d[mine], target[mine], listed=listed_d[mine, :4 + r], drop_listed=True,
                            bias=bias_d, group=group_d[mine], floor=floor[mine]).cpu()
        assert torch.equal(res['ahead_dp'], w), r
