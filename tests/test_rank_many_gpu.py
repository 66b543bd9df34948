"""Many-targets served rank on the GPU (csrc/rank_served_many.hip through ops.score_ahead_many, model.rank_items,
dist.VocabParallel.ahead_many, train.evaluate_rest) against the float64 oracle of tests/rank_many_oracle.py and against the
product's own single-label route (ops.score_ahead, csrc/rank_served.hip), which this change leaves as it is.

Random inputs are checked by the interval every count consistent with scores known to +-1e-4 must fall in (N; the targets
among themselves are ordered by their given values, exactly); tests/test_rank_many_cpu.py checks at these very shapes that the
intervals stay narrow and that few targets lie within round-off of each other.  The checks without a tolerance: M = 1 is
score_ahead, a column is score_ahead for its item where no other target is within round-off, positions in the selection
kernel's own list, exact ties, shard additivity, column permutations, and repeatability."""
import json
import os
import subprocess
import sys

import pytest
import torch

import rank_many_oracle as mo
import rank_served_oracle as ro
from util import ROOT, pkg

pytestmark = pytest.mark.gpu

NINF = float('-inf')
MS = (1, 5, 64)


def _ops():
    return pkg('ops')


def _dev(kw, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _split(kw):
    return kw['cs'], {k: v for k, v in kw.items() if k != 'cs'}


def _values(ops, srs, E, items, kw):
    """the items' served scores by the route model.rank_items takes: score_items"""
    cs, rest = _split(kw)
    return ops.score_items(srs, E, cs, items, **rest)


def _many(ops, srs, E, items, target, kw, floor=None, id_lo=0, among_targets=True):
    cs, rest = _split(kw)
    return ops.score_ahead_many(srs, E, cs, items, target, id_lo=id_lo, floor=floor, among_targets=among_targets, **rest)


def _one(ops, srs, E, labels, target, kw, floor=None):
    cs, rest = _split(kw)
    return ops.score_ahead(srs, E, cs, labels, target.contiguous(), floor=floor, **rest)


def _cases(dev, B, V, d, C):
    """every operand variant of one shape: (what, device keywords, float64 scores, eligibility, floor or None)"""
    case = ro.kernel_case(B, V, d, C)
    for lists, bias, floored, with_cs in ro.variants():
        kw = ro.variant(case, lists, bias, with_cs)
        s64, elig = ro.served64(case['srs'], case['E'], id_lo=0, **kw)
        floor = ro.median_floor(s64, elig) if floored else None
        what = '%s lists %s bias %s floor %s cs %s' % ((B, V, d, C), lists, bias, floored, with_cs)
        yield what, case, _dev(kw, dev), s64, elig, floor


# ------------------------------------------------------------------------------------------- 1) - 3) kernel cases
@pytest.mark.parametrize('B,V,d,C', ro.SHAPES)
def test_counts_inside_the_roundoff_interval_and_columns_equal_the_single_label_kernel(dev, B, V, d, C):
    """1) every count lies inside the oracle interval, empty slots give 0;  2) M = 1 is ops.score_ahead, bit for bit;
    3) column j is ops.score_ahead(labels=items[:, j], target=target[:, j]) wherever no other target of the session lies
    within 2 TOL of the slot's value (at most 5 % of the live slots are left out).
    With a floor one more thing is decided by round-off, and differently by the two calls: whether ANOTHER target i that lies
    within 2 TOL of the floor counts at all - the single-label call tests the pass's score of row i against the floor, the
    many-targets call the given value target[b,i], as the contract says (median_floor() IS the score of one row of the
    session, and that row is sometimes a target).  Such slots are COMPARED too, not left out: the two counts may differ by at
    most the number of the session's other targets within 2 TOL of the floor that could stand ahead of the slot."""
    ops = _ops()
    slots = skipped = at_floor = 0
    for what, case, kw, s64, elig, floor in _cases(dev, B, V, d, C):
        srs, E = case['srs'].to(dev), case['E'].to(dev)
        fl = None if floor is None else floor.to(dev)
        for M in MS:
            items = mo.targets(case, B, V, d, C, M)
            items_d = items.to(dev)
            target = _values(ops, srs, E, items_d, kw)
            t64 = mo.target_values64(s64, elig, items)
            tc = target.cpu().double()
            assert torch.equal(tc == NINF, t64 == NINF), what
            fin = t64 > NINF
            assert float((tc[fin] - t64[fin]).abs().max()) < ro.TOL
            got = _many(ops, srs, E, items_d, target, kw, fl)
            assert got.dtype == torch.int32 and got.shape == (B, M)
            lo, hi = mo.assert_many_in_interval(got, s64, elig, items, target.cpu(), ro.TOL, floor, what='%s M %d' % (what, M))
            assert bool((got.cpu()[items < 0] == 0).all()), what
            cols = torch.stack([_one(ops, srs, E, items_d[:, j], target[:, j], kw, fl) for j in range(M)], 1)
            if M == 1:
                assert torch.equal(got, cols), (what, got.flatten().tolist(), cols.flatten().tolist())
                continue
            live = items >= 0
            close = mo.close_targets(items, t64) & live
            edge = mo.targets_at_the_floor_ahead(items, t64, floor)             # [B, M] int: 0 almost everywhere
            check = (live & ~close).to(dev)
            diff = (got.long() - cols.long()).abs().cpu()
            bad = (live & ~close) & (diff > edge)
            assert not bool(bad.any()), (what, M, bad.nonzero().tolist()[:8], diff[bad].tolist()[:8], edge[bad].tolist()[:8])
            exact = check & (edge == 0).to(dev)
            assert torch.equal(got[exact], cols[exact])
            slots += int(live.sum())
            skipped += int(close.sum())
            at_floor += int((live & ~close & (edge > 0)).sum())
        print(what, 'M 64: got', got[0, :6].tolist(), 'lo', lo[0, :6].tolist(), 'hi', hi[0, :6].tolist())
    print('shape', (B, V, d, C), 'live slots', slots, 'left out as close', skipped, 'compared within the floor bound', at_floor)
    assert skipped <= 0.05 * slots, (skipped, slots)


# ------------------------------------------------------------------------------------------- 4) positions in the selection
@pytest.mark.parametrize('B,V,d,C', [(33, 300, 32, 1), (33, 5000, 36, 1), (33, 5000, 32, 3), (33, 300, 320, 4)])
def test_every_second_slot_of_the_selection_ranks_at_its_position(dev, B, V, d, C):
    """targets := every second slot of ops.score_select(k = 20) with its values, columns shuffled: the rank is exactly the
    slot's position - the odd slots are counted by the pass, the even ones among the targets - with and without a floor that
    cuts into the list"""
    ops = _ops()
    K = 20
    case = ro.kernel_case(B, V, d, C)
    srs, E = case['srs'].to(dev), case['E'].to(dev)
    g = torch.Generator().manual_seed(8)
    perm = torch.randperm(K // 2, generator=g).to(dev)
    for lists, bias, floored, with_cs in ro.variants():
        kw = _dev(ro.variant(case, lists, bias, with_cs), dev)
        cs, rest = _split(kw)
        floor = None
        if floored:                                         # a floor that cuts into the list: the session's 10th best value
            floor = ops.score_select(srs, E, cs, K, **rest)[0][:, 9].contiguous()
        val, idx = ops.score_select(srs, E, cs, K, floor=floor, **rest)
        pos = (2 * perm)[None, :].expand(B, -1)
        items, target = idx.gather(1, pos).contiguous(), val.gather(1, pos).contiguous()
        got = _many(ops, srs, E, items, target, kw, floor)
        filled = items >= 0
        assert bool(filled[:, 0].all()) and (not floored or not bool((idx[:, 12:] >= 0).any()) or V < 100)
        assert torch.equal(got[filled], pos[filled].to(torch.int32)), (lists, bias, floored, got.tolist()[:3], pos.tolist()[:1])
        assert bool((got[~filled] == 0).all())              # an unfilled slot is an empty slot


# ------------------------------------------------------------------------------------------- 5) exact ties
def _pass_value(ops, srs, E, cs, u, rest, V, dev):
    """the score THE PASS forms for item u of every session (fp32 [B]): the selection kernel with everything but u outside
    the catalogue (s + bias with the bias the call already has, or + 0)"""
    only = torch.full((V,), NINF, device=dev)
    only[u] = rest['bias'][u] if rest.get('bias') is not None else 0.0
    return ops.score_select(srs, E, cs, 1, **{**rest, 'bias': only, 'group': None})[0][:, 0].contiguous()


@pytest.mark.parametrize('B,V,d,C', [(33, 300, 36, 3), (33, 5000, 36, 1)])
def test_exact_ties_go_to_the_lower_id_and_shown_ranks_are_distinct(dev, B, V, d, C):
    ops = _ops()
    case = ro.kernel_case(B, V, d, C)
    u, x, w = 17, 140, 291
    E, cs_, bias = case['E'].clone(), case['cs'].clone(), case['bias_vec'].clone()
    E[x], E[w], cs_[x], cs_[w] = E[u], E[u], cs_[u], cs_[u]
    bias[u] = bias[x] = bias[w] = 0.25
    srs, E, cs_, bias = case['srs'].to(dev), E.to(dev), cs_.to(dev), bias.to(dev)
    off_ex = case['off_ex'].to(dev)
    for rest in (dict(off_ex=off_ex), dict(off_ex=off_ex, bias=bias)):
        t = _pass_value(ops, srs, E, cs_, u, rest, V, dev)
        assert torch.equal(t, _pass_value(ops, srs, E, cs_, w, rest, V, dev)) and bool((t > NINF).all())
        items = torch.tensor([[w, u]], device=dev).expand(B, 2).contiguous()
        target = torch.stack([t, t], 1)
        got = ops.score_ahead_many(srs, E, cs_, items, target, **rest)
        # the non-target copy x counts ahead of w (x < w) but not of u (u < x), and u is ahead of w
        assert torch.equal(got[:, 0], got[:, 1] + 2), (sorted(rest), got.tolist()[:6])
        # x among the targets as well: three distinct consecutive ranks in id order
        items3 = torch.tensor([[x, w, u]], device=dev).expand(B, 3).contiguous()
        got3 = ops.score_ahead_many(srs, E, cs_, items3, torch.stack([t, t, t], 1), **rest)
        assert torch.equal(got3[:, 0], got3[:, 2] + 1) and torch.equal(got3[:, 1], got3[:, 2] + 2)
        assert torch.equal(got3[:, 2], got[:, 1])
    # random targets: the shown ones of every session get pairwise distinct ranks, ordered as (value descending, id ascending)
    for M in (5, 64):
        items = mo.targets(case, B, V, d, C, M).to(dev)
        kw = _dev(ro.variant(case, 'drop', 'vec', True), dev)
        target = _values(ops, srs, case['E'].to(dev), items, kw)
        got = _many(ops, srs, case['E'].to(dev), items, target, kw).cpu()
        items_c, target_c = items.cpu(), target.cpu()
        for b in range(B):
            shown = ((items_c[b] >= 0) & (target_c[b] > NINF)).nonzero().flatten().tolist()
            order = sorted(shown, key=lambda j: (-float(target_c[b, j]), int(items_c[b, j])))
            ranks = [int(got[b, j]) for j in order]
            assert all(a < c for a, c in zip(ranks, ranks[1:])), (M, b, ranks)


# ------------------------------------------------------------------------------------------- 6) - 8) exact properties
def test_counts_of_two_row_shards_plus_the_targets_among_themselves_equal_the_whole_table(dev):
    ops = _ops()
    B, V, d, C = 33, 5000, 32, 3
    cut = 2500
    for what, case, kw, s64, elig, floor in _cases(dev, B, V, d, C):
        srs, E = case['srs'].to(dev), case['E'].to(dev)
        fl = None if floor is None else floor.to(dev)
        for M in (5, 64):
            items = mo.targets(case, B, V, d, C, M).to(dev)
            target = _values(ops, srs, E, items, kw)
            whole = _many(ops, srs, E, items, target, kw, fl)
            parts = []
            for lo, hi in ((0, cut), (cut, V)):
                sub = dict(kw)
                if sub['cs'] is not None:
                    sub['cs'] = sub['cs'][lo:hi]
                if sub['bias'] is not None:
                    sub['bias'] = sub['bias'][..., lo:hi]                    # a column slice: the row stride stays V
                parts.append(_many(ops, srs, E[lo:hi], items, target, sub, fl, id_lo=lo, among_targets=False))
            among = ops.ahead_among_targets(items, target, fl)
            assert torch.equal(parts[0] + parts[1] + among, whole), (what, M)
            assert int(parts[0].max()) > 0 and int(parts[1].max()) > 0 and int(among.max()) > 0
            assert torch.equal(_many(ops, srs, E, items, target, kw, fl, among_targets=False) + among, whole)


def test_permuting_the_target_columns_permutes_the_output(dev):
    ops = _ops()
    g = torch.Generator().manual_seed(4)
    for shape in (ro.SHAPES[1], ro.SHAPES[2], ro.SHAPES[4]):
        case = ro.kernel_case(*shape)
        srs, E = case['srs'].to(dev), case['E'].to(dev)
        kw = _dev(ro.variant(case, 'score', 'grouped', True), dev)
        for M in (5, 64):
            items = mo.targets(case, *shape, M).to(dev)
            target = _values(ops, srs, E, items, kw)
            got = _many(ops, srs, E, items, target, kw)
            perm = torch.randperm(M, generator=g).to(dev)
            again = _many(ops, srs, E, items[:, perm].contiguous(), target[:, perm].contiguous(), kw)
            assert torch.equal(again, got[:, perm]), (shape, M)
            # a wider row with empty slots in between changes nothing for the live ones
            wide = torch.full((items.shape[0], min(64, M + 3)), -1, device=dev, dtype=items.dtype)
            wt = torch.zeros(wide.shape, device=dev)
            keep = M - (M + 3 - wide.shape[1])
            wide[:, 3:], wt[:, 3:] = items[:, :keep], target[:, :keep]
            if keep == M:
                assert torch.equal(_many(ops, srs, E, wide, wt, kw)[:, 3:], got)


def test_a_call_repeats_its_bits_whatever_ran_in_between(dev):
    ops = _ops()
    outs = []
    for shape in (ro.SHAPES[3], ro.SHAPES[4], ro.SHAPES[3]):
        case = ro.kernel_case(*shape)
        srs, E = case['srs'].to(dev), case['E'].to(dev)
        kw = _dev(ro.variant(case, 'score', 'grouped', True), dev)
        items = mo.targets(case, *shape, 64).to(dev)
        target = _values(ops, srs, E, items, kw)
        outs.append(_many(ops, srs, E, items, target, kw).cpu())
    assert torch.equal(outs[0], outs[2]) and int(outs[0].max()) > 0 and outs[0].shape == outs[1].shape


# ------------------------------------------------------------------------------------------- 9) models
@pytest.mark.parametrize('name', ['srgnn', 'niser', 'lessr_L2', 'msgifsr_K2_ext_fus'])
def test_model_rank_items_gives_the_positions_in_recommend(dev, name):
    from test_rank_served_gpu import _model_case
    ops = _ops()
    model, inputs, data_labels, samples, V = _model_case(name, dev)
    B = len(samples)
    g = torch.Generator().manual_seed(5)
    deny_ids = torch.randperm(V, generator=g)[:300].tolist()
    deny = ops.catalog_bias(V, deny=deny_ids, device=dev)
    slots = torch.tensor([0, 9, 27, 50, 88, 127], device=dev)
    rows = torch.arange(B, device=dev)
    for kw in (dict(), dict(exclude_seen=True), dict(exclude_seen=True, item_bias=deny)):
        ids = model.recommend(*inputs, k=128, **kw)[1].long()
        pos = (slots[None, :] + rows[:, None]) % 128                          # other positions in every session
        items = ids.gather(1, pos)
        shuffle = torch.tensor([3, 0, 5, 1, 4, 2], device=dev)
        items, pos = items[:, shuffle], pos[:, shuffle]
        seen_item = torch.tensor([samples[b][0][-1] for b in range(B)], device=dev)
        items = torch.cat([items, seen_item[:, None], torch.full((B, 1), deny_ids[0], device=dev), torch.full((B, 1), -1, device=dev)], 1)
        clash = (items[:, :6] == items[:, 6:7]) | (items[:, :6] == items[:, 7:8])      # (without a filter they may be in the list)
        items[:, :6] = torch.where(clash, torch.full_like(items[:, :6], -1), items[:, :6])
        items[:, 7] = torch.where(items[:, 7] == items[:, 6], torch.full_like(items[:, 7], -1), items[:, 7])
        r = model.rank_items(*inputs, items=items, **kw)
        assert r.dtype == torch.int32 and r.shape == (B, 9) and not model.training
        live = items[:, :6] >= 0
        assert torch.equal(r[:, :6][live].long(), pos[live]), (name, sorted(kw), r[:4].tolist(), pos[:4].tolist())
        assert int(live.sum()) > 5 * B and bool((r[:, 8] == -1).all()) and bool((r[:, :6][~live] == -1).all())
        if kw.get('exclude_seen'):
            assert bool((r[:, 6] == -2).all()), (name, sorted(kw))
        if 'item_bias' in kw:
            assert bool((r[:, 7][items[:, 7] >= 0] == -2).all()), (name, sorted(kw))
        # column 0 is served_rank for the same labels
        one = model.served_rank(*inputs, labels=items[:, 0], **kw)
        assert torch.equal(r[:, 0], one), (name, sorted(kw), r[:, 0].tolist(), one.tolist())
        # one item per session takes served_rank's route, a shared 1-D list is every session's list
        assert torch.equal(model.rank_items(*inputs, items=items[:, :1], **kw)[:, 0], one)
        shared = model.rank_items(*inputs, items=items[0, :6][items[0, :6] >= 0], **kw)
        assert torch.equal(shared[0], r[0, :6][items[0, :6] >= 0])
    # a top_k truncation: targets inside keep their rank, targets outside could not have been shown
    ids = model.recommend(*inputs, k=128)[1].long()
    items = ids[:, [3, 40, 100]]
    rk = model.rank_items(*inputs, items=items, top_k=50)
    assert bool((rk[:, 0] == 3).all()) and bool((rk[:, 1] == 40).all()) and bool((rk[:, 2] == -2).all()), (name, rk[:4].tolist())


# ------------------------------------------------------------------------------------------- 10) launcher
def test_evaluate_launcher_rest_protocol_prints_the_metrics_of_the_in_process_call(dev, tmp_path):
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
    base = [sys.executable, os.path.join(ROOT, 'src', 'scripts', 'evaluate.py'), '--model', 'SRGNN', '--dataset-dir', str(data),
            '--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt), '--cutoffs', '5,50,500',
            '--deny', str(tmp_path / 'deny.txt'), '--sample-top-k', '1000', '--batch-size', '64']
    r = subprocess.run(base + ['--protocol', 'rest', '--max-targets', '4'], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    test_set = ds.AugmentedDataset(ds.read_sessions(str(data / 'test.txt')))
    fn = col.collate_fn_factory(col.seq_to_session_graph)
    model = model.to(dev).eval()
    served = dict(exclude_seen=False, item_bias=ops.catalog_bias(V, deny=deny, device=dev), top_k=1000)
    want = train.evaluate_rest(model, test_set, fn, dev, 64, (5, 50, 500), max_targets=4, **served)
    assert set(out) == {'metrics', 'sessions', 'truncated', 'flags'}
    assert out['sessions'] == len(test_set) > 64 and out['flags']['protocol'] == 'rest' and out['flags']['max_targets'] == 4
    assert out['truncated'] == want.pop('truncated') > 0
    assert set(out['metrics']) == set(want) == {m + '@%d' % k for m in ('hit', 'recall', 'precision', 'mrr', 'map', 'ndcg')
                                               for k in (5, 50, 500)} | {'shown'}
    for k, v in want.items():
        assert abs(out['metrics'][k] - v) < 1e-12, (k, out['metrics'][k], v)
    assert 0.0 < want['shown'] < 0.9 and want['recall@5'] <= want['recall@50'] <= want['recall@500'] <= want['shown']
    assert want['recall@500'] <= want['hit@500']
    # column 0 of the targets is the next-item label: the hit rate of the rest protocol is at least the next-item one
    nxt = train.evaluate_served(model, torch.utils.data.DataLoader(test_set, batch_size=64, shuffle=False, collate_fn=fn), dev,
                                (5, 50, 500), **served)
    assert want['hit@500'] >= nxt['hit@500'] and want['mrr@500'] >= nxt['mrr@500']
    # --protocol next prints exactly evaluate_served's key set
    r = subprocess.run(base + ['--protocol', 'next'], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(line) == {'metrics', 'sessions', 'flags'} and set(line['metrics']) == set(nxt)
    assert 'protocol' not in line['flags'] and 'max_targets' not in line['flags']
    for k, v in nxt.items():
        assert abs(line['metrics'][k] - v) < 1e-12, (k, line['metrics'][k], v)
    print('evaluate.py --protocol rest:', json.dumps(out)[:300])


# ------------------------------------------------------------------------------------------- 11) sharded, W = 2 on one GPU
def test_sharded_ahead_many_and_rank_items_equal_single_device(dev, tmp_path):
    import torch.multiprocessing as mp
    from item_bias_gpu_worker import sharded_bias
    from rank_many_gpu_worker import run_rank, sharded_items
    from rank_served_gpu_worker import TOP_K, seen_model
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
    items = sharded_items()
    model = seen_model(E, listed).to(dev)
    sr, E, cs, listed_d, bias_d, group_d, items_d = [x.to(dev) for x in (sr, E, cs, listed, bias, group, items)]
    kw = dict(listed=listed_d, drop_listed=True, bias=bias_d, group=group_d)
    target = ops.score_items(sr, E, cs, items_d, **kw)
    floor = ops.score_cutoff(sr, E, cs, top_k=TOP_K, **kw)[0]
    want = dict(target=target.cpu(), floor=floor.cpu(), ahead=ops.score_ahead_many(sr, E, cs, items_d, target, **kw).cpu(),
                ahead_floor=ops.score_ahead_many(sr, E, cs, items_d, target, floor=floor, **kw).cpu())
    want['ahead_routed'] = want['ahead']
    want['ranks'] = model.rank_items(sr, items=items_d, exclude_seen=True, item_bias=bias_d, item_group=group_d).cpu()
    want['ranks_top_k'] = model.rank_items(sr, items=items_d, exclude_seen=True, item_bias=bias_d, item_group=group_d,
                                           top_k=TOP_K).cpu()
    # the single-device counts against the oracle (exact inputs: equal)
    s64, elig = ro.served64(sr.cpu(), E.cpu(), cs.cpu(), None, None, listed, True, 0, bias, group)
    assert torch.equal(want['ahead'].long(), mo.ahead_many_exact(s64, elig, items, target.cpu()))
    assert want['ranks'][0, 0] == -1 and want['ranks'][1, 0] == -2 and want['ranks'][4, 2] == -1
    assert int((want['ranks'] >= 0).sum()) > 8 * items.shape[1] // 2
    assert int((want['ranks_top_k'] == -2).sum()) > int((want['ranks'] == -2).sum())
    n = sr.shape[0] // world
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['hi'] - res['lo'] == res['n_live'] and (r == 0 or res['n_live'] < res['rows'])      # a padding row on the last shard
        for key, w in want.items():                       # every rank feeds the same sessions: the full answer on every rank
            assert res[key].dtype == w.dtype and torch.equal(res[key], w), (r, key, res[key].tolist(), w.tolist())
        mine = slice(r * n, (r + 1) * n)
        w = ops.score_ahead_many(sr[mine], E, cs, items_d[mine], target[mine], listed=listed_d[mine, :4 + r], drop_listed=True,
                                 bias=bias_d, group=group_d[mine], floor=floor[mine]).cpu()
        assert torch.equal(res['ahead_dp'], w), r
        w = model.rank_items(sr[mine], items=items_d[mine], item_bias=bias_d, item_group=group_d[mine], top_k=TOP_K).cpu()
        assert torch.equal(res['ranks_dp'], w), r
