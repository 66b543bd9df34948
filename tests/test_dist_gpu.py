"""The row-sharded (vocab-parallel) path with MORE THAN ONE shard, on the one GPU a test box has: W rank processes on
cuda:0 over gloo, the real HIP kernels on every rank (tests/dist_gpu_worker.py), against the plain single-GPU path on
the concatenated global batch - the single-device step of /root/reference/src/utils/train.py:94-101.

Checked per rank: the global mean loss, this rank's rows of the table gradient, the all-reduced gradients of the
replicated encoder, every parameter after the fused Adam step, the data-parallel top-20 and (fixtures) the
log-probabilities.  Then one rank of the same job is re-run alone from the recorded collective results
(dist.ReplayGroup) - eagerly and as a captured + replayed hipGraph - and must land on the parameters it reached inside
the job: the kernels of a rank with shard offset > 0 under graph capture."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from dist_gpu_worker import (build_on, digest, digest_rows, live_samples, make_case, rank_slice, run_rank, step_seed,
                             touched_items)
from test_models_gpu import adam_close
from util import close, pkg, reseed

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _launch(world, case, tmp_path):
    ctx = mp.get_context('spawn')
    port = _free_port()
    procs = [ctx.Process(target=run_rank, args=(r, world, port, case, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=1500)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
    assert codes == [0] * world, 'rank exit codes %r' % (codes,)
    return [torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False) for r in range(world)]


def _plain(case, world, dev, steps):
    """the single-device path on the global batch (live sessions only)"""
    ops, train, optim = pkg('ops'), pkg('train'), pkg('optim')
    ops.set_precision(case.get('precision', 'fp32'))
    build, collate, samples, V = make_case(case)
    live = live_samples(samples, world, bool(case.get('partial')))
    inputs, labels = collate(None)(live)
    inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
    model = build().to(dev)
    opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model, fuse_projection=True)
    model.train()
    out = []
    for step in range(steps):
        opt.zero_grad()
        loss = model.fused_loss(*inputs, labels)
        loss.backward()
        rec = dict(loss=float(loss.item()))
        if step == 0:
            rec['dE'] = model.table_grad.buf.detach().cpu().clone()
            rec['grads'] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()
                            if p.grad is not None and p is not model._table()}
        opt.step()
        rec['table'] = model._table().detach().cpu().clone()
        rec['params'] = {k: p.detach().cpu().clone() for k, p in model.named_parameters() if p is not model._table()}
        out.append(rec)
    model.eval()
    extra = {}
    if not (getattr(model, 'extra', False) or (getattr(model, 'fusion', False) and getattr(model, 'order', 1) > 1)):
        v, i = model.topk(*inputs, k=20)
        extra['topk'] = (v.cpu(), i.cpu())
    if case['kind'] == 'fixture':
        with torch.no_grad():
            extra['logp'] = model(*inputs).cpu()
    return out, extra, live


def _compare(case, world, res, ref, extra, live, gtol=1e-4, ltol=1e-5, bf16=False):
    samples = make_case(case)[2]
    off = 0
    for r, out in enumerate(res):
        lo, hi = out['lo'], out['hi']
        assert out['n_live'] == hi - lo and (r == 0) == (lo == 0)
        s0, r0 = out['steps'][0], ref[0]
        assert abs(s0['loss'] - r0['loss']) <= ltol * max(1.0, abs(r0['loss'])), (r, s0['loss'], r0['loss'])
        if bf16:
            # different item tilings per shard: bf16 products are the same, fp32 accumulation order differs
            rel = (s0['dE'] - r0['dE'][lo:hi]).norm() / r0['dE'][lo:hi].norm().clamp(min=1e-20)
            assert rel < 2e-3, ('table grad', r, float(rel))
        else:
            close(s0['dE'], r0['dE'][lo:hi], rtol=gtol, atol=1e-7, what='rank %d: table gradient rows [%d, %d)' % (r, lo, hi))
        for k, g in r0['grads'].items():
            assert k in s0['grads'], 'rank %d: replicated gradient %s missing from the bucket' % (r, k)
            if bf16:
                rel = (s0['grads'][k] - g).norm() / g.norm().clamp(min=1e-20)
                assert rel < 5e-3, (k, r, float(rel))
            else:
                close(s0['grads'][k], g, rtol=gtol, atol=1e-7, what='rank %d: all-reduced gradient of %s' % (r, k))
        for si, (s, rr) in enumerate(zip(out['steps'], ref)):
            assert abs(s['loss'] - rr['loss']) <= (5e-4 if bf16 else ltol * 4) * max(1.0, abs(rr['loss'])), (r, si, s['loss'], rr['loss'])
            if not bf16:
                adam_close(s['table'], rr['table'][lo:hi], steps=si + 1, what='rank %d step %d: table rows' % (r, si))
                for k, p in rr['params'].items():
                    adam_close(s['params'][k], p, steps=si + 1, what='rank %d step %d: %s' % (r, si, k))
        n_live = len(rank_slice(samples, world, r, bool(case.get('partial')))[0])
        if 'topk' in extra and 'topk' in out:
            v, i = out['topk']
            rv, ri = extra['topk']
            if not bf16:
                same = (i[:n_live] == ri[off:off + n_live]).float().mean().item()
                assert same > 0.995, 'rank %d: top-20 ids agree on %.4f' % (r, same)     # (an fp32 near-tie may swap two neighbours)
                close(v[:n_live], rv[off:off + n_live], rtol=1e-5, atol=1e-5, what='rank %d: top-20 scores' % r)
        if 'logp' in extra and 'logp' in out and not bf16:
            close(out['logp'][:n_live], extra['logp'][off:off + n_live], rtol=1e-4, atol=1e-4, what='rank %d: log-probs' % r)
        off += n_live
    assert off == len(live)


FIXTURE_CASES = [
    ('msgifsr_K3_s32', 2, {}),
    ('msgifsr_K3_s32', 8, {}),
    ('msgifsr_K3_fus_s32', 2, {}),
    ('msgifsr_K3_ext_s32', 2, {}),
    ('msgifsr_K3_edge', 2, {}),
    ('niser_s32', 2, {}),
    ('msgifsr_K3_s32', 2, dict(partial=True)),                       # exact layouts: filler sessions with label -1
    ('msgifsr_K3_s32', 8, dict(partial=True, padded=True)),          # capacity-padded layouts: fewer live sessions
    ('msgifsr_K3_s32', 2, dict(dead=True)),                          # relations without edges on one rank
]


@pytest.mark.parametrize('name,world,opts', FIXTURE_CASES)
def test_sharded_ranks_on_one_gpu_match_the_single_device_step(dev, tmp_path, name, world, opts):
    case = dict(kind='fixture', name=name, steps=2, **opts)
    res = _launch(world, case, tmp_path)
    ref, extra, live = _plain(case, world, dev, 2)
    _compare(case, world, res, ref, extra, live)
    # the exchange really happened: > 0 collectives per step, the same count on every rank
    counts = {out['steps'][1]['collectives']['count'] for out in res}
    assert len(counts) == 1 and min(counts) >= 5, counts
    # the replicated gradients travel in three buckets in backward completion order (dist.VocabParallel.sync_replicated_grads),
    # with the same byte layout on every rank; MSGIFSR's first two (read-out head, MSHGNN layers) are issued from INSIDE the
    # backward pass (ops.grad_mark -> bucket_ready) on every rank whose batch gives all their parameters a gradient - from the
    # second step on (the first agrees on the layout)
    lay = {tuple(out['steps'][1]['buckets']) for out in res}
    assert len(lay) == 1 and len(next(iter(lay))) == 3 and sum(next(iter(lay))) > 0, lay
    if name.startswith('msgifsr') and '_fus' not in name and '_ext' not in name and not opts:
        assert all(b > 0 for b in next(iter(lay))), lay
        assert all(out['steps'][1]['early'] == 2 for out in res), [out['steps'][1]['early'] for out in res]
    if opts.get('dead'):
        # the short-session rank has no edges of the higher-order relations; in a multi-rank job every relation of the schema
        # counts as live (it is, in the global batch: msgifsr.MSHGNN.plan), so its nodes still get those relations' residual
        # and bias terms and the rank still lands on the single-device parameters (checked by _compare)
        assert any('intra3' in k for k in ref[0]['grads'])


@pytest.mark.parametrize('precision,world', [('fp32', 2), ('bf16', 2), ('bf16', 8)])
def test_sharded_ranks_at_the_benchmarked_shape(dev, tmp_path, precision, world):
    """config C3's shape (V = 37 484, d = 256, order 3, 512 sessions in total) split over W row shards"""
    case = dict(kind='synth', V=37484, d=256, order=3, B=512, precision=precision, steps=1, padded=True)
    try:
        res = _launch(world, case, tmp_path)
        ref, extra, live = _plain(case, world, dev, 1)
        _compare(case, world, res, ref, extra, live, bf16=(precision == 'bf16'))
    finally:
        pkg('ops').set_precision('fp32')


# ---- config C5 (BASELINE.json configs[4]): synthetic 10 M-item catalog, sessions of <= 50 clicks, d = 256, 8 row shards.
#      Neither a rank's 1.25 M x 256 rows nor the single device's 10 M x 256 (2.56 G elements: 64-bit offsets) travel whole;
#      every matrix is compared through float64 row sums + row norms of ALL rows and the full contents of a stride sample of
#      ~4096 rows + every row the batch touches (dist_gpu_worker.digest).
def _plain_big(case, world, dev, steps):
    D, ops, train, optim = pkg('dist'), pkg('ops'), pkg('train'), pkg('optim')
    ops.set_precision(case.get('precision', 'fp32'))
    build, collate, samples, V = make_case(case)
    live = live_samples(samples, world, False)
    touched = touched_items(samples)
    inputs, labels = collate(None)(live)
    inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
    model = build_on(build, dev, True)
    opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model, fuse_projection=True)
    model.train()

    def per_shard(mat):
        out = []
        for r in range(world):
            lo, hi, _ = D.shard_bounds(V, world, r)
            out.append(digest(mat[lo:hi], digest_rows(hi - lo, lo, touched)))
        return out
    recs = []
    for step in range(steps):
        opt.zero_grad()
        loss = model.fused_loss(*inputs, labels)
        loss.backward()
        rec = dict(loss=float(loss.item()))
        if step == 0:
            rec['dE'] = per_shard(model.table_grad.buf)
            rec['grads'] = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()
                            if p.grad is not None and p is not model._table()}
        opt.step()
        rec['table'] = per_shard(model._table().detach())
        rec['params'] = {k: p.detach().cpu().clone() for k, p in model.named_parameters() if p is not model._table()}
        recs.append(rec)
    model.eval()
    v, i = model.topk(*inputs, k=20)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    return recs, dict(topk=(v.cpu(), i.cpu())), live, peak


def _vec_close(a, b, tol, what):
    rel = float((a.double() - b.double()).norm() / b.double().norm().clamp(min=1e-30))
    assert rel <= tol, '%s: norm-wise relative error %.3e > %.1e' % (what, rel, tol)


def _compare_big(case, world, res, ref, extra, bf16):
    samples = make_case(case)[2]
    tol = 2e-3 if bf16 else 1e-5                          # norm-wise, whole vectors / row blocks
    off = 0
    for r, out in enumerate(res):
        s0, r0 = out['steps'][0], ref[0]
        assert abs(s0['loss'] - r0['loss']) <= (5e-4 if bf16 else 1e-5) * max(1.0, abs(r0['loss'])), (r, s0['loss'], r0['loss'])
        a, b = s0['dE'], r0['dE'][r]
        assert torch.equal(a['idx'], b['idx']) and a['rows'].shape[0] > 4000
        _vec_close(a['rowsum'], b['rowsum'], tol * 5, 'rank %d: row sums of the table gradient (all %d rows)' % (r, len(a['rowsum'])))
        _vec_close(a['rownorm'], b['rownorm'], tol, 'rank %d: row norms of the table gradient' % r)
        if bf16:
            _vec_close(a['rows'], b['rows'], tol, 'rank %d: sampled + touched rows of the table gradient' % r)
        else:
            close(a['rows'], b['rows'], rtol=1e-4, atol=1e-7, what='rank %d: sampled + touched rows of the table gradient' % r)
        for k, g in r0['grads'].items():
            assert k in s0['grads'], 'rank %d: replicated gradient %s missing from the bucket' % (r, k)
            if bf16:
                _vec_close(s0['grads'][k], g, 5e-3, 'rank %d: all-reduced gradient of %s' % (r, k))
            else:
                close(s0['grads'][k], g, rtol=1e-4, atol=1e-7, what='rank %d: all-reduced gradient of %s' % (r, k))
        for si, (s, rr) in enumerate(zip(out['steps'], ref)):
            assert abs(s['loss'] - rr['loss']) <= (5e-4 if bf16 else 4e-5) * max(1.0, abs(rr['loss'])), (r, si, s['loss'], rr['loss'])
            ta, tb = s['table'], rr['table'][r]
            if bf16:
                # Adam's first steps move every element by ~lr whatever its gradient: bf16 round-off in a near-zero gradient
                # component flips its sign - bounded movement, and the rows' norms barely change
                assert float((ta['rows'] - tb['rows']).abs().max()) <= 2.2e-3 * (si + 1)
                _vec_close(ta['rownorm'], tb['rownorm'], 1e-3, 'rank %d step %d: row norms of the table' % (r, si))
            else:
                adam_close(ta['rows'], tb['rows'], steps=si + 1, what='rank %d step %d: sampled + touched table rows' % (r, si))
                _vec_close(ta['rownorm'], tb['rownorm'], 1e-5, 'rank %d step %d: row norms of the table' % (r, si))
                for k, p in rr['params'].items():
                    # 512 sessions of up to 49 clicks: ~7 k node rows feed every encoder gradient, and the two ranks' halves are
                    # summed in another order than on one device.  Adam's first steps move an element by ~lr whatever its
                    # size, so a gradient component that cancels to ~0 may step with either sign (the gradients themselves
                    # are compared above at 1e-4): 99.9 % of the elements within 2e-6, none further than a full flip
                    a_, b_ = s['params'][k].float(), p.float()
                    err = (a_ - b_).abs()
                    frac = (err <= 2e-6 + 1e-4 * b_.abs()).float().mean().item()
                    # (the second step starts from weights that already differ in those components: 99 % there)
                    assert frac >= (0.999 if si == 0 else 0.99), 'rank %d step %d: %s: only %.5f of the elements within 2e-6' % (r, si, k, frac)
                    assert err.max().item() <= 2.02e-3 * (si + 1), 'rank %d step %d: %s: max err %.3e' % (r, si, k, err.max().item())
        n_live = len(rank_slice(samples, world, r, False)[0])
        v, i = out['topk']
        rv, ri = extra['topk']
        hits = sum(len(set(i[b].tolist()) & set(ri[off + b].tolist())) for b in range(n_live)) / (20.0 * n_live)
        assert hits >= (0.97 if bf16 else 0.995), 'rank %d: top-20 sets overlap %.4f' % (r, hits)
        if not bf16:
            # (scores 12 cos(.) of models that have taken two Adam steps from weights equal to ~1e-6)
            close(v[:n_live], rv[off:off + n_live], rtol=1e-4, atol=1e-4, what='rank %d: top-20 scores' % r)
        off += n_live


C5 = dict(kind='synth', d=256, order=3, B=512, max_len=50, mean_len=14.0, padded=True, big=True)


@pytest.mark.parametrize('precision,world,V,steps', [('bf16', 8, 10_000_000, 1), ('fp32', 2, 1_000_000, 2)])
def test_sharded_ranks_at_the_c5_shape(dev, tmp_path, precision, world, V, steps):
    """config C5 on the one GPU: 8 rank processes x 1.25 M rows (bf16, the benchmarked arithmetic) against the single-device
    step over all 10 M rows - 2.56 G table elements, i.e. every kernel that walks the table runs past 32-bit element
    offsets (lookup over 10 M ids, adam_rows, renorm + bf16 copy, flash-CE, top-k) - and a 2-shard fp32 run at 1 M rows
    with the tight tolerances.  /root/reference/src/utils/train.py:94-101, src/models/msgifsr.py:276-321."""
    case = dict(C5, V=V, precision=precision, steps=steps)
    smp = make_case(case)[2]
    assert max(len(s) for s, _ in smp) >= 40              # the batch really holds long sessions
    try:
        res = _launch(world, case, tmp_path)
        ref, extra, live, peak = _plain_big(case, world, dev, steps)
        _compare_big(case, world, res, ref, extra, bf16=(precision == 'bf16'))
        print('single-device peak memory %.1f GiB' % peak)
        # 6 exchanges of the sharded table + 3 gradient buckets per step (+ the one-off agreement on the bucket layout in the
        # first step)
        counts = {out['steps'][-1]['collectives']['count'] for out in res}
        assert counts == ({10} if steps == 1 else {9}), counts
    finally:
        pkg('ops').set_precision('fp32')
        torch.cuda.empty_cache()


def test_rank_5_of_the_c5_job_replayed_under_hipgraph_capture(dev, tmp_path):
    """rank 5 of the 8-rank C5 job (rows [6.25 M, 7.5 M) of the 10 M-row table, bf16), re-run alone from the recorded
    collective results: step 1 eagerly, step 2 captured + replayed - the launch mode of bench.py on an 8-GPU node."""
    D, G, ops, train, optim = pkg('dist'), pkg('graph'), pkg('ops'), pkg('train'), pkg('optim')
    world, rank = 8, 5
    case = dict(C5, V=10_000_000, precision='bf16', steps=2, record=True)
    try:
        res = _launch(world, case, tmp_path)
        job = res[rank]
        ops.set_precision('bf16')
        build, collate, samples, V = make_case(case)
        mine, n = rank_slice(samples, world, rank, False)
        caps = pkg('collate').default_caps(n, case['max_len'])
        inputs, labels = collate(caps)(mine)
        inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
        model = build_on(build, dev, True)
        group = D.ReplayGroup(world, rank, dev, rtol=2e-3, atol=1e-5).load(job['steps'][0]['tape'])
        vp = D.VocabParallel(model, group=group, idx_cap=inputs[0].cap('uniq_items'))
        torch.cuda.empty_cache()
        assert (vp.lo, vp.hi) == (job['lo'], job['hi']) == D.shard_bounds(V, world, rank)[:2] and vp.lo > 6_000_000
        rows = job['steps'][0]['table']['idx'].to(dev)
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model, fuse_projection=True)
        replicated = [p for p in model.parameters() if p is not model._table() and p.requires_grad]
        model.train()
        opt.zero_grad()
        loss = model.fused_loss(*inputs, labels)
        loss.backward()
        vp.sync_replicated_grads(replicated, opt)
        opt.step()
        assert group.pos == len(group.kinds) and group.checked == len(group.kinds)
        assert abs(loss.item() - job['steps'][0]['loss']) <= 1e-5 * max(1.0, abs(job['steps'][0]['loss']))
        del loss
        # same kernels on the same inputs as inside the job (up to the order in which 8 processes' atomics-free reductions
        # ran: none): the rows agree to fp32 round-off
        close(model._table().detach()[rows], job['steps'][0]['table']['rows'], rtol=1e-5, atol=1e-6, what='table rows after the eager step')
        group.load(job['steps'][1]['tape'])
        gs = G.GraphedTrainStep(model, opt, inputs, labels, after_backward=lambda: vp.sync_replicated_grads(replicated, opt),
                                warmup=1)
        loss2 = gs(inputs, labels)
        torch.cuda.synchronize()
        assert abs(loss2.item() - job['steps'][1]['loss']) <= 1e-5 * max(1.0, abs(job['steps'][1]['loss'])), \
            (loss2.item(), job['steps'][1]['loss'])
        close(model._table().detach()[rows], job['steps'][1]['table']['rows'], rtol=1e-5, atol=1e-6, what='table rows after the replayed step')
        rn = model._table().detach()[:vp.n_live].double().norm(dim=1).cpu()
        _vec_close(rn, job['steps'][1]['table']['rownorm'], 1e-6, 'row norms of all 1.25 M rows after the replayed step')
        nodes = gs.node_counts()
        if nodes is not None:
            assert nodes['kernel'] > 10
    finally:
        ops.set_precision('fp32')
        torch.cuda.empty_cache()


@pytest.mark.parametrize('name,world,rank', [('msgifsr_K3_s32', 2, 1), ('msgifsr_K3_s32', 8, 5), ('niser_s32', 2, 1)])
def test_one_rank_of_the_job_replayed_under_hipgraph_capture(dev, tmp_path, name, world, rank):
    """rank `rank` of a W-rank job, re-run alone from the recorded collective results: step 1 eagerly (every collective
    input is checked against what the rank handed in inside the job), step 2 as a captured and replayed hipGraph -
    the launch mode of bench.py / TrainRunner - and the rank must land where it landed inside the job."""
    D, G, train, optim = pkg('dist'), pkg('graph'), pkg('train'), pkg('optim')
    case = dict(kind='fixture', name=name, steps=2, padded=True, record=True)
    res = _launch(world, case, tmp_path)
    job = res[rank]
    assert job['lo'] > 0
    build, collate, samples, V = make_case(case)
    mine, n = rank_slice(samples, world, rank, False)
    caps = pkg('collate').default_caps(n, 20)
    inputs, labels = collate(caps)(mine)
    inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
    model = build().to(dev)
    group = D.ReplayGroup(world, rank, dev).load(job['steps'][0]['tape'])
    vp = D.VocabParallel(model, group=group, idx_cap=inputs[0].cap('uniq_items'))
    assert (vp.lo, vp.hi) == (job['lo'], job['hi'])
    # the early gradient buckets on a SIDE stream (what an RCCL job does), forked and joined inside the captured step
    vp.side_stream = name.startswith('msgifsr')
    opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model, fuse_projection=True)
    replicated = [p for p in model.parameters() if p is not model._table() and p.requires_grad]
    model.train()
    # step 1, eager
    opt.zero_grad()
    loss = model.fused_loss(*inputs, labels)
    loss.backward()
    vp.sync_replicated_grads(replicated, opt)
    opt.step()
    assert group.pos == len(group.kinds) and group.checked == len(group.kinds)
    assert abs(loss.item() - job['steps'][0]['loss']) <= 1e-6 * max(1.0, abs(job['steps'][0]['loss']))
    del loss          # (a live loss of an eager default-stream step must not outlive into the capture: graph.GraphedTrainStep)
    # (inside the job the row-normalisation projection of the table gradient ran as a separate pass - the worker materialises
    # model.table_grad to record it - here it is fused into the optimizer's row pass: two roundings of the same algebra.  A
    # component whose projected gradient cancels to ~eps (1e-8) turns a last-bit difference into ~0.1 % of its first Adam step
    # of lr = 1e-3, d step / d g = eps / (|g| + eps)^2: hence 3e-6 absolute on the table here and - the second step starts
    # from those rows - below; the replicated parameters keep the tight bound)
    close(model._table().detach()[:vp.n_live], job['steps'][0]['table'], rtol=1e-6, atol=3e-6, what='table rows after the eager step')
    # step 2, captured (one eager warm-up lap with checks, one capture lap) and replayed
    group.load(job['steps'][1]['tape'])
    gs = G.GraphedTrainStep(model, opt, inputs, labels, after_backward=lambda: vp.sync_replicated_grads(replicated, opt),
                            warmup=1)
    assert group.pos == 2 * len(group.kinds) and group.checked == len(group.kinds)
    loss2 = gs(inputs, labels)
    torch.cuda.synchronize()
    assert abs(loss2.item() - job['steps'][1]['loss']) <= 1e-6 * max(1.0, abs(job['steps'][1]['loss'])), \
        (loss2.item(), job['steps'][1]['loss'])
    close(model._table().detach()[:vp.n_live], job['steps'][1]['table'], rtol=1e-6, atol=3e-6, what='table rows after the replayed step')
    for k, p in model.named_parameters():
        if p is not model._table():
            close(p, job['steps'][1]['params'][k], rtol=1e-6, atol=1e-7, what='replayed step: ' + k)
    nodes = gs.node_counts()
    if nodes is not None:
        assert nodes['kernel'] > 10
    if name.startswith('msgifsr'):
        assert vp.early_launches >= 2 and vp._side is not None      # buckets 0 and 1 left from inside the (captured) backward


@pytest.mark.parametrize('world,rank', [(2, 1), (8, 5)])
def test_step_rider_in_a_captured_row_sharded_step_with_dropout(dev, tmp_path, monkeypatch, world, rank):
    """The optimizer's step-scalar kernel rides in the END-of-backward slab-sum launch of a captured step
    (optim.FusedAdam.hyper_rider).  It advances the (0, 0) step counter the dropout masks are keyed by, and in a row-sharded
    step the gradient buckets flush the deferred slab sums from INSIDE the backward (dist.VocabParallel.bucket_ready): were the
    rider to leave with such a flush, the GAT layers' backward and the sharded lookup's backward behind it would re-derive their
    masks from the next step's counter.  Rank `rank` of a W-rank job with feature, attention and lookup dropout at the width
    whose backward defers slab sums (bf16 matmuls, d = 128, order 3), re-run from its tape and captured twice - with and
    without the rider - must land BIT-identically after several replays: table rows, replicated parameters, the losses of the
    loss ring and the step counter, and - since under replay every collective's RESULT comes from the tape, so that the
    parameters follow the job whatever this rank's own backward computed - what the captured step hands IN to each of its
    collectives: the lookup's masked per-item gradient rows and the gradient buckets."""
    D, G, ops, train, optim = pkg('dist'), pkg('graph'), pkg('ops'), pkg('train'), pkg('optim')
    p = 0.2
    # (512 sessions per rank, the benchmarked batch: the read-out head's weight gradients are split-K sums that wait for a flush)
    case = dict(kind='synth', V=5000, d=128, order=3, B=512 * world, precision='bf16', dropout=p, steps=2, padded=True,
                record=True)
    replays = 5

    class Tapped(D.ReplayGroup):
        """under replay every collective's RESULT comes from the tape, so the rank's parameters follow the job whatever its own
        backward computed: what the captured step hands IN to each collective is copied into static buffers by the graph
        itself (they hold the last replay's inputs) - among them the lookup's per-item gradient rows and the gradient buckets"""

        def load(self, tape):
            self.taps = []
            return super().load(tape)

        def collective(self, kind, t):
            if t.is_cuda and torch.cuda.is_current_stream_capturing():
                keep = torch.empty_like(t)
                keep.copy_(t)
                self.taps.append((kind, keep))
            return super().collective(kind, t)

    try:
        res = _launch(world, case, tmp_path)
        job = res[rank]
        assert job['lo'] > 0
        ops.set_precision('bf16')
        build, collate, samples, V = make_case(case)
        mine, n = rank_slice(samples, world, rank, False)
        caps = pkg('collate').default_caps(n, 20)
        inputs, labels = collate(caps)(mine)
        inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
        runs = {}
        for rider in ('0', '1'):
            monkeypatch.setenv('SREC_HYPER_RIDER', rider)
            model = build().to(dev)
            group = Tapped(world, rank, dev).load(job['steps'][0]['tape'])
            vp = D.VocabParallel(model, group=group, idx_cap=inputs[0].cap('uniq_items'))
            vp.side_stream = True
            opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model, fuse_projection=True)
            replicated = [q for q in model.parameters() if q is not model._table() and q.requires_grad]
            model.train()
            # step 1, eager, with the job's nonces (every collective input is checked against the tape)
            reseed(step_seed(0))
            ops.DROP_TAP = []
            try:
                opt.zero_grad()
                loss = model.fused_loss(*inputs, labels)
                loss.backward()
                taps = ops.DROP_TAP
            finally:
                ops.DROP_TAP = None
            vp.sync_replicated_grads(replicated, opt)
            opt.step()
            assert group.pos == len(group.kinds) and group.checked == len(group.kinds)
            assert abs(loss.item() - job['steps'][0]['loss']) <= 1e-6 * max(1.0, abs(job['steps'][0]['loss']))
            del loss
            # dropout really is on: the GAT layer's feature masks drop ~p and scale the rest by 1 / (1 - p)
            assert len(taps) >= 1
            ms = taps[0]['ms']
            assert abs((ms == 0).float().mean().item() - p) < 0.03
            assert torch.allclose(ms[ms != 0], torch.full_like(ms[ms != 0], 1 / (1 - p)), rtol=1e-6)
            # step 2: the eager warm-up lap draws the job's nonces of step 2 (its collective inputs are checked against the
            # tape), then the capture; the replays run on the recorded collective results
            group.load(job['steps'][1]['tape'])
            reseed(step_seed(1))
            early0 = vp.early_launches
            gs = G.GraphedTrainStep(model, opt, inputs, labels, after_backward=lambda: vp.sync_replicated_grads(replicated, opt),
                                    warmup=1)
            assert group.pos == 2 * len(group.kinds) and group.checked == len(group.kinds)
            # buckets 0 and 1 left from inside the backward: in the warm-up lap and in the capture
            assert vp.early_launches - early0 >= 4 and vp._side is not None, (early0, vp.early_launches)
            losses = [gs(inputs, labels).item() for _ in range(replays)]
            torch.cuda.synchronize()
            gs.check()
            nodes = gs.node_counts()
            runs[rider] = dict(table=model._table().detach()[:vp.n_live].clone(),
                               params={k: q.detach().clone() for k, q in model.named_parameters() if q is not model._table()},
                               losses=losses, ring=gs.loss_ring.clone(),
                               counter=int(opt._hyper[(0, 0)]['counter'].item()), kernels=nodes['kernel'] if nodes else None,
                               taps=[(k, t.clone()) for k, t in group.taps])
            del gs, model, opt, vp
            torch.cuda.empty_cache()
        r0, r1 = runs['0'], runs['1']
        diffs = {'table': (r0['table'] - r1['table']).abs().max().item()}
        for k in r0['params']:
            diffs[k] = (r0['params'][k] - r1['params'][k]).abs().max().item()
        kinds = [k for k, _ in r0['taps']]
        assert kinds == [k for k, _ in r1['taps']] and 'all_gather' in kinds and 'all_reduce:SUM' in kinds, kinds
        for i, ((k, a), (_, b)) in enumerate(zip(r0['taps'], r1['taps'])):
            diffs['collective %d (%s) input' % (i, k)] = (a.double() - b.double()).abs().max().item() if a.numel() else 0.0
        worst = sorted(diffs.items(), key=lambda kv: -kv[1])[:6]
        print('rider on vs off: largest differences', worst, 'kernels', r0['kernels'], r1['kernels'])
        # the rider IS taken in the captured step (one kernel node less) - else the comparison below would hold by construction
        if r0['kernels'] is not None:
            assert r1['kernels'] == r0['kernels'] - 1, (r0['kernels'], r1['kernels'])
        # what this rank hands in to every collective of the replayed step - the masked per-item rows of the lookup backward, the
        # gradient buckets of the GAT layers and the GRUs - is the same with and without the rider
        for i, ((k, a), (_, b)) in enumerate(zip(r0['taps'], r1['taps'])):
            assert torch.equal(a, b), 'input of collective %d (%s) differs with the rider: %r' % (i, k, worst)
        assert r0['counter'] == r1['counter'] == 1 + replays, (r0['counter'], r1['counter'])   # (the eager step + the replays)
        assert torch.equal(r0['table'], r1['table']), 'table rows differ with the rider: %r' % (worst,)
        for k in r0['params']:
            assert torch.equal(r0['params'][k], r1['params'][k]), '%s differs with the rider: %r' % (k, worst)
        assert torch.equal(r0['ring'], r1['ring']) and r0['losses'] == r1['losses']
        assert bool(torch.isfinite(torch.tensor(r0['losses'])).all()), r0['losses']
    finally:
        ops.DROP_TAP = None
        ops.set_precision('fp32')
        torch.cuda.empty_cache()


def test_bench_two_ranks_over_gloo_on_one_gpu(dev):
    """`python bench.py --gpus 2` for real (not --launch-only): the launcher re-executes itself under torch.distributed.run
    with two ranks, both on cuda:0, collectives over gloo staged through the host (SREC_BENCH_BACKEND=gloo) - the complete
    N-rank line (`n_gpus`, `ranks_seen`, `collectives`, `scaling`, `config.global_batch`) is produced once before an 8-GPU
    node ever runs it.  Host-staged collectives cannot be captured in a hipGraph, so this run also takes bench.py's
    "capture of the collectives refused" branch: both ranks agree to fall back, and the EAGER steps with the 9 collectives
    train to a finite loss."""
    import json
    import subprocess
    import sys
    from util import ROOT
    env = dict(os.environ, SREC_BENCH_BACKEND='gloo')
    env.pop('WORLD_SIZE', None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1',
                        '--repeats', '1', '--no-cpu-baseline', '--full'], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=1200)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['ranks_seen'] == 2 and out['scaling'] == 'weak'
    assert out['unit'] == 'sessions/s' and out['value'] > 0 and out['steps'] == 3
    assert out['config']['global_batch'] == 1024 and 'row-sharded x2' in out['config']['parallelism']
    c = out['collectives']
    assert c['count'] == 9 and c['backend'] == 'gloo' and c['captured_in_graph'] is False and c['bytes'] > 0
    # the replicated gradients travel as three all-reduces in backward completion order: read-out head, MSHGNN layers, rest
    assert len(c['buckets']) == 3 and all(b > 0 for b in c['buckets']) and c['buckets'][1] > c['buckets'][0]
    assert out['launch'] == 'eager' and 'graph capture with the collectives failed' in p.stderr
    assert 1.0 < out['config']['final_loss'] < 12.0          # ~ln V at the start of training
    assert out['roofline']['frac'] > 0 and out['cpu_baseline'] is None and out['fp32'] is None
    # round 6: the line carries the whole metric - the agreed capture verdict, a correctness bit (row-sharded loss of the first
    # global batch vs the single-device loss rank 0 computes on the same 1024 sessions), per-exchange times of eager steps, and
    # the STRONG-scaling point (the reference's own 512-session batch, train.py:94-101) next to the weak one
    assert c['captured_on_all_ranks'] is False and c['capture_attempts'] == 1
    ok = out['correctness']
    assert ok['ok'] and ok['sessions'] == 1024 and ok['rel_err'] <= ok['tol'], ok
    t = c['timed']
    assert len(t['per_exchange']) == 9 and all(e['us'] > 0 for e in t['per_exchange']) and t['sum_us'] > 0
    assert [e['kind'] for e in t['per_exchange']].count('all_reduce') == 3
    st = out['strong']
    assert st['scaling'] == 'strong' and st['global_batch'] == 512 and st['sessions_encoded_per_rank'] == 256
    assert st['value'] > 0 and st['collectives']['count'] == 9 and st['correctness']['ok'] and st['correctness']['sessions'] == 512
    assert 1.0 < st['final_loss'] < 12.0
