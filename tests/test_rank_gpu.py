"""Full-catalog target-rank evaluation on the GPU (csrc/rank.hip through ops.score_rank, model.target_rank,
dist.VocabParallel.target_rank and train.evaluate(method='rank')) against materialised float64 scores.

Exact inputs (every product and sum representable) must give EQUAL ranks - off-by-one, lost tail tiles and the tie
direction show there.  Random inputs are checked by the interval every rank consistent with scores known to +-1e-4 (the
fp32 round-off bound of tests/test_ops_gpu.py's top-K test at these magnitudes) must fall in."""
import os

import numpy as np
import pytest
import torch

from rank_oracle import assert_in_interval, rank_interval, ranks_exact, scores64
from util import GOLDEN, ROOT, load_golden, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _ops():
    return pkg('ops')


# ------------------------------------------------------------------------------------------- 1) exact case
def _exact_case(B, V, d, dev):
    g = torch.Generator().manual_seed(B * 7 + V)
    sr = torch.randint(-8, 9, (B, d), generator=g).float() / 8
    E = torch.randint(-8, 9, (V, d), generator=g).float() / 8
    cs = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (V,), generator=g)]
    dup = [(3, 17)] + ([(100, 101)] if V > 101 else [])
    for a, b in dup:
        E[b], cs[b] = E[a], cs[a]
    labels = torch.randint(0, V, (B,), generator=g)
    fixed = [x for p in dup for x in p] + [0, V - 1, -1, -1]
    pos = torch.randperm(B, generator=g)[:len(fixed)]
    for p, x in zip(pos.tolist(), fixed[:B]):
        labels[p] = x
    return sr, E, cs, labels


@pytest.mark.parametrize('B,V,d', [(5, 300, 32), (33, 5000, 96), (3, 20, 32), (64, 37484, 256)])
def test_exact_inputs_give_equal_ranks(dev, B, V, d):
    ops = _ops()
    sr, E, cs, labels = _exact_case(B, V, d, dev)
    if B >= 8:
        assert sorted(set(labels.tolist()) & {0, 3, 17, V - 1}) == sorted({0, 3, 17, V - 1}) and (labels < 0).sum() >= 2
    rank, target = ops.score_rank(sr.to(dev), E.to(dev), cs.to(dev), labels.to(dev))
    s64 = scores64(sr, E, cs)
    ref = ranks_exact(s64, labels)
    t64 = s64.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    live = labels >= 0
    print('exact', (B, V, d), 'rank', rank.tolist()[:12], 'ref', ref.tolist()[:12])
    assert rank.dtype == torch.int32 and target.dtype == torch.float32
    assert torch.equal(rank.cpu().long(), ref)
    assert torch.equal(target.cpu()[live].double(), t64[live])
    # the same answer without the column scale
    rank1, _ = ops.score_rank(sr.to(dev), E.to(dev), None, labels.to(dev))
    assert torch.equal(rank1.cpu().long(), ranks_exact(scores64(sr, E), labels))


@pytest.mark.parametrize('B,V,d,C', [(37, 700, 100, 2), (40, 600, 512, 4), (33, 500, 1024, 2)])
def test_exact_mixture_inputs_on_every_kernel_path(dev, B, V, d, C):
    """the paths the shapes above do not reach: a d that is no multiple of the 32-column group (zero-padded tail), C = 2 and
    C = 4, and session tiles beyond the LDS budget that are read through the cache (C = 4, d = 512; C = 2, d = 1024).
    Exact inputs again; session b's component b % C carries an offset that is a multiple of 1/8 and the others -1e5, so
    exp() of the others is exactly 0 in fp32 and in the float64 oracle alike and the mixture is exact: ranks must be EQUAL,
    and every component's accumulator tile is the deciding one for some session."""
    ops = _ops()
    sr, E, cs, labels = _exact_case(B, V, d, dev)
    g = torch.Generator().manual_seed(d + C)
    srs = torch.randint(-8, 9, (C, B, d), generator=g).float() / 8
    srs[0] = sr
    off = torch.full((C, B), -1.0e5)
    off[torch.arange(B) % C, torch.arange(B)] = -torch.randint(0, 9, (B,), generator=g).float() / 8
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    listed[:, 4] = -1
    off_in = off.clone()
    off_in[torch.arange(B) % C, torch.arange(B)] += 2.0
    for lst, oi in ((None, None), (listed, off_in)):
        t = lambda x: None if x is None else x.to(dev)
        rank, target = ops.score_rank(srs.to(dev), E.to(dev), cs.to(dev), labels.to(dev), off.to(dev), t(oi), t(lst))
        s64 = scores64(srs, E, cs, off, oi, lst)
        ref = ranks_exact(s64, labels)
        live = labels >= 0
        print('exact mix', (B, V, d, C), 'listed' if lst is not None else 'plain', rank.tolist()[:10], ref.tolist()[:10])
        assert torch.equal(rank.cpu().long(), ref)
        assert torch.equal(target.cpu()[live].double(), s64.gather(1, labels.clamp(min=0)[:, None])[:, 0][live])


# ------------------------------------------------------------------------------------------- 2) random case, interval check
def _random_case(B, V, d, kind, dev):
    g = torch.Generator().manual_seed(B + V + len(kind))
    C = 1 if kind == 'single' else 3
    srs = torch.randn(C, B, d, generator=g) * 0.3
    E = torch.randn(V, d, generator=g) * 0.2
    cs = torch.rand(V, generator=g) + 0.5
    labels = torch.randint(0, V, (B,), generator=g)
    off_ex = off_in = listed = None
    if kind != 'single':
        off_ex = -2.0 * torch.rand(C, B, generator=g)
    if kind == 'listed':
        L = 7
        off_in = off_ex + torch.rand(C, B, generator=g) * 3 - 1.0
        listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])       # distinct ids per session
        listed[torch.rand(B, L, generator=g) < 0.25] = -1
        third = torch.arange(B) % 3 == 0
        listed[third, 2] = labels[third]                                                  # the label is in the list ...
        for j in (0, 1, 3, 4, 5, 6):                                                      # ... once
            listed[:, j] = torch.where(listed[:, j] == labels, torch.full_like(labels, -1), listed[:, j])
    return srs, E, cs, labels, off_ex, off_in, listed


@pytest.mark.parametrize('kind', ['single', 'mix3', 'listed'])
@pytest.mark.parametrize('B,V,d', [(33, 5000, 96), (40, 3429, 64)])
def test_random_inputs_rank_inside_the_roundoff_interval(dev, B, V, d, kind):
    ops = _ops()
    srs, E, cs, labels, off_ex, off_in, listed = _random_case(B, V, d, kind, dev)
    g = lambda t: None if t is None else t.to(dev)
    rank, target = ops.score_rank([s.to(dev) for s in srs], g(E), g(cs), g(labels), g(off_ex), g(off_in), g(listed))
    s64 = scores64(srs, E, cs, off_ex, off_in, listed)
    lo, hi = assert_in_interval(rank, s64, labels, TOL, what='%s %s' % (kind, (B, V, d)), max_width=16)
    print(kind, (B, V, d), 'rank', rank.tolist()[:10], 'lo', lo.tolist()[:10], 'hi', hi.tolist()[:10])
    t64 = s64.gather(1, labels[:, None])[:, 0]
    assert float((target.cpu().double() - t64).abs().max()) < TOL
    if kind == 'listed':        # the fix-up pass matters here: without it the ranks leave the interval
        wrong = ranks_exact(scores64(srs, E, cs, off_ex), labels, t64)
        assert int(((wrong < lo) | (wrong > hi)).sum()) > 0


# ------------------------------------------------------------------------------------------- 3) non-contiguous inputs
def test_strided_table_and_session_views(dev):
    ops = _ops()
    B, V, d = 33, 1000, 96
    srs, E, cs, labels, off_ex, off_in, listed = _random_case(B, V, d, 'single', dev)
    Ew = torch.zeros(V, d + 32, device=dev)
    Ew[:, :d] = E.to(dev)
    sw = torch.full((B, d + 8), 7.0, device=dev)
    sw[:, :d] = srs[0].to(dev)
    tv, sv = Ew[:, :d], sw[:, :d]
    assert tv.stride(0) == d + 32 and sv.stride(0) == d + 8 and not tv.is_contiguous()
    r1, t1 = ops.score_rank(sv, tv, cs.to(dev), labels.to(dev))
    r0, t0 = ops.score_rank(sv.contiguous(), tv.contiguous(), cs.to(dev), labels.to(dev))
    assert torch.equal(r1, r0) and torch.equal(t1, t0)
    assert_in_interval(r1, scores64(srs, E, cs), labels, TOL, what='strided')


# ------------------------------------------------------------------------------------------- 4) models against fixtures
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith('.npz') and (f.endswith('_s32.npz') or f.endswith('_edge.npz'))
                  and not f.startswith('srgnn_layer_'))


def _fixture_model(name, dev):
    """the product model with the reference's trained weights: the fixture's `final/` tensors.  The `_s32` fixtures of
    MSGIFSR (all but msgifsr_K3_s32) and lessr_L3_* leave the item table or unused GRU weights out of `final/` (size); for
    those the three fused Adam steps of tests/test_models_gpu.py reproduce the missing tensors first, as that test does
    ahead of its own evaluation check.  Part (a) is the check against the reference there; part (b) compares the fused
    rank with the same model's materialised forward() - two code paths of the product, one set of weights."""
    from test_models_gpu import _build, _collate
    train, optim = pkg('train'), pkg('optim')
    z, samples, init = load_golden(name)
    V = init[[k for k in init if k.startswith('embedding')][0]].shape[0]
    model = _build(name, init, V, dev)
    inputs, labels = _collate(name, samples)
    inputs, labels = [x.to(dev) for x in inputs], labels.to(dev)
    finals = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('final/')}
    sd = model.state_dict()
    if not all(k in finals for k, _ in model.named_parameters()):
        model.train()
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-3, weight_decay=1e-4, model=model)
        for _ in range(3):
            opt.zero_grad()
            model.fused_loss(*inputs, labels).backward()
            opt.step()
        sd = model.state_dict()
    model.load_state_dict({**sd, **{k: v.to(dev) for k, v in finals.items() if k in sd}})
    pkg('ops').weights_changed()           # cached operand copies of the old weights
    model.table_written()                  # ... and the model's notes about its table
    return z, model.eval(), inputs, labels


@pytest.mark.parametrize('name', FIXTURES)
def test_model_target_rank_against_fixture(dev, name):
    z, model, inputs, labels = _fixture_model(name, dev)
    assert 'eval_top20' in z.files
    # (a) the reference's own log-probabilities of the first sessions
    head = torch.from_numpy(z['eval_logprobs_head']).double()
    r = model.target_rank(*inputs, labels=labels)
    assert r.dtype == torch.int32 and r.shape == labels.shape
    assert_in_interval(r[:head.shape[0]], head, labels[:head.shape[0]], TOL, what=name + ' vs reference log-probs')
    # (b) the model's own materialised forward(), labels from both ends of the reference's top-20
    with torch.no_grad():
        s64 = model(*inputs).double().cpu()
    top = torch.from_numpy(z['eval_top20']).long()
    for col in (0, 19):
        lab = top[:, col].to(labels.device)
        r = model.target_rank(*inputs, labels=lab)
        lo, hi = assert_in_interval(r, s64, lab, TOL, what='%s vs forward(), top-20 column %d' % (name, col))
        print(name, 'col', col, 'rank', r.tolist()[:8], 'lo', lo.tolist()[:8], 'hi', hi.tolist()[:8])
        # (c) an item of the reference's top-20 has fewer than 20 items ahead of it
        sure = hi < 20
        assert bool((r.cpu().long()[sure] < 20).all()), (name, col, r.tolist())


# ------------------------------------------------------------------------------------------- 5) evaluate(method='rank')
def test_evaluate_rank_method_reproduces_the_reference_metrics(dev):
    sp, train, col, ds = pkg(), pkg('train'), pkg('collate'), pkg('dataset')
    z = np.load(os.path.join(GOLDEN, 'srgnn_evaluate.npz'))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init/')}
    model = sp.SRGNN(3429, 32, 1)
    model.load_state_dict(init)
    model = model.to(dev)
    data = ds.AugmentedDataset(ds.read_sessions(os.path.join(ROOT, 'tests', 'golden', 'sample_test.txt')))
    fn = col.collate_fn_factory(col.seq_to_session_graph)
    batches = [fn([data[i] for i in range(b * 32, b * 32 + 32)]) for b in range(10)]
    mrr, hit = train.evaluate(model, batches, dev, method='rank')
    print('evaluate(rank):', mrr, hit, 'reference:', float(z['mrr']), float(z['hit']))
    assert abs(mrr - float(z['mrr'])) < 1e-7 and abs(hit - float(z['hit'])) < 1e-9, (mrr, hit, z['mrr'], z['hit'])
    m = train.evaluate(model, batches, dev, method='rank', cutoffs=(5, 10, 20))
    assert m['mrr@20'] == mrr and m['hit@20'] == hit
    ranks = torch.cat([model.target_rank(*[x.to(dev) for x in inp], labels=lab.to(dev)).cpu() for inp, lab in batches]).numpy()
    for k in (5, 10, 20):
        ndcg = float(np.where(ranks < k, 1.0 / np.log2(ranks + 2.0), 0.0).sum() / len(ranks))
        assert abs(m['ndcg@%d' % k] - ndcg) < 1e-12, (k, m['ndcg@%d' % k], ndcg)
        assert abs(m['hit@%d' % k] - float((ranks < k).mean())) < 1e-12


# ------------------------------------------------------------------------------------------- 6) no (B, V) allocation
def test_mixture_target_rank_allocates_no_score_matrix(dev):
    from dist_gpu_worker import synth_samples
    sp, col = pkg(), pkg('collate')
    V, d, B, K = 200000, 32, 64, 3
    torch.manual_seed(3)
    model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
    (mg,), labels = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 5))
    mg, labels = mg.to(dev), labels.to(dev)
    model.target_rank(mg, labels=labels)                 # workspaces and column scales are cached by the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = model.target_rank(mg, labels=labels)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.2f MB, one (B, V) fp32 matrix %.2f MB' % (rise / 2 ** 20, B * V * 4 / 2 ** 20))
    assert rise < B * V * 4 / 4, rise
    assert int(r.min()) >= 0 and int(r.max()) < V
    # today's path, for scale: forward() holds more than three such matrices
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        s = model(mg)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before > 3 * B * V * 4
    assert_in_interval(r, s.double().cpu(), labels, TOL, what='V = 200000 mixture')


# ------------------------------------------------------------------------------------------- 7) sharded, W = 2 on one GPU
@pytest.mark.parametrize('name', ['msgifsr_K3_ext_fus_s32', 'srgnn_s32'])
def test_sharded_target_rank_two_ranks_on_one_gpu_equal_single_device(dev, tmp_path, name):
    import torch.multiprocessing as mp
    from dist_gpu_worker import make_case, rank_slice
    from rank_gpu_worker import run_rank
    from test_dist_gpu import _free_port
    world = 2
    ctx = mp.get_context('spawn')
    port = _free_port()
    case = dict(kind='fixture', name=name)
    procs = [ctx.Process(target=run_rank, args=(r, world, port, case, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    build, collate, samples, V = make_case(case)
    model = build().to(dev).eval()

    def single(part):
        inputs, labels = collate(None)(part)
        return model.target_rank(*[x.to(dev) for x in inputs], labels=labels.to(dev)).cpu()
    whole = single(samples)
    assert int(whole.min()) >= 0
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r))
        assert res['lo'] == (0 if r == 0 else res['lo']) and res['hi'] - res['lo'] == res['n_live'] < V
        # every rank feeds the same sessions (replicated evaluation loader): the full answer on every rank
        assert torch.equal(res['replicated'], whole), (r, res['replicated'].tolist(), whole.tolist())
        # every rank feeds its own slice (data-parallel evaluation): its own sessions' ranks
        mine, _ = rank_slice(samples, world, r, False)
        assert torch.equal(res['data_parallel'], single(mine)), (r, res['data_parallel'].tolist())
