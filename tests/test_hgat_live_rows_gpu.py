"""The MSHGNN layer's 'g16' forward projects only the rows some edge reads as its source (MSHGNN layer: who reads P).
Three pieces, each against something that does not share their code:
  * the live-source row lists (csrc/hgat.hip, srec_hg_live_rows) against the set of edge sources, numpy, on a hand-built batch;
  * srec_gemm16_nt_rows (csrc/gemm16.hip) against the unlisted launch on the same inputs: a listed row is byte-equal, every
    other row of C keeps its sentinel;
  * the layer and a captured training step with the switch ops.HG_LIVE_ROWS on against off: the projection rows the graph kernels
    read are byte-equal, so every output, gradient, loss and parameter is byte-equal."""
import ctypes

import numpy as np
import pytest
import torch

from util import load_golden, pkg, reseed

K, V = 3, 3429
# 8 sessions of 2 or 3 clicks: two of a single repeated item, four that end in a repeat (their last node has an out-edge: the
# conv1 'intra1' block is live in every row) and none with two trigram nodes (the 'intra3' relation has no edge)
HAND = [([5, 9, 9], 1), ([3, 4, 4], 2), ([7, 7, 7], 3), ([1, 2, 1], 4), ([6, 6], 5), ([10, 11, 11], 6), ([13, 14, 13], 7), ([8, 2, 8], 9)]


def hand_batch():
    c = pkg('collate')
    (mg,), _ = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=c.default_caps(12, 6))(HAND)
    return mg


def hand_plan(mg, d=64):
    torch.manual_seed(0)
    model = pkg().MSGIFSR(100, 'x', d, 1, dropout=0.0, order=K, extra=False, fusion=False)
    return model, model.layers[0].plan(mg, d, True)


def edge_sources(plan, mg):
    """per projection block: (live rows of its type, sorted rows that are the source of an edge of an instance reading the block
    as source, sorted rows that are not) - from the edge lists, not from the CSR the kernel walks"""
    out = []
    for b, (m, t) in enumerate(plan.blocks):
        n, src = mg.count('N%d' % (t + 1)), set()
        for (_, sb, _, gr) in plan.insts:
            if sb == b:
                E = int(gr[0].cpu().max())                      # in_ptr ends at the relation's edge count
                src |= set(gr[4].cpu()[:E].tolist())
        assert all(0 <= u < n for u in src)
        out.append((n, sorted(src), sorted(set(range(n)) - src)))
    return out


def test_hand_batch_is_not_vacuous():
    """what the list test relies on, checked on the expectation itself (no GPU): capacities above the live counts, a block with
    an empty list, one with every row listed, one strictly shorter, and chain ends (rows without an out-edge) that stay out"""
    mg = hand_batch()
    _, (plan, _) = hand_plan(mg)
    want = edge_sources(plan, mg)
    assert all(mg.meta['ncap'][t + 1] > n for (_, t), (n, _, _) in zip(plan.blocks, want))
    assert any(n > 0 and not src for n, src, _ in want)
    assert any(n > 0 and len(src) == n for n, src, _ in want)
    assert any(0 < len(src) < n for n, src, _ in want)
    # conv2 walks the reversed graph: a session's FIRST click has no out-edge there unless it is clicked again
    (m2, t2) = next((m, t) for (m, t) in plan.blocks if plan.mod_conv[m] == 1 and t == 0 and plan.modules[m][2] is not None)
    n, src, ends = want[plan.blocks.index((m2, t2))]
    # (sessions 0, 1 and 5 - their first nodes are rows 0, 2 and 8 of the order-1 type: 2 + 2 + 1 + 2 + 1 nodes before session 5)
    assert ends == [0, 2, 8] and not set(ends) & set(src)


@pytest.mark.gpu
def test_live_source_lists_equal_the_edge_sources(dev):
    ops, hg, L = pkg('ops'), pkg('hgat'), pkg('_lib')
    mg_cpu = hand_batch()
    model, _ = hand_plan(mg_cpu)
    mg = mg_cpu.to(dev)
    plan, params = model.to(dev).layers[0].plan(mg, 64, True)
    want = edge_sources(plan, mg_cpu)
    small, lay = plan.scratch(dev)
    small.view(torch.int32).fill_(-7)
    flat = [p.reshape(-1) if i % 4 else p for i, p in enumerate(params)]
    desc = plan.fill(ops.HgDesc(), small, lay, None, None, flat, None, None)
    lists, counts = plan.live_rows(small, lay)
    la = L.ptr_array(lists)
    L.lib.srec_hg_live_rows(ctypes.addressof(desc), ctypes.addressof(la), L.ptr(counts), L.stream())
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [len(src) for _, src, _ in want]
    for b, (n, src, _) in enumerate(want):
        got = lists[b].cpu().tolist()
        assert got[:len(src)] == src, (b, got[:n], src)
        assert all(v == -7 for v in got[len(src):]), (b, 'entries past the count are not written')


def _bf(dev, *s):
    return (torch.randn(*s, device=dev) * 0.5).bfloat16()


# (M capacity, N, K, list lengths): the small shapes take the 64 x 64 tiles, the two wide ones the 64 x 128 and 128 x 128 tiles of the
# benchmarked projections (tile-shape heuristics of srec_gemm16_nt); 127 / 128 / 129: a tile boundary of either tile height
NT_CASES = [(384, 512, 64, (0, 1, 127, 128, 129, 300)), (384, 512, 256, (0, 1, 127, 128, 129, 300)),
            (1536, 2048, 256, (1000,)), (3072, 2048, 256, (2000,))]


@pytest.mark.gpu
@pytest.mark.parametrize('M,N,Kd,lens', NT_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_gemm16_nt_with_a_row_list(dev, M, N, Kd, lens):
    ops = pkg('ops')
    torch.manual_seed(4)
    rng = np.random.default_rng(M + Kd)
    A, B = _bf(dev, M, Kd), _bf(dev, N, Kd)
    full = torch.full((M, N), 3.0, device=dev, dtype=torch.bfloat16)
    ops.gemm16('nt', [ops.GemmProb(M, N, Kd, [(A, B)], full, None)], Kd, Kd, N, c16=True, keep_dead=True)
    for n in lens:
        rows = np.sort(rng.choice(M, size=n, replace=False)).astype(np.int32)
        lst = torch.full((M,), M + 5, dtype=torch.int32)          # (entries past the count are never used: out of range on purpose)
        lst[:n] = torch.from_numpy(rows)
        lst, cnt = lst.to(dev), torch.tensor([n], device=dev, dtype=torch.int32)
        C = torch.full((M, N), 3.0, device=dev, dtype=torch.bfloat16)
        ops.gemm16('nt', [ops.GemmProb(M, N, Kd, [(A, B)], C, cnt, rows=lst)], Kd, Kd, N, c16=True, keep_dead=True)
        torch.cuda.synchronize()
        listed = torch.zeros(M, dtype=torch.bool, device=dev)
        listed[torch.from_numpy(rows).long().to(dev)] = True
        assert torch.equal(C[listed].view(torch.int16), full[listed].view(torch.int16)), (n, 'a listed row differs from the unlisted launch')
        assert bool((C[~listed] == 3.0).all()), (n, 'a row outside the list was written')


@pytest.mark.gpu
def test_gemm16_nt_listed_and_unlisted_problems_in_one_launch(dev):
    ops = pkg('ops')
    torch.manual_seed(5)
    M, N, Kd = 200, 256, 64
    A1, A2, B = _bf(dev, M, Kd), _bf(dev, M, Kd), _bf(dev, N, Kd)
    dyn = torch.tensor([150], device=dev, dtype=torch.int32)
    rows = torch.arange(0, 2 * 70, 2, dtype=torch.int32, device=dev)
    cnt = torch.tensor([70], device=dev, dtype=torch.int32)
    want = [torch.full((M, N), 3.0, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    ops.gemm16('nt', [ops.GemmProb(M, N, Kd, [(A1, B)], want[0], None), ops.GemmProb(M, N, Kd, [(A2, B)], want[1], dyn)],
               Kd, Kd, N, c16=True, keep_dead=True)
    got = [torch.full((M, N), 3.0, device=dev, dtype=torch.bfloat16) for _ in range(2)]
    ops.gemm16('nt', [ops.GemmProb(M, N, Kd, [(A1, B)], got[0], cnt, rows=rows), ops.GemmProb(M, N, Kd, [(A2, B)], got[1], dyn)],
               Kd, Kd, N, c16=True, keep_dead=True)
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0][0:140:2], want[0][0:140:2]) and bool((got[0][1:140:2] == 3.0).all()) and bool((got[0][140:] == 3.0).all())
    with pytest.raises(RuntimeError):                                # a list needs bf16 output that keeps dead rows
        ops.gemm16('nt', [ops.GemmProb(M, N, Kd, [(A1, B)], got[0], cnt, rows=rows)], Kd, Kd, N, c16=True, keep_dead=False)


def _layer_run(dev, layer, mg, x, g, drop, seed=21):
    """forward + backward of ops.hgat_layer -> dict of every result: out, arg, the projections, dx, every parameter gradient"""
    ops = pkg('ops')
    plan, params = layer.plan(mg, x.shape[1], False)
    ps = [p.detach().clone().requires_grad_() for p in params]
    xr = x.clone().requires_grad_()
    reseed(seed)
    out = ops.hgat_layer(xr, plan, ps, drop)
    saved = out.grad_fn.saved_tensors
    res = {'out': out.detach().clone(), 'arg': saved[2].clone()}
    res.update({'P%d' % m: saved[3 + m] for m in range(len(plan.modules))})
    gs = torch.autograd.grad(out, [xr] + ps, g)
    res['dx'] = gs[0]
    res.update({'g%d' % i: t for i, t in enumerate(gs[1:])})
    torch.cuda.synchronize()
    return plan, res


@pytest.mark.gpu
@pytest.mark.parametrize('batch', ['edge', 'synth16'])
@pytest.mark.parametrize('d', [64, 256])
@pytest.mark.parametrize('drop', [None, (0.1, 0.1)], ids=['nodrop', 'drop0.1'])
def test_layer_with_live_rows_equals_the_dense_projection(dev, batch, d, drop, monkeypatch):
    """switch on against off: out, arg, dx and every parameter gradient byte-equal (the weight gradient reads dP and x only); of the
    projections, the listed rows"""
    ops, c = pkg('ops'), pkg('collate')
    if batch == 'edge':
        samples = load_golden('msgifsr_K3_edge')[1]
    else:
        from dist_gpu_worker import synth_samples
        samples = synth_samples(16, V, 11)
    (mg,), _ = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=c.default_caps(len(samples), 20))(samples)
    mg = mg.to(dev)
    torch.manual_seed(d)
    layer = pkg().MSGIFSR(V, 'x', d, 1, dropout=0.0, order=K, extra=False, fusion=False).to(dev).layers[0]
    NT = sum(mg.meta['ncap'][k] for k in range(1, K + 1))
    x, g = torch.randn(NT, d, device=dev) * 0.5, torch.randn(NT, d, device=dev)
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    ops.weights_changed()
    runs, listed, gemm16 = {}, {False: 0, True: 0}, ops.gemm16

    def spy(kind, probs, *a, **kw):                  # how many problems of the call's launches carried a row list
        listed[sw] += sum(getattr(q, 'rows', None) is not None for q in probs)
        return gemm16(kind, probs, *a, **kw)
    monkeypatch.setattr(ops, 'gemm16', spy)
    for sw in (False, True):
        monkeypatch.setattr(ops, 'HG_LIVE_ROWS', sw)
        plan, runs[sw] = _layer_run(dev, layer, mg, x, g, drop)
    assert listed[False] == 0 and listed[True] == len(plan.blocks), listed
    for k in runs[False]:
        if not k.startswith('P'):
            assert torch.equal(runs[True][k], runs[False][k]), k
    # the listed rows of P (recomputed from the edge sources) are the dense ones; some live row is NOT listed
    skipped = 0
    for b, (n, src, ends) in enumerate(edge_sources(plan, mg)):
        m, t = plan.blocks[b]
        r0 = plan.types[t][0] - plan.modules[m][0]
        idx = torch.tensor(src, dtype=torch.long, device=dev) + r0
        assert torch.equal(runs[True]['P%d' % m][idx], runs[False]['P%d' % m][idx]), (b, 'listed projection rows')
        skipped += len(ends)
    assert skipped > 0


@pytest.mark.gpu
@pytest.mark.parametrize('pdrop', [0.0, 0.2], ids=['nodrop', 'drop0.2'])
def test_captured_step_with_live_rows_is_bit_identical(dev, pdrop, monkeypatch):
    """a captured bf16 training step, first step + three replays: losses and parameters bit-identical with the switch on and off;
    with dropout the lists ride in the dropout launch (no kernel node more), without it they are one launch per layer call"""
    from test_graph_gpu import _samples, _setup
    c, train, optim, G, ops = pkg('collate'), pkg('train'), pkg('optim'), pkg('graph'), pkg('ops')
    Vs = 400
    caps = c.default_caps(32, 12)
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    ops.weights_changed()
    runs = {}
    for sw in (False, True):
        monkeypatch.setattr(ops, 'HG_LIVE_ROWS', sw)
        rng = np.random.default_rng(9)
        model, mk = _setup('msgifsr', dev, Vs, d=128, dropout=pdrop)
        reseed(5)
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model)
        model.train()
        padded = [mk(caps)(_samples(rng, n, Vs)) for n in (32, 20, 32, 27)]
        x0, l0 = padded[0]
        step = G.GraphedTrainStep(model, opt, [x.to(dev) for x in x0], l0.to(dev))
        losses = [step([x.to(dev) for x in xs], lab.to(dev)).item() for xs, lab in padded]
        step.check()
        nodes = step.node_counts()
        runs[sw] = (losses, {k: p.detach().clone() for k, p in model.named_parameters()}, nodes['kernel'] if nodes else None)
    (l0_, p0, n0), (l1_, p1, n1) = runs[False], runs[True]
    assert l0_ == l1_, (l0_, l1_)
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    if n0 is not None:
        assert n1 == n0 + (0 if pdrop > 0 else 1), (n0, n1)
