"""The normalisations around MSGIFSR's MSHGNN layer ride in the layer's own launches (ops.NORM_FOLD, hgat.norm_fold_bits; DESIGN.md,
"who writes allf / g now").  Acceptance is byte-equality with the launches they replace:
  * layer level: ops.hgat_layer with an entry and an exit record under every mask against mask 0 (the launches of ops.normalize_stack
    and ops.norm_permute_pick) on the same inputs - every output, every saved buffer, every gradient, whole buffers;
  * kernel level: srec_hg_drop_prep_norm directly, and all four fused entry points through the layer call, against the pair of
    launches each replaces - every buffer of the call pre-filled with a sentinel and with guard elements behind it;
  * step level: loss, gradients and parameters of training steps, eager and captured, under every mask against mask 0; the captured
    graph loses one kernel node per fold."""
import ctypes

import numpy as np
import pytest
import torch

from util import pkg, reseed

V = 400
MASKS = [0, 1, 2, 4, 8, 15]
SENT = -7.25


def _clicks(rng, n, max_len=12):
    """n sessions; the first is a single click (no order-2 / order-3 node), the second ends in one item clicked after every other
    one of a long session (its node has more than 8 in-edges in the order-1 relation: the kernels' general path)"""
    out = [([5], 3), ([11, 7, 12, 7, 13, 7, 14, 7, 15, 7, 16, 7, 17, 7, 18, 7, 19, 7, 20, 7], 2)]
    while len(out) < n:
        L = int(rng.integers(1, max_len))
        seq = rng.integers(0, V, size=L).tolist()
        if L > 1 and rng.random() < 0.3:
            seq[1] = seq[0]
        out.append((seq, int(rng.integers(0, V))))
    return out[:n]


def _batch(dev, K, B, cap, seed=3):
    c = pkg('collate')
    samples = _clicks(np.random.default_rng(seed), B, 12)
    (mg,), _ = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=c.default_caps(cap, 24))(samples)
    return mg.to(dev)


def _records(ops, mg, K, raws, npick):
    ncap = mg.meta['ncap']
    dyns = tuple(mg.dynp('N%d' % k) for k in range(1, K + 1))
    types, r0 = [], 0
    for k in range(1, K + 1):
        types.append((r0, ncap[k], mg.dynp('N%d' % k)))
        r0 += ncap[k]
    entry = ops.NormEntry(list(raws), dyns, 0)
    exit_ = ops.NormExit(mg.cat_perm, mg.field('cat_inv'), mg.cat_seg, [mg.field('lastcat%d' % (i + 1)) for i in range(npick)],
                         types, mg.dynp('NT'), mg.dynp('B'), 0)
    return entry, exit_


def _layer_run(dev, ops, layer, mg, K, d, drop, npick, mask, monkeypatch):
    """forward + backward of the layer between its two normalisations -> every tensor anybody can see afterwards"""
    monkeypatch.setattr(ops, 'NORM_FOLD', mask)
    plan, params = layer.plan(mg, d, False)
    ps = [p.detach().clone().requires_grad_() for p in params]
    g0 = torch.Generator(device='cpu').manual_seed(17)
    ncap = mg.meta['ncap']
    raws = [(torch.randn(ncap[k], d, generator=g0) * 0.7).to(dev).requires_grad_() for k in range(1, K + 1)]
    entry, exit_ = _records(ops, mg, K, raws, npick)
    reseed(21)
    allf, picks = ops.hgat_layer(None, plan, ps, drop, entry, exit_)
    res = {'allf': allf.detach().clone()}
    for k, pk in enumerate(picks):
        assert getattr(pk, '_srec_cat_left', False) and pk.stride(0) == 2 * d, 'the pick buffers keep their left-half tag'
        res['pick%d' % k] = pk.detach().clone()
    g_allf = torch.randn(allf.shape, generator=g0).to(dev)
    g_picks = [torch.randn(pk.shape, generator=g0).to(dev) for pk in picks]
    gs = torch.autograd.grad([allf] + list(picks), raws + ps, [g_allf] + g_picks)
    res.update({'d%d' % i: t.detach().clone() for i, t in enumerate(gs)})
    torch.cuda.synchronize()
    return plan, res


@pytest.mark.gpu
@pytest.mark.parametrize('K,d,B,cap,npick', [(3, 256, 5, 8, 1), (2, 64, 37, 64, 2), (3, 64, 37, 64, 3), (2, 256, 5, 8, 1)],
                         ids=['K3-d256-B5', 'K2-d64-B37', 'K3-d64-B37-fusion', 'K2-d256-B5'])
def test_layer_under_every_mask_equals_the_separate_launches(dev, K, d, B, cap, npick, monkeypatch):
    ops, hg = pkg('ops'), pkg('hgat')
    mg = _batch(dev, K, B, cap)
    assert mg.count('B') < mg.B and all(mg.count('N%d' % k) < mg.meta['ncap'][k] for k in range(1, K + 1))     # capacity padding
    assert mg.count('N2') != mg.count('N1')
    deg = np.diff(mg.field('r_1_intra1_1_in_ptr').cpu().numpy()[:mg.count('N1') + 1])
    assert deg.max() > 8, 'some node takes the general path'
    torch.manual_seed(d + K)
    layer = pkg().MSGIFSR(V, 'x', d, 1, dropout=0.0, order=K, extra=False, fusion=False).to(dev).layers[0]
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    ops.weights_changed()
    taken = {}
    bits_fn = hg.norm_fold_bits
    monkeypatch.setattr(hg, 'norm_fold_bits', lambda *a: taken.setdefault('bits', bits_fn(*a)))
    ref = None
    for mask in MASKS:
        taken.clear()
        plan, res = _layer_run(dev, ops, layer, mg, K, d, (0.1, 0.1), npick, mask, monkeypatch)
        assert taken['bits'] == mask & hg.FOLDS_BUILT, (mask, taken)
        if ref is None:
            ref = res
            continue
        assert res.keys() == ref.keys()
        for k in ref:
            assert torch.equal(res[k].view(torch.int32), ref[k].view(torch.int32)), (mask, k)
    # without a dropout launch the entry folds decline (p = 0): the call falls back to the separate launches
    taken.clear()
    _, r0 = _layer_run(dev, ops, layer, mg, K, d, None, npick, 0, monkeypatch)
    taken.clear()
    _, r1 = _layer_run(dev, ops, layer, mg, K, d, None, npick, 15, monkeypatch)
    assert taken['bits'] & (hg.FOLD_A | hg.FOLD_D) == 0
    for k in r0:
        assert torch.equal(r1[k].view(torch.int32), r0[k].view(torch.int32)), ('p = 0', k)


def _guarded(dev, rows, cols, dtype=torch.float32, guard=2):
    """[rows + guard, cols] filled with a sentinel; the kernels see the first rows"""
    t = torch.full((rows + guard, cols), SENT if dtype != torch.uint8 else 201, device=dev, dtype=dtype)
    return t


def _same(a, b):
    a, b = a.contiguous(), b.contiguous()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize('K,d,B,cap', [(3, 256, 5, 8), (2, 64, 37, 64), (3, 64, 37, 64)], ids=['K3-d256-B5', 'K2-d64-B37', 'K3-d64-B37'])
def test_entry_forward_kernel_equals_normalize_then_drop_prep(dev, K, d, B, cap):
    """srec_hg_drop_prep_norm against srec_normalize_group_fwd + srec_hg_drop_prep16 on sentinel-filled buffers with guard rows:
    Y, inv, xc, xc16, xres and the attention multipliers byte-equal, guards untouched"""
    ops, hg, L = pkg('ops'), pkg('hgat'), pkg('_lib')
    mg = _batch(dev, K, B, cap)
    ncap = mg.meta['ncap']
    ns = [ncap[k] for k in range(1, K + 1)]
    NT = sum(ns)
    g0 = torch.Generator(device='cpu').manual_seed(5)
    raws = [(torch.randn(n, d + 4, generator=g0) * 0.7).to(dev)[:, :d] for n in ns]         # (row stride d + 4: ld is honoured)
    dyns = [mg.dynp('N%d' % k) for k in range(1, K + 1)]
    cnt = torch.randint(0, 4, (2, NT, 1), generator=g0).float().to(dev)
    seed, rc = ops.rng_args(dev)
    na = 1000
    out = {}
    for fused in (False, True):
        Y, inv = _guarded(dev, NT, d), _guarded(dev, NT, 1)
        xc, xres, mk = _guarded(dev, 2 * NT, d), _guarded(dev, NT, d), _guarded(dev, na, 1)
        x16 = torch.full((2 * NT + 2, d), 3.0, device=dev, dtype=torch.bfloat16)
        a_x, a_l, a_n, a_d = hg._group_arrays(raws, dyns)
        tail = (L.ptr(cnt), NT, d, 0.1, seed, rc, 103, None, L.ptr(xc), None, L.ptr(xres), 0.1, na, L.ptr(mk))
        if fused:
            L.lib.srec_hg_drop_prep_norm(K, ctypes.addressof(a_x), ctypes.addressof(a_l), ctypes.addressof(a_n), ctypes.addressof(a_d),
                                         L.ptr(Y), L.ptr(inv), 0, 1e-12, *tail, L.ptr(x16), None, None, None, L.stream())
        else:
            L.lib.srec_normalize_group_fwd(K, ctypes.addressof(a_x), ctypes.addressof(a_l), ctypes.addressof(a_n), ctypes.addressof(a_d),
                                           L.ptr(Y), d, L.ptr(inv), d, 0, 1e-12, L.stream())
            L.lib.srec_hg_drop_prep16(L.ptr(Y), *tail, L.ptr(x16), L.stream())
        torch.cuda.synchronize()
        out[fused] = dict(Y=Y, inv=inv, xc=xc, xres=xres, mk=mk, x16=x16)
    for k in out[False]:
        assert _same(out[True][k], out[False][k]), k
    assert bool((out[True]['Y'][NT:] == SENT).all()) and bool((out[True]['xres'][NT:] == SENT).all())
    assert float(out[True]['Y'][:NT].abs().max()) > 0 and not bool((out[True]['Y'][:NT] == SENT).any())


class _GuardedTorch:
    """stands in for the torch module inside hgat.py / ops.py: every torch.empty there becomes a sentinel-filled buffer with guard
    elements behind it, remembered under the name of the variable it is assigned to (`g` is `dx` inside ops.npp_backward)"""
    GUARD = 512

    def __init__(self):
        self.bufs = {}

    def __getattr__(self, name):
        return getattr(torch, name)

    ALIAS = {('npp_backward', 'dx'): 'g', ('forward', 'y'): 'x'}          # (ops.NormPermutePick / ops.NormalizeStack at mask 0)

    def _alloc(self, shape, dtype, device, depth):
        import linecache
        import re
        import sys
        n = int(np.prod(shape)) if len(shape) else 1
        big = torch.empty(n + self.GUARD, device=device, dtype=dtype)
        big.fill_(201 if dtype == torch.uint8 else SENT)
        fr = sys._getframe(depth)
        line = linecache.getline(fr.f_code.co_filename, fr.f_lineno)
        m = re.match(r'\s*([\w, ]+?)\s*=', line)
        var = m.group(1).replace(' ', '') if m else fr.f_code.co_name          # (`return torch.empty(...)`: the function's name)
        if re.search(r'\bfor\b.*\bin\b', line) and '[' in line:           # a list comprehension: one name for its elements
            var += '[]'
        self.bufs.setdefault(self.ALIAS.get((fr.f_code.co_name, var), var), []).append(big)
        return big[:n].view(shape)

    def empty(self, *shape, **kw):
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else tuple(shape)
        return self._alloc(shape, kw.get('dtype', torch.float32), kw.get('device'), 2)

    def empty_like(self, t, **kw):
        return self._alloc(tuple(t.shape), kw.get('dtype', t.dtype), kw.get('device', t.device), 2)


@pytest.mark.gpu
@pytest.mark.parametrize('K,d,B,cap,npick', [(3, 256, 5, 8, 1), (2, 64, 37, 64, 2), (3, 64, 37, 64, 3), (2, 256, 37, 64, 1)],
                         ids=['K3-d256-B5', 'K2-d64-B37', 'K3-d64-B37-fusion', 'K2-d256-B37'])
def test_every_buffer_of_the_layer_call_is_byte_equal_with_guards(dev, K, d, B, cap, npick, monkeypatch):
    """each fold against the pair of launches it replaces, on whole buffers: every buffer the layer call allocates (Y / x, inv, xc,
    xc16 / x16, xres, the attention masks, arg, allf, invr, the [v | read-out] pick buffers with their untouched right halves, g,
    the scratch with A / DP / der, the projection gradients, the per-order dX) starts from a sentinel with guard elements behind
    it; after forward + backward it is byte-equal to mask 0's, guards included.  Buffers only one side allocates (the
    un-normalised out, the stacked dx) are the ones the folds no longer write."""
    ops, hg = pkg('ops'), pkg('hgat')
    mg = _batch(dev, K, B, cap)
    torch.manual_seed(d + K)
    layer = pkg().MSGIFSR(V, 'x', d, 1, dropout=0.0, order=K, extra=False, fusion=False).to(dev).layers[0]
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    ops.weights_changed()
    runs = {}
    for mask in MASKS:
        proxy = _GuardedTorch()
        monkeypatch.setattr(hg, 'torch', proxy)
        monkeypatch.setattr(ops, 'torch', proxy)
        _, res = _layer_run(dev, ops, layer, mg, K, d, (0.1, 0.1), npick, mask, monkeypatch)
        monkeypatch.setattr(hg, 'torch', torch)
        monkeypatch.setattr(ops, 'torch', torch)
        runs[mask] = proxy.bufs
    ref = runs[0]
    must = {'x', 'inv', 'xcs,xres', 'x16', 'allm', 'scratch', 'P', 'arg', 'out', 'allf', 'invr', 'bufs[]', 'g', 'dP[]', 'dx', 'dxall'}
    assert must <= set(ref), sorted(ref)
    gone = {1: set(), 2: {'out'}, 4: set(), 8: {'dx'}, 15: {'out', 'dx'}}
    for mask in MASKS[1:]:
        got = runs[mask]
        assert must - set(got) == gone[mask], (mask, sorted(must - set(got)))
        for key in must - gone[mask]:
            assert len(got[key]) == len(ref[key]), (mask, key)
            for i, (a, b) in enumerate(zip(got[key], ref[key])):
                assert a.shape == b.shape and _same(a, b), (mask, key, i)
    for key, bufs in ref.items():                                        # nobody writes behind a buffer
        for b in bufs:
            tail = b[-_GuardedTorch.GUARD:]
            assert bool((tail == (201 if b.dtype == torch.uint8 else SENT)).all()), key


def _step_config(name):
    # (order, d, dropout, layers, extra, fusion)
    return {'K3-d256-drop': (3, 256, 0.1, 1, False, False), 'K2-d64-drop-fusion': (2, 64, 0.1, 1, False, True),
            'K3-d64-nodrop': (3, 64, 0.0, 1, False, False), 'K2-d256-drop-2layers': (2, 256, 0.1, 2, False, False),
            'K3-d64-drop-extra': (3, 64, 0.1, 1, True, True)}[name]


def _expected_folds(hg, mask, cfg):
    """how many launches the mask takes out of a step of the configuration"""
    K, d, p, layers, extra, fusion = cfg
    bits = hg.FOLD_B | hg.FOLD_C
    if p > 0 and not extra:
        bits |= hg.FOLD_A | hg.FOLD_D
    return bin(bits & mask & hg.FOLDS_BUILT).count('1')


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['eager', 'captured'])
@pytest.mark.parametrize('name', ['K3-d256-drop', 'K2-d64-drop-fusion', 'K3-d64-nodrop', 'K2-d256-drop-2layers', 'K3-d64-drop-extra'])
def test_training_steps_under_every_mask_are_bit_identical(dev, name, mode, monkeypatch):
    """bf16 training steps (eager: three; captured: first step + three replays): losses, gradients (eager) and parameters
    bit-identical to mask 0 under every mask; the captured graph has one kernel node fewer per fold the configuration takes"""
    c, train, optim, G, ops, hg = pkg('collate'), pkg('train'), pkg('optim'), pkg('graph'), pkg('ops'), pkg('hgat')
    cfg = _step_config(name)
    K, d, p, layers, extra, fusion = cfg
    caps = c.default_caps(32, 12)
    monkeypatch.setitem(ops.PRECISION, 'matmul', 'bf16')
    ops.weights_changed()
    mk = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=caps)
    runs = {}
    for mask in MASKS:
        monkeypatch.setattr(ops, 'NORM_FOLD', mask)
        rng = np.random.default_rng(9)
        torch.manual_seed(1)
        model = pkg().MSGIFSR(V, 'x', d, layers, dropout=p, order=K, extra=extra, fusion=fusion).to(dev)
        reseed(5)
        opt = optim.FusedAdam(train.fix_weight_decay(model), lr=1e-2, weight_decay=1e-4, model=model)
        model.train()
        padded = [mk(_clicks(rng, n, 12)) for n in (32, 20, 32, 27)]
        grads, nodes = None, None
        if mode == 'eager':
            losses = []
            for xs, lab in padded[:3]:
                opt.zero_grad()
                loss = model.fused_loss(*[x.to(dev) for x in xs], lab.to(dev))
                loss.backward()
                grads = {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}
                opt.step()
                losses.append(loss.item())
            del loss
        else:
            x0, l0 = padded[0]
            step = G.GraphedTrainStep(model, opt, [x.to(dev) for x in x0], l0.to(dev))
            losses = [step([x.to(dev) for x in xs], lab.to(dev)).item() for xs, lab in padded]
            step.check()
            nodes = step.node_counts()
            assert nodes, 'the captured graph\'s node counts are not available: the node assertion cannot be made'
            nodes = nodes['kernel']
        runs[mask] = (losses, {k: q.detach().clone() for k, q in model.named_parameters()}, grads, nodes)
    l0_, p0, g0_, n0 = runs[0]
    for mask in MASKS[1:]:
        l1_, p1, g1_, n1 = runs[mask]
        assert l1_ == l0_, (mask, l0_, l1_)
        for k in p0:
            assert torch.equal(p0[k].view(torch.int32), p1[k].view(torch.int32)), (mask, 'parameter', k)
        if g0_ is not None:
            assert g0_.keys() == g1_.keys()
            for k in g0_:
                assert torch.equal(g0_[k].view(torch.int32), g1_[k].view(torch.int32)), (mask, 'gradient', k)
        if n0 is not None:
            assert n0 - n1 == _expected_folds(hg, mask, cfg), (mask, n0, n1)
