"""Ensembles on the GPU: csrc/ensemble.hip through ops.ens_select / ops.ens_ahead, Ensemble and src/scripts/ensemble.py, against
materialised float64 scores (tests/ensemble_oracle.py; selection and ranks by select_oracle / rank_oracle).

One component must be the existing kernel, bit for bit.  Exact inputs (every product and sum representable, mixtures with one
live component per session) must give EQUAL lists and ranks on every path of the kernel: a width that is no multiple of 32,
mixed widths, tiles too large for LDS, eight components, lists scored and dropped, a grouped bias.  Genuine mixtures and the
models are checked by what every list / rank consistent with scores known to +-1e-4 (the fp32 bound of tests/test_select_gpu.py
at this scaling) must satisfy.

(The issue asks for K = 350 > V on the eight-component case; the selection keeps at most SREC_SELECT_MAXK = 128 items, which
the issue fixes too, so the tail slots are covered at K = 128 > V = 100 on the same component layout, and K = 350 must be
refused.)"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

from ensemble_oracle import exact_bias, exact_mixture, exact_tables, random_mixture, scores64_multi
from item_bias_oracle import bias_rows
from rank_oracle import assert_in_interval, ranks_exact
from select_oracle import assert_list_consistent, drop_mask, exact_case, scores64, select64, window_count
from util import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

TOL = 1e-4
NINF = float('-inf')


def _ops():
    return pkg('ops')


def _to(comps, dev):
    return [(sr.to(dev), E.to(dev), None if cs is None else cs.to(dev)) for sr, E, cs in comps]


def _t(x, dev):
    return None if x is None else x.to(dev)


def _equal(val, idx, ref, what):
    rv, ri = ref
    val, idx = val.cpu(), idx.cpu()
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == rv.shape == idx.shape, what
    bad = (idx.long() != ri).any(1) | (val.double() != rv).any(1)
    assert not bool(bad.any()), '%s: sessions %s differ, e.g. ids %s, expected %s' % (
        what, bad.nonzero().flatten().tolist()[:8], idx[bad][0].tolist()[:12], ri[bad][0].tolist()[:12])


# ------------------------------------------------------------------------------------------- 1) one component
@pytest.mark.parametrize('B,V,d,K', [(5, 300, 32, 32), (33, 5000, 96, 128)])
def test_one_component_is_the_existing_kernel(dev, B, V, d, K):
    """B = 33: a partial second session tile; V = 5000: several ranges, the pass-2 merge and a tail chunk of 8 rows"""
    ops = _ops()
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(B)
    off = -torch.randint(0, 9, (1, B), generator=g).float() / 8
    for scale in (cs, None):
        comps = _to([(sr, E, scale)], dev)
        val, idx = ops.ens_select(comps, K, off.to(dev))
        old = ops.score_select(sr.to(dev), E.to(dev), _t(scale, dev), K, off.to(dev))
        assert torch.equal(val, old[0]) and torch.equal(idx, old[1])
        _equal(val, idx, select64(scores64(sr, E, scale, off), K), 'C = 1 %s' % ((B, V, d, K),))
        # ... and the count is the existing count
        lab, tgt = idx[:, K // 2].contiguous(), val[:, K // 2].contiguous()
        ahead = ops.ens_ahead(comps, lab, tgt, off.to(dev))
        assert torch.equal(ahead, ops.score_ahead(sr.to(dev), E.to(dev), _t(scale, dev), lab, tgt, off.to(dev)))
        assert bool((ahead == K // 2).all())


# ------------------------------------------------------------------------------------------- 2) exact mixtures, every path
CASES = {'d32-100': ((32, 100), 37, 700),                       # a width that is no multiple of 32
         'mixed4': ((512, 256, 64, 32), 40, 600),               # four components of mixed widths
         'cache': ((1024, 1024), 33, 500),                      # tiles exceed 160 KB: read through the cache
         'eight': ((32,) * 8, 33, 300),                         # the maximum component count
         'eight-tail': ((32,) * 8, 33, 100)}                    # ... with K = 128 > V: tail slots

_EXACT = {}


def _exact(name):
    """(comps, off, off_in, listed, bias, group) and the oracle scores per list mode, computed once"""
    if name not in _EXACT:
        ds, B, V = CASES[name]
        comps, off, off_in, listed = exact_mixture(ds, B, V, seed=len(ds) * 1000 + V)
        s = {'plain': scores64_multi(comps, off), 'score': scores64_multi(comps, off, off_in, listed)}
        s['drop'] = s['plain']
        _EXACT[name] = (comps, off, off_in, listed, exact_bias(V, seed=V), torch.arange(B) % 2, s)
    return _EXACT[name]


def _modes(listed, off_in, V):
    return (('plain', None, None, False, None), ('score', listed, off_in, False, None),
            ('drop', listed, off_in, True, drop_mask(listed, V)))


@pytest.mark.parametrize('biased', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('name', list(CASES))
def test_exact_mixtures_on_every_kernel_path(dev, name, biased):
    ops = _ops()
    comps, off, off_in, listed, bias, group, s64 = _exact(name)
    B, V = off.shape[1], comps[0][1].shape[0]
    K = 128 if name == 'eight-tail' else 40
    dcomps = _to(comps, dev)
    for what, lst, oi, drop, dm in _modes(listed, off_in, V):
        s = s64[what]
        kw = {}
        if biased:
            rows = bias_rows(bias, group, B)
            s = s + rows
            dm = (rows == NINF) if dm is None else (dm | (rows == NINF))
            kw = dict(bias=bias.to(dev), group=group.to(dev))
        assert torch.equal(s.float().double()[s > NINF], s[s > NINF])            # the case is exact in fp32
        val, idx = ops.ens_select(dcomps, K, off.to(dev), _t(oi, dev), _t(lst, dev), drop_listed=drop, **kw)
        ref = select64(s, K, dm)
        print('exact', name, what, 'bias' if biased else '', idx[0].tolist()[:8], ref[1][0].tolist()[:8])
        _equal(val, idx, ref, 'exact %s %s' % (name, what))
        if name == 'eight-tail':
            assert bool((idx[:, V:] == -1).all()) and bool((val[:, V:] == NINF).all())
        if what == 'score' and not biased:      # the listed items' offsets matter: scored as "ex" the lists differ
            assert not torch.equal(select64(s64['plain'], K)[1], ref[1])


def test_k_beyond_the_selection_limit_is_refused(dev):
    comps, off = _exact('eight')[:2]
    with pytest.raises(ValueError, match='k = 350'):
        _ops().ens_select(_to(comps, dev), 350, off.to(dev))


# ------------------------------------------------------------------------------------------- 3) adversarial orders
@pytest.mark.parametrize('K', [1, 128])
@pytest.mark.parametrize('order', ['rising', 'falling', 'tied'])
def test_adversarial_score_orders(dev, order, K):
    """rising scores: every item of every chunk beats the running K-th best; all-tied: nothing after the first K items may
    enter.  Component 0 carries the live scores, component 1 is another table at offset -1e5"""
    ops = _ops()
    B, V, d = 33, 3000, 32
    sr = torch.zeros(B, d)
    sr[:, 0] = 1.0
    E = torch.zeros(V, d)
    v = torch.arange(V).float()
    E[:, 0] = {'rising': v / 8, 'falling': (V - 1 - v) / 8, 'tied': torch.full((V,), 0.5)}[order]
    E[:, 1] = 1.0
    (sr1, E1, cs1), = exact_tables((64,), B, V, seed=5)
    off = torch.zeros(2, B)
    off[1] = -1.0e5
    val, idx = ops.ens_select(_to([(sr, E, None), (sr1, E1, cs1)], dev), K, off.to(dev))
    j = torch.arange(K)
    ids = (V - 1 - j) if order == 'rising' else j
    vals = torch.full((K,), 0.5, dtype=torch.float64) if order == 'tied' else (V - 1 - j).double() / 8
    _equal(val, idx, (vals[None].expand(B, K), ids[None].expand(B, K)), '%s K=%d' % (order, K))


# ------------------------------------------------------------------------------------------- 4) genuine mixtures
_RANDOM = {}


def _random():
    if not _RANDOM:
        comps, off, off_in, listed = random_mixture((64, 128, 256), 70, 4000, seed=7)
        _RANDOM.update(comps=comps, off=off, off_in=off_in, listed=listed, plain=scores64_multi(comps, off),
                       score=scores64_multi(comps, off, off_in, listed))
    return _RANDOM


@pytest.mark.parametrize('mode', ['score', 'drop'])
def test_genuine_mixtures_give_consistent_lists(dev, mode):
    ops = _ops()
    r = _random()
    K, V = 50, 4000
    drop = mode == 'drop'
    s64 = r['plain'] if drop else r['score']
    dm = drop_mask(r['listed'], V) if drop else None
    dcomps, off, off_in, listed = _to(r['comps'], dev), r['off'].to(dev), r['off_in'].to(dev), r['listed'].to(dev)
    val, idx = ops.ens_select(dcomps, K, off, off_in, listed, drop_listed=drop)
    w = window_count(s64, K, TOL, dm)
    print('random C = 3', mode, 'window', w.tolist()[:12], 'max', int(w.max()))
    assert int(w.max()) < 8
    assert_list_consistent(val, idx, s64, TOL, dm, what='random C = 3 ' + mode)
    # the sentence of srec.h: with (labels, target) = (out_idx[:, j], out_val[:, j]) the count is j
    for j in range(K):
        ahead = ops.ens_ahead(dcomps, idx[:, j].contiguous(), val[:, j].contiguous(), off, off_in, listed, drop_listed=drop)
        assert bool((ahead == j).all()), (mode, j, ahead.tolist())


# ------------------------------------------------------------------------------------------- 5) rank
def _labels(B, V, seed):
    """labels spread over the item ranges, the second one missing"""
    g = torch.Generator().manual_seed(seed)
    lab = (torch.arange(B) * (V // B) + torch.randint(0, V // B, (B,), generator=g)).clamp(max=V - 1)
    lab[1] = -1
    return lab


@pytest.mark.parametrize('biased', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('name', ['d32-100', 'mixed4', 'cache', 'eight'])
def test_exact_ranks(dev, name, biased):
    ops = _ops()
    comps, off, off_in, listed, bias, group, s64 = _exact(name)
    B, V = off.shape[1], comps[0][1].shape[0]
    lab = _labels(B, V, seed=V)
    dcomps = _to(comps, dev)
    for what, lst, oi, drop, dm in _modes(listed, off_in, V):
        s = s64[what]
        kw = {}
        if biased:
            s = s + bias_rows(bias, group, B)
            kw = dict(bias=bias.to(dev), group=group.to(dev))
        if dm is not None:
            s = s.masked_fill(dm, NINF)                     # an ineligible row is ahead of nothing that can be a target here
        labs = lab.clone()
        dead = s.gather(1, labs.clamp(min=0)[:, None])[:, 0] == NINF          # move labels off ineligible rows
        labs[dead & (labs >= 0)] = s[dead & (labs >= 0)].argmax(1)
        target = s.gather(1, labs.clamp(min=0)[:, None])[:, 0]
        assert bool((target[labs >= 0] > NINF).all())
        got = ops.ens_ahead(dcomps, labs.to(dev), target.float().to(dev), off.to(dev), _t(oi, dev), _t(lst, dev), drop_listed=drop, **kw)
        want = ranks_exact(s, labs, target)
        print('rank', name, what, 'bias' if biased else '', got.tolist()[:8], want.tolist()[:8])
        assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want), (name, what)
        assert int(got[1]) == -1


def test_random_ranks_fall_in_the_oracle_interval(dev):
    ops = _ops()
    r = _random()
    B, V = 70, 4000
    lab = _labels(B, V, seed=3)
    s64 = r['score']
    target = s64.gather(1, lab.clamp(min=0)[:, None])[:, 0].float()
    got = ops.ens_ahead(_to(r['comps'], dev), lab.to(dev), target.to(dev), r['off'].to(dev), r['off_in'].to(dev), r['listed'].to(dev))
    lo, hi = assert_in_interval(got, s64, lab, tol=TOL, what='random C = 3', max_width=8)
    print('random ranks', got.tolist()[:8], 'width', (hi - lo).tolist()[:8])


# ------------------------------------------------------------------------------------------- 6) models
DATA = os.path.join(ROOT, 'datasets', 'sample')


def _sessions(n=40):
    out = []
    with open(os.path.join(GOLDEN, 'sample_test.txt')) as f:
        for line in f:
            if line.strip():
                out.append([int(x) for x in line.strip().split(',')])
    return out[:n]


_MODELS = {}


def _members(dev):
    """small seeded random-weight members over the sample catalogue and their inputs for the same 40 sessions"""
    if not _MODELS:
        sp, col = pkg(), pkg('collate')
        V = int(open(os.path.join(DATA, 'num_items.txt')).readline())
        torch.manual_seed(21)
        models = dict(srgnn=sp.SRGNN(V, 32, 1), niser=sp.NISER(V, 32, 1),
                      msgifsr=sp.MSGIFSR(V, 'synthetic', 32, 1, dropout=0.0, order=3, extra=False, fusion=True),
                      extra=sp.MSGIFSR(V, 'synthetic', 32, 1, dropout=0.0, order=2, extra=True, fusion=False))
        samples = [(s, 0) for s in _sessions()]
        flat = tuple(x.to(dev) for x in col.collate_fn_factory(col.seq_to_session_graph)(samples)[0])
        inputs = dict(srgnn=flat, niser=flat,
                      msgifsr=tuple(x.to(dev) for x in col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), 3)(samples)[0]),
                      extra=tuple(x.to(dev) for x in col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), 2)(samples)[0]))
        for m in models.values():
            m.to(dev).eval()
        pkg('ops').weights_changed()
        _MODELS.update(V=V, models=models, inputs=inputs, samples=samples)
    return _MODELS


def _blend64(models, inputs, weights):
    """log sum_m w_m p_m in float64 from the members' forward()"""
    with torch.no_grad():
        return torch.logsumexp(torch.stack([m(*i).double().cpu() + math.log(w) for m, i, w in zip(models, inputs, weights)], 0), 0)


def _seen(samples, V):
    m = torch.zeros(len(samples), V, dtype=torch.bool)
    for b, (seq, _) in enumerate(samples):
        m[b, torch.tensor(seq)] = True
    return m


def test_one_member_is_the_member(dev):
    M = _members(dev)
    Ensemble = pkg('ensemble').Ensemble
    for name in ('srgnn', 'msgifsr'):
        model, inp = M['models'][name], M['inputs'][name]
        for kw in ({}, dict(exclude_seen=True)):
            val, idx = Ensemble([model]).recommend([inp], k=20, **kw)
            old = model.recommend(*inp, k=20, **kw)
            if name == 'srgnn':
                assert torch.equal(val, old[0]) and torch.equal(idx, old[1]), kw
            else:       # (a mixture member folds its components in another order: the last bits may differ)
                assert_list_consistent(val, idx, _blend64([model], [inp], [1.0]), TOL, _seen(M['samples'], M['V']) if kw else None)


def test_three_members_against_the_materialised_blend(dev):
    M = _members(dev)
    ops, Ensemble = _ops(), pkg('ensemble').Ensemble
    names, weights = ('srgnn', 'niser', 'msgifsr'), (.2, .3, .5)
    models, inputs = [M['models'][n] for n in names], [M['inputs'][n] for n in names]
    ens = Ensemble(models, weights=weights)
    s64 = _blend64(models, inputs, weights)
    seen = _seen(M['samples'], M['V'])
    val, idx = ens.recommend(inputs, k=20)
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and val.shape == idx.shape == (len(M['samples']), 20)
    assert not any(m.training for m in models)
    print('blend window', window_count(s64, 20, TOL).tolist()[:8])
    assert_list_consistent(val, idx, s64, TOL, what='blend')
    err = float((val - ens.score_items(inputs, idx)).abs().max())
    print('max |recommend - score_items| %.2e' % err)
    assert err < TOL
    # exclude_seen, and an item_bias with a deny list
    v2, i2 = ens.recommend(inputs, k=20, exclude_seen=True)
    assert not bool(seen.gather(1, i2.cpu().long()).any())
    assert_list_consistent(v2, i2, s64, TOL, seen, what='blend exclude_seen')
    deny = idx[:, :3].flatten().unique()
    bias = ops.catalog_bias(M['V'], deny=deny, boost=(torch.arange(50, 60), torch.full((10,), 0.5)), device=dev)
    v3, i3 = ens.recommend(inputs, k=20, item_bias=bias)
    assert not bool(torch.isin(i3, deny).any())
    assert_list_consistent(v3, i3, s64 + bias.double().cpu()[None, :], TOL, (bias == NINF).cpu()[None, :].expand_as(s64), what='blend bias')
    assert float((v3 - ens.score_items(inputs, i3, item_bias=bias)).abs().max()) < TOL
    # the rank of the item at position 7 is 7 wherever round-off cannot move it
    lab = idx[:, 7]
    rank = ens.served_rank(inputs, lab).cpu().long()
    t = s64.gather(1, lab.cpu().long()[:, None])
    crowd = ((s64 - t).abs() <= 2 * TOL).sum(1) - 1                 # other items inside the window at position 7
    clear = crowd == 0
    share = float(clear.float().mean())
    print('served_rank: window at position 7 empty for %.0f %% of the sessions' % (100 * share), rank.tolist()[:8])
    assert share >= 0.9
    assert bool((rank[clear] == 7).all()) and bool(((rank - 7).abs() <= 1).all())
    lab2 = lab.clone()
    lab2[0] = -1
    r2 = ens.served_rank(inputs, lab2, exclude_seen=True)
    own = seen.gather(1, lab.cpu().long()[:, None])[:, 0]
    assert int(r2[0]) == -1 and bool((r2.cpu()[1:][own[1:]] == -2).all()) and bool((r2.cpu()[1:][~own[1:]] >= 0).all())
    # log-probabilities of a proper distribution
    v128, _ = ens.recommend(inputs, k=128)
    mass = v128.double().exp().sum(1)
    print('mass of the 128 best', mass.tolist()[:4])
    assert float(mass.max()) <= 1 + 1e-4


def test_extra_member_lists_travel(dev):
    """MSGIFSR `extra` scores a session's own items through its repeat branch (off_in): beside an SRGNN, which has none, the
    blend must still be the materialised one"""
    M = _members(dev)
    Ensemble = pkg('ensemble').Ensemble
    names, weights = ('extra', 'srgnn'), (.6, .4)
    models, inputs = [M['models'][n] for n in names], [M['inputs'][n] for n in names]
    ens = Ensemble(models, weights)
    with ens._serving():
        comps, off_ex, off_in, listed = ens._operands('test', inputs, False)
    assert len(comps) == 2 and off_in is not None and listed is not None and listed.shape[0] == len(M['samples'])
    assert torch.equal(off_in[1], off_ex[1]) and not torch.equal(off_in[0], off_ex[0])
    s64 = _blend64(models, inputs, weights)
    val, idx = ens.recommend(inputs, k=20)
    assert_list_consistent(val, idx, s64, TOL, what='extra + srgnn')
    assert float((val - ens.score_items(inputs, idx)).abs().max()) < TOL
    seen = _seen(M['samples'], M['V'])
    v2, i2 = ens.recommend(inputs, k=20, exclude_seen=True)
    assert_list_consistent(v2, i2, s64, TOL, seen, what='extra + srgnn exclude_seen')


# ------------------------------------------------------------------------------------------- 7) the launcher
def test_launcher_with_one_member_is_recommend_py_and_evaluates(dev, tmp_path):
    sp, col, train, ds = pkg(), pkg('collate'), pkg('train'), pkg('dataset')
    scripts = os.path.join(ROOT, 'src', 'scripts')
    V = int(open(os.path.join(DATA, 'num_items.txt')).readline())
    torch.manual_seed(12)
    model = sp.SRGNN(V, 32, 1)
    ckpt = tmp_path / 'run.pt'
    torch.save(dict(model=model.state_dict(), optimizer={}, scheduler={}, epoch=1, batch=0, best=[0.0, 0.0]), str(ckpt))
    (tmp_path / 'sessions.txt').write_text(''.join(','.join(str(i) for i in s) + '\n' for s in _sessions()))
    flags = ['--embedding-dim', '32', '--num-layers', '1', '--checkpoint', str(ckpt)]
    (tmp_path / 'members.txt').write_text('--model SRGNN %s --weight 2\n' % ' '.join(flags))
    serve = ['--dataset-dir', DATA, '--sessions', str(tmp_path / 'sessions.txt'), '--top', '30', '--exclude-seen']

    def run(script, *args):
        r = subprocess.run([sys.executable, os.path.join(scripts, script)] + list(args), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    one = run('recommend.py', '--model', 'SRGNN', *flags, *serve)
    ens = run('ensemble.py', '--members', str(tmp_path / 'members.txt'), *serve)
    assert len(one.splitlines()) == 40 and ens == one
    line = run('ensemble.py', '--members', str(tmp_path / 'members.txt'), '--evaluate', '--dataset-dir', DATA, '--cutoffs', '5,20',
               '--batch-size', '512').splitlines()
    assert len(line) == 1
    rep = json.loads(line[0])
    assert rep['weights'] == [1.0] and set(rep['metrics']) == {'hit@5', 'mrr@5', 'ndcg@5', 'hit@20', 'mrr@20', 'ndcg@20', 'shown'}
    # the same number in process
    model = model.to(dev).eval()
    pkg('ops').weights_changed()
    e = pkg('ensemble').Ensemble([model])
    test_set = ds.AugmentedDataset(ds.read_sessions(os.path.join(DATA, 'test.txt')))
    samples = [test_set[i] for i in range(len(test_set))]
    ranks = []
    for b in range(0, len(samples), 512):
        inputs, labels = col.collate_fn_factory(col.seq_to_session_graph)(samples[b:b + 512])
        ranks.append(e.served_rank([tuple(x.to(dev) for x in inputs)], labels.to(dev)).cpu())
    want = train.metrics_from_served_ranks(torch.cat(ranks), [5, 20])
    assert rep['sessions'] == len(samples) and rep['metrics']['hit@20'] == want['hit@20'] and rep['metrics'] == want
