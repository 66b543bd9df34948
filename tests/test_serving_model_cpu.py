"""The model-level serving entry points (serving.ServingMixin) end to end on the CPU: a table-only model whose session
vectors are its input, with a dist.VocabParallel of ONE rank attached (no process group) whose Local is the float64 stand-in
of every served route the CPU sharding tests already have.  What is under test is the mixin's dispatch - the query record,
_run's positional order, renormalisation through _replace, the shared tail of served_rank / rank_items - not a kernel.

Expected values: the fp32 matrix the same model's forward() returns, plus bias and masks, through the oracles of tests/ and
train.py's materialised routes.  Table and session vectors are multiples of 1/8: every logit is exact (a multiple of 1/64,
below 16), two items of a session score the same only where their logits are equal, and a per-session constant (the
soft-max normaliser, known to a few fp32 roundings) moves no order.  The finite bias values are 0, +-0.3 and +-0.6: two
biased scores are equal only where logit AND bias are (j * 0.3 is no multiple of 1/64: the nearest misses by 0.2 / 64 = 3e-3,
thousands of fp32 roundings), so adding the bias before or after the score is rounded to fp32 decides every order the same
way.  Ids, ranks and counts compare exactly, values to TOL_NORM (tests/test_serve_dist_cpu.py: fewer than ten fp32 roundings
of values below 16).

Two models: one soft-max (_ScoringMixin's own _scoring_args: off_ex = -lse, raw logits under renormalize), and a mixture of
C = 2 components with an off_in for the session's own items that overrides _scoring_args as MSGIFSR does."""
import pytest
import torch

import cutoff_oracle as co
import diversify_oracle as do
from item_bias_oracle import NINF, bias_rows
from items_oracle import items64, order64
from norm_oracle import norm64
from rank_oracle import scores64
from sample_oracle import key64
from select_oracle import drop_mask, select64
from test_diversify_cpu import _oracle_local
from test_rank_cpu import RankLocal
from test_rank_many_cpu import ManyLocal as AheadManyLocal
from test_select_many_dist_cpu import ManyLocal as SelectManyLocal
from test_serve_dist_cpu import TOL_NORM
from util import pkg

V, D, B, L, M, C, K = 150, 16, 8, 4, 6, 2, 5
T, SEED = 0.5, 9
BIAS_STEP = 0.3             # finite bias values: -2 .. 2 steps (see the module docstring)
KINDS = ('softmax', 'mixture')


class AllLocal(SelectManyLocal, AheadManyLocal, RankLocal, type(_oracle_local())):
    """every served route of dist.HipLocal from the float64 oracles: select / sample / score_items / norm / cutoff /
    select_many, ahead / ahead_many, rank, diversify"""


def _case():
    g = torch.Generator().manual_seed(41)
    eighth = lambda *shape: torch.randint(-8, 9, shape, generator=g).float() / 8      # exact products and sums
    table, srs = eighth(V, D), eighth(C, B, D)
    table[130], table[9] = table[7], table[8]            # exact ties: the lower id goes first
    off_ex = -eighth(C, B).abs()
    off_in = off_ex + 0.5
    listed = torch.stack([torch.randperm(V, generator=g)[:L] for _ in range(B)])
    listed[:, 3] = -1
    bias = torch.randint(-2, 3, (2, V), generator=g).float() * BIAS_STEP
    bias[0, ::5] = NINF
    bias[1] = NINF                                       # group 1 keeps four items: fewer than K
    bias[1, [3, 40, 77, 130]] = torch.tensor([1.0, -1.0, 2.0, 0.0]) * BIAS_STEP
    group = torch.zeros(B, dtype=torch.int64)
    group[6] = 1
    labels = torch.randint(0, V, (B,), generator=g)
    labels[0], labels[1], labels[2] = -1, listed[1, 0], 7                      # no label; a label its session lists; a tied item
    items = torch.stack([torch.randperm(V, generator=g)[:M] for _ in range(B)])
    items[:, 0] = labels.clamp(min=0)
    items[3, 2], items[4, 5] = -1, -1                    # empty slots
    items[5, 1] = listed[5, 1]
    keys = torch.arange(B) * 7 + 3
    return dict(table=table, srs=srs, off_ex=off_ex, off_in=off_in, listed=listed, bias=bias, group=group, labels=labels,
                items=items, keys=keys)


CASE = _case()


def _models(Query=None):
    """Query: the record _scoring_args returns (default: serving.Query)"""
    mixin, Query = pkg('srgnn')._ScoringMixin, Query or pkg('serving').Query
    listed = CASE['listed'].to(torch.int32)

    class TableOnly(mixin, torch.nn.Module):
        """one soft-max: the session vectors are the input [B, d]"""

        def __init__(self):
            super().__init__()
            self.embedding = torch.nn.Embedding(V, D)
            with torch.no_grad():
                self.embedding.weight.copy_(CASE['table'])

        def session_repr(self, sr, tgrad=None):
            return sr

        _session_items = staticmethod(lambda sr: listed)

        def forward(self, sr, exclude_seen=False):
            return self._log_probs(sr)

    class Mixture(TableOnly):
        """C = 2 components, the input is [C, B, d]; the session's own items score through off_in unless they are dropped"""

        def session_repr(self, srs, tgrad=None):
            return list(srs)

        def _scoring_args(self, *inputs, exclude_seen, raw=False):
            srs = self.session_repr(*inputs)
            cs, _ = self._col_scale(self._state(srs[0].shape[0]))
            return Query(srs, cs, CASE['off_ex'], None if exclude_seen else CASE['off_in'], listed, exclude_seen)

        def forward(self, srs, exclude_seen=False):
            """the score of the mixture, rounded once to fp32: what a materialising model would return"""
            E = self._table().detach()[:V]
            if exclude_seen:
                return scores64(srs, E, None, CASE['off_ex']).float()
            return scores64(srs, E, None, CASE['off_ex'], CASE['off_in'], listed).float()
    return TableOnly, Mixture


@pytest.fixture(scope='module', params=KINDS)
def served(request):
    """(model with the one-rank shard attached, its input, S: forward()'s matrix without / with exclude_seen)"""
    TableOnly, Mixture = _models()
    model = (TableOnly if request.param == 'softmax' else Mixture)().train()
    pkg('dist').VocabParallel(model, local=AllLocal(V))
    x = CASE['srs'][0] if request.param == 'softmax' else CASE['srs']
    with torch.no_grad():
        S = {drop: model(x, exclude_seen=drop).double() for drop in (False, True)}
    assert S[False].shape == (B, V) and model.training
    return model, x, S


def _biased(S, drop, biased):
    """(s float64 [B, V]: forward()'s matrix plus the bias, ineligible bool [B, V] or None, the bias keywords)"""
    s, dm, kw = S[drop], (drop_mask(CASE['listed'], V) if drop else None), {}
    if biased:
        rows = bias_rows(CASE['bias'], CASE['group'], B)
        s, dm = s + rows, (rows == NINF) if dm is None else dm | (rows == NINF)
        kw = dict(item_bias=CASE['bias'], item_group=CASE['group'])
    return s, dm, kw


def _close(got, want, what):
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    off = want == NINF
    assert torch.equal(got == NINF, off), (what, got, want)
    err = float((got - want)[~off].abs().max()) if not bool(off.all()) else 0.0
    print('%s: max abs err %.3e' % (what, err))
    assert err <= TOL_NORM, (what, err)


def _same(got, want, what):
    assert torch.equal(got.detach().long().cpu(), want.long().cpu()), (what, got, want)


def _lists(got, s, dm, k, what):
    """got = (values, ids) against select64 of the served matrix"""
    val, ids = select64(s, k, dm)
    assert got[1].dtype == torch.int32 and got[0].dtype == torch.float32
    _same(got[1], ids, what + ' ids')
    _close(got[0], val, what + ' values')


def test_recommend(served):
    model, x, S = served
    s, dm, _ = _biased(S, False, False)
    _lists(model.recommend(x, k=K), s, dm, K, 'recommend')
    s, dm, kw = _biased(S, True, True)
    got = model.recommend(x, k=K, exclude_seen=True, **kw)
    _lists(got, s, dm, K, 'recommend filtered')
    assert bool((got[1][6, 4:] == -1).all()) and bool((got[1][6, :3] >= 0).all())         # group 1: fewer than K items
    Z = norm64(S[True], CASE['bias'], CASE['group'], drop_mask(CASE['listed'], V))
    _lists(model.recommend(x, k=K, exclude_seen=True, renormalize=True, **kw), s - Z[:, None], dm, K, 'recommend renormalized')
    assert model.training                                                                  # (_Serving put the flag back)


def test_log_mass(served):
    model, x, S = served
    _close(model.log_mass(x), norm64(S[False]), 'log_mass')
    _close(model.log_mass(x, exclude_seen=True, item_bias=CASE['bias'], item_group=CASE['group']),
           norm64(S[True], CASE['bias'], CASE['group'], drop_mask(CASE['listed'], V)), 'log_mass filtered')


@pytest.mark.parametrize('crit', [dict(top_k=3), dict(top_p=0.6, temperature=T), dict(min_p=0.2), dict()], ids=str)
def test_cutoff(served, crit):
    model, x, S = served
    s, dm, kw = _biased(S, True, True)
    floor, count, kept = model.cutoff(x, exclude_seen=True, **crit, **kw)
    Tq = crit.get('temperature', 1.0)
    f = co.floor64(s, dm, Tq, **{k: v for k, v in crit.items() if k != 'temperature'})
    _close(floor, f, 'cutoff floor')
    _same(count, co.count64(s, dm, f), 'cutoff count')
    _close(kept, co.kept64(s, dm, Tq, f), 'cutoff log_kept')


def test_sample_with_top_p(served):
    model, x, S = served
    s, dm, kw = _biased(S, True, True)
    val, ids = model.sample(x, k=K, temperature=T, seed=SEED, session_keys=CASE['keys'], exclude_seen=True, top_p=0.6, **kw)
    out = dm | (s < co.floor64(s, dm, T, top_p=0.6)[:, None])
    _, want = select64(key64(s, T, SEED, CASE['keys']), K, out)
    _same(ids, want, 'sample ids')
    _close(val, items64(s, want, 0, dm), 'sample values')                                   # score_items of the draw
    assert bool((ids[6, 4:] == -1).all())
    # no truncation, renormalised: the values are those of score_items(renormalize=True)
    val, ids = model.sample(x, k=3, temperature=T, seed=SEED, exclude_seen=True, renormalize=True, **kw)
    _, want = select64(key64(s, T, SEED), 3, dm)
    Z = norm64(S[True], CASE['bias'], CASE['group'], drop_mask(CASE['listed'], V))
    _same(ids, want, 'sample renormalized ids')
    _close(val, items64(s - Z[:, None], want, 0, dm), 'sample renormalized values')


def _ranks(S, ids, drop, biased, **crit):
    train = pkg('train')
    return train.item_ranks_from_scores(S[drop].float(), ids, item_bias=CASE['bias'] if biased else None,
                                        item_group=CASE['group'] if biased else None, seen=CASE['listed'] if drop else None, **crit)


@pytest.mark.parametrize('crit', [dict(), dict(top_k=30)], ids=str)
def test_served_rank(served, crit):
    model, x, S = served
    lab = CASE['labels']
    _, _, kw = _biased(S, True, True)
    got = model.served_rank(x, labels=lab, exclude_seen=True, **crit, **kw)
    assert got.dtype == torch.int32 and got.shape == (B,)
    _same(got, _ranks(S, lab[:, None], True, True, **crit)[:, 0], 'served_rank')
    assert int(got[0]) == -1 and int(got[1]) == -2                         # no label; the label is the session's own item
    _same(model.served_rank(x, labels=lab), _ranks(S, lab[:, None], False, False)[:, 0], 'served_rank unfiltered')


@pytest.mark.parametrize('crit', [dict(), dict(top_k=30)], ids=str)
def test_rank_items(served, crit):
    model, x, S = served
    items = CASE['items']
    _, _, kw = _biased(S, True, True)
    got = model.rank_items(x, items=items, exclude_seen=True, **crit, **kw)
    assert got.dtype == torch.int32 and got.shape == (B, M)
    _same(got, _ranks(S, items, True, True, **crit), 'rank_items')
    assert int(got[3, 2]) == -1 and int(got[5, 1]) == -2                   # an empty slot; the session's own item
    _same(model.rank_items(x, items=items), _ranks(S, items, False, False), 'rank_items unfiltered')
    _same(model.rank_items(x, items=items[:, :1], exclude_seen=True, **crit, **kw), _ranks(S, items[:, :1], True, True, **crit),
          'rank_items M = 1')
    _same(model.rank_items(x, items=items[2]), _ranks(S, items[2], False, False), 'rank_items shared')


def test_score_items_and_rerank(served):
    model, x, S = served
    items = CASE['items']
    s, dm, _ = _biased(S, False, False)
    _close(model.score_items(x, items=items), items64(s, items, 0, dm), 'score_items')
    s, dm, kw = _biased(S, True, True)
    Z = norm64(S[True], CASE['bias'], CASE['group'], drop_mask(CASE['listed'], V))
    got = model.score_items(x, items=items, exclude_seen=True, renormalize=True, **kw)
    _close(got, items64(s - Z[:, None], items, 0, dm), 'score_items filtered')
    assert float(got[3, 2]) == NINF and float(got[5, 1]) == NINF
    val, ids = model.rerank(x, items=items, k=4, exclude_seen=True, **kw)
    wval, wids = order64(items64(s, items, 0, dm), items, 4)
    _same(ids, wids, 'rerank ids')
    _close(val, wval, 'rerank values')


def test_recommend_many(served):
    model, x, S = served
    s, dm, kw = _biased(S, True, True)
    got = model.recommend_many(x, k=200, exclude_seen=True, **kw)                           # more than the catalogue holds
    assert got[0].shape == (B, 200)
    _lists(got, s, dm, 200, 'recommend_many')
    s, dm, _ = _biased(S, False, False)
    _lists(model.recommend_many(x, k=K), s, dm, K, 'recommend_many k <= 128')


def test_recommend_diverse_and_list_diversity(served):
    model, x, S = served
    s, dm, kw = _biased(S, True, True)
    pool, theta = 12, 0.75
    pval, pids = select64(s, pool, dm)
    rows = CASE['table'][pids.clamp(min=0)]
    r = do.greedy64(rows, pval.float(), theta, K, pids >= 0)
    val, ids = model.recommend_diverse(x, k=K, diversity=theta, pool=pool, exclude_seen=True, **kw)
    want = torch.where(r['pick'] < 0, torch.full_like(r['pick'], -1), pids.gather(1, r['pick'].clamp(min=0)))
    _same(ids, want, 'recommend_diverse ids')
    _close(val, torch.where(r['pick'] < 0, torch.full_like(r['val'], NINF), r['val']), 'recommend_diverse values')
    got = model.list_diversity(pids[:, :K])
    _close(got, do.greedy64(rows[:, :K], torch.zeros(B, K), 0.0, K, pids[:, :K] >= 0)['ild'], 'list_diversity')


def test_target_rank_single_soft_max():
    TableOnly, _ = _models()
    model = TableOnly()
    pkg('dist').VocabParallel(model, local=AllLocal(V))
    x, lab = CASE['srs'][0], CASE['labels']
    with torch.no_grad():
        S = model(x)
    got = model.target_rank(x, labels=lab)
    _same(got, pkg('train').ranks_from_scores(S, lab), 'target_rank')
    assert int(got[0]) == -1
