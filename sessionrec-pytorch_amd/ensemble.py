"""Serve and evaluate an ENSEMBLE of models: the probability-averaged blend ("soft voting") p(v) = sum_m w_m p_m(v) of several
members - a cheap SRGNN beside a strong MSGIFSR, several seeds of one model - without one (B, V) matrix per member.

The served score of every model is already a mixture, logsumexp_c(cs[v] <sr_c[b], E_v> + off[c, b]) (serving.Query); the blend
is the same expression over the members' components side by side, each with its own table, width and column scale, and
log w_m added to the member's offsets.  ops.ens_select / ops.ens_ahead (csrc/ensemble.hip) run the catalogue pass over that.

Out of scope: row-sharded members (a member with `shard` is refused), renormalize (it would need a third multi-table kernel:
the values are renormalised over NOTHING - with exclude_seen or an item_bias they are log sum_m w_m p_m(v) (+ bias) as they
stand), truncation and sampling, the re-rankers (feed recommend()'s ordered pool to ops.cap_select / ops.calibrate /
ops.personal_merge yourself), log-linear (product-of-experts) blending, and more than 8 components in all.
"""
import contextlib
import math

import torch

from . import _lib, ops
from .serving import _Serving

MAX_COMPONENTS = _lib.ENS_CONST['SREC_ENS_MAXCOMP']


def _components_of(model):
    """how many soft-maxes the served score of a member mixes: an MSGIFSR order-k `fusion` member counts k, anything else 1"""
    order = int(getattr(model, 'order', 1))
    return order if getattr(model, 'fusion', False) and order > 1 else 1


class Ensemble:
    """Ensemble(models, weights=None): the blend sum_m w_m p_m of the members' next-item distributions.

    models: one or more models with the serving surface of serving.ServingMixin (SRGNN, NISER, LESSR, MSGIFSR), over the same
    catalogue and on one device; weights: one positive number per member, normalised to sum to one (None: uniform).
    ValueError if the members disagree on the number of items or sit on different devices, if a member is row-sharded
    (`shard is not None`: out of scope), or if the members' components sum to more than 8 (an MSGIFSR order-3 `fusion` member
    counts 3).

    Every method takes `inputs`: a sequence with ONE tuple of model inputs per member - the members collate differently - of
    the SAME sessions in the same order (the batch sizes are checked, the sessions cannot be).  A single tensor-like entry
    stands for a one-element tuple."""

    def __init__(self, models, weights=None):
        models = list(models)
        M = len(models)
        if M < 1:
            raise ValueError('Ensemble: no members')
        if weights is None:
            w = [1.0 / M] * M
        else:
            try:
                w = [float(x) for x in weights]
            except (TypeError, ValueError):
                raise ValueError('Ensemble: weights must be a sequence of numbers, one per member') from None
            if len(w) != M:
                raise ValueError('Ensemble: %d weights for %d members' % (len(w), M))
            for m, x in enumerate(w):
                if not (0.0 < x < float('inf')):
                    raise ValueError('Ensemble: weight %r of member %d; weights are positive and finite' % (x, m))
            total = math.fsum(w)
            w = [x / total for x in w]
        n0 = dev0 = None
        comps = 0
        for m, model in enumerate(models):
            if getattr(model, 'shard', None) is not None:
                raise ValueError('Ensemble: member %d is row-sharded; sharded members are out of scope' % m)
            n = int(model._num_items())
            if n0 is None:
                n0 = n
            if n != n0:
                raise ValueError('Ensemble: member %d has %d items, member 0 has %d' % (m, n, n0))
            dev = model._table().device if hasattr(model, '_table') else None
            if dev0 is None:
                dev0 = dev
            if dev != dev0:
                raise ValueError('Ensemble: member %d is on %s, member 0 on %s' % (m, dev, dev0))
            comps += _components_of(model)
        if comps > MAX_COMPONENTS:
            raise ValueError('Ensemble: the members mix %d soft-maxes in all; csrc/ensemble.hip takes at most %d '
                             '(an MSGIFSR order-k fusion member counts k)' % (comps, MAX_COMPONENTS))
        self.models, self.weights, self.num_items = models, w, n0

    def _inputs(self, who, inputs):
        inputs = list(inputs)
        if len(inputs) != len(self.models):
            raise ValueError('%s: inputs for %d members, the ensemble has %d (one tuple of model inputs per member)'
                             % (who, len(inputs), len(self.models)))
        return [tuple(x) if isinstance(x, (list, tuple)) else (x,) for x in inputs]

    def _serving(self):
        stack = contextlib.ExitStack()
        for m in self.models:
            stack.enter_context(_Serving(m))
        return stack

    def _operands(self, who, inputs, exclude_seen):
        """(comps, off_ex [C, B], off_in [C, B] or None, listed or None) of ops.ens_select / ens_ahead: every member's Query
        (its own _scoring_args) with log w_m on its offsets, the components side by side.  listed: the sessions' own items
        whenever a member lists them (MSGIFSR extra: they score through its repeat branch, off_in) or exclude_seen drops
        them; a member without off_in uses its off_ex for both.  Call inside _serving()."""
        comps, off_ex, off_in, listed, B = [], [], [], None, None
        any_in = False
        for m, (model, inp, w) in enumerate(zip(self.models, inputs, self.weights)):
            q = model._scoring_args(*inp, exclude_seen=exclude_seen)
            b = q.srs[0].shape[0]
            if B is None:
                B = b
            if b != B:
                raise ValueError('%s: member %d was given %d sessions, member 0 %d' % (who, m, b, B))
            table = model._table()
            comps += [(sr, table, q.cs) for sr in q.srs]
            C = len(q.srs)
            ex = (q.off_ex if q.off_ex is not None else q.srs[0].new_zeros(C, B)).reshape(C, B) + math.log(w)
            off_ex.append(ex)
            if q.off_in is not None and not exclude_seen:
                any_in = True
                off_in.append(q.off_in.reshape(C, B) + math.log(w))
            else:
                off_in.append(ex)
            if listed is None and q.listed is not None:
                listed = q.listed
        if exclude_seen and listed is None:
            listed = self.models[0]._session_items(inputs[0][0])
        off_ex = torch.cat(off_ex, 0).float().contiguous()
        off_in = torch.cat(off_in, 0).float().contiguous() if (any_in and not exclude_seen) else None
        if off_in is None and not exclude_seen:
            listed = None                       # nobody scores its listed items differently: no list at all
        return comps, off_ex, off_in, listed

    def recommend(self, inputs, k=20, exclude_seen=False, item_bias=None, item_group=None):
        """(log_probs fp32 [B,k] descending, item_ids int32 [B,k]): the k most probable next items under the blend, k <= 128.
        The values are log sum_m w_m p_m(v) (plus item_bias), p_m the distribution member m's forward() returns: log-
        probabilities of a proper distribution, renormalised over NOTHING (there is no renormalize keyword).  Ties towards
        the lower id; a session with fewer than k eligible items ends in (-inf, -1) slots.  exclude_seen, item_bias /
        item_group mean what they mean in model.recommend() (the bias is checked through the first member's _item_bias and
        added once, after the blend).  One fused pass over the members' tables (csrc/ensemble.hip; ops.ens_select).  Runs
        every member in eval mode under torch.no_grad()."""
        who = 'Ensemble.recommend'
        inputs = self._inputs(who, inputs)
        bias = self.models[0]._item_bias(who, item_bias, item_group)
        with self._serving():
            comps, off_ex, off_in, listed = self._operands(who, inputs, exclude_seen)
            return ops.ens_select(comps, k, off_ex, off_in, listed, bool(exclude_seen), **bias)

    def _score_items(self, inputs, items, exclude_seen, bias):
        """logsumexp_m(log w_m + member m's score_items) - every member adds the bias, which therefore comes out of the
        log-sum-exp once.  Call inside _serving()."""
        vals = [model._score_items(*inp, items=items, exclude_seen=exclude_seen, **bias) + math.log(w)
                for model, inp, w in zip(self.models, inputs, self.weights)]
        return vals[0] - math.log(self.weights[0]) if len(vals) == 1 else torch.logsumexp(torch.stack(vals, 0), dim=0)

    def score_items(self, inputs, items, exclude_seen=False, item_bias=None, item_group=None):
        """fp32 [B, M]: the blend's value at given items, logsumexp_m(log w_m + member.score_items(...)) - host arithmetic over
        the members' gather kernel (csrc/score_items.hip).  It is the number recommend() returns for the same item (to fp32
        round-off) and the `target` of served_rank().  items, exclude_seen, item_bias / item_group as model.score_items();
        -1 is padding and gives -inf."""
        who = 'Ensemble.score_items'
        inputs = self._inputs(who, inputs)
        bias = self.models[0]._item_bias(who, item_bias, item_group)
        items = torch.as_tensor(items)
        self.models[0]._check_ids(who, items)
        with self._serving():
            return self._score_items(inputs, items, exclude_seen, bias)

    def served_rank(self, inputs, labels, exclude_seen=False, item_bias=None, item_group=None):
        """int32 [B]: the rank of every session's label among what the ensemble SERVES, with the meanings of
        model.served_rank(): -1 no label (labels[b] < 0); -2 the label's blended value is -inf (the session's own item under
        exclude_seen, item_bias -inf); otherwise the number of eligible items ahead of it under recommend()'s order - when it
        is r < k <= 128 the label sits at position r of recommend(k=k, same keywords).  The label's value is score_items()';
        one fused counting pass over the members' tables (csrc/ensemble.hip; ops.ens_ahead).  No truncation keywords.
        train.metrics_from_served_ranks turns the ranks into HR / MRR / NDCG."""
        who = 'Ensemble.served_rank'
        inputs = self._inputs(who, inputs)
        bias = self.models[0]._item_bias(who, item_bias, item_group)
        lab = torch.as_tensor(labels).detach()
        if lab.is_floating_point() or lab.is_complex() or lab.dtype == torch.bool:
            raise ValueError('%s: labels must be an integer tensor (one item id per session), got %s' % (who, lab.dtype))
        lab = lab.reshape(-1).to(torch.int64)
        if lab.numel() > 0 and int(lab.max()) >= self.num_items:
            raise ValueError('%s: label %d; item ids are in [0, %d), or negative for a session without a label'
                             % (who, int(lab.max()), self.num_items))
        with self._serving():
            comps, off_ex, off_in, listed = self._operands(who, inputs, exclude_seen)
            dev = off_ex.device
            lab = lab.to(dev).clamp(min=-1)
            if lab.numel() != off_ex.shape[1]:
                raise ValueError('%s: %d labels for %d sessions' % (who, lab.numel(), off_ex.shape[1]))
            target = self._score_items(inputs, lab[:, None], exclude_seen, bias)[:, 0]
            ahead = ops.ens_ahead(comps, lab.to(torch.int32), target, off_ex, off_in, listed, bool(exclude_seen), **bias)
            out = torch.where(target > float('-inf'), ahead, torch.full_like(ahead, -2))
            return torch.where(lab < 0, torch.full_like(ahead, -1), out)

    @staticmethod
    def fit_weights(label_logp, iters=50):
        """float64 [M]: the mixture weights that maximise the mean ensemble log-likelihood mean_n log sum_m w_m exp(label_logp
        [n, m]) of held-out labels, by EM from uniform weights: r_nm ~ w_m exp(label_logp[n, m]) (normalised over m), w_m =
        mean_n r_nm, in float64.  label_logp [N, M]: member m's log-probability of example n's label - the members'
        score_items() at the labels.  Every iteration leaves the likelihood no lower.  An example no member gives any
        probability (a row of -inf) is left out.  Pure torch, no kernel."""
        lp = torch.as_tensor(label_logp).detach().to(torch.float64)
        if lp.dim() != 2 or lp.shape[1] < 1:
            raise ValueError('fit_weights: label_logp must be [N, M] (examples, members), got %s' % (tuple(lp.shape),))
        lp = lp[torch.isfinite(lp).any(1) & ~torch.isnan(lp).any(1)]
        M = lp.shape[1]
        w = torch.full((M,), 1.0 / M, dtype=torch.float64, device=lp.device)
        if lp.shape[0] == 0:
            return w
        for _ in range(int(iters)):
            r = torch.softmax(lp + torch.log(w)[None, :], dim=1)
            w = r.mean(0)
            w = w / w.sum()
        return w

    @staticmethod
    def mean_log_likelihood(label_logp, weights):
        """the objective of fit_weights: mean_n log sum_m w_m exp(label_logp[n, m]) in float64 (rows of -inf left out)"""
        lp = torch.as_tensor(label_logp).detach().to(torch.float64)
        lp = lp[torch.isfinite(lp).any(1)]
        w = torch.as_tensor(weights, dtype=torch.float64, device=lp.device)
        return float(torch.logsumexp(lp + torch.log(w)[None, :], dim=1).mean()) if lp.shape[0] else float('nan')
