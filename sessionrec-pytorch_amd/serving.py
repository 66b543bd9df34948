"""The serving surface every model shares: recommend / recommend_many / recommend_diverse / recommend_capped /
recommend_calibrated / recommend_personal, sample, cutoff, log_mass, score_items / rerank, served_rank / rank_items, the list measures
list_diversity / list_calibration, and the evaluation calls topk / target_rank.

ServingMixin is the base of srgnn._ScoringMixin, which supplies what it needs of a model: _table, _state, _col_scale, _lse,
session_repr, shard.  Every served call scores with one Query - the operands of the score, the exclude_seen flag and the
bias keywords - and reaches its kernel through one method, _run: the launcher of ops on one device, the route of
dist.VocabParallel over a row-sharded table.
"""
from collections import namedtuple

import torch

from . import ops

# what a served call scores with: logsumexp_c(cs[v] <srs[c][b], E_v> + off[c, b]) (off_in for the items of listed[b, :] unless
# `drop` - exclude_seen - drops them, off_ex elsewhere) plus the keywords of _item_bias, {} or dict(bias=, group=).  The
# model-side record: score.ServedArgs is the normalised one a launcher builds from these.
Query = namedtuple('Query', 'srs cs off_ex off_in listed drop bias', defaults=(False, {}))


class _Serving:
    """`with _Serving(model):` around a serving entry point: eval mode and torch.no_grad(), the training flag put back"""

    def __init__(self, model):
        self.model, self.no_grad = model, torch.no_grad()

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        self.no_grad.__enter__()

    def __exit__(self, *exc):
        self.no_grad.__exit__(*exc)
        self.model.train(self.was_training)


class ServingMixin:
    """Everything that serves, for a model with the scoring head of srgnn._ScoringMixin (its subclass)."""

    def topk(self, *inputs, k=20):
        """(scores [B,k], item ids [B,k]) of the k best items per session WITHOUT the (B, V) score matrix
        (train.evaluate: train.py:36-55).  Models whose score mixes several soft-maxes (MSGIFSR fusion / extra)
        rank through forward()."""
        with torch.no_grad():
            sr = self.session_repr(*inputs)
            mixed = isinstance(sr, (list, tuple)) or getattr(self, 'extra', False)
            if mixed:
                v, i = self(*inputs).topk(k)          # sharded table: forward() assembles (B, V) from the column blocks
                return v, i.to(torch.int32)
            st = self._state(sr.shape[0])
            cs, _ = self._col_scale(st)
            if self.shard is not None:       # local top-k per shard -> all-gather -> merge
                return self.shard.topk(sr, self._table(), cs, k, data_parallel=self.shard.eval_data_parallel)
            return ops.score_topk(sr, self._table(), cs, k)

    def target_rank(self, *inputs, labels):
        """int32 [B]: how many catalog items score ahead of each session's label (0 = the label is the top item; ties count
        towards the lower item id, as topk does; a label < 0 gives -1) - one fused pass over the table, no (B, V) score
        matrix and no cutoff: every HR / MRR / NDCG @k of train.evaluate(method='rank') follows from it (train.py:36-55)."""
        with torch.no_grad():
            sr = self.session_repr(*inputs)
            cs, _ = self._col_scale(self._state(sr.shape[0]))
            return self._label_rank(Query([sr], cs, None, None, None), labels)

    # served call of dist.VocabParallel over a row-sharded table <-> (launcher of ops on one device, its own keywords)
    _ROUTES = {'target_rank': ('score_rank', {}), 'select': ('score_select', {}), 'sample': ('score_sample', {}),
               'select_many': ('score_select_many', {}),
               'norm': ('score_norm', {}), 'cutoff': ('score_cutoff', {}), 'diversify': ('diversify', {'checked': True}),      # (the pool's ids are the select kernel's)
               'cap': ('cap_select', {'checked': True}),            # (the pool's ids are the select kernels')
               'calibrate': ('calibrate', {'checked': True}),       # (... and the target is _calibration_target's)
               'personal': ('personal_merge', {'checked': True}),   # (... and the lists are ops.personal_lists')
               'score_items': ('score_items', {'checked': True}),   # (model.score_items looked; sample() passes the kernel's ids)
               'ahead': ('score_ahead', {}), 'ahead_many': ('score_ahead_many', {})}

    def _route(self, name):
        """(callable, its route keywords) of served call `name`: shard.<name> fed as evaluate() feeds the shard
        (eval_data_parallel) - every shard works on its own rows and ONE small collective combines them (dist.py) - or the
        launcher of ops on one device.  Both take (srs, table, cs, ...) in the same positional order."""
        if self.shard is not None:
            return getattr(self.shard, name), {'data_parallel': self.shard.eval_data_parallel}
        fn, kw = self._ROUTES[name]
        return getattr(ops, fn), kw

    def _run(self, q, name, *lead, **kw):
        """served call `name` (a key of _ROUTES but 'diversify', 'cap', 'calibrate' and 'personal', which score nothing) over the Query q.  The one place that
        knows the routes' positional order: (srs, table, cs, *lead, off_ex, off_in, listed, drop_listed - not for
        'target_rank', which drops nothing - then keywords only).  lead: k | items | (labels, target) | (items, target), as
        the route takes them; kw: keywords of the call beyond the route's own and the bias (the criteria of cutoff, floor=,
        temperature= / seed= / session_keys=)."""
        fn, route_kw = self._route(name)
        drop = () if name == 'target_rank' else (q.drop,)
        return fn(q.srs, self._table(), q.cs, *lead, q.off_ex, q.off_in, q.listed, *drop, **route_kw, **q.bias, **kw)

    def _num_items(self):
        return self.shard.V if self.shard is not None else self._table().shape[0]

    def _check_id_range(self, who, lo, hi):
        """lo / hi: the smallest and largest of the item ids a caller gave (host integers)"""
        n = self._num_items()
        if lo < -1 or hi >= n:
            raise ValueError('%s: item id %d; ids are in [0, %d), or -1 for a padding slot' % (who, lo if lo < -1 else hi, n))

    def _check_ids(self, who, ids):
        """_check_id_range of an integer tensor of item ids, at the price of one device-to-host read"""
        if ids.numel() > 0:
            self._check_id_range(who, *(int(x) for x in torch.aminmax(ids.detach())))

    def _label_rank(self, q, labels):
        """target_rank under the Query q (no drop flag, no bias)"""
        rank = self._run(q, 'target_rank', labels)
        if self.shard is not None:       # (ranks of disjoint row shards add up: the shard's answer is final)
            return rank
        rank = rank[0]                   # (one device: (rank, target))
        if q.listed is not None:
            # the fix-up pass re-scores a listed item in another summation order than the count pass: where its "ex" score is
            # within round-off of the target the two comparisons can disagree and the correction overshoots by one
            rank = torch.where(labels >= 0, rank.clamp(min=0), rank)
        return rank

    def _item_bias(self, who, item_bias, item_group):
        """the keywords ops.score_select / ops.score_items (and the sharded routes) take for item_bias / item_group - none at
        all without a bias, so the call is then what it was.  Checked here, before anything of the model runs: the shape
        ([num_items] or [G, num_items], floating; item_group integer, only with a 2-D bias and needed for G > 1), and the
        VALUES the kernels assume - no NaN, no +inf (the all-reduce of the sharded score_items relies on "no slot is ever
        +inf"), every group id in [0, G) - at the price of ONE device-to-host read of two flags behind a pass over the bias:
        measured at V 37 484, 74 us per call for [V] and 88 us for [4, V] with 512 group ids, beside 0.46-1.7 ms for the
        selection itself (profiles/item_bias_timing.md)."""
        if item_bias is None:
            if item_group is not None:
                raise ValueError('%s: item_group is given without an item_bias' % who)
            return {}
        n = self._num_items()
        dev = self._table().device
        b = item_bias.detach()
        if not b.is_floating_point() or b.dim() not in (1, 2) or b.shape[-1] != n:
            raise ValueError('%s: item_bias must be a floating tensor [%d] or [G, %d] (one entry per catalogue item), got %s %s'
                             % (who, n, n, b.dtype, tuple(b.shape)))
        G = b.shape[0] if b.dim() == 2 else 1
        if G < 1 or (item_group is None and G > 1) or (item_group is not None and b.dim() != 2):
            raise ValueError('%s: item_group (one row id per session) goes with an item_bias [G, %d], and G > 1 needs it; got '
                             'item_bias %s, item_group %s' % (who, n, tuple(b.shape), 'None' if item_group is None else 'given'))
        b = b.to(dev)
        flags = [(torch.isnan(b) | (b == float('inf'))).any()]
        g = None
        if item_group is not None:
            g = item_group.detach()
            if g.is_floating_point() or g.is_complex() or g.dtype == torch.bool:
                raise ValueError('%s: item_group must be an integer tensor, got %s' % (who, g.dtype))
            g = g.to(dev).reshape(-1)
            flags.append(((g < 0) | (g >= G)).any())
        bad = torch.stack(flags).tolist()                   # the one device-to-host read
        if bad[0]:
            raise ValueError('%s: item_bias holds NaN or +inf; values are finite, or -inf for an item outside the catalogue' % who)
        if len(bad) > 1 and bad[1]:
            raise ValueError('%s: item_group holds a row id outside [0, %d)' % (who, G))
        return dict(bias=b, group=g)

    def recommend(self, *inputs, k=20, exclude_seen=False, item_bias=None, item_group=None, renormalize=False):
        """(log_probs fp32 [B,k] descending, item_ids int32 [B,k]): the k most probable next items of every session, k <= 128.
        The values are the numbers forward() returns at those items (log-probabilities); ties go towards the lower item
        id.  One fused selection pass over the table (csrc/recommend.hip): no (B, V) score matrix, sharded table included.
        exclude_seen=True never returns an item of the session itself (at most 64 distinct items per session); the remaining
        items keep forward()'s log-probabilities (renormalize=True: see below).  A session with fewer than k eligible items
        ends in (-inf, -1) slots.  Runs in eval mode under torch.no_grad().
        item_bias: fp32 [num_items], or [G, num_items] with item_group [B] row ids in [0, G) (sessions of several markets in
        one batch), over GLOBAL item ids (ops.catalog_bias builds one from allow / deny / boost lists).  The values are then
        forward()'s log-probabilities PLUS the bias, ordered by that sum; an item whose bias is -inf is never returned.  A
        wrong length, NaN or +inf in the bias and a group id outside [0, G) raise ValueError before anything is launched
        (_item_bias: one device-to-host read).
        renormalize=False: the values are not renormalised over the items that remain.  renormalize=True: they are the
        log-probabilities of the model's distribution RESTRICTED to the eligible items (not the session's own under
        exclude_seen, bias > -inf) and tilted by the finite bias, p(v) ~ p_model(v) exp(bias_v): per session exp(value) sums to
        one over the eligible catalogue.  Order and ids are those of renormalize=False, -inf slots stay -inf.  One more fused
        pass over the table (csrc/score_norm.hip, no (B, V) matrix) - and for a single soft-max the full-catalogue statistics
        pass is skipped instead, the normaliser being taken over the raw logits.  With nothing to renormalise (no item_bias,
        no exclude_seen) the call is the one of renormalize=False, bit for bit."""
        bias = self._item_bias('recommend', item_bias, item_group)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            return self._run(q, 'select', k)

    def recommend_many(self, *inputs, k, exclude_seen=False, item_bias=None, item_group=None, renormalize=False):
        """(log_probs fp32 [B,k] descending, item_ids int32 [B,k]): recommend() beyond 128 items, 1 <= k <= 4096 - the candidate
        stage of a two-stage set-up (rerank() / score_items() of a second model take lists of any length) and the export of
        long lists.  Values, order, ties, (-inf, -1) slots and every keyword (exclude_seen, item_bias / item_group,
        renormalize, mixtures, row-sharded tables) mean what they mean in recommend(); k and item_bias / item_group are
        checked before anything of the model runs.  No (B, V) score matrix: the k-th best score of every session is found
        by the radix search of cutoff(top_k=k), one more pass collects the items at or above it and one workgroup per
        session orders them (csrc/select_many.hip; ops.score_select_many) - about seven passes over the table and ONE
        device-to-host read (the largest count sizes the buffer).  For k <= 128 the call IS recommend(): the selection
        kernel takes one pass over the table instead of seven (ops.score_select_many itself always takes the long route).
        Runs in eval mode under torch.no_grad()."""
        k = ops.select_many_k('recommend_many', k)
        bias = self._item_bias('recommend_many', item_bias, item_group)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            return self._run(q, 'select' if k <= 128 else 'select_many', k)

    def recommend_diverse(self, *inputs, k=20, diversity=0.5, pool=None, exclude_seen=False, item_bias=None, item_group=None,
                          renormalize=False):
        """(log_probs fp32 [B,k], item_ids int32 [B,k]) in PICK order: a slate of k items that trades a little probability for
        coverage - the greedy MMR re-rank (csrc/diversify.hip, ops.diversify) of the `pool` most probable items.  The pool is
        exactly what recommend(k=pool, same keywords) returns (pool: default min(128, max(4 k, k)); k <= pool <= 128), so
        exclude_seen, item_bias / item_group, renormalize and mixtures mean what they mean there.  With slot i of the pool
        holding item v_i and value s_i (its log-probability, plus bias), and sim the cosine of two rows of the item table
        (sim(i, j) = <E_i, E_j> / (max(|E_i|, 1e-12) max(|E_j|, 1e-12)), a zero row: 0), step t picks the slot with the
        largest  s_i - diversity * max_{j picked} sim(i, j)  (no penalty at t = 0; the raw maximum, not clamped at 0; ties
        to the better-ranked slot).  The values are the pool's own numbers at the picks, bit for bit; unfilled slots (the
        pool had fewer than k eligible items) are (-inf, -1).  diversity: finite, >= 0; 0 returns the first k columns of
        recommend(k=pool).  One more launch, one workgroup per session: no [B, pool, d] gather and no [B, pool, pool] Gram
        matrix on one device; a row-sharded table exchanges B * pool * d * 4 bytes (dist.VocabParallel.diversify).  Runs in
        eval mode under torch.no_grad(); k, diversity, pool and item_bias / item_group are checked before anything of the
        model runs."""
        k, diversity, pool = self._diverse_args('recommend_diverse', k, diversity, pool)
        bias = self._item_bias('recommend_diverse', item_bias, item_group)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            val, ids = self._run(q, 'select', pool)
            pval, pick, _, _ = self._diversify(ids, val, k, diversity)
            picked = ids.gather(1, pick.clamp(min=0).long())
            return pval, torch.where(pick < 0, torch.full_like(picked, -1), picked)

    @staticmethod
    def _diverse_args(who, k, diversity, pool):
        """(k, diversity, pool) checked: pool defaults to min(128, max(4 k, k)), k <= pool <= 128 (ValueError otherwise)"""
        k, diversity = ops.diversify_scalars(who, k, diversity)
        pool = min(128, max(4 * k, k)) if pool is None else int(pool)
        if not k <= pool <= 128:
            raise ValueError('%s: pool = %d; it holds at least the k = %d items asked for and at most 128 (recommend()\'s limit)'
                             % (who, pool, k))
        return k, diversity, pool

    def _diversify(self, ids, val, k, diversity):
        """(val, pick, mmr, ild) of ops.diversify over the rows of the item table at the global ids [B, M] (-1: unfilled)"""
        fn, kw = self._route('diversify')
        return fn(self._table(), ids, val, k, diversity, **kw)

    def recommend_capped(self, *inputs, k=20, item_category=None, max_per_category=None, rule=None, pool=None, exclude_seen=False,
                         item_bias=None, item_group=None, renormalize=False, return_complete=False):
        """(log_probs fp32 [B,k], item_ids int32 [B,k]) in served order: the first k items of recommend()'s order, with the same
        keywords, that respect "at most m items of one category (brand, seller) in the list", 1 <= k <= 4096.  Walking the
        served order and skipping an item once its category is full is the optimum under such caps (a partition matroid), so
        the catalogue pass stays what it is and ONE more launch walks the ordered pool (csrc/cap_select.hip; ops.cap_select,
        one workgroup per session, integer logic only): no [B, 4096] host read, no Python loop per session.  The values are
        the pool's own numbers at the kept items, bit for bit; a list that runs short ends in (-inf, -1) slots.
        The rule: either item_category ([num_items] integers over GLOBAL item ids, -1 = no category, never capped) with
        max_per_category (an int >= 0 for every category, or one cap per category; 0 = never shown) - ops.cap_rule builds the
        record at the price of one device-to-host read - or rule=, the record itself, which a server builds once.  Not both.
        The pool: pool=P (k <= P <= 4096) takes that pool alone - recommend(k=P) for P <= 128, recommend_many(k=P) beyond.
        pool=None with k <= 128: the one-pass pool of 128 items first; a session is COMPLETE when it kept k items or the pool's
        last slot is unfilled (the pool was the whole eligible catalogue); ONE device-to-host read of "any session incomplete"
        follows, and if so the WHOLE batch is re-run on a 4096-item pool and that result is returned - one pool per call, so
        the values never mix two kernels' round-off.  pool=None with k > 128: the 4096-item pool directly.
        return_complete=True adds a bool [B]: False where even the last pool used was full and gave fewer than k items (the
        catalogue may hold more that fit).  exclude_seen, item_bias / item_group, renormalize, mixtures (MSGIFSR fusion /
        extra) and row-sharded tables mean what they mean in recommend(): the caps themselves need no collective
        (dist.VocabParallel.cap_select), and where every rank feeds its own sessions the "any session incomplete" flag is
        max-all-reduced first, so that all ranks enter the 4096-item pool's collectives together or not at all.  Runs
        in eval mode under torch.no_grad(); k, pool, the rule and item_bias / item_group are checked before anything of the
        model runs (ValueError).
        Out of scope: caps together with sample() or recommend_diverse(), more than one attribute per item, minimum quotas
        (recommend_calibrated is the soft answer to those), and served_rank() / rank_items() under caps."""
        who = 'recommend_capped'
        k = ops.cap_k(who, k)
        if pool is not None:
            pool = int(pool)
            if not k <= pool <= ops.CONST['SREC_CAP_MAXP']:
                raise ValueError('%s: pool = %d; it holds at least the k = %d items asked for and at most %d (recommend_many()\'s '
                                 'limit)' % (who, pool, k, ops.CONST['SREC_CAP_MAXP']))
        rule = self._cap_rule(who, item_category, max_per_category, rule)
        bias = self._item_bias(who, item_bias, item_group)
        stages = [pool] if pool is not None else [128, ops.CONST['SREC_CAP_MAXP']] if k <= 128 else [ops.CONST['SREC_CAP_MAXP']]
        fn, kw = self._route('cap')
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            for P in stages:
                val, ids = self._run(q, 'select' if P <= 128 else 'select_many', P)
                pval, pick, kept, _ = fn(ids, val, rule, k, **kw)
                complete = (kept == k) | (ids[:, -1] < 0)
                if P == stages[-1] or not self._any_session(~complete):      # (the one device-to-host read, only with a stage to go)
                    break
            picked = ids.gather(1, pick.clamp(min=0).long())
            out = pval, torch.where(pick < 0, torch.full_like(picked, -1), picked)
            return out + (complete,) if return_complete else out

    def recommend_personal(self, *inputs, k=20, personal_items, personal_bias=None, pool=None, exclude_seen=False, item_bias=None,
                           item_group=None, return_complete=False):
        """(log_probs fp32 [B,k], item_ids int32 [B,k]) in served order: recommend()'s top-k under the same keywords with a
        sparse list of items PER SESSION re-scored - "never show this user what they bought or dismissed", "page 2 without
        page 1", "discount what was shown without a click", "lift what is in the cart" - without the dense [B, V] bias that
        item_bias [B, V] with item_group = arange(B) would be.  personal_items: [B, M] integer ids, or [M] shared by all
        sessions, -1 = padding - or Python lists, one per session, of unequal length; M <= 1024 and every id at most once
        per session.  personal_bias: shaped like personal_items, floating, ADDED to the listed item's value (-inf hides it);
        None: none of the listed items is ever shown.  A listed item's value is score_items(same keywords) of it plus its bias
        (one fp32 add; an item that scores -inf - the session's own under exclude_seen, item_bias -inf - stays out whatever its
        bias); every other value is the pool's own number, bit for bit.  A list that runs short ends in (-inf, -1) slots.
        If M items of a session change their value, its new top-k is the top-k of (the old top-(k + M) without them) and (the M
        items re-scored): the catalogue pass stays what it is, score_items() gives the M base values and ONE more launch merges
        the two per session (csrc/personal.hip; ops.personal_merge).  1 <= k, k + M <= 4096.
        The pool: pool=P (k <= P <= 4096) takes that pool alone - recommend(k=P) for P <= 128, recommend_many(k=P) beyond.
        pool=None with k + M <= 128: one pool of k + M items, always complete.  pool=None with k <= 128 < k + M: the one-pass
        pool of 128 first; with hit = the pool's items on the session's list, a session is COMPLETE when 128 - hit >= k or the
        pool's last slot is unfilled (the pool was the whole eligible catalogue); ONE device-to-host read of "any session
        incomplete" follows, and if so the WHOLE batch is re-run on recommend_many(k + M) and that result is returned - one
        pool per call, so the values never mix two kernels' round-off.  pool=None with k > 128: k + M directly.
        return_complete=True adds a bool [B]: False where the list may differ from the top-k of the adjusted catalogue (only
        with pool= too small for the list).  exclude_seen, item_bias / item_group, mixtures (MSGIFSR fusion / extra) and
        row-sharded tables mean what they mean in recommend(): the merge needs no collective
        (dist.VocabParallel.personal_merge), under data-parallel feeding the lists travel with the rank's own sessions, and
        the "any session incomplete" flag is max-all-reduced first, so that all ranks enter the larger pool's collectives
        together or not at all.  Runs in eval mode under torch.no_grad(); k, pool, the lists and item_bias / item_group are
        checked before anything of the model runs (ValueError; one device-to-host read for the lists).
        Out of scope: renormalize=True (the normaliser would need the listed items' mass corrected, and that subtraction
        cancels in fp32: there is no such keyword); lists together with sample(), cutoff(), recommend_diverse() /
        recommend_capped() / recommend_calibrated(); served_rank() / rank_items() under lists; more than 1024 listed items."""
        who, pmax = 'recommend_personal', ops.CONST['SREC_CAP_MAXP']
        lists = ops.personal_lists(who, personal_items, personal_bias, None, self._num_items(), self._table().device)
        M = lists.M
        k = ops.personal_k(who, k, M)
        if pool is not None:
            pool = int(pool)
            if not k <= pool <= pmax:
                raise ValueError('%s: pool = %d; it holds at least the k = %d items asked for and at most %d (recommend_many()\'s '
                                 'limit)' % (who, pool, k, pmax))
        bias = self._item_bias(who, item_bias, item_group)
        stages = [pool] if pool is not None else [128, k + M] if k <= 128 < k + M else [k + M]
        fn, kw = self._route('personal')
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=False, **bias)
            B = q.srs[0].shape[0]
            if lists.items.shape[0] not in (1, B):
                raise ValueError('%s: personal_items for %d sessions, the batch has %d' % (who, lists.items.shape[0], B))
            items = lists.items.expand(B, M).contiguous()
            pbias = None if lists.bias is None else lists.bias.expand(B, M).contiguous()
            base = self._run(q, 'score_items', items)
            for P in stages:
                val, ids = self._run(q, 'select' if P <= 128 else 'select_many', P)
                pval, pids, _, hit, _ = fn(ids, val, items, base, pbias, k, **kw)
                complete = (hit <= P - k) | (ids[:, -1] < 0)
                if P == stages[-1] or not self._any_session(~complete):      # (the one device-to-host read, only with a stage to go)
                    break
            return (pval, pids, complete) if return_complete else (pval, pids)

    def _any_session(self, flag):
        """host bool: is flag [B] set for any session of the call - of ANY rank's sessions over a sharded table fed
        data-parallel (dist.VocabParallel.any_session: one small all-reduce), so that every rank takes the same branch
        between two sharded calls, which are chains of collectives.  One device-to-host read"""
        if self.shard is not None:
            return self.shard.any_session(flag, data_parallel=self.shard.eval_data_parallel)
        return bool(flag.any())

    def _cap_rule(self, who, item_category, max_per_category, rule):
        """the ops.CapRule of recommend_capped on the table's device: `rule` as given (its category covers the catalogue) or
        built from item_category / max_per_category - one of the two, ValueError otherwise"""
        pair = item_category is not None or max_per_category is not None
        if (rule is not None) == pair or (pair and (item_category is None or max_per_category is None)):
            raise ValueError('%s: give either rule= (the record of ops.cap_rule) or item_category= with max_per_category=' % who)
        n, dev = self._num_items(), self._table().device
        if rule is None:
            return ops.cap_rule(n, item_category, max_per_category, device=dev)
        rule = ops.cap_rule_check(who, rule)
        if rule.category.numel() != n:
            raise ValueError('%s: the rule covers %d items, the catalogue has %d' % (who, rule.category.numel(), n))
        return ops.CapRule(rule.category.to(dev), rule.caps.to(dev), rule.G)

    def recommend_calibrated(self, *inputs, k=20, weight=0.5, item_category=None, target=None, alpha=0.01, pool=None,
                             exclude_seen=False, item_bias=None, item_group=None, renormalize=False, return_kl=False):
        """(log_probs fp32 [B,k], item_ids int32 [B,k]) in PICK order: a slate of k items whose category mix follows the
        session's own - CALIBRATION (Steck, "Calibrated Recommendations", RecSys 2018), the soft counterpart of
        recommend_capped's hard caps and the answer to "minimum quotas": a session that was 70 % shoes and 30 % socks gets a
        list of roughly that mix, and no per-category number is asked of the operator.  The greedy re-rank (csrc/calibrate.hip,
        ops.calibrate: ONE more launch, one workgroup per session, no loop of launches) of the `pool` most probable items.
        The pool is exactly what recommend(k=pool, same keywords) returns (pool: default min(128, max(4 k, k)); k <= pool
        <= 128), so exclude_seen, item_bias / item_group, renormalize, mixtures and row-sharded tables mean what they mean
        there (the re-rank itself needs no collective: dist.VocabParallel.calibrate).
        item_category: [num_items] integers over GLOBAL item ids, < 0 = the item has no category; moved to the table's device
        once - an int32 tensor already there is taken as it is, with no device read (category ids are only compared: any
        int32 is fine).  target=None: the session's own DISTINCT items (_session_items), weight 1 each, through
        item_category - how often an item was clicked is not seen.  target=(cats [B,T], weights [B,T]): an explicit sparse
        target of category ids (not item ids) and weights >= 0, finite; a category < 0 or a weight 0 is an empty pair,
        duplicates add up; at most 128 pairs per session (ValueError otherwise, also for a batch with a session of more
        than 128 distinct items under target=None).  A session without any pair has no target: it gets the plain order.
        With p the target distribution over its categories S, n_c the picks of category c and N the picks with any category,
          KL = sum_{c in S} p_c log(p_c / ((1 - alpha) n_c / max(N, 1) + alpha p_c))
        and step t picks the pool slot with the largest (1 - weight) value - weight KL(picks so far + the slot), ties to the
        better-ranked slot; weight in [0, 1], alpha in (0, 1).  weight=0 returns the first k columns of recommend(k=pool).
        The values are the pool's own numbers at the picks, bit for bit; unfilled slots (fewer than k eligible items) are
        (-inf, -1).  return_kl=True adds kl fp32 [B], the KL of the returned list (list_calibration of it).  Runs in eval
        mode under torch.no_grad(); k, weight, alpha, pool, item_category, the target and item_bias / item_group are
        checked before anything of the model runs.
        Out of scope: calibration together with caps, MMR (recommend_diverse) or sampling, pools beyond 128, several
        categories per item, recency-weighted default targets, and served_rank() / rank_items() under calibration."""
        who = 'recommend_calibrated'
        k, weight, alpha = ops.calibrate_scalars(who, k, weight, alpha)
        pool = min(128, max(4 * k, k)) if pool is None else int(pool)
        if not k <= pool <= 128:
            raise ValueError('%s: pool = %d; it holds at least the k = %d items asked for and at most 128 (recommend()\'s limit)'
                             % (who, pool, k))
        category = self._item_category(who, item_category)
        tcat, tw = self._calibration_target(who, category, target, inputs)
        bias = self._item_bias(who, item_bias, item_group)
        fn, kw = self._route('calibrate')
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            val, ids = self._run(q, 'select', pool)
            pval, pick, _, kl = fn(ids, val, category, k, weight, tcat, tw, alpha, **kw)
            picked = ids.gather(1, pick.clamp(min=0).long())
            out = pval, torch.where(pick < 0, torch.full_like(picked, -1), picked)
            return out + (kl,) if return_kl else out

    def list_calibration(self, *inputs, item_ids, item_category=None, target=None, alpha=0.01):
        """fp32 [B]: how far the category mix of given lists is from the target's - the KL of recommend_calibrated (0 for a
        session without a target) - the number that compares a plain, a diversified, a capped and a calibrated list.
        item_ids: [B, M] integer ids, -1 = padding, M <= 128; an id < -1 or >= num_items raises ValueError before anything
        is launched.  item_category, target (None: the distinct items of the sessions in `inputs`) and alpha as in
        recommend_calibrated.  The kernel of recommend_calibrated at weight 0 over zero values with k = M; the model itself
        does not run.  Under torch.no_grad()."""
        who = 'list_calibration'
        ids = item_ids.detach()
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() != 2:
            raise ValueError('%s: item_ids must be an integer tensor [B, M], got %s %s' % (who, ids.dtype, tuple(ids.shape)))
        M = ids.shape[1]
        _, _, alpha = ops.calibrate_scalars(who, M, 0.0, alpha, M)
        category = self._item_category(who, item_category)
        tcat, tw = self._calibration_target(who, category, target, inputs)
        self._check_ids(who, ids)
        fn, kw = self._route('calibrate')
        with torch.no_grad():
            ids = ids.to(category.device)
            return fn(ids, torch.zeros(ids.shape, device=ids.device, dtype=torch.float32), category, M, 0.0, tcat, tw, alpha, **kw)[3]

    def _item_category(self, who, item_category):
        """item_category as int32 [num_items] on the table's device.  An int32 tensor there is taken as it is (no device read:
        the kernel only compares category ids); anything else is converted at the price of one read of its extremes"""
        if item_category is None:
            raise ValueError('%s: item_category= (the category of every item, [num_items] integers) is needed' % who)
        n, dev = self._num_items(), self._table().device
        cat = ops._int_vector(who, 'item_category', item_category, None)
        if cat.numel() != n:
            raise ValueError('%s: item_category has %d entries for %d items' % (who, cat.numel(), n))
        if cat.dtype == torch.int32:
            return cat.to(dev).contiguous()
        if n > 0 and int(cat.max()) > 2 ** 31 - 1:
            raise ValueError('%s: item_category holds a category id beyond int32' % who)
        return cat.clamp(min=-1).to(device=dev, dtype=torch.int32).contiguous()

    def _calibration_target(self, who, category, target, inputs):
        """(tcat int32 [B,T], tw fp32 [B,T]) on the device of category, or (None, None) for T = 0.  target=None: the sessions'
        own distinct items through category, weight 1 each.  target=(cats, weights): checked - shapes, dtypes, at most
        SREC_CALIB_MAXT pairs, weights finite and >= 0 (one device-to-host read)"""
        tmax, dev = ops.CONST['SREC_CALIB_MAXT'], category.device
        if target is None:
            if not inputs:
                raise ValueError('%s: target=None takes the sessions\' own items: give the model\'s inputs, or target=' % who)
            listed = self._session_items(inputs[0]).to(dev).long()
            if listed.shape[1] > tmax:
                raise ValueError('%s: a session of %d distinct items; the target holds at most %d pairs per session'
                                 % (who, listed.shape[1], tmax))
            if listed.shape[1] == 0 or category.numel() == 0:
                return None, None
            cats = category[listed.clamp(0, category.numel() - 1)]
            return torch.where(listed < 0, torch.full_like(cats, -1), cats).contiguous(), torch.ones(listed.shape, device=dev)
        try:
            cats, weights = target
            cats, weights = torch.as_tensor(cats).detach(), torch.as_tensor(weights).detach()
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('%s: target must be a pair (categories [B, T], weights [B, T])' % who) from None
        if cats.is_floating_point() or cats.is_complex() or cats.dtype == torch.bool or cats.dim() != 2:
            raise ValueError('%s: the target\'s categories must be an integer tensor [B, T], got %s %s' % (who, cats.dtype, tuple(cats.shape)))
        if not weights.is_floating_point() or weights.shape != cats.shape:
            raise ValueError('%s: the target\'s weights must be a floating tensor %s like its categories, got %s %s'
                             % (who, tuple(cats.shape), weights.dtype, tuple(weights.shape)))
        if cats.shape[1] > tmax:
            raise ValueError('%s: %d target pairs per session; at most %d' % (who, cats.shape[1], tmax))
        if cats.shape[1] == 0:
            return None, None
        weights = weights.to(device=dev, dtype=torch.float32)
        if not bool((torch.isfinite(weights) & (weights >= 0)).all()):          # the one device-to-host read
            raise ValueError('%s: the target holds a NaN, infinite or negative weight' % who)
        cats = cats.to(dev)
        if cats.dtype != torch.int32:
            cats = torch.where((cats < 0) | (cats > 2 ** 31 - 1), torch.full_like(cats, -1), cats).to(torch.int32)
        return cats.contiguous(), weights.contiguous()

    def list_diversity(self, item_ids):
        """fp32 [B]: the intra-list diversity of given lists, 1 - the mean cosine between the item-table rows of every pair of
        a list's items (the similarity of recommend_diverse; 0 for a list with fewer than two items) - the number that
        compares a plain top-N with a diversified one.  item_ids: [B, M] integer ids, -1 = padding, M <= 128; an id < -1 or
        >= num_items raises ValueError before anything is launched.  The kernel of recommend_diverse with diversity 0 and
        k = M; sharded table included.  Runs under torch.no_grad()."""
        ids = item_ids.detach()
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() != 2:
            raise ValueError('list_diversity: item_ids must be an integer tensor [B, M], got %s %s' % (ids.dtype, tuple(ids.shape)))
        B, M = ids.shape
        ops.diversify_scalars('list_diversity', M, 0.0, M)
        self._check_ids('list_diversity', ids)
        with _Serving(self):
            ids = ids.to(self._table().device)
            return self._diversify(ids, torch.zeros(ids.shape, device=ids.device, dtype=torch.float32), M, 0.0)[3]

    def _scoring_args(self, *inputs, exclude_seen, raw=False):
        """the Query (srs, cs, off_ex, off_in, listed; drop = exclude_seen, no bias) under which the score of ops.score_select /
        score_items / score_norm, logsumexp_c(z_c[b,v] + off_c[b]), is what forward() returns: one soft-max here, off_ex = -lse.  listed: the
        session's own items when exclude_seen drops them.  raw=True (the caller normalises over the eligible items itself):
        the full-catalogue statistics pass is skipped and off_ex is None - the score is the raw logit."""
        sr = self.session_repr(*inputs)
        st = self._state(sr.shape[0])
        cs, inv_scale = self._col_scale(st)
        off_ex = None if raw else -self._lse(sr, cs, inv_scale, st).unsqueeze(0)      # log softmax = z - lse
        listed = self._session_items(inputs[0]) if exclude_seen else None
        return Query([sr], cs, off_ex, None, listed, exclude_seen)

    def _served(self, *inputs, exclude_seen, renormalize, **bias):
        """the Query of _scoring_args with the bias keywords; renormalize with something to renormalise (a bias or
        exclude_seen): the offsets minus Z, the log-normaliser over the eligible items, so that the kernels return s - Z (a session with nothing eligible: Z = -inf,
        offsets unchanged - all its slots are -inf anyway)"""
        todo = bool(renormalize) and (bool(bias) or bool(exclude_seen))
        q = self._scoring_args(*inputs, exclude_seen=exclude_seen, raw=todo)._replace(bias=bias)
        if todo:
            Z = self._run(q, 'norm')
            Zs = torch.where(Z == float('-inf'), torch.zeros_like(Z), Z).unsqueeze(0)
            q = q._replace(off_ex=-Zs if q.off_ex is None else q.off_ex - Zs,
                           off_in=None if q.off_in is None else q.off_in - Zs)
        return q

    def log_mass(self, *inputs, exclude_seen=False, item_bias=None, item_group=None):
        """fp32 [B]: the log of the probability mass, under forward()'s distribution, of the items a filter leaves - the
        items recommend() could return with the same keywords (not the session's own under exclude_seen, item_bias > -inf);
        with a finite bias the log-partition of the tilted distribution, log sum_v p_model(v) exp(bias_v).  0 up to round-off
        without a filter, -inf for a session with nothing eligible.  It is what renormalize=True subtracts.  One fused pass
        over the table (csrc/score_norm.hip), no (B, V) matrix, sharded table included; eval mode under torch.no_grad(),
        item_bias / item_group checked first as in recommend()."""
        bias = self._item_bias('log_mass', item_bias, item_group)
        with _Serving(self):
            return self._run(self._scoring_args(*inputs, exclude_seen=exclude_seen)._replace(bias=bias), 'norm')

    @staticmethod
    def _session_items(mg):
        """dense int32 [B, L] view of every session's distinct items (-1 = empty slot), from the batch's segment offsets
        and item ids (the order-1 nodes of a k-gram batch); L = the longest session of the batch"""
        ccs = mg.meta.get('kind') == 'ccs'
        seg = mg.field('seg1' if ccs else 'seg').long()[:mg.B + 1]
        iid = mg.field('iid1' if ccs else 'iid').long()
        L = max(1, int((seg[1:] - seg[:-1]).max())) if seg.numel() > 1 else 1
        pos = seg[:-1, None] + torch.arange(L, device=seg.device)[None, :]
        items = iid[pos.clamp(max=iid.numel() - 1)]
        return torch.where(pos < seg[1:, None], items, torch.full_like(items, -1)).to(torch.int32)

    @staticmethod
    def _cutoff_args(who, top_k, top_p, min_p, temperature):
        """the criteria as the 'cutoff' route takes them, checked (ops.cutoff_scalars); None when none of the three is given"""
        if top_k is None and top_p is None and min_p is None:
            return None
        ops.cutoff_scalars(who, top_k, top_p, min_p, temperature)
        return dict(top_k=top_k, top_p=top_p, min_p=min_p, temperature=temperature)

    def cutoff(self, *inputs, top_k=None, top_p=None, min_p=None, temperature=1.0, exclude_seen=False, item_bias=None,
               item_group=None, renormalize=False):
        """(floor fp32 [B], count int32 [B], log_kept fp32 [B]): where truncated sampling cuts every session's distribution -
        what sample(top_k=, top_p=, min_p=, temperature=, same keywords) draws inside.  floor is in the units of recommend()'s
        values (log-probability plus bias; renormalize=True: under the distribution restricted to the eligible catalogue): an
        eligible item is kept when its value is >= floor.  top_k: keep the k most probable items (any k, not limited to 128;
        ties with the k-th are kept); top_p: the smallest set of most probable items holding probability p AT THE GIVEN
        TEMPERATURE, i.e. under p(v) ~ exp(value_v / temperature) (ties at the boundary are kept); min_p = q: the items at least
        q times as probable as the best one, at that temperature.  Several criteria: the largest floor.  None: floor = -inf.
        count: the number of kept items; log_kept: the log of the share of that distribution they hold (<= 0).  At
        temperature=1, value - log_kept is an item's log-probability INSIDE the kept set.  A session with nothing eligible
        gives (-inf, 0, -inf).  Fused passes over the table (csrc/score_cutoff.hip; ops.score_cutoff): no (B, V) matrix, no
        sort, sharded table included.  Runs in eval mode under torch.no_grad(); the arguments are checked before anything of
        the model runs."""
        bias = self._item_bias('cutoff', item_bias, item_group)
        ops.cutoff_scalars('cutoff', top_k, top_p, min_p, temperature)
        crit = dict(top_k=top_k, top_p=top_p, min_p=min_p, temperature=temperature)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            return self._run(q, 'cutoff', **crit)[:3]

    def sample(self, *inputs, k=1, temperature=1.0, seed=0, session_keys=None, exclude_seen=False, item_bias=None,
               item_group=None, renormalize=False, top_k=None, top_p=None, min_p=None):
        """(log_probs fp32 [B,k], item_ids int32 [B,k] in DRAW order): k distinct next items per session drawn without
        replacement from the model's distribution - p(v) ~ exp((log p_model(v) + bias_v) / temperature) over the items
        recommend() could return with the same keywords (not the session's own under exclude_seen, item_bias > -inf); k <= 128.
        One fused pass over the table (csrc/recommend.hip with Gumbel noise; ops.score_sample): no (B, V) matrix, no (B, V)
        noise, sharded table included.  seed: an integer in [0, 2^64); session_keys: [B] integers, None = the row index of
        the batch - a session with the same (seed, key) draws the same items in any batch, on any number of shards
        (ops.sample_noise restates the noise).  The VALUES are not the sampled keys: they are what score_items(items=ids)
        returns with the same keywords, bit for bit - forward()'s log-probabilities (plus bias; renormalize=True: under the
        distribution restricted to the eligible catalogue) at temperature 1, the number an off-policy log needs.  A session
        with fewer than k eligible items ends in (-inf, -1) slots.  Runs in eval mode under torch.no_grad(); item_bias /
        item_group, k, temperature and seed are checked before anything of the model runs.
        top_k / top_p / min_p: TRUNCATED sampling - the draw is among the items cutoff() keeps for the same keywords and
        temperature (the k most probable, the nucleus of mass p, the items at least q times as probable as the best; several:
        the smallest set).  The floor is found with the very offsets of the draw (csrc/score_cutoff.hip, no (B, V) matrix).  The
        values stay what score_items returns - they are NOT renormalised over the kept set (cutoff()'s log_kept is that
        normaliser) - and a session that keeps fewer than k items ends in (-inf, -1) slots.  With none of the three the call is
        what it was, bit for bit."""
        bias = self._item_bias('sample', item_bias, item_group)
        k, _, seed = ops.sample_scalars('sample', k, temperature, seed)
        crit = self._cutoff_args('sample', top_k, top_p, min_p, temperature)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            cut = {} if crit is None else dict(floor=self._run(q, 'cutoff', **crit)[0])
            _, ids = self._run(q, 'sample', k, temperature=temperature, seed=seed, session_keys=session_keys, **cut)
            return self._run(q, 'score_items', ids), ids

    def served_rank(self, *inputs, labels, exclude_seen=False, item_bias=None, item_group=None, top_k=None, top_p=None, min_p=None,
                    temperature=1.0):
        """int32 [B]: the rank of every session's label among what is SERVED - the number of items recommend() / sample() could
        return with the same keywords (not the session's own under exclude_seen, item_bias > -inf, inside the kept set of
        top_k / top_p / min_p at `temperature`) that stand ahead of the label under recommend()'s order (log-probability plus
        bias, ties towards the lower item id).  target_rank() is this number for the unfiltered model; every HR / MRR / NDCG @k
        of what users are shown follows from it (train.metrics_from_served_ranks, train.evaluate_served).
          -1: the session has no label (labels[b] < 0).
          -2: the label could NOT have been shown: its served value is -inf - it is the session's own item under exclude_seen,
              its item_bias is -inf, or it merely scores -inf, which counts as not shown by definition - or it lies below the
              truncation floor.  A miss at every cutoff.
          otherwise the count r >= 0: when r < k <= 128 the label sits at position r of recommend(k=k, same keywords).
        The label's own value is what score_items() returns for it; one more fused pass over the table counts the eligible
        items ahead of it (csrc/rank_served.hip; ops.score_ahead), listed items and the bias resolved inside the pass: no (B, V)
        score matrix, sharded table included (one integer all-reduce).  Renormalising shifts a session's values by a constant
        and cannot change a rank, so there is no renormalize keyword.  Runs in eval mode under torch.no_grad(); item_bias /
        item_group, the labels (integers below num_items) and the truncation keywords are checked before anything of the
        model runs (ValueError)."""
        bias = self._item_bias('served_rank', item_bias, item_group)
        n = self._num_items()
        lab = torch.as_tensor(labels).detach()
        if lab.is_floating_point() or lab.is_complex() or lab.dtype == torch.bool:
            raise ValueError('served_rank: labels must be an integer tensor (one item id per session), got %s' % lab.dtype)
        lab = lab.reshape(-1).to(torch.int64)
        if lab.numel() > 0 and int(lab.max()) >= n:
            raise ValueError('served_rank: label %d; item ids are in [0, %d), or negative for a session without a label'
                             % (int(lab.max()), n))
        ops.cutoff_scalars('served_rank', top_k, top_p, min_p, temperature)
        crit = self._cutoff_args('served_rank', top_k, top_p, min_p, temperature)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=False, **bias)
            lab = lab.to(q.srs[0].device).clamp(min=-1)
            if lab.numel() != q.srs[0].shape[0]:
                raise ValueError('served_rank: %d labels for %d sessions' % (lab.numel(), q.srs[0].shape[0]))
            return self._ranks_among_served(q, lab[:, None], crit)[:, 0]

    def _ranks_among_served(self, q, ids, crit):
        """int32 [B, M], the tail of served_rank (M = 1) and rank_items: the rank of the items ids [B, M] (int64 on the device,
        checked; < 0 = empty slot) under the Query q and the criteria of _cutoff_args (None: no truncation) - their values
        by the score_items route, the floor by the cutoff route, the eligible items ahead by one counting pass (M = 1:
        ahead, else ahead_many); -2 where the value is -inf or below the floor, -1 in an empty slot"""
        target = self._run(q, 'score_items', ids)
        cut = {} if crit is None else dict(floor=self._run(q, 'cutoff', **crit)[0])
        if ids.shape[1] == 1:
            ahead = self._run(q, 'ahead', ids[:, 0].to(torch.int32), target[:, 0], **cut)[:, None]
        else:
            ahead = self._run(q, 'ahead_many', ids.to(torch.int32), target, **cut)
        shown = target > float('-inf')
        if cut:
            shown = shown & ~(target < cut['floor'][:, None])           # (the kernels' own test of a floor)
        out = torch.where(shown, ahead, torch.full_like(ahead, -2))
        return torch.where(ids < 0, torch.full_like(ahead, -1), out)

    def rank_items(self, *inputs, items, exclude_seen=False, item_bias=None, item_group=None, top_k=None, top_p=None, min_p=None,
                   temperature=1.0):
        """int32 [B, M]: the rank of each of M given items per session among what is SERVED - served_rank() for several items
        at once, the counterpart of score_items(): rest-of-session evaluation (every remaining item of a session is relevant;
        train.evaluate_rest, train.metrics_from_item_ranks) and "where would these items land?" (a campaign, a re-ranker's
        candidates).  items: [B, M] item ids per session or [M] shared by all sessions, any integer dtype, M <= 64, -1 =
        padding; an id may not appear twice in a row.
          -1: an empty slot.
          -2: the item could NOT be shown: its served value is -inf (the session's own item under exclude_seen, item_bias -inf,
              or a score of -inf) or it lies below the truncation floor.
          otherwise the rank r >= 0: when r < k <= 128 the item sits at position r of recommend(k=k, same keywords).
        The rank counts the eligible items ahead - the catalogue's by the counting pass, the session's other given items by the
        values score_items() returns for them - so the shown items of a session always get pairwise distinct ranks, in
        recommend()'s order.  The values come from the gather kernel; ONE more fused pass over the table compares every score
        with the session's M thresholds (csrc/rank_served_many.hip; ops.score_ahead_many), instead of M passes of served_rank():
        no (B, V) score matrix, sharded table included (one integer all-reduce).  M = 1 takes served_rank()'s route.  There is
        no renormalize keyword: a per-session constant shifts no rank.  Runs in eval mode under torch.no_grad(); item_bias /
        item_group, the items and the truncation keywords are checked before anything of the model runs (ValueError), at the
        price of the one device-to-host read score_items() pays."""
        bias = self._item_bias('rank_items', item_bias, item_group)
        ids = torch.as_tensor(items).detach()
        if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() not in (1, 2):
            raise ValueError('rank_items: items must be an integer tensor [B, M] or [M], got %s %s' % (ids.dtype, tuple(ids.shape)))
        M = ids.shape[-1]
        if not 1 <= M <= ops.CONST['SREC_AHEAD_MAXT']:
            raise ValueError('rank_items: %d items per session; between 1 and %d are ranked in one call'
                             % (M, ops.CONST['SREC_AHEAD_MAXT']))
        ids = ids.to(torch.int64)
        if ids.numel() > 0:
            rows = ids.reshape(-1, M).sort(dim=1).values
            dup = ((rows[:, 1:] == rows[:, :-1]) & (rows[:, 1:] >= 0)).any()
            lo, hi, dup = torch.stack([ids.min(), ids.max(), dup.to(torch.int64)]).tolist()      # the one device-to-host read
            self._check_id_range('rank_items', lo, hi)
            if dup:
                raise ValueError('rank_items: an item id appears twice in a row of items; every id at most once per session')
        ops.cutoff_scalars('rank_items', top_k, top_p, min_p, temperature)
        crit = self._cutoff_args('rank_items', top_k, top_p, min_p, temperature)
        with _Serving(self):
            q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=False, **bias)
            B = q.srs[0].shape[0]
            if ids.dim() == 2 and ids.shape[0] != B:
                raise ValueError('rank_items: items for %d sessions, the batch has %d' % (ids.shape[0], B))
            return self._ranks_among_served(q, ids.to(q.srs[0].device).expand(B, M).contiguous(), crit)

    def score_items(self, *inputs, items, exclude_seen=False, item_bias=None, item_group=None, renormalize=False):
        """fp32 [B, M]: the log-probability forward() returns at the given items of every session - full-catalog soft-max
        (or mixture), never renormalised over the CANDIDATES (log_softmax over the returned row is the caller's one-liner).  items: [B, M] item ids per session or [M] shared by all
        sessions, any integer dtype, any M; -1 is padding and gives -inf; duplicates are allowed.  exclude_seen=True gives
        -inf at the session's own items (at most 64 distinct items per session) and leaves the rest unchanged.  An id
        < -1 or >= num_items raises ValueError before anything is launched.  One gather pass over the candidates' rows
        (csrc/score_items.hip): no (B, V) score matrix, sharded table included.  Runs in eval mode under torch.no_grad().
        item_bias / item_group as in recommend(): the values are forward()'s log-probabilities PLUS the bias (-inf stays
        -inf); checked before anything is launched (_item_bias: one more device-to-host read).
        renormalize as in recommend(): True gives log-probabilities under the distribution restricted to the eligible
        CATALOGUE (every item exclude_seen and item_bias leave, whether it is among the candidates or not) and tilted by the
        bias - the numbers recommend(renormalize=True) returns for the same items."""
        bias = self._item_bias('score_items', item_bias, item_group)
        self._check_ids('score_items', items)
        with _Serving(self):
            return self._score_items(*inputs, items=items, exclude_seen=exclude_seen, renormalize=renormalize, **bias)

    def _score_items(self, *inputs, items, exclude_seen, renormalize=False, **bias):
        q = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
        return self._run(q, 'score_items', items.to(q.srs[0].device))

    def rerank(self, *inputs, items, k=None, exclude_seen=False, item_bias=None, item_group=None, renormalize=False):
        """(log_probs fp32 [B, n], item_ids int32 [B, n]), n = M or min(k, M): the candidates of score_items ordered by
        (value descending, id ascending) - the contract of recommend()'s lists without its limit of 128.  Slots that score
        -inf (padding, the session's own items under exclude_seen, and items whose item_bias is -inf) come last with id -1; a
        candidate named twice is returned twice.  item_bias / item_group as in score_items(): ordered by log-probability PLUS
        bias.  renormalize as in score_items(): the normaliser is over the eligible CATALOGUE, not over the candidates - the
        order is unchanged."""
        val = self.score_items(*inputs, items=items, exclude_seen=exclude_seen, item_bias=item_bias, item_group=item_group,
                               renormalize=renormalize)
        ids = items.to(val.device).to(torch.int64)
        ids = torch.where(val == float('-inf'), torch.full_like(val, -1, dtype=torch.int64), ids.expand_as(val))
        # two stable sorts, as the merge of dist.VocabParallel.select: by id (unfilled slots last), then by value
        o = torch.argsort(torch.where(ids < 0, torch.full_like(ids, 2 ** 62), ids), dim=1, stable=True)
        val, ids = val.gather(1, o), ids.gather(1, o)
        o = torch.argsort(val, dim=1, descending=True, stable=True)
        if k is not None:
            o = o[:, :max(int(k), 0)]
        return val.gather(1, o).contiguous(), ids.gather(1, o).to(torch.int32).contiguous()
