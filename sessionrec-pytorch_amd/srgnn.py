"""SRGNN and NISER on the HIP path - host-side mirror of
/root/reference/src/models/srgnn.py:93-148 and niser.py:91-157.

Same constructor signatures, parameter names and shapes (state_dicts interchange
with the reference / the oracle), same `forward(mg, sg=None) -> (B, num_items)`
log-probabilities.  The nn.Embedding / nn.Linear / nn.GRUCell children are
parameter containers only: all arithmetic goes through sessionrec-pytorch_amd.ops
(hand-written gfx950 kernels).  `fused_loss(mg, labels)` is the training entry the
TrainRunner uses: logits are never materialised and the dense table gradient is
written once, in place, by the scoring backward.

Reference quirk kept: the SRGNNLayer outputs are not consumed by the
readout (srgnn.py:135-142), so by default the layers are not even executed;
`use_gnn_output=True` runs them and feeds their output on (a documented extension).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


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


class _ScoringMixin:
    """Shared scoring head: fused CE for training, materialised log-probs for the forward() API."""

    def _table(self):
        return self.embedding.weight

    def _cosine(self):
        return None            # (scale, eps_mode) for cosine-scored models

    def _state(self, B):
        dev = self._table().device
        st = self.__dict__.setdefault('_srec_state', {})
        if st.get('dev') != dev:
            st.clear()
            st['dev'] = dev
            st['tgrad'] = ops.TableGrad(self._table(), defer=bool(getattr(self, '_defer_projection', False)))
            st['ws'] = {}
            st['cs'] = None
            st['cs_fresh'] = False
        if B not in st['ws']:
            V, d = self._table().shape
            st['ws'][B] = ops.CEWorkspace(B, V, d, dev)
        return st

    @property
    def table_grad(self):
        tg = self._state(1)['tgrad']
        tg.materialize()               # (a projection left to the optimizer is applied before anybody else looks)
        return tg

    def _col_scale(self, st):
        cos = self._cosine()
        if cos is None:
            return None, 1.0
        scale, eps_mode = cos
        W = self._table()
        if st['cs'] is None:
            st['cs'] = torch.empty(W.shape[0], device=W.device, dtype=torch.float32)
        if not st['cs_fresh']:
            from ._lib import lib, ptr, stream
            lib.srec_row_invnorm(ptr(W), W.stride(0), W.shape[0], W.shape[1], eps_mode, 1e-12, float(scale),
                                 ptr(st['cs']), stream())
        st['cs_fresh'] = False          # the optimizer sets it again after refreshing cs in its row pass
        return st['cs'], 1.0 / float(scale)

    def _prepare_table(self):
        """in-place, no-grad mutation of the table the reference's forward performs before reading it
        (Embedding(max_norm): lessr.py:126, msgifsr.py:162); called once per step ahead of everything that reads rows"""
        self._table_ready = False

    # FusedAdam's row pass over the table also leaves the rows renormalised (models with max_norm) and writes the bf16 operand
    # copy of the bf16 scoring kernels (optim.py: st['table_prepared']); the next forward then skips its stand-alone pass.
    # One device only: the row-sharded path refreshes its shard's copy itself (dist.HipLocal._tb).
    _fold_table_prep = True

    def _table_copy(self, st, W):
        """the TableBF16 the optimizer's row pass should fill (None: no bf16 scoring on this path).  Row-sharded table: the
        copy of this rank's LIVE rows that dist.HipLocal keeps (the scoring kernels read table[:n_live])."""
        if not ops.use_bf16_scoring(W.shape[1]) or not W.is_cuda:
            return None
        if self.shard is not None:
            local, n_live = self.shard.local, self.shard.n_live
            if not hasattr(local, '_tb') or n_live <= 0:
                return None
            live = W[:n_live] if n_live < W.shape[0] else W    # (the rows the scoring kernels read: VocabParallel._live)
            tb = local._tb(live, False)
            local._tb_written = ((live.data_ptr(), tuple(live.shape)), W._version)
            return tb
        if st.get('tb16') is None:
            st['tb16'] = ops.TableBF16(W)
        return st['tb16']

    def _take_prepared(self, st, mark=True):
        """(rows renormalised, bf16 copy written) by the optimizer's last row pass - consumed once, and only while the table
        has not been written through PyTorch since (copy_ / load_state_dict bump its version counter; the HIP kernels do not).
        mark: leave the "copy is fresh" note for the _table_bf16 call of THIS forward (_prepare_table runs ahead of it); the
        note carries the table version it was taken at, so a write through PyTorch in between voids it."""
        prep = st.pop('table_prepared', None) if st is not None else None
        if prep is None or prep[2] != self._table()._version:
            return False, False
        if mark and prep[1] and self.shard is None:
            self._tb16_fresh = self._table()._version    # consumed by _table_bf16 of this forward
        return prep[0], prep[1] and self.shard is None

    def _pop_tb16_fresh(self):
        """the note _prepare_table / _take_prepared left: valid for the table version it was written at only"""
        v = self.__dict__.pop('_tb16_fresh', None)
        return v is not None and v is not False and v == self._table()._version

    def table_written(self):
        """the table (or its optimizer state) was replaced from outside the step (load_state_dict, a restored checkpoint):
        every note about prepared rows / fresh bf16 copies is void"""
        self.__dict__.pop('_tb16_fresh', None)
        self.__dict__.pop('_table_ready', None)
        st = self.__dict__.get('_srec_state')
        if st is not None:
            st.pop('table_prepared', None)
            st['cs_fresh'] = False

    shard = None               # set by dist.VocabParallel(model): row-sharded table over the node's GPUs
    graph_capable = False      # True: every kernel of the step reads its live extents from the padded batch (hipGraph replay)

    def _lookup(self, idx, uniq, tgrad, dyn_n=None, dyn_u=None, drop=None, inv=None):
        """item rows for the batch: local gather, or the collective lookup when the table is sharded.  drop: an nn.Dropout
        applied to the rows - fused into the gather kernels on the single-device path."""
        p = drop.p if isinstance(drop, nn.Dropout) and drop.training else 0.0
        # the device step counter the dropout masks of THIS model's forward are keyed by (ops.rng_args): that of its own
        # FusedAdam, or none (another optimizer: the per-call nonce alone renews the masks)
        ops.flush_intake()          # (a captured step's batch intake: ahead of the first read)
        W = self._table()
        c = self.__dict__.get('_srec_rng_counter')
        if c is not None and c.device == W.device:
            ops.RNG_COUNTER[str(W.device)] = c
        else:
            ops.RNG_COUNTER.pop(str(W.device), None)
        if self.shard is not None:
            fused = p > 0 and getattr(self.shard.local, 'fused_dropout', False)      # HipLocal: the mask rides in the gather
            rows = self.shard.lookup(self._table(), idx, uniq, (p, 7) if fused else None, inv=inv)
            return rows if (fused or drop is None) else drop(rows)
        if drop is not None and not isinstance(drop, nn.Dropout):
            return drop(ops.embedding_lookup(self._table(), idx, uniq, tgrad, dyn_n, dyn_u))    # replaced module (tests)
        return ops.embedding_lookup(self._table(), idx, uniq, tgrad, dyn_n, dyn_u, (p, 7) if p > 0 else None)

    def fused_loss(self, *inputs_and_labels, dynB=None):
        *inputs, labels = inputs_and_labels
        B = labels.numel()
        if dynB is None and hasattr(inputs[0], 'dynp'):
            dynB = inputs[0].dynp('B')
        st = self._state(B)
        self._prepare_table()                        # Embedding(max_norm) renorm BEFORE the cosine column scale is taken
        cs, inv_scale = self._col_scale(st)
        if self.shard is not None:
            self.shard.labels_hint = labels          # gathered together with the lookup's request lists
        # bf16 scoring on one device: the model's final normalisation writes the session vectors' bf16 operand copy itself
        self._sr_ws = st['ws'][B] if (self.shard is None and ops.use_bf16_scoring(self._table().shape[1])) else None
        # every parameter of these models feeds exactly one backward node: the split-K sums of the small grouped backward
        # launches may wait for ONE launch at the end of the backward pass (ops.defer_scope; MSGIFSR switches it itself)
        defer = ops.STEP.may_defer or (self.training and self._table().is_cuda and getattr(self, 'defer_slab_sums', True))
        try:
            with ops.STEP.deferring(defer):
                sr = self.session_repr(*inputs, tgrad=st['tgrad'])
        finally:
            self._sr_ws = None
        if self.shard is not None:
            return self.shard.loss(sr, self._table(), cs, labels, inv_scale)
        loss, _ = ops.score_ce(sr, self._table(), cs, labels.to(torch.int32), st['ws'][B], st['tgrad'], dynB, inv_scale,
                               self._table_bf16(st))
        return loss

    def _table_bf16(self, st):
        """bf16 operand copies of the table for the bf16 scoring kernels (precision 'bf16'), refreshed per step"""
        W = self._table()
        if not ops.use_bf16_scoring(W.shape[1]):
            return None
        if st.get('tb16') is None:
            st['tb16'] = ops.TableBF16(W)
        if self._pop_tb16_fresh():                       # _prepare_table wrote the copy together with the renorm
            return st['tb16']
        if self._take_prepared(st, mark=False)[1]:       # the optimizer's row pass of the previous step wrote it
            return st['tb16']
        return st['tb16'].refresh(W)

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
            return self._rank_of([sr], cs, labels, None, None, None)

    # served call of dist.VocabParallel over a row-sharded table <-> (launcher of ops on one device, its own keywords)
    _ROUTES = {'target_rank': ('score_rank', {}), 'select': ('score_select', {}), 'sample': ('score_sample', {}),
               'select_many': ('score_select_many', {}),
               'norm': ('score_norm', {}), 'cutoff': ('score_cutoff', {}), 'diversify': ('diversify', {'checked': True}),      # (the pool's ids are the select kernel's)
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

    def _rank_of(self, srs, cs, labels, off_ex, off_in, listed):
        fn, kw = self._route('target_rank')
        rank = fn(srs, self._table(), cs, labels, off_ex, off_in, listed, **kw)
        if self.shard is not None:       # (ranks of disjoint row shards add up: the shard's answer is final)
            return rank
        rank = rank[0]                   # (one device: (rank, target))
        if listed is not None:
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
        n = self.shard.V if self.shard is not None else self._table().shape[0]
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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            return self._select_of(srs, cs, k, off_ex, off_in, listed, exclude_seen, **bias)

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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            fn, kw = self._route('select' if k <= 128 else 'select_many')
            return fn(srs, self._table(), cs, k, off_ex, off_in, listed, exclude_seen, **kw, **bias)

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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            val, ids = self._select_of(srs, cs, pool, off_ex, off_in, listed, exclude_seen, **bias)
            pval, pick, _, _ = self._diversify_of(ids, val, k, diversity)
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

    def _diversify_of(self, ids, val, k, diversity):
        """(val, pick, mmr, ild) of ops.diversify over the rows of the item table at the global ids [B, M] (-1: unfilled)"""
        fn, kw = self._route('diversify')
        return fn(self._table(), ids, val, k, diversity, **kw)

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
        n = self.shard.V if self.shard is not None else self._table().shape[0]
        if ids.numel() > 0:
            lo, hi = (int(x) for x in torch.aminmax(ids))
            if lo < -1 or hi >= n:
                raise ValueError('list_diversity: item id %d; ids are in [0, %d), or -1 for a padding slot' % (lo if lo < -1 else hi, n))
        with _Serving(self):
            ids = ids.to(self._table().device)
            return self._diversify_of(ids, torch.zeros(ids.shape, device=ids.device, dtype=torch.float32), M, 0.0)[3]

    def _scoring_args(self, *inputs, exclude_seen, raw=False):
        """(srs, cs, off_ex, off_in, listed) under which the score of ops.score_select / score_items / score_norm,
        logsumexp_c(z_c[b,v] + off_c[b]), is what forward() returns: one soft-max here, off_ex = -lse.  listed: the
        session's own items when exclude_seen drops them.  raw=True (the caller normalises over the eligible items itself):
        the full-catalogue statistics pass is skipped and off_ex is None - the score is the raw logit."""
        sr = self.session_repr(*inputs)
        st = self._state(sr.shape[0])
        cs, inv_scale = self._col_scale(st)
        off_ex = None if raw else -self._lse(sr, cs, inv_scale, st).unsqueeze(0)      # log softmax = z - lse
        listed = self._session_items(inputs[0]) if exclude_seen else None
        return [sr], cs, off_ex, None, listed

    def _served(self, *inputs, exclude_seen, renormalize, **bias):
        """_scoring_args; renormalize with something to renormalise (a bias or exclude_seen): the offsets minus Z, the
        log-normaliser over the eligible items, so that the kernels return s - Z (a session with nothing eligible: Z = -inf,
        offsets unchanged - all its slots are -inf anyway)"""
        todo = bool(renormalize) and (bool(bias) or bool(exclude_seen))
        srs, cs, off_ex, off_in, listed = self._scoring_args(*inputs, exclude_seen=exclude_seen, raw=todo)
        if todo:
            Z = self._norm_of(srs, cs, off_ex, off_in, listed, exclude_seen, **bias)
            Zs = torch.where(Z == float('-inf'), torch.zeros_like(Z), Z).unsqueeze(0)
            off_ex = -Zs if off_ex is None else off_ex - Zs
            off_in = None if off_in is None else off_in - Zs
        return srs, cs, off_ex, off_in, listed

    def _norm_of(self, srs, cs, off_ex, off_in, listed, drop_listed, **bias):
        fn, kw = self._route('norm')
        return fn(srs, self._table(), cs, off_ex, off_in, listed, drop_listed, **kw, **bias)

    def log_mass(self, *inputs, exclude_seen=False, item_bias=None, item_group=None):
        """fp32 [B]: the log of the probability mass, under forward()'s distribution, of the items a filter leaves - the
        items recommend() could return with the same keywords (not the session's own under exclude_seen, item_bias > -inf);
        with a finite bias the log-partition of the tilted distribution, log sum_v p_model(v) exp(bias_v).  0 up to round-off
        without a filter, -inf for a session with nothing eligible.  It is what renormalize=True subtracts.  One fused pass
        over the table (csrc/score_norm.hip), no (B, V) matrix, sharded table included; eval mode under torch.no_grad(),
        item_bias / item_group checked first as in recommend()."""
        bias = self._item_bias('log_mass', item_bias, item_group)
        with _Serving(self):
            srs, cs, off_ex, off_in, listed = self._scoring_args(*inputs, exclude_seen=exclude_seen)
            return self._norm_of(srs, cs, off_ex, off_in, listed, exclude_seen, **bias)

    def _lse(self, sr, cs, inv_scale, st, labels=None):
        """log-sum-exp of every session's logits over the whole catalog: the fused statistics pass (no gradient kept)"""
        B = sr.shape[0]
        if labels is None:
            labels = torch.zeros(B, dtype=torch.int64, device=sr.device)
        if self.shard is not None:
            return self.shard.stats(sr, self._table(), cs, labels, inv_scale)[0]
        return ops.score_stats(sr, self._table(), cs, labels.to(torch.int32), st['ws'][B], st['tgrad'], None, inv_scale, None)[0]

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

    def _select_of(self, srs, cs, k, off_ex, off_in, listed, drop_listed, **bias):
        """bias: `bias=` / `group=` over global ids (_item_bias), added after the mixture"""
        fn, kw = self._route('select')
        return fn(srs, self._table(), cs, k, off_ex, off_in, listed, drop_listed, **kw, **bias)

    def _cutoff_of(self, srs, cs, off_ex, off_in, listed, drop_listed, crit, **bias):
        """(floor, count, log_kept, top) of ops.score_cutoff; crit: top_k / top_p / min_p / temperature"""
        fn, kw = self._route('cutoff')
        return fn(srs, self._table(), cs, off_ex, off_in, listed, drop_listed, **crit, **kw, **bias)

    @staticmethod
    def _cutoff_args(who, top_k, top_p, min_p, temperature):
        """the criteria as _cutoff_of takes them, checked (ops.cutoff_scalars); None when none of the three is given"""
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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            return self._cutoff_of(srs, cs, off_ex, off_in, listed, exclude_seen, crit, **bias)[:3]

    def _sample_of(self, srs, cs, k, off_ex, off_in, listed, drop_listed, temperature, seed, session_keys, **bias):
        """bias: `bias=` / `group=` as in _select_of, and `floor=` when the draw is truncated"""
        fn, kw = self._route('sample')
        return fn(srs, self._table(), cs, k, off_ex, off_in, listed, drop_listed, temperature=temperature, seed=seed,
                  session_keys=session_keys, **kw, **bias)

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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
            cut = {} if crit is None else dict(floor=self._cutoff_of(srs, cs, off_ex, off_in, listed, exclude_seen, crit, **bias)[0])
            _, ids = self._sample_of(srs, cs, k, off_ex, off_in, listed, exclude_seen, temperature, seed, session_keys, **cut,
                                     **bias)
            return self._items_of(srs, cs, ids, off_ex, off_in, listed, exclude_seen, **bias), ids

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
        n = self.shard.V if self.shard is not None else self._table().shape[0]
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
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=False, **bias)
            lab = lab.to(srs[0].device).clamp(min=-1)
            if lab.numel() != srs[0].shape[0]:
                raise ValueError('served_rank: %d labels for %d sessions' % (lab.numel(), srs[0].shape[0]))
            target = self._items_of(srs, cs, lab[:, None], off_ex, off_in, listed, exclude_seen, **bias)[:, 0]
            cut = {} if crit is None else dict(floor=self._cutoff_of(srs, cs, off_ex, off_in, listed, exclude_seen, crit, **bias)[0])
            fn, kw = self._route('ahead')
            ahead = fn(srs, self._table(), cs, lab.to(torch.int32), target, off_ex, off_in, listed, exclude_seen, **kw, **cut, **bias)
            shown = target > float('-inf')
            if cut:
                shown = shown & ~(target < cut['floor'])           # (the kernels' own test of a floor)
            out = torch.where(shown, ahead, torch.full_like(ahead, -2))
            return torch.where(lab < 0, torch.full_like(ahead, -1), out)

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
        n = self.shard.V if self.shard is not None else self._table().shape[0]
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
            if lo < -1 or hi >= n:
                raise ValueError('rank_items: item id %d; ids are in [0, %d), or -1 for a padding slot' % (lo if lo < -1 else hi, n))
            if dup:
                raise ValueError('rank_items: an item id appears twice in a row of items; every id at most once per session')
        ops.cutoff_scalars('rank_items', top_k, top_p, min_p, temperature)
        crit = self._cutoff_args('rank_items', top_k, top_p, min_p, temperature)
        with _Serving(self):
            srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=False, **bias)
            B = srs[0].shape[0]
            if ids.dim() == 2 and ids.shape[0] != B:
                raise ValueError('rank_items: items for %d sessions, the batch has %d' % (ids.shape[0], B))
            ids = ids.to(srs[0].device).expand(B, M).contiguous()
            target = self._items_of(srs, cs, ids, off_ex, off_in, listed, exclude_seen, **bias)
            cut = {} if crit is None else dict(floor=self._cutoff_of(srs, cs, off_ex, off_in, listed, exclude_seen, crit, **bias)[0])
            if M == 1:
                fn, kw = self._route('ahead')
                ahead = fn(srs, self._table(), cs, ids[:, 0].to(torch.int32), target[:, 0], off_ex, off_in, listed, exclude_seen,
                           **kw, **cut, **bias)[:, None]
            else:
                fn, kw = self._route('ahead_many')
                ahead = fn(srs, self._table(), cs, ids.to(torch.int32), target, off_ex, off_in, listed, exclude_seen, **kw, **cut,
                           **bias)
            shown = target > float('-inf')
            if cut:
                shown = shown & ~(target < cut['floor'][:, None])           # (the kernels' own test of a floor)
            out = torch.where(shown, ahead, torch.full_like(ahead, -2))
            return torch.where(ids < 0, torch.full_like(ahead, -1), out)

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
        n = self.shard.V if self.shard is not None else self._table().shape[0]
        if items.numel() > 0:
            lo, hi = (int(x) for x in torch.aminmax(items.detach()))
            if lo < -1 or hi >= n:
                raise ValueError('score_items: item id %d; ids are in [0, %d), or -1 for a padding slot' % (lo if lo < -1 else hi, n))
        with _Serving(self):
            return self._score_items(*inputs, items=items, exclude_seen=exclude_seen, renormalize=renormalize, **bias)

    def _score_items(self, *inputs, items, exclude_seen, renormalize=False, **bias):
        srs, cs, off_ex, off_in, listed = self._served(*inputs, exclude_seen=exclude_seen, renormalize=renormalize, **bias)
        return self._items_of(srs, cs, items, off_ex, off_in, listed, exclude_seen, **bias)

    def _items_of(self, srs, cs, items, off_ex, off_in, listed, drop_listed, **bias):
        fn, kw = self._route('score_items')
        return fn(srs, self._table(), cs, items.to(srs[0].device), off_ex, off_in, listed, drop_listed, **kw, **bias)

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

    def _log_probs(self, sr):
        B = sr.shape[0]
        st = self._state(B)
        cs, inv_scale = self._col_scale(st)
        if self.shard is not None:           # evaluation / compat only (no gradient through the sharded (B, V) matrix)
            return self.shard.log_probs(sr, self._table(), cs, data_parallel=self.shard.eval_data_parallel)
        return ops.score_logp(sr, self._table(), cs, st['ws'][B], inv_scale)


class AttnReadout(nn.Module):
    """srgnn.py:53-91 / niser.py:51-89 (batch_norm=None there).  fc_u/fc_v run as MFMA GEMMs over all
    nodes of the batch; sigmoid / fc_e / per-session softmax / weighted sum is one wave per session."""

    def __init__(self, input_dim, hidden_dim, output_dim, batch_norm=None, feat_drop=0.0, activation=None):
        super().__init__()
        assert not batch_norm and output_dim == input_dim and activation is None
        self.feat_drop = nn.Dropout(feat_drop)
        self.fc_u = nn.Linear(input_dim, hidden_dim, bias=False)
        self.fc_v = nn.Linear(input_dim, hidden_dim, bias=True)
        self.fc_e = nn.Linear(hidden_dim, 1, bias=False)

    def forward(self, mg, feat):
        dN, dB = mg.dynp('N'), mg.dynp('B')
        feat = self.feat_drop(feat)
        U = ops.linear(feat, self.fc_u.weight, None, dN, exact=True)
        Vq = ops.linear(ops.row_gather(feat, mg.last, dB, ascending=True), self.fc_v.weight, self.fc_v.bias, dB, exact=True)
        return ops.seg_attn(U, Vq, self.fc_e.weight, feat, mg.seg, dB)


class SRGNNLayer(nn.Module):
    """Parameter container for srgnn.py:11-51 (kernel: ops.srgnn_layer, see gnn.py)."""

    def __init__(self, input_dim, output_dim, feat_drop=0.0):
        super().__init__()
        self.dropout = nn.Dropout(feat_drop)
        self.gru = nn.GRUCell(2 * input_dim, output_dim)
        self.W1 = nn.Linear(input_dim, output_dim, bias=False)
        self.W2 = nn.Linear(input_dim, output_dim, bias=False)

    def forward(self, mg, feat):
        from . import gnn
        return gnn.srgnn_layer(self, mg, feat)


class SRGNN(_ScoringMixin, nn.Module):
    graph_capable = True

    def __init__(self, num_items, embedding_dim, num_layers, feat_drop=0.0, use_gnn_output=False):
        super().__init__()
        self.embedding = nn.Embedding(num_items, embedding_dim)
        self.register_buffer('indices', torch.arange(num_items, dtype=torch.long))
        self.embedding_dim = embedding_dim
        self.num_layers = num_layers
        self.use_gnn_output = use_gnn_output
        self.layers = nn.ModuleList([SRGNNLayer(embedding_dim, embedding_dim, feat_drop) for _ in range(num_layers)])
        self.readout = AttnReadout(embedding_dim, embedding_dim, embedding_dim, feat_drop=feat_drop)
        self.feat_drop = nn.Dropout(feat_drop)
        self.fc_sr = nn.Linear(2 * embedding_dim, embedding_dim, bias=False)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.embedding_dim)
        for w in self.parameters():
            w.data.uniform_(-stdv, stdv)

    def _pre(self, feat, dyn=None):
        return feat

    def _post(self, sr, dyn=None):
        return sr

    def session_repr(self, mg, sg=None, tgrad=None):
        dN, dB = mg.dynp('N'), mg.dynp('B')
        if mg.buf.is_cuda:
            ops.check_limits(mg)
        feat = self._lookup(mg.iid, (mg.uniq_items, mg.uniq_ptr, mg.uniq_pos, mg.uniq_cptr, mg.chunk_ptr), tgrad,
                            dN, mg.dynp('U'), inv=mg.uniq_inv if mg.has('uniq_inv') else None)
        feat = self._pre(self.feat_drop(feat), dN)
        if self.use_gnn_output:
            for layer in self.layers:
                feat = layer(mg, feat)
        sr_l = ops.row_gather(feat, mg.last, dB, ascending=True)
        ro = self.readout
        if feat.is_cuda and not (self.training and ro.feat_drop.p > 0):
            # read-out + fc_sr as grouped exact-fp32 launches (ops.ReadoutHead, as in MSGIFSR).  fc_v's bias rides on the U
            # product instead: sigmoid(U + (Vq + b)) = sigmoid((U + b) + Vq), and d b = sum_n dU = sum_b dVq.  (With read-out
            # dropout the fc_v input is the DROPPED last-node row while fc_sr takes the clean one: separate ops below.)
            (s,) = ops.readout_head(feat, mg.seg, dN, dB, [(sr_l, ro.fc_u.weight, ro.fc_v.bias, ro.fc_v.weight, ro.fc_e.weight,
                                                            self.fc_sr.weight)])
            return self._post(s, dB)
        sr_g = ro(mg, feat)
        return self._post(ops.linear_cat([sr_l, sr_g], self.fc_sr.weight, None, dB, exact=True), dB)

    def forward(self, mg, sg=None):
        return self._log_probs(self.session_repr(mg))


class NISER(SRGNN):
    """niser.py:91-157: L2-normalised item / session vectors, logits scaled by `scale`."""

    def __init__(self, num_items, embedding_dim, num_layers, feat_drop=0.0, norm=True, scale=12,
                 use_gnn_output=False):
        self.norm, self.scale = norm, scale
        super().__init__(num_items, embedding_dim, num_layers, feat_drop, use_gnn_output)

    def _cosine(self):
        if self.norm:
            return (self.scale if self.scale else 1.0, 1)
        return None

    def _col_scale(self, st):
        if self.norm or not self.scale:
            return super()._col_scale(st)
        W = self._table()                 # un-normalised but scaled logits
        if st['cs'] is None or st['cs'].numel() != W.shape[0]:
            st['cs'] = torch.full((W.shape[0],), float(self.scale), device=W.device)
        return st['cs'], 0.0

    def _pre(self, feat, dyn=None):
        # niser.py:135 and :142 normalise twice; the second one divides a unit vector by its norm
        # (identity up to 1 ulp, and its Jacobian is the same projection): applied once here.
        return ops.normalize(feat, 1, dyn) if self.norm else feat

    def _post(self, sr, dyn=None):
        return ops.normalize(sr, 1, dyn, getattr(self, '_sr_ws', None)) if self.norm else sr
