"""Row-sharded (vocab-parallel) item table over the GPUs of one node - RCCL over xGMI.

Reference: none (the reference is single-device); the partitioning is the one
BASELINE.json's north star names: the item-embedding table and its use as output projection are
sharded row-wise, the small session encoder is replicated, and each rank feeds its OWN batch of B
sessions (weak scaling: global batch = world * B, one optimiser step on the mean loss of all of them).

Per step and rank r (rows [lo, hi) of the table, Adam state for those rows only):
  lookup   all-gather the (padded) item-id lists -> every rank gathers the rows it owns for every
           request (others zero) -> reduce-scatter(sum): each rank receives the rows of its own nodes.
           backward: local segmented sum to one row per distinct item -> all-gather (ids, rows) ->
           each rank adds the rows it owns into its dense shard gradient, rank by rank (deterministic).
  scoring  all-gather sr (world*B, d) and labels -> fused flash-CE forward on the local shard for ALL
           sessions -> all-gather the per-shard log-sum-exp, all-reduce the label logit -> global lse
           and loss.  backward: fused kernels with the GLOBAL lse: dE for the shard is complete
           locally; d sr partials are reduce-scattered to the owners of the sessions.
  encoder  replicated parameters: gradients all-reduced (sum of per-rank contributions to the global
           mean loss) in three flat buckets in backward completion order (sync_replicated_grads), then the same fused
           Adam everywhere.
All exchanges are small (<= a few MB): latency-bound on xGMI, so they are few and flat (one
collective per exchange, no ring of tiny messages).  The local compute goes through `local`, an
object with the HIP kernels (HipLocal); tests drive the same algebra on CPU/gloo with a plain-torch
stand-in to prove the collectives reassemble the single-device result.
"""
import os

import torch
import torch.distributed as dist

# SREC_FORCE_COLLECTIVES=1: issue the RCCL calls even on a 1-rank communicator (they are then copies) - lets the
# collective sequence and its hipGraph capture be exercised on a single-GPU box (bench.py --shard)
FORCE = bool(os.environ.get('SREC_FORCE_COLLECTIVES'))


# ------------------------------------------------------------------------------- collectives
# `group` is a torch.distributed process group (None = the default one) OR an object with `srec_loopback = True`
# (RecordingGroup / ReplayGroup below): the single-GPU rehearsal of one rank of an N-rank job.
BUCKETS = {'bytes': []}                # payload of the replicated-gradient buckets of the last step (sync_replicated_grads)
STATS = {'count': 0, 'bytes': 0}      # collectives issued through this module and their payload (bytes of the full exchanged
#                                       buffer as this rank sees it): bench.py reports them per step


def _loop(group):
    return group is not None and getattr(group, 'srec_loopback', False)


def _world(group=None):
    if _loop(group):
        return group.world
    return dist.get_world_size(group) if dist.is_initialized() else 1


def _rank(group=None):
    if _loop(group):
        return group.rank
    return dist.get_rank(group) if dist.is_initialized() else 0


def _active(group=None):
    """collectives are issued: more than one rank, or forced on a 1-rank communicator"""
    return _world(group) > 1 or (FORCE and dist.is_initialized())


def _count(nbytes):
    STATS['count'] += 1
    STATS['bytes'] += int(nbytes)


TIMING = None                         # a list: every collective issued through this module is bracketed by HIP events on the
#                                       stream it is issued from and appended as (kind, payload bytes, start, end) - eager steps
#                                       only (bench.py's `collectives.timed`: what an exchange costs on the rank's timeline,
#                                       waiting for the slowest rank included)


def _timed(kind, nbytes, fn, t):
    if TIMING is None or not t.is_cuda or torch.cuda.is_current_stream_capturing():
        return fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    TIMING.append((kind, int(nbytes), e0, e1))
    return out


def timing_summary(entries):
    """[(kind, bytes, start, end)] of whole steps -> [dict(kind, bytes, us)] (device synchronised by the caller)"""
    return [dict(kind=k, bytes=b, us=round(e0.elapsed_time(e1) * 1e3, 2)) for k, b, e0, e1 in entries]


def _host_staged(t, group):
    """gloo moves host memory: device tensors are staged through the host (the W-ranks-on-one-GPU tests; production = RCCL)"""
    return t.is_cuda and dist.get_backend(group) != 'nccl'


def all_gather_cat(t, group=None):
    """[n, ...] per rank -> [world*n, ...] (same n everywhere)"""
    if not _active(group):
        return t
    t = t.contiguous()
    nb = _world(group) * t.numel() * t.element_size()
    _count(nb)
    return _timed('all_gather', nb, lambda: group.collective('all_gather', t) if _loop(group) else all_gather_cat_pg(t, group), t)


def reduce_scatter_sum(t, group=None):
    """[world*n, ...] per rank -> [n, ...]: rank r receives the sum over ranks of block r"""
    if not _active(group):
        return t
    t = t.contiguous()
    _count(t.numel() * t.element_size())
    return _timed('reduce_scatter', t.numel() * t.element_size(),
                  lambda: group.collective('reduce_scatter', t) if _loop(group) else reduce_scatter_pg(t, group), t)


def all_reduce_(t, op=None, group=None, always=False):
    """in-place all-reduce (SUM unless `op`) through the job's backend.  always: also on a 1-rank world without FORCE"""
    if not (_active(group) or (always and (dist.is_initialized() or _loop(group)))):
        return t
    op = dist.ReduceOp.SUM if op is None else op
    _count(t.numel() * t.element_size())

    def run():
        if _loop(group):
            t.copy_(group.collective('all_reduce:' + {dist.ReduceOp.MAX: 'MAX', dist.ReduceOp.MIN: 'MIN'}.get(op, 'SUM'), t))
        elif _host_staged(t, group):
            h = t.cpu()
            dist.all_reduce(h, op=op, group=group)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=op, group=group)
        return t
    return _timed('all_reduce', t.numel() * t.element_size(), run, t)


def all_reduce_sum(t, group=None):
    return all_reduce_(t, None, group)


# ---- single-GPU rehearsal of ONE rank of an N-rank job: record what the collectives returned on that rank in a real
#      multi-process run (RecordingGroup wraps the process group), then replay that rank's step alone - eagerly or under
#      hipGraph capture - with the recorded results standing in for the other ranks (ReplayGroup).  What a rank computes
#      between two collectives depends only on its own inputs and on what the collectives handed it, so the replayed step
#      runs the very kernels, with the very operands (shard offset > 0, foreign item ids, other ranks' session vectors),
#      that the rank ran inside the job.
class RecordingGroup:
    srec_loopback = True

    def __init__(self, group=None):
        self.pg, self.world, self.rank = group, dist.get_world_size(group), dist.get_rank(group)
        self.tape = []

    def collective(self, kind, t):
        if kind == 'all_gather':
            out = all_gather_cat_pg(t, self.pg)
        elif kind == 'reduce_scatter':
            out = reduce_scatter_pg(t, self.pg)
        else:
            out = t.clone()
            h = out.cpu() if _host_staged(out, self.pg) else out
            dist.all_reduce(h, op=getattr(dist.ReduceOp, kind.split(':')[1]), group=self.pg)
            out.copy_(h)
        self.tape.append((kind, t.detach().clone().cpu(), out.detach().clone().cpu()))
        return out


class ReplayGroup:
    """answers the collectives of rank `rank` from a RecordingGroup tape (load(tape); a tape holds one step and is cycled when
    the step is run again).  Outside stream capture every call checks that the rank hands in what it handed in when the
    tape was made; under capture the recorded result is copied out of a static device tensor (a memcpy node in the graph
    where the job has its RCCL call)."""
    srec_loopback = True

    def __init__(self, world, rank, device, rtol=1e-4, atol=1e-6):
        self.world, self.rank, self.device, self.rtol, self.atol = world, rank, device, rtol, atol
        self.kinds, self.inputs, self.outputs = [], [], []
        self.pos = self.checked = 0

    def load(self, tape):
        self.kinds = [k for k, _, _ in tape]
        self.inputs = [i for _, i, _ in tape]
        self.outputs = [o.to(self.device) for _, _, o in tape]   # static device tensors: a captured copy reads them
        self.pos = self.checked = 0
        return self

    def collective(self, kind, t):
        i = self.pos % len(self.kinds)
        self.pos += 1
        assert kind == self.kinds[i], 'collective %d is %s, the recorded step issued %s' % (i, kind, self.kinds[i])
        out = self.outputs[i]
        assert t.dtype == out.dtype, (i, kind, t.dtype, out.dtype)
        if not (t.is_cuda and torch.cuda.is_current_stream_capturing()):
            a, b = t.detach().cpu(), self.inputs[i]
            assert a.shape == b.shape, (i, kind, a.shape, b.shape)
            if a.dtype.is_floating_point:
                err = (a - b).abs().max().item() if a.numel() else 0.0
                tol = max(self.atol, self.rtol * (float(b.abs().max()) if b.numel() else 0.0))
                assert torch.allclose(a, b, rtol=self.rtol, atol=tol), \
                    'collective %d (%s): this rank hands in something else than in the recorded run (max |diff| %.3e)' % (i, kind, err)
            else:
                assert torch.equal(a, b), 'collective %d (%s): integer payload differs from the recorded run' % (i, kind)
            self.checked += 1
        return out.clone()


def all_gather_cat_pg(t, pg):
    w = dist.get_world_size(pg)
    shape = (w * t.shape[0],) + tuple(t.shape[1:])
    src = t.cpu() if _host_staged(t, pg) else t
    out = torch.empty(shape, dtype=t.dtype, device=src.device)
    if dist.get_backend(pg) == 'nccl':
        dist.all_gather_into_tensor(out, src, group=pg)
    else:
        dist.all_gather(list(out.chunk(w, 0)), src, group=pg)
    return out.to(t.device)


def reduce_scatter_pg(t, pg):
    w, r = dist.get_world_size(pg), dist.get_rank(pg)
    n = t.shape[0] // w
    if dist.get_backend(pg) == 'nccl':
        out = torch.empty((n,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
        dist.reduce_scatter_tensor(out, t, op=dist.ReduceOp.SUM, group=pg)
        return out
    h = t.cpu() if t.is_cuda else t.clone()
    dist.all_reduce(h, op=dist.ReduceOp.SUM, group=pg)
    return h[r * n:(r + 1) * n].clone().to(t.device)


def lse_fold(z):
    """[W, B] -> [B]: log-sum-exp over the rows, folded in row order; a column of -inf gives -inf (never exp(-inf - -inf)).
    Elementwise torch in a fixed order: equal inputs give equal bits"""
    m = z.max(dim=0).values
    ms = torch.where(m == float('-inf'), torch.zeros_like(m), m)
    l = torch.zeros_like(m)
    for w in range(z.shape[0]):
        l = l + torch.exp(z[w] - ms)
    return torch.where(m == float('-inf'), m, ms + torch.log(l))


def shard_bounds(V, world, rank):
    per = (V + world - 1) // world
    per = (per + 63) // 64 * 64                 # whole 64-row scoring tiles per shard
    lo = min(V, rank * per)
    return lo, min(V, lo + per), per


# ------------------------------------------------------------------------------- local compute (HIP)
class HipLocal:
    """The per-rank compute of the sharded path, on the HIP kernels."""

    def __init__(self):
        from . import ops
        self.ops = ops

    def localize(self, idx_all, lo, n_loc, zero=None, zero_from=0):
        """global ids (int64 / int32, -1 padding) -> int32 rows of this shard, -1 elsewhere.  zero: a float array as long as the
        list from entry zero_from on, cleared by the same launch (int32 ids) - else by a fill"""
        from ._lib import lib, ptr, stream
        idx_all = idx_all.contiguous()
        out = torch.empty(idx_all.numel(), device=idx_all.device, dtype=torch.int32)
        if idx_all.dtype == torch.int32:
            assert zero is None or (zero.numel() == idx_all.numel() - zero_from and zero.is_contiguous())
            lib.srec_localize_idx32(ptr(idx_all), idx_all.numel(), int(lo), int(n_loc), ptr(out), ptr(zero), int(zero_from), stream())
        else:
            lib.srec_localize_idx(ptr(idx_all), idx_all.numel(), int(lo), int(n_loc), ptr(out), stream())
            if zero is not None:
                zero.zero_()
        return out

    def merge_stats(self, st, lab_all=None):
        """st [w, 2, B] gathered per-shard statistics (+ the gathered global labels, < 0 = capacity padding) ->
        (lse [B], label logit [B], mean loss over the live sessions, gw [B] = d loss / d (lse_b - lab_b))"""
        from ._lib import lib, ptr, stream
        st = st.contiguous()
        w, _, B = st.shape
        lse = torch.empty(B, device=st.device, dtype=torch.float32)
        lab = torch.empty(B, device=st.device, dtype=torch.float32)
        gw = torch.empty(B, device=st.device, dtype=torch.float32)
        loss = torch.empty((), device=st.device, dtype=torch.float32)
        fn = lib.srec_merge_stats32 if (lab_all is not None and lab_all.dtype == torch.int32) else lib.srec_merge_stats
        fn(ptr(st), w, B, ptr(lab_all), ptr(lse), ptr(lab), ptr(loss), ptr(gw), stream())
        return lse, lab, loss, gw

    def inverse_index(self, uptr, upos, U, n):
        """inv[p] = u for every position p of item u (positions listed in upos[uptr[u]:uptr[u+1]]); -1 where no item claims p"""
        from ._lib import lib, ptr, stream
        inv = torch.empty(n, device=upos.device, dtype=torch.int32)
        lib.srec_inverse_index(ptr(uptr), ptr(upos), U, n, ptr(inv), stream())
        return inv

    takes_gl = True                # stats_bwd(gl=): the upstream loss gradient as a device scalar
    fused_dropout = True           # gather_masked / segment_rows take drop = (p, seed, counter, salt): the lookup's feature
    #                                dropout rides in the last gather and in the first level of its backward (ops.EmbeddingLookup)

    def gather_masked(self, table, idx, drop=None):
        from ._lib import lib, ptr, stream
        n, d = idx.numel(), table.shape[1]
        out = torch.empty(n, d, device=table.device, dtype=torch.float32)
        if drop is not None:
            lib.srec_gather_rows_drop(ptr(table), table.stride(0), ptr(idx), ptr(out), d, n, None, d, drop[0], drop[1],
                                      drop[2], drop[3], stream())
        else:
            lib.srec_gather_rows(ptr(table), table.stride(0), ptr(idx), ptr(out), d, n, None, d, stream())
        return out

    def segment_rows(self, g, uniq, drop=None):
        """one summed row per distinct item of the local batch: [U, d].  With the (cptr, chunk_ptr) pair of the FlatBatch
        the sum runs in two balanced levels (<= 16 positions per wavefront, then the pieces of each item): a
        Zipf-popular item would otherwise serialise ~1000 row reads in one wavefront."""
        from ._lib import lib, ptr, stream
        items, uptr, upos = uniq[:3]
        U, d = items.numel(), g.shape[1]
        g = g.contiguous()
        out = torch.empty(U, d, device=g.device, dtype=torch.float32)
        if len(uniq) == 5:
            cptr, chunk_ptr = uniq[3], uniq[4]
            C = chunk_ptr.numel() - 1
            part = torch.empty(max(C, 1), d, device=g.device, dtype=torch.float32)
            ar = self.ops._arange(max(C, U) + 1, g.device)
            if drop is not None:
                lib.srec_scatter_add_sorted_drop(ptr(g), d, ptr(ar), ptr(chunk_ptr), ptr(upos), ptr(part), d, C, None, d, 0,
                                                 drop[0], drop[1], drop[2], drop[3], stream())
            else:
                lib.srec_scatter_add_sorted(ptr(g), d, ptr(ar), ptr(chunk_ptr), ptr(upos), ptr(part), d, C, None, d, 0, stream())
            lib.srec_scatter_add_sorted(ptr(part), d, ptr(ar), ptr(cptr), ptr(ar), ptr(out), d, U, None, d, 0, stream())
        else:
            ar = self.ops._arange(U + 1, g.device)
            if drop is not None:
                lib.srec_scatter_add_sorted_drop(ptr(g), d, ptr(ar), ptr(uptr), ptr(upos), ptr(out), d, U, None, d, 0,
                                                 drop[0], drop[1], drop[2], drop[3], stream())
            else:
                lib.srec_scatter_add_sorted(ptr(g), d, ptr(ar), ptr(uptr), ptr(upos), ptr(out), d, U, None, d, 0, stream())
        return out

    def add_rows(self, rows, items_local, dst, proj=None):
        """dst[items_local[u]] += rows[u] for items_local[u] >= 0 (distinct within the call).  proj = (table, radial): the
        deferred row-normalisation projection is pending on dst (ops.TableGrad) - the rows' radial parts are recorded"""
        from ._lib import lib, ptr, stream
        U, d = rows.shape
        ar = self.ops._arange(U + 1, rows.device)
        if proj is not None:
            lib.srec_scatter_add_sorted_ex(ptr(rows), d, ptr(items_local), ptr(ar), ptr(ar), ptr(dst), dst.stride(0), U, None,
                                           d, 1, 0.0, 0, None, 0, ptr(proj[0]), proj[0].stride(0), ptr(proj[1]), stream())
        else:
            lib.srec_scatter_add_sorted(ptr(rows), d, ptr(items_local), ptr(ar), ptr(ar), ptr(dst), dst.stride(0), U, None,
                                        d, 1, stream())

    def add_rows_all(self, rows_all, rel, ids, w, ucap, dst, proj=None):
        """add_rows for the lists of all w ranks in ONE launch, per item in rank order (csrc/rowops.hip add_rows_ranks_kernel);
        False when the shapes are outside the kernel's contract (the caller then loops over the ranks)"""
        from ._lib import lib, ptr, stream
        if w > 16 or ids is None or ids.dtype != torch.int32 or rel.dtype != torch.int32 or not rows_all.is_contiguous():
            return False
        d = rows_all.shape[1]
        lib.srec_add_rows_ranks(ptr(rows_all), d, ptr(rel), ptr(ids), w, ucap, ptr(dst), dst.stride(0),
                                ptr(proj[0]) if proj is not None else None, proj[0].stride(0) if proj is not None else 0,
                                ptr(proj[1]) if proj is not None else None, stream())
        return True

    def _tb(self, table, refresh):
        """bf16 operand copies of this rank's shard when set_precision('bf16') is on (refreshed once per step)"""
        ops = self.ops
        if not ops.use_bf16_scoring(table.shape[1]):
            return None
        key = (table.data_ptr(), tuple(table.shape))
        tb = self.__dict__.setdefault('_tb16', {}).get(key)
        if tb is None:
            tb = self._tb16[key] = ops.TableBF16(table)
            refresh = True
        elif refresh and self.__dict__.pop('_tb_written', None) == (key, table._version):
            refresh = False                    # FusedAdam's row pass of the previous step wrote the copy (optim.py)
        return tb.refresh(table) if refresh else tb

    def ce_fwd(self, sr, table, cs, labels_local, ws, pair=None):
        B, d = sr.shape
        dev = sr.device
        # (lse, label logit) as the two rows of ONE buffer: it is what _merge_stats all-gathers (no stack / clone launches)
        if pair is None:                           # (pair given: its label-logit row has been cleared by the caller's localize)
            pair = torch.empty(2, B, device=dev, dtype=torch.float32)
            pair[1].zero_()
        lossvec = torch.empty(B, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        self.ops._ce_fwd(sr, table, cs, labels_local, ws, None, self._tb(table, True), pair[1], pair[0], lossvec, loss)
        return pair[0], pair[1]

    def ce_bwd(self, sr, table, cs, labels_local, lse, gscale, dE, ws, cs_inv_scale, defer_tg=None):
        B, d = sr.shape
        dsr = torch.empty(B, d, device=sr.device, dtype=torch.float32)
        self.ops._ce_bwd(sr, table, cs, labels_local, lse, gscale, None, None, ws, None, self._tb(table, False), dE, dsr, 3)
        self.ops.finish_table_grad(table, cs, cs_inv_scale, dE, defer_tg)
        return dsr

    def stats_bwd(self, sr, table, cs, labels_local, lse, ga, gc, dE, ws, cs_inv_scale, accumulate, defer_tg=None, gl=None):
        """d z[b, v] = ga[b] * softmax(z_b)[v] - gc[b] * [v == label_b] through this rank's rows: dE (+)= dz^T sr,
        returns the partial d sr = dz E_local"""
        B, d = sr.shape
        dsr = torch.empty(B, d, device=sr.device, dtype=torch.float32)
        if defer_tg is not None and not accumulate:
            defer_tg.overwritten()                     # stale pending / radial of a backward no optimizer step consumed
        self.ops._ce_bwd(sr, table, cs, labels_local, lse, gl, ga, gc, ws, None, self._tb(table, False), dE, dsr,
                         3 | (4 if accumulate else 0))
        self.ops.finish_table_grad(table, cs, cs_inv_scale, dE, defer_tg)
        return dsr

    def logp_cols(self, sr, table, cs, lse):
        """this rank's columns of the (B, V) log-probabilities: z[b, v] - lse[b] for the local rows v (fp32)"""
        sr = sr.contiguous()
        return self.ops._logp_cols(sr, sr.stride(0), table, cs, lse)

    def topk(self, sr, table, cs, k):
        return self.ops.score_topk(sr, table, cs, k)

    def rank(self, srs, table, cs, labels, off_ex, off_in, listed, id_lo, target=None, target_only=False):
        """this shard's share of (rank, target) of ops.score_rank: rows [id_lo, id_lo + n) of the catalog"""
        return self.ops.score_rank(srs, table, cs, labels, off_ex, off_in, listed, id_lo, target, target_only)

    def select(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        """this shard's k best rows (values, global ids) of ops.score_select: rows [id_lo, id_lo + n) of the catalog.
        bias: `bias=` (this shard's columns) and `group=` of ops.score_select, only when there is a bias, and `floor=`
        ([B], the sessions' cutoff) only when there is one"""
        return self.ops.score_select(srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, **bias)

    def select_many(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, floor, cap, **bias):
        """this shard's k best rows (values, global ids) of ops.score_select_many, 128 < k <= 4096 included: rows
        [id_lo, id_lo + n) of the catalog at or above floor ([B]: the k-th best score over the WHOLE catalogue, cutoff()'s),
        cap = the largest of cutoff()'s counts.  bias: as in select()"""
        return self.ops.score_select_many(srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, floor=floor, cap=cap,
                                          **bias)

    def sample(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, temperature, seed, session_keys, **bias):
        """this shard's k best sampled keys (keys, global ids) of ops.score_sample: rows [id_lo, id_lo + n) of the catalog.
        session_keys: one integer per session (the noise is a function of the key, never of the row).  bias: as in select()"""
        return self.ops.score_sample(srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, temperature=temperature,
                                     seed=seed, session_keys=session_keys, **bias)

    def cutoff(self, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, crit, reduce_max, reduce_sum, **bias):
        """(floor, count, log_kept, top) of ops.score_cutoff over the WHOLE catalogue, this shard scoring rows [id_lo, id_lo + n)
        (n = 0: it only joins the reduces): reduce_max / reduce_sum combine the shards' maxima and integer partials between
        the passes.  crit: top_k / top_p / min_p / temperature.  bias: as in select()"""
        return self.ops.score_cutoff(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, reduce_max=reduce_max,
                                     reduce_sum=reduce_sum, **crit, **bias)

    def score_items(self, srs, table, cs, items, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        """this shard's share of ops.score_items: rows [id_lo, id_lo + n) of the catalog score, every other id gives 0.
        bias: as in select()"""
        return self.ops.score_items(srs, table, cs, items, off_ex, off_in, listed, drop_listed, id_lo, **bias)

    def norm(self, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        """this shard's log-normaliser of ops.score_norm: rows [id_lo, id_lo + n) of the catalog.  bias: as in select()"""
        return self.ops.score_norm(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)

    def ahead(self, srs, table, cs, labels, target, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        """this shard's count of ops.score_ahead: the eligible rows of [id_lo, id_lo + n) ahead of (labels, target).  bias: as in select()"""
        return self.ops.score_ahead(srs, table, cs, labels, target, off_ex, off_in, listed, drop_listed, id_lo, **bias)

    def ahead_many(self, srs, table, cs, items, target, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        """this shard's N of ops.score_ahead_many: per target, the eligible rows of [id_lo, id_lo + n) ahead of it that are not
        targets of the session themselves (among_targets=False: the caller adds A once).  bias: as in select()"""
        return self.ops.score_ahead_many(srs, table, cs, items, target, off_ex, off_in, listed, drop_listed, id_lo,
                                         among_targets=False, **bias)

    def diversify(self, X, row, val, k, diversity):
        """ops.diversify over rows the caller has bounded (checked): (val [B,k], pick [B,k], mmr [B,k], ild [B])"""
        return self.ops.diversify(X, row, val, k, diversity, checked=True)

    def cap_select(self, ids, val, rule, k):
        """ops.cap_select over a pool whose ids the select kernels wrote (checked): (val [B,k], pick [B,k], kept [B], scanned [B])"""
        return self.ops.cap_select(ids, val, rule, k, checked=True)

    def personal_merge(self, pool_ids, pool_val, items, base, bias, k):
        """ops.personal_merge over a pool whose ids the select kernels wrote and lists ops.personal_lists looked at (checked):
        (val [B,k], ids [B,k], src [B,k], hit [B], kept [B])"""
        return self.ops.personal_merge(pool_ids, pool_val, items, base, bias, k, checked=True)

    def calibrate(self, ids, val, category, k, weight, tcat, tw, alpha):
        """ops.calibrate over a pool whose ids the select kernel wrote and a target the caller has looked at (checked):
        (val [B,k], pick [B,k], obj [B,k], kl [B])"""
        return self.ops.calibrate(ids, val, category, k, weight, tcat, tw, alpha, checked=True)

    def workspace(self, B, V, d, device):
        return self.ops.CEWorkspace(B, V, d, device)


# ------------------------------------------------------------------------------- autograd functions
def _merge_stats(lse_r, lab_logit_r, group, local=None, lab_all=None):
    """per-shard (log-sum-exp, label logit) of every session -> global (lse, label logit, mean loss, gw): ONE all-gather of
    the [2, B] pair (the label logit is non-zero on exactly one shard, so its sum over the gathered copies is the
    all-reduce it replaces) and one merge kernel.  lab_all (optional): the gathered global labels; sessions with a
    label < 0 are the capacity padding of a rank's (partial) batch and are left out of the mean.  gw [B] =
    d loss / d (lse_b - lab_b): 1 / n_live on live sessions, 0 on padding."""
    def torch_merge(lse, lab):
        if lab_all is None:
            live = torch.ones_like(lse)
        else:
            live = (lab_all >= 0).to(lse.dtype)
        gw = live / live.sum().clamp(min=1.0)
        return lse, lab, ((lse - lab) * gw).sum(), gw
    if not _active(group):
        return torch_merge(lse_r, lab_logit_r)
    B = lse_r.numel()
    if lse_r.is_contiguous() and lab_logit_r.is_contiguous() and lab_logit_r.data_ptr() == lse_r.data_ptr() + 4 * B \
            and lse_r.dtype == torch.float32:
        pair = lse_r.as_strided((1, 2, B), (2 * B, B, 1))                      # HipLocal.ce_fwd: already adjacent rows
    else:
        pair = torch.stack([lse_r, lab_logit_r]).unsqueeze(0)
    st = all_gather_cat(pair, group)                                           # [w, 2, B]
    if local is not None and hasattr(local, 'merge_stats'):
        return local.merge_stats(st, lab_all)
    return torch_merge(torch.logsumexp(st[:, 0], dim=0).contiguous(), st[:, 1].sum(0))


def _follows(a, b):
    """b starts where a ends, in the same storage (two fields of one batch buffer): a | b is then one contiguous list"""
    return (a.dtype == b.dtype and a.dim() == 1 and b.dim() == 1 and a.is_contiguous() and b.is_contiguous() and a.device == b.device
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.storage_offset() == a.storage_offset() + a.numel())


class ShardedLookup(torch.autograd.Function):
    """rows = E[idx] with E row-sharded.  Only the DISTINCT items of a rank's batch travel: their ids are all-gathered
    (padded with -1 to a capacity that is equal on all ranks), every rank contributes the rows it owns (zeros elsewhere),
    a reduce-scatter hands each rank the rows of its own items and the positions of the batch are filled from those by a
    local gather (inv: position -> slot of its item).  The exchange volume is (distinct items) x d per rank and direction,
    not (positions) x d - ~4x less at the MSGIFSR shapes, where every click is looked up once per n-gram order."""

    @staticmethod
    def forward(ctx, shard, items_pad, inv, uniq, dE, lo, local, group, vp=None, drop=None):
        n_loc = shard.shape[0]
        # ONE integer exchange per step: the padded distinct-item list (used again by the backward) and, when the caller has
        # announced them (VocabParallel.labels_hint), the labels of the loss - a few KB each, i.e. latencies on xGMI
        ucap = items_pad.numel()
        parts = [items_pad]
        lab = vp.labels_hint if vp is not None else None
        if lab is not None:
            parts.append(lab if lab.dtype == items_pad.dtype else lab.to(items_pad.dtype))
        if len(parts) > 1 and _follows(items_pad, parts[1]):
            # the batch buffer already holds (distinct items | labels) back to back (collate._items_last): the request list is a view
            req = items_pad.as_strided((ucap + parts[1].numel(),), (1,), items_pad.storage_offset())
        elif len(parts) > 1 and vp is not None and items_pad.is_cuda and items_pad.dtype == torch.int32:
            # (ids | labels) into a request buffer by the library's multi-copy launch (no aten concatenation in the rank step)
            req = torch.empty(ucap + parts[1].numel(), device=items_pad.device, dtype=torch.int32)
            vp._copy_tasks([(items_pad.view(torch.float32), req[:ucap].view(torch.float32)),
                            (parts[1].contiguous().view(torch.float32), req[ucap:].view(torch.float32))])
        else:
            req = torch.cat(parts) if len(parts) > 1 else parts[0]
        packed = all_gather_cat(req.unsqueeze(0), group)                                      # [w, ucap (+ B)]
        w_ = packed.shape[0]
        if lab is not None and w_ > 1 and w_ <= 16 and vp is not None and packed.is_cuda and packed.dtype == torch.int32:
            # the two column blocks as contiguous lists, one multi-copy launch (two strided aten copies before)
            nb = packed.shape[1] - ucap
            both = torch.empty(w_ * (ucap + nb), device=packed.device, dtype=torch.int32)
            ctx.items_all, vp.lab_all = both[:w_ * ucap], both[w_ * ucap:]
            pf, bf = packed.view(torch.float32), both.view(torch.float32)
            vp._copy_tasks([(pf[r, :ucap], bf[r * ucap:(r + 1) * ucap]) for r in range(w_)] +
                           [(pf[r, ucap:], bf[w_ * ucap + r * nb:w_ * ucap + (r + 1) * nb]) for r in range(w_)])
        else:
            both = None
            ctx.items_all = packed[:, :ucap].reshape(-1)
            if lab is not None:
                vp.lab_all = packed[:, ucap:].reshape(-1)
        if both is not None and getattr(local, 'takes_gl', False):
            # requests and labels localised by ONE launch, which also clears the label-logit row of the scoring forward
            # (ShardedScoreCE takes both from vp.lab_pre: one small launch less in front of it)
            pair = torch.empty(2, w_ * nb, device=both.device, dtype=torch.float32)
            rel_both = local.localize(both, lo, n_loc, zero=pair[1], zero_from=w_ * ucap)
            ctx.rel, vp.lab_pre = rel_both[:w_ * ucap], (rel_both[w_ * ucap:], pair, n_loc, lo)
        else:
            ctx.rel = local.localize(ctx.items_all, lo, n_loc)     # local row of every requested item (-1: another rank's); reused by the backward
        rows_all = local.gather_masked(shard, ctx.rel)                                        # [w * ucap, d]
        mine = reduce_scatter_sum(rows_all, group)                                            # [ucap, d]: my items' rows
        ctx.drop = None
        if drop is not None and drop[0] > 0:       # feature dropout of the looked-up rows (msgifsr.py:247) fused into the gather
            seed, cnt = local.ops.rng_args(shard.device)
            ctx.drop = (float(drop[0]), seed, cnt, int(drop[1]))
            out = local.gather_masked(mine, inv, ctx.drop)                                    # [n, d]: my positions
        else:
            out = local.gather_masked(mine, inv)
        ctx.uniq, ctx.ucap, ctx.dE, ctx.lo, ctx.local, ctx.group, ctx.n_loc = uniq, ucap, dE, lo, local, group, n_loc
        ctx.vp, ctx.shard = vp, shard
        return out

    @staticmethod
    def backward(ctx, g):
        # [U, d]: one summed row per distinct item of my batch (the dropout mask re-derived while summing)
        rows = ctx.local.segment_rows(g, ctx.uniq, ctx.drop) if ctx.drop is not None else ctx.local.segment_rows(g, ctx.uniq)
        U, ucap = rows.shape[0], ctx.ucap
        if U < ucap:
            rows = torch.cat([rows, rows.new_zeros(ucap - U, rows.shape[1])])
        rows_all = all_gather_cat(rows, ctx.group)
        rel = ctx.rel
        tg = ctx.vp.tgrad if ctx.vp is not None else None
        proj = (ctx.shard, tg.radial) if (tg is not None and tg.pending is not None) else None
        if proj is not None:
            tg.radial_dirty = True
        w = _world(ctx.group)
        if w > 1 and hasattr(ctx.local, 'add_rows_all') and \
                ctx.local.add_rows_all(rows_all, rel, ctx.items_all, w, ucap, ctx.dE, proj):
            return (None,) * 10
        for r in range(w):                                   # rank by rank: distinct items within each call
            if proj is not None:
                ctx.local.add_rows(rows_all[r * ucap:(r + 1) * ucap], rel[r * ucap:(r + 1) * ucap], ctx.dE, proj)
            else:
                ctx.local.add_rows(rows_all[r * ucap:(r + 1) * ucap], rel[r * ucap:(r + 1) * ucap], ctx.dE)
        return (None,) * 10


class ShardedScoreCE(torch.autograd.Function):
    """mean CE over the GLOBAL batch (world*B sessions) against the row-sharded catalog."""

    @staticmethod
    def forward(ctx, sr, shard, cs, labels, dE, lo, ws, cs_inv_scale, local, group, lab_all=None, tgrad=None, lab_pre=None):
        n_loc = shard.shape[0]
        sr_all = all_gather_cat(sr.contiguous(), group)
        if lab_all is None:                                            # not exchanged with the lookup's request lists
            lab_all = all_gather_cat(labels if labels.dtype == torch.int32 else labels.to(torch.int64), group)
            lab_pre = None
        if lab_pre is not None and lab_pre[3] == lo and lab_pre[2] >= n_loc and lab_pre[0].numel() == sr_all.shape[0]:
            # (the lookup localised against ALL rows of the shard, capacity padding included: no label names a padding row)
            lab_loc, pair = lab_pre[:2]            # localised (and the label-logit row cleared) by the lookup's launch
            lse_r, lab_logit = local.ce_fwd(sr_all, shard, cs, lab_loc, ws, pair=pair)
        elif getattr(local, 'takes_gl', False):      # HipLocal: the label-logit row is cleared by the launch that localises the labels
            pair = torch.empty(2, sr_all.shape[0], device=sr_all.device, dtype=torch.float32)
            lab_loc = local.localize(lab_all, lo, n_loc, zero=pair[1])
            lse_r, lab_logit = local.ce_fwd(sr_all, shard, cs, lab_loc, ws, pair=pair)
        else:
            lab_loc = local.localize(lab_all, lo, n_loc)
            lse_r, lab_logit = local.ce_fwd(sr_all, shard, cs, lab_loc, ws)
        lse, lab_logit, loss, gw = _merge_stats(lse_r, lab_logit, group, local, lab_all)
        ctx.save_for_backward(sr_all, shard, cs, lab_loc, lse, gw)
        ctx.misc = (dE, ws, cs_inv_scale, local, group, tgrad)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        sr_all, shard, cs, lab_loc, lse, gw = ctx.saved_tensors
        dE, ws, cs_inv_scale, local, group, tgrad = ctx.misc
        # d z[b, v] = g_b (softmax_b[v] - [v == label_b]) with g_b = gloss / n_live on live sessions, 0 on the capacity
        # padding of a rank's partial batch (the mean runs over the live sessions of the GLOBAL batch)
        kw = {}
        if getattr(local, 'takes_gl', False):      # the HIP kernels take the upstream scalar as a pointer and multiply the
            g = gw                                 # per-session coefficients by it themselves: no scaling launch
            kw['gl'] = gloss.reshape(()).to(torch.float32)
        else:
            g = (gw * gloss.reshape(()).to(torch.float32)).contiguous()
        if tgrad is not None and tgrad.defer:
            dsr_part = local.stats_bwd(sr_all, shard, cs, lab_loc, lse, g, g, dE, ws, cs_inv_scale, False, tgrad, **kw)
        else:
            dsr_part = local.stats_bwd(sr_all, shard, cs, lab_loc, lse, g, g, dE, ws, cs_inv_scale, False, **kw)
        dsr = reduce_scatter_sum(dsr_part, group)
        return (dsr,) + (None,) * 12


class ShardedScoreStats(torch.autograd.Function):
    """(lse_b, z[b, label_b]) of this rank's sessions against the row-sharded catalog, differentiable in both outputs:
    the sharded counterpart of ops.ScoreStats, for losses that mix several soft-maxes (MSGIFSR order fusion / extra,
    msgifsr.py:281-317).  Several heads share one table: the first backward of a step overwrites dE, later ones
    accumulate (tgrad.fresh)."""

    @staticmethod
    def forward(ctx, sr, shard, cs, labels, dE, lo, ws, cs_inv_scale, local, group, tgrad):
        n_loc, n = shard.shape[0], sr.shape[0]
        sr_all = all_gather_cat(sr.contiguous(), group)
        lab_all = all_gather_cat(labels.to(torch.int64), group)
        lab_loc = local.localize(lab_all, lo, n_loc)
        lse_r, lab_logit = local.ce_fwd(sr_all, shard, cs, lab_loc, ws)
        lse, lab_logit, _, _ = _merge_stats(lse_r, lab_logit, group, local)
        r = _rank(group)
        ctx.save_for_backward(sr_all, shard, cs, lab_loc, lse)
        ctx.misc = (dE, ws, cs_inv_scale, local, group, tgrad)
        return lse[r * n:(r + 1) * n].clone(), lab_logit[r * n:(r + 1) * n].clone()

    @staticmethod
    def backward(ctx, dlse, dlab):
        sr_all, shard, cs, lab_loc, lse = ctx.saved_tensors
        dE, ws, cs_inv_scale, local, group, tgrad = ctx.misc
        ga = all_gather_cat(dlse.contiguous().float(), group)
        gc = all_gather_cat((-dlab).contiguous().float(), group)
        if tgrad.defer:
            dsr_part = local.stats_bwd(sr_all, shard, cs, lab_loc, lse, ga, gc, dE, ws, cs_inv_scale, tgrad.fresh, tgrad)
        else:
            dsr_part = local.stats_bwd(sr_all, shard, cs, lab_loc, lse, ga, gc, dE, ws, cs_inv_scale, tgrad.fresh)
        tgrad.fresh = True
        dsr = reduce_scatter_sum(dsr_part, group)
        return (dsr,) + (None,) * 10


# ------------------------------------------------------------------------------- model wiring
class VocabParallel:
    """Attach to a model (`model.shard = VocabParallel(model)`): the model's table parameter becomes this
    rank's row shard and the lookup / fused loss route through the collectives above."""

    def __init__(self, model, group=None, local=None, idx_cap=None):
        self.group = group
        self.world, self.rank = _world(group), _rank(group)
        self.local = local if local is not None else HipLocal()
        table = model._table()
        self.V, self.d = table.shape
        self.lo, self.hi, self.per = shard_bounds(self.V, self.world, self.rank)
        with torch.no_grad():
            shard = torch.zeros(self.per, self.d, device=table.device, dtype=table.dtype)
            shard[:self.hi - self.lo] = table[self.lo:self.hi]
            table.data = shard                      # parameter now holds only this rank's rows
        self.n_live = self.hi - self.lo
        model.__dict__.pop('_srec_state', None)     # rebuild the scoring state for the sharded table
        self.tgrad = model._state(1)['tgrad']
        self.dE = self.tgrad.buf
        self.idx_cap = idx_cap
        self.labels_hint = None             # set by the model before the lookup of a training step: labels ride along
        self.lab_all = None                 # ... and come back gathered for loss()
        self.eval_data_parallel = False     # evaluate(): True when every rank feeds its own equal-sized slice of a batch
        self._ws = {}
        self.model = model
        self._names = {id(p): n for n, p in model.named_parameters()} if hasattr(model, 'named_parameters') else {}
        self._bucket_early, self._bucket_zero = {}, {}
        self._side, self._side_used, self._no_sync = None, False, False
        self._arena, self._slot = [], {}
        self.early_launches = 0                # buckets whose all-reduce was issued from inside a backward pass (bucket_ready)
        # side stream for the early buckets: on by default where the collective is RCCL between real ranks (it then runs beside
        # the backward); a 1-rank / loopback rehearsal keeps one stream unless asked (graph branches cost there: DESIGN 7)
        self.side_stream = bool(self.world > 1 and not _loop(group) and dist.is_initialized()
                                and dist.get_backend(group) == 'nccl') or bool(os.environ.get('SREC_BUCKET_SIDE_STREAM'))
        model.shard = self

    def _pad(self, t, cap, fill=-1):
        out = torch.full((cap,), fill, device=t.device, dtype=t.dtype)
        out[:t.numel()] = t
        return out

    def capacity(self, n):
        """a common padded length for the distinct-item lists: `idx_cap` (capacity-padded batches: no exchange, no host
        sync, graph-capturable) or the max over ranks, rounded up (one tiny all-reduce per batch)"""
        if self.idx_cap is not None:
            assert n <= self.idx_cap
            return self.idx_cap
        t = torch.tensor([n], dtype=torch.int64, device=self.dE.device)
        if self.world > 1:
            all_reduce_(t, dist.ReduceOp.MAX, self.group)
        return (int(t.item()) + 255) // 256 * 256

    def lookup(self, table, idx, uniq, drop=None, inv=None):
        """inv: position -> slot of its item in `items` (-1: padding) when the batch carries it (FlatBatch.uniq_inv, built by
        the collate workers) - else derived from the item CSR here (two small launches)"""
        if torch.is_grad_enabled() and table.requires_grad:
            self.begin_step()                  # (a training forward: every model's first use of the sharded table is its lookup)
        items, uptr, upos = uniq[:3]
        n, U = idx.numel(), items.numel()
        ucap = self.capacity(U)
        # capacity-padded batches: the distinct-item field of the batch buffer IS the padded request list (int32, -1 in the
        # unused slots) - no conversion, no copy; exact layouts pad a copy
        items_pad = items if U == ucap else self._pad(items if items.dtype == torch.int32 else items.to(torch.int64), ucap)
        if inv is None or inv.numel() != n or inv.dtype != torch.int32:
            inv = self.local.inverse_index(uptr, upos, U, n)      # position -> slot of its item in `items`
        uq = (items, uptr[:U + 1], upos) + tuple(uniq[3:])
        self.lab_all = self.lab_pre = None
        rows = ShardedLookup.apply(table, items_pad, inv, uq, self.dE, self.lo, self.local, self.group, self, drop)
        self.labels_hint = None
        return rows

    def loss(self, sr, table, cs, labels, cs_inv_scale):
        B = sr.shape[0] * self.world
        key = B
        if key not in self._ws:
            self._ws[key] = self.local.workspace(B, table.shape[0], self.d, sr.device)
        live = table[:self.n_live] if self.n_live < table.shape[0] else table
        dE = self.dE[:self.n_live] if self.n_live < table.shape[0] else self.dE
        csl = None if cs is None else cs[:self.n_live]
        lab_all, self.lab_all = self.lab_all, None
        if lab_all is not None and lab_all.numel() != B:
            lab_all = None
        lab_pre, self.lab_pre = self.__dict__.get('lab_pre'), None
        out = ShardedScoreCE.apply(sr, live, csl, labels, dE, self.lo, self._ws[key], cs_inv_scale, self.local, self.group,
                                   lab_all, self.tgrad, lab_pre if lab_all is not None else None)
        self.tgrad.fresh = True                      # the backward of `out` overwrites every live row of dE
        return out

    def _live(self, table, cs):
        if self.n_live < table.shape[0]:
            return table[:self.n_live], self.dE[:self.n_live], (None if cs is None else cs[:self.n_live])
        return table, self.dE, cs

    def _workspace(self, B, table, device):
        if B not in self._ws:
            self._ws[B] = self.local.workspace(B, table.shape[0], self.d, device)
        return self._ws[B]

    def stats(self, sr, table, cs, labels, cs_inv_scale):
        """(lse, label logit) of this rank's sessions over the whole catalog (see ShardedScoreStats).  The caller
        clears `self.tgrad.fresh` once per step before the first head."""
        live, dE, csl = self._live(table, cs)
        ws = self._workspace(sr.shape[0] * self.world, table, sr.device)
        return ShardedScoreStats.apply(sr, live, csl, labels, dE, self.lo, ws, cs_inv_scale, self.local, self.group,
                                       self.tgrad)

    def log_probs(self, sr, table, cs, data_parallel=False):
        """(B, V) log-probabilities (the reference models' forward() output; compat / evaluation path, no gradient):
        local log-sum-exp per shard -> global lse -> each rank's columns -> all-gather of the column blocks."""
        with torch.no_grad():
            n_loc = sr.shape[0]
            sr_all = all_gather_cat(sr.contiguous(), self.group) if data_parallel else sr.contiguous()
            B = sr_all.shape[0]
            live, _, csl = self._live(table, cs)
            ws = self._workspace(B, table, sr.device)
            none = torch.full((B,), -1, dtype=torch.int32, device=sr.device)
            lse_r, _ = self.local.ce_fwd(sr_all, live, csl, none, ws)
            gathered = _active(self.group)
            lse = torch.logsumexp(all_gather_cat(lse_r.unsqueeze(0), self.group), dim=0).contiguous() if gathered else lse_r
            cols = self.local.logp_cols(sr_all, live, csl, lse)                    # [B, n_live]
            if gathered:
                pad = cols.new_full((B, self.per), float('-inf'))
                pad[:, :self.n_live] = cols
                allc = all_gather_cat(pad.t().contiguous(), self.group)            # [world*per, B]
                cols = allc[:self.V].t().contiguous()
            if data_parallel:
                cols = cols[self.rank * n_loc:(self.rank + 1) * n_loc]
            return cols

    def topk(self, sr, table, cs, k, data_parallel=False):
        """evaluation over the sharded table (SURVEY 8(e) "Eval"): every rank ranks its own rows with the fused
        top-k kernel, the (B, k) lists are all-gathered and merged (ties -> lower item id, like one device).
        data_parallel=False: every rank passes the SAME sessions (replicated evaluation loader) and gets the full
        answer.  data_parallel=True: each rank passes its own B/world sessions (same count everywhere); the session
        vectors are all-gathered first and each rank gets the answer for its own sessions."""
        n_loc = sr.shape[0]
        sr_all = all_gather_cat(sr.contiguous(), self.group) if data_parallel else sr
        live = table[:self.n_live]
        csl = None if cs is None else cs[:self.n_live]
        kk = min(k, self.n_live)
        B = sr_all.shape[0]
        if kk > 0:
            val, idx = self.local.topk(sr_all, live, csl, kk)
            idx = idx.to(torch.int64) + self.lo
        else:
            val = sr_all.new_empty(B, 0)
            idx = torch.empty(B, 0, dtype=torch.int64, device=sr.device)
        if kk < k:                                   # a shard with fewer than k live rows: pad with -inf
            val = torch.cat([val, val.new_full((B, k - kk), float('-inf'))], 1)
            idx = torch.cat([idx, idx.new_full((B, k - kk), 2 ** 62)], 1)
        if _active(self.group):
            w = self.world
            val = all_gather_cat(val, self.group).view(w, B, k).permute(1, 0, 2).reshape(B, w * k)
            idx = all_gather_cat(idx, self.group).view(w, B, k).permute(1, 0, 2).reshape(B, w * k)
        # merge: descending value, ties towards the lower item id (two stable sorts)
        o = torch.argsort(idx, dim=1, stable=True)
        val, idx = val.gather(1, o), idx.gather(1, o)
        o = torch.argsort(val, dim=1, descending=True, stable=True)[:, :k]
        val, idx = val.gather(1, o), idx.gather(1, o)
        if data_parallel:
            val, idx = val[self.rank * n_loc:(self.rank + 1) * n_loc], idx[self.rank * n_loc:(self.rank + 1) * n_loc]
        return val, idx.to(torch.int32)

    def target_rank(self, srs, table, cs, labels, off_ex=None, off_in=None, listed=None, data_parallel=False):
        """rank of every session's label over the sharded table (ops.score_rank's contract; srs: list of C [B, d] session
        vectors, off_ex / off_in [C, B], listed [B, L]).  The number of items ahead of the label is a SUM over disjoint row
        ranges: each rank scores the labels and listed items it owns (every id has one owner, the others contribute 0 ->
        sum-all-reduce of `target`), counts its own rows against that common target, and one sum-all-reduce of B integers
        finishes it - no gather of candidate lists, no merge.  data_parallel as in topk(): every rank passes its own B / world
        sessions (session vectors, labels, offsets and lists are all-gathered first) and gets its own sessions' ranks."""
        def two_passes(tab, mix, labels):
            if self.n_live > 0:
                _, target = self.local.rank(*tab, labels, *mix, self.lo, None, True)
            else:
                target = torch.zeros(labels.numel(), device=tab[0][0].device, dtype=torch.float32)
            all_reduce_sum(target, self.group)
            if self.n_live > 0:
                rank, _ = self.local.rank(*tab, labels, *mix, self.lo, target, False)
            else:
                rank = torch.where(labels < 0, -1, 0).to(torch.int32)
            if _active(self.group):
                # sessions without a label carry -1 on every rank: summed as 0, restored afterwards
                rank = all_reduce_sum(torch.where(labels < 0, torch.zeros_like(rank), rank), self.group)
            # (a fix-up correction within round-off of the target may overshoot by one: see serving.ServingMixin._label_rank)
            return torch.where(labels < 0, torch.full_like(rank, -1), rank.clamp(min=0))
        # (no neutral value: the two passes meet in a collective, so a rank without live rows runs the body as well)
        return self._serve(two_passes, srs, table, cs, off_ex, off_in, listed, data_parallel, extra=labels.to(torch.int64))

    def _serve(self, entry, srs, table, cs, off_ex, off_in, listed, data_parallel, bias=None, group=None, extra=None,
                neutral=None, combine=None):
        """The skeleton of every served call over the sharded table (target_rank, select, sample, norm, score_items; diversify
        gathers its pool's rows through it, the ids standing where the session vectors do).  This
        rank's columns of the bias (_bias_cols); under data_parallel the sessions of all ranks (_gather_sessions) and `extra`,
        one more per-session tensor [B, ...] (labels, session keys, per-session items); then
        `entry((srs, live rows, their cs), (off_ex, off_in, listed), extra, **bias keywords)` on a rank with live rows and
        `neutral(B, device)` - the value `combine` ignores - on a rank without (padding rows are never scored; neutral None:
        entry runs there too); `combine(result)` over the ranks; under data_parallel this rank's own sessions of the result
        (a tensor or a tuple of tensors).  The callers' entries splice the two tuples into HipLocal's positional order:
        (srs, table, cs, [k | items | labels], off_ex, off_in, listed, [drop_listed,] id_lo, ...)."""
        n_loc = srs[0].shape[0]
        bkw = self._bias_cols(bias, group, data_parallel)
        if data_parallel:
            srs, off_ex, off_in, listed = self._gather_sessions(srs, off_ex, off_in, listed)
            if isinstance(extra, tuple):           # (several per-session tensors; None entries stay None)
                extra = tuple(None if e is None else all_gather_cat(e.contiguous(), self.group) for e in extra)
            elif extra is not None:
                extra = all_gather_cat(extra.contiguous(), self.group)
        if neutral is None or self.n_live > 0:
            csl = None if cs is None else cs[:self.n_live]
            out = entry((srs, table[:self.n_live], csl), (off_ex, off_in, listed), extra, **bkw)
        else:
            out = neutral(srs[0].shape[0], srs[0].device)
        if combine is not None:
            out = combine(out)
        if data_parallel:
            own = slice(self.rank * n_loc, (self.rank + 1) * n_loc)
            out = tuple(t[own] for t in out) if isinstance(out, tuple) else out[own]
        return out

    def _bias_cols(self, bias, group, data_parallel):
        """the keywords the local select / score_items take for a bias over GLOBAL ids ([V] or [G, V], the same on every
        rank): this rank's columns [lo, lo + n_live) as a view (the row stride stays the full one), and the sessions' group
        ids - all-gathered with the sessions under data_parallel.  No bias: no keywords, the call is what it was."""
        if bias is None:
            return {}
        if data_parallel and group is not None:
            group = all_gather_cat(group.reshape(-1).to(torch.int32).contiguous(), self.group)
        return dict(bias=bias[..., self.lo:self.lo + self.n_live], group=group)

    def _gather_sessions(self, srs, off_ex, off_in, listed):
        """data_parallel: every rank's own B / world sessions -> the sessions of all ranks, in rank order (session vectors,
        offsets [C, B] and listed [B, L]; lists of different widths on the ranks are padded with -1 to the widest)"""
        srs = [all_gather_cat(s.contiguous(), self.group) for s in srs]
        gat = lambda o: None if o is None else all_gather_cat(o.t().contiguous(), self.group).t().contiguous()
        off_ex, off_in = gat(off_ex), gat(off_in)
        if listed is not None:
            w = torch.tensor([listed.shape[1]], dtype=torch.int64, device=listed.device)
            if _active(self.group):
                all_reduce_(w, dist.ReduceOp.MAX, self.group)
            pad = listed.new_full((listed.shape[0], int(w.item())), -1)
            pad[:, :listed.shape[1]] = listed
            listed = all_gather_cat(pad, self.group)
        return srs, off_ex, off_in, listed

    def select(self, srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False,
               bias=None, group=None, floor=None):
        """the k best items of every session over the sharded table (ops.score_select's contract; srs: list of C [B, d]
        session vectors, off_ex / off_in [C, B], listed [B, L] global ids): every rank selects among its own LIVE rows with
        its id_lo (padding rows are never scored), ONE all-gather carries the (value, id) pairs of all ranks, and the lists
        are merged by (value descending, id ascending) - the order of one device.  data_parallel as in topk().  bias ([V] or
        [G, V] over GLOBAL ids, the same on every rank) / group ([B] of this rank's sessions): ops.score_select's.  floor ([B]
        of this rank's sessions, what cutoff() returned): ops.score_select's; under data_parallel it travels with the sessions."""
        return self._serve(lambda tab, mix, fl, **b: self.local.select(*tab, k, *mix, drop_listed, self.lo, **b, **self._floor_kw(fl)),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group, extra=floor,
                           neutral=self._no_lists(k), combine=self._merge_lists)

    def select_many(self, srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False,
                    bias=None, group=None):
        """select() beyond 128 items (ops.score_select_many's contract, 1 <= k <= 4096): cutoff(top_k=k) gives every rank the
        same floor - the k-th best score over the whole catalogue - and the same counts, so the buffer size needs no
        collective of its own; every rank then collects and orders the rows at or above the floor among its own LIVE rows
        with its id_lo, and select()'s merge (ONE all-gather of the pairs) orders the ranks' lists: the single-device
        call's result, bit for bit.  A rank without live rows joins the cutoff's collectives and contributes unfilled lists.
        data_parallel: floor and count travel with the sessions (one all-gather of a [B, 2] tensor), as select()'s floor does;
        the largest count is read on the host (the one device-to-host read of ops.score_select_many)."""
        floor, count, _, _ = self.cutoff(srs, table, cs, off_ex, off_in, listed, drop_listed, data_parallel, bias, group, top_k=k)
        cut = torch.stack([floor.contiguous().view(torch.int32), count.to(torch.int32)], 1)       # [B, 2]: one tensor to gather

        def entry(tab, mix, fc, **b):
            fl, cap = fc[:, 0].contiguous().view(torch.float32), int(fc[:, 1].max()) if fc.shape[0] else 0
            if cap < 1:                                            # nothing eligible in any session
                return self._no_lists(k)(fc.shape[0], fc.device)
            return self.local.select_many(*tab, k, *mix, drop_listed, self.lo, fl, cap, **b)
        return self._serve(entry, srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group, extra=cut,
                           neutral=self._no_lists(k), combine=self._merge_lists)

    @staticmethod
    def _floor_kw(floor):
        """the keyword the local select / sample take for a floor - none at all without one, so the call is then what it was"""
        return {} if floor is None else {'floor': floor}

    @staticmethod
    def _no_lists(k):
        """the lists of a rank without live rows: k unfilled slots (-inf, -1) per session"""
        return lambda B, dev: (torch.full((B, k), float('-inf'), device=dev),
                               torch.full((B, k), -1, device=dev, dtype=torch.int32))

    def _merge_lists(self, pair):
        """the ranks' (value, id) lists [B, k] -> the k best of all of them: ONE all-gather of the pairs, then the order of one
        device (select() and sample())"""
        val, idx = pair
        if _active(self.group):
            (B, k), w = val.shape, self.world
            pair = all_gather_cat(torch.stack([val.view(torch.int32), idx], 0), self.group).view(w, 2, B, k)
            val = pair[:, 0].permute(1, 0, 2).reshape(B, w * k).view(torch.float32)
            idx = pair[:, 1].permute(1, 0, 2).reshape(B, w * k)
            # merge: descending value, ties towards the lower item id, unfilled slots (-inf, -1) last (two stable sorts)
            key = torch.where(idx < 0, torch.full_like(idx, 2 ** 31 - 1), idx)
            o = torch.argsort(key, dim=1, stable=True)
            val, idx = val.gather(1, o), idx.gather(1, o)
            o = torch.argsort(val, dim=1, descending=True, stable=True)[:, :k]
            val, idx = val.gather(1, o).contiguous(), idx.gather(1, o).contiguous()
        return val, idx

    def sample(self, srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False,
               bias=None, group=None, temperature=1.0, seed=0, session_keys=None, floor=None):
        """k distinct items per session DRAWN from softmax(score / temperature) over the eligible items of the sharded table
        (ops.score_sample's contract; the arguments of select()): every rank keeps the k best sampled keys among its own LIVE
        rows with its id_lo, ONE all-gather carries the (key, id) pairs and select()'s merge orders them.  The noise is a
        function of (seed, session key, GLOBAL id), so the result is the single-device call's, bit for bit.  session_keys:
        [B] integers of this rank's sessions; None = the row index - under data_parallel the GLOBAL row index (rank * B + b),
        and given keys are all-gathered with the sessions.  floor: as in select() - the draw is inside the kept set of cutoff()."""
        if data_parallel and session_keys is not None:
            session_keys = session_keys.reshape(-1).to(torch.int32)        # (as they travel)
        return self._serve(lambda tab, mix, kf, **b: self.local.sample(*tab, k, *mix, drop_listed, self.lo, temperature, seed,
                                                                       kf[0], **b, **self._floor_kw(kf[1])),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group, extra=(session_keys, floor),
                           neutral=self._no_lists(k), combine=self._merge_lists)

    def cutoff(self, srs, table, cs, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False, bias=None,
               group=None, top_k=None, top_p=None, min_p=None, temperature=1.0):
        """(floor fp32 [B], count int32 [B], log_kept fp32 [B], top fp32 [B]): the cutoff of truncated sampling over the eligible
        items of the sharded table (ops.score_cutoff's contract; the arguments of select()).  Every rank runs the passes over
        its own LIVE rows with its id_lo and its columns of the bias; between the passes the ranks all-reduce small tensors -
        MAX over the [B] fp32 maxima once, SUM over the int64 [B, 3, 256] histogram after each of the up to 5 passes.  The
        partials are integers, so the result is the single-device call's, bit for bit, on every rank.  A rank without live
        rows launches no pass and joins every collective with neutral partials (there is no shortcut past the collectives).
        data_parallel: the sessions are gathered ONCE, ahead of the first pass; every rank gets its own sessions' rows."""
        crit = dict(top_k=top_k, top_p=top_p, min_p=min_p, temperature=temperature)
        rmax = lambda t: all_reduce_(t, dist.ReduceOp.MAX, self.group)
        rsum = lambda t: all_reduce_sum(t, self.group)
        # (neutral None: the entry runs on a rank without live rows too - on an empty table)
        return self._serve(lambda tab, mix, _, **b: self.local.cutoff(*tab, *mix, drop_listed, self.lo, crit, rmax, rsum, **b),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group)

    def norm(self, srs, table, cs, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False, bias=None,
             group=None):
        """fp32 [B]: the log-normaliser of select()'s score over the eligible items of the sharded table (ops.score_norm's
        contract): every rank takes Z over its own LIVE rows with its id_lo and its columns of the bias (a rank without live
        rows gives -inf), ONE all-gather carries the [world, B] values, and every rank folds them in rank order with the same
        -inf-safe log-sum-exp - equal bits on every rank.  data_parallel, bias and group as in select()."""
        return self._serve(lambda tab, mix, _, **b: self.local.norm(*tab, *mix, drop_listed, self.lo, **b),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group,
                           neutral=lambda B, dev: torch.full((B,), float('-inf'), device=dev, dtype=torch.float32),
                           combine=lambda z: lse_fold(all_gather_cat(z.unsqueeze(0), self.group)) if _active(self.group) else z)

    def score_items(self, srs, table, cs, items, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False,
                    bias=None, group=None):
        """the scores of given items over the sharded table (ops.score_items' contract; srs: list of C [B, d] session
        vectors, off_ex / off_in [C, B], listed [B, L] global ids, items [B, M] or [M] global ids): every rank scores the ids
        among its own LIVE rows with its id_lo (padding rows are never owners) and gives 0 for the others, -inf for padding
        slots and dropped items - ONE sum-all-reduce of [B, M] floats finishes it.  data_parallel as in select(): every rank
        passes its own B / world sessions (and their [B / world, M] items; a 1-D list is the same on every rank) and gets its
        own sessions' scores.  bias / group as in select(): the owner of an id adds its bias, so the sum is still one device's
        (the bias holds no +inf: the model-level entry points check it)."""
        M = items.shape[-1]
        return self._serve(lambda tab, mix, its, **b: self.local.score_items(*tab, items if its is None else its, *mix,
                                                                             drop_listed, self.lo, **b),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group,
                           extra=items if items.dim() == 2 else None,      # (a 1-D list is every rank's already: not gathered)
                           # a rank without live rows owns nothing
                           neutral=lambda B, dev: torch.zeros(B, M, device=dev, dtype=torch.float32),
                           # (-inf + 0 and -inf + -inf stay -inf: no slot is ever +inf)
                           combine=lambda out: all_reduce_sum(out, self.group))

    def ahead(self, srs, table, cs, labels, target, off_ex=None, off_in=None, listed=None, drop_listed=False, data_parallel=False,
              bias=None, group=None, floor=None):
        """int32 [B]: the eligible items ahead of every session's label over the sharded table (ops.score_ahead's contract; the
        arguments of select(); labels [B] global ids, target fp32 [B] the labels' served scores - what score_items() over the
        sharded table returned at labels[:, None], the same on every rank; floor [B] or None: cutoff()'s).  The count is a SUM
        over disjoint row ranges: every rank counts among its own LIVE rows with its id_lo and its columns of the bias (a rank
        without live rows counts nothing), and ONE sum-all-reduce of B integers finishes it - the single-device result, bit for
        bit.  data_parallel as in select(): labels, target and floor travel with the sessions."""
        return self._serve(lambda tab, mix, ltf, **b: self.local.ahead(*tab, ltf[0], ltf[1], *mix, drop_listed, self.lo, **b,
                                                                       **self._floor_kw(ltf[2])),
                           srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group,
                           extra=(labels.reshape(-1).to(torch.int64), target.reshape(-1), floor),
                           neutral=lambda B, dev: torch.zeros(B, device=dev, dtype=torch.int32),
                           combine=lambda n: all_reduce_sum(n, self.group))

    def ahead_many(self, srs, table, cs, items, target, off_ex=None, off_in=None, listed=None, drop_listed=False,
                   data_parallel=False, bias=None, group=None, floor=None):
        """int32 [B, M]: where each of M given items per session stands over the sharded table (ops.score_ahead_many's contract;
        the arguments of select(); items [B, M] global ids, -1 = empty; target fp32 [B, M] their served scores - what
        score_items() over the sharded table returned at `items`, the same on every rank; floor [B] or None: cutoff()'s).  N is
        a SUM over disjoint row ranges: every rank counts among its own LIVE rows with its id_lo and its columns of the bias,
        leaving the targets' own rows out (a rank without live rows counts nothing), and ONE sum-all-reduce of [B, M] integers
        follows; A - the targets among themselves - needs no table and is added once, from the values every rank holds alike
        (ops.ahead_among_targets): the single-device result, bit for bit.  data_parallel as in select(): items, target and
        floor travel with the sessions."""
        from .score import ahead_among_targets
        M = items.shape[-1]
        items, target = items.reshape(-1, M).to(torch.int64), target.reshape(-1, M)
        n = self._serve(lambda tab, mix, itf, **b: self.local.ahead_many(*tab, itf[0], itf[1], *mix, drop_listed, self.lo, **b,
                                                                         **self._floor_kw(itf[2])),
                        srs, table, cs, off_ex, off_in, listed, data_parallel, bias, group, extra=(items, target, floor),
                        neutral=lambda B, dev: torch.zeros(B, M, device=dev, dtype=torch.int32),
                        combine=lambda c: all_reduce_sum(c, self.group))
        # (under data_parallel n is this rank's own sessions again, as items, target and floor are)
        return n + ahead_among_targets(items, target, floor).to(device=n.device, dtype=n.dtype)

    def diversify(self, table, ids, val, k, diversity, data_parallel=False):
        """the greedy MMR re-rank of ops.diversify over the sharded table (val [B,k], pick [B,k], mmr [B,k], ild [B]): ids
        [B, M] GLOBAL item ids of every session's pool (-1 = unfilled), val [B, M] their values - what select() returned, the
        same on every rank (data_parallel: this rank's own sessions, as select() returned them).  A cosine needs both rows, and
        they may live on different shards: every rank writes the rows it owns among the pool's ids into a zeroed [B, M, d]
        buffer (the owner rule of score_items: an id in [lo, lo + n_live); padding rows are never owners, an unfilled slot has
        none), ONE sum-all-reduce completes it - x + 0 is exact, so the rows are one device's rows - and the kernel runs on
        the buffer with row = arange, on every rank or, under data_parallel, on the rank's own sessions: the result is the
        single-device call's, bit for bit.  The exchange is B * M * d * 4 bytes per call (B: the sessions of all ranks;
        8 MB at B 64, M 128, d 256) - the price of cosines across shards; through _serve, which gathers the ids of all ranks'
        sessions under data_parallel and hands back this rank's slice of the buffer."""
        M, d = ids.shape[1], self.d

        def owned(tab, _mix, _extra):
            (all_ids,), live = tab[0], tab[1]
            loc = all_ids.to(torch.int64) - self.lo
            own = (loc >= 0) & (loc < self.n_live)
            rows = live.detach().index_select(0, loc.clamp(0, self.n_live - 1).reshape(-1)).view(all_ids.shape[0], M, d)
            return torch.where(own.unsqueeze(-1), rows, torch.zeros((), device=rows.device, dtype=rows.dtype))
        # (the ids stand where the session vectors of the other routes do: _serve gathers them with the sessions)
        buf = self._serve(owned, [ids.contiguous()], table, None, None, None, None, data_parallel,
                          neutral=lambda B, dev: torch.zeros(B, M, d, device=dev, dtype=torch.float32),
                          combine=lambda rows: all_reduce_sum(rows.contiguous(), self.group))
        B = ids.shape[0]
        row = torch.arange(B * M, device=ids.device, dtype=torch.int32).view(B, M)
        row = torch.where(ids < 0, torch.full_like(row, -1), row)
        return self.local.diversify(buf.reshape(B * M, d), row, val, k, diversity)

    def cap_select(self, ids, val, rule, k, data_parallel=False):
        """the per-category caps of ops.cap_select over the sharded table (val [B,k], pick [B,k], kept [B], scanned [B]): ids
        [B, P] GLOBAL item ids of every session's ordered pool (-1 = unfilled), val [B, P] their values - what select() /
        select_many() returned, the same on every rank (data_parallel: this rank's own sessions, as they returned them).  The
        rule is over global ids and replicated, and the caps look at nothing but the pool: no row of the table is read, so
        there is NO collective - every rank runs the kernel on the pool it holds and gets the single-device call's result,
        bit for bit."""
        return self.local.cap_select(ids, val, rule, k)

    cap = cap_select        # (the name of the served call: ServingMixin._ROUTES)

    def calibrate(self, ids, val, category, k, weight, tcat, tw, alpha, data_parallel=False):
        """the calibrated re-rank of ops.calibrate over the sharded table (val [B,k], pick [B,k], obj [B,k], kl [B]): ids [B, M]
        GLOBAL item ids of every session's pool (-1 = unfilled), val [B, M] their values - what select() returned, the same on
        every rank (data_parallel: this rank's own sessions, as they returned them) - and tcat / tw [B, T] the sessions' target
        pairs (None: no target).  The category vector is over global ids and replicated, as the cap rule is, and the re-rank
        looks at nothing but the pool and the target: no row of the table is read, so there is NO collective - every rank
        runs the kernel on the pool it holds and gets the single-device call's result, bit for bit."""
        return self.local.calibrate(ids, val, category, k, weight, tcat, tw, alpha)

    def personal_merge(self, pool_ids, pool_val, items, base, bias, k, data_parallel=False):
        """the per-session list merge of ops.personal_merge over the sharded table (val [B,k], ids [B,k], src [B,k], hit [B],
        kept [B]): pool_ids / pool_val [B, P] every session's ordered pool - what select() / select_many() returned - items
        [B, M] its list, base [B, M] what score_items() over the sharded table returned for it and bias [B, M] or None; the same
        on every rank (data_parallel: this rank's own sessions, as those calls returned them).  The merge compares global ids
        and values it is handed: no row of the table is read, so there is NO collective - every rank runs the kernel on what
        it holds and gets the single-device call's result for those operands, bit for bit."""
        return self.local.personal_merge(pool_ids, pool_val, items, base, bias, k)

    personal = personal_merge   # (the name of the served call: ServingMixin._ROUTES)

    def any_session(self, flag, data_parallel=False):
        """host bool, the SAME on every rank: is `flag` (bool [B], one entry per session) set for any session of the call?
        A caller that branches on it between two sharded calls (recommend_capped: whether the batch goes to the larger pool,
        whose selection is a chain of collectives) must branch alike on every rank.  Replicated sessions: every rank holds
        the same flags, no collective.  data_parallel: the flags are the rank's own sessions', so ONE max-all-reduce of one
        integer makes the ranks agree before the device-to-host read."""
        any_ = flag.any().to(torch.int32).reshape(1)
        if data_parallel and _active(self.group):
            all_reduce_(any_, dist.ReduceOp.MAX, self.group)
        return bool(any_.item())

    # ---- replicated-parameter gradients: bucketed all-reduce, launched in backward order ----------------------------------
    N_BUCKETS = 3

    def _bucket_index(self, p, order):
        """bucket of a replicated parameter: the model's own grouping by backward completion (model.grad_bucket(name): 0 = the
        gradients that are complete first), else thirds of the parameter list from its end (the last layers' gradients come
        first) - a function of the parameter list only, identical on every rank"""
        fn = getattr(self.model, 'grad_bucket', None)
        if fn is not None:
            return max(0, min(self.N_BUCKETS - 1, int(fn(self._names.get(id(p), '')))))
        i, n = order
        return min(self.N_BUCKETS - 1, (n - 1 - i) * self.N_BUCKETS // max(n, 1))

    def _arena_setup(self, parts, n_flags):
        """one flat fp32 ARENA per bucket, laid out in parameter order; the last one ends in the flag tail.  Every bucketed
        parameter gets its slot (`p._srec_gslot`): the backward nodes that allocate a gradient write it straight into the
        slot (ops.grad_buf), the all-reduce runs in place on the arena, the optimizer reads views of it - no concatenation
        pass, no copy back (round 5: four torch.cat kernels, 23 us of the rank step)."""
        for p in getattr(self, '_bucket_live', ()):
            p.__dict__.pop('_srec_gslot', None)
        self._arena, self._slot = [], {}
        last = len(parts) - 1
        for k, bp in enumerate(parts):
            n = sum((int(p.numel()) + 3) // 4 * 4 for p in bp) + (n_flags if k == last else 0)
            dev = bp[0].device if bp else self.dE.device
            buf = torch.zeros(n, device=dev, dtype=torch.float32) if n else None
            off = 0
            for p in bp:
                assert p.dtype == torch.float32, 'replicated parameters are fp32'
                self._slot[id(p)] = (k, off, int(p.numel()))
                p._srec_gslot = [buf, off, -1]
                off += (int(p.numel()) + 3) // 4 * 4       # slots start on 16-byte boundaries (the kernels' float4 accesses)
            self._arena.append(buf)

    def release_slots(self):
        """detach the parameters from the arenas (the model goes on without this VocabParallel)"""
        for p in getattr(self, '_bucket_live', ()):
            p.__dict__.pop('_srec_gslot', None)

    def _zero_of(self, p):
        z = self._bucket_zero.get(id(p))
        if z is None:
            z = self._bucket_zero[id(p)] = torch.zeros(p.numel(), device=p.device, dtype=torch.float32)
        return z

    @staticmethod
    def _copy_tasks(tasks):
        """[(src flat, dst flat)]: ONE launch for all of them on the GPU (the multi-slab sum with one slab per task)"""
        if not tasks:
            return
        if tasks[0][1].is_cuda:
            from . import ops
            # (16-byte column threads where sizes and addresses allow, the scalar row-lane form otherwise)
            odd = lambda a, b: bool(a.numel() & 3 or (a.data_ptr() | b.data_ptr()) & 15)
            ops._launch_slab_sums([(src.reshape(1, -1), dst, odd(src, dst)) for src, dst in tasks])
        else:
            for src, dst in tasks:
                dst.copy_(src)

    def _bucket_fill(self, k, bp, tail=None):
        """make arena k hold this rank's contribution: gradients already written into their slots stay, the others are copied
        in (a gradient autograd summed from two nodes, a slot taken twice, an aten-made gradient), parameters without a
        gradient on this rank contribute zeros; `tail` = the flag tail of the last bucket.  One copy launch for all of it."""
        buf = self._arena[k]
        tasks = []
        esz = 4
        for p in bp:
            _, off, n = self._slot[id(p)]
            dst = buf[off:off + n]
            g = p.grad
            if g is None:
                tasks.append((self._zero_of(p), dst))
            elif g.data_ptr() != buf.data_ptr() + off * esz or not g.is_contiguous():
                tasks.append((g.contiguous().reshape(-1), dst))
        if tail is not None:
            tasks.append((tail, buf[buf.numel() - tail.numel():]))
        self._copy_tasks(tasks)
        self.copy_tasks_last = getattr(self, 'copy_tasks_last', {})
        self.copy_tasks_last[k] = len(tasks)
        return buf

    def _bucket_reduce(self, k, bp, side, tail=None):
        """fill arena k (see _bucket_fill) and all-reduce it IN PLACE - on the side stream when `side` (the collective then runs
        beside whatever the compute stream does next; sync_replicated_grads joins before the optimizer)"""
        if side:
            cur = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self._arena[k].device)
            self._side.wait_stream(cur)                # the gradients are complete; the buffer's last reader (Adam) is behind us
            with torch.cuda.stream(self._side):
                flat = self._bucket_fill(k, bp, tail)
                all_reduce_(flat, None, self.group)
            self._side_used = True
        else:
            flat = self._bucket_fill(k, bp, tail)
            all_reduce_(flat, None, self.group)
        return flat

    def begin_step(self):
        """called at the head of every training forward (lookup): a new hand-out round of the arena slots, and the state of a
        step that never reached sync_replicated_grads is dealt with - an aborted backward / a refused capture (no gradients
        held any more: forget its early launches) or, loudly, a second backward on top of all-reduced gradients."""
        from . import ops
        ops.grad_epoch()
        if self._bucket_early or self._side_used:
            held = any(p.grad is not None for p in getattr(self, '_bucket_live', ()))
            if held and not self._no_sync:
                raise RuntimeError('a backward pass launched the all-reduce of its gradient buckets and no '
                                   'sync_replicated_grads() / optimizer step followed: the gradients held are partly summed '
                                   'over the ranks.  Accumulating micro-batches: run all but the last under `with '
                                   'shard.no_sync():`, or zero_grad() first.')
            if self._side_used and self._side is not None and not torch.cuda.is_current_stream_capturing():
                torch.cuda.current_stream().wait_stream(self._side)
            self._bucket_early, self._side_used = {}, False

    def abort_step(self):
        """a capture of the step was refused / a step was abandoned: nothing of it ran or will be used - forget its early
        bucket launches (GraphedTrainStep's failure path; the eager fallback starts from a clean slate)"""
        self._bucket_early, self._side_used = {}, False

    def no_sync(self):
        """context for gradient accumulation (like DDP's): backward passes inside it launch no bucket all-reduce; the LAST
        micro-batch runs outside it and sync_replicated_grads() then exchanges the accumulated sums once."""
        vp = self

        class _NoSync:
            def __enter__(self_):
                self_.prev, vp._no_sync = vp._no_sync, True

            def __exit__(self_, *exc):
                vp._no_sync = self_.prev
                return False
        return _NoSync()

    def bucket_ready(self, k):
        """called from inside the backward pass (ops.grad_mark placed by the model) when every gradient of bucket k has been
        accumulated: its all-reduce is issued NOW, under the rest of the backward, instead of after it.  Never for the last
        bucket (it carries the presence flags).  The decision depends on rank-AGREED state only (the bucket partition fixed by
        agree(), the marker the model places in every training forward): every rank issues the same collectives in the same
        order; a parameter without a gradient on this rank contributes zeros."""
        parts = getattr(self, '_bucket_parts', None)
        if not _active(self.group) or parts is None or self._no_sync or not (0 <= k < len(parts) - 1) \
                or k in self._bucket_early or not parts[k]:
            return
        self.ops_flush()                               # waiting weight-gradient products, then the deferred slab sums of the layers behind us: their gradients are written
        self._bucket_early[k] = self._bucket_reduce(k, parts[k], self.side_stream)
        self.early_launches += 1

    def ops_flush(self):
        from . import ops
        ops.flush_deferred()                           # (the mid-backward flush: the step-scalar rider stays, stepq.StepQueue)

    def sync_replicated_grads(self, params, optimizer=None):
        """sum the replicated-parameter gradients over ranks in N_BUCKETS flat buckets whose layout is the same on every
        rank, in the order the backward pass completes them (bucket 0 first).  A bucket whose gradients were all complete
        when the backward passed the model's marker (bucket_ready) is already on its way - on a side stream when
        `side_stream` - ; the rest, always including the last one, are issued here, and the compute stream waits for the
        side stream before the optimizer reads the result.
        `params` is the model's replicated parameter list (same order everywhere).  Which of them carry a gradient can
        differ between ranks and between steps (MSHGNN only instantiates the GAT modules of relations with live edges in
        THIS rank's batch).  The buckets hold the parameters that had a gradient on ANY rank when the layout was agreed
        on (first call: all-reduce(MAX) of a presence mask, outside any graph capture), a rank without a gradient for one
        contributing zeros; the LAST bucket ends in a tail of flags that rides in its all-reduce: one presence count per
        bucketed parameter and one count of ranks holding a gradient for a parameter OUTSIDE the layout.  Eager steps
        read the tail back (one host sync): a parameter nobody had a gradient for this step is skipped like on one
        device (no weight decay on a zero gradient), and a late parameter makes every rank re-agree on the layout and
        repeat the exchange - the same decision everywhere, because it is taken on all-reduced values.  A captured
        step replays the layout and the skip pattern of its capture.  With `optimizer` (FusedAdam) the reduced buckets are
        handed over as the gradient source (views), so nothing is copied back per parameter."""
        if not _active(self.group):
            return
        if self._no_sync:
            raise RuntimeError('sync_replicated_grads() inside no_sync(): run the last micro-batch outside the context')
        params = list(params)
        key = tuple(id(p) for p in params)
        capturing = bool(params) and params[0].is_cuda and torch.cuda.is_current_stream_capturing()
        dev = params[0].device if params else self.dE.device

        def agree():
            if capturing:
                raise RuntimeError('the gradient bucket layout must be agreed on by an eager step before graph capture')
            present = torch.tensor([1.0 if p.grad is not None else 0.0 for p in params], device=dev)
            if self.world > 1:
                all_reduce_(present, dist.ReduceOp.MAX, self.group)
            old = getattr(self, '_bucket_ids', set()) if getattr(self, '_bucket_key', None) == key else set()
            live = [p for p, f in zip(params, present.tolist()) if f > 0 or id(p) in old]
            n = len(params)
            idx = {id(p): i for i, p in enumerate(params)}
            parts = [[] for _ in range(self.N_BUCKETS)]
            for p in live:
                parts[self._bucket_index(p, (idx[id(p)], n))].append(p)
            self._arena_setup(parts, len(live) + 1)        # (detaches the old layout's parameters from their slots first)
            self._bucket_live = live
            self._bucket_ids = {id(p) for p in live}
            self._bucket_key = key
            self._bucket_zero = {}
            self._bucket_flags = None
            self._bucket_parts = parts
            self._bucket_early = {}                        # (early results were laid out for the old partition)
            self._bucket_seen = None
            return old
        if getattr(self, '_bucket_key', None) != key:
            agree()
        ps, parts, arenas, slots = self._bucket_live, self._bucket_parts, self._arena, self._slot
        n_late = sum(1 for p in params if p.grad is not None and id(p) not in self._bucket_ids)
        if n_late and capturing:
            raise RuntimeError('%d replicated parameters carry a gradient that the captured bucket layout has no room for' % n_late)
        pat = tuple(p.grad is not None for p in ps) + (n_late,)
        fl = self._bucket_flags
        if fl is None or fl[0] != pat:                     # the tail changes only when this rank's presence pattern does
            if capturing and fl is not None:
                raise RuntimeError('gradient presence pattern changed between the warm-up and the capture')
            fl = self._bucket_flags = (pat, torch.tensor([1.0 if f else 0.0 for f in pat[:-1]] + [float(n_late)],
                                                        device=dev, dtype=torch.float32))
        flats = []
        last = len(parts) - 1
        for k, bp in enumerate(parts):
            if k in self._bucket_early:
                flats.append(self._bucket_early[k])
                continue
            # the flag tail is read by eager steps only: a captured step replays the skip pattern of its capture (the tail's
            # slots still travel - every rank all-reduces the same length - but nobody refreshes or reads them)
            tail = fl[1] if (k == last and not capturing) else None
            # (under capture also the late buckets leave on the side stream: the table's Adam pass runs beside them)
            flats.append(self._bucket_reduce(k, bp, self.side_stream and capturing, tail) if arenas[k] is not None else None)
        self._bucket_early = {}
        if self._side_used:
            # join: the early buckets become visible to the compute stream.  FusedAdam takes the join over and places it
            # behind its row pass over the table, which needs none of these gradients (optim.FusedAdam.grad_join) - unless
            # this (eager) step is about to read the flag tail back, which synchronises anyway
            self._side_used = False
            if capturing and optimizer is not None and hasattr(optimizer, '_join_grads'):
                side = self._side
                optimizer.grad_join = lambda: torch.cuda.current_stream().wait_stream(side)
            else:
                torch.cuda.current_stream().wait_stream(self._side)
        BUCKETS['bytes'] = [0 if f is None else int(f.numel()) * 4 for f in flats]
        nfl = len(ps) + 1
        pos = {id(p): i for i, p in enumerate(ps)}
        extra = {}
        if not capturing:
            seen = flats[last][-nfl:].tolist()
            self._bucket_seen = seen
            if seen[-1] > 0:
                # somebody holds a gradient the layout has no slot for - everybody sees the same count.  The buckets above are
                # exchanged and stay as they are (the all-reduce ran in place: the local values are gone); the ranks agree on a
                # layout with room for the newcomers (from the next step on) and exchange THEIR gradients in one more
                # all-reduce now - nothing dropped, no rank raises alone
                old_ids = agree()
                late = [p for p in self._bucket_live if id(p) not in old_ids]
                pieces = [(p.grad.reshape(-1).to(torch.float32) if p.grad is not None else self._zero_of(p)) for p in late]
                pieces.append(torch.tensor([1.0 if p.grad is not None else 0.0 for p in late], device=dev))
                buf = torch.cat(pieces)
                all_reduce_(buf, None, self.group)
                seen_late = buf[-len(late):].tolist()
                off = 0
                for p, f in zip(late, seen_late):
                    if f > 0:
                        extra[id(p)] = buf[off:off + p.numel()].view_as(p)
                    off += p.numel()
        else:
            seen = getattr(self, '_bucket_seen', None)
        views = dict(extra)
        for p in ps:
            k, off, n = slots[id(p)]
            if seen is None or seen[pos[id(p)]] > 0:       # nobody had a gradient this step: skipped, as on one device
                views[id(p)] = arenas[k][off:off + n].view_as(p)
        if optimizer is not None and hasattr(optimizer, 'grad_override'):
            optimizer.grad_override = views
        else:
            for p in params:
                v = views.get(id(p))
                if v is None:
                    continue
                if p.grad is None:
                    p.grad = v.clone()
                elif p.grad.data_ptr() != v.data_ptr():
                    p.grad.copy_(v)
