"""Full-catalog scoring (csrc/score_ce*.hip, rank.hip, recommend.hip, select_many.hip, score_items.hip, ensemble.hip): the fused CE / statistics
nodes, top-K, target rank, top-N select (and beyond 128 items), the scores of given items, the multi-table select / count of ensembles and the (B, V) log-probabilities, with the workspaces and argument conventions they share.
ops.py keeps the GEMM wrappers and the tests' switches (reached through the module object at call time) and re-exports this."""
import ctypes as _ct
import numbers
from collections import namedtuple

import torch

from . import ops                    # (ops.py imports this module at its end: import the package or ops first, never score alone)
from ._lib import CONST, ENS_CONST, ENS_STRUCTS, STRUCTS, lib, ptr, stream
from .ops import _ld, _rows, gemm_nn, gemm_tn


def _bf16_dim_ok(d):
    return d <= 256 and d % 4 == 0


class CEWorkspace:
    """Reusable scratch of the fused scoring/CE kernels for one (B, V, d) (sized for the fp32 and bf16 plans).

    sr16 (bf16 scoring only) is the bf16 operand copy of the session vectors the kernels read.  Two parties write it:
      * the normalisation that PRODUCES the session vectors (ops.Normalize, ops.ReadoutHeadFused), in its own launch; it
        then calls sr16_written(ws, y, n, d), which records sr_fresh = (data_ptr, rows, columns) of what it wrote;
      * _prepare_sr, one conversion launch, which records sr_key = (data_ptr, version, shape) of what it converted.
    _ce_fwd asks sr16_claim(ws, sr): when sr is exactly the tensor announced in sr_fresh it skips _prepare_sr and only
    sets sr_key; otherwise it drops sr_key and converts.  Either way the claim clears sr_fresh, so an announcement serves
    one forward.  _ce_bwd calls _prepare_sr, which is free while sr_key still names its sr (the backward of the head whose
    forward ran last) and converts again when another forward has taken the buffer since."""

    def __init__(self, B, V, d, device):
        nt, nr, dp = _ct.c_int(), _ct.c_int(), _ct.c_int()
        lib.srec_ce_plan(B, V, d, _ct.addressof(nt), _ct.addressof(nr))
        nrange, nstat = nr.value, nt.value
        if _bf16_dim_ok(d):
            lib.srec_ce_plan_bf16(B, V, d, _ct.addressof(nt), _ct.addressof(nr), _ct.addressof(dp))
            nrange, nstat = max(nrange, nr.value), max(nstat, nt.value)
        self.B, self.V, self.d = B, V, d
        self.stats = torch.empty(2 * nstat * B, device=device, dtype=torch.float32)
        self.dsr_part = torch.empty(nrange * B * d, device=device, dtype=torch.float32)
        self.lab_logit = torch.zeros(B, device=device, dtype=torch.float32)
        # bf16 operand copies of the session vectors (row-major + transposed), zero padded to 128 rows / d_pad columns
        self.Bp = (B + 127) // 128 * 128
        self.sr16 = self.srT16 = None
        self.sr_key = self.sr_fresh = None
        self._de = {}
        if _bf16_dim_ok(d):
            self.sr16 = torch.zeros(self.Bp, dp.value, device=device, dtype=torch.bfloat16)

    def de_slabs(self, B, V, d):
        """(split, workspace) of the session-split scoring backward at this shape (allocated by an eager step: a captured step
        finds it in the cache)"""
        ent = self._de.get((B, V))
        if ent is None:
            sp = _ct.c_int(1)
            lib.srec_ce_de_split(B, V, d, _ct.addressof(sp))
            split = int(sp.value)
            if split > 1 and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('the scoring workspace must be sized by an eager warm-up step before graph capture')
            buf = torch.empty(split * V * d, device=self.stats.device, dtype=torch.float32) if split > 1 else None
            ent = self._de[(B, V)] = (split, buf)
        return ent


def sr16_written(ws, y, n, d):
    """the launch that produced the session vectors y [n, d] also wrote their bf16 copy into ws.sr16 (see CEWorkspace)"""
    ws.sr_fresh = (y.data_ptr(), n, d)


def sr16_claim(ws, sr):
    """True when ws.sr16 was announced (sr16_written) as the copy of exactly sr; the announcement is spent either way"""
    fresh = getattr(ws, 'sr_fresh', None) == (sr.data_ptr(), sr.shape[0], sr.shape[1])
    ws.sr_fresh = None
    return fresh


class TableBF16:
    """bf16 copy of the item table for the bf16 scoring kernels: E16 [Vp, d_pad] (row-major only: the backward takes its
    transposed fragments with transposing LDS reads), refreshed once per step (one pass over the table)."""

    def __init__(self, table):
        V, d = table.shape
        nt, nr, dp = _ct.c_int(), _ct.c_int(), _ct.c_int()
        lib.srec_ce_plan_bf16(1, V, d, _ct.addressof(nt), _ct.addressof(nr), _ct.addressof(dp))
        self.Vp = (V + 127) // 128 * 128
        self.E16 = torch.zeros(self.Vp, dp.value, device=table.device, dtype=torch.bfloat16)

    def refresh(self, table, max_norm=0.0):
        """one streaming pass: bf16 copy of every row; max_norm > 0: Embedding(max_norm)'s in-place renorm of the fp32 rows
        in the same pass (msgifsr.py:162 / lessr.py:126)"""
        V, d = table.shape
        if d <= 1024:
            with torch.no_grad():
                lib.srec_renorm_rows_bf16(ptr(table), table.stride(0), V, d, float(max_norm), ptr(self.E16), self.E16.shape[1],
                                          stream())
        else:
            assert max_norm <= 0
            lib.srec_bf16_prepare(ptr(table), table.stride(0), V, None, d, ptr(self.E16), None, self.Vp, stream())
        return self


def use_bf16_scoring(d):
    return ops.PRECISION['matmul'] == 'bf16' and _bf16_dim_ok(d)


def _prepare_sr(sr, ws, dynB):
    """bf16 copies of the session vectors; skipped when the workspace still holds exactly this tensor (the backward
    of the head whose forward ran last)."""
    key = (sr.data_ptr(), sr._version, tuple(sr.shape))
    if ws.sr_key != key:
        B, d = sr.shape
        lib.srec_bf16_prepare(ptr(sr), _ld(sr), B, ptr(dynB), d, ptr(ws.sr16), None, ws.Bp, stream())
        ws.sr_key = key


def _ce_fwd(sr, table, cs, labels, ws, dynB, tb, lab, lse, lossvec, loss):
    B, d = sr.shape
    V = table.shape[0]
    if tb is not None:
        if sr16_claim(ws, sr):
            ws.sr_key = (sr.data_ptr(), sr._version, tuple(sr.shape))     # written by the normalisation that produced sr
        else:
            ws.sr_key = None
            _prepare_sr(sr, ws, dynB)
        lib.srec_score_ce_fwd_bf16(ptr(ws.sr16), ws.Bp, ptr(tb.E16), tb.Vp, ptr(cs), ptr(labels), B, V, d, ptr(dynB),
                                   ptr(ws.stats), ptr(lab), ptr(lse), ptr(lossvec), ptr(loss), stream())
    else:
        lib.srec_score_ce_fwd(ptr(sr), _ld(sr), ptr(table), table.stride(0), ptr(cs), ptr(labels), B, V, d, ptr(dynB),
                              ptr(ws.stats), ptr(lab), ptr(lse), ptr(lossvec), ptr(loss), stream())


def _ce_bwd(sr, table, cs, labels, lse, gl, ga, gc, ws, dynB, tb, dE, dsr, parts):
    B, d = sr.shape
    V = table.shape[0]
    if tb is not None:
        _prepare_sr(sr, ws, dynB)
        # many sessions against few table rows (a rank's shard scored for the sessions of ALL ranks): the item tiles of the
        # backward are split over the sessions, slabs in a workspace the split decides the size of (srec_ce_de_split)
        split, slabs = ws.de_slabs(B, V, d) if (parts & 1) and dE.stride(0) == d else (1, None)
        lib.srec_score_ce_bwd_bf16(ptr(ws.sr16), ptr(slabs), ws.Bp, ptr(tb.E16), None, tb.Vp, ptr(cs),
                                   ptr(labels), ptr(lse), ptr(gl), ptr(ga), ptr(gc), B, V, d, ptr(dynB), ptr(dE),
                                   dE.stride(0), ptr(ws.dsr_part), ptr(dsr), parts | (split << 8), stream())
    else:
        lib.srec_score_ce_bwd(ptr(sr), _ld(sr), ptr(table), table.stride(0), ptr(cs), ptr(labels), ptr(lse), ptr(gl),
                              ptr(ga), ptr(gc), B, V, d, ptr(dynB), ptr(dE), dE.stride(0), ptr(ws.dsr_part), ptr(dsr),
                              parts, stream())


def finish_table_grad(table, cs, cs_inv_scale, dE, tg):
    """the chain rule of the row normalisation on a table gradient dE the scoring backward has just written (cs None: the
    rows were scored as they are, nothing to do).  tg (an ops.TableGrad or None) with tg.defer: recorded in tg.pending and
    applied by the optimizer's row pass or TableGrad.materialize - linear, so once over the sum of several heads'
    contributions.  Otherwise projected out here, one row pass; the projection is idempotent, so safe after every
    accumulation."""
    if cs is None:
        return
    if tg is not None and tg.defer:
        tg.pending = (table, cs, cs_inv_scale)
    else:
        lib.srec_rownorm_project(ptr(table), table.stride(0), ptr(cs), cs_inv_scale, ptr(dE), dE.stride(0), table.shape[0],
                                 table.shape[1], stream())


def _ce_outputs(B, device):
    """(lse [B], lossvec [B], loss []) the forward kernels write"""
    return (torch.empty(B, device=device, dtype=torch.float32), torch.empty(B, device=device, dtype=torch.float32),
            torch.empty((), device=device, dtype=torch.float32))


def _ce_backward(ctx, gl, ga, gc, accumulate):
    """the backward both scoring nodes share: d sr returned, the dense table gradient overwritten in (or, accumulate, added to)
    ctx.tgrad.buf.  gl: the upstream scalar; ga / gc: per-session coefficients of softmax / label one-hot (None = 1)"""
    sr, table, cs, labels, lse = ctx.saved_tensors
    tg = ctx.tgrad
    dsr = torch.empty(sr.shape, device=sr.device, dtype=torch.float32)
    if not accumulate:
        tg.overwritten()
    _ce_bwd(sr, table, cs, labels, lse, gl, ga, gc, ctx.ws, ctx.dynB, ctx.tb, tg.buf, dsr, 3 | (4 if accumulate else 0))
    finish_table_grad(table, cs, ctx.cs_inv_scale, tg.buf, tg)
    tg.fresh = True
    return (dsr,) + (None,) * 8


class ScoreCE(torch.autograd.Function):
    """loss = mean_b CE(cs * sr_b E^T, label_b), logits never materialised.  Writes the dense
    table gradient into `tgrad.buf` (all rows) instead of returning it."""

    @staticmethod
    def forward(ctx, sr, table, cs, labels, ws, tgrad, dynB, cs_inv_scale, tb=None):
        sr = _rows(sr)
        lse, lossvec, loss = _ce_outputs(sr.shape[0], sr.device)
        _ce_fwd(sr, table, cs, labels, ws, dynB, tb, ws.lab_logit, lse, lossvec, loss)
        ctx.save_for_backward(sr, table, cs, labels, lse)
        ctx.ws, ctx.tgrad, ctx.dynB, ctx.cs_inv_scale, ctx.tb = ws, tgrad, dynB, cs_inv_scale, tb
        ctx.mark_non_differentiable(lse)
        ctx.set_materialize_grads(False)       # no zero-filled [B] gradient for the unused lse output (a fill kernel per step)
        return loss, lse

    @staticmethod
    def backward(ctx, gloss, _glse):
        return _ce_backward(ctx, gloss.reshape(1).to(torch.float32).contiguous(), None, None, False)


class ScoreStats(torch.autograd.Function):
    """(lse_b, z[b,label_b]) of the full-catalog logits, logits never materialised; differentiable in both
    outputs, so any loss built from them (mixtures of soft-maxes: msgifsr.py:311-317) trains through the
    fused kernels.  Several heads may share one table: the first backward of a step overwrites the dense
    table gradient, later ones accumulate."""

    @staticmethod
    def forward(ctx, sr, table, cs, labels, ws, tgrad, dynB, cs_inv_scale, tb=None):
        sr = _rows(sr)
        B, dev = sr.shape[0], sr.device
        lse, lossvec, loss = _ce_outputs(B, dev)
        lab = torch.zeros(B, device=dev, dtype=torch.float32)
        _ce_fwd(sr, table, cs, labels, ws, dynB, tb, lab, lse, lossvec, loss)
        ctx.save_for_backward(sr, table, cs, labels, lse)
        ctx.ws, ctx.tgrad, ctx.dynB, ctx.cs_inv_scale, ctx.tb = ws, tgrad, dynB, cs_inv_scale, tb
        return lse, lab

    @staticmethod
    def backward(ctx, dlse, dlab):
        return _ce_backward(ctx, None, dlse.contiguous().float(), (-dlab).contiguous().float(), ctx.tgrad.fresh)


def score_stats(sr, table, cs, labels, ws, tgrad, dynB=None, cs_inv_scale=1.0, tb=None):
    return ScoreStats.apply(sr, table, cs, labels, ws, tgrad, dynB, cs_inv_scale, tb)


def score_ce(sr, table, cs, labels, ws, tgrad, dynB=None, cs_inv_scale=1.0, tb=None):
    return ScoreCE.apply(sr, table, cs, labels, ws, tgrad, dynB, cs_inv_scale, tb)


_BYTE_WS = {}          # the evaluation / selection kernels: kinds 'topk', 'rank', 'select'
_NORM_WS = {}          # the log-normaliser of the serving calls: kind 'norm'
_SAMPLE_WS = {}        # the draws of the serving calls: kind 'sample'


def _byte_ws(kind, device, nbytes, cache=None):
    """never-resized byte scratch, one per (kind, device, size): the five kinds never share a buffer, so no two of their
    launches alias scratch that separate caches kept apart.  cache: the dict that holds it - _BYTE_WS (default) for the
    evaluation / selection kernels ('topk', 'rank', 'select'), _NORM_WS for score_norm ('norm') and _SAMPLE_WS for
    score_sample ('sample'), whose scratch lives beside them, not among them"""
    cache = _BYTE_WS if cache is None else cache
    key = (kind, device.index, nbytes)
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return ws


def _scratch(kind, device, ws_fn, *shape, cache=None):
    """the scratch of one launch: ask the library's *_ws entry point for the bytes of this shape (it refuses a shape outside
    the contract up front), take the never-resized buffer of that kind (_byte_ws)"""
    n = _ct.c_long()
    ws_fn(*shape, _ct.addressof(n))
    return _byte_ws(kind, device, n.value, cache)


def score_topk(sr, table, cs, k):
    """(values [B,k], item ids [B,k]) of the k largest z[b,v] = cs[v] <sr_b, E_v> - no (B, V) tensor (evaluation)"""
    sr = _rows(sr.detach())
    B, d = sr.shape
    V = table.shape[0]
    ws = _scratch('topk', sr.device, lib.srec_score_topk_ws, B, V, k)
    val = torch.empty(B, k, device=sr.device, dtype=torch.float32)
    idx = torch.empty(B, k, device=sr.device, dtype=torch.int32)
    lib.srec_score_topk(ptr(sr), _ld(sr), ptr(table), table.stride(0), ptr(cs), B, V, d, k, ptr(val), ptr(idx), ptr(ws),
                        stream())
    return val, idx


# what score_rank / score_select / score_items launch with: srs as (pointer, row stride, component stride), C components of [B, d];
# table [V, d] as rows; off_ex / off_in fp32 [C, B] or None; listed int32 [B, L] or None with L = 0
MixtureArgs = namedtuple('MixtureArgs', 'srs ld_sr comp C B d table V off_ex off_in listed L')
_LISTED_MAX = 64
_LISTED_TOO_MANY = {
    'score_rank': 'score_rank: %d listed items per session; the fix-up pass of csrc/rank.hip takes at most 64 '
                  '(evaluate such sessions with method="topk")',
    'score_select': 'score_select: %d listed items per session; csrc/recommend.hip takes at most 64',
    'score_items': 'score_items: %d listed items per session; csrc/score_items.hip takes at most 64',
    'score_norm': 'score_norm: %d listed items per session; csrc/score_norm.hip takes at most 64',
    'score_sample': 'score_sample: %d listed items per session; csrc/recommend.hip takes at most 64',
    'score_cutoff': 'score_cutoff: %d listed items per session; csrc/score_cutoff.hip takes at most 64',
    'score_select_many': 'score_select_many: %d listed items per session; csrc/select_many.hip takes at most 64',
    'score_ahead': 'score_ahead: %d listed items per session; csrc/rank_served.hip takes at most 64',
    'score_ahead_many': 'score_ahead_many: %d listed items per session; csrc/rank_served_many.hip takes at most 64',
}
_LISTED_TOO_MANY['cutoff_passes'] = _LISTED_TOO_MANY['score_cutoff']      # (score_cutoff's generator speaks of lists in its words)


def _mixture_args(who, srs, table, off_ex, off_in, listed):
    """The argument conventions score_rank, score_select and score_items share, as one MixtureArgs.  srs: [B, d] (row-strided views are
    taken as they are), [C, B, d], [1, B, d] or a list of C [B, d] tensors; off_ex / off_in: anything of C * B numbers or
    None; listed: [B, L] item ids, empty or None = no list.  More than 64 listed items per session raise ValueError in the
    words of `who`.  Pure torch (no launch, no library call): it checks CPU tensors as well."""
    if isinstance(srs, (list, tuple)):
        srs = srs[0] if len(srs) == 1 else torch.stack([s.detach() for s in srs], 0)
    srs = srs.detach()
    if srs.dim() == 3 and srs.shape[0] == 1:
        srs = srs[0]
    if srs.dim() == 2:
        srs = _rows(srs)
        C, (B, d) = 1, srs.shape
        ld_sr, comp = _ld(srs), 0
    else:
        assert srs.dim() == 3 and srs.dtype == torch.float32, (srs.shape, srs.dtype)
        srs = srs.contiguous()
        C, B, d = srs.shape
        ld_sr, comp = d, B * d
    table = _rows(table.detach())

    def offs(o):
        return None if o is None else o.detach().to(torch.float32).reshape(C, B).contiguous()
    L = 0
    if listed is not None and listed.numel() > 0:
        listed = listed.detach().to(torch.int32).reshape(B, -1).contiguous()
        L = listed.shape[1]
        if L > _LISTED_MAX:
            raise ValueError(_LISTED_TOO_MANY[who] % L)
    else:
        listed = None
    return MixtureArgs(srs, ld_sr, comp, C, B, d, table, table.shape[0], offs(off_ex), offs(off_in), listed, L)


# the per-item bias of score_select / score_items: bias fp32 [V] or [G, V] with unit column stride (None = no bias), its row
# stride, group int32 [B] or None, G rows
BiasArgs = namedtuple('BiasArgs', 'bias ld_bias group G')
_NO_BIAS = BiasArgs(None, 0, None, 1)


def _bias_args(who, bias, group, B, V):
    """The per-item bias of score_select and score_items as one BiasArgs.  bias: floating [V] (one row for all sessions) or
    [G, V] with group [B] integer row ids in [0, G) (a [1, V] bias needs none); None = no bias.  A tensor with unit column
    stride is taken as it is, whatever its row stride (a column slice of a wider tensor: a row shard of the catalogue);
    anything else is made contiguous fp32.  A wrong last dimension, more than 2 dimensions, a non-floating dtype, `group`
    without a 2-D bias or missing with G > 1, and a `group` that does not have B integer entries raise ValueError in the
    words of `who`.  The VALUES are not looked at (NaN, +inf and group ids out of range are the caller's to exclude: the
    model-level entry points check them).  Pure torch (no launch, no library call): it checks CPU tensors as well."""
    if bias is None:
        if group is not None:
            raise ValueError('%s: group is given without a bias' % who)
        return _NO_BIAS
    bias = bias.detach()
    if not bias.is_floating_point():
        raise ValueError('%s: bias must be a floating tensor, got %s' % (who, bias.dtype))
    if bias.dim() not in (1, 2):
        raise ValueError('%s: bias must be [V] or [G, V], got %d dimensions' % (who, bias.dim()))
    if bias.shape[-1] != V:
        raise ValueError('%s: bias has %d columns for %d table rows' % (who, bias.shape[-1], V))
    if bias.dim() == 1 and group is not None:
        raise ValueError('%s: group needs a 2-D bias [G, V], got [V]' % who)
    G = bias.shape[0] if bias.dim() == 2 else 1
    if G < 1:
        raise ValueError('%s: bias has no rows' % who)
    if G > 1 and group is None:
        raise ValueError('%s: a bias of %d rows needs group, one row id per session' % (who, G))
    if group is not None:
        group = group.detach()
        if group.is_floating_point() or group.is_complex() or group.dtype == torch.bool or group.numel() != B:
            raise ValueError('%s: group must hold %d integer row ids (one per session), got %s %s'
                             % (who, B, group.dtype, tuple(group.shape)))
        group = group.to(torch.int32).reshape(B).contiguous()
    if bias.dtype != torch.float32 or bias.stride(-1) != 1 or (bias.dim() == 2 and G > 1 and bias.stride(0) < V):
        bias = bias.to(torch.float32).contiguous()
    return BiasArgs(bias, bias.stride(0) if bias.dim() == 2 else V, group if G > 1 else None, G)


_Served = STRUCTS['srec_served']           # bound from include/srec.h (_lib.parse_structs), never retyped


class ServedArgs(namedtuple('ServedArgs', 'srs ld_sr comp table cs off_ex off_in listed L listed_mode id_lo B V d C '
                                          'bias ld_bias group G')):
    """The operands of the served score as every score_* call launches with them: the members of srec_served (include/srec.h)
    in its order, tensors where the struct has pointers - the record owns what the pointers will name."""
    __slots__ = ()

    def struct(self):
        """the host srec_served of one library call (keep it, and this record, alive across the call).  ptr(): a CPU tensor
        raises here, after every argument check"""
        srs, ld_sr, comp, table, cs, off_ex, off_in, listed, L, listed_mode, id_lo, B, V, d, C, bias, ld_bias, group, G = self
        return _Served(ptr(srs), ld_sr, comp, ptr(table), table.stride(0), ptr(cs), ptr(off_ex), ptr(off_in), ptr(listed), L,
                       listed_mode, id_lo, B, V, d, C, ptr(bias), ld_bias, ptr(group), G)


def _served_args(who, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group):
    """_mixture_args and _bias_args as one ServedArgs, errors in the words of `who`.  THE place where drop_listed becomes the
    listed mode and off_in is ignored under it.  Pure torch (no launch, no library call): it checks CPU tensors as well."""
    srs, ld_sr, comp, C, B, d, table, V, off_ex, off_in, listed, L = _mixture_args(who, srs, table, off_ex,
                                                                                  None if drop_listed else off_in, listed)
    mode = CONST['SREC_LISTED_DROP'] if drop_listed else CONST['SREC_LISTED_SCORE']
    return ServedArgs(srs, ld_sr, comp, table, cs, off_ex, off_in, listed, L, mode, int(id_lo), B, V, d, C,
                      *_bias_args(who, bias, group, B, V))


def catalog_bias(num_items, allow=None, deny=None, boost=None, device=None):
    """fp32 [num_items], the `bias` of score_select / score_items and the `item_bias` of the models' recommend / score_items /
    rerank, from the usual catalogue controls: allow (ids) - -inf everywhere EXCEPT these; deny (ids) - -inf on these; boost
    ((ids, values)) - added on top (an id named twice: its values add up); a boost on a filtered item stays -inf.  Ids are
    sequences or integer tensors; an id outside [0, num_items) raises ValueError.  Pure torch."""
    def ids_of(x, what):
        x = torch.as_tensor(x, device=device).reshape(-1)
        if x.numel() and (x.is_floating_point() or x.dtype == torch.bool):
            raise ValueError('catalog_bias: %s ids must be integers, got %s' % (what, x.dtype))
        x = x.long()
        if x.numel():
            lo, hi = (int(v) for v in torch.aminmax(x))
            if lo < 0 or hi >= num_items:
                raise ValueError('catalog_bias: %s id %d; ids are in [0, %d)' % (what, lo if lo < 0 else hi, num_items))
        return x
    ninf = float('-inf')
    if allow is not None:
        out = torch.full((num_items,), ninf, dtype=torch.float32, device=device)
        out[ids_of(allow, 'allow')] = 0.0
    else:
        out = torch.zeros(num_items, dtype=torch.float32, device=device)
    if deny is not None:
        out[ids_of(deny, 'deny')] = ninf
    if boost is not None:
        ids, vals = boost
        ids = ids_of(ids, 'boost')
        vals = torch.as_tensor(vals, dtype=torch.float32, device=device).reshape(-1)
        if vals.numel() != ids.numel():
            raise ValueError('catalog_bias: boost has %d ids and %d values' % (ids.numel(), vals.numel()))
        out.index_add_(0, ids, vals)
    return out


def score_rank(srs, table, cs, labels, off_ex=None, off_in=None, listed=None, id_lo=0, target=None, target_only=False):
    """(rank int32 [B], target fp32 [B]): the number of rows of `table` that score ahead of each session's label under
    s[b,v] = logsumexp_c(cs[v] <sr_c[b], E_v> + off[c,b]) (off_in for the items of listed[b,:], off_ex elsewhere; ties
    towards the lower item id) - no (B, V) tensor, no cutoff (csrc/rank.hip).  srs: [B, d], [C, B, d] or a list of C
    [B, d] tensors, C <= 4; off_ex / off_in: [C, B] or None (= 0); listed: [B, L] item ids, -1 = empty slot; labels:
    global item ids (< 0: rank -1); id_lo: global id of table row 0 (a row shard).  target: the labels' scores when they
    are already known (the sharded case: summed over the shards) - else computed here, 0 for labels other shards own.
    target_only: (None, target) from the target pass alone - a shard's share ahead of that sum."""
    a = _served_args('score_rank', srs, table, cs, off_ex, off_in, listed, False, id_lo, None, None)
    B, dev = a.B, a.srs.device
    if B == 0:
        return torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.float32)
    labels = labels.detach().to(torch.int32).contiguous()
    assert labels.numel() == B, (labels.shape, B)
    # the C ABI carries a workspace (partial counts per range are one legal implementation); the current kernels meet in
    # integer atomics and ask for a token size only - the call still validates the shape contract up front
    ws = _scratch('rank', dev, lib.srec_score_rank_ws, B, a.V, a.d, a.C, a.L)
    given = target is not None
    target = target.detach().to(torch.float32).contiguous() if given else torch.empty(B, device=dev, dtype=torch.float32)
    rank = None if target_only else torch.empty(B, device=dev, dtype=torch.int32)
    desc = a.struct()
    lib.srec_score_rank(_ct.addressof(desc), ptr(labels), ptr(target), int(given), ptr(rank), ptr(ws), stream())
    return rank, target


def _floor_arg(who, floor, B, dev):
    """floor as fp32 [B] on the device (None stays None: no floor)"""
    if floor is None:
        return None
    f = torch.as_tensor(floor).detach()
    if not f.is_floating_point() or f.numel() != B:
        raise ValueError('%s: floor must hold %d floating numbers (one per session), got %s %s' % (who, B, f.dtype, tuple(f.shape)))
    return f.to(device=dev, dtype=torch.float32).reshape(B).contiguous()


def score_select(srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
                 floor=None):
    """(values fp32 [B,k] descending, item ids int32 [B,k]): the k best rows of `table` per session under the score of
    score_rank, s[b,v] = logsumexp_c(cs[v] <sr_c[b], E_v> + off[c,b]) - no (B, V) tensor, k <= 128 (csrc/recommend.hip).
    Argument conventions as score_rank: srs [B, d], [C, B, d] or a list of C [B, d] tensors, C <= 4; off_ex / off_in [C, B]
    or None (= 0); listed [B, L] global item ids, -1 = empty slot; id_lo: global id of table row 0 (a row shard).
    drop_listed=False: listed items score with off_in; True: listed items are never returned (off_in is ignored).  Ties go
    towards the lower id; a session with fewer than k eligible rows ends in (-inf, -1) slots.
    bias: fp32 [V] or [G, V] aligned with the rows of `table` (group: [B] row ids in [0, G)), added AFTER the mixture -
    s + bias[group[b], v]; -inf = the item is not in the catalogue for this call and is never returned, the order and the
    values are those of the biased score (_bias_args; no NaN, no +inf, no group id out of range: not checked here).  Without a
    bias the call and its result are what they were.
    floor: fp32 [B] or None - a row whose biased score is below floor[b] is ineligible for session b (score_cutoff finds the
    floor of a top-k / top-p / min-p truncation); None: the call is what it was, the same kernel instances."""
    k = int(k)
    if k < 1 or k > CONST['SREC_SELECT_MAXK']:
        raise ValueError('score_select: k = %d; the selection kernel of csrc/recommend.hip keeps between 1 and %d items per '
                         'session' % (k, CONST['SREC_SELECT_MAXK']))
    a = _served_args('score_select', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    val = torch.empty(B, k, device=dev, dtype=torch.float32)
    idx = torch.empty(B, k, device=dev, dtype=torch.int32)
    if B == 0:
        return val, idx
    ws = _scratch('select', dev, lib.srec_score_select_ws, B, a.V, a.d, a.C, a.L, k)
    floor = _floor_arg('score_select', floor, B, dev)
    desc = a.struct()
    # (no bias: bias NULL, G 1; no floor: NULL - the plain call, the same kernel instances)
    lib.srec_score_select(_ct.addressof(desc), k, ptr(floor), ptr(val), ptr(idx), ptr(ws), stream())
    return val, idx


def score_ahead(srs, table, cs, labels, target, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None,
                group=None, floor=None):
    """int32 [B]: the number of ELIGIBLE rows of `table` that stand ahead of each session's label under the biased score s' of
    score_select - the rank of the label among what is SERVED (a bias, allow / deny lists, exclude-seen, a truncation floor),
    which score_rank refuses to compute - no (B, V) tensor (csrc/rank_served.hip: one pass, listed items resolved inside it,
    integer atomics; equal bits on every call).  labels: [B] global item ids (< 0: 0); target: fp32 [B], the label's own s' -
    what score_items returns at labels[:, None] with the same operands (summed over row shards).  A row counts when it is
    eligible (not listed under drop_listed, bias > -inf), is not the label (by id), is not below floor[b] (floor: fp32 [B] or
    None, score_cutoff's) and scores above target[b], or equal to it with a lower id - the tie rule of score_select, so with
    (labels, target) = (ids[:, j], values[:, j]) of score_select over the same operands the result is j.  Whether the label
    itself could be shown (target > -inf, target >= floor) is the caller's test: model.served_rank makes it.  Other arguments
    as score_select; id_lo: global id of table row 0 - counts of disjoint row shards add up, a shard without rows gives 0."""
    a = _served_args('score_ahead', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    labels = torch.as_tensor(labels).detach()
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool or labels.numel() != B:
        raise ValueError('score_ahead: labels must hold %d integer item ids (one per session), got %s %s'
                         % (B, labels.dtype, tuple(labels.shape)))
    target = torch.as_tensor(target).detach()
    if not target.is_floating_point() or target.numel() != B:
        raise ValueError('score_ahead: target must hold %d floating numbers (the labels\' scores), got %s %s'
                         % (B, target.dtype, tuple(target.shape)))
    floor = _floor_arg('score_ahead', floor, B, dev)
    if B == 0 or a.V == 0:
        return torch.zeros(B, device=dev, dtype=torch.int32)
    if labels.dtype != torch.int32:         # (an id beyond int32 stays beyond every local row: the kernel clamps around them)
        labels = labels.to(torch.int64).clamp(min=-1, max=2 ** 31 - 1).to(torch.int32)
    labels = labels.to(dev).reshape(B).contiguous()
    target = target.to(device=dev, dtype=torch.float32).reshape(B).contiguous()
    # no scratch: the counts meet in integer atomics (srec_score_ahead_ws is a token); the call validates the shape up front
    n = _ct.c_long()
    lib.srec_score_ahead_ws(B, a.V, a.d, a.C, a.L, _ct.addressof(n))
    out = torch.empty(B, device=dev, dtype=torch.int32)
    desc = a.struct()
    lib.srec_score_ahead(_ct.addressof(desc), ptr(labels), ptr(target), ptr(floor), ptr(out), None, stream())
    return out


def ahead_among_targets(items, target, floor=None):
    """int32 [B, M]: the A part of score_ahead_many - how many of a session's OTHER targets stand ahead of each of them by
    their given values: A[b,j] = #{ i != j live : items[b,i] != items[b,j], target[b,i] > -inf, !(target[b,i] < floor[b]),
    target[b,i] > target[b,j] or (equal and items[b,i] < items[b,j]) }; a slot with items < 0 is empty, counts for nobody and
    gets 0.  It needs no table: the sharded route adds it once after the all-reduce, the materialised evaluation uses it too.
    Plain torch on any device."""
    items = torch.as_tensor(items).detach()
    target = torch.as_tensor(target).detach().to(device=items.device, dtype=torch.float32)
    B, M = items.shape
    u = items.to(torch.int64)
    live = u >= 0
    f = torch.full((B,), float('-inf'), device=items.device) if floor is None else \
        torch.as_tensor(floor).detach().to(device=items.device, dtype=torch.float32).reshape(B)
    counts = live & (target > float('-inf')) & ~(target < f[:, None])                  # [B, i]: i can stand ahead of somebody
    ti, tj, ui, uj = target[:, :, None], target[:, None, :], u[:, :, None], u[:, None, :]
    ahead = counts[:, :, None] & live[:, None, :] & (ui != uj) & ((ti > tj) | ((ti == tj) & (ui < uj)))
    return ahead.sum(1).to(torch.int32)


def score_ahead_many(srs, table, cs, items, target, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None,
                     group=None, floor=None, among_targets=True):
    """int32 [B, M]: score_ahead for M given items per session in ONE pass over the table (csrc/rank_served_many.hip) - where
    each of them stands among what is SERVED.  items: [B, M] global item ids, 1 <= M <= 64, an entry < 0 is an empty slot
    (result 0), every id at most once per row (not checked here: the model-level entry points refuse duplicates); target:
    fp32 [B, M], the items' own s' - what score_items returns at `items` with the same operands (summed over row shards).
    ahead[b,j] = N + A.  N: the eligible rows that are NOT one of items[b,:] (left out by id), are not below floor[b] and score
    above target[b,j], or equal to it with a lower id.  A (among_targets=True): the session's other targets that could be
    shown (target > -inf, not below the floor) and stand ahead of j by their GIVEN values, ties towards the lower id
    (ahead_among_targets) - so a session's shown targets get pairwise distinct ranks, and round-off between the gather kernel
    and the pass cannot make two targets count against each other.  With M = 1 the result is score_ahead's, bit for bit; N of
    disjoint row shards adds up (among_targets=False on the shards, A added once).  Whether a target itself could be shown is
    the caller's test: model.rank_items makes it.  Integer atomics: equal bits on every call.  Other arguments as score_ahead."""
    a = _served_args('score_ahead_many', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    items = torch.as_tensor(items).detach()
    if items.is_floating_point() or items.is_complex() or items.dtype == torch.bool or items.dim() != 2 or items.shape[0] != B:
        raise ValueError('score_ahead_many: items must hold [%d, M] integer item ids, got %s %s' % (B, items.dtype, tuple(items.shape)))
    M = items.shape[1]
    if not 1 <= M <= CONST['SREC_AHEAD_MAXT']:
        raise ValueError('score_ahead_many: %d items per session; csrc/rank_served_many.hip takes between 1 and %d'
                         % (M, CONST['SREC_AHEAD_MAXT']))
    target = torch.as_tensor(target).detach()
    if not target.is_floating_point() or tuple(target.shape) != (B, M):
        raise ValueError('score_ahead_many: target must hold [%d, %d] floating numbers (the items\' scores), got %s %s'
                         % (B, M, target.dtype, tuple(target.shape)))
    floor = _floor_arg('score_ahead_many', floor, B, dev)
    if B == 0:
        return torch.zeros(0, M, device=dev, dtype=torch.int32)
    if items.dtype != torch.int32:          # (an id beyond int32 stays beyond every local row: the kernel clamps around them)
        items = items.to(torch.int64).clamp(min=-1, max=2 ** 31 - 1).to(torch.int32)
    items = items.to(dev).contiguous()
    target = target.to(device=dev, dtype=torch.float32).contiguous()
    if a.V == 0:                            # a shard without rows: the targets among themselves, or nothing
        return ahead_among_targets(items, target, floor) if among_targets else torch.zeros(B, M, device=dev, dtype=torch.int32)
    # no scratch: the counts meet in integer atomics (srec_score_ahead_many_ws is a token); the call validates the shape up front
    n = _ct.c_long()
    lib.srec_score_ahead_many_ws(B, a.V, a.d, a.C, a.L, M, _ct.addressof(n))
    out = torch.empty(B, M, device=dev, dtype=torch.int32)
    desc = a.struct()
    lib.srec_score_ahead_many(_ct.addressof(desc), ptr(items), ptr(target), M, M, ptr(floor), int(bool(among_targets)), ptr(out),
                              None, stream())
    return out


def _seed_words(who, seed):
    """a seed as the int the library takes: any integer in [0, 2^64)"""
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError('%s: seed must be an integer in [0, 2^64), got %r' % (who, seed))
    return seed


def _session_keys(who, session_keys, B):
    """session_keys as int32 [B] on their device (None stays None: the row index).  Keys are 32-bit values: an integer outside
    [-2^31, 2^31) is taken modulo 2^32"""
    if session_keys is None:
        return None
    q = torch.as_tensor(session_keys).detach()
    if q.is_floating_point() or q.is_complex() or q.dtype == torch.bool or q.numel() != B:
        raise ValueError('%s: session_keys must hold %d integers (one per session), got %s %s'
                         % (who, B, q.dtype, tuple(q.shape)))
    return q.reshape(B).to(torch.int32).contiguous()


def _mul32(x, c):
    """x * c mod 2^32 for int64 tensors x in [0, 2^32) and an int c in [0, 2^32) - no product leaves int64"""
    return ((x & 0xffff) * c + ((((x >> 16) * c) & 0xffff) << 16)) & 0xffffffff


def _h32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


_LN2 = 0.6931471805599453


def _log64(x):
    """natural log of positive finite float64 x from +, -, *, / and frexp alone (each correctly rounded everywhere), so that
    sample_noise gives the same BITS on every host and in every restatement that follows these lines - a library log does
    not (torch, numpy and libm differ in the last bit).  x = m 2^e with m in [sqrt(1/2), sqrt(2)), t = (m - 1) / (m + 1),
    log m = 2 t (1 + t^2/3 + ... + t^26/27): |t| <= 0.172, truncation below 2e-22; error a few 1e-16 relative to max(1, |log x|)"""
    m, e = torch.frexp(x)
    small = m < 0.7071067811865476
    m = torch.where(small, m * 2.0, m)
    e = e.double() - small.double()
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = torch.full_like(t, 1.0 / 27.0)
    for n in range(25, 0, -2):
        p = p * t2 + 1.0 / n
    return e * _LN2 + 2.0 * t * p


def sample_scalars(who, k, temperature, seed):
    """(k, 1 / temperature, seed) as the library takes them, or ValueError in the words of `who`: k in 1 .. 128, temperature
    positive and finite (and 1 / temperature finite in fp32), seed an integer in [0, 2^64).  No launch, no library call"""
    k = int(k)
    if k < 1 or k > CONST['SREC_SELECT_MAXK']:
        raise ValueError('%s: k = %d; the selection kernel of csrc/recommend.hip keeps between 1 and %d items per session'
                         % (who, k, CONST['SREC_SELECT_MAXK']))
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise ValueError('%s: temperature must be a number, got %r' % (who, temperature)) from None
    if not (0.0 < temperature < float('inf')) or not (1.0 / temperature < 3.4e38):
        raise ValueError('%s: temperature = %r; it must be positive and finite' % (who, temperature))
    return k, 1.0 / temperature, _seed_words(who, seed)


def sample_noise(seed, session_keys, ids):
    """float64 [nb, nv]: the Gumbel noise g(seed, q, id) score_sample adds to score / temperature, for session keys q
    (integers, taken modulo 2^32) and GLOBAL item ids - the documented way to reproduce a draw: the ids score_sample returns
    are the k best of  score / T + g  over the eligible items (to the fp32 rounding of the kernel's own score and logs).  Pure
    torch on the CPU, no library call; the formula is that of include/srec.h (srec_score_sample): w is formed in fp32 exactly
    as the kernel forms it, the two logarithms are taken in float64 by _log64 (arithmetic only: equal bits on every host)."""
    seed = _seed_words('sample_noise', seed)
    m = 0xffffffff
    q = torch.as_tensor(session_keys).detach().cpu().reshape(-1).to(torch.int64) & m
    gid = torch.as_tensor(ids).detach().cpu().reshape(-1).to(torch.int64) & m
    lo, hi = seed & m, seed >> 32
    skey = _h32(lo ^ _h32((_mul32(q, 0x9E3779B9) + (hi * 0x85EBCA6B + 0x165667B1) % 2 ** 32) & m))
    h = _h32(skey[:, None] ^ ((_mul32(gid, 0x9E3779B1) + 0x7F4A7C15) & m)[None, :])
    # fmaf((float)h, 2^-32, 2^-33): the product and the sum are exact in float64, so one rounding to fp32 is the fused result
    w = (h.to(torch.float32).double() * 2.0 ** -32 + 2.0 ** -33).to(torch.float32).clamp(max=1.0 - 2.0 ** -24)
    # log1p(-w) by Kahan's identity on the rounded u = 1 - w (u == 1: -w itself), then g = -log(-log1p(-w))
    w = w.double()
    u = 1.0 - w
    one = u == 1.0
    l1 = torch.where(one, -w, _log64(u) * (-w) / torch.where(one, torch.full_like(u, -1.0), u - 1.0))
    return -_log64(-l1)


def score_sample(srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
                 temperature=1.0, seed=0, session_keys=None, floor=None):
    """(keys fp32 [B,k] descending, item ids int32 [B,k] in draw order): k DISTINCT rows of `table` per session drawn without
    replacement (Plackett-Luce) from p(v) ~ exp(s'[b,v] / temperature) over the eligible rows, s' the biased score of
    score_select and its eligibility - no (B, V) tensor, k <= 128 (csrc/recommend.hip, the selection over the sampled key
    s' / T + g; Gumbel-top-k).  Arguments as score_select.  temperature: a positive finite scalar.  seed: an integer in
    [0, 2^64).  session_keys: [B] integers (32-bit values), None = the row index; the noise g is a pure function of (seed,
    session key, global item id) - sample_noise() restates it - so a call is reproducible, a session with the same key draws
    the same items in any batch, and row shards (id_lo) merge by (key, id) to the bits of one call over the whole table.  A
    session with fewer than k eligible rows ends in (-inf, -1) slots.  The keys are NOT log-probabilities: score the ids
    (score_items) for those.
    floor: fp32 [B] or None - the draw is among the rows with s' >= floor[b] only (tested on s', before temperature and noise:
    truncated sampling, the floor of score_cutoff); None: the call is what it was, the same kernel instances."""
    k, inv_t, seed = sample_scalars('score_sample', k, temperature, seed)
    a = _served_args('score_sample', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    q = _session_keys('score_sample', session_keys, B)
    key = torch.empty(B, k, device=dev, dtype=torch.float32)
    idx = torch.empty(B, k, device=dev, dtype=torch.int32)
    if B == 0:
        return key, idx
    if q is not None:
        q = q.to(dev)
    ws = _scratch('sample', dev, lib.srec_score_sample_ws, B, a.V, a.d, a.C, a.L, k, cache=_SAMPLE_WS)
    floor = _floor_arg('score_sample', floor, B, dev)
    desc = a.struct()
    lib.srec_score_sample(_ct.addressof(desc), k, inv_t, seed, ptr(q), ptr(floor), ptr(key), ptr(idx), ptr(ws), stream())
    return key, idx


def score_items(srs, table, cs, items, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, checked=False,
                bias=None, group=None):
    """fp32 [B, M]: the score of score_rank / score_select, s[b,v] = logsumexp_c(cs[v] <sr_c[b], E_v> + off[c,b]), at the
    given items of every session - no (B, V) tensor, no limit on M (csrc/score_items.hip: one gather pass, the session
    vectors in registers).  items: [B, M] global ids per session or [M] shared by all sessions, any integer dtype; -1 is
    padding and gives -inf; duplicates are scored independently.  Argument conventions as score_select: srs [B, d],
    [C, B, d] or a list of C [B, d] tensors, C <= 4; off_ex / off_in [C, B] or None (= 0); listed [B, L] global item ids,
    -1 = empty slot; drop_listed=False: listed items score with off_in; True: they give -inf (off_in is ignored).  id_lo:
    global id of table row 0 (a row shard): an id outside [id_lo, id_lo + rows) gives 0.0, so the results of disjoint shards
    add up.  An id < -1 raises ValueError before any launch (one device-to-host read of the smallest id; checked=True: the
    caller has looked already); an upper bound cannot be checked here - a shard sees only its own range - the model-level
    entry (model.score_items) checks it.
    bias / group as in score_select: the rows' owner adds bias[group[b], row] after the mixture and -inf stays -inf; a padding
    slot still gives -inf and a foreign id 0.0 without a read of the table or of the bias, so shards still add up.
    Measured at B 512, V 37 484, d 256 (profiles/score_items_timing.txt): with the lse pass a single
    soft-max needs ahead of it, this route beats score_logp(...).gather(1, items) up to M = 2000 (342 against 352 us) and
    loses at M = 4000 (462 against 370 us) - for lists of several thousand items per session materialise instead; a C = 3
    mixture stays 2.6x ahead of forward().gather at M = 4000."""
    a = _served_args('score_items', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    items = items.detach()
    if items.is_floating_point() or items.is_complex() or items.dtype == torch.bool or items.dim() not in (1, 2):
        raise TypeError('score_items: items must be an integer tensor [B, M] or [M], got %s %s' % (items.dtype, tuple(items.shape)))
    if items.dim() == 2 and items.shape[0] != B:
        raise ValueError('score_items: items has %d rows for %d sessions' % (items.shape[0], B))
    M = items.shape[-1]
    out = torch.empty(B, M, device=dev, dtype=torch.float32)
    if B == 0 or M == 0:
        return out
    if not checked and int(items.min()) < -1:
        raise ValueError('score_items: item id %d; ids are >= 0, or -1 for a padding slot' % int(items.min()))
    items = items.to(torch.int32).contiguous()
    desc = a.struct()
    lib.srec_score_items(_ct.addressof(desc), ptr(items), M if items.dim() == 2 else 0, M, ptr(out), stream())
    return out


def score_norm(srs, table, cs, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None):
    """fp32 [B]: Z[b] = logsumexp over the ELIGIBLE rows v of `table` of the score of score_select, s[b,v] + bias[group[b], v]
    with s[b,v] = logsumexp_c(cs[v] <sr_c[b], E_v> + off[c,b]) - the normaliser under which the values of score_select /
    score_items become log-probabilities over what can be shown: pass off_ex - Z (and off_in - Z) to them.  No (B, V)
    tensor (csrc/score_norm.hip: one online log-sum-exp pass over the table, partials folded in a fixed order - no atomics,
    equal bits on every call).  Argument conventions and eligibility as score_select: srs [B, d], [C, B, d] or a list of C
    [B, d] tensors, C <= 4; off_ex / off_in [C, B] or None (= 0); listed [B, L] global item ids, -1 = empty slot;
    drop_listed=False: listed items contribute with off_in; True: they do not contribute (off_in is ignored); an item whose
    bias is -inf does not contribute; id_lo: global id of table row 0 (a row shard: the Z of disjoint shards combine by
    logsumexp).  A session with no eligible row gives exactly -inf, never NaN.
    Measured at B 512, V 37 484, d 256 (profiles/score_norm_timing.md): 180 us at C = 1 against 427 us
    for score_logp(...) + torch.logsumexp and 203 us for the statistics pass (score_stats); 506 - 552 us at C = 3 (a [4, V]
    bias, a 20-item list scored or dropped) against 1.7 - 3.2 ms for the three-matrix mixture - no row in which materialising
    is faster."""
    a = _served_args('score_norm', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    out = torch.empty(B, device=dev, dtype=torch.float32)
    if B == 0:
        return out
    ws = _scratch('norm', dev, lib.srec_score_norm_ws, B, a.V, a.d, a.C, a.L, cache=_NORM_WS)
    desc = a.struct()
    lib.srec_score_norm(_ct.addressof(desc), ptr(out), ptr(ws), stream())
    return out


_CUTOFF_WS = {}        # the cutoff of truncated sampling: kind 'cutoff' (and its own 'select' scratch for the K = 1 maximum)


def cutoff_scalars(who, top_k, top_p, min_p, temperature):
    """(top_k, top_p, min_gap, 1 / temperature) as the library takes them, or ValueError in the words of `who`.  top_k: None
    or an integer in [1, 2^31) (-> 0 = absent); top_p: None or a number > 0, not NaN (>= 1 and None -> 1.0 = absent; a p that
    rounds to 0 in fp32 is refused); min_p: None or a number q in (0, 1] (-> min_gap = -T ln q, computed in double and rounded
    once to fp32; None -> inf = absent); temperature positive and finite, as sample_scalars.  No launch, no library call"""
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise ValueError('%s: temperature must be a number, got %r' % (who, temperature)) from None
    if not (0.0 < temperature < float('inf')) or not (1.0 / temperature < 3.4e38):
        raise ValueError('%s: temperature = %r; it must be positive and finite' % (who, temperature))
    k = 0
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k < 2 ** 31:
            raise ValueError('%s: top_k = %r; it is an integer >= 1 (any size below 2^31), or None' % (who, top_k))
        k = top_k
    p = 1.0
    if top_p is not None:
        try:
            p = float(top_p)
        except (TypeError, ValueError):
            raise ValueError('%s: top_p must be a number, got %r' % (who, top_p)) from None
        if isinstance(top_p, bool) or not p > 0.0 or _ct.c_float(p).value <= 0.0:
            raise ValueError('%s: top_p = %r; it is a probability mass in (0, 1) (>= 1 or None: no nucleus)' % (who, top_p))
        p = min(_ct.c_float(p).value, 1.0)          # (as the library sees it: a p that rounds to 1 in fp32 is no criterion)
    gap = float('inf')
    if min_p is not None:
        try:
            q = float(min_p)
        except (TypeError, ValueError):
            raise ValueError('%s: min_p must be a number, got %r' % (who, min_p)) from None
        if isinstance(min_p, bool) or not 0.0 < q <= 1.0:
            raise ValueError('%s: min_p = %r; it is a fraction of the best item\'s probability in (0, 1], or None' % (who, min_p))
        import math
        gap = _ct.c_float(abs(-temperature * math.log(q))).value
    return k, p, gap, 1.0 / temperature


def score_cutoff(srs, table, cs, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
                 top_k=None, top_p=None, min_p=None, temperature=1.0, reduce_max=None, reduce_sum=None):
    """(floor fp32 [B], count int32 [B], log_kept fp32 [B], top fp32 [B]): the score cutoff of TRUNCATED sampling over the
    eligible rows of `table` under the biased score s' of score_select, at the temperature the draw will use - no (B, V)
    tensor, no sort, no cumulative sum (csrc/score_cutoff.hip; the contract is in include/srec.h).  With m the largest eligible
    s', w_v = exp((s'_v - m) / temperature) and W their sum: top_k (any size) - the k-th largest eligible s' (-inf with fewer
    than k eligible rows); top_p - the largest score value t whose items at or above it hold w >= p W (the nucleus; ties at the
    boundary are all inside); min_p = q - m + temperature * ln q.  floor is the largest of those given (-inf with none); count
    the eligible rows with s' >= floor; log_kept = log(their w / W) <= 0; top = m.  Nothing eligible: (-inf, 0, -inf, -inf).
    Pass floor to score_select / score_sample (floor=) to select or draw inside the kept set.
    Arguments as score_norm.  The search is exact: an order-preserving 32-bit key of s', 8 bits per pass over the table, integer
    histograms (counts; fixed-point mass, quantum 2^-44), so the result is a pure function of the inputs - equal bits on
    every call, for any launch split, and for row shards: reduce_max (on the fp32 [B] maxima) and reduce_sum (on every int64
    partial between the passes) are the shards' all-reduces (dist.VocabParallel.cutoff); None = one device, one library call.
    A shard without rows (an empty `table`) joins every reduce with neutral partials and launches no pass.
    Measured at B 512, V 37 484, d 256 (profiles/score_cutoff_timing.md): C = 1 - 1.17 ms for top_k alone,
    1.50 ms for top_p alone and 1.60 ms for both (a histogram pass costs 159 - 311 us beside 177 us for the log-mass pass of
    score_norm) against 1.65 ms for score_logp + torch.sort + cumsum; C = 3 with a [4, V] bias and a 20-item dropped list -
    2.99 ms for top_p against 2.92 ms materialised: there the materialised route is 2.5 % ahead, and 23 % with both criteria
    (3.58 ms); at a shard of V 1 250 000 (C = 1) 37.8 ms against 70.1 ms.  min_p alone needs no search: 0.52 ms."""
    c = _cutoff_operands('score_cutoff', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group, top_k, top_p,
                         min_p, temperature)
    a = c.a
    if a.B == 0:
        return c.out
    if reduce_max is None and reduce_sum is None:
        ws = _scratch('cutoff', a.srs.device, lib.srec_score_cutoff_ws, a.B, a.V, a.d, a.C, a.L, cache=_CUTOFF_WS)
        lib.srec_score_cutoff(_ct.addressof(c.desc), c.inv_t, c.k, c.p, c.gap, *[ptr(t) for t in c.out], ptr(ws), stream())
        return c.out
    same = lambda t: t
    reduce = {'max': reduce_max or same, 'sum': reduce_sum or same}
    steps = _cutoff_passes(c)
    try:
        kind, part = next(steps)
        while True:
            kind, part = steps.send(reduce[kind](part).contiguous())
    except StopIteration as done:
        return done.value


def cutoff_passes(srs, table, cs, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
                  top_k=None, top_p=None, min_p=None, temperature=1.0):
    """score_cutoff pass by pass, as a generator - for callers that combine the partials of row shards themselves: it yields
    ('max', fp32 [B]) once and then ('sum', int64 [B, 3, 256]) after every pass over the table, expects the combined tensor
    back (generator.send; it may be the yielded tensor itself, reduced in place) and returns score_cutoff's tuple
    (StopIteration.value).  score_cutoff(reduce_max=, reduce_sum=) is this loop with the two callables."""
    return _cutoff_passes(_cutoff_operands('cutoff_passes', srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group,
                                           top_k, top_p, min_p, temperature))


# what the library calls of one cutoff take: the checked scalars, the served operands (a: the ServedArgs, which owns the
# tensors; desc: its srec_served, None for an empty batch) and the outputs (floor, count, log_kept, top)
CutoffOperands = namedtuple('CutoffOperands', 'k p gap inv_t a desc out')


def _cutoff_operands(who, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group, top_k, top_p, min_p, temperature):
    k_, p_, gap, inv_t = cutoff_scalars(who, top_k, top_p, min_p, temperature)
    a = _served_args(who, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    desc = a.struct() if B > 0 else None
    out = (torch.empty(B, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.int32),
           torch.empty(B, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32))
    return CutoffOperands(k_, p_, gap, inv_t, a, desc, out)


def _cutoff_passes(c):
    floor, count, log_kept, top = c.out
    a = c.a
    B, dev = a.B, a.srs.device
    if B == 0:
        return c.out
    served = _ct.addressof(c.desc)
    rows = a.V > 0                       # (a shard without rows: neutral partials in EVERY reduce, no pass over a table)
    if rows:
        ws = _scratch('select', dev, lib.srec_score_select_ws, B, a.V, a.d, a.C, a.L, 1, cache=_CUTOFF_WS)
        ids = torch.empty(B, device=dev, dtype=torch.int32)
        lib.srec_score_select(served, 1, None, ptr(top), ptr(ids), ptr(ws), stream())
    else:
        top.fill_(float('-inf'))
    top = yield 'max', top
    hist = torch.zeros(B, 3, 256, device=dev, dtype=torch.int64)
    state = torch.zeros(B, CONST['SREC_CUTOFF_STATE'], device=dev, dtype=torch.int64)
    passes = CONST['SREC_CUTOFF_PASSES']

    def partial(launch, *args):
        """this shard's histogram of one pass: the pass entry points zero `hist` themselves; a shard without rows zeroes it
        here - what came back from the last reduce (possibly in place) is the sum over ALL shards, not a neutral partial"""
        if rows:
            launch(served, c.inv_t, *args, ptr(hist), stream())
        else:
            hist.zero_()
        return hist
    if c.k > 0 or c.p < 1.0:
        for j in range(passes):
            hist = yield 'sum', partial(lib.srec_score_cutoff_hist, c.k, c.p, j, ptr(top), ptr(state))
            lib.srec_score_cutoff_advance(B, j, c.k, c.p, c.gap, ptr(hist), ptr(state), ptr(top), ptr(floor), stream())
    else:
        lib.srec_score_cutoff_advance(B, passes, 0, 1.0, c.gap, None, None, ptr(top), ptr(floor), stream())
    hist = yield 'sum', partial(lib.srec_score_cutoff_tail, ptr(top), ptr(floor))
    lib.srec_score_cutoff_finish(B, ptr(hist), ptr(count), ptr(log_kept), stream())
    return floor, count, log_kept, top


_MANY_WS = {}          # the collect buffers of score_select_many: kind 'select_many'


def select_many_k(who, k):
    """k of a long list as the library takes it, or ValueError in the words of `who`: 1 .. SREC_SELECT_MANY_MAXK"""
    k = int(k)
    if k < 1 or k > CONST['SREC_SELECT_MANY_MAXK']:
        raise ValueError('%s: k = %d; csrc/select_many.hip orders between 1 and %d items per session'
                         % (who, k, CONST['SREC_SELECT_MANY_MAXK']))
    return k


def _collect_many(a, floor, cap):
    """the collect pass of csrc/select_many.hip over the ServedArgs a: (values fp32 [B, capq], ids int32 [B, capq], n int32
    [B], capq) - row b holds, in no particular order, the n[b] eligible pairs at or above floor[b] (the first capq of them
    if there were more).  capq: cap rounded up to a multiple of 256 (and not past SREC_SELECT_MANY_SORT when cap is within
    it), so that the never-resized scratch (_byte_ws) comes in a few sizes"""
    B, dev = a.B, a.srs.device
    sort = CONST['SREC_SELECT_MANY_SORT']
    capq = (cap + 255) // 256 * 256
    if cap <= sort:
        capq = min(capq, sort)
    ws = _byte_ws('select_many', dev, B * capq * 8 + B * 4, _MANY_WS)
    bv = ws[:B * capq * 4].view(torch.float32).view(B, capq)
    bi = ws[B * capq * 4:B * capq * 8].view(torch.int32).view(B, capq)
    n = ws[B * capq * 8:].view(torch.int32)
    desc = a.struct()
    lib.srec_score_select_many_collect(_ct.addressof(desc), ptr(floor), capq, ptr(bv), ptr(bi), ptr(n), stream())
    return bv, bi, n, capq


def _order_many(bv, bi, n, capq, k):
    """(values [B, k], ids [B, k]) by (value descending, id ascending) from the buffers of _collect_many, unfilled slots
    (-inf, -1): the order kernel of csrc/select_many.hip, or - more than SREC_SELECT_MANY_SORT pairs in a row: ties without
    end - the two stable torch sorts of model.rerank / dist._merge_lists"""
    B, dev = bv.shape[0], bv.device
    if capq <= CONST['SREC_SELECT_MANY_SORT']:
        val = torch.empty(B, k, device=dev, dtype=torch.float32)
        idx = torch.empty(B, k, device=dev, dtype=torch.int32)
        lib.srec_score_select_many_order(B, capq, ptr(n), ptr(bv), ptr(bi), k, ptr(val), ptr(idx), stream())
        return val, idx
    filled = torch.arange(capq, device=dev)[None, :] < n[:, None]
    val = torch.where(filled, bv + 0.0, torch.full_like(bv, float('-inf')))          # (-0.0 canonicalised, as the kernel)
    idx = torch.where(filled, bi, torch.full_like(bi, -1))
    o = torch.argsort(torch.where(idx < 0, torch.full_like(idx, 2 ** 31 - 1), idx), dim=1, stable=True)
    val, idx = val.gather(1, o), idx.gather(1, o)
    o = torch.argsort(val, dim=1, descending=True, stable=True)[:, :k]
    return val.gather(1, o).contiguous(), idx.gather(1, o).contiguous()


def score_select_many(srs, table, cs, k, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
                      floor=None, cap=None):
    """(values fp32 [B,k] descending, item ids int32 [B,k]): score_select beyond 128 items - the k best rows of `table` per
    session under its score, its eligibility and its contract (arguments as score_select; ties towards the lower id; a
    session with fewer than k eligible rows ends in (-inf, -1) slots), 1 <= k <= 4096, no (B, V) tensor
    (csrc/select_many.hip).  The first stage of a two-stage set-up: model.rerank / score_items take lists of any length.
    floor=None (one device): score_cutoff(top_k=k) at temperature 1 over the very same operands finds every session's k-th
    best score and the number of rows at or above it, count; cap = int(count.max()) - ONE device-to-host read per call -
    sizes the buffer; one more pass over the table collects the (value, id) pairs at or above the floor (integer atomics
    hand out the slots: arrival decides where a pair sits, never which pairs are there), and one workgroup per session
    sorts its pairs in LDS by (value descending, id ascending).  The cutoff and the collect pass form the score through the
    same tile product, so exactly count pairs arrive; count exceeds k only by rows that tie with the k-th.
    floor [B] and cap given (a row shard: both from score_cutoff(top_k=k) over the WHOLE catalogue, cap = int(count.max())):
    no cutoff, this shard's rows are collected under the given floor and ordered; the lists of disjoint shards merge by
    (value, id) to the bits of the call over the whole table (dist.VocabParallel.select_many).  floor and cap come together.
    Tie overflow: more than 8192 pairs in a row (thousands of rows tie with a session's k-th: a table of identical rows) do
    not fit the order kernel; the buffer is then ordered by two stable torch sorts - slower, the same contract, never an error.
    An eligible row that merely scores -inf is treated as score_cutoff counts it: it is returned (value -inf, its own id,
    ahead of the unfilled slots) only when the floor is -inf, i.e. when the session has fewer than k eligible rows.  Values
    come back as s + 0.0 (-0.0 canonicalised, as score_cutoff compares).
    k, floor and cap are checked before any launch (ValueError, CPU tensors included).
    Measured at B 512, V 37 484, d 256 (profiles/select_many_timing.md): C = 1 - 1.40 / 1.43 / 1.48 ms
    at k = 256 / 1000 / 4096 (the top_k cutoff's six passes, 224 - 240 us for the collect pass, 20 - 72 us for the order
    kernel) against 0.62 - 0.65 ms for score_logp + torch.topk; C = 3 with a [4, V] bias and a 20-item dropped list - 3.61 -
    3.68 ms against 1.91 - 1.94 ms; at a shard of V 1 250 000 (C = 1) 33.5 - 33.7 ms against 14.8 ms.  The materialised route
    is 2.0 - 2.3x FASTER in every row; it allocates 77 - 100 MB (C = 1), 588 MB (C = 3) and 2.5 GB (the shard) per call
    where this route allocates 1 - 17 MB.  The route exists for the matrix it does not form, not for speed."""
    who = 'score_select_many'
    k = select_many_k(who, k)
    a = _served_args(who, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs.device
    if (floor is None) != (cap is None):
        raise ValueError('%s: floor and cap come together (both from score_cutoff(top_k=k) over the whole catalogue), got %s '
                         'without %s' % ((who,) + (('cap', 'floor') if floor is None else ('floor', 'cap'))))
    if cap is not None:
        cap = int(cap)
        if cap < 1:
            raise ValueError('%s: cap = %d; it is the largest count of score_cutoff(top_k=k), at least 1' % (who, cap))
    floor = _floor_arg(who, floor, B, dev)
    if B == 0:
        return torch.empty(0, k, device=dev, dtype=torch.float32), torch.empty(0, k, device=dev, dtype=torch.int32)
    if floor is None:
        floor, count, _, _ = score_cutoff(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group, top_k=k)
        cap = int(count.max())                              # the one device-to-host read
    if cap < 1 or a.V == 0:                                 # nothing eligible in any session / a shard without rows
        return (torch.full((B, k), float('-inf'), device=dev, dtype=torch.float32),
                torch.full((B, k), -1, device=dev, dtype=torch.int32))
    return _order_many(*_collect_many(a, floor, cap), k)


def diversify_scalars(who, k, diversity, M=None):
    """(k, diversity) as the library takes them, or ValueError in the words of `who`: k in 1 .. 128 (and <= M, the pool, when
    given: M itself in 1 .. 128), diversity a finite number >= 0.  No launch, no library call"""
    kmax = CONST['SREC_SELECT_MAXK']
    k = int(k)
    if M is not None and not 1 <= int(M) <= kmax:
        raise ValueError('%s: a pool of %d slots per session; csrc/diversify.hip takes between 1 and %d' % (who, M, kmax))
    if k < 1 or k > (kmax if M is None else int(M)):
        raise ValueError('%s: k = %d; csrc/diversify.hip picks between 1 and %s items per session'
                         % (who, k, '%d' % kmax if M is None else 'the pool\'s %d' % M))
    try:
        diversity = float(diversity)
    except (TypeError, ValueError):
        raise ValueError('%s: diversity must be a number, got %r' % (who, diversity)) from None
    if not (0.0 <= diversity <= 3.4e38):
        raise ValueError('%s: diversity = %r; it must be finite and >= 0' % (who, diversity))
    return k, diversity


def diversify(X, row, val, k, diversity, checked=False):
    """(val fp32 [B,k], pick int32 [B,k], mmr fp32 [B,k], ild fp32 [B]): the greedy MMR re-rank of a pool of M <= 128 slots
    per session (csrc/diversify.hip, one workgroup per session: no [B, M, d] gather, no [B, M, M] Gram matrix, no loop of
    launches).  Slot i of session b has the row X[row[b, i]] and the value val[b, i]; row < 0 is an unfilled slot.
      sim(i, j) = <X_i, X_j> / (max(|X_i|, 1e-12) max(|X_j|, 1e-12))  (a zero row: 0 to everything, never NaN)
      for t = 0 .. k-1: m_t(i) = val[i] - diversity * pen_t(i) over the filled slots not yet picked, pen_0 = 0, pen_t(i) =
      the maximum of sim(i, j) over the slots picked so far (raw, not clamped at 0); the pick is the largest m_t, ties to
      the lower slot.
    pick: the slot numbers in pick order, -1 once the filled slots run out; the returned val: val[pick] copied bit for bit,
    -inf in the tail; mmr: the winning m_t; ild: 1 - the mean of sim over the pairs of filled picks, 0 with fewer than two.
    diversity is finite and >= 0; 0 gives m_t = val[i] whatever the rows are (equal values: the first k filled slots in slot
    order).  A positive factor per row (the column scale cs) does not change sim, so none is taken.
    X: fp32 [n, d] (a row-strided view is taken as it is), d % 4 == 0, d <= 1024; row: [B, M] of any integer dtype;
    val: fp32 [B, M]; 1 <= k <= M <= 128.  Wrong shapes, dtypes and scalars raise ValueError before any launch, and - unless
    checked=True, the caller has looked - so does a row >= n (one aminmax, one device-to-host read).  The kernel itself
    treats a row >= n as unfilled and never dereferences it."""
    who = 'diversify'
    if X.dim() != 2 or X.dtype != torch.float32:
        raise ValueError('%s: X must be a 2-D fp32 tensor of rows, got %s %s' % (who, X.dtype, tuple(X.shape)))
    n, d = X.shape
    if d < 4 or d % 4 or d > 1024:
        raise ValueError('%s: rows of %d columns; csrc/diversify.hip takes d %% 4 == 0, d <= 1024' % (who, d))
    row, val = row.detach(), val.detach()
    if row.is_floating_point() or row.is_complex() or row.dtype == torch.bool or row.dim() != 2:
        raise ValueError('%s: row must be an integer tensor [B, M], got %s %s' % (who, row.dtype, tuple(row.shape)))
    if val.dtype != torch.float32 or val.shape != row.shape:
        raise ValueError('%s: val must be fp32 %s like row, got %s %s' % (who, tuple(row.shape), val.dtype, tuple(val.shape)))
    B, M = row.shape
    k, diversity = diversify_scalars(who, k, diversity, M)
    if not checked and B > 0:
        lo, hi = (int(x) for x in torch.aminmax(row))
        if hi >= n:
            raise ValueError('%s: row %d; X has %d rows (a negative row is an unfilled slot)' % (who, hi, n))
    X = _rows(X.detach())
    dev = X.device
    out_val = torch.empty(B, k, device=dev, dtype=torch.float32)
    pick = torch.empty(B, k, device=dev, dtype=torch.int32)
    mmr = torch.empty(B, k, device=dev, dtype=torch.float32)
    ild = torch.empty(B, device=dev, dtype=torch.float32)
    if B == 0:
        return out_val, pick, mmr, ild
    row = row.to(device=dev, dtype=torch.int32).contiguous()
    val = val.to(dev).contiguous()
    lib.srec_diversify(ptr(X), _ld(X), n, ptr(row), ptr(val), B, M, k, d, diversity, ptr(pick), ptr(out_val), ptr(mmr),
                       ptr(ild), stream())
    return out_val, pick, mmr, ild


# per-category caps on a served list: category int32 [num_items] (-1: the item has none), caps int32 [G], G (cap_rule builds it)
CapRule = namedtuple('CapRule', 'category caps G')


def _int_vector(who, what, x, device):
    """x (an integer tensor or sequence) as a 1-D integer tensor on `device` (None: where it is), ValueError otherwise"""
    try:
        x = torch.as_tensor(x, device=device).detach()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError('%s: %s must be an integer tensor or sequence' % (who, what)) from None
    if x.is_floating_point() or x.is_complex() or x.dtype == torch.bool or x.dim() != 1:
        raise ValueError('%s: %s must be a 1-D integer tensor or sequence, got %s %s' % (who, what, x.dtype, tuple(x.shape)))
    return x


def cap_rule(num_items, item_category, max_per_category, device=None):
    """CapRule(category int32 [num_items], caps int32 [G], G): the rule "at most caps[c] items of category c in a served list"
    as cap_select and the models' recommend_capped take it.  item_category: an integer tensor or sequence [num_items] over
    GLOBAL item ids with values in [-1, G), -1 = the item has no category and is never capped.  max_per_category: an int >= 0
    for every category (G = the largest category + 1, at least 1), or an integer tensor or sequence [G]; a cap of 0 means
    the category is never shown.  ValueError for a wrong length, a non-integer dtype, a category < -1 or >= G, a negative
    cap, and G > SREC_CAP_MAXG (the counters of csrc/cap_select.hip live in LDS).  Pure torch, at the price of ONE
    device-to-host read: a server builds the rule once and passes the record from then on."""
    who, gmax = 'cap_rule', CONST['SREC_CAP_MAXG']
    num_items = int(num_items)
    cat = _int_vector(who, 'item_category', item_category, device)
    if cat.numel() != num_items:
        raise ValueError('%s: item_category has %d entries for %d items' % (who, cat.numel(), num_items))
    cat = cat.to(torch.int64)
    one = isinstance(max_per_category, numbers.Integral) and not isinstance(max_per_category, bool)
    if one:
        caps = None
        if max_per_category < 0:
            raise ValueError('%s: max_per_category = %d; a cap is >= 0' % (who, max_per_category))
    elif isinstance(max_per_category, (bool, numbers.Number)):
        raise ValueError('%s: max_per_category must be an int or an integer tensor or sequence, got %r' % (who, max_per_category))
    else:
        caps = _int_vector(who, 'max_per_category', max_per_category, cat.device).to(torch.int64)
        if not 1 <= caps.numel() <= gmax:
            raise ValueError('%s: %d categories; csrc/cap_select.hip counts between 1 and %d' % (who, caps.numel(), gmax))
    seen = [cat.min(), cat.max()] if num_items > 0 else [cat.new_tensor(-1)] * 2
    lo, hi, cap_lo = torch.stack(seen + [cat.new_tensor(0) if one else caps.min()]).tolist()     # the one device-to-host read
    if lo < -1:
        raise ValueError('%s: category %d; categories are in [0, G), or -1 for an item without one' % (who, lo))
    if cap_lo < 0:
        raise ValueError('%s: max_per_category holds the cap %d; a cap is >= 0' % (who, cap_lo))
    if one:
        G = max(hi + 1, 1)
        if G > gmax:
            raise ValueError('%s: %d categories; csrc/cap_select.hip counts at most %d' % (who, G, gmax))
        caps = torch.full((G,), min(int(max_per_category), 2 ** 31 - 1), dtype=torch.int64, device=cat.device)
    G = caps.numel()
    if hi >= G:
        raise ValueError('%s: category %d; max_per_category names %d categories' % (who, hi, G))
    return CapRule(cat.to(torch.int32).contiguous(), caps.clamp(max=2 ** 31 - 1).to(torch.int32).contiguous(), G)


def cap_rule_check(who, rule):
    """rule as a CapRule whose tensors agree with each other, or ValueError in the words of `who`.  No device read: the
    VALUES are cap_rule's business (and the kernel never indexes out of range whatever they are)"""
    if not isinstance(rule, CapRule):
        raise ValueError('%s: rule must be the record ops.cap_rule returns, got %s' % (who, type(rule).__name__))
    cat, caps, G = rule
    if not (torch.is_tensor(cat) and cat.dtype == torch.int32 and cat.dim() == 1 and torch.is_tensor(caps)
            and caps.dtype == torch.int32 and caps.dim() == 1 and isinstance(G, int) and caps.numel() == G
            and 1 <= G <= CONST['SREC_CAP_MAXG']):
        raise ValueError('%s: rule must hold category int32 [num_items], caps int32 [G] and 1 <= G <= %d (ops.cap_rule builds it)'
                         % (who, CONST['SREC_CAP_MAXG']))
    return rule


def cap_k(who, k, P=None):
    """k of a capped list as the library takes it, or ValueError in the words of `who`: 1 .. SREC_CAP_MAXP (and <= P, the
    pool, when given: P itself in 1 .. SREC_CAP_MAXP)"""
    pmax = CONST['SREC_CAP_MAXP']
    k = int(k)
    if P is not None and not 1 <= int(P) <= pmax:
        raise ValueError('%s: a pool of %d slots per session; csrc/cap_select.hip takes between 1 and %d' % (who, P, pmax))
    if k < 1 or k > (pmax if P is None else int(P)):
        raise ValueError('%s: k = %d; csrc/cap_select.hip keeps between 1 and %s items per session'
                         % (who, k, '%d' % pmax if P is None else 'the pool\'s %d' % P))
    return k


def cap_select(ids, val, rule, k, checked=False):
    """(val fp32 [B,k], pick int32 [B,k], kept int32 [B], scanned int32 [B]): the first k slots of an ORDERED pool per session
    that respect the per-category caps of `rule` (cap_rule's record) - csrc/cap_select.hip, one workgroup per session, integer
    logic only: no [B, P] host read, no loop per session.  Slot i of session b holds the item ids[b, i] and the value
    val[b, i] - what score_select / score_select_many return; ids < 0 is an unfilled slot.
      c_i = rule.category[ids[b, i]]; -1: the item has no category and is always accepted;
      otherwise the slot is accepted iff fewer than rule.caps[c_i] EARLIER filled slots of the session have category c_i
      (= fewer than that many earlier accepted ones: the greedy over a partition matroid, which is the optimum).
    Duplicate ids each count.  pick: the slot numbers of the first k accepted slots in slot order, -1 once they run out; the
    returned val: val[pick] copied bit for bit, -inf in the tail; kept = min(k, accepted); scanned: the pool slots consumed -
    the index after the k-th accepted slot, or P with fewer than k (slots past it play no part in the result).
    ids: [B, P] of any integer dtype; val: fp32 [B, P] (views are taken as they are: made contiguous here);
    1 <= k <= P <= 4096; ids, val and the rule's tensors on ONE device (nothing is moved).  Wrong shapes, dtypes, devices, k
    and rule raise ValueError before any launch, and - unless checked=True, the caller vouches - so does an id >= num_items
    (one max, one device-to-host read).  Under checked=True an id outside
    [0, num_items) is an unfilled slot; the kernel never dereferences it."""
    who = 'cap_select'
    rule = cap_rule_check(who, rule)
    ids, val = ids.detach(), val.detach()
    if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() != 2:
        raise ValueError('%s: ids must be an integer tensor [B, P], got %s %s' % (who, ids.dtype, tuple(ids.shape)))
    if val.dtype != torch.float32 or val.shape != ids.shape:
        raise ValueError('%s: val must be fp32 %s like ids, got %s %s' % (who, tuple(ids.shape), val.dtype, tuple(val.shape)))
    B, P = ids.shape
    k = cap_k(who, k, P)
    n = rule.category.numel()
    dev = rule.category.device
    if not (ids.device == val.device == dev == rule.caps.device):
        raise ValueError('%s: ids (%s), val (%s) and the rule (%s, %s) must be on one device (ops.cap_rule(..., device=) places '
                         'the rule)' % (who, ids.device, val.device, dev, rule.caps.device))
    if not checked and B > 0:
        hi = int(ids.max())                                         # the one device-to-host read
        if hi >= n:
            raise ValueError('%s: item id %d; the rule covers %d items (a negative id is an unfilled slot)' % (who, hi, n))
    if ids.dtype != torch.int32:                                    # (an id beyond int32 must not wrap into the catalogue)
        ids = torch.where((ids < 0) | (ids >= n), torch.full_like(ids, -1), ids)
    ids = ids.to(torch.int32).contiguous()
    val = val.contiguous()
    out_val = torch.empty(B, k, device=dev, dtype=torch.float32)
    pick = torch.empty(B, k, device=dev, dtype=torch.int32)
    kept = torch.empty(B, device=dev, dtype=torch.int32)
    scanned = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return out_val, pick, kept, scanned
    lib.srec_cap_select(ptr(ids), ptr(val), B, P, k, ptr(rule.category), n, ptr(rule.caps), rule.G, ptr(pick), ptr(out_val),
                        ptr(kept), ptr(scanned), stream())
    return out_val, pick, kept, scanned


# per-session hide / boost lists: items int32 [rows, M] (-1: padding), bias fp32 [rows, M] or None (every listed item is hidden),
# M; rows = the sessions, or 1 for a list shared by all of them while their number is not known (personal_lists builds it)
PersonalLists = namedtuple('PersonalLists', 'items bias M')


def _padded_rows(who, what, x, pad, dtype):
    """(tensor [rows, M] or [M], row lengths or None) of x - a tensor, a flat sequence or a sequence of sequences of unequal
    length, short rows padded with `pad` (the lengths are then given); ValueError in the words of `who`"""
    if torch.is_tensor(x):
        return x.detach(), None
    try:
        rows = list(x)
        if rows and all(isinstance(r, (list, tuple)) for r in rows):
            M = max(len(r) for r in rows)
            return torch.tensor([list(r) + [pad] * (M - len(r)) for r in rows], dtype=dtype).view(len(rows), M), [len(r) for r in rows]
        return torch.as_tensor(rows), None
    except (TypeError, ValueError, RuntimeError, OverflowError):
        raise ValueError('%s: %s must be a tensor [B, M] or [M], or a list of per-session lists' % (who, what)) from None


def personal_lists(who, items, bias, B, num_items, device):
    """PersonalLists(items int32 [B, M], bias fp32 [B, M] or None, M) on `device`: the per-session lists personal_merge and the
    models' recommend_personal take.  items: an integer tensor [B, M], or [M] shared by all sessions, -1 = padding - or Python
    lists, one per session, of unequal length (padded here).  bias: None (every listed item is hidden) or floating, shaped
    like items (lists: as long as the items' lists), the number ADDED to the item's score; -inf hides the item; the entry of
    a padding slot is not looked at.  B: the sessions, or None while their number is not known - a shared list then stays one
    row.  Checked before any launch, with ONE device-to-host read: every id in [-1, num_items), no id twice in a row, bias
    without NaN and +inf; and 1 <= M <= SREC_PERSONAL_MAXM.  ValueError in the words of `who`."""
    mmax = CONST['SREC_PERSONAL_MAXM']
    it, lens = _padded_rows(who, 'personal_items', items, -1, torch.int64)
    if it.is_floating_point() or it.is_complex() or it.dtype == torch.bool or it.dim() not in (1, 2):
        raise ValueError('%s: personal_items must be an integer tensor [B, M] or [M], got %s %s' % (who, it.dtype, tuple(it.shape)))
    M = it.shape[-1]
    if not 1 <= M <= mmax:
        raise ValueError('%s: %d listed items per session; between 1 and %d are merged in one call' % (who, M, mmax))
    it = it.reshape(-1, M)
    if B is not None and it.shape[0] not in (1, int(B)):
        raise ValueError('%s: personal_items for %d sessions, the batch has %d' % (who, it.shape[0], B))
    bs = None
    if bias is not None:
        bs, blens = _padded_rows(who, 'personal_bias', bias, 0.0, torch.float32)
        if blens is not None and blens != (lens if lens is not None else [M] * len(blens)):
            raise ValueError('%s: the lists of personal_bias must be as long as those of personal_items' % who)
        if not bs.is_floating_point() or bs.numel() != it.numel() or bs.shape[-1] != M:
            raise ValueError('%s: personal_bias must be a floating tensor %s like personal_items, got %s %s'
                             % (who, tuple(it.shape), bs.dtype, tuple(bs.shape)))
        bs = bs.reshape(-1, M).to(device=device, dtype=torch.float32)
    it = it.to(device=device, dtype=torch.int64)
    if it.numel() > 0:
        rows = it.sort(dim=1).values
        flags = [it.min(), it.max(), ((rows[:, 1:] == rows[:, :-1]) & (rows[:, 1:] >= 0)).any().to(torch.int64)]
        if bs is not None:
            flags.append(((torch.isnan(bs) | (bs == float('inf'))) & (it >= 0)).any().to(torch.int64))
        lo, hi, dup, *bad = torch.stack(flags).tolist()             # the one device-to-host read
        if lo < -1 or hi >= int(num_items):
            raise ValueError('%s: listed item id %d; ids are in [0, %d), or -1 for a padding slot'
                             % (who, lo if lo < -1 else hi, num_items))
        if dup:
            raise ValueError('%s: an item id appears twice in a session\'s list; every id at most once per session' % who)
        if bad and bad[0]:
            raise ValueError('%s: personal_bias holds NaN or +inf; values are finite, or -inf to hide the item' % who)
    if B is not None and it.shape[0] != int(B):
        it = it.expand(int(B), M)
        bs = None if bs is None else bs.expand(int(B), M)
    return PersonalLists(it.to(torch.int32).contiguous(), None if bs is None else bs.contiguous(), M)


def personal_k(who, k, M):
    """k of a personalised list as recommend_personal takes it, or ValueError in the words of `who`: 1 <= k and k + M <=
    SREC_CAP_MAXP (the pool that is always complete holds k + M items)"""
    pmax = CONST['SREC_CAP_MAXP']
    k = int(k)
    if k < 1 or k + int(M) > pmax:
        raise ValueError('%s: k = %d with %d listed items per session; k >= 1 and k + the list\'s length <= %d (recommend_many()\'s '
                         'limit: the pool that is always complete holds both)' % (who, k, M, pmax))
    return k


def personal_merge(pool_ids, pool_val, items, base, bias, k, checked=False):
    """(val fp32 [B,k], ids int32 [B,k], src int32 [B,k], hit int32 [B], kept int32 [B]): the first k items per session of an
    ORDERED pool after a sparse list of items changed its scores - csrc/personal.hip, one workgroup per session, no [B, V] bias
    and no catalogue pass.  Pool slot i of session b holds the item pool_ids[b, i] and the value pool_val[b, i] - what
    score_select / score_select_many return; ids < 0 is an unfilled slot.  List slot j holds items[b, j] (-1: padding), its
    score base[b, j] - what score_items returns for it - and bias[b, j]; its new value is t = base + bias (one fp32 add), and
    bias=None hides every listed item.
      a pool slot SURVIVES iff its id is in no filled list slot; hit = the filled pool slots that do not;
      a listed item is a CANDIDATE iff t > -inf (a -inf base - seen, filtered - stays out whatever the bias);
      the output is the first k of survivors and candidates by (value descending, id ascending): val (the pool's bits, or t),
      ids, src (pool slot i, or P + j for list slot j), the tail (-inf, -1, -1); kept = the filled output slots.
    With hit <= P - k, or the pool's last slot unfilled, that is the exact top-k of the adjusted catalogue.
    pool_ids: [B, P] and items: [B, M] of any integer dtype (in a wider dtype an id of 2^31 - 1 or more is an unfilled slot: no
    catalogue of int32 size holds it); pool_val, base: fp32 like them; bias: floating like items, or None (views are taken as
    they are: made contiguous here); 1 <= P <= 4096, 1 <= M <= 1024, 1 <= k <= 4096; everything on ONE device (nothing is moved).
    Wrong shapes, dtypes, devices and k raise ValueError before any launch, and - unless checked=True, the caller vouches - so
    does an id that stands twice in a row of items (ONE device-to-host read).  Under checked=True the first slot of a repeated
    id wins and the later ones are ignored."""
    who = 'personal_merge'
    pmax, mmax = CONST['SREC_CAP_MAXP'], CONST['SREC_PERSONAL_MAXM']
    pool_ids, pool_val, items, base = pool_ids.detach(), pool_val.detach(), items.detach(), base.detach()
    for what, t in (('pool_ids', pool_ids), ('items', items)):
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or t.dim() != 2:
            raise ValueError('%s: %s must be an integer tensor [B, %s], got %s %s'
                             % (who, what, 'P' if what == 'pool_ids' else 'M', t.dtype, tuple(t.shape)))
    if pool_val.dtype != torch.float32 or pool_val.shape != pool_ids.shape:
        raise ValueError('%s: pool_val must be fp32 %s like pool_ids, got %s %s'
                         % (who, tuple(pool_ids.shape), pool_val.dtype, tuple(pool_val.shape)))
    if base.dtype != torch.float32 or base.shape != items.shape:
        raise ValueError('%s: base must be fp32 %s like items, got %s %s' % (who, tuple(items.shape), base.dtype, tuple(base.shape)))
    if bias is not None:
        bias = bias.detach()
        if not bias.is_floating_point() or bias.shape != items.shape:
            raise ValueError('%s: bias must be a floating tensor %s like items (or None: hide them), got %s %s'
                             % (who, tuple(items.shape), bias.dtype, tuple(bias.shape)))
    (B, P), M = pool_ids.shape, items.shape[1]
    if items.shape[0] != B:
        raise ValueError('%s: items for %d sessions, the pool has %d' % (who, items.shape[0], B))
    if not 1 <= P <= pmax:
        raise ValueError('%s: a pool of %d slots per session; csrc/personal.hip takes between 1 and %d' % (who, P, pmax))
    if not 1 <= M <= mmax:
        raise ValueError('%s: %d listed items per session; csrc/personal.hip takes between 1 and %d' % (who, M, mmax))
    k = int(k)
    if not 1 <= k <= pmax:
        raise ValueError('%s: k = %d; csrc/personal.hip returns between 1 and %d items per session' % (who, k, pmax))
    dev = pool_ids.device
    if not (pool_val.device == items.device == base.device == dev) or (bias is not None and bias.device != dev):
        raise ValueError('%s: pool_ids (%s), pool_val (%s), items (%s), base (%s) and bias must be on one device'
                         % (who, dev, pool_val.device, items.device, base.device))
    if not checked and B > 0:
        rows = items.sort(dim=1).values
        if bool(((rows[:, 1:] == rows[:, :-1]) & (rows[:, 1:] >= 0)).any()):       # the one device-to-host read
            raise ValueError('%s: an item id appears twice in a row of items; every id at most once per session (checked=True: '
                             'the first slot wins)' % who)

    def int32(t):                                                   # (an id beyond int32 must not wrap into the catalogue)
        if t.dtype == torch.int64:
            t = torch.where((t < 0) | (t >= 2 ** 31 - 1), torch.full_like(t, -1), t)
        return t.to(torch.int32).contiguous()
    pool_ids, items = int32(pool_ids), int32(items)
    pool_val, base = pool_val.contiguous(), base.contiguous()
    if bias is not None:
        bias = bias.to(torch.float32).contiguous()
    val = torch.empty(B, k, device=dev, dtype=torch.float32)
    ids = torch.empty(B, k, device=dev, dtype=torch.int32)
    src = torch.empty(B, k, device=dev, dtype=torch.int32)
    hit = torch.empty(B, device=dev, dtype=torch.int32)
    kept = torch.empty(B, device=dev, dtype=torch.int32)
    if B == 0:
        return val, ids, src, hit, kept
    lib.srec_personal_merge(ptr(pool_ids), ptr(pool_val), B, P, ptr(items), ptr(base), ptr(bias), M, k, ptr(ids), ptr(val),
                            ptr(src), ptr(hit), ptr(kept), stream())
    return val, ids, src, hit, kept


def calibrate_scalars(who, k, weight, alpha, M=None):
    """(k, weight, alpha) as the library takes them, or ValueError in the words of `who`: k in 1 .. 128 (and <= M, the pool,
    when given: M itself in 1 .. 128), weight a number in [0, 1], alpha (the smoothing of the calibration term) in (0, 1).
    weight and alpha come back ROUNDED TO fp32, as the kernel receives them.  No launch, no library call"""
    kmax = CONST['SREC_SELECT_MAXK']
    k = int(k)
    if M is not None and not 1 <= int(M) <= kmax:
        raise ValueError('%s: a pool of %d slots per session; csrc/calibrate.hip takes between 1 and %d' % (who, M, kmax))
    if k < 1 or k > (kmax if M is None else int(M)):
        raise ValueError('%s: k = %d; csrc/calibrate.hip picks between 1 and %s items per session'
                         % (who, k, '%d' % kmax if M is None else 'the pool\'s %d' % M))
    try:
        weight, alpha = float(weight), float(alpha)
    except (TypeError, ValueError):
        raise ValueError('%s: weight and alpha must be numbers, got %r and %r' % (who, weight, alpha)) from None
    if not 0.0 <= weight <= 1.0:
        raise ValueError('%s: weight = %r; it must be in [0, 1]' % (who, weight))
    weight, alpha = _ct.c_float(weight).value, _ct.c_float(alpha).value
    if not 0.0 < alpha < 1.0:
        raise ValueError('%s: alpha = %r; it must be in (0, 1) (as fp32)' % (who, alpha))
    return k, weight, alpha


def calibrate(ids, val, category, k, weight, target_cat=None, target_w=None, alpha=0.01, checked=False):
    """(val fp32 [B,k], pick int32 [B,k], obj fp32 [B,k], kl fp32 [B]): the greedy CALIBRATED re-rank of a pool of M <= 128
    slots per session (Steck, "Calibrated Recommendations", RecSys 2018; csrc/calibrate.hip, one workgroup per session: no
    loop of launches, no [B, M, categories] temporaries).  Slot i of session b holds the item ids[b, i] and the value
    val[b, i] - what score_select returns; ids < 0 is an unfilled slot.  c_i = category[ids[b, i]], < 0: the item has none.
      target: the pairs (target_cat[b, j], target_w[b, j]) of a CATEGORY id and a weight, T <= 128 per session; a category
      < 0 or a weight <= 0 is an empty pair, duplicates add up.  P_c = the weights of category c summed, S = {c: P_c > 0},
      p_c = P_c / sum_S P_c.  No pair at all (or target_cat = target_w = None): no target, the calibration term is 0.
      state: n_c picks of category c, N picks with any category >= 0 (in S or not);
      KL(n, N) = sum_{c in S} p_c log(p_c / ((1 - alpha) n_c / max(N, 1) + alpha p_c))
      for t = 0 .. k-1: m_t(i) = (1 - weight) val[i] - weight KL(state with slot i added) over the filled slots not yet
      picked; the pick is the largest m_t, ties to the lower slot.  weight 0: m_t = val[i]; val[i] = -inf: m_t = -inf.
    pick: the slot numbers in pick order, -1 once the filled slots run out; the returned val: val[pick] copied bit for bit,
    -inf in the tail; obj: the winning m_t; kl: KL of the final picks, 0 without a target.  The term, the sums and m_t are
    double inside the kernel, weight and alpha fp32 (calibrate_scalars returns the rounded values).
    ids: [B, M] of any integer dtype; val: fp32 [B, M] (views are made contiguous here); category: int32 [num_items];
    target_cat: [B, T] of any integer dtype with target_w floating [B, T], or both None; 1 <= k <= M <= 128; everything on
    ONE device (nothing is moved).  Wrong shapes, dtypes, devices and scalars raise ValueError before any launch, and -
    unless checked=True, the caller vouches - so do an id >= num_items and a weight that is NaN, infinite or negative (ONE
    device-to-host read for both).  Under checked=True an id outside [0, num_items) is an unfilled slot; the kernel never
    dereferences it.  A category id beyond int32 is mapped to an empty pair."""
    who = 'calibrate'
    if not (torch.is_tensor(category) and category.dtype == torch.int32 and category.dim() == 1):
        raise ValueError('%s: category must be an int32 tensor [num_items]' % who)
    ids, val = ids.detach(), val.detach()
    if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.dim() != 2:
        raise ValueError('%s: ids must be an integer tensor [B, M], got %s %s' % (who, ids.dtype, tuple(ids.shape)))
    if val.dtype != torch.float32 or val.shape != ids.shape:
        raise ValueError('%s: val must be fp32 %s like ids, got %s %s' % (who, tuple(ids.shape), val.dtype, tuple(val.shape)))
    B, M = ids.shape
    k, weight, alpha = calibrate_scalars(who, k, weight, alpha, M)
    n, dev = category.numel(), category.device
    if (target_cat is None) != (target_w is None):
        raise ValueError('%s: target_cat and target_w go together' % who)
    T = 0
    if target_cat is not None:
        tc, tw = target_cat.detach(), target_w.detach()
        if tc.is_floating_point() or tc.is_complex() or tc.dtype == torch.bool or tc.dim() != 2 or tc.shape[0] != B:
            raise ValueError('%s: target_cat must be an integer tensor [%d, T], got %s %s' % (who, B, tc.dtype, tuple(tc.shape)))
        if not tw.is_floating_point() or tw.shape != tc.shape:
            raise ValueError('%s: target_w must be a floating tensor %s like target_cat, got %s %s'
                             % (who, tuple(tc.shape), tw.dtype, tuple(tw.shape)))
        T = tc.shape[1]
        if T > CONST['SREC_CALIB_MAXT']:
            raise ValueError('%s: %d target pairs per session; csrc/calibrate.hip takes at most %d' % (who, T, CONST['SREC_CALIB_MAXT']))
        if not (tc.device == tw.device == dev):
            raise ValueError('%s: the target (%s, %s) must be on the device of category (%s)' % (who, tc.device, tw.device, dev))
        tw = tw.to(torch.float32)                                   # (the weights the kernel sees are the ones checked)
    if not (ids.device == val.device == dev):
        raise ValueError('%s: ids (%s), val (%s) and category (%s) must be on one device' % (who, ids.device, val.device, dev))
    if not checked and B > 0:
        flags = [ids.max() >= n]
        if T > 0:
            flags.append(~(torch.isfinite(tw) & (tw >= 0)).all())
        bad = torch.stack(flags).tolist()                           # the one device-to-host read
        if bad[0]:
            raise ValueError('%s: an item id >= %d, the items category covers (a negative id is an unfilled slot)' % (who, n))
        if len(bad) > 1 and bad[1]:
            raise ValueError('%s: target_w holds a NaN, infinite or negative weight' % who)
    if ids.dtype != torch.int32:                                    # (an id beyond int32 must not wrap into the catalogue)
        ids = torch.where((ids < 0) | (ids >= n), torch.full_like(ids, -1), ids)
    ids = ids.to(torch.int32).contiguous()
    val = val.contiguous()
    if T > 0:
        if tc.dtype != torch.int32:
            tc = torch.where((tc < 0) | (tc > 2 ** 31 - 1), torch.full_like(tc, -1), tc)
        tc = tc.to(torch.int32).contiguous()
        tw = tw.contiguous()
    out_val = torch.empty(B, k, device=dev, dtype=torch.float32)
    pick = torch.empty(B, k, device=dev, dtype=torch.int32)
    obj = torch.empty(B, k, device=dev, dtype=torch.float32)
    kl = torch.empty(B, device=dev, dtype=torch.float32)
    if B == 0:
        return out_val, pick, obj, kl
    lib.srec_calibrate(ptr(ids), ptr(val), B, M, k, ptr(category), n, ptr(tc) if T > 0 else None, ptr(tw) if T > 0 else None, T,
                       weight, alpha, ptr(pick), ptr(out_val), ptr(obj), ptr(kl), stream())
    return out_val, pick, obj, kl


def _logp_cols(sr, ld_sr, table, cs, lse):
    """[B, V] log-probabilities z[b, v] - lse[b] of the rows of `table` (fp32): a view of a buffer whose rows are padded to
    a multiple of 4 columns"""
    B, d = sr.shape
    V = table.shape[0]
    ldp = (V + 3) & ~3
    out = torch.empty(B, ldp, device=sr.device, dtype=torch.float32)
    lib.srec_score_logp(ptr(sr), ld_sr, ptr(table), table.stride(0), ptr(cs), ptr(lse), B, V, d, None, ptr(out), ldp, stream())
    return out[:, :V]


class ScoreLogProb(torch.autograd.Function):
    """(B,V) log-probabilities - the tensor the reference models' forward() returns (compat /
    evaluation path).  Backward materialises d z (B,V) and runs two MFMA GEMMs."""

    @staticmethod
    def forward(ctx, sr, table, cs, ws, cs_inv_scale):
        sr = _rows(sr)
        B, d = sr.shape
        V = table.shape[0]
        lse, lossvec, loss = _ce_outputs(B, sr.device)
        zeros = torch.zeros(B, device=sr.device, dtype=torch.int32)
        lib.srec_score_ce_fwd(ptr(sr), _ld(sr), ptr(table), table.stride(0), ptr(cs), ptr(zeros), B, V, d, None,
                              ptr(ws.stats), ptr(ws.lab_logit), ptr(lse), ptr(lossvec), ptr(loss), stream())
        logp = _logp_cols(sr, _ld(sr), table, cs, lse)
        ctx.save_for_backward(sr, table, cs, logp)
        ctx.cs_inv_scale = cs_inv_scale
        return logp

    @staticmethod
    def backward(ctx, g):
        sr, table, cs, logp = ctx.saved_tensors
        dz = g - torch.exp(logp) * g.sum(dim=1, keepdim=True)
        if cs is not None:
            dz = dz * cs.unsqueeze(0)
        V, d = table.shape
        ldp = (V + 3) & ~3
        dzp = torch.zeros(dz.shape[0], ldp, device=dz.device, dtype=torch.float32)
        dzp[:, :V] = dz
        tablep = table if ldp == V else _pad_rows(table, ldp)
        dsr = torch.empty_like(sr)
        gemm_nn(dzp, tablep, dsr)
        dEp = torch.empty(ldp, d, device=dz.device, dtype=torch.float32)
        gemm_tn(dzp, sr, dEp)
        dE = dEp[:V]
        finish_table_grad(table, cs, ctx.cs_inv_scale, dE, None)
        return dsr, dE, None, None, None


def _pad_rows(t, n):
    out = torch.zeros(n, t.shape[1], device=t.device, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def score_logp(sr, table, cs, ws, cs_inv_scale=1.0):
    return ScoreLogProb.apply(sr, table, cs, ws, cs_inv_scale)


# ---- ensembles: the served score over several tables in one pass (csrc/ensemble.hip) ------------------------------------

_ServedMulti = ENS_STRUCTS['srec_served_multi']    # bound from include/srec_ens.h (_lib.parse_structs), never retyped
_ENS_MAXCOMP = ENS_CONST['SREC_ENS_MAXCOMP']
_ENS_WS = {}           # the scratch of ens_select / ens_ahead: kinds 'ens_select', 'ens_ahead', beside _BYTE_WS, not in it
_LISTED_TOO_MANY['ens_select'] = 'ens_select: %d listed items per session; csrc/ensemble.hip takes at most 64'
_LISTED_TOO_MANY['ens_ahead'] = 'ens_ahead: %d listed items per session; csrc/ensemble.hip takes at most 64'


class EnsArgs(namedtuple('EnsArgs', 'srs tables css ds C off_ex off_in listed L listed_mode id_lo B V bias ld_bias group G')):
    """The operands of the multi-table served score as ens_select / ens_ahead launch with them: per component the session
    vectors [B, d_c], the table [V, d_c] and the column scale (or None), then the shared members of srec_served_multi
    (include/srec_ens.h) - the record owns what the pointers will name."""
    __slots__ = ()

    def struct(self):
        """the host srec_served_multi of one library call (keep it, and this record, alive across the call).  ptr(): a CPU
        tensor raises here, after every argument check"""
        s = _ServedMulti()
        for c in range(self.C):
            s.sr[c], s.ld_sr[c] = ptr(self.srs[c]), _ld(self.srs[c])
            s.E[c], s.ld_e[c] = ptr(self.tables[c]), _ld(self.tables[c])
            s.cs[c], s.d[c] = ptr(self.css[c]), self.ds[c]
        s.C = self.C
        s.off_ex, s.off_in, s.listed, s.L = ptr(self.off_ex), ptr(self.off_in), ptr(self.listed), self.L
        s.listed_mode, s.id_lo, s.B, s.V = self.listed_mode, self.id_lo, self.B, self.V
        s.bias, s.ld_bias, s.group, s.G = ptr(self.bias), self.ld_bias, ptr(self.group), self.G
        return s


def _ens_args(who, comps, off_ex, off_in, listed, drop_listed, id_lo, bias, group):
    """The argument conventions of ens_select / ens_ahead as one EnsArgs, errors (ValueError) in the words of `who`, naming the
    offender.  comps: a sequence of 1 .. 8 (sr [B, d_c], table [V, d_c], cs [V] or None), all fp32 on one device, B and V
    equal across the components, d_c % 4 == 0 and <= 1024; off_ex / off_in: [C, B] or None (= 0; off_in is ignored under
    drop_listed); listed: [B, L] item ids, L <= 64, empty or None = no list; bias / group as _bias_args.  Pure torch (no
    launch, no library call): it checks CPU tensors as well."""
    try:
        comps = [tuple(c) for c in comps]
    except TypeError:
        raise ValueError('%s: comps must be a sequence of (sr, table, cs) triples' % who) from None
    C = len(comps)
    if not 1 <= C <= _ENS_MAXCOMP:
        raise ValueError('%s: %d components; csrc/ensemble.hip mixes between 1 and %d' % (who, C, _ENS_MAXCOMP))
    srs, tables, css, ds = [], [], [], []
    B = V = dev = None
    for c, comp in enumerate(comps):
        if len(comp) != 3:
            raise ValueError('%s: component %d is not a (sr, table, cs) triple' % (who, c))
        sr, table, cs = comp
        for name, t, dims in (('sr', sr, 2), ('table', table, 2), ('cs', cs, 1)):
            if t is None and name == 'cs':
                continue
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != dims:
                raise ValueError('%s: component %d: %s must be a float32 tensor of %d dimensions, got %s' % (
                    who, c, name, dims, '%s %s' % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
            if dev is None:
                dev = t.device
            if t.device != dev:
                raise ValueError('%s: component %d: %s is on %s, component 0 on %s' % (who, c, name, t.device, dev))
        if B is None:
            B, V = sr.shape[0], table.shape[0]
        if sr.shape[0] != B:
            raise ValueError('%s: component %d has %d sessions, component 0 has %d' % (who, c, sr.shape[0], B))
        if table.shape[0] != V:
            raise ValueError('%s: component %d scores %d items, component 0 scores %d' % (who, c, table.shape[0], V))
        d = sr.shape[1]
        if table.shape[1] != d:
            raise ValueError('%s: component %d: sr has %d columns, its table %d' % (who, c, d, table.shape[1]))
        if d < 4 or d % 4 or d > 1024:
            raise ValueError('%s: component %d: width %d; csrc/ensemble.hip takes multiples of 4 up to 1024' % (who, c, d))
        if cs is not None and cs.shape[0] != V:
            raise ValueError('%s: component %d: cs has %d entries for %d items' % (who, c, cs.shape[0], V))
        srs.append(_rows(sr.detach()))
        tables.append(_rows(table.detach()))
        css.append(None if cs is None else cs.detach().contiguous())
        ds.append(d)

    def offs(name, o):
        if o is None:
            return None
        o = torch.as_tensor(o).detach()
        if tuple(o.shape) != (C, B):
            raise ValueError('%s: %s must be [%d, %d] (components, sessions), got %s' % (who, name, C, B, tuple(o.shape)))
        if o.dtype != torch.float32 or o.device != dev:
            raise ValueError('%s: %s must be float32 on %s, got %s on %s' % (who, name, dev, o.dtype, o.device))
        return o.contiguous()
    off_ex, off_in = offs('off_ex', off_ex), offs('off_in', None if drop_listed else off_in)
    L = 0
    if listed is not None and listed.numel() > 0:
        if listed.is_floating_point() or listed.dim() != 2 or listed.shape[0] != B:
            raise ValueError('%s: listed must hold [%d, L] integer item ids, got %s %s' % (who, B, listed.dtype, tuple(listed.shape)))
        listed = listed.detach().to(torch.int32).contiguous()
        L = listed.shape[1]
        if L > _LISTED_MAX:
            raise ValueError(_LISTED_TOO_MANY[who] % L)
    else:
        listed = None
    mode = CONST['SREC_LISTED_DROP'] if drop_listed else CONST['SREC_LISTED_SCORE']
    return EnsArgs(srs, tables, css, ds, C, off_ex, off_in, listed, L, mode, int(id_lo), B, V, *_bias_args(who, bias, group, B, V))


def ens_select(comps, k, off_ex, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None):
    """(values fp32 [B,k] descending, item ids int32 [B,k]): score_select over SEVERAL tables - the k best items per session
    under s[b,v] = logsumexp_c(cs_c[v] <sr_c[b], E_c[v]> + off[c,b]) (+ bias[group[b], v]), every component with its own table,
    width and column scale: the served score of a probability-averaged ensemble, log w_m folded into the member's offsets - no
    (B, V) matrix per member, k <= 128 (csrc/ensemble.hip: one pass, the components folded into a running log-sum-exp).
    comps: a sequence of 1 .. 8 (sr [B, d_c], table [V, d_c], cs [V] or None), fp32 on one device, equal B and V; off_ex /
    off_in [C, B] or None (= 0); listed / drop_listed / id_lo / bias / group, ties, (-inf, -1) slots and eligibility as
    score_select.  One component gives score_select's values and ids, bit for bit.  No floor, no sampling, no bf16; a wrong
    argument raises ValueError before anything is launched (_ens_args).
    Measured at B 512, V 37 484, d 256 (profiles/ensemble_timing.md): two single-soft-max members at k = 20
    take 1 102 us against 1 406 us for one (B, V) log-prob matrix per component + logsumexp + topk, and 1 + 3 components 1 450
    against 2 325 us (k = 100: 1 490 against 2 322 us); with two members at k = 100 this route LOSES to the materialised one
    (1 700 against 1 409 us: torch.topk does not grow with k, the running lists do) - materialise there if memory allows."""
    k = int(k)
    if k < 1 or k > CONST['SREC_SELECT_MAXK']:
        raise ValueError('ens_select: k = %d; the selection kernel of csrc/ensemble.hip keeps between 1 and %d items per '
                         'session' % (k, CONST['SREC_SELECT_MAXK']))
    a = _ens_args('ens_select', comps, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs[0].device
    val = torch.empty(B, k, device=dev, dtype=torch.float32)
    idx = torch.empty(B, k, device=dev, dtype=torch.int32)
    if B == 0:
        return val, idx
    ws = _scratch('ens_select', dev, lib.srec_ens_select_ws, B, a.V, max(a.ds), a.C, a.L, k, cache=_ENS_WS)
    desc = a.struct()
    lib.srec_ens_select(_ct.addressof(desc), k, ptr(val), ptr(idx), ptr(ws), stream())
    return val, idx


def ens_ahead(comps, labels, target, off_ex, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None):
    """int32 [B]: score_ahead over SEVERAL tables - the number of ELIGIBLE items that stand ahead of each session's label under
    the score of ens_select (value above target[b], or equal to it with a lower id; the label is left out by id); -1 for a
    session without a label (labels[b] < 0).  target: fp32 [B], the label's own value, always given by the caller
    (Ensemble.score_items forms it).  With (labels, target) = (ids[:, j], values[:, j]) of ens_select over the same operands
    the result is j.  Integer atomics: equal bits on every call; counts of disjoint row ranges (id_lo) add up.  Other arguments
    as ens_select; no floor."""
    a = _ens_args('ens_ahead', comps, off_ex, off_in, listed, drop_listed, id_lo, bias, group)
    B, dev = a.B, a.srs[0].device
    labels = torch.as_tensor(labels).detach()
    if labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool or labels.numel() != B:
        raise ValueError('ens_ahead: labels must hold %d integer item ids (one per session), got %s %s'
                         % (B, labels.dtype, tuple(labels.shape)))
    target = torch.as_tensor(target).detach()
    if not target.is_floating_point() or target.numel() != B:
        raise ValueError('ens_ahead: target must hold %d floating numbers (the labels\' values), got %s %s'
                         % (B, target.dtype, tuple(target.shape)))
    if B == 0:
        return torch.zeros(0, device=dev, dtype=torch.int32)
    if labels.dtype != torch.int32:         # (an id beyond int32 stays beyond every local row: the kernel clamps around them)
        labels = labels.to(torch.int64).clamp(min=-1, max=2 ** 31 - 1).to(torch.int32)
    labels = labels.to(dev).reshape(B).contiguous()
    target = target.to(device=dev, dtype=torch.float32).reshape(B).contiguous()
    ws = _scratch('ens_ahead', dev, lib.srec_ens_ahead_ws, B, a.V, max(a.ds), a.C, a.L, cache=_ENS_WS)
    out = torch.empty(B, device=dev, dtype=torch.int32)
    desc = a.struct()
    lib.srec_ens_ahead(_ct.addressof(desc), ptr(labels), ptr(target), ptr(out), ptr(ws), stream())
    return out
