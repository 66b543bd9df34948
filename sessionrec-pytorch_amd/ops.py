"""torch.autograd.Function wrappers over the C ABI (include/srec.h).

PyTorch is plumbing here: it owns device memory, the current HIP stream and the
autograd tape; every forward AND backward below is a hand-written gfx950 kernel
launched through libsrec_hip.so.  CPU tensors raise (no fallback).

`dyn` arguments are optional 1-element int32 device tensors holding the live
extent of a capacity-padded dimension (see batch.FlatBatch.dyn).

Re-exported from the modules imported at the end of this file (ops.X stays the way to reach them):
  hgat.py   the batched MSHGNN layer: HgPlan, HGATLayer, hgat_layer
  gru.py    the GRU step and the k-gram GRU expander: GRUPointwise, GramCombine, GRUExpand, GRUExpandAll, gru_step, gram_combine,
            gru_expand, gru_expand_all, gru_wfrag, gru_wfrag_both, gru_fused_ok, gru_expand_fast_ok, expand_path, GruOrder,
            gru_step_desc, gru_fused_desc, gru_fused_bwd_desc, _gru_wfrag_args
  score.py  full-catalog scoring: CEWorkspace, TableBF16, ScoreCE, ScoreStats, ScoreLogProb, score_ce, score_stats, score_logp,
            score_topk, score_rank, score_select, score_sample, sample_noise, sample_scalars, score_items, score_norm, use_bf16_scoring, sr16_written, sr16_claim, finish_table_grad, MixtureArgs,
            _bf16_dim_ok, _prepare_sr, _ce_fwd, _ce_bwd, _mixture_args, _byte_ws, _logp_cols, _pad_rows, BiasArgs, _bias_args,
            catalog_bias, diversify, diversify_scalars, cutoff_scalars, score_cutoff, cutoff_passes, select_many_k, score_select_many, score_ahead,
            score_ahead_many, ahead_among_targets, CapRule, cap_rule, cap_rule_check, cap_k, cap_select, calibrate, calibrate_scalars,
            PersonalLists, personal_lists, personal_k, personal_merge, EnsArgs, _ens_args, ens_select, ens_ahead
  head.py   the attention read-out head: SegAttn, seg_attn, ReadoutHead, ReadoutHeadFused, readout_head, readout_head_fused,
            readout_head_fused_ok, head_path, head_wfrag, _head_wfrag_args, wfrag_missing, wfrag_put, HeadOrder, head_fwd_desc,
            head_bwd_desc, HEAD_FUSED_MAX_B
"""
import ctypes as _ct
import os
from collections import namedtuple

import torch

from ._lib import CONST, STRUCTS, lib, ptr, ptr_array, stream
from .stepq import StepQueue

# host descriptor structs and capacity limits of the launchers: bound from include/srec_hg.h (_lib.parse_structs), never retyped
HgDesc = STRUCTS['srec_hg_desc']
GemmGroup = STRUCTS['srec_gemm_group']
GemmGroup16 = STRUCTS['srec_gemm16_group']
GemmF32Group = STRUCTS['srec_gemm_f32_group']
GruStepDesc = STRUCTS['srec_gru_step_desc']
GruFusedDesc = STRUCTS['srec_gru_fused_desc']
GruFusedBwdDesc = STRUCTS['srec_gru_fused_bwd_desc']
HeadDesc = STRUCTS['srec_head_desc']
HeadBwdDesc = STRUCTS['srec_head_bwd_desc']
StepPrepDesc = STRUCTS['srec_step_prep_desc']
G16_MAXP, GEMM32_MAXP, GRU_MAXP = CONST['SREC_G16_MAXP'], CONST['SREC_GEMM32_MAXP'], CONST['SREC_GRU_MAXP']
HEAD_MAXH, HEAD_MAXW = CONST['SREC_HEAD_MAXH'], CONST['SREC_HEAD_MAXW']


def _rows(t):
    """2-D fp32 tensor with unit inner stride (row-strided views allowed) -> tensor usable as (ptr, ld)."""
    assert t.dim() == 2 and t.dtype == torch.float32, (t.shape, t.dtype)
    if t.stride(1) != 1 or (t.stride(0) & 3) or (t.data_ptr() & 15) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


_WS = {}


def _ws(n, device):
    """grow-only fp32 scratch per device (column-sum partials, split-K slabs)"""
    t = _WS.get(str(device))
    if t is None or t.numel() < n:
        t = torch.empty(max(n, 1 << 22), device=device, dtype=torch.float32)
        _WS[str(device)] = t
    return t


_GEMM_WS = {}


def _gemm_ws(device):
    t = _GEMM_WS.get(str(device))
    if t is None:
        t = _GEMM_WS[str(device)] = torch.empty(1 << 24, device=device, dtype=torch.float32)   # 64 MiB of split-K slabs
    return t.data_ptr(), t.numel()


def col_sum(X, n, ncol, out, dyn=None, wgt=None, H=1, D=1, accumulate=0):
    ws = _ws(128 * ncol, X.device)            # NCHUNK_V partial rows of the vector path (32 for the weighted one)
    lib.srec_col_sum(ptr(X), _ld(X), ptr(wgt), H, D, n, ptr(dyn), ncol, ptr(out), accumulate, ptr(ws), stream())


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


_LIMITS = None


def limits():
    """static per-session budgets of the kernels (include/srec.h srec_limits)"""
    global _LIMITS
    if _LIMITS is None:
        a, b, c = _ct.c_int(), _ct.c_int(), _ct.c_int()
        lib.srec_limits(_ct.addressof(a), _ct.addressof(b), _ct.addressof(c))
        _LIMITS = dict(nodes=a.value, deg=b.value, sgat_deg=c.value)
    return _LIMITS


def copy_words(src, dst, n):
    """dst[:n] (device int32) = src[:n] (page-locked host or device int32) by a kernel on the current stream (srec_copy_words)"""
    assert dst.is_cuda and src.dtype == dst.dtype == torch.int32 and (src.is_cuda or src.is_pinned())
    lib.srec_copy_words(src.data_ptr(), dst.data_ptr(), int(n), stream())


def check_limits(mg, deg=None):
    """a batch whose longest session / largest node degree exceeds what the per-session kernels hold in LDS is refused here
    (collate records both in FlatBatch.meta): a clean error, never a silently truncated soft-max.  Host-only (two meta
    values): called by the models' forward AND by graph.GraphedTrainStep for every replayed batch - a replay never runs
    the models' Python again.  deg: which degree budget applies (default: by the batch kind - LESSR's shortcut graphs
    go through the SGAT kernels)"""
    L, m = limits(), mg.meta
    if deg is None:
        deg = 'sgat_deg' if m.get('kind') == 'shortcut' else 'deg'
    if m.get('max_nodes', 0) > L['nodes']:
        raise ValueError('a session of this batch has %d read-out nodes; the per-session kernels hold at most %d '
                         '(SREC_MAX_SESSION_NODES, csrc/common.h): truncate sessions (the reference preprocessing keeps the '
                         'last 20 clicks, preprocess.py:45-50) or lower the n-gram order' % (m['max_nodes'], L['nodes']))
    if m.get('max_deg', 0) > L[deg]:
        raise ValueError('a node of this batch has degree %d in one relation; the graph-attention kernels hold at most %d '
                         '(csrc/common.h): truncate sessions' % (m['max_deg'], L[deg]))


FUSED_GRU = True        # tests flip this to compare the fused GRU kernels (gruf.hip / grufb.hip) with the step-by-step
#                         launch sequence they replace; the product path never does
PRECISION = {'matmul': 'fp32'}      # 'fp32': exact fp32 MFMA everywhere; 'bf16': bf16-operand MFMA for the
                                    # forward / backward-data products and the scoring kernels (config C3)


def set_precision(mode):
    assert mode in ('fp32', 'bf16')
    PRECISION['matmul'] = mode
    weights_changed()


def weights_changed():
    """called by the optimizer after it updated parameters: the per-step operand copies of weights are stale"""
    _HEAD_WF.clear()
    _WPREP.clear()


# bf16 operand copies of weights made by the prologue launch of the CURRENT forward pass (step_prologue) for the one node that
# reads them (weights_bf16 in HGATLayer, gru_wfrag_both in GRUExpandAll): (kind, data_ptr, shape) -> (tensor version, buffers).
# The reader TAKES its entry - nothing outlives the forward it was made for; weights_changed drops what was never read.
_WPREP = {}


def _wprep_take(kind, w):
    e = _WPREP.pop((kind, w.data_ptr(), tuple(w.shape)), None)
    return e[1] if e is not None and e[0] == w._version else None


def _wprep_put(kind, w, bufs):
    _WPREP[(kind, w.data_ptr(), tuple(w.shape))] = (w._version, bufs)


def _bf16_ok(K, *ts):
    return PRECISION['matmul'] == 'bf16' and K % 32 == 0 and all((_ld(t) & 3) == 0 and (t.data_ptr() & 15) == 0 for t in ts)


def gemm_nt(x, w, out, bias=None, dyn=None, dyn_mode=0, beta=0.0):
    """out[M,N] = x[M,K] @ w[N,K]^T (+bias) (+beta*out)"""
    M, K = x.shape
    N = w.shape[0]
    if dyn_mode in (0, 1) and _bf16_ok(K, x, w):
        lib.srec_gemm_bf16_nt(ptr(x), _ld(x), ptr(w), _ld(w), ptr(out), _ld(out), ptr(bias), M, N, K,
                              ptr(dyn) if dyn_mode == 1 else None, 1.0, beta, *_gemm_ws(x.device), stream())
        return
    lib.srec_gemm_f32(ptr(x), _ld(x), 1, ptr(w), _ld(w), 1, ptr(out), _ld(out), ptr(bias), M, N, K, ptr(dyn), dyn_mode,
                      1.0, beta, *_gemm_ws(x.device), stream())


def gemm_nn(g, w, out, dyn=None, dyn_mode=0, beta=0.0):
    """out[M,K] = g[M,N] @ w[N,K]"""
    M, N = g.shape
    K = w.shape[1]
    if dyn_mode in (0, 1) and _bf16_ok(N, g) and not (K & 3) and not (_ld(w) & 3) and not (w.data_ptr() & 15):
        # B operand reduction-major: the weight is transposed while it is staged into LDS (no transposed copy, no
        # split-K slabs: gemm_group_bf16.hip)
        gemm_group(1, [(M, K, N, [(g, w)], out, dyn if dyn_mode == 1 else None)], _ld(g), _ld(w), _ld(out), beta)
        return
    lib.srec_gemm_f32(ptr(g), _ld(g), 1, ptr(w), 1, _ld(w), ptr(out), _ld(out), None, M, K, N, ptr(dyn), dyn_mode, 1.0,
                      beta, *_gemm_ws(g.device), stream())


def gemm_tn(g, x, out, dyn=None, beta=0.0):
    """out[N,K] = g[M,N]^T @ x[M,K]   (reduction over the M rows; dyn clamps M)"""
    M, N = g.shape
    K = x.shape[1]
    if (PRECISION['matmul'] == 'bf16' and M >= 256 and not ((N | K | _ld(g) | _ld(x) | _ld(out)) & 3)
            and not ((g.data_ptr() | x.data_ptr() | out.data_ptr()) & 15)):
        lib.srec_gemm_bf16_tn(ptr(g), _ld(g), ptr(x), _ld(x), ptr(out), _ld(out), M, N, K, ptr(dyn), 1.0, beta,
                              *_gemm_ws(g.device), stream())
        return
    lib.srec_gemm_f32(ptr(g), 1, _ld(g), ptr(x), 1, _ld(x), ptr(out), _ld(out), None, N, K, M, ptr(dyn),
                      2 if dyn is not None else 0, 1.0, beta, *_gemm_ws(g.device), stream())


_SMALL_LINEAR = 128 * 256       # weight elements up to which a linear layer is launch-bound, not flop-bound


def _small_linear(*ws):
    return sum(w.numel() for w in ws) <= _SMALL_LINEAR


def _linear_backward_group(gy, xs, ws, gws, need_x, need_b, dyn, defer=False):
    """backward of y = sum_i x_i W_i^T + b as ONE grouped exact-fp32 launch (+ its slab sum): d x_i = gy W_i, d W_i =
    gy^T x_i into gws[i] (None: not needed), d b = column sums of gy as a product with a block of ones - instead of a GEMM
    per product, a split-K sum per weight gradient and two column-sum launches.  -> ([d x_i], d b)"""
    M, N = gy.shape
    probs, gxs = [], []
    for x, w, gw, nx in zip(xs, ws, gws, need_x):
        gx = None
        if nx:
            gx = torch.empty_like(x, memory_format=torch.contiguous_format)
            probs.append(('nn', gy, w, gx, None, dyn, 0.0))
        if gw is not None:
            probs.append(('tn', gy, x, gw, None, dyn, 0.0))
        gxs.append(gx)
    gb = None
    if need_b:
        sums = torch.empty(4, N, device=gy.device, dtype=torch.float32)
        probs.append(('tn', _ones4(M, gy.device)[:M], gy, sums, None, dyn, 0.0))
        gb = sums[0]
    outs = ([gw for gw in gws if gw is not None] + ([sums] if need_b else [])) if defer else None
    for c in range(0, len(probs), GEMM32_MAXP):
        gemm_f32_group(probs[c:c + GEMM32_MAXP], defer=outs)
    return gxs, gb


class LinearCat(torch.autograd.Function):
    """y = sum_i x_i @ W[:, off_i:off_i+k_i]^T + b   == nn.Linear(cat(x_i, dim=1)) without the concat.  Exact fp32 products
    when asked for (exact) and for small weights (launch-bound either way: one rounding fewer, and the backward becomes
    one grouped launch)."""

    @staticmethod
    def forward(ctx, weight, bias, dyn, exact, *xs):
        exact = exact or _small_linear(weight)
        ctx.exact = exact
        ctx.defer, ctx.wparams = defer_scope(), [weight] + ([bias] if bias is not None else [])
        if exact and PRECISION['matmul'] != 'fp32':         # session-vector head: exact fp32 MFMA even in bf16 mode
            prev, PRECISION['matmul'] = PRECISION['matmul'], 'fp32'
            try:
                return LinearCat._fwd(ctx, weight, bias, dyn, xs)
            finally:
                PRECISION['matmul'] = prev
        return LinearCat._fwd(ctx, weight, bias, dyn, xs)

    @staticmethod
    def _fwd(ctx, weight, bias, dyn, xs):
        xs = [_rows(x) for x in xs]
        M = xs[0].shape[0]
        N = weight.shape[0]
        w = _rows(weight)
        y = torch.empty(M, N, device=w.device, dtype=torch.float32)
        off = 0
        for i, x in enumerate(xs):
            k = x.shape[1]
            gemm_nt(x, w[:, off:off + k], y, bias if i == 0 else None, dyn, 1 if dyn is not None else 0,
                    0.0 if i == 0 else 1.0)
            off += k
        assert off == w.shape[1], (off, w.shape)
        ctx.save_for_backward(w, *xs)
        ctx.dyn = dyn
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.exact and PRECISION['matmul'] != 'fp32':
            prev, PRECISION['matmul'] = PRECISION['matmul'], 'fp32'
            try:
                return LinearCat._bwd(ctx, gy)
            finally:
                PRECISION['matmul'] = prev
        return LinearCat._bwd(ctx, gy)

    @staticmethod
    def _bwd(ctx, gy):
        w, *xs = ctx.saved_tensors
        dyn = ctx.dyn
        gy = _rows(gy)
        need_x = ctx.needs_input_grad[4:]
        gw = torch.empty_like(w) if ctx.needs_input_grad[0] else None
        if _small_linear(w) and gy.shape[0] > 0:
            offs = [0]
            for x in xs:
                offs.append(offs[-1] + x.shape[1])
            gxs, gb = _linear_backward_group(gy, xs, [w[:, a:b] for a, b in zip(offs, offs[1:])],
                                             [None if gw is None else (gw if len(xs) == 1 else gw[:, a:b]) for a, b in zip(offs, offs[1:])],
                                             need_x, ctx.has_bias and ctx.needs_input_grad[1], dyn,
                                             defer=can_defer(ctx.defer, ctx.wparams))
            return (gw, gb, None, None) + tuple(gxs)
        gb = None
        gxs = []
        off = 0
        for i, x in enumerate(xs):
            k = x.shape[1]
            if need_x[i]:
                gx = torch.empty_like(x, memory_format=torch.contiguous_format)
                gemm_nn(gy, w[:, off:off + k], gx, dyn, 1 if dyn is not None else 0)
                gxs.append(gx)
            else:
                gxs.append(None)
            if gw is not None:
                gemm_tn(gy, x, gw[:, off:off + k], dyn)
            off += k
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb = torch.empty(w.shape[0], device=w.device, dtype=torch.float32)
            col_sum(gy, gy.shape[0], w.shape[0], gb, dyn)
        return (gw, gb, None, None) + tuple(gxs)


class LinearSum(torch.autograd.Function):
    """y = sum_i x_i @ W_i^T (+ b): nn.Linear(cat(x_i, dim=1)) with the weight kept as separate blocks W_i [out, k_i] - no
    concatenation of weights in the forward, no slicing of a combined weight gradient in the backward (LESSR's EOPA:
    fc_self(feat) + fc_neigh(neigh), lessr.py:36-38)"""

    @staticmethod
    def forward(ctx, bias, dyn, n, *args):
        xs, ws = [_rows(x) for x in args[:n]], [_rows(w) for w in args[n:]]
        M, N = xs[0].shape[0], ws[0].shape[0]
        y = torch.empty(M, N, device=xs[0].device, dtype=torch.float32)
        ctx.small = _small_linear(*ws)
        prev = PRECISION['matmul']
        if ctx.small:
            PRECISION['matmul'] = 'fp32'
        try:
            for i, (x, w) in enumerate(zip(xs, ws)):
                gemm_nt(x, w, y, bias if i == 0 else None, dyn, 1 if dyn is not None else 0, 0.0 if i == 0 else 1.0)
        finally:
            PRECISION['matmul'] = prev
        ctx.save_for_backward(*xs, *ws)
        ctx.dyn, ctx.n, ctx.has_bias = dyn, n, bias is not None
        ctx.defer, ctx.wparams = defer_scope(), list(args[n:]) + ([bias] if bias is not None else [])
        return y

    @staticmethod
    def backward(ctx, gy):
        n, dyn = ctx.n, ctx.dyn
        xs, ws = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        gy = _rows(gy)
        if ctx.small and gy.shape[0] > 0:
            gws = [torch.empty_like(w) if ctx.needs_input_grad[3 + n + i] else None for i, w in enumerate(ws)]
            gxs, gb = _linear_backward_group(gy, xs, ws, gws, ctx.needs_input_grad[3:3 + n],
                                             ctx.has_bias and ctx.needs_input_grad[0], dyn, defer=can_defer(ctx.defer, ctx.wparams))
            return (gb, None, None) + tuple(gxs) + tuple(gws)
        gxs, gws = [], []
        for i, (x, w) in enumerate(zip(xs, ws)):
            gx = None
            if ctx.needs_input_grad[3 + i]:
                gx = torch.empty_like(x, memory_format=torch.contiguous_format)
                gemm_nn(gy, w, gx, dyn, 1 if dyn is not None else 0)
            gw = None
            if ctx.needs_input_grad[3 + n + i]:
                gw = torch.empty_like(w)
                gemm_tn(gy, x, gw, dyn)
            gxs.append(gx)
            gws.append(gw)
        gb = None
        if ctx.has_bias and ctx.needs_input_grad[0]:
            gb = torch.empty(ws[0].shape[0], device=gy.device, dtype=torch.float32)
            col_sum(gy, gy.shape[0], ws[0].shape[0], gb, dyn)
        return (gb, None, None) + tuple(gxs) + tuple(gws)


def linear_sum(xs, ws, bias=None, dyn=None):
    return LinearSum.apply(bias, dyn, len(xs), *xs, *ws)


def linear(x, weight, bias=None, dyn=None, exact=False):
    """exact=True: fp32 MFMA regardless of set_precision (the readout / session-vector head, whose output is scaled
    by 12 before the soft-max in NISER / MSGIFSR)"""
    return LinearCat.apply(weight, bias, dyn, exact, x)


def linear_cat(xs, weight, bias=None, dyn=None, exact=False):
    return LinearCat.apply(weight, bias, dyn, exact, *xs)


class CatCols(torch.autograd.Function):
    """[a | b] along the feature axis; the backward hands out the two column halves of the incoming gradient as views"""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _rows(a), _rows(b)
        n, da, db = a.shape[0], a.shape[1], b.shape[1]
        out = torch.empty(n, da + db, device=a.device, dtype=torch.float32)
        lib.srec_cat_cols(ptr(a), _ld(a), da, ptr(b), _ld(b), db, n, ptr(out), stream())
        ctx.da = da
        return out

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.da], g[:, ctx.da:]


def cat_cols(a, b):
    return CatCols.apply(a, b)


# ------------------------------------------------------------------------------------------ dropout masks
RNG_COUNTER = {}     # str(device) -> int32[1] device tensor: the device-side step counter in effect.  A model installs the
#                      counter of ITS FusedAdam at the start of every forward (srgnn._ScoringMixin._lookup); models trained
#                      with another optimizer have none.


_NONCE = {'seed': None, 'gen': None}


def seed_dropout(seed=None):
    """(re)start the nonce stream of the dropout masks: from `seed`, or from torch.initial_seed().  Called implicitly when
    torch.initial_seed() has CHANGED since the last draw (torch.manual_seed with another value); a program that re-seeds
    with the SAME value to replay a run's masks calls it explicitly (re-seeding with an equal value is not observable)."""
    base = torch.initial_seed()
    _NONCE['seed'] = base
    # (seeded with the value itself: the first draws equal what torch's global generator would hand out right after
    #  torch.manual_seed(value) - the masks of a seeded run are the ones it had when the nonces still came from there)
    _NONCE['gen'] = torch.Generator().manual_seed(base if seed is None else int(seed))


def _nonce():
    """a fresh 31-bit draw from a PRIVATE generator seeded from torch.initial_seed(): the nonces follow torch.manual_seed
    but never advance torch's global CPU stream - the stream RandomSampler (NISER / SRGNN shuffling) and user code draw
    from - so the batch order of a seeded run does not depend on how many dropout call sites a step has (eager vs
    replayed steps, model configurations)."""
    if _NONCE['gen'] is None or _NONCE['seed'] != torch.initial_seed():
        seed_dropout()
    return int(torch.randint(0, 0x7fffffff, (1,), generator=_NONCE['gen']).item())


def rng_args(device):
    """(nonce, counter pointer) of the counter-based dropout masks (csrc/common.h srec_rng).  The nonce is a fresh draw
    from a private CPU generator per call (_nonce): it follows torch.manual_seed and renews the masks on every eager forward -
    with any optimizer, and for each of several micro-batches per optimizer step.  The callers keep it for their
    backward, which recomputes the mask.  Under hipGraph replay the kernel arguments (the nonce) are frozen; there the
    device counter, advanced by the captured optimizer step itself, renews the masks - a capture without one would
    replay ONE mask for ever and is refused."""
    c = RNG_COUNTER.get(str(device))
    dev = torch.device(device)
    if c is None and dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        raise RuntimeError('dropout inside a captured step needs a device-side step counter: construct FusedAdam(..., '
                           'model=model) before capturing (a frozen nonce alone would replay the same mask every step)')
    return _nonce(), (c.data_ptr() if c is not None else None)


class TableGrad:
    """Dense gradient buffer of the item table, shared by the scoring backward (writes every row)
    and the embedding-lookup backward (adds its rows in place): no dense+dense autograd sum."""

    def __init__(self, weight, defer=False):
        self.buf = torch.zeros_like(weight)
        self.fresh = False       # True once the scoring backward has overwritten it this step
        # Deferred row-normalisation projection (cosine-scored models, FusedAdam(fuse_projection=True)): the scoring backward
        # leaves `buf` unprojected and records pending = (table, cs, inv_scale); the lookup backward adds its rows AND their
        # radial sums radial[v] += <W_v, l_v>; the optimizer's row pass applies g = G - W (<W, G> - radial) inv^2 while it reads
        # the gradient (srec_adam_rows_proj) - one pass over the table gradient less per step.  Any other reader of the
        # gradient calls materialize() first.
        self.defer = defer
        self.pending = None
        self.radial = torch.zeros(weight.shape[0], device=weight.device, dtype=torch.float32) if defer else None
        self.radial_dirty = False    # a lookup backward has added radial sums that no row pass has consumed yet
        # Lookup gradient summed by the row pass (two-level lookup backward under a pending projection, SREC_LOOKUP_IN_ROWPASS):
        # the first level stamps slot[item] = u + 1 and the backward records lookup = (part, cptr, items, dyn_u) INSTEAD of
        # launching the second level; the optimizer's row pass (srec_adam_rows_lookup) sums the pieces of every stamped row
        # into the gradient as it reads it, adds their radial part, and clears the stamps.  `lookup` keeps `part` alive until
        # that launch has been issued (under capture it lives in the graph's pool).  slot is all zero whenever lookup is None
        # and slot_dirty is False.  Any other reader goes through materialize(), which runs the second level after all.
        self.slot = torch.zeros(weight.shape[0], device=weight.device, dtype=torch.int32) if defer else None
        self.lookup = None
        self.slot_dirty = False      # stamps that no row pass has cleared

    def lookup_in_rowpass(self):
        """may a two-level lookup backward leave its second level to the optimizer's row pass?"""
        return self.defer and self.slot is not None and self.pending is not None \
            and os.environ.get('SREC_LOOKUP_IN_ROWPASS', '1') != '0'

    def hand_over(self, part, cptr, items, dyn_u):
        assert self.lookup is None
        self.lookup = (part, cptr, items, dyn_u)
        self.slot_dirty = True
        self.radial_dirty = True

    def take_lookup(self):
        """the row pass consumes the recorded lookup (its launch clears the stamps)"""
        lk, self.lookup = self.lookup, None
        self.slot_dirty = False
        return lk

    def flush_lookup(self):
        """a recorded lookup goes through the second-level launch after all (another reader than the row pass; a second lookup
        backward before the step): buf and radial as if it had never been deferred, stamps cleared"""
        if self.lookup is not None:
            part, cptr, items, dyn_u = self.lookup
            d = self.buf.shape[1]
            ar = _arange(part.shape[0] + 1, part.device)
            if self.pending is not None:
                table = self.pending[0]
                lib.srec_scatter_add_sorted_ex(ptr(part), d, ptr(items), ptr(cptr), ptr(ar), ptr(self.buf), self.buf.stride(0),
                                               items.numel(), ptr(dyn_u), d, 1, 0.0, 0, None, 0, ptr(table), table.stride(0),
                                               ptr(self.radial), stream())
            else:
                lib.srec_scatter_add_sorted(ptr(part), d, ptr(items), ptr(cptr), ptr(ar), ptr(self.buf), self.buf.stride(0),
                                            items.numel(), ptr(dyn_u), d, 1, stream())
            self.lookup = None
        self._clear_slot()

    def _clear_slot(self):
        if self.slot is not None and self.slot_dirty:         # (never in the regular backward -> step sequence)
            self.slot.zero_()
        self.slot_dirty = False

    def overwritten(self):
        """the scoring backward has just overwritten every row of `buf` (non-accumulating): whatever an earlier backward
        left behind - a pending projection that no optimizer step consumed, radial sums of lookup gradients that went
        into the old contents (a skipped / NaN-guarded step, two backwards before a step, a training loss evaluated
        without stepping) - belongs to the old contents and goes with them"""
        self.pending = None
        self.lookup = None                                    # (its rows were meant for the old contents)
        self._clear_slot()
        if self.radial is not None and self.radial_dirty:     # (never in the regular backward -> step sequence: no fill
            self.radial.zero_()                               #  kernel in a captured step)
        self.radial_dirty = False

    def reset(self):
        """forget the current contents (optimizer.zero_grad, the undo of a graph-capture warm-up)"""
        self.fresh = False
        self.overwritten()

    def materialize(self):
        """apply a pending projection to `buf` (after it, buf is the true table gradient)"""
        self.flush_lookup()
        if self.pending is not None:
            table, cs, inv_scale = self.pending
            lib.srec_rownorm_project_radial(ptr(table), table.stride(0), ptr(cs), float(inv_scale), ptr(self.buf),
                                            self.buf.stride(0), table.shape[0], table.shape[1], ptr(self.radial), stream())
            self.pending = None
            self.radial_dirty = False
        return self.buf


class EmbeddingLookup(torch.autograd.Function):
    """rows = table[idx].  Backward = deterministic segmented row sums (no atomics): added in place
    into TableGrad when the fused loss owns the table gradient, else returned as a dense grad."""

    @staticmethod
    def forward(ctx, table, idx, uniq, tgrad, dyn_n, dyn_u, drop=None):
        n = idx.numel()
        d = table.shape[1]
        out = torch.empty(n, d, device=table.device, dtype=torch.float32)
        ctx.drop = None
        if drop is not None and drop[0] > 0:
            # feature dropout fused into the lookup (msgifsr.py:247): mask recomputed by the backward, nothing stored
            seed, cnt = rng_args(table.device)
            ctx.drop = (float(drop[0]), seed, cnt, int(drop[1]))
            lib.srec_gather_rows_drop(ptr(table), table.stride(0), ptr(idx), ptr(out), d, n, ptr(dyn_n), d, ctx.drop[0],
                                      seed, cnt, ctx.drop[3], stream())
        else:
            lib.srec_gather_rows(ptr(table), table.stride(0), ptr(idx), ptr(out), d, n, ptr(dyn_n), d, stream())
        ctx.uniq, ctx.tgrad, ctx.dyn_u, ctx.shape = uniq, tgrad, dyn_u, tuple(table.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        items, uptr, upos = ctx.uniq[:3]
        tg = ctx.tgrad
        g = _rows(g)
        V, d = ctx.shape
        if ctx.drop is not None:
            g = g.contiguous()
            pdrop, seed, cnt, salt = ctx.drop

            def first_level(gp, ldg, it, pt, ps, dst, ldd, ucap, dyn, acc):
                lib.srec_scatter_add_sorted_drop(gp, ldg, it, pt, ps, dst, ldd, ucap, dyn, d, acc, pdrop, seed, cnt, salt, stream())
        else:
            def first_level(gp, ldg, it, pt, ps, dst, ldd, ucap, dyn, acc):
                lib.srec_scatter_add_sorted(gp, ldg, it, pt, ps, dst, ldd, ucap, dyn, d, acc, stream())
        radial = ptable = None
        if tg is not None and tg.pending is not None:     # deferred projection: this gradient's radial part is recorded
            radial, ptable = tg.radial, tg.pending[0]
            tg.radial_dirty = True
        if tg is not None:
            dst, acc, ret = tg.buf, 1, None
        else:
            dst = torch.zeros(V, d, device=g.device, dtype=torch.float32)
            acc, ret = 0, dst
        if len(ctx.uniq) == 5:
            # two balanced levels: <=16 positions per wavefront, then the pieces of each item
            cptr, chunk_ptr = ctx.uniq[3], ctx.uniq[4]
            C = chunk_ptr.numel() - 1
            part = torch.empty(max(C, 1), d, device=g.device, dtype=torch.float32)
            ar = _arange(C + 1, g.device)
            if radial is not None and tg.lookup_in_rowpass() and 0 < items.numel() <= C and tg.buf.stride(0) == d:
                # the optimizer's row pass sums the pieces of each item itself (TableGrad.slot / lookup): no second-level launch.
                # An earlier lookup of this step that still waits goes through its second-level launch first.
                tg.flush_lookup()
                pdrop, seed, cnt, salt = ctx.drop if ctx.drop is not None else (0.0, 0, None, 0)
                lib.srec_scatter_add_sorted_stamp(ptr(g), _ld(g), ptr(ar), ptr(chunk_ptr), ptr(upos), ptr(part), d, C, None, d, 0,
                                                  pdrop, seed, cnt, salt, ptr(items), items.numel(), ptr(ctx.dyn_u), ptr(tg.slot),
                                                  stream())
                tg.hand_over(part, cptr, items, ctx.dyn_u)
                return ret, None, None, None, None, None, None
            if tg is not None:
                tg.flush_lookup()                           # (order of the additions into buf / radial: as the backwards ran)
            first_level(ptr(g), _ld(g), ptr(ar), ptr(chunk_ptr), ptr(upos), ptr(part), d, C, None, 0)   # padded chunks are
            if radial is not None:                                                                          # empty segments
                lib.srec_scatter_add_sorted_ex(ptr(part), d, ptr(items), ptr(cptr), ptr(ar), ptr(dst), dst.stride(0),
                                               items.numel(), ptr(ctx.dyn_u), d, acc, 0.0, 0, None, 0, ptr(ptable),
                                               ptable.stride(0), ptr(radial), stream())
            else:
                lib.srec_scatter_add_sorted(ptr(part), d, ptr(items), ptr(cptr), ptr(ar), ptr(dst), dst.stride(0),
                                            items.numel(), ptr(ctx.dyn_u), d, acc, stream())
        elif radial is not None:
            tg.flush_lookup()
            pdrop, seed, cnt, salt = ctx.drop if ctx.drop is not None else (0.0, 0, None, 0)
            lib.srec_scatter_add_sorted_ex(ptr(g), _ld(g), ptr(items), ptr(uptr), ptr(upos), ptr(dst), dst.stride(0),
                                           items.numel(), ptr(ctx.dyn_u), d, acc, pdrop, seed, cnt, salt, ptr(ptable),
                                           ptable.stride(0), ptr(radial), stream())
        else:
            first_level(ptr(g), _ld(g), ptr(items), ptr(uptr), ptr(upos), ptr(dst), dst.stride(0), items.numel(),
                        ptr(ctx.dyn_u), acc)
        return ret, None, None, None, None, None, None


def embedding_lookup(table, idx, uniq, tgrad=None, dyn_n=None, dyn_u=None, drop=None):
    """drop = (p, salt): feature dropout of the looked-up rows fused into the gather (and its backward)"""
    return EmbeddingLookup.apply(table, idx, uniq, tgrad, dyn_n, dyn_u, drop)


class RowGather(torch.autograd.Function):
    """out = x[idx] for DISTINCT idx (last-node pick, permutations); backward scatters rows back.  ascending: idx is
    non-negative and strictly ascending (one last node per session, sessions stacked in order) - the backward is then ONE
    launch that writes every row (srec_expand_rows_sorted) instead of a zero fill + a scatter."""

    @staticmethod
    def forward(ctx, x, idx, dyn, ascending=False):
        x = _rows(x)
        n, d = idx.numel(), x.shape[1]
        out = torch.empty(n, d, device=x.device, dtype=torch.float32)
        lib.srec_gather_rows(ptr(x), _ld(x), ptr(idx), ptr(out), d, n, ptr(dyn), d, stream())
        ctx.save_for_backward(idx)
        ctx.nrows, ctx.dyn, ctx.ascending = x.shape[0], dyn, ascending
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        g = _rows(g)
        n, d = g.shape
        if ctx.ascending and d % 4 == 0:
            gx = torch.empty(ctx.nrows, d, device=g.device, dtype=torch.float32)
            lib.srec_expand_rows_sorted(ptr(g), _ld(g), ptr(idx), n, ptr(ctx.dyn), ctx.nrows, d, ptr(gx), d, stream())
            return gx, None, None, None
        gx = torch.zeros(ctx.nrows, d, device=g.device, dtype=torch.float32)
        ar = _arange(n + 1, g.device)
        lib.srec_scatter_add_sorted(ptr(g), _ld(g), ptr(idx), ptr(ar), ptr(ar), ptr(gx), d, n, ptr(ctx.dyn), d, 0,
                                    stream())
        return gx, None, None, None


_ARANGE = {}


def _arange(n, device):
    key = (str(device),)
    t = _ARANGE.get(key)
    if t is None or t.numel() < n:
        t = torch.arange(max(n, 4096), device=device, dtype=torch.int32)
        _ARANGE[key] = t
    return t


def row_gather(x, idx, dyn=None, ascending=False):
    return RowGather.apply(x, idx, dyn, ascending)


class PermuteAndPick(torch.autograd.Function):
    """(x[perm], x[pick_0], x[pick_1], ...) for a PERMUTATION perm of the live rows (inv = its inverse, -1 on padded
    rows) and small distinct pick lists: MSGIFSR's per-session concatenation and last-node picks (msgifsr.py:131-147).
    Backward = one inverse-permutation gather (writes every row, padded rows zero) + one in-place scatter per pick list,
    instead of a zero-fill + scatter per output and autograd's adds."""

    @staticmethod
    def forward(ctx, x, perm, inv, dyn_n, dyn_b, *picks):
        x = _rows(x)
        d = x.shape[1]
        outs = []
        for k, (idx, dyn) in enumerate([(perm, dyn_n)] + [(p, dyn_b) for p in picks]):
            if k == 0:
                o = torch.empty(idx.numel(), d, device=x.device, dtype=torch.float32)
            else:
                # a pick is the left half of a [n, 2 d] buffer: the read-out head (ReadoutHead) puts the session's attention
                # read-out into the right half and has its fc_sr input [x_last | sr_g] without a concatenation kernel
                o = torch.empty(idx.numel(), 2 * d, device=x.device, dtype=torch.float32)[:, :d]
            lib.srec_gather_rows(ptr(x), _ld(x), ptr(idx), ptr(o), _ld(o), idx.numel(), ptr(dyn), d, stream())
            outs.append(o)
        ctx.save_for_backward(inv, *picks)
        ctx.nrows, ctx.dyn_b = x.shape[0], dyn_b
        return tuple(outs)

    @staticmethod
    def backward(ctx, g_perm, *g_picks):
        inv, *picks = ctx.saved_tensors
        g_perm = _rows(g_perm)
        d = g_perm.shape[1]
        gx = torch.empty(ctx.nrows, d, device=g_perm.device, dtype=torch.float32)
        lib.srec_gather_rows(ptr(g_perm), _ld(g_perm), ptr(inv), ptr(gx), d, ctx.nrows, None, d, stream())
        for idx, g in zip(picks, g_picks):
            if g is None:
                continue
            g = _rows(g)
            ar = _arange(idx.numel() + 1, g.device)
            lib.srec_scatter_add_sorted(ptr(g), _ld(g), ptr(idx), ptr(ar), ptr(ar), ptr(gx), d, idx.numel(),
                                        ptr(ctx.dyn_b), d, 1, stream())
        return (gx, None, None, None, None) + (None,) * len(picks)


def permute_and_pick(x, perm, inv, picks, dyn_n=None, dyn_b=None):
    outs = PermuteAndPick.apply(x, perm, inv, dyn_n, dyn_b, *picks)
    for o in outs[1:]:
        o._srec_cat_left = True          # the left half of a private [n, 2 d] buffer (ReadoutHead writes the right half)
    return outs[0], list(outs[1:])


# ------------------------------------------------------------------------------------------ deferred slab sums, riders
# Small launches of a training step that wait to leave inside other launches (the slab sums of the backward pass, the optimizer's
# step-scalar rider, the batch intake of a captured step): STEP owns what waits and says who may send it off when
# (stepq.StepQueue); the launches themselves are here.
def defer_scope():
    """snapshot for an autograd node's forward: may its backward defer its slab sums at all?"""
    return STEP.may_defer


def can_defer(flag, params):
    """backward-time check: every target parameter still without a gradient and without tensor hooks"""
    if not flag:
        return False
    for q in params:
        if not q.is_leaf:                           # a derived weight (folded norm, slice): its gradient is READ by the next node
            return False
        if q.grad is not None or getattr(q, '_backward_hooks', None) or getattr(q, '_post_accumulate_grad_hooks', None):
            return False
    return True


def _launch_slab_sums(tasks, rider=None):
    """out: contiguous, or a column block [r, w] of a row-major matrix (stride(0) = ld > w: a slice of a weight gradient).
    rider: arguments of srec_adam_hyper_multi (without the stream) that leave with the LAST launch"""
    for i in range(0, len(tasks), 32):
        chunk = tasks[i:i + 32]
        m = len(chunk)
        arr = _ct.c_void_p * m
        a_p, a_o = arr(*[t[0].data_ptr() for t in chunk]), arr(*[t[1].data_ptr() for t in chunk])
        a_r, a_n = (_ct.c_int * m)(*[t[0].shape[0] for t in chunk]), (_ct.c_long * m)(*[t[1].numel() for t in chunk])
        a_t = (_ct.c_int * m)(*[int(len(t) > 2 and bool(t[2])) for t in chunk])
        wl = [(0, 0) if t[1].is_contiguous() else (t[1].shape[1], t[1].stride(0)) for t in chunk]
        for t, (w, ld) in zip(chunk, wl):
            assert w == 0 or (t[1].dim() == 2 and t[1].stride(1) == 1), (t[1].shape, t[1].stride())
        a_w, a_l = (_ct.c_int * m)(*[w for w, _ in wl]), (_ct.c_int * m)(*[ld for _, ld in wl])
        if rider is not None and i + 32 >= len(tasks):
            lib.srec_sum_slabs_multi_hyper(m, _ct.addressof(a_p), _ct.addressof(a_r), _ct.addressof(a_n), _ct.addressof(a_o),
                                           _ct.addressof(a_t), _ct.addressof(a_w), _ct.addressof(a_l), *rider, stream())
        else:
            lib.srec_sum_slabs_multi_ld(m, _ct.addressof(a_p), _ct.addressof(a_r), _ct.addressof(a_n), _ct.addressof(a_o),
                                        _ct.addressof(a_t), _ct.addressof(a_w), _ct.addressof(a_l), stream())


def _launch_intake(box, M, counter, dst, cap, err):
    lib.srec_copy_words_mailbox(box, M, counter, dst, cap, err, stream())


# The MSHGNN layer's weight-gradient products wait for the k-gram GRU's and leave in its launch (StepQueue, "Waiting tn products");
# 0 = every node launches its own (tests / A-B runs).  Family order: which family takes the low workgroup indices of the one
# launch, 'a' = the waiting (long) problems, 'b' = the GRU's short ones.  Measured: profiles/r09_notes.md (72.9 us for the two
# launches, 64.3 us merged with 'a', 60.2 us with 'b')
WGRAD_ONE_LAUNCH = os.environ.get('SREC_WGRAD_ONE_LAUNCH', '1') != '0'
WGRAD_FAMILY_ORDER = os.environ.get('SREC_WGRAD_FAMILY_ORDER', 'b')


def _launch_tn_products(fam_a, fam_b=None):
    """fam_a / fam_b: [GemmProb with ld set] or None.  Both: one two-family launch (srec_gemm16_tn2, together at most one problem
    table); one: its own srec_gemm16_tn launches"""
    if fam_a and fam_b:
        assert WGRAD_FAMILY_ORDER in ('a', 'b'), WGRAD_FAMILY_ORDER
        ga, gb = gemm16_desc(fam_a, *fam_a[0].ld), gemm16_desc(fam_b, *fam_b[0].ld)
        lib.srec_gemm16_tn2(_ct.addressof(ga), _ct.addressof(gb), int(WGRAD_FAMILY_ORDER == 'b'), stream())
        return
    probs = fam_a or fam_b
    for i in range(0, len(probs), G16_MAXP):
        gemm16('tn', probs[i:i + G16_MAXP], *probs[0].ld)


STEP = StepQueue(_launch_slab_sums, _launch_intake, _launch_tn_products)
defer_slab_sum = STEP.defer_slab_sum
flush_deferred = STEP.flush                  # (from inside a backward pass; its end: STEP.finish)
drop_stale_deferred = STEP.drop_stale
flush_intake = STEP.flush_intake             # (where a model first reads its batch on the device: the lookup)


# ------------------------------------------------------------------------------------------ gradient arenas
# Row-sharded training all-reduces the replicated parameters' gradients in a few flat buckets (dist.VocabParallel).  A
# parameter with a slot in such a bucket carries `_srec_gslot = [arena, offset, epoch]`; a backward node that ALLOCATES the
# gradient it returns asks grad_buf(p) for the destination and gets the slot itself - the kernel then writes the gradient where
# the all-reduce reads it, and autograd's AccumulateGrad takes the view over as p.grad (no concatenation pass).  A slot is
# handed out once per training forward (`grad_epoch()`): a parameter that feeds two backward nodes gets a private buffer for
# the second one (the engine sums the two before AccumulateGrad runs), and one that already holds a gradient (accumulation
# over micro-batches) always does - whatever does not end up in its slot is copied there by the bucket code.
_GRAD_EPOCH = [0]


def grad_epoch():
    """a new training forward begins: every arena slot may be handed out once more"""
    _GRAD_EPOCH[0] += 1


def grad_slot(p, numel=None):
    """the arena view for parameter p's gradient (flat, `numel` elements: p's own slot, or a run of adjacent slots starting
    at p's), or None when p has no slot / the slot is taken / p already holds a gradient or carries hooks"""
    slot = getattr(p, '_srec_gslot', None)
    if slot is None or slot[2] == _GRAD_EPOCH[0] or p.grad is not None or not p.is_leaf:
        return None
    if getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None):
        return None
    n = p.numel() if numel is None else numel
    if slot[1] + n > slot[0].numel():
        return None
    slot[2] = _GRAD_EPOCH[0]
    return slot[0][slot[1]:slot[1] + n]


def grad_buf(p, like=None):
    """where a backward node writes the gradient of parameter p (shape of `like`, default p): its bucket slot or a new tensor"""
    like = p if like is None else like
    v = grad_slot(p) if like.numel() == p.numel() else None
    if v is not None:
        return v.view(like.shape)
    return torch.empty(like.shape, device=like.device, dtype=torch.float32)


def grad_buf_pair(p, q):
    """ONE flat buffer [p.numel() + q.numel()] for two gradients a kernel writes back to back (the GRU's two bias vectors):
    the two slots when they are neighbours in the arena (nn.GRU lists bias_ih, bias_hh one after the other)"""
    sp, sq = getattr(p, '_srec_gslot', None), getattr(q, '_srec_gslot', None)
    if sp is not None and sq is not None and sp[0] is sq[0] and sq[1] == sp[1] + p.numel() and sq[2] != _GRAD_EPOCH[0] \
            and q.grad is None and q.is_leaf and not getattr(q, '_backward_hooks', None) \
            and not getattr(q, '_post_accumulate_grad_hooks', None):
        v = grad_slot(p, p.numel() + q.numel())
        if v is not None:
            sq[2] = _GRAD_EPOCH[0]
            return v
    return torch.empty(p.numel() + q.numel(), device=p.device, dtype=torch.float32)


class GradMark(torch.autograd.Function):
    """identity; its backward calls fn() when the gradient of x has arrived - i.e. when every node downstream of x, and the
    AccumulateGrad nodes of their parameters (the engine runs those first), are done.  dist.VocabParallel.bucket_ready hangs
    the early launch of a gradient bucket's all-reduce here."""

    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def grad_mark(x, fn):
    return GradMark.apply(x, fn) if (x.requires_grad and torch.is_grad_enabled()) else x


def parse_norm_fold(text):
    """SREC_NORM_FOLD: bit mask of the normalisation folds around the MSHGNN layer (hgat.norm_fold_bits): bit 0 layer entry forward,
    1 layer exit forward, 2 layer exit backward, 3 layer entry backward.  Unset / empty: all (15)"""
    text = (text or '').strip()
    if not text:
        return 15
    v = int(text, 0)
    if not 0 <= v <= 15:
        raise ValueError('SREC_NORM_FOLD must be a bit mask 0 .. 15, got %r' % text)
    return v


NORM_FOLD = parse_norm_fold(os.environ.get('SREC_NORM_FOLD'))       # (tests / A-B runs: 0 = a launch per normalisation)


def npp_forward(x, perm, dyn_t, dyn_b, eps_mode, picks):
    """srec_norm_perm_pick_fwd -> (allf [n_cap, D], invr [n_cap], [B, 2 D] buffers whose left halves are the pick rows)"""
    NTs, D = x.shape
    n_cap, B, P = perm.numel(), picks[0].numel(), len(picks)
    dev = x.device
    allf = torch.empty(n_cap, D, device=dev, dtype=torch.float32)
    invr = torch.empty(n_cap, device=dev, dtype=torch.float32)
    bufs = [torch.empty(B, 2 * D, device=dev, dtype=torch.float32) for _ in range(P)]   # v = left half of [v | read-out]
    arr, ints = _ct.c_void_p * P, _ct.c_int * P
    a_pick, a_out = arr(*[p.data_ptr() for p in picks]), arr(*[b.data_ptr() for b in bufs])
    a_ld = ints(*([2 * D] * P))                         # (ctypes arrays must outlive the call: no temporaries in addressof)
    lib.srec_norm_perm_pick_fwd(ptr(x), _ld(x), ptr(perm), n_cap, ptr(dyn_t), D, eps_mode, 1e-12, ptr(allf), ptr(invr),
                                P, B, ptr(dyn_b), _ct.addressof(a_pick), _ct.addressof(a_out), _ct.addressof(a_ld), stream())
    return allf, invr, bufs


def npp_backward(allf, invr, g_allf, perm, cat_seg, picks, gps, types, dyn_b, NTs):
    """srec_norm_perm_pick_bwd -> dx [NTs, D] (stacked order, every row written)"""
    D, B, P, nt = allf.shape[1], picks[0].numel(), len(picks), len(types)
    dx = torch.empty(NTs, D, device=allf.device, dtype=torch.float32)
    arr, ints = _ct.c_void_p * P, _ct.c_int * P
    a_pick = arr(*[p.data_ptr() for p in picks])
    a_g = arr(*[(g.data_ptr() if g is not None else None) for g in gps])
    a_ld = ints(*[(_ld(g) if g is not None else D) for g in gps])
    tarr = _ct.c_void_p * nt
    a_dyn = tarr(*[ptr(t[2]) for t in types])
    a_r0, a_nc = (_ct.c_int * nt)(*[t[0] for t in types]), (_ct.c_int * nt)(*[t[1] for t in types])
    lib.srec_norm_perm_pick_bwd(ptr(allf), ptr(invr), ptr(g_allf), _ld(g_allf), ptr(perm), perm.numel(), ptr(cat_seg), B,
                                ptr(dyn_b), D, P,
                                _ct.addressof(a_pick), _ct.addressof(a_g), _ct.addressof(a_ld), ptr(dx), D, nt,
                                _ct.addressof(a_r0), _ct.addressof(a_nc), _ct.addressof(a_dyn), NTs, stream())
    return dx


class NormPermutePick(torch.autograd.Function):
    """(allf, v_0, v_1, ...) = (normalize(x)[perm], normalize(x)[pick_0], ...): MSGIFSR between its last MSHGNN layer and the
    read-out (msgifsr.py:260-264 F.normalize, :131-147 per-session concatenation and last-node picks) in ONE launch, and its
    backward (inverse permutation, pick scatter-add, normalisation backward) in one."""

    @staticmethod
    def forward(ctx, x, perm, cat_seg, dyn_t, dyn_b, types, eps_mode, *picks):
        x = _rows(x)
        NTs, D = x.shape
        allf, invr, bufs = npp_forward(x, perm, dyn_t, dyn_b, eps_mode, picks)
        ctx.save_for_backward(perm, cat_seg, allf, invr, *picks)
        ctx.meta = (NTs, D, picks[0].numel(), dyn_b, types)
        return (allf,) + tuple(b[:, :D] for b in bufs)

    @staticmethod
    def backward(ctx, g_allf, *g_picks):
        perm, cat_seg, allf, invr, *picks = ctx.saved_tensors
        NTs, D, B, dyn_b, types = ctx.meta
        P = len(picks)
        g_allf = _rows(g_allf)
        gps = [(_rows(g) if g is not None else None) for g in g_picks]
        dx = npp_backward(allf, invr, g_allf, perm, cat_seg, picks, gps, types, dyn_b, NTs)
        return (dx,) + (None,) * (6 + P)


def norm_permute_pick(x, perm, cat_seg, picks, types, dyn_t=None, dyn_b=None, eps_mode=0):
    """types: [(first stacked row, capacity, dyn live count)] of the node types stacked in x.  -> (allf, [v_k]); every v_k is
    the tagged left half of a private [B, 2 D] buffer whose right half the read-out head fills"""
    outs = NormPermutePick.apply(x, perm, cat_seg, dyn_t, dyn_b, tuple(types), eps_mode, *picks)
    for o in outs[1:]:
        o._srec_cat_left = True
    return outs[0], list(outs[1:])


class _GradArena:
    """gradient buffer of a row-split tensor, shared through the pieces: a consumer whose backward produces the gradient of a
    piece (normalize_stack, gru_expand_all) writes it straight into that piece's rows of ONE buffer, and SplitRows.backward
    hands the buffer on instead of concatenating (the concatenation was the last aten kernel of the captured step)."""

    def __init__(self, shape, device):
        self.shape, self.device, self.buf = tuple(shape), device, None

    def rows(self, off, n):
        if self.buf is None:
            self.buf = torch.empty(self.shape, device=self.device, dtype=torch.float32)
        return self.buf[off:off + n]


def _arena_tag(x):
    """(arena, first row) of a tensor that SplitRows handed out, else None"""
    return getattr(x, '_srec_arena', None)


def _arena_rows(tag, n, d, device):
    """gradient rows for a piece: inside its arena when it has one"""
    if tag is not None and len(tag[0].shape) == 2 and tag[0].shape[1] == d:
        return tag[0].rows(tag[1], n)
    return torch.empty(n, d, device=device, dtype=torch.float32)


class SplitRows(torch.autograd.Function):
    """row-range views x[o_i : o_i + n_i]; the backward is ONE buffer (filled in place by the consumers, see _GradArena)
    or one concatenation, instead of a zero-fill, a slice copy and an add per piece (autograd's SliceBackward)."""

    @staticmethod
    def forward(ctx, x, sizes):
        ctx.sizes, ctx.shape = sizes, x.shape
        ctx.arena = _GradArena(x.shape, x.device)
        outs, off = [], 0
        for n in sizes:
            outs.append(x[off:off + n])
            off += n
        assert off == x.shape[0]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        buf = ctx.arena.buf
        if buf is not None and all(g is not None for g in gs):
            off, esz, ok = 0, buf.element_size() * (buf.stride(0) if buf.dim() > 1 else 1), True
            for g, n in zip(gs, ctx.sizes):
                ok = ok and g.shape[0] == n and g.is_contiguous() and g.data_ptr() == buf.data_ptr() + off * esz
                off += n
            if ok:
                return buf, None
        dev = next(t for t in gs if t is not None).device
        gs = [g if g is not None else torch.zeros((n,) + tuple(ctx.shape[1:]), device=dev) for g, n in zip(gs, ctx.sizes)]
        return torch.cat(gs, 0), None


def split_rows(x, sizes):
    outs = SplitRows.apply(x, tuple(sizes))
    fn = outs[0].grad_fn if len(outs) else None
    arena = getattr(fn, 'arena', None)               # the node's ctx attributes are visible on grad_fn
    if arena is not None:
        off = 0
        for o, n in zip(outs, sizes):
            o._srec_arena = (arena, off)
            off += n
    return outs


class Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps_mode, dyn, ws=None):
        x = _rows(x)
        n, d = x.shape
        y = torch.empty(n, d, device=x.device, dtype=torch.float32)
        inv = torch.empty(n, device=x.device, dtype=torch.float32)
        sr16 = getattr(ws, 'sr16', None)
        if sr16 is not None and n <= sr16.shape[0] and d <= sr16.shape[1]:
            # ws: the scoring workspace this session vector is headed for - its bf16 operand copy is written here
            lib.srec_normalize_fwd_bf16(ptr(x), _ld(x), ptr(y), d, ptr(inv), n, ptr(dyn), d, eps_mode, 1e-12, ptr(sr16),
                                        sr16.shape[1], stream())
            sr16_written(ws, y, n, d)
        else:
            lib.srec_normalize_fwd(ptr(x), _ld(x), ptr(y), d, ptr(inv), n, ptr(dyn), d, eps_mode, 1e-12, stream())
        ctx.save_for_backward(y, inv)
        ctx.dyn = dyn
        return y

    @staticmethod
    def backward(ctx, gy):
        y, inv = ctx.saved_tensors
        gy = _rows(gy)
        n, d = y.shape
        gx = torch.empty_like(y)
        lib.srec_normalize_bwd(ptr(y), d, ptr(gy), _ld(gy), ptr(inv), ptr(gx), d, n, ptr(ctx.dyn), d, stream())
        return gx, None, None, None


def normalize(x, eps_mode=0, dyn=None, ws=None):
    """ws (a CEWorkspace in bf16 scoring mode): also write the bf16 operand copy of the rows into ws.sr16"""
    return Normalize.apply(x, eps_mode, dyn, ws)


class NormalizeStack(torch.autograd.Function):
    """stacked [sum n_p, d] = concatenation of the row-normalised x_p (np <= 4 tensors, each with its own live count): one
    launch forward, one backward, no concatenation kernel (the per-order features MSGIFSR feeds its batched MSHGNN layer)"""

    @staticmethod
    def forward(ctx, eps_mode, dyns, *xs):
        ctx.tags = [_arena_tag(x) for x in xs]              # pieces of a split tensor: their gradients go into its buffer
        xs = [_rows(x) for x in xs]
        P, d, dev = len(xs), xs[0].shape[1], xs[0].device
        ns = [x.shape[0] for x in xs]
        y = torch.empty(sum(ns), d, device=dev, dtype=torch.float32)
        inv = torch.empty(sum(ns), device=dev, dtype=torch.float32)
        arr = _ct.c_void_p * P
        a_x, a_d = arr(*[x.data_ptr() for x in xs]), arr(*[ptr(t) for t in dyns])
        a_l, a_n = (_ct.c_int * P)(*[_ld(x) for x in xs]), (_ct.c_int * P)(*ns)
        lib.srec_normalize_group_fwd(P, _ct.addressof(a_x), _ct.addressof(a_l), _ct.addressof(a_n), _ct.addressof(a_d), ptr(y),
                                     d, ptr(inv), d, eps_mode, 1e-12, stream())
        ctx.save_for_backward(y, inv)
        ctx.meta = (ns, dyns)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, inv = ctx.saved_tensors
        ns, dyns = ctx.meta
        gy = _rows(gy)
        P, d = len(ns), y.shape[1]
        dxall = torch.empty_like(y)
        dxs, o = [], 0
        for n, tag in zip(ns, ctx.tags):
            dxs.append(_arena_rows(tag, n, d, y.device) if tag is not None else dxall[o:o + n])
            o += n
        arr = _ct.c_void_p * P
        a_x, a_d = arr(*[t.data_ptr() for t in dxs]), arr(*[ptr(t) for t in dyns])
        a_l, a_n = (_ct.c_int * P)(*([d] * P)), (_ct.c_int * P)(*ns)
        lib.srec_normalize_group_bwd(P, _ct.addressof(a_x), _ct.addressof(a_l), _ct.addressof(a_n), _ct.addressof(a_d), ptr(y), d,
                                     ptr(gy), _ld(gy), ptr(inv), d, stream())
        return (None, None) + tuple(dxs)


def normalize_stack(xs, eps_mode=0, dyns=None):
    dyns = tuple(dyns) if dyns is not None else (None,) * len(xs)
    return NormalizeStack.apply(eps_mode, dyns, *xs)


def gemm_f32_group(probs, split3=False, defer=None):
    """defer: a list of output tensors - the split-K slab sums of the group's weight-gradient ('tn', whole contiguous output
    tensor) problems that write one of them join the end-of-backward slab-sum launch (defer_slab_sum) instead of a reduce
    launch behind this one; the caller has checked can_defer() for the parameters those outputs become the gradients of.
    ONE launch of up to 16 independent exact-fp32 products (csrc/gemm.hip, srec_gemm_f32_group_run; split3: as 3-term
    hi / lo bf16 splits on the bf16 matrix pipe, ~2^-17 relative).  A problem is
    (kind, a, b, out, bias, dyn, beta):  'nt' out[M,N] = a[M,K] b[N,K]^T + bias (dyn clamps M);  'nn' out[M,K] = a[M,N] b[N,K]
    (dyn clamps M);  'tn' out[N,K] = a[M,N]^T b[M,K] (dyn clamps the reduction rows M).  (+ beta * out)"""
    assert 0 < len(probs) <= GEMM32_MAXP
    g = GemmF32Group()
    g.np, g.split3 = len(probs), int(split3)
    for p, (kind, a, b, out, bias, dyn, beta) in enumerate(probs):
        if kind == 'nt':
            M, K = a.shape
            N = b.shape[0]
            g.a_rs[p], g.a_cs[p], g.b_rs[p], g.b_cs[p], mode = _ld(a), 1, _ld(b), 1, 1
        elif kind == 'nn':
            M, K = a.shape
            N = b.shape[1]
            g.a_rs[p], g.a_cs[p], g.b_rs[p], g.b_cs[p], mode = _ld(a), 1, 1, _ld(b), 1
        else:
            K, M = a.shape
            N = b.shape[1]
            g.a_rs[p], g.a_cs[p], g.b_rs[p], g.b_cs[p], mode = 1, _ld(a), 1, _ld(b), 2
        g.A[p], g.B[p], g.C[p], g.ldc[p], g.bias[p] = ptr(a), ptr(b), ptr(out), _ld(out), ptr(bias)
        g.M[p], g.N[p], g.K[p] = M, N, K
        g.dyn[p], g.dyn_mode[p] = ptr(dyn), (mode if dyn is not None else 0)
        g.alpha[p], g.beta[p] = 1.0, beta
    dev = probs[0][1].device
    if defer:
        ok = [kind == 'tn' and out.dim() == 2 and out.stride(1) == 1 and beta == 0.0 and any(out is t for t in defer)
              for (kind, a, b, out, bias, dyn, beta) in probs]
        # (the launcher only splits problems of < 128 output tiles, into <= 32 slabs)
        need = sum(32 * int(g.M[p]) * int(g.N[p]) for p in range(len(probs))
                   if ((int(g.M[p]) + 63) // 64) * ((int(g.N[p]) + 63) // 64) < 128)
        if any(ok) and need <= (1 << 24):
            # a PRIVATE slab buffer: it has to survive until the end of the backward pass (the shared one is rewritten by the
            # next group); problems that may not wait (cnt[p] = 0 on entry: accumulating / clamped / strided outputs, outputs
            # somebody reads during the backward pass) keep their reduce launch
            ws = torch.empty(need, device=dev, dtype=torch.float32)
            off, cnt = (_ct.c_long * GEMM32_MAXP)(), (_ct.c_int * GEMM32_MAXP)(*[int(o) for o in ok])
            lib.srec_gemm_f32_group_run_defer(_ct.addressof(g), ptr(ws), need, _ct.addressof(off), _ct.addressof(cnt), stream())
            for p, (kind, a, b, out, bias, dyn, beta) in enumerate(probs):
                if off[p] >= 0 and cnt[p] > 1:
                    n = out.numel()
                    defer_slab_sum(ws[off[p]:off[p] + cnt[p] * n].view(cnt[p], n), out)
            if _GROUP_DEBUG:
                print('gemm_f32_group', [(kind, int(g.M[p]), int(g.N[p]), int(g.K[p]), bool(ok[p]), off[p], cnt[p])
                                         for p, (kind, *_r) in enumerate(probs)], flush=True)
            return
    lib.srec_gemm_f32_group_run(_ct.addressof(g), *_gemm_ws(dev), stream())


_ONES4 = {}
_GROUP_DEBUG = bool(os.environ.get('SREC_GROUP_DEBUG'))


def _ones4(n, device):
    t = _ONES4.get(str(device))
    if t is None or t.shape[0] < n:
        t = _ONES4[str(device)] = torch.ones(n, 4, device=device, dtype=torch.float32)
    return t


class SegMeanAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, H, F, seg, B, dynB):
        H, F = _rows(H), _rows(F)
        N, D = F.shape
        out = torch.zeros(N, D, device=F.device, dtype=torch.float32)
        lib.srec_seg_mean_add_fwd(ptr(H), _ld(H), ptr(F), _ld(F), ptr(seg), B, ptr(dynB), D, ptr(out), D, stream())
        ctx.save_for_backward(seg)
        ctx.B, ctx.dynB = B, dynB
        return out

    @staticmethod
    def backward(ctx, g):
        (seg,) = ctx.saved_tensors
        g = _rows(g)
        N, D = g.shape
        dF = torch.zeros(N, D, device=g.device, dtype=torch.float32)
        lib.srec_seg_mean_add_bwd(ptr(g), _ld(g), ptr(seg), ctx.B, ptr(ctx.dynB), D, ptr(dF), D, stream())
        return g, dF, None, None, None


def seg_mean_add(H, F, seg, B, dynB=None):
    return SegMeanAdd.apply(H, F, seg, B, dynB)


# ------------------------------------------------------------------------------------------ GAT
class GATRelation(torch.autograd.Function):
    """rst[v,h,:] = sum_{u->v} softmax_v(LeakyReLU(el_u + er_v)) * feat_src[u,h,:] for one relation.
    graph = (in_ptr, in_idx, out_ptr, out_idx, esrc, edst); feats are [N, H*D]."""

    @staticmethod
    def forward(ctx, Fs, Fd, attn_l, attn_r, graph, H, dyn_ns, dyn_nd, slope):
        Fs, Fd = _rows(Fs), _rows(Fd)
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = graph
        Ns, HD = Fs.shape
        Nd = Fd.shape[0]
        D = HD // H
        E = esrc.numel()
        dev = Fs.device
        al, ar = attn_l.reshape(-1).contiguous(), attn_r.reshape(-1).contiguous()
        el = torch.empty(Ns, H, device=dev, dtype=torch.float32)
        er = torch.empty(Nd, H, device=dev, dtype=torch.float32)
        lib.srec_head_dot(ptr(Fs), _ld(Fs), ptr(al), Ns, ptr(dyn_ns), H, D, ptr(el), stream())
        lib.srec_head_dot(ptr(Fd), _ld(Fd), ptr(ar), Nd, ptr(dyn_nd), H, D, ptr(er), stream())
        A = torch.empty(max(E, 1), H, device=dev, dtype=torch.float32)    # every live edge written by the kernel
        rst = torch.empty(Nd, HD, device=dev, dtype=torch.float32)
        lib.srec_gat_agg_fwd(ptr(Fs), _ld(Fs), ptr(el), ptr(er), ptr(in_ptr), ptr(in_idx), ptr(esrc), Nd, ptr(dyn_nd),
                             H, D, slope, ptr(A), ptr(rst), HD, stream())
        ctx.save_for_backward(Fs, Fd, al, ar, el, er, A)
        ctx.same = Fs.data_ptr() == Fd.data_ptr() and Fs.shape == Fd.shape
        ctx.graph, ctx.H, ctx.dyn, ctx.slope = graph, H, (dyn_ns, dyn_nd), slope
        ctx.shapes = (attn_l.shape, attn_r.shape)
        return rst

    @staticmethod
    def backward(ctx, dR):
        Fs, Fd, al, ar, el, er, A = ctx.saved_tensors
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = ctx.graph
        dyn_ns, dyn_nd = ctx.dyn
        H = ctx.H
        dR = _rows(dR)
        Ns, HD = Fs.shape
        Nd = Fd.shape[0]
        D = HD // H
        dev = Fs.device
        DP = torch.empty_like(A)
        der = torch.empty(Nd, H, device=dev, dtype=torch.float32)
        lib.srec_gat_bwd_dst(ptr(dR), _ld(dR), ptr(Fs), _ld(Fs), ptr(el), ptr(er), ptr(A), ptr(in_ptr), ptr(in_idx),
                             ptr(esrc), Nd, ptr(dyn_nd), H, D, ctx.slope, ptr(DP), ptr(der), stream())
        dFs = torch.empty(Ns, HD, device=dev, dtype=torch.float32)
        del_ = torch.empty(Ns, H, device=dev, dtype=torch.float32)
        same = ctx.same
        lib.srec_gat_bwd_src(ptr(dR), _ld(dR), ptr(A), ptr(DP), ptr(al), ptr(out_ptr), ptr(out_idx), ptr(edst), Ns,
                             ptr(dyn_ns), H, D, ptr(dFs), HD, ptr(del_), ptr(der) if same else None,
                             ptr(ar) if same else None, stream())
        dFd = None                                    # same tensor as Fs: its er-side term is already in dFs
        if not same:
            dFd = torch.empty(Nd, HD, device=dev, dtype=torch.float32)
            lib.srec_head_outer(ptr(der), ptr(ar), Nd, ptr(dyn_nd), H, D, ptr(dFd), HD, stream())
        dal = torch.empty(HD, device=dev, dtype=torch.float32)
        dar = torch.empty(HD, device=dev, dtype=torch.float32)
        col_sum(Fs, Ns, HD, dal, dyn_ns, del_, H, D)
        col_sum(Fd, Nd, HD, dar, dyn_nd, der, H, D)
        return dFs, dFd, dal.view(ctx.shapes[0]), dar.view(ctx.shapes[1]), None, None, None, None, None


def gat_relation(Fs, Fd, attn_l, attn_r, graph, H, dyn_ns=None, dyn_nd=None, slope=0.2):
    return GATRelation.apply(Fs, Fd, attn_l, attn_r, graph, H, dyn_ns, dyn_nd, slope)


class HeadCombine(torch.autograd.Function):
    """out[v,:] = max_head( sum_i R_i[v,h,:] + bias[h,:] + nres * x[v,:] )"""

    @staticmethod
    def forward(ctx, x, bias, nres, H, dyn, *rsts):
        import ctypes
        x = _rows(x)
        N, D = x.shape
        dev = x.device
        rsts = [_rows(r) for r in rsts]
        bias = bias.reshape(-1).contiguous()
        out = torch.empty(N, D, device=dev, dtype=torch.float32)
        arg = torch.empty(N, D, device=dev, dtype=torch.uint8)
        arr = (ctypes.c_void_p * max(len(rsts), 1))(*[r.data_ptr() for r in rsts])
        lib.srec_head_combine_fwd(ctypes.addressof(arr), len(rsts), H * D, ptr(x), _ld(x), ptr(bias), float(nres), N,
                                  ptr(dyn), H, D, ptr(out), D, ptr(arg), stream())
        ctx.save_for_backward(arg)
        ctx.meta = (H, D, N, nres, dyn, len(rsts))
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        H, D, N, nres, dyn, nr = ctx.meta
        g = _rows(g)
        dR = torch.empty(N, H * D, device=g.device, dtype=torch.float32)
        lib.srec_head_combine_bwd(ptr(g), _ld(g), ptr(arg), N, ptr(dyn), H, D, ptr(dR), H * D, stream())
        dbias = torch.empty(H * D, device=g.device, dtype=torch.float32)
        col_sum(dR, N, H * D, dbias, dyn)
        dx = g * nres if nres != 0 else None
        return (dx, dbias, None, None, None) + tuple(dR for _ in range(nr))


def head_combine(x, bias, nres, H, rsts, dyn=None):
    return HeadCombine.apply(x, bias, nres, H, dyn, *rsts)


# ------------------------------------------------------------------------------------------ LESSR
class BatchNorm(torch.autograd.Function):
    """nn.BatchNorm1d over the live rows (training: batch statistics + running-stat update)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rmean, rvar, nbt, training, momentum, eps, dyn):
        x = _rows(x)
        n, D = x.shape
        dev = x.device
        y = torch.empty(n, D, device=dev, dtype=torch.float32)
        if training:
            mean = torch.empty(D, device=dev, dtype=torch.float32)
            var = torch.empty(D, device=dev, dtype=torch.float32)
            assert nbt is None or nbt.dtype == torch.int64
            lib.srec_bn_fwd_train(ptr(x), _ld(x), n, ptr(dyn), D, ptr(gamma), ptr(beta), float(eps), float(momentum),
                                  ptr(rmean), ptr(rvar), ptr(nbt), ptr(mean), ptr(var), ptr(y), D, ptr(_ws(64 * D, dev)),
                                  stream())
        else:
            mean, var = rmean, rvar
            lib.srec_bn_apply_fwd(ptr(x), _ld(x), ptr(mean), ptr(var), float(eps), ptr(gamma), ptr(beta), n, ptr(dyn), D,
                                  ptr(y), D, stream())
        ctx.save_for_backward(x, mean, var, gamma)
        ctx.meta = (training, eps, dyn)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, var, gamma = ctx.saved_tensors
        training, eps, dyn = ctx.meta
        gy = _rows(gy)
        n, D = x.shape
        dev = x.device
        dx = torch.empty(n, D, device=dev, dtype=torch.float32)
        dg = torch.empty(D, device=dev, dtype=torch.float32)
        db = torch.empty(D, device=dev, dtype=torch.float32)
        lib.srec_bn_bwd(ptr(gy), _ld(gy), ptr(x), _ld(x), ptr(mean), ptr(var), float(eps), ptr(gamma),
                        1 if training else 0, n, ptr(dyn), D, ptr(dx), D, ptr(dg), ptr(db), ptr(_ws(64 * D, dev)),
                        stream())
        return dx, dg, db, None, None, None, None, None, None, None


def batch_norm(x, bn, dyn=None):
    """bn: an nn.BatchNorm1d used as parameter / running-stat container"""
    track = bn.training and bn.track_running_stats
    return BatchNorm.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked if track else None,
                           bn.training, bn.momentum, bn.eps, dyn)


class PReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, dyn):
        x = _rows(x)
        n, D = x.shape
        y = torch.empty(n, D, device=x.device, dtype=torch.float32)
        lib.srec_prelu_fwd(ptr(x), _ld(x), ptr(a), n, ptr(dyn), D, ptr(y), D, stream())
        ctx.save_for_backward(x, a)
        ctx.dyn = dyn
        ctx.defer, ctx.wparams = defer_scope(), [a]
        return y

    @staticmethod
    def backward(ctx, gy):
        x, a = ctx.saved_tensors
        gy = _rows(gy)
        n, D = x.shape
        dx = torch.empty(n, D, device=x.device, dtype=torch.float32)
        da = torch.empty(D, device=x.device, dtype=torch.float32)
        if D % 4 == 0 and n > 0 and can_defer(ctx.defer, ctx.wparams):
            # the 32 chunk partials of d a wait (private buffer) for the end-of-backward slab-sum launch: da = NULL skips the
            # kernel's own final sum
            part = torch.empty(32, D, device=x.device, dtype=torch.float32)
            lib.srec_prelu_bwd(ptr(gy), _ld(gy), ptr(x), _ld(x), ptr(a), n, ptr(ctx.dyn), D, ptr(dx), D, None, ptr(part), stream())
            defer_slab_sum(part, da, True, tall=True)
        else:
            lib.srec_prelu_bwd(ptr(gy), _ld(gy), ptr(x), _ld(x), ptr(a), n, ptr(ctx.dyn), D, ptr(dx), D, ptr(da),
                               ptr(_ws(32 * D, x.device)), stream())
        return dx, da, None


def prelu(x, a, dyn=None):
    return PReLU.apply(x, a, dyn)


GRU_SEQ_MAXD = 256      # MAXD of csrc/gruseq.hip: the hidden state and the three gate rows of one node live in LDS


class GRUSeq(torch.autograd.Function):
    """EOPA: last hidden state of a GRU run over each node's in-neighbours in edge-id order.
    GI = ft W_ih^T + b_ih (per source node); graph = (in_ptr, in_idx, out_ptr, out_idx, esrc, edst)."""

    @staticmethod
    def forward(ctx, GI, Whh, bhh, graph, dyn, dynE=None):
        GI = _rows(GI)
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = graph
        N, D3 = GI.shape
        D = D3 // 3
        E = esrc.numel()
        dev = GI.device
        Whh = Whh.contiguous()
        WhhT = Whh.t().contiguous() if D > 32 else None      # D <= 32: the kernel keeps W_hh's rows in registers
        neigh = torch.empty(N, D, device=dev, dtype=torch.float32)
        # edge records: every live edge is an in-edge of exactly one live node and is written by the kernel; every reader
        # (the backward kernel, the dyn-clamped weight-gradient products) stops at the live edges - no zero fill
        gates = torch.empty(max(E, 1), D3, device=dev, dtype=torch.float32)
        Hprev = torch.empty(max(E, 1), D, device=dev, dtype=torch.float32)
        ghn = torch.empty(max(E, 1), D, device=dev, dtype=torch.float32)
        lib.srec_gru_seq_fwd(ptr(GI), _ld(GI), ptr(Whh), ptr(WhhT), ptr(bhh), ptr(in_ptr), ptr(in_idx), ptr(esrc), N, ptr(dyn), D,
                             ptr(neigh), D, ptr(gates), ptr(Hprev), ptr(ghn), stream())
        ctx.save_for_backward(Whh, gates, Hprev, ghn)
        ctx.graph, ctx.dyn, ctx.dynE, ctx.shape = graph, dyn, dynE, (N, D, E)
        ctx.defer, ctx.wparams = defer_scope(), [Whh, bhh]
        return neigh

    @staticmethod
    def backward(ctx, dneigh):
        Whh, gates, Hprev, ghn = ctx.saved_tensors
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = ctx.graph
        N, D, E = ctx.shape
        dev = Whh.device
        dneigh = _rows(dneigh)
        dGIe = torch.empty(max(E, 1), 3 * D, device=dev, dtype=torch.float32)
        dGHe = torch.empty(max(E, 1), 3 * D, device=dev, dtype=torch.float32)
        lib.srec_gru_seq_bwd(ptr(dneigh), _ld(dneigh), ptr(Whh), ptr(gates), ptr(Hprev), ptr(ghn), ptr(in_ptr),
                             ptr(in_idx), N, ptr(ctx.dyn), D, ptr(dGIe), ptr(dGHe), stream())
        # per-source sum of the edge records (out-edge CSR), then weight gradients as GEMMs over the E records
        dGI = torch.empty(N, 3 * D, device=dev, dtype=torch.float32)      # every live row written (rows past dyn: never read)
        ar = _arange(N + 1, dev)
        lib.srec_scatter_add_sorted(ptr(dGIe), 3 * D, ptr(ar), ptr(out_ptr), ptr(out_idx), ptr(dGI), 3 * D, N,
                                    ptr(ctx.dyn), 3 * D, 0, stream())
        dWhh = (torch.empty if E > 0 else torch.zeros)(3 * D, D, device=dev, dtype=torch.float32)
        dbhh = (torch.empty if E > 0 else torch.zeros)(3 * D, device=dev, dtype=torch.float32)
        if E > 0 and _small_linear(Whh):                       # one grouped launch: d W_hh and d b_hh (product with ones)
            sums = torch.empty(4, 3 * D, device=dev, dtype=torch.float32)
            gemm_f32_group([('tn', dGHe[:E], Hprev[:E], dWhh, None, ctx.dynE, 0.0),
                            ('tn', _ones4(E, dev)[:E], dGHe[:E], sums, None, ctx.dynE, 0.0)],
                           defer=[dWhh, sums] if can_defer(ctx.defer, ctx.wparams) else None)
            dbhh = sums[0]
        elif E > 0:
            gemm_tn(dGHe[:E], Hprev[:E], dWhh, ctx.dynE)       # padded edge records are zero rows
            col_sum(dGHe, E, 3 * D, dbhh, ctx.dynE)
        return dGI, dWhh, dbhh, None, None, None


def gru_seq(GI, Whh, bhh, graph, dyn=None, dynE=None):
    return GRUSeq.apply(GI, Whh, bhh, graph, dyn, dynE)


class SGATAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, we, Vf, graph, dyn):
        Q, K, Vf = _rows(Q), _rows(K), _rows(Vf)
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = graph
        N, Hh = Q.shape
        Do = Vf.shape[1]
        E = esrc.numel()
        dev = Q.device
        we = we.reshape(-1).contiguous()
        A = torch.zeros(max(E, 1), device=dev, dtype=torch.float32)
        out = torch.empty(N, Do, device=dev, dtype=torch.float32)
        lib.srec_sgat_fwd(ptr(Q), _ld(Q), ptr(K), _ld(K), ptr(we), ptr(Vf), _ld(Vf), ptr(in_ptr), ptr(in_idx), ptr(esrc),
                          N, ptr(dyn), Hh, Do, ptr(A), ptr(out), Do, stream())
        ctx.save_for_backward(Q, K, we, Vf, A)
        ctx.graph, ctx.dyn = graph, dyn
        return out

    @staticmethod
    def backward(ctx, g):
        Q, K, we, Vf, A = ctx.saved_tensors
        in_ptr, in_idx, out_ptr, out_idx, esrc, edst = ctx.graph
        g = _rows(g)
        N, Hh = Q.shape
        Do = Vf.shape[1]
        E = esrc.numel()
        dev = Q.device
        dQe = torch.zeros(max(E, 1), Hh, device=dev, dtype=torch.float32)
        dK = torch.empty(N, Hh, device=dev, dtype=torch.float32)
        dwp = torch.empty(N, Hh, device=dev, dtype=torch.float32)
        lib.srec_sgat_bwd_dst(ptr(g), _ld(g), ptr(Q), _ld(Q), ptr(K), _ld(K), ptr(we), ptr(Vf), _ld(Vf), ptr(A),
                              ptr(in_ptr), ptr(in_idx), ptr(esrc), N, ptr(ctx.dyn), Hh, Do, ptr(dQe), ptr(dK), Hh,
                              ptr(dwp), Hh, stream())
        dQ = torch.empty(N, Hh, device=dev, dtype=torch.float32)
        dV = torch.empty(N, Do, device=dev, dtype=torch.float32)
        lib.srec_sgat_bwd_src(ptr(g), _ld(g), ptr(A), ptr(dQe), ptr(out_ptr), ptr(out_idx), ptr(edst), N, ptr(ctx.dyn),
                              Hh, Do, ptr(dQ), Hh, ptr(dV), Do, stream())
        dwe = torch.empty(Hh, device=dev, dtype=torch.float32)
        col_sum(dwp, N, Hh, dwe, ctx.dyn)
        return dQ, dK, dwe.view(1, Hh), dV, None, None


def sgat_attn(Q, K, we, Vf, graph, dyn=None):
    return SGATAttn.apply(Q, K, we, Vf, graph, dyn)


class EdgeAgg(torch.autograd.Function):
    """out[v] = sum_{e into v} coef[e] x[src(e)] (coef constant); backward = the same kernel on the out-edge CSR."""

    @staticmethod
    def forward(ctx, x, coef, fwd_csr, bwd_csr, dyn):
        x = _rows(x)
        N, D = x.shape
        out = torch.empty(N, D, device=x.device, dtype=torch.float32)
        p, i, o = fwd_csr
        lib.srec_edge_agg(ptr(x), _ld(x), ptr(p), ptr(i), ptr(o), ptr(coef), N, ptr(dyn), D, ptr(out), D, stream())
        ctx.save_for_backward(coef)
        ctx.bwd_csr, ctx.dyn = bwd_csr, dyn
        return out

    @staticmethod
    def backward(ctx, g):
        (coef,) = ctx.saved_tensors
        g = _rows(g)
        N, D = g.shape
        dx = torch.empty(N, D, device=g.device, dtype=torch.float32)
        p, i, o = ctx.bwd_csr
        lib.srec_edge_agg(ptr(g), _ld(g), ptr(p), ptr(i), ptr(o), ptr(coef), N, ptr(ctx.dyn), D, ptr(dx), D, stream())
        return dx, None, None, None, None


def edge_coef(ptr_, idx, ew, n, dyn=None):
    coef = torch.zeros(max(ew.numel(), 1), device=ew.device, dtype=torch.float32)
    lib.srec_edge_coef(ptr(ptr_), ptr(idx), ptr(ew), n, ptr(dyn), ptr(coef), stream())
    return coef


def edge_agg(x, coef, fwd_csr, bwd_csr, dyn=None):
    return EdgeAgg.apply(x, coef, fwd_csr, bwd_csr, dyn)


# ------------------------------------------------------------------------------------------ MSHGNN layer (batched)
# one problem of a grouped GEMM launch: C [M, N] from the segments [(A, B), ...], dyn = device live count; a plain 6-tuple is the
# same problem.  gemm16 only: koff (tn: first reduction row of this piece of a row-split product), nsplit (tn: in-kernel row
# split, C = [nsplit, M, N] slabs), ld = per-problem (lda, ldb, ldc), mhint (nt: expected live rows of a capacity-padded problem),
# rows (nt, bf16 output: int32 device list of the rows to compute, dyn = its device count; the other rows of C stay unwritten)
GemmProb = namedtuple('GemmProb', 'M N K segs C dyn koff nsplit ld mhint rows', defaults=(0, 1, None, 0, None))


def gemm_group(mode, probs, lda, ldb, ldc, beta=0.0, a16=False, c16=False):
    """probs: [GemmProb or (M, N, K, [(A, B), ...] segments, C, dyn)] tensors -> one srec_gemm_group_bf16 launch"""
    g = GemmGroup()
    g.np, g.lda, g.ldb, g.ldc, g.beta, g.a16, g.c16 = len(probs), lda, ldb, ldc, beta, int(a16), int(c16)
    for p, q in enumerate(GemmProb(*q) for q in probs):
        g.M[p], g.N[p], g.K[p], g.nseg[p], g.C[p], g.dyn[p] = q.M, q.N, q.K, len(q.segs), ptr(q.C), ptr(q.dyn)
        for si, (A, B) in enumerate(q.segs):
            g.A[p][si], g.B[p][si] = ptr(A), ptr(B)
    lib.srec_gemm_group_bf16(_ct.addressof(g), mode, stream())


def gemm16_desc(probs, lda, ldb, ldc, beta=0.0, c16=False, keep_dead=False):
    """the srec_gemm16_group of one gemm16 launch (host struct; its pointers are the tensors' device pointers)"""
    assert 0 < len(probs) <= G16_MAXP
    g = GemmGroup16()
    g.np, g.lda, g.ldb, g.ldc, g.beta = len(probs), lda, ldb, ldc, beta
    g.c16 = (CONST['SREC_G16_C_BF16'] if c16 else 0) | (CONST['SREC_G16_KEEP_DEAD'] if keep_dead else 0)
    for p, q in enumerate(GemmProb(*q) for q in probs):
        g.M[p], g.N[p], g.K[p], g.nseg[p], g.C[p], g.dyn[p] = q.M, q.N, q.K, len(q.segs), ptr(q.C), ptr(q.dyn)
        g.koff[p], g.nsplit[p], g.mhint[p] = q.koff, q.nsplit, int(q.mhint or 0)
        if q.ld is not None:                             # (0 = the group's)
            g.lda_p[p], g.ldb_p[p], g.ldc_p[p] = q.ld
        for si, (A, B) in enumerate(q.segs):
            g.A[p][si], g.B[p][si] = ptr(A), ptr(B)
    return g


def gemm16(kind, probs, lda, ldb, ldc, beta=0.0, c16=False, keep_dead=False):
    """one grouped launch of the bf16-in-HBM GEMMs (csrc/gemm16.hip) over probs.  kind 'nt': C [M, N] (+)= sum_s A_s [M, K] B_s [N, K]^T
    (c16: bf16 output);  'tn': C [M, N] = sum_s A_s [K, M]^T B_s [K, N] (reduction over the K rows, clamped by dyn)."""
    g = gemm16_desc(probs, lda, ldb, ldc, beta, c16, keep_dead)
    rows = [GemmProb(*q).rows for q in probs]
    if any(r is not None for r in rows):
        assert kind == 'nt', 'row lists: nt launches only'
        ra = ptr_array(rows)                             # (host array: alive across the call)
        lib.srec_gemm16_nt_rows(_ct.addressof(g), _ct.addressof(ra), stream())
        return
    (lib.srec_gemm16_nt if kind == 'nt' else lib.srec_gemm16_tn)(_ct.addressof(g), stream())


def rows_bf16(x, dyn=None):
    """bf16 copy of fp32 rows [n, d] (zero rows past the live count)"""
    x = _rows(x)
    n, d = x.shape
    out = torch.empty(n, d, device=x.device, dtype=torch.bfloat16)
    lib.srec_rows_bf16(ptr(x), _ld(x), n, ptr(dyn), d, ptr(out), stream())
    return out


def _weights_bf16_args(ws, transposed=True):
    n = len(ws)
    assert 0 < n <= 8
    dev = ws[0].device
    w16 = [torch.empty(w.shape, device=dev, dtype=torch.bfloat16) for w in ws]
    wt16 = [torch.empty(w.shape[1], w.shape[0], device=dev, dtype=torch.bfloat16) if transposed else None for w in ws]
    return w16, wt16, (ptr_array(ws), ptr_array(w16), ptr_array(wt16),
                       (_ct.c_int * n)(*[w.shape[0] for w in ws]), (_ct.c_int * n)(*[w.shape[1] for w in ws]))


def weights_bf16(ws, transposed=True):
    """[(W16, WT16)] bf16 copies (and transposed copies) of up to 8 contiguous fp32 matrices, one launch - unless the prologue
    launch of this forward pass made them (step_prologue)"""
    hit = [_wprep_take('w16', w) for w in ws]
    if all(h is not None and (h[1] is not None or not transposed) for h in hit):
        return [h[0] for h in hit], [h[1] for h in hit]
    w16, wt16, args = _weights_bf16_args(ws, transposed)          # (args: kept alive across the call)
    lib.srec_weights_bf16(len(ws), *[_ct.addressof(a) for a in args], stream())
    return w16, wt16


# ---- the step's prologue launch (csrc/prep.hip) ----------------------------------------------------------------------------
STEP_PROLOGUE = os.environ.get('SREC_STEP_PROLOGUE', '1') != '0'     # (tests / A-B runs: 0 = the one-launch-per-reader sequence)


def step_prologue(w16=(), gru=(), head=(), fold=None):
    """Everything a forward pass does to its WEIGHTS before it reads the first row of its batch, plus a pending batch intake, as
    ONE launch (srec_step_prep, csrc/prep.hip) instead of one small launch in front of each reader:
      w16:  fp32 matrices (<= 8) -> bf16 + transposed bf16 copies, taken by weights_bf16 (HGATLayer);
      gru:  GRU weights [3 d, d] (<= 2 SREC_GRU_MAXP) -> both fragment-major layouts, taken by gru_wfrag_both / gru_wfrag (GRUExpandAll);
      head: [(W, trans)] (<= SREC_HEAD_MAXW) -> hi / lo fragment-major copies, found by head_wfrag (ReadoutHeadFused) in its per-step cache;
      fold: (plan, params) of an MSHGNN layer call -> its scratch with V / the bias sums written, handed to plan.put_fold (HGATLayer).
    Purely an optimisation: a reader that does not find its copies makes them itself."""
    q, keep = StepPrepDesc(), []
    w16 = [w for i, w in enumerate(w16) if all(w is not v for v in w16[:i])][:8]
    if w16:
        a16, t16, args = _weights_bf16_args(w16)
        q.n_w16 = len(w16)
        q.w16_W, q.w16_out, q.w16_T, q.w16_R, q.w16_C = (_ct.addressof(a) for a in args)
        keep.append(args)
    gru = list(gru)[:2 * GRU_MAXP]
    if gru:
        of, ob, args = _gru_wfrag_args(gru)
        q.n_gru, q.gru_d = len(gru), gru[0].shape[1]
        q.gru_W, q.gru_fwd, q.gru_bwd = (_ct.addressof(a) for a in args)
        keep.append(args)
    head = wfrag_missing(head)
    if head:
        hb, args = _head_wfrag_args([w for w, _ in head], [t for _, t in head])
        q.n_head = len(head)
        q.head_W, q.head_out, q.head_rows, q.head_cols, q.head_trans = (_ct.addressof(a) for a in args)
        keep.append(args)
    if fold is not None:
        plan, params = fold
        small, lay = plan.scratch(params[0].device)
        flat = [p_.reshape(-1) if i % 4 else p_ for i, p_ in enumerate(params)]
        hd = plan.fill(HgDesc(), small, lay, None, None, flat, None, None)
        q.hg = _ct.addressof(hd)
        keep.append((hd, flat))
    box = STEP.take_intake()                       # (one intake of a captured step rides along; others leave ahead of it)
    if box is not None:
        q.mailbox, q.M, q.counter, q.box_dst, q.box_cap, q.box_err = box[:6]
    lib.srec_step_prep(_ct.addressof(q), stream())
    for w, a, t in zip(w16, a16 if w16 else (), t16 if w16 else ()):
        _wprep_put('w16', w, (a, t))
    for w, f, b_ in zip(gru, of if gru else (), ob if gru else ()):
        _wprep_put('gru', w, (f, b_))
    for (w, t), b_ in zip(head, hb if head else ()):
        wfrag_put(w, t, b_)
    if fold is not None:
        plan.put_fold(small, lay)


# MSHGNN 'g16' forward: project only the rows some edge reads as its source (csrc/hgat.hip live-source rows + the row lists of
# csrc/gemm16.hip); 0 = every live row (tests / A-B runs)
HG_LIVE_ROWS = os.environ.get('SREC_HG_LIVE_ROWS', '1') != '0'
DROP_TAP = None      # tests: set to a list to receive {'ms': [2, NT, D], 'mk': [per instance (E*H,)]} of every dropout layer call

from .hgat import HgPlan, HGATLayer, NormEntry, NormExit, hgat_layer, norm_fold_bits  # noqa: E402,F401  (the MSHGNN layer: hgat.py imports this module)
from .gru import (  # noqa: E402,F401  (the GRU step, the k-gram expander: gru.py imports this module)
    GramCombine, GruOrder, GRUExpand, GRUExpandAll, GRUPointwise, _gru_wfrag_args, expand_path, gram_combine, gru_expand,
    gru_expand_all, gru_expand_fast_ok, gru_fused_bwd_desc, gru_fused_desc, gru_fused_ok, gru_step, gru_step_desc, gru_wfrag,
    gru_wfrag_both)
from .score import (  # noqa: E402,F401  (full-catalog scoring: score.py imports this module)
    BiasArgs, CEWorkspace, MixtureArgs, ScoreCE, ScoreLogProb, ScoreStats, TableBF16, _bf16_dim_ok, _byte_ws, _ce_bwd, _ce_fwd, _logp_cols,
    _bias_args, _mixture_args, _pad_rows, _prepare_sr, catalog_bias, diversify, diversify_scalars, finish_table_grad, score_ce, score_items, score_logp, score_norm, score_rank,
    sample_noise, sample_scalars, score_sample, score_select, score_stats, score_topk, sr16_claim, sr16_written, use_bf16_scoring,
    cutoff_passes, cutoff_scalars, score_cutoff, select_many_k, score_select_many, score_ahead,
    score_ahead_many, ahead_among_targets, CapRule, cap_rule, cap_rule_check, cap_k, cap_select, calibrate, calibrate_scalars, _int_vector,
    PersonalLists, personal_lists, personal_k, personal_merge, EnsArgs, _ens_args, ens_select, ens_ahead)
from .head import (  # noqa: E402,F401  (the attention read-out head: head.py imports this module and score.py)
    HEAD_FUSED_MAX_B, HeadOrder, ReadoutHead, ReadoutHeadFused, SegAttn, _head_wfrag_args, head_bwd_desc, head_fwd_desc, head_path,
    head_wfrag, readout_head, readout_head_fused, readout_head_fused_ok, seg_attn, wfrag_missing, wfrag_put)
from .head import _WF as _HEAD_WF  # noqa: E402  (the head's fragment copies of this step: weights_changed drops them)
