"""The attention read-out head (csrc/segops.hip, csrc/headf.hip around the grouped exact-fp32 GEMMs): the single read-out node,
the grouped head, the fused head with its descriptors and fragment copies, the one backward tail both heads share and the path choice.
ops.py keeps the GEMM wrappers and the precision switch (reached through the module object at call time) and re-exports this."""
import ctypes as _ct
from collections import namedtuple

import torch

from . import ops                    # (ops.py imports this module at its end: import the package or ops first, never head alone)
from ._lib import lib, ptr, ptr_array, stream
from .ops import (GEMM32_MAXP, HEAD_MAXH, HEAD_MAXW, HeadBwdDesc, HeadDesc, _ld, _ones4, _rows, can_defer, col_sum, defer_scope,
                  defer_slab_sum, gemm_f32_group, grad_buf)
from .score import sr16_written


def _attn_fwd(U, Vq, we, X, seg, dynB, out=None):
    """srec_seg_attn_fwd on row-strided U, Vq, X -> (alpha, out);  out: where the session rows go (default: a new [B, D])"""
    B, h = Vq.shape
    N, D = X.shape
    alpha = torch.empty(N, device=X.device, dtype=torch.float32)      # live nodes written, padded never read
    if out is None:
        out = torch.empty(B, D, device=X.device, dtype=torch.float32)
    lib.srec_seg_attn_fwd(ptr(U), _ld(U), ptr(Vq), _ld(Vq), ptr(we), ptr(X), _ld(X), ptr(seg), B, ptr(dynB), h, D,
                          ptr(alpha), ptr(out), _ld(out), stream())
    return alpha, out


def _attn_bwd(gout, X, alpha, U, Vq, we, seg, dynB):
    """srec_seg_attn_bwd -> (dX, dU, dVq, dwp);  dwp [B, h]: per-session rows whose column sums are d fc_e"""
    B, h = Vq.shape
    N, D = X.shape
    dX = torch.empty(N, D, device=X.device, dtype=torch.float32)      # rows behind the live nodes zeroed in-kernel
    dU = torch.empty(N, h, device=X.device, dtype=torch.float32)
    dVq = torch.empty(B, h, device=X.device, dtype=torch.float32)
    dwp = torch.empty(B, h, device=X.device, dtype=torch.float32)
    lib.srec_seg_attn_bwd(ptr(gout), _ld(gout), ptr(X), _ld(X), ptr(alpha), ptr(U), _ld(U), ptr(Vq), _ld(Vq), ptr(we), ptr(seg),
                          B, ptr(dynB), h, D, N, ptr(dX), D, ptr(dU), h, ptr(dVq), h, ptr(dwp), h, stream())
    return dX, dU, dVq, dwp


class SegAttn(torch.autograd.Function):
    """alpha = softmax_session(fc_e(sigmoid(U + Vq[b])));  out_b = sum_i alpha_i x_i"""

    @staticmethod
    def forward(ctx, U, Vq, we, X, seg, dynB):
        U, Vq, X = _rows(U), _rows(Vq), _rows(X)
        ctx.defer, ctx.wparams = defer_scope(), [we]
        we = we.reshape(-1).contiguous()
        alpha, out = _attn_fwd(U, Vq, we, X, seg, dynB)
        ctx.save_for_backward(U, Vq, we, X, alpha, seg)
        ctx.dynB = dynB
        return out

    @staticmethod
    def backward(ctx, gout):
        U, Vq, we, X, alpha, seg = ctx.saved_tensors
        B, h = Vq.shape
        dX, dU, dVq, dwp = _attn_bwd(_rows(gout), X, alpha, U, Vq, we, seg, ctx.dynB)
        dwe = torch.empty(h, device=X.device, dtype=torch.float32)
        if h % 4 == 0 and can_defer(ctx.defer, ctx.wparams):
            # d fc_e = the column sums of the per-session rows (dead sessions' rows are zeros): a 'tall' task of the ONE
            # end-of-backward slab-sum launch instead of two launches here
            defer_slab_sum(dwp, dwe, True, tall=True)
        else:
            col_sum(dwp, B, h, dwe, ctx.dynB)
        return dU, dVq, dwe.view(1, h), dX, None, None


def seg_attn(U, Vq, we, X, seg, dynB=None):
    return SegAttn.apply(U, Vq, we, X, seg, dynB)


# one live order of a head call, in the order of the flat argument list: query rows v [B, dv], fc_u (Wu, bu or None), fc_v (Wv),
# fc_e (we) and fc_sr (Wsr [out, dv + D])
HeadOrder = namedtuple('HeadOrder', 'v Wu bu Wv we Wsr')
# what a head node saves per order for its backward (after allf, seg); the fused head adds its normalised output and 1 / norm
HeadSaved = namedtuple('HeadSaved', 'v Wu Wv we Wsr U Vq alpha cat')
HeadSavedFused = namedtuple('HeadSavedFused', HeadSaved._fields + ('y', 'inv'))
# per-order buffers of the two fused launches (what srec_head_fwd / srec_head_bwd write; gy: the gradient srec_head_bwd reads)
HeadFwdBufs = namedtuple('HeadFwdBufs', 'cat alpha U Vq y inv')
HeadBwdBufs = namedtuple('HeadBwdBufs', 'gy gs gcat dX dU dVq dwp')


def _orders(flat):
    """the flat argument list of a head node -> [HeadOrder]"""
    n = len(HeadOrder._fields)
    assert flat and len(flat) % n == 0, len(flat)
    return [HeadOrder(*flat[j:j + n]) for j in range(0, len(flat), n)]


def _saved(ctx, record):
    """ctx.saved_tensors of a head node -> (allf, seg, [record per order])"""
    allf, seg, *rest = ctx.saved_tensors
    n = len(record._fields)
    return allf, seg, [record(*rest[j:j + n]) for j in range(0, len(rest), n)]


def tail_problems(probs, s, allf, dT, dB, ones, dU, dVq, dwp, dX, gv, gWu, gWv, wsr=None, bias=None):
    """appends the batch-wide products of one order's backward (s: its HeadSaved) to the problem list of gemm_f32_group:
        d allf (this order) = dX + dU Wu,  d Wu = dU^T allf,  d v = gv + dVq Wv,  d Wv = dVq^T v,
        wsr = (gs, cat, gWsr):  d Wsr = gs^T cat  (the fused head; the grouped head has it in its first launch),
        bias = (rows, operand, dyn):  d bu = the column sums of the operand's rows, as a product with `ones` (a block of ones),
        d we = the column sums of dwp, likewise (as col_sum calls the two sums were two kernel nodes each).
    -> (d bu or None, d we, the sum blocks the products write)"""
    B, h = dwp.shape
    probs.append(('nn', dU, s.Wu, dX, None, dT, 1.0))
    probs.append(('tn', dU, allf, gWu, None, dT, 0.0))
    probs.append(('nn', dVq, s.Wv, gv, None, dB, 1.0))
    probs.append(('tn', dVq, s.v, gWv, None, dB, 0.0))
    if wsr is not None:
        gs, cat, gWsr = wsr
        probs.append(('tn', gs, cat, gWsr, None, dB, 0.0))
    sums = torch.empty(8, h, device=dwp.device, dtype=torch.float32)
    s_bu, s_we = sums[:4], sums[4:]
    gbu, blocks = None, [s_we]
    if bias is not None:
        rows, operand, dyn = bias
        probs.append(('tn', ones[:rows], operand, s_bu, None, dyn, 0.0))
        gbu, blocks = sums[0], [s_bu, s_we]
    probs.append(('tn', ones[:B], dwp, s_we, None, dB, 0.0))
    return gbu, sums[4:5], blocks


def launch_orders(probs, per_order, split3, defer=None):
    """the problem list of a backward tail in launches of whole orders (per_order problems each, nominally: an order without
    a bias has one fewer) - one launch when everything fits"""
    step = GEMM32_MAXP if len(probs) <= GEMM32_MAXP else GEMM32_MAXP // per_order * per_order
    for c in range(0, len(probs), step):
        gemm_f32_group(probs[c:c + step], split3=split3, defer=defer)


class ReadoutHead(torch.autograd.Function):
    """Attention read-out + session-vector projection of MSGIFSR (msgifsr.py:127-146 AttnReadout, :272-279 fc_sr) for
    every live order as grouped launches - exact fp32 in fp32 mode, 3-term hi / lo bf16 splits (fp32-grade, ~2^-17) in
    bf16 mode, like the fused head of d = 128 / 256:
        U_i = allf Wu_i^T + bu_i;  Vq_i = v_i Wv_i^T;  alpha_i = softmax_session(we_i . sigmoid(U_i + Vq_i[b]));
        g_i = sum alpha_i allf;  s_i = [v_i | g_i] Wsr_i^T
    forward: 1 grouped GEMM (all U, Vq) + per order (read-out kernel, concat) + 1 grouped GEMM (all s);
    backward: 1 grouped GEMM (d cat, d Wsr) + per order read-out backward + 1 grouped GEMM (+ 1 slab reduce) for
    d allf += dU Wu, d Wu, d v += dVq Wv, d Wv + the two bias / fc_e column sums.  The same products launched one by one
    were 9 GEMM + 7 split-K reduce + 2 accumulate nodes of the captured step."""

    @staticmethod
    def forward(ctx, allf, seg, dT, dB, *flat):
        given = _orders(flat)
        allf = _rows(allf)
        NT, D = allf.shape
        dev = allf.device
        split3 = ops.PRECISION['matmul'] == 'bf16'
        run = [HeadOrder(_rows(o.v), _rows(o.Wu), o.bu, _rows(o.Wv), o.we.reshape(-1).contiguous(), _rows(o.Wsr)) for o in given]
        B, h = run[0].v.shape[0], run[0].Wu.shape[0]
        Us = [torch.empty(NT, h, device=dev, dtype=torch.float32) for _ in run]
        Vqs = [torch.empty(B, h, device=dev, dtype=torch.float32) for _ in run]
        probs = []
        for o, U, Vq in zip(run, Us, Vqs):
            probs.append(('nt', allf, o.Wu, U, o.bu, dT, 0.0))
            probs.append(('nt', o.v, o.Wv, Vq, None, dB, 0.0))
        gemm_f32_group(probs, split3=split3)
        saved, outs, probs = [], [], []
        for o, g, U, Vq in zip(run, given, Us, Vqs):
            v, dv = o.v, o.v.shape[1]
            cat = None
            # only a tensor its producer tagged as the left half of a PRIVATE [B, dv + D] buffer (permute_and_pick /
            # norm_permute_pick): any other column slice of a live [B, 2 d] tensor must not have its right half overwritten
            if B > 1 and getattr(g.v, '_srec_cat_left', False) and v.stride(0) == dv + D and v.stride(1) == 1:
                try:                                       # v already is the left half of a [B, dv + D] buffer (permute_and_pick)
                    cat = v.as_strided((B, dv + D), (dv + D, 1))
                except RuntimeError:
                    cat = None
            # the read-out rows go straight into the right half, or into a buffer of their own, concatenated behind the launch
            alpha, srg = _attn_fwd(U, Vq, o.we, allf, seg, dB, cat[:, dv:] if cat is not None else None)
            if cat is None:
                cat = torch.empty(B, dv + D, device=dev, dtype=torch.float32)
                lib.srec_cat_cols(ptr(v), _ld(v), dv, ptr(srg), D, D, B, ptr(cat), stream())
            out = torch.empty(B, o.Wsr.shape[0], device=dev, dtype=torch.float32)
            probs.append(('nt', cat, o.Wsr, out, None, dB, 0.0))
            saved.append(HeadSaved(v, o.Wu, o.Wv, o.we, o.Wsr, U, Vq, alpha, cat))
            outs.append(out)
        gemm_f32_group(probs, split3=split3)
        ctx.save_for_backward(allf, seg, *[t for s in saved for t in s])
        ctx.dT, ctx.dB = dT, dB
        ctx.has_bu = [o.bu is not None for o in run]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        """-> (d allf, None, None, None, per order: d v, d Wu, d bu, d Wv, d we, d Wsr)"""
        allf, seg, per = _saved(ctx, HeadSaved)
        dT, dB = ctx.dT, ctx.dB
        NT, B, dev = allf.shape[0], per[0].v.shape[0], allf.device
        split3 = ops.PRECISION['matmul'] == 'bf16'
        gcats, gWsrs, probs = [], [], []
        for s, g in zip(per, gs):
            g = _rows(g)
            gcat, gWsr = torch.empty_like(s.cat), torch.empty_like(s.Wsr)
            probs.append(('nn', g, s.Wsr, gcat, None, dB, 0.0))
            probs.append(('tn', g, s.cat, gWsr, None, dB, 0.0))
            gcats.append(gcat)
            gWsrs.append(gWsr)
        gemm_f32_group(probs, split3=split3)
        probs, grads, dXs = [], [], []
        for s, gcat, gWsr, has_bu in zip(per, gcats, gWsrs, ctx.has_bu):
            dv = s.v.shape[1]
            dX, dU, dVq, dwp = _attn_bwd(gcat[:, dv:], allf, s.alpha, s.U, s.Vq, s.we, seg, dB)
            gWu, gWv = torch.empty_like(s.Wu), torch.empty_like(s.Wv)
            gv = gcat[:, :dv]                                             # d v: the concat half, + dVq Wv in place
            gbu, gwe, _ = tail_problems(probs, s, allf, dT, dB, _ones4(max(NT, B), dev), dU, dVq, dwp, dX, gv, gWu, gWv,
                                        bias=(NT, dU, dT) if has_bu else None)        # d bu = sum_n dU: over the node rows
            grads += [gv, gWu, gbu, gWv, gwe, gWsr]
            dXs.append(dX)
        launch_orders(probs, 6, split3)
        return (sum(dXs[1:], dXs[0]), None, None, None) + tuple(grads)


# ---- fused read-out head (csrc/headf.hip) ----------------------------------------------------------------------------------
_WF = {}    # _wf_key -> hi / lo fragment-major bf16 copy of this step (dropped by ops.weights_changed)


def _wf_key(w, trans):
    return (w.data_ptr(), tuple(w.shape), int(trans))


def wfrag_get(w, trans):
    return _WF.get(_wf_key(w, trans))


def wfrag_put(w, trans, buf):
    _WF[_wf_key(w, trans)] = buf
    return buf


def wfrag_missing(entries):
    """those of the [(W, trans)] entries this step has no copy of yet, as many as one launch takes"""
    return [(w, int(t)) for w, t in entries if wfrag_get(w, t) is None][:HEAD_MAXW]


def _head_wfrag_args(ws, trans):
    """output buffers + the HOST argument arrays of srec_head_wfrag for <= SREC_HEAD_MAXW weights (kept alive by the caller across the call)"""
    m = len(ws)
    assert 0 < m <= HEAD_MAXW
    for w in ws:
        assert w.is_contiguous() and w.dtype == torch.float32
    bufs = [torch.empty(2 * w.numel(), device=w.device, dtype=torch.bfloat16) for w in ws]
    ints = _ct.c_int * m
    return bufs, (ptr_array(ws), ptr_array(bufs), ints(*[w.shape[0] for w in ws]),
                  ints(*[w.shape[1] for w in ws]), ints(*[int(t) for t in trans]))


def head_wfrag(ws, trans):
    """hi / lo fragment-major bf16 operand copies of fp32 weights (W_i or W_i^T), computed once per optimizer step, all
    missing ones in ONE launch (srec_head_wfrag) - normally none: the step's prologue launch made them (ops.step_prologue)"""
    out = [wfrag_get(w, t) for w, t in zip(ws, trans)]
    todo = [i for i, c in enumerate(out) if c is None]
    for c0 in range(0, len(todo), HEAD_MAXW):
        ch = todo[c0:c0 + HEAD_MAXW]
        bufs, args = _head_wfrag_args([ws[i] for i in ch], [trans[i] for i in ch])
        lib.srec_head_wfrag(len(ch), *[_ct.addressof(a) for a in args], stream())
        for i, b in zip(ch, bufs):
            out[i] = wfrag_put(ws[i], trans[i], b)
    return out


def head_fwd_desc(allf, seg, dB, eps_mode, orders, wf, bufs, sr16=None):
    """the srec_head_desc of one forward launch; per order: its HeadOrder (we flat), wf = the (fc_u, fc_v, fc_sr) fragment
    copies, its HeadFwdBufs.  sr16: the bf16 operand copy of head 0's output, or None"""
    assert 0 < len(orders) <= HEAD_MAXH
    q = HeadDesc()
    NT, D = allf.shape
    q.nh, q.d, q.B, q.NT, q.ld_x, q.eps_mode, q.eps = len(orders), D, orders[0].v.shape[0], NT, _ld(allf), int(eps_mode), 1e-12
    q.X, q.seg, q.dynB = ptr(allf), ptr(seg), ptr(dB)
    q.ld16 = sr16.shape[1] if sr16 is not None else 0
    q.y16[0] = ptr(sr16)
    for i, (o, w, b) in enumerate(zip(orders, wf, bufs)):
        q.cat[i], q.Wu_f[i], q.Wv_f[i], q.Wsr_f[i] = ptr(b.cat), ptr(w[0]), ptr(w[1]), ptr(w[2])
        q.bu[i], q.we[i], q.alpha[i], q.U[i], q.Vq[i] = ptr(o.bu), ptr(o.we), ptr(b.alpha), ptr(b.U), ptr(b.Vq)
        q.y[i], q.inv[i] = ptr(b.y), ptr(b.inv)
    return q


def head_bwd_desc(allf, seg, dB, saved, wft, bufs):
    """the srec_head_bwd_desc of one backward launch; per order: its HeadSavedFused, wft = the fc_sr^T fragment copy, its
    HeadBwdBufs (every gy with the row stride of the first)"""
    assert 0 < len(saved) <= HEAD_MAXH
    q = HeadBwdDesc()
    NT, D = allf.shape
    q.nh, q.d, q.B, q.NT, q.ld_x, q.ld_gy = len(saved), D, saved[0].v.shape[0], NT, _ld(allf), _ld(bufs[0].gy)
    q.X, q.seg, q.dynB = ptr(allf), ptr(seg), ptr(dB)
    for i, (s, w, b) in enumerate(zip(saved, wft, bufs)):
        assert _ld(b.gy) == q.ld_gy
        q.gy[i], q.y[i], q.inv[i], q.WsrT_f[i], q.alpha[i] = ptr(b.gy), ptr(s.y), ptr(s.inv), ptr(w), ptr(s.alpha)
        q.U[i], q.Vq[i], q.we[i] = ptr(s.U), ptr(s.Vq), ptr(s.we)
        q.gs[i], q.gcat[i], q.dX[i], q.dU[i], q.dVq[i], q.dwp[i] = ptr(b.gs), ptr(b.gcat), ptr(b.dX), ptr(b.dU), ptr(b.dVq), ptr(b.dwp)
    return q


class ReadoutHeadFused(torch.autograd.Function):
    """ReadoutHead + the normalisation of its outputs (msgifsr.py:124-155, :269-273) with the FORWARD as one launch: a
    workgroup owns 8 sessions and runs Vq, U, the soft-max read-out, fc_sr and F.normalize on them, every product as a
    3-term hi / lo bf16 split on the matrix pipe (csrc/headf.hip; results to ~2^-16 of the exact-fp32 grouped head).
    Returns the NORMALISED session vectors; `ws` (CEWorkspace, optional) receives the bf16 operand copy of head 0.
    Backward: the normalisation backward + the grouped launches of ReadoutHead."""

    @staticmethod
    def forward(ctx, allf, seg, dT, dB, ws, eps_mode, *flat):
        given = _orders(flat)
        n = len(given)
        allf = _rows(allf)
        NT, D = allf.shape
        dev = allf.device
        run = [HeadOrder(o.v, _rows(o.Wu), o.bu, _rows(o.Wv), o.we.reshape(-1).contiguous(), _rows(o.Wsr)) for o in given]
        B = run[0].v.shape[0]
        # fragment-major hi / lo copies of fc_u, fc_v, fc_sr - and of fc_sr^T for the backward - in ONE launch per step
        need_bwd = any(ctx.needs_input_grad)
        wf = head_wfrag([w for o in run for w in (o.Wu, o.Wv, o.Wsr)] + ([o.Wsr for o in run] if need_bwd else []),
                        [0] * (3 * n) + ([1] * n if need_bwd else []))
        ctx.wft = wf[3 * n:] if need_bwd else None
        sr16 = getattr(ws, 'sr16', None) if n == 1 else None
        if sr16 is not None and not (B <= sr16.shape[0] and D <= sr16.shape[1]):
            sr16 = None
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        # cat: v is the left half of a private [B, 2 D] buffer (checked: readout_head_fused_ok)
        bufs = [HeadFwdBufs(o.v.as_strided((B, 2 * D), (2 * D, 1)), new(NT), new(NT, D), new(B, D), new(B, D), new(B)) for o in run]
        q = head_fwd_desc(allf, seg, dB, eps_mode, run, [wf[3 * i:3 * i + 3] for i in range(n)], bufs, sr16)
        lib.srec_head_fwd(_ct.addressof(q), stream())
        if sr16 is not None:
            sr16_written(ws, bufs[0].y, B, D)
        saved = [HeadSavedFused(o.v, o.Wu, o.Wv, o.we, o.Wsr, b.U, b.Vq, b.alpha, b.cat, b.y, b.inv) for o, b in zip(run, bufs)]
        ctx.save_for_backward(allf, seg, *[t for s in saved for t in s])
        ctx.dT, ctx.dB = dT, dB
        ctx.has_bu = [o.bu is not None for o in run]
        ctx.defer = defer_scope()
        ctx.wparams = [p for o in given for p in o[1:] if p is not None]
        return tuple(b.y for b in bufs)

    @staticmethod
    def backward(ctx, *gys):
        """one launch for everything per session (normalise-backward, d cat = g_s Wsr, the attention read-out backward:
        srec_head_bwd), then the batch-wide products as ONE grouped exact-fp32 launch + its split-K sum:
        d allf += dU Wu, d v += dVq Wv, d Wu, d Wv, d Wsr and the two column sums (d bu, d we)"""
        allf, seg, per = _saved(ctx, HeadSavedFused)
        dT, dB = ctx.dT, ctx.dB
        NT, D = allf.shape
        dev = allf.device
        B = per[0].v.shape[0]
        wft = ctx.wft if ctx.wft is not None else head_wfrag([s.Wsr for s in per], [1] * len(per))   # fc_sr^T [2 D, D], fragment-major
        new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        gy0 = _rows(gys[0])
        bufs = []
        for g in gys:
            gy = _rows(g)
            if _ld(gy) != _ld(gy0):
                gy = gy.contiguous() if _ld(gy0) == D else gy0.new_empty(B, _ld(gy0))[:, :D].copy_(gy)
            bufs.append(HeadBwdBufs(gy, new(B, D), new(B, 2 * D), new(NT, D), new(NT, D), new(B, D), new(B, D)))
        q = head_bwd_desc(allf, seg, dB, per, wft, bufs)
        lib.srec_head_bwd(_ct.addressof(q), stream())
        probs, grads, gws, blocks = [], [], [], []
        for s, b, has_bu in zip(per, bufs, ctx.has_bu):
            gWu, gWv, gWsr = grad_buf(s.Wu), grad_buf(s.Wv), grad_buf(s.Wsr)       # (bucket slots when the table is row-sharded)
            gv = b.gcat[:, :D]                                            # d v: the concat half, + dVq Wv in place
            gbu, gwe, bl = tail_problems(probs, s, allf, dT, dB, _ones4(B, dev), b.dU, b.dVq, b.dwp, b.dX, gv, gWu, gWv,
                                         wsr=(b.gs, s.cat, gWsr),
                                         bias=(B, b.dVq, dB) if has_bu else None)   # d bu = sum_n dU = sum_b dVq: over the sessions
            grads += [gv, gWu, gbu, gWv, gwe, gWsr]
            gws += [gWu, gWv, gWsr]
            blocks += bl
        later = gws + blocks if can_defer(ctx.defer, ctx.wparams) else None
        launch_orders(probs, 7, True, later)                              # (the forward's products are 3-term splits too)
        return (sum([b.dX for b in bufs[1:]], bufs[0].dX), None, None, None, None, None) + tuple(grads)


HEAD_FUSED_MAX_B = 8192      # session capacity of the fused read-out head kernels (csrc/headf.hip: srec_head_fwd / srec_head_bwd)


def head_path(d, n_heads, B, norm):
    """which head a model of n_heads live orders, hidden size d and session capacity B takes: 'fused' (ReadoutHeadFused: bf16
    mode, normalised outputs, d = hidden = output in (128, 256), <= SREC_HEAD_MAXH heads, 1 < B <= what the kernels keep of seg[]
    in LDS) or 'grouped' (ReadoutHead)"""
    fused = (ops.PRECISION['matmul'] == 'bf16' and norm and 1 <= n_heads <= HEAD_MAXH and d in (128, 256)
             and 1 < B <= HEAD_FUSED_MAX_B)
    return 'fused' if fused else 'grouped'


def readout_head_fused_ok(allf, per_order):
    """the fused forward applies to these tensors: head_path says 'fused', contiguous weights, every query tensor the tagged left
    half of a private [B, 2 d] buffer (norm_permute_pick / permute_and_pick)"""
    if not (allf.is_cuda and len(per_order) > 0):
        return False
    D, B = allf.shape[1], per_order[0][0].shape[0]
    if head_path(D, len(per_order), B, True) != 'fused' or allf.stride(1) != 1 or allf.stride(0) % 4:
        return False
    for v, Wu, bu, Wv, we, Wsr in per_order:
        if not (getattr(v, '_srec_cat_left', False) and tuple(v.shape) == (B, D) and v.stride(0) == 2 * D and v.stride(1) == 1):
            return False
        if tuple(Wu.shape) != (D, D) or tuple(Wv.shape) != (D, D) or tuple(Wsr.shape) != (D, 2 * D) or we.numel() != D:
            return False
        if not (Wu.is_contiguous() and Wv.is_contiguous() and Wsr.is_contiguous()):
            return False
    return True


def readout_head_fused(allf, seg, dT, dB, per_order, ws=None, eps_mode=0):
    """-> tuple of NORMALISED session vectors y_i [B, d] (ReadoutHeadFused)"""
    flat = [t for po in per_order for t in po]
    return ReadoutHeadFused.apply(allf, seg, dT, dB, ws, eps_mode, *flat)


def readout_head(allf, seg, dT, dB, per_order):
    """per_order: [(v_i, Wu_i, bu_i, Wv_i, we_i, Wsr_i)] -> tuple of s_i [B, d] (before the optional normalisation): the grouped
    exact-fp32 launches (ReadoutHead).  bf16 mode at d = 128 / 256 takes readout_head_fused instead."""
    flat = [t for po in per_order for t in po]
    return ReadoutHead.apply(allf, seg, dT, dB, *flat)
