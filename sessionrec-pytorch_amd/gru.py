"""The k-gram GRU of MSGIFSR's SemanticExpander (csrc/gru.hip, grux.hip, gruf.hip, grufb.hip around the GEMMs): the single-step
nodes, the per-order exact-fp32 node, the all-orders bf16 node with its descriptors, weight copies and path choice.
ops.py keeps the GEMM wrappers and the tests' switches (reached through the module object at call time) and re-exports this."""
import ctypes as _ct
from collections import namedtuple

import torch

from . import ops                    # (ops.py imports this module at its end: import the package or ops first, never gru alone)
from ._lib import lib, ptr, ptr_array, stream
from .ops import (G16_MAXP, GRU_MAXP, GemmProb, GruFusedBwdDesc, GruFusedDesc, GruStepDesc, _arena_rows, _arena_tag, _ld, _rows,
                  _wprep_take, can_defer, col_sum, defer_scope, defer_slab_sum, gemm16, gemm_nn, gemm_nt, gemm_tn, grad_buf,
                  grad_buf_pair, weights_bf16)


class GRUPointwise(torch.autograd.Function):
    """One GRU time step given the two projections (GI, GH); GH=None <=> h_prev = 0 (gh = b_hh)."""

    @staticmethod
    def forward(ctx, GI, GH, bhh, Hp, dyn):
        GI = _rows(GI)
        n, d3 = GI.shape
        d = d3 // 3
        dev = GI.device
        Hn = torch.empty(n, d, device=dev, dtype=torch.float32)
        gates = torch.empty(n, d3, device=dev, dtype=torch.float32)
        if GH is not None:
            GH, Hp = _rows(GH), _rows(Hp)
            lib.srec_gru_pointwise_fwd(ptr(GI), _ld(GI), ptr(GH), _ld(GH), None, ptr(Hp), _ld(Hp), n, ptr(dyn), d,
                                       ptr(Hn), d, ptr(gates), stream())
        else:
            bhh = bhh.contiguous()
            lib.srec_gru_pointwise_fwd(ptr(GI), _ld(GI), None, 0, ptr(bhh), None, 0, n, ptr(dyn), d, ptr(Hn), d,
                                       ptr(gates), stream())
        ctx.save_for_backward(gates, GH, bhh, Hp)
        ctx.dyn = dyn
        return Hn

    @staticmethod
    def backward(ctx, dHn):
        gates, GH, bhh, Hp = ctx.saved_tensors
        dHn = _rows(dHn)
        n, d3 = gates.shape
        d = d3 // 3
        dev = gates.device
        dGI = torch.empty(n, d3, device=dev, dtype=torch.float32)
        dGH = torch.empty(n, d3, device=dev, dtype=torch.float32)
        if GH is not None:
            dHp = torch.empty(n, d, device=dev, dtype=torch.float32)
            lib.srec_gru_pointwise_bwd(ptr(dHn), _ld(dHn), ptr(gates), ptr(GH), _ld(GH), None, ptr(Hp), _ld(Hp), n,
                                       ptr(ctx.dyn), d, ptr(dGI), d3, ptr(dGH), d3, ptr(dHp), d, stream())
            return dGI, dGH, None, dHp, None
        lib.srec_gru_pointwise_bwd(ptr(dHn), _ld(dHn), ptr(gates), None, 0, ptr(bhh), None, 0, n, ptr(ctx.dyn), d,
                                   ptr(dGI), d3, ptr(dGH), d3, None, 0, stream())
        db = torch.empty(d3, device=dev, dtype=torch.float32)
        col_sum(dGH, n, d3, db, ctx.dyn)
        return dGI, None, db, None, None


def gru_step(GI, GH, bhh, Hp, dyn=None):
    return GRUPointwise.apply(GI, GH, bhh, Hp, dyn)


class GramCombine(torch.autograd.Function):
    """0.5 * mean_t x[n,t,:] + 0.5 * h_last[n,:]"""

    @staticmethod
    def forward(ctx, X, Hl, k, dyn):
        X = X.contiguous()
        Hl = _rows(Hl)
        n, d = Hl.shape
        out = torch.empty(n, d, device=Hl.device, dtype=torch.float32)
        lib.srec_gram_combine_fwd(ptr(X), ptr(Hl), _ld(Hl), n, ptr(dyn), k, d, ptr(out), d, stream())
        ctx.k, ctx.dyn, ctx.xshape = k, dyn, tuple(X.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        g = _rows(g)
        n, d = g.shape
        dX = torch.empty(ctx.xshape, device=g.device, dtype=torch.float32)
        dH = torch.empty(n, d, device=g.device, dtype=torch.float32)
        lib.srec_gram_combine_bwd(ptr(g), _ld(g), n, ptr(ctx.dyn), ctx.k, d, ptr(dX), ptr(dH), d, stream())
        return dX, dH, None, None


def gram_combine(X, Hl, k, dyn=None):
    return GramCombine.apply(X, Hl, k, dyn)


class GRUExpand(torch.autograd.Function):
    """MSGIFSR SemanticExpander for one order k (msgifsr.py:32-45): out = 0.5 * mean_t x[n,t,:] + 0.5 * GRU(x).h_last,
    as ONE autograd node on stacked buffers: the time steps share [k, n, *] tensors, so the backward needs one
    weight-gradient GEMM and one bias column-sum for W_hh / b_hh over all steps, the hidden-state gradient is
    accumulated by the backward-data GEMM itself (beta = 1) and nothing goes through autograd's select / add kernels."""

    @staticmethod
    def forward(ctx, x, Wih, bih, Whh, bhh, k, dyn_n, dyn_rows, combine=True):
        x = x.contiguous()
        nk, d = x.shape
        n, d3 = nk // k, 3 * d
        dev = x.device
        Wih, Whh, bhh = _rows(Wih), _rows(Whh), bhh.contiguous()
        GI = torch.empty(nk, d3, device=dev, dtype=torch.float32)
        gemm_nt(x, Wih, GI, bih, dyn_rows, 1 if dyn_rows is not None else 0)
        H = torch.empty(k, n, d, device=dev, dtype=torch.float32)
        gates = torch.empty(k, n, d3, device=dev, dtype=torch.float32)
        GH = torch.empty(max(k - 1, 1), n, d3, device=dev, dtype=torch.float32)
        st = stream()
        for t in range(k):
            gi = GI.data_ptr() + 4 * t * d3                                   # GI[:, t, :], row stride k * 3d
            if t == 0:
                lib.srec_gru_pointwise_fwd(gi, k * d3, None, 0, ptr(bhh), None, 0, n, ptr(dyn_n), d, ptr(H[0]), d,
                                           ptr(gates[0]), st)
            else:
                gemm_nt(H[t - 1], Whh, GH[t - 1], bhh, dyn_n, 1 if dyn_n is not None else 0)
                lib.srec_gru_pointwise_fwd(gi, k * d3, ptr(GH[t - 1]), d3, None, ptr(H[t - 1]), d, n, ptr(dyn_n), d,
                                           ptr(H[t]), d, ptr(gates[t]), st)
        ctx.save_for_backward(x, Wih, Whh, bhh, H, gates, GH)
        ctx.k, ctx.dyn_n, ctx.dyn_rows, ctx.combine = k, dyn_n, dyn_rows, combine
        if not combine:                                   # 'max' / 'concat' reducers: only the GRU's last hidden state
            return H[k - 1].clone()
        out = torch.empty(n, d, device=dev, dtype=torch.float32)
        lib.srec_gram_combine_fwd(ptr(x), ptr(H[k - 1]), d, n, ptr(dyn_n), k, d, ptr(out), d, st)
        return out

    @staticmethod
    def backward(ctx, g):
        x, Wih, Whh, bhh, H, gates, GH = ctx.saved_tensors
        k, dyn_n, dyn_rows = ctx.k, ctx.dyn_n, ctx.dyn_rows
        g = _rows(g)
        n, d = g.shape
        d3, dev, st = 3 * d, g.device, stream()
        if ctx.combine:
            dX = torch.empty(n * k, d, device=dev, dtype=torch.float32)
            dh = torch.empty(n, d, device=dev, dtype=torch.float32)
            lib.srec_gram_combine_bwd(ptr(g), _ld(g), n, ptr(dyn_n), k, d, ptr(dX), ptr(dh), d, st)
        else:
            dX = torch.zeros(n * k, d, device=dev, dtype=torch.float32)
            dh = g.contiguous()
        # d(gi) and d(gh) side by side in ONE [n k, 2 d3] buffer: both bias gradients are then one column-sum launch.
        # d(gi) rows are (node, t) = node k + t; d(gh) slot t = rows [t n, (t+1) n).  The gate kernel writes every row of
        # both (zeros for nodes past the live count).
        dG = torch.empty(n * k, 2 * d3, device=dev, dtype=torch.float32)
        dGI = dG[:, :d3]
        dGH = [dG[t * n:(t + 1) * n, d3:] for t in range(k)]
        for t in range(k - 1, -1, -1):
            dgi = dG.data_ptr() + 4 * t * 2 * d3
            if t > 0:
                dhp = torch.empty(n, d, device=dev, dtype=torch.float32)
                lib.srec_gru_pointwise_bwd(ptr(dh), d, ptr(gates[t]), ptr(GH[t - 1]), d3, None, ptr(H[t - 1]), d, n,
                                           ptr(dyn_n), d, dgi, k * 2 * d3, ptr(dGH[t]), 2 * d3, ptr(dhp), d, st)
                gemm_nn(dGH[t], Whh, dhp, dyn_n, 1 if dyn_n is not None else 0, beta=1.0)      # dh_{t-1} += dgh_t W_hh
                dh = dhp
            else:
                lib.srec_gru_pointwise_bwd(ptr(dh), d, ptr(gates[0]), None, 0, ptr(bhh), None, 0, n, ptr(dyn_n), d,
                                           dgi, k * 2 * d3, ptr(dGH[0]), 2 * d3, None, 0, st)
        gWhh = torch.zeros_like(Whh) if k == 1 else torch.empty_like(Whh)
        if k > 1:
            gemm_tn(dG[n:, d3:], H[:k - 1].reshape((k - 1) * n, d), gWhh, None)
        gb = torch.empty(2 * d3, device=dev, dtype=torch.float32)
        col_sum(dG, n * k, 2 * d3, gb, None)
        gbih, gbhh = gb[:d3], gb[d3:]
        gemm_nn(dGI, Wih, dX, dyn_rows, 1 if dyn_rows is not None else 0, beta=1.0)             # + the mean term
        gWih = torch.empty_like(Wih)
        gemm_tn(dGI, x, gWih, dyn_rows)
        return dX, gWih, gbih, gWhh, gbhh, None, None, None, None


def gru_expand(x, gru, k, dyn_n=None, dyn_rows=None, combine=True):
    return GRUExpand.apply(x, gru.weight_ih_l0, gru.bias_ih_l0, gru.weight_hh_l0, gru.bias_hh_l0, k, dyn_n, dyn_rows, combine)


def _gru_wfrag_args(ws, backward=True):
    """buffers and HOST pointer arrays (W, forward[, backward] copies) of one fragment-copy launch: _wfrag's or step_prologue's"""
    of = [torch.empty(w.numel(), device=w.device, dtype=torch.bfloat16) for w in ws]
    ob = [torch.empty(w.numel(), device=w.device, dtype=torch.bfloat16) for w in ws] if backward else None
    return of, ob, (ptr_array(ws), ptr_array(of)) + ((ptr_array(ob),) if backward else ())


def _wfrag(ws, backward):
    """fragment-major bf16 copies of GRU weights [3 d, d] -> (the B operands of the fused forward, csrc/gruf.hip; those of the
    backward-data products, csrc/grufb.hip, or None), one launch - unless this forward pass's prologue made them (step_prologue)"""
    hit = [_wprep_take('gru', w) for w in ws]
    if all(h is not None for h in hit):
        return [h[0] for h in hit], [h[1] for h in hit] if backward else None
    of, ob, args = _gru_wfrag_args(ws, backward)
    launch = lib.srec_gru_wfrag_both if backward else lib.srec_gru_wfrag
    launch(len(ws), *[_ct.addressof(a) for a in args], ws[0].shape[1], stream())
    return of, ob


def gru_wfrag_both(ws):
    """-> (forward copies, backward copies) of the weights ws, see _wfrag"""
    return _wfrag(ws, True)


def gru_wfrag(ws):
    """-> forward copies of the weights ws, see _wfrag"""
    return _wfrag(ws, False)[0]


def gru_fused_ok(d, P):
    return d in (128, 256) and P <= GRU_MAXP and ops.FUSED_GRU


def gru_expand_fast_ok(d, reducer):
    return ops.PRECISION['matmul'] == 'bf16' and reducer == 'mean' and d % 64 == 0 and d <= 1024 and 256 % (d // 4) == 0


def expand_path(d, reducer, K):
    """how a model of n-gram order K expands its orders 2 .. K: None (GRUExpand per order), or all of them in one GRUExpandAll
    node, 'step' (one launch per time step) or 'fused' (one launch each way)"""
    if not (1 < K <= 5 and gru_expand_fast_ok(d, reducer)):
        return None
    return 'fused' if gru_fused_ok(d, K - 1) else 'step'


# one order of a GRUExpandAll call: n nodes of k rows each (live: *dyn_n nodes, *dyn_rows rows) and its GRU's parameters
GruOrder = namedtuple('GruOrder', 'k n dyn_n dyn_rows Wih bih Whh bhh')
# ctx.meta of GRUExpandAll.  orders hold the parameters AS GIVEN: the gradient targets (bucket slots when row-sharded);
# tags: the arena pieces the inputs are (their gradients go into that buffer) or None;  defer: defer_scope() of the forward
GruMeta = namedtuple('GruMeta', 'orders d fused tags defer')
# one order's tensors for gru_step_desc, whole: it takes the slices of step t.  dH / dHp: the d h_t read (not at t = k - 1) and the
# d h_{t-1} written (not at t = 0) by THIS step
StepFwd = namedtuple('StepFwd', 'GI GH H H16 gates X out')
StepBwd = namedtuple('StepBwd', 'gates H dout dX dGI16 dGH16 part dH dHp')


def _grouped(flat, n):          # [a0, b0, a1, b1, ...] -> [(a0, b0), (a1, b1), ...] for n = 2
    return list(zip(*[iter(flat)] * n))


def pieces(buf, row_counts):
    """the per-order row views of one buffer that holds the orders' rows one after the other"""
    return list(buf.split(list(row_counts)))


def gru_step_blocks(n, d):      # blocks of srec_gru_step_bwd (max(8, 1024 / d) nodes each): one partial bias row per block and step
    return -(-n // max(8, 1024 // d))


def _desc(struct, orders, d):   # a descriptor with its problem table filled: slot p = orders[p]
    assert 0 < len(orders) <= GRU_MAXP
    q = struct()
    q.np, q.d = len(orders), d
    for p, o in enumerate(orders):
        q.n[p], q.k[p], q.dyn[p] = o.n, o.k, ptr(o.dyn_n)
    return q


def gru_fused_desc(orders, d, X, X16, wf, H, H16, gates, out):
    """the srec_gru_fused_desc of one forward launch; per order: wf = (W_ih, W_hh) fragment-major copies, the rest one tensor"""
    q = _desc(GruFusedDesc, orders, d)
    for p, o in enumerate(orders):
        q.X[p], q.X16[p], q.Wih_f[p], q.Whh_f[p] = ptr(X[p]), ptr(X16[p]), ptr(wf[p][0]), ptr(wf[p][1])
        q.bih[p], q.bhh[p], q.H[p], q.H16[p] = ptr(o.bih), ptr(o.bhh), ptr(H[p]), ptr(H16[p])
        q.gates[p], q.out[p] = ptr(gates[p]), ptr(out[p])
    return q


def gru_fused_bwd_desc(orders, d, gates, H, dout, wt, dGI16, dGH16, dX, part):
    """the srec_gru_fused_bwd_desc of one backward launch; wt = (W_ih, W_hh) backward fragment copies per order"""
    q = _desc(GruFusedBwdDesc, orders, d)
    for p in range(len(orders)):
        q.gates[p], q.H[p], q.dout[p], q.Wih_f[p], q.Whh_f[p] = ptr(gates[p]), ptr(H[p]), ptr(dout[p]), ptr(wt[p][0]), ptr(wt[p][1])
        q.dGI16[p], q.dGH16[p], q.dX[p], q.bias_part[p], q.part_row0[p] = ptr(dGI16[p]), ptr(dGH16[p]), ptr(dX[p]), ptr(part[p]), 0
    return q


def gru_step_desc(active, t, d, backward=False):
    """the srec_gru_step_desc of time step t; active = [(GruOrder, StepFwd or StepBwd)] of the orders with k > t, in slot order"""
    q = _desc(GruStepDesc, [o for o, _ in active], d)
    for i, (o, b) in enumerate(active):
        last = t == o.k - 1
        q.t[i], q.gates[i] = t, ptr(b.gates[t])
        if t > 0:
            q.Hp[i] = ptr(b.H[t - 1])
        if not backward:
            q.GI[i], q.bih[i], q.bhh[i], q.Hn[i] = ptr(b.GI), ptr(o.bih), ptr(o.bhh), ptr(b.H[t])
            if t > 0:
                q.GH[i] = ptr(b.GH)
            if last:
                q.X[i], q.out[i] = ptr(b.X), ptr(b.out)
            else:
                q.Hn16[i] = ptr(b.H16[t])
            continue
        if last:
            q.dout[i], q.dX[i] = ptr(b.dout), ptr(b.dX)
        else:
            q.dH[i] = ptr(b.dH)
        if t > 0:
            q.dGH16[i], q.dHp[i] = ptr(b.dGH16[t - 1]), ptr(b.dHp)                               # dGH16: slot t - 1
        q.dGI16[i], q.bias_part[i], q.part_row0[i] = ptr(b.dGI16), ptr(b.part), t * gru_step_blocks(o.n, d)
    return q


def _saved(ctx):
    """ctx.saved_tensors of GRUExpandAll -> (x16, H, H16, gates, wt), one entry per order; wt[p] = the bf16 (W_ih, W_hh) copies
    the backward-data products read: transposed (step path) or fragment-major (fused path)"""
    sv, P = ctx.saved_tensors, len(ctx.meta.orders)
    return (*(sv[i * P:(i + 1) * P] for i in range(4)), _grouped(sv[4 * P:], 2))


class GRUExpandAll(torch.autograd.Function):
    """SemanticExpander (msgifsr.py:32-45, reducer 'mean') for ALL orders k >= 2 of a batch as one autograd node on the bf16
    path (csrc/grux.hip + csrc/gemm16.hip): one grouped GEMM and one fused gate kernel per time step serve every order;
    in the backward the hidden-state gradient is accumulated by the backward-data GEMM itself (beta = 1), the bias
    gradients come from per-block partial sums of the gate kernels, the weight gradients from row-split products."""

    @staticmethod
    def forward(ctx, ks, dyn_ns, dyn_rows, *args):
        P = len(ks)
        xs = [a.contiguous() for a in args[:P]]
        d = xs[0].shape[1]
        d3, dev, st = 3 * d, xs[0].device, stream()
        orders = [GruOrder(k, x.shape[0] // k, dn, dr, *w)
                  for k, x, dn, dr, w in zip(ks, xs, dyn_ns, dyn_rows, _grouped(args[P:], 4))]
        fused = gru_fused_ok(d, P)
        ctx.meta = GruMeta(orders, d, fused, [_arena_tag(a) for a in args[:P]], defer_scope())
        run = [GruOrder(*o[:4], *(w.contiguous() for w in o[4:])) for o in orders]        # ... as the kernels read them
        ws = [w for o in run for w in (o.Wih, o.Whh)]
        # bf16 (W_ih, W_hh) per order, wf for this pass and wt for the backward: fragment-major when fused, else plain / transposed
        wf, wt = (_grouped(c or (), 2) for c in (_wfrag(ws, any(ctx.needs_input_grad)) if fused else weights_bf16(ws)))
        H = [torch.empty(o.k, o.n, d, device=dev, dtype=torch.float32) for o in run]
        H16 = [torch.empty(max(o.k - 1, 1), o.n, d, device=dev, dtype=torch.bfloat16) for o in run]
        # saved gates: fp16 on the fused path (values in [-1, 1] and gh_n; half the bytes of the expander's largest tensor)
        gates = [torch.empty(o.k, o.n, 4 * d, device=dev, dtype=torch.float16 if fused else torch.float32) for o in run]
        outs = [torch.empty(o.n, d, device=dev, dtype=torch.float32) for o in run]
        rows = [x.shape[0] for x in xs]
        x16all = torch.empty(sum(rows), d, device=dev, dtype=torch.bfloat16)
        x16 = pieces(x16all, rows)
        if fused:
            # the whole recurrence in one launch (csrc/gruf.hip): a workgroup owns 32 nodes, the weights stream from L2; writes x16
            q = gru_fused_desc(run, d, xs, x16, wf, H, H16, gates, outs)
            lib.srec_gru_fused_fwd(_ct.addressof(q), st)
        else:
            # bf16 copy of the gathered rows: one pass when the orders' rows are adjacent pieces of one buffer
            if all(b.data_ptr() == a.data_ptr() + a.numel() * a.element_size() for a, b in zip(xs, xs[1:])):
                lib.srec_rows_bf16(ptr(xs[0]), d, sum(rows), None, d, ptr(x16all), st)
            else:
                for x, o in zip(xs, x16):
                    lib.srec_rows_bf16(ptr(x), d, x.shape[0], None, d, ptr(o), st)
            GI = [torch.empty(r, d3, device=dev, dtype=torch.float32) for r in rows]
            gemm16('nt', [(rows[p], d3, d, [(x16[p], wf[p][0])], GI[p], o.dyn_rows) for p, o in enumerate(run)], d, d, d3,
                   keep_dead=True)
            GH = [torch.empty(o.n, d3, device=dev, dtype=torch.float32) for o in run]
            bufs = [StepFwd(GI[p], GH[p], H[p], H16[p], gates[p], xs[p], outs[p]) for p in range(P)]
            for t in range(max(ks)):
                act = [p for p in range(P) if t < ks[p]]
                if t > 0:
                    gemm16('nt', [(run[p].n, d3, d, [(H16[p][t - 1], wf[p][1])], GH[p], run[p].dyn_n) for p in act], d, d, d3,
                           keep_dead=True)
                q = gru_step_desc([(run[p], bufs[p]) for p in act], t, d)
                lib.srec_gru_step_fwd(_ct.addressof(q), st)
        ctx.save_for_backward(*x16, *H, *H16, *gates, *(w for pair in wt for w in pair))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        orders, d, fused, tags, _ = ctx.meta
        P = len(orders)
        x16, H, H16, gates, wt = _saved(ctx)
        d3, dev, st = 3 * d, H[0].device, stream()
        gs = [g.contiguous() if g is not None else torch.zeros(o.n, d, device=dev) for o, g in zip(orders, gs)]
        rows = [o.n * o.k for o in orders]
        if all(t is not None for t in tags):
            dX = [_arena_rows(t, r, d, dev) for t, r in zip(tags, rows)]
        else:
            dX = pieces(torch.empty(sum(rows), d, device=dev, dtype=torch.float32), rows)
        dGI16 = [torch.empty(r, d3, device=dev, dtype=torch.bfloat16) for r in rows]
        dGH16 = [torch.empty(max(o.k - 1, 1), o.n, d3, device=dev, dtype=torch.bfloat16) for o in orders]   # slot t - 1
        if fused:
            # every time step of every order in one launch (csrc/grufb.hip); wt = the fragment-major weights here
            nr, ns_c = _ct.c_int(0), (_ct.c_int * P)(*[o.n for o in orders])
            lib.srec_gru_fused_nodes(P, _ct.addressof(ns_c), d, _ct.addressof(nr))  # nodes per workgroup: one partial bias row each
            part = [torch.empty(-(-o.n // nr.value), 6 * d, device=dev, dtype=torch.float32) for o in orders]
            q = gru_fused_bwd_desc(orders, d, gates, H, gs, wt, dGI16, dGH16, dX, part)
            lib.srec_gru_fused_bwd(_ct.addressof(q), st)
        else:
            part = [torch.empty(o.k * gru_step_blocks(o.n, d), 6 * d, device=dev, dtype=torch.float32) for o in orders]
            dH = {}
            for t in range(max(o.k for o in orders) - 1, -1, -1):
                act = [p for p in range(P) if t < orders[p].k]
                dHp = {p: torch.empty(orders[p].n, d, device=dev, dtype=torch.float32) for p in act} if t > 0 else {}
                bufs = [StepBwd(gates[p], H[p], gs[p], dX[p], dGI16[p], dGH16[p], part[p], dH.get(p), dHp.get(p)) for p in act]
                q = gru_step_desc([(orders[p], b) for p, b in zip(act, bufs)], t, d, backward=True)
                lib.srec_gru_step_bwd(_ct.addressof(q), st)
                if t > 0:          # d h_{t-1} += d(gh_t) W_hh
                    gemm16('nt', [(orders[p].n, d, d3, [(dGH16[p][t - 1], wt[p][1])], dHp[p], orders[p].dyn_n) for p in act],
                           d3, d3, d, beta=1.0)
                dH = dHp               # (an order that joins at a smaller t starts from its dout)
            # d x += d(gi) W_ih  (onto the mean term the last-step kernels wrote)
            gemm16('nt', [(rows[p], d, d3, [(dGI16[p], wt[p][0])], dX[p], o.dyn_rows) for p, o in enumerate(orders)], d3, d3, d,
                   beta=1.0)
        return GRUExpandAll._weight_grads(ctx, x16, H16, dGI16, dGH16, part, dX)

    @staticmethod
    def _weight_grads(ctx, x16, H16, dGI16, dGH16, part, dX):
        orders, d, defer = ctx.meta.orders, ctx.meta.d, ctx.meta.defer
        P = len(orders)
        d3, dev, st = 3 * d, dX[0].device, stream()
        # weight gradients: the reduction runs over rows - split in-kernel into ~512-row pieces (hundreds of short workgroups
        # instead of a dozen long ones), each writing its own slab; the slabs are summed in fixed order
        probs, slabs = [], []
        gWih = [grad_buf(o.Wih) for o in orders]
        gWhh = [grad_buf(o.Whh) for o in orders]
        for p, o in enumerate(orders):
            hh = [(dGH16[p][t - 1], H16[p][t - 1]) for t in range(1, o.k)]
            for gW, nrow, segs, dyn in ((gWih[p], o.n * o.k, [(dGI16[p], x16[p])], o.dyn_rows), (gWhh[p], o.n, hh, o.dyn_n)):
                nsp = max(1, (nrow + 511) // 512)
                sl = torch.empty(nsp, d3, d, device=dev, dtype=torch.float32) if nsp > 1 else gW.unsqueeze(0)
                probs.append(GemmProb(d3, d, nrow, segs, sl, dyn, nsplit=nsp, ld=(d3, d, d)))
                if nsp > 1:
                    slabs.append((sl, gW))
        if ops.WGRAD_ONE_LAUNCH and len(probs) <= G16_MAXP:
            # ... and the MSHGNN layers' weight-gradient products that wait (ops.STEP) leave in this launch as its other family
            ops.STEP.leave_with(probs, G16_MAXP)
        else:
            for i in range(0, len(probs), G16_MAXP):
                gemm16('tn', probs[i:i + G16_MAXP], d3, d, d)
        gb = [grad_buf_pair(o.bih, o.bhh) for o in orders]
        # the weight-gradient slab sums join the ONE end-of-backward launch (defer_slab_sum); the bias partials keep their own
        # kernel: hundreds of partial rows of only 6 d columns - as a task of the generic slab sum (one thread per 4 columns
        # walking all rows) they made that launch 44 us (profiles/r03d), gru_bias_final splits the rows over 16 lanes: 5 us
        ok = can_defer(defer, [w for o in orders for w in (o.Wih, o.Whh)])
        for sl, o_ in slabs:
            defer_slab_sum(sl, o_, ok)
        if ok and can_defer(defer, [b for o in orders for b in (o.bih, o.bhh)]):
            # ... and so do the bias partials (hundreds of rows of 6 d columns: the "tall" tasks of srec_sum_slabs_multi)
            for p in range(P):
                defer_slab_sum(part[p], gb[p], True, tall=True)
        else:
            a_p, a_o = ptr_array(part), ptr_array(gb)
            a_r = (_ct.c_int * P)(*[t_.shape[0] for t_ in part])
            lib.srec_gru_bias_final(P, _ct.addressof(a_p), _ct.addressof(a_r), 6 * d, _ct.addressof(a_o), st)
        grads = [g for p in range(P) for g in (gWih[p], gb[p][:d3], gWhh[p], gb[p][d3:])]
        return (None, None, None) + tuple(dX) + tuple(grads)


def gru_expand_all(xs, grus, ks, dyn_ns, dyn_rows):
    """xs[i]: [N_k k, d] gathered rows of order ks[i] (>= 2) -> [N_k, d] expander outputs, all orders in one node"""
    params = [w for g in grus for w in (g.weight_ih_l0, g.bias_ih_l0, g.weight_hh_l0, g.bias_hh_l0)]
    return GRUExpandAll.apply(tuple(ks), tuple(dyn_ns), tuple(dyn_rows), *xs, *params)
