"""The batched MSHGNN layer (csrc/hgat.hip around the fc GEMMs): its static plan, the autograd node and the glue between them.
ops.py keeps the GEMM wrappers and the tests' switches (reached through the module object at call time) and re-exports this."""
import ctypes as _ct
from collections import namedtuple

import torch

from . import ops                    # (ops.py imports this module at its end: import the package or ops first, never hgat alone)
from ._lib import CONST, lib, ptr, ptr_array, stream
from .ops import GemmProb, HgDesc, _ld, _rows

# dropout state of one call.  xc [2, NT, D]: dropped inputs of conv1 / conv2;  xres [NT, D]: residual rows summed over the instances;
# mk: attention masks per instance or None;  ms: feature masks, kept for the tests' tap only;  rng = (p, seed, counter, salt)
DropState = namedtuple('DropState', 'xc xres mk ms rng cnt')
# entry record of a layer call: x = the L2-normalised rows of one raw tensor per node type (what ops.normalize_stack would hand over).
# raws [n_types] tensors [ncap_t, D];  dyns: their live counts;  eps_mode of ops.normalize
NormEntry = namedtuple('NormEntry', 'raws dyns eps_mode')
# exit record: the layer's output goes on as ops.norm_permute_pick(out, ...) would hand it over.  cat_perm [n_cat] concatenated row ->
# stacked row, cat_inv [NT] its inverse (-1: capacity padding), cat_seg [B + 1];  picks: [B] stacked rows per pick list;  types
# [(row0, ncap, dyn)];  dyn_t / dyn_b: live concatenated rows / sessions
NormExit = namedtuple('NormExit', 'cat_perm cat_inv cat_seg picks types dyn_t dyn_b eps_mode')
FOLD_A, FOLD_B, FOLD_C, FOLD_D = 1, 2, 4, 8          # entry forward, exit forward, exit backward, entry backward (ops.NORM_FOLD)
FOLDS_BUILT = FOLD_A | FOLD_B | FOLD_C | FOLD_D      # (a fold without a kernel would be masked out here)


def norm_fold_bits(mask, H, D, inst_per_type, has_entry, has_exit, p_feat, p_attn, tap_on):
    """the normalisation folds a layer call takes (bits FOLD_*), like head_path / readout_head_fused_ok: one place decides.
    The hosts are the node kernels (H == 8, <= 8 relation instances into every type, 8-column lanes) with one wavefront per row
    (D <= 256).  Entry folds ride in the dropout launches: A needs a dropout launch (p_feat or p_attn > 0), D the one-pass d x of a
    feature-dropout call with recomputed masks (the tap off)."""
    node = H == 8 and D % 8 == 0 and 0 < D <= 256 and len(inst_per_type) > 0 and 0 < max(inst_per_type) <= 8
    bits = 0
    if node and has_entry and (p_feat > 0 or p_attn > 0):
        bits |= FOLD_A | (0 if tap_on else FOLD_D)
    if node and has_exit:
        bits |= FOLD_B | FOLD_C
    return bits & mask & FOLDS_BUILT


class HgPlan:
    """Static topology of one MSHGNN layer call (built by msgifsr.MSHGNN from the FlatBatch).
    types:   [(row0, ncap, dyn_n, seg)]                          node types, stacked rows
    modules: [(row_start, n_rows, dyn)]                          rows of x each GAT module projects (dyn or None)
    blocks:  [(module, type)]                                    projection blocks
    insts:   [(module, src_block, dst_block, (in_ptr, in_idx, out_ptr, out_idx, esrc, edst))]
    mod_conv: per module 0 (conv1) or 1 (conv2, reversed graph);  layer_id: dropout-mask salt, distinct per MSHGNN layer of a
    model;  live: {first stacked row of a type: host-side live row count} - hints for the GEMM tile heuristics only"""

    def __init__(self, H, D, slope, B, dynB, types, modules, blocks, insts, mod_conv=None, layer_id=0, live=None):
        self.mod_conv = mod_conv if mod_conv is not None else [0] * len(modules)
        self.layer_id, self.live = layer_id, dict(live or {})
        self.H, self.D, self.slope, self.B, self.dynB = H, D, slope, B, dynB
        self.types, self.modules, self.blocks, self.insts, self._fold = types, modules, blocks, insts, None
        assert (len(types) <= CONST['SREC_HG_MAXT'] and len(modules) <= CONST['SREC_HG_MAXM'] and
                len(blocks) <= CONST['SREC_HG_MAXB'] and len(insts) <= CONST['SREC_HG_MAXI'])

    def put_fold(self, small, lay):          # ops.step_prologue folded the weights into this scratch: the next forward takes it
        self._fold = (small, lay)

    def take_fold(self):
        fold, self._fold = self._fold, None
        return fold

    def pieces(self, m):
        """[(row offset inside module m's projection, first stacked row, rows, dyn)] per node type the module covers: GEMM problems
        are cut at type boundaries, so every piece has its own live row count (the shared 'inter' module spans all types)"""
        r0, nr, dyn = self.modules[m]
        out = [(t0 - r0, t0, nc, dyn_t) for (t0, nc, dyn_t, _) in self.types if r0 <= t0 and t0 + nc <= r0 + nr]
        assert sum(p[2] for p in out) == nr, 'a module projects whole node types'
        return out

    def projectors(self, cv, t):
        """the modules of conv cv (None: either conv) that project node type t for some relation instance"""
        t0, nc = self.types[t][:2]
        return [m for m, (r0, nr, _) in enumerate(self.modules)
                if (cv is None or self.mod_conv[m] == cv) and r0 <= t0 and t0 + nc <= r0 + nr
                and any(bm == m and bt == t for bm, bt in self.blocks)]

    def scratch(self, dev):
        """-> (fp32 tensor, offsets) of the small per-call scratch: eL,eR,wL,wR per block; V,Z per module; A,DP,der per instance;
        the live-source row list of every block and their counts (int32, live_rows)"""
        H, ncap = self.H, [tp[1] for tp in self.types]
        sizes = [((nm, b), ncap[t] * H) for b, (m, t) in enumerate(self.blocks) for nm in ('eL', 'eR', 'wL', 'wR')]
        # (Z slot t < n_types also holds the summed bias row of node type t during the forward: slots for max(modules, types))
        sizes += [((nm, m), 2 * self.D * H) for m in range(max(len(self.modules), len(ncap))) for nm in ('V', 'Z')]
        for i, (m, sb, db, gr) in enumerate(self.insts):
            E = max(gr[4].numel(), 1) * H
            sizes += [(('A', i), E), (('DP', i), E), (('der', i), ncap[self.blocks[db][1]] * H)]
        sizes += [(('smean', t), self.B * self.D) for t in range(len(ncap))]       # session means of the input rows per type [B, D]
        sizes.append((('sess', 0), sum(ncap)))                                     # session of every stacked row (int32)
        sizes += [(('live', b), max(ncap[t], 1)) for b, (m, t) in enumerate(self.blocks)]
        sizes.append((('nlive', 0), max(len(self.blocks), 1)))
        off, lay = 0, {}
        for key, n in sizes:
            lay[key] = off
            off += n
        return torch.empty(max(off, 1), device=dev, dtype=torch.float32), lay

    def live_rows(self, small, lay):
        """-> ([int32 row list per projection block], int32 counts [n_blocks]) inside the scratch: the type-local rows of the block
        that some edge reads as its source, ascending (srec_hg_live_rows) - the only rows of P anybody reads"""
        i32 = small.view(torch.int32)
        lists = [i32[lay[('live', b)]:][:max(self.types[t][1], 1)] for b, (m, t) in enumerate(self.blocks)]
        return lists, i32[lay[('nlive', 0)]:][:len(self.blocks)]

    def fill_drop(self, d, drop):                          # (d.rm stays NULL: srec_hg_bwd recomputes it from the masks' hash)
        for m in range(len(self.modules)):
            d.xin[m] = ptr(drop.xc[self.mod_conv[m]])
        d.xres, d.rm_cnt = ptr(drop.xres), ptr(drop.cnt)
        d.rm_p, d.rm_seed, d.rm_counter, d.rm_salt = drop.rng
        for i in range(len(self.insts)):
            d.Mk[i] = ptr(drop.mk[i]) if drop.mk is not None else None

    def fill(self, d, small, lay, P, dP, params, grads, drop=None):
        if drop is not None:
            self.fill_drop(d, drop)
        d.H, d.D, d.slope, d.B, d.dynB = self.H, self.D, self.slope, self.B, ptr(self.dynB)
        d.p16 = CONST['SREC_HG_P16_BF16'] if P and P[0].dtype == torch.bfloat16 else 0      # (P = None: the view srec_hg_fold reads)
        d.n_types, d.n_mods, d.n_blocks, d.n_inst = len(self.types), len(self.modules), len(self.blocks), len(self.insts)
        base = small.data_ptr()
        for t, (r0, nc, dyn, seg) in enumerate(self.types):
            d.row0[t], d.ncap[t], d.dyn_n[t], d.seg[t] = r0, nc, ptr(dyn), ptr(seg)
            d.smean[t], d.Z[t] = base + 4 * lay[('smean', t)], base + 4 * lay[('Z', t)]
        for m in range(len(self.modules)):
            W, al, ar, bias = params[4 * m:4 * m + 4]
            d.P[m], d.W[m] = ptr(P[m]) if P else None, ptr(W)
            d.V[m], d.Z[m] = base + 4 * lay[('V', m)], base + 4 * lay[('Z', m)]
            d.attn_l[m], d.attn_r[m], d.bias[m] = ptr(al), ptr(ar), ptr(bias)
            if dP is not None:
                d.dP[m] = ptr(dP[m])
                d.d_attn_l[m], d.d_attn_r[m], d.d_bias[m] = (grads[m][j].data_ptr() for j in range(3))
        d.sess = base + 4 * lay[('sess', 0)]
        for b, (m, t) in enumerate(self.blocks):
            d.blk_mod[b], d.blk_type[b] = m, t
            d.blk_row[b] = self.types[t][0] - self.modules[m][0]
            for nm in ('eL', 'eR', 'wL', 'wR'):
                getattr(d, nm)[b] = base + 4 * lay[(nm, b)]
        for i, (m, sb, db, gr) in enumerate(self.insts):
            d.inst_mod[i], d.inst_sblk[i], d.inst_dblk[i] = m, sb, db
            for nm, g in zip(('in_ptr', 'in_idx', 'out_ptr', 'out_idx', 'esrc', 'edst'), gr):
                getattr(d, nm)[i] = ptr(g)
            for nm in ('A', 'DP', 'der'):
                getattr(d, nm)[i] = base + 4 * lay[(nm, i)]
        return d


_HG_WS = {}
_CNT_CACHE = {}


def _inst_counts(plan, NT, dev):
    """[2, NT, 1]: how many relation instances of conv1 / conv2 use each stacked row as a DESTINATION (identity residual
    count, gatconv.py:306-308) - a function of the plan's static topology"""
    key = (str(dev), NT, tuple(plan.mod_conv), tuple((m, tuple(plan.types[plan.blocks[db][1]][:2])) for (m, sb, db, gr) in plan.insts))
    cnt = _CNT_CACHE.get(key)
    if cnt is None:
        host = torch.zeros(2, NT, 1)
        for (m, sb, db, gr) in plan.insts:
            t0, nc = plan.types[plan.blocks[db][1]][:2]
            host[plan.mod_conv[m], t0:t0 + nc] += 1.0
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('instance counts must be cached by an eager warm-up step before graph capture')
        cnt = _CNT_CACHE[key] = host.to(dev)
    return cnt


def gemm_strategy(mode, D, ldx, n_mods, w_contiguous):
    """which GEMMs compute the projections and their gradients, decided once per layer call.  'g16': every operand bf16 in HBM
    (ops.gemm16);  'grouped': fp32 operands converted on the way, one launch per product kind (ops.gemm_group) - both STORE the
    projections as bf16;  'plain': one fp32-in / fp32-out product per module (ops.gemm_nt / gemm_nn / gemm_tn)."""
    if mode != 'bf16' or D % 8 or ldx != D or not 0 < n_mods <= 8:          # (no module: no GEMM)
        return 'plain'
    return 'g16' if D % 64 == 0 and w_contiguous else 'grouped'


def _drop_prep(x, plan, drop, strategy, live=None, norm=None):
    """-> (DropState, x16 or None): both convs' feature masks and every instance's attention mask in ONE launch (counter-based
    hash: no generator state, replay-safe); the 'g16' strategy reads bf16(xc), written by the same pass.  live = (desc, lists,
    counts): the live-source row lists of the call ride in the same launch ('g16' only).  norm = (NormEntry, inv): x is still
    unwritten - the launch forms it (and inv) from the entry record's raw rows first (fold A)"""
    (pf, pa), (NT, D), dev, tap = drop, x.shape, x.device, ops.DROP_TAP
    cnt = _inst_counts(plan, NT, dev)                     # (depends on the plan only: cached)
    ms = torch.empty(2, NT, D, device=dev, dtype=torch.float32) if tap is not None else None
    xcs, xres = torch.empty(2, NT, D, device=dev, dtype=torch.float32), torch.empty(NT, D, device=dev)
    sizes = [max(gr[4].numel(), 1) * plan.H for (_, _, _, gr) in plan.insts] if pa > 0 else []
    na = sum(sizes)
    allm = torch.empty(na, device=dev, dtype=torch.float32) if pa > 0 else None
    mk = list(torch.split(allm, sizes)) if pa > 0 else None
    seed, rc = ops.rng_args(dev)
    salt = 101 + 2 * plan.layer_id                        # (rm = cnt0 m0 + cnt1 m1 is never stored: NULL, the backward recomputes it)
    args = (ptr(x), ptr(cnt), NT, D, float(pf), seed, rc, salt, ptr(ms), ptr(xcs), None, ptr(xres), float(pa), na, ptr(allm))
    x16 = torch.empty(2, NT, D, device=dev, dtype=torch.bfloat16) if strategy == 'g16' else None
    if norm is not None:
        entry, inv = norm
        a_x, a_l, a_n, a_d = _group_arrays(entry.raws, entry.dyns)
        use_live = x16 is not None and live is not None
        la = ptr_array(live[1]) if use_live else None
        lib.srec_hg_drop_prep_norm(len(entry.raws), _ct.addressof(a_x), _ct.addressof(a_l), _ct.addressof(a_n), _ct.addressof(a_d),
                                   ptr(x), ptr(inv), entry.eps_mode, 1e-12, *args[1:], ptr(x16),
                                   _ct.addressof(live[0]) if use_live else None, _ct.addressof(la) if use_live else None,
                                   ptr(live[2]) if use_live else None, stream())
    elif x16 is not None and live is not None:
        la = ptr_array(live[1])
        lib.srec_hg_drop_prep16_live(*args, ptr(x16), _ct.addressof(live[0]), _ct.addressof(la), ptr(live[2]), stream())
    elif x16 is not None:
        lib.srec_hg_drop_prep16(*args, ptr(x16), stream())
    else:
        lib.srec_hg_drop_prep(*args, stream())
    if tap is not None:
        tap.append(dict(ms=ms.clone(), mk=[m.clone() for m in mk] if mk is not None else None))
    return DropState([xcs[0], xcs[1]], xres, mk, ms, (float(pf), seed, rc, salt), cnt), x16


def _group_arrays(xs, dyns, lds=None):
    """HOST arrays (pointers, row strides, rows, live counts) of a row-block group: srec_normalize_group_* and the folds' records"""
    P = len(xs)
    arr = _ct.c_void_p * P
    return (arr(*[x.data_ptr() for x in xs]), (_ct.c_int * P)(*(lds or [_ld(x) for x in xs])), (_ct.c_int * P)(*[x.shape[0] for x in xs]),
            arr(*[ptr(t) for t in dyns]))


def _project(xin, x16, plan, params, strategy, P, live=None):
    """P[m] = xin[m][rows of m] fc_m^T for every module -> (bf16 inputs per module, wt16): what the 'g16' backward reads, or None.
    live = (lists, counts) of HgPlan.live_rows ('g16'): only the listed rows of a projection block are computed and written"""
    D, HD, nm = plan.D, plan.H * plan.D, len(plan.modules)
    if strategy == 'g16':
        # the small weights as bf16 once per call (+ transposed copies for the backward-data product)
        w16, wt16 = ops.weights_bf16([params[4 * m] for m in range(nm)])
        xin16 = [x16[cv] for cv in plan.mod_conv] if x16 is not None else [ops.rows_bf16(xin[0])] * nm
        type_of = {tp[0]: t for t, tp in enumerate(plan.types)}
        probs = []
        for m in range(nm):
            for (o, t0, nc, dyn_t) in plan.pieces(m):
                rows = None
                if live is not None and (m, type_of[t0]) in plan.blocks:      # (a piece no instance uses keeps the dense product)
                    b = plan.blocks.index((m, type_of[t0]))
                    rows, dyn_t = live[0][b], live[1][b:b + 1]
                probs.append(GemmProb(nc, HD, D, [(xin16[m][t0:t0 + nc], w16[m])], P[m][o:o + nc], dyn_t,
                                      mhint=plan.live.get(t0, 0), rows=rows))
        for i in range(0, len(probs), ops.G16_MAXP):
            # rows past a type's live count are never read (every hgat.hip kernel walks the live prefix only), and of the live
            # rows only those some edge reads as its source (MSHGNN layer: who reads P)
            ops.gemm16('nt', probs[i:i + ops.G16_MAXP], D, D, HD, c16=True, keep_dead=True)
        return xin16, wt16
    if strategy == 'grouped':
        ops.gemm_group(0, [(nr, HD, D, [(xin[m][r0:r0 + nr], params[4 * m])], P[m], dyn)
                           for m, (r0, nr, dyn) in enumerate(plan.modules)], D, D, HD, c16=True)
    else:
        for m, (r0, nr, dyn) in enumerate(plan.modules):
            ops.gemm_nt(xin[m][r0:r0 + nr], _rows(params[4 * m]), P[m], None, dyn, 1 if dyn is not None else 0)
    return None


def _backward_graph(ctx, x, g, small, arg, P, params, late_dx, xrec=None, need_dx=True):
    """srec_hg_bwd: the graph kernels' half of the backward -> (desc, dP, [attn_l, attn_r, bias gradients per module], dx).
    xrec = (cat_inv, allf, invr, g_allf, picks, g_picks): g is still unwritten - the score-gradient launch forms it (fold C);
    need_dx False (a late_dx call whose d x leaves through the entry normalisation, fold D): no stacked dx, None"""
    plan, nm = ctx.plan, len(ctx.plan.modules)
    # rows of a module's projection that no relation instance touches (a type without live 'inter' edges) get no
    # gradient from the kernels: those buffers start from zero
    cov = [sum(plan.types[bt][1] for bm, bt in plan.blocks if bm == m) for m in range(nm)]
    dP = [torch.empty_like(p) if cov[m] == p.shape[0] else torch.zeros_like(p) for m, p in enumerate(P)]
    # (attn_l, attn_r, bias gradients: [HD] each - the parameters' bucket slots when the table is row-sharded, ops.grad_buf)
    grads = [[ops.grad_buf(params[4 * m + 1 + j]).view(-1) for j in range(3)] for m in range(nm)]
    dx = torch.empty(x.shape, device=x.device, dtype=torch.float32) if need_dx else None
    flat = [p.reshape(-1) if i % 4 else p for i, p in enumerate(params)]
    desc = plan.fill(HgDesc(), small, ctx.lay, P, dP, flat, grads, ctx.drop)
    # (both gemm16 consumers of dP stop at the live rows)
    desc.p16 |= (CONST['SREC_HG_SKIP_DEAD_DP'] if ctx.strategy == 'g16' else 0) | (CONST['SREC_HG_LATE_DX'] if late_dx else 0)
    n = _ct.c_long()
    lib.srec_hg_ws_floats(_ct.addressof(desc), _ct.addressof(n))
    key = (x.device.index, n.value)
    ws = _HG_WS.get(key)
    if ws is None:
        ws = _HG_WS[key] = torch.empty(max(n.value, 1), device=x.device, dtype=torch.float32)
    if xrec is not None:
        cat_inv, allf, invr, g_allf, picks, gps = xrec
        a_pick, a_g = ptr_array(picks), ptr_array(gps)
        a_ld = (_ct.c_int * len(picks))(*[(_ld(gp) if gp is not None else x.shape[1]) for gp in gps])
        lib.srec_hg_bwd_exit(_ct.addressof(desc), ptr(x), _ld(x), ptr(g), _ld(g), ptr(arg), ptr(dx), x.shape[1], ptr(ws), ptr(cat_inv),
                             ptr(allf), ptr(invr), ptr(g_allf), _ld(g_allf), len(picks), _ct.addressof(a_pick), _ct.addressof(a_g),
                             _ct.addressof(a_ld), stream())
    else:
        lib.srec_hg_bwd(_ct.addressof(desc), ptr(x), _ld(x), ptr(g), _ld(g), ptr(arg), ptr(dx), x.shape[1], ptr(ws), stream())
    return desc, dP, grads, dx


def _backward_data(ctx, dP, params, dx):
    """d x of a node type += sum over the modules that project it of dP fc (the module sum is the K loop: segments).  With feature
    dropout the convs see differently masked inputs: one term per conv in tgts [2, S, NT, D] for the merge kernel -> (tgts, S)"""
    plan, strategy, drop = ctx.plan, ctx.strategy, ctx.drop
    NT, D = dx.shape
    HD, nt = plan.H * D, len(plan.types)
    tgts, S, full = None, 1, False
    if drop is not None:
        # every node type is projected by some module of each conv in the usual plans: the grouped GEMM then writes all
        # rows (beta = 0 zeroes rows past the live count) and the buffers need no fill
        nproj = {len(plan.projectors(cv, t)) for cv in (0, 1) for t in range(nt)}
        full = strategy != 'plain' and min(nproj) > 0
        # gemm16: when every (conv, type) is projected by the same number S of modules (intra_k + the shared 'inter'), each
        # module's product goes to its own partial buffer (S x more, S x shorter reduction loops); the merge kernel sums them
        if strategy == 'g16' and full and len(nproj) == 1 and 1 < min(nproj) <= 4:
            S = min(nproj)
        tgts = (torch.empty if full else torch.zeros)(2, S, NT, D, device=dx.device, dtype=torch.float32)
    beta, convs = 0.0 if full else 1.0, (0, 1) if drop is not None else (None,)
    tgt = lambda cv, j=0: dx if cv is None else tgts[cv, j]
    if strategy == 'plain':
        for cv in convs:
            for m, (r0, nr, dyn) in enumerate(plan.modules):
                if cv is None or plan.mod_conv[m] == cv:
                    ops.gemm_nn(dP[m], _rows(params[4 * m]), tgt(cv)[r0:r0 + nr], dyn, 1 if dyn is not None else 0, beta=1.0)
        return tgts, S
    W = ctx.g16[1] if strategy == 'g16' else params[::4]

    def problems(cv):
        """conv cv: one problem per node type, or (S > 1) per node type and projecting module"""
        out = []
        for t, (t0, nc, dyn_t, _) in enumerate(plan.types):
            mods = plan.projectors(cv, t)
            for j, grp in enumerate([[m] for m in mods] if S > 1 else [mods] if mods else []):
                segs = [(dP[m][t0 - plan.modules[m][0]:][:nc], W[m]) for m in grp]
                out.append(GemmProb(nc, D, HD, segs, tgt(cv, j)[t0:t0 + nc], dyn_t, mhint=plan.live.get(t0, 0)))
        return out
    if strategy == 'grouped':                    # one launch per conv
        for probs in filter(None, map(problems, convs)):
            ops.gemm_group(1, probs, HD, D, D, beta=beta, a16=True)
    else:                                        # 'g16': the two convs' problems share the launches
        probs = [q for cv in convs for q in problems(cv)]
        for i in range(0, len(probs), ops.G16_MAXP):
            ops.gemm16('nt', probs[i:i + ops.G16_MAXP], HD, HD, D, beta=beta)
    return tgts, S


def _weight_grads(ctx, x, dP, gWs):
    """gWs[m] = dP[m]^T (dropped) x[rows of m]"""
    plan, D, HD, nm = ctx.plan, x.shape[1], ctx.plan.H * x.shape[1], len(ctx.plan.modules)
    xin = [ctx.drop.xc[cv] for cv in plan.mod_conv] if ctx.drop is not None else [x] * nm
    if ctx.strategy == 'g16':
        # one balanced problem per (module, node type): a module that spans several types (the shared 'inter' one) writes
        # one slab per type, summed in fixed order afterwards
        xin16 = ctx.g16[0]
        pcs = [plan.pieces(m) for m in range(nm)]
        slabs = {m: torch.empty(len(pcs[m]), HD, D, device=x.device, dtype=torch.float32) for m in range(nm) if len(pcs[m]) > 1}
        # the launch may wait for the k-gram GRU's weight-gradient launch and leave inside it (ops.STEP, "Waiting tn products"):
        # autograd is then handed EVERY gWs[m] unwritten, so the permission is asked for all module weights, and the waiting
        # problems hold aliases (a second reference to a returned gradient would make AccumulateGrad clone it, unwritten)
        wait = ops.WGRAD_ONE_LAUNCH and 0 < sum(map(len, pcs)) <= ops.G16_MAXP and ops.can_defer(ctx.defer, ctx.wparams)
        gC = [g.detach() for g in gWs] if wait else gWs
        probs = [GemmProb(HD, D, nc, [(dP[m][o:o + nc], xin16[m][t0:t0 + nc])], slabs[m][pi:pi + 1] if m in slabs else gC[m], dyn_t,
                          ld=(HD, D, D))
                 for m in range(nm) for pi, (o, t0, nc, dyn_t) in enumerate(pcs[m])]
        if wait:
            ops.STEP.defer_product(probs, (dP, xin16, slabs))
        else:
            for i in range(0, len(probs), ops.G16_MAXP):
                ops.gemm16('tn', probs[i:i + ops.G16_MAXP], HD, D, D)
        if slabs and ops.can_defer(ctx.defer, [ctx.wparams[m] for m in slabs]):
            for m, sl in slabs.items():
                ops.defer_slab_sum(sl, gWs[m])
        elif slabs:
            ops._launch_slab_sums([(sl, gWs[m]) for m, sl in slabs.items()])
    elif ctx.strategy == 'grouped':
        ops.gemm_group(2, [(HD, D, nr, [(dP[m], xin[m][r0:r0 + nr])], gWs[m], dyn)
                           for m, (r0, nr, dyn) in enumerate(plan.modules)], HD, D, D, a16=True)
    else:
        for m, (r0, nr, dyn) in enumerate(plan.modules):
            ops.gemm_tn(dP[m], xin[m][r0:r0 + nr], gWs[m], dyn)


class HGATLayer(torch.autograd.Function):
    """out = MSHGNN(x): all relation instances of conv1 / conv2 in one batched pass (csrc/hgat.hip) around the fc
    GEMMs.  params = (fc.weight, attn_l, attn_r, bias) per module, in plan.modules order.
    drop = (p_feat, p_attn) in training: feature dropout with ONE mask per (conv, node type) on the inputs of that
    conv's GATConv modules (projection, logits and identity residual all see the dropped rows, gatconv.py:268-308;
    the reference draws one mask per (relation, role) - documented deviation) and attention dropout on the edge
    soft-max (gatconv.py:300)."""

    @staticmethod
    def forward(ctx, x, plan, drop, entry, exit_, bits, *params):
        """entry (NormEntry, x = None) / exit_ (NormExit): the normalisations around the call belong to it - the raw tensors come
        first in params, the results are (allf, picks...), and the launches of bits (FOLD_*) carry them; a bit that is off runs
        the launch of ops.normalize_stack / ops.norm_permute_pick at that boundary"""
        ctx.entry, ctx.exit, ctx.bits = entry is not None, exit_, bits
        inv = None
        if entry is not None:
            K = len(entry.raws)
            ctx.tags = [ops._arena_tag(r) for r in params[:K]]          # pieces of a split tensor: their gradients go into its buffer
            entry = entry._replace(raws=[_rows(r) for r in params[:K]])
            params = params[K:]
            ns, D0 = [r.shape[0] for r in entry.raws], entry.raws[0].shape[1]
            x = torch.empty(sum(ns), D0, device=entry.raws[0].device, dtype=torch.float32)
            inv = torch.empty(sum(ns), device=x.device, dtype=torch.float32)
            ctx.nmeta = (ns, entry.dyns)
            if not bits & FOLD_A:
                a_x, a_l, a_n, a_d = _group_arrays(entry.raws, entry.dyns)
                lib.srec_normalize_group_fwd(K, _ct.addressof(a_x), _ct.addressof(a_l), _ct.addressof(a_n), _ct.addressof(a_d), ptr(x),
                                             D0, ptr(inv), D0, entry.eps_mode, 1e-12, stream())
        x = _rows(x)
        (NT, D), dev, nm = x.shape, x.device, len(plan.modules)
        strategy = gemm_strategy(ops.PRECISION['matmul'], D, _ld(x), nm, all(params[4 * m].is_contiguous() for m in range(nm)))
        dstate, x16 = None, None
        fold = plan.take_fold()                      # the prologue launch of this forward already folded the weights (step_prologue)
        small, lay = fold or plan.scratch(dev)
        # bf16 strategies: the projections (and their gradients) are STORED as bf16 too - every pass over them is HBM bound
        P = [torch.empty(nr, plan.H * D, device=dev, dtype=torch.float32 if strategy == 'plain' else torch.bfloat16)
             for (r0, nr, dyn) in plan.modules]
        flat = [p.reshape(-1) if i % 4 else p for i, p in enumerate(params)]
        desc = plan.fill(HgDesc(), small, lay, P, None, flat, None, None)
        if fold is not None:
            desc.p16 |= CONST['SREC_HG_FOLDED']
        live = plan.live_rows(small, lay) if strategy == 'g16' and ops.HG_LIVE_ROWS and plan.blocks else None
        dropping = drop is not None and (drop[0] > 0 or drop[1] > 0)
        if dropping:
            x = x.contiguous()          # srec_hg_fwd / srec_hg_bwd read the dropped copies (xin, xres: [NT, D]) with x's row stride
            dstate, x16 = _drop_prep(x, plan, drop, strategy, (desc,) + live if live is not None else None,
                                     (entry, inv) if bits & FOLD_A else None)
            plan.fill_drop(desc, dstate)
        elif live is not None:                       # (the lists ride in the dropout launch when there is one)
            la = ptr_array(live[0])
            lib.srec_hg_live_rows(_ct.addressof(desc), _ct.addressof(la), ptr(live[1]), stream())
        xin = [dstate.xc[cv] for cv in plan.mod_conv] if dstate is not None else [x] * nm      # what each module projects
        g16 = _project(xin, x16, plan, params, strategy, P, live)
        arg = torch.empty(NT, D, device=dev, dtype=torch.uint8)
        allf = None
        if exit_ is not None and bits & FOLD_B:              # the aggregation launch writes allf / invr / the pick rows itself
            n_cat, B = exit_.cat_perm.numel(), exit_.picks[0].numel()
            allf = torch.empty(n_cat, D, device=dev, dtype=torch.float32)
            invr = torch.empty(n_cat, device=dev, dtype=torch.float32)
            bufs = [torch.empty(B, 2 * D, device=dev, dtype=torch.float32) for _ in exit_.picks]   # v = left half of [v | read-out]
            a_pick, a_out, a_ld = ptr_array(exit_.picks), ptr_array(bufs), (_ct.c_int * len(bufs))(*([2 * D] * len(bufs)))
            lib.srec_hg_fwd_exit(_ct.addressof(desc), ptr(x), _ld(x), ptr(arg), ptr(exit_.cat_inv), ptr(allf), ptr(invr), len(bufs),
                                 _ct.addressof(a_pick), _ct.addressof(a_out), _ct.addressof(a_ld), exit_.eps_mode, 1e-12, stream())
            out = None
        else:
            out = torch.empty(NT, D, device=dev, dtype=torch.float32)
            lib.srec_hg_fwd(_ct.addressof(desc), ptr(x), _ld(x), ptr(out), D, ptr(arg), stream())
        ctx.plan, ctx.lay, ctx.strategy, ctx.drop, ctx.g16 = plan, lay, strategy, dstate, g16
        ctx.defer, ctx.wparams = ops.defer_scope(), [params[4 * m] for m in range(nm)]
        extra = [inv] if inv is not None else []
        if exit_ is None:
            ctx.save_for_backward(x, small, arg, *P, *params, *extra)
            return out
        if allf is None:
            allf, invr, bufs = ops.npp_forward(out, exit_.cat_perm, exit_.dyn_t, exit_.dyn_b, exit_.eps_mode, exit_.picks)
        extra += [exit_.cat_perm, exit_.cat_inv, exit_.cat_seg, allf, invr] + list(exit_.picks)
        ctx.save_for_backward(x, small, arg, *P, *params, *extra)
        return (allf,) + tuple(b[:, :D] for b in bufs)

    @staticmethod
    def backward(ctx, g, *g_picks):
        plan, drop, nm, bits = ctx.plan, ctx.drop, len(ctx.plan.modules), ctx.bits
        x, small, arg, *rest = ctx.saved_tensors
        P, params, extra = rest[:nm], rest[nm:5 * nm], rest[5 * nm:]
        inv = extra.pop(0) if ctx.entry else None
        NT, D = x.shape
        xrec = None
        if ctx.exit is not None:
            perm, cat_inv, cat_seg, allf, invr, *picks = extra
            g_allf = _rows(g)
            gps = [(_rows(gp) if gp is not None else None) for gp in g_picks]
            if bits & FOLD_C and _ld(g_allf) % 4 == 0:
                g = torch.empty(NT, D, device=x.device, dtype=torch.float32)       # written by the score-gradient launch
                xrec = (cat_inv, allf, invr, g_allf, picks, gps)
            else:
                g = ops.npp_backward(allf, invr, g_allf, perm, cat_seg, picks, gps, ctx.exit.types, ctx.exit.dyn_b, NT)
        g = _rows(g)
        # feature dropout with recomputed masks (the tap is off): d x is written once, after the backward-data GEMMs
        late_dx = drop is not None and drop.ms is None and _ld(g) % 4 == 0
        fold_d = bool(late_dx and ctx.entry and bits & FOLD_D)
        desc, dP, grads, dx = _backward_graph(ctx, x, g, small, arg, P, params, late_dx, xrec, not fold_d)
        gWs = [ops.grad_buf(params[4 * m]) for m in range(nm)]
        tgts, S = _backward_data(ctx, dP, params, dx if dx is not None else x)       # (late_dx: only shape and device are read)
        dxs = None
        if ctx.entry:                                  # the raw tensors' gradient rows (inside their arena when they have one)
            ns, dyns = ctx.nmeta
            dxall, dxs, o = None, [], 0
            for n, tag in zip(ns, ctx.tags):
                if tag is None and dxall is None:
                    dxall = torch.empty(NT, D, device=x.device, dtype=torch.float32)
                dxs.append(ops._arena_rows(tag, n, D, x.device) if tag is not None else dxall[o:o + n])
                o += n
        if fold_d:
            a_dx, a_ld = ptr_array(dxs), (_ct.c_int * len(dxs))(*[_ld(t) for t in dxs])
            lib.srec_hg_pre_merge_norm(_ct.addressof(desc), ptr(g), _ld(g), ptr(tgts), S, ptr(x), ptr(inv), _ct.addressof(a_dx),
                                       _ct.addressof(a_ld), stream())
            dxs_done = True
        else:
            dxs_done = False
            if late_dx:
                lib.srec_hg_pre_merge(_ct.addressof(desc), ptr(g), _ld(g), ptr(tgts), S, ptr(dx), D, stream())
            elif drop is not None:
                lib.srec_hg_drop_merge(ptr(tgts), S, ptr(drop.ms), NT * D, ptr(dx), *drop.rng, stream())
        _weight_grads(ctx, x, dP, gWs)
        if dxs is not None and not dxs_done:
            a_x, a_l, a_n, a_d = _group_arrays(dxs, dyns, [D] * len(dxs))
            lib.srec_normalize_group_bwd(len(dxs), _ct.addressof(a_x), _ct.addressof(a_l), _ct.addressof(a_n), _ct.addressof(a_d), ptr(x),
                                         D, ptr(dx), D, ptr(inv), D, stream())
        outs = [o for m in range(nm) for o in [gWs[m]] + [grads[m][j].view(params[4 * m + 1 + j].shape) for j in range(3)]]
        return (None if dxs is not None else dx, None, None, None, None, None) + tuple(dxs or ()) + tuple(outs)


def hgat_layer(x, plan, params, drop=None, entry=None, exit_=None):
    """entry (NormEntry; x is then None) / exit_ (NormExit): the caller's normalisations in front of / behind the layer.  Returns
    out [NT, D], or with exit_ (allf, [picks]) as ops.norm_permute_pick.  Whether a normalisation rides in the layer's launches
    is decided here (norm_fold_bits); a boundary that takes no fold at all runs ops.normalize_stack / ops.norm_permute_pick."""
    D = (entry.raws[0] if entry is not None else x).shape[1]
    per_type = [sum(1 for (m, sb, db, gr) in plan.insts if plan.blocks[db][1] == t) for t in range(len(plan.types))]
    if entry is not None and [r.shape[0] for r in entry.raws] != [tp[1] for tp in plan.types]:
        x, entry = ops.normalize_stack(entry.raws, entry.eps_mode, entry.dyns), None          # (one raw tensor per node type only)
    if exit_ is not None and not (exit_.cat_perm.numel() == exit_.cat_inv.numel() == sum(tp[1] for tp in plan.types)
                                  and 0 < len(exit_.picks) <= 4 and all(pk.numel() == plan.B for pk in exit_.picks)):
        fexit, exit_ = exit_, None               # (the folds pair every stacked row with one concatenated row)
        outs = hgat_layer(x, plan, params, drop, entry)
        return ops.norm_permute_pick(outs, fexit.cat_perm, fexit.cat_seg, fexit.picks, fexit.types, fexit.dyn_t, fexit.dyn_b,
                                     fexit.eps_mode)
    pf, pa = drop if drop is not None else (0.0, 0.0)
    bits = norm_fold_bits(ops.NORM_FOLD, plan.H, D, per_type, entry is not None, exit_ is not None, pf, pa, ops.DROP_TAP is not None)
    if entry is not None and not bits & (FOLD_A | FOLD_D):
        x, entry = ops.normalize_stack(entry.raws, entry.eps_mode, entry.dyns), None
    fexit = exit_ if bits & (FOLD_B | FOLD_C) else None
    outs = HGATLayer.apply(x, plan, drop, entry, fexit, bits, *(tuple(entry.raws) if entry is not None else ()), *params)
    if exit_ is None:
        return outs
    if fexit is None:
        return ops.norm_permute_pick(outs, exit_.cat_perm, exit_.cat_seg, exit_.picks, exit_.types, exit_.dyn_t, exit_.dyn_b,
                                     exit_.eps_mode)
    for o in outs[1:]:
        o._srec_cat_left = True          # the left half of a private [B, 2 D] buffer (ReadoutHead writes the right half)
    return outs[0], list(outs[1:])
