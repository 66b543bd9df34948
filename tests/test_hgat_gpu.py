"""The batched MSHGNN layer (ops.hgat_layer: csrc/hgat.hip around the fc GEMMs) against the CPU oracle's MSHGNN in float64,
operator level, on every product route: exact fp32, bf16 grouped (D % 8 == 0) and bf16 gemm16 (D % 64 == 0); with and without
dropout (masks replayed in the oracle), exact and capacity-padded layouts, batches with an edgeless relation.

What is compared: the output, d x and the gradient of every parameter the plan returns, ROW by row (a pooled norm over ~2 000
rows cannot see one wrong row).  How close they must be is not a constant of this file: the oracle is run a second time with
the route's own rounding (bf16 x / W operands, bf16-stored projection and projection gradient, as ops.HGATLayer documents; a
plain fp32 run for the exact route, and beside the bf16 emulation too, because every route accumulates in fp32) and the HIP
result may be MARGIN x further from the float64 run than that run is.

The arg-max.  The layer takes a max over 8 heads; where two heads nearly tie, a bf16 run and a float64 run may pick different
heads and the gradients then differ by O(1) for a legitimate reason.  The cotangent d(loss)/d(out) is therefore ZERO in every
cell whose top-two gap IN THE FLOAT64 REFERENCE is below delta = ARGMAX_MULT x (largest head-value difference between the
rounding-emulated reference run and the float64 one): no gradient flows through a contested cell in either implementation.
At most 5 % of a case's cells may be zeroed (asserted); the per-head biases are drawn from N(0, 2^2) so that the heads of a
cell are separated by more than the identical residual leaves them (3 - 6 % of the cells are contested with the default
initialisation).  The LeakyReLU kink needs no such treatment: a logit that changes sign under rounding changes one (edge,
head)'s slope by a bounded factor (1 against 0.2), and the product computes the logits in fp32 from the fp32 rows on every route
(folded attention vectors, hgat.hip), so such flips happen at the fp32 level only - as they do in the yardstick runs (the
bf16 emulation leaves the logits unrounded for the same reason, the fp32 run rounds them as the product does), whose errors
the bounds are derived from."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import close, load_golden, pkg, reseed

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import collate_ref as oc, models_ref as om          # noqa: E402

pytestmark = pytest.mark.gpu

K, H, V = 3, 8, 3429
# a contested cell: the HIP run's head values are ANOTHER draw of the rounding the emulated oracle run makes (other summation
# order, the logits from the folded fp32 vectors instead of the rounded projection, one rounding of a summed dP instead of one
# per relation role) - allow its largest head-value error to be 4 x the emulated run's largest; two heads of a cell can err in
# opposite directions: x 2.  delta = 8 x the emulated run's largest head-value difference.
ARGMAX_MULT = 8.0
MAX_ZEROED = 0.05
# HIP error <= MARGIN x the reference's own error at that precision (the convention of test_models_gpu.py's step-0 gradient
# yardstick: sequential MFMA accumulation against torch's pairwise sums, one draw of the rounding against another).  That test
# uses 16; here 8 holds: the largest measured ratio is 3.8 (a bias gradient, a cancelling column sum over ~3 000 rows), 1.0 -
# 1.6 for everything else
MARGIN = 8.0
BIAS_STD = 2.0
ATTN_SCALE = 6.0          # attn_l / attn_r = their U(-1/sqrt d, 1/sqrt d) initialisation x 6: edge logits of spread ~ 1


# ------------------------------------------------------------------------------------------------------------ inputs
_SHORT = {'short2212': (2, 2, 1, 2), 'short231': (2, 3, 1), 'single111': (1, 1, 1)}     # lens of test_msgifsr_batches_with_missing_relations
ROWS532 = [([11, 12, 13], 15), ([16, 17], 18)]                  # 5 / 3 / 2 nodes of order 1 / 2 / 3


def _samples(batch):
    if batch in ('s32', 'edge'):
        return load_golden('msgifsr_K3_' + batch)[1]
    if batch == 'rows532':
        return ROWS532
    if batch == 'big':
        from dist_gpu_worker import synth_samples
        return synth_samples(512, V, 11)
    lens = _SHORT[batch]
    rng = np.random.default_rng(sum(lens))
    return [(rng.integers(0, 300, size=L).tolist(), int(rng.integers(0, 300))) for L in lens]


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def make_case(d, batch, rounded, seed=0):
    """-> (product model (CPU), float64 oracle layer, samples, oracle graph): the same seeded state in both, the GAT biases
    from N(0, BIAS_STD^2), the attention vectors x ATTN_SCALE, the fc weights bf16-representable when `rounded`"""
    sp = pkg()
    torch.manual_seed(1000 + seed + d)
    model = sp.MSGIFSR(V, 'sample', d, 1, dropout=0.0, order=K, extra=False, fusion=False)
    gen = torch.Generator().manual_seed(77 + seed)
    with torch.no_grad():
        for conv in (model.layers[0].conv1, model.layers[0].conv2):
            for et in sorted(conv.mods.keys()):
                mod = conv.mods[et]
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=gen) * BIAS_STD)
                mod.attn_l.mul_(ATTN_SCALE)
                mod.attn_r.mul_(ATTN_SCALE)
                if rounded:
                    mod.fc.weight.copy_(_bf16(mod.fc.weight))
    ref = om.MSGIFSR(V, 'sample', d, 1, dropout=0.0, order=K, extra=False, fusion=False)
    ref.load_state_dict(model.state_dict())
    samples = _samples(batch)
    (og,), _ = oc.collate_fn_factory_ccs((oc.seq_to_ccs_graph,), K)(samples)
    return model, ref.layers[0].double(), samples, om.to_torch(og)


def make_x(og, d, rounded, seed=0):
    """{k: [N_k, d]} float32 rows, randn * 0.5 (bf16-representable when `rounded`)"""
    gen = torch.Generator().manual_seed(5 + seed)
    x = {}
    for k in range(1, K + 1):
        v = torch.randn(int(og['num_nodes'][k].sum()), d, generator=gen) * 0.5
        x[k] = _bf16(v) if rounded else v
    return x


def random_masks(og, d, drop, all_rels, seed=3):
    """masks of the product's KIND from torch's generator (the CPU-only check of the 5 % cap; on the GPU the product's own
    masks are replayed)"""
    pf, pa = drop
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for c in ('conv1', 'conv2'):
        feat = {k: (torch.rand(int(og['num_nodes'][k].sum()), d, generator=gen) >= pf).double() / (1 - pf)
                for k in range(1, K + 1)}
        attn = {key: (torch.rand(len(r['src']), H, generator=gen) >= pa).double() / (1 - pa)
                for key, r in og['rel'].items() if all_rels or len(r['src']) > 0}
        out[c] = dict(feat=feat, attn=attn)
    return out


# ------------------------------------------------------------------------------------------------------------ reference
class _StoreBf16(torch.autograd.Function):
    """a tensor STORED as bf16: the value is rounded on the way forward, its gradient on the way back (P and dP)"""

    @staticmethod
    def forward(ctx, t):
        return _bf16(t)

    @staticmethod
    def backward(ctx, g):
        return _bf16(g)


class _OperandBf16(torch.autograd.Function):
    """a GEMM operand read as bf16: rounded forward; the gradient w.r.t. the fp32 master passes (fp32 accumulators)"""

    @staticmethod
    def forward(ctx, t):
        return _bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


def emu_gat(mod, src, dst, h_src_in, h_dst_in, masks=None):
    """the oracle's GATConv.forward (models_ref.py, line by line) with the rounding points of the product's bf16 routes
    (ops.HGATLayer, csrc/hgat.hip): the projection the aggregation reads is P = bf16(bf16(x) bf16(W)^T) and its gradient is
    stored as bf16; the attention logits do NOT come from that projection but from the fp32 rows and the folded fp32 vectors
    (el = x . (W^T a_l), hgat.hip `logits`): unrounded here"""
    Hh, D = mod._num_heads, mod._out_feats
    if masks is not None:
        h_src, h_dst = h_src_in * masks[0], h_dst_in * masks[1]
    else:
        h_src, h_dst = h_src_in, h_dst_in
    W = mod.fc.weight
    feat_src = _StoreBf16.apply(F.linear(_OperandBf16.apply(h_src), _OperandBf16.apply(W))).view(-1, Hh, D)
    el = (F.linear(h_src, W).view(-1, Hh, D) * mod.attn_l).sum(dim=-1).unsqueeze(-1)
    er = (F.linear(h_dst, W).view(-1, Hh, D) * mod.attn_r).sum(dim=-1).unsqueeze(-1)
    e = mod.leaky_relu(el[src] + er[dst])
    a = om.edge_softmax(dst, e, h_dst.shape[0])
    if masks is not None:
        a = a * masks[2].view(-1, Hh, 1)
    rst = torch.zeros(h_dst.shape[0], Hh, D, dtype=feat_src.dtype).index_add_(0, dst, feat_src[src] * a)
    rst = rst + h_dst.view(h_dst.shape[0], -1, D)
    return rst + mod.bias.view(1, -1, D)


def _hetero(conv, rels, feat, reverse, masks, all_rels, emu=False):
    """oracle HeteroConv.forward (same relation order, same stack-and-sum) that, for all_rels, also runs the GATConv of a
    relation WITHOUT edges on empty edge lists: every destination node then gets its identity residual and bias
    (MSHGNN.plan's docstring; HeteroGraphConv itself skips such a relation)"""
    outs = {}
    gat = (lambda mod, *a: emu_gat(mod, *a)) if emu else (lambda mod, *a: mod(*a))
    order = sorted(rels.keys(), key=(lambda t: ('s%d' % t[2], t[1], 's%d' % t[0])) if reverse else
                   (lambda t: ('s%d' % t[0], t[1], 's%d' % t[2])))
    for key in order:
        s, et, d_ = key
        r = rels[key]
        if len(r['src']) == 0 and not all_rels:
            continue
        src, dst = r['src'].long().view(-1), r['dst'].long().view(-1)
        if reverse:
            mk = None if masks is None else (masks['feat'][d_], masks['feat'][s], masks['attn'][key])
            outs.setdefault(s, []).append(gat(conv.mods[et], dst, src, feat[d_], feat[s], mk))
        else:
            mk = None if masks is None else (masks['feat'][s], masks['feat'][d_], masks['attn'][key])
            outs.setdefault(d_, []).append(gat(conv.mods[et], src, dst, feat[s], feat[d_], mk))
    return {k: torch.stack(v, 0).sum(0) for k, v in outs.items()}


def ref_forward(layer, og, feat, masks, all_rels, emu=False):
    """oracle MSHGNN.forward, restated only to expose the pre-max head values: -> (out {k: [N_k, D]}, heads {k: [N_k, H, D]
    or None}).  Equality with MSHGNN.forward itself is asserted by the callers wherever all_rels is off."""
    h1 = _hetero(layer.conv1, og['rel'], feat, False, None if masks is None else masks['conv1'], all_rels, emu)
    h2 = _hetero(layer.conv2, og['rel'], feat, True, None if masks is None else masks['conv2'], all_rels, emu)
    out, heads = {}, {}
    for k in range(1, layer.order + 1):
        z = torch.zeros(1, layer.output_dim, dtype=feat[k].dtype)
        x = h1.get(k, z) + h2.get(k, z)
        heads[k] = x if x.dim() > 2 else None
        if x.dim() > 2:
            x = x.max(1)[0]
        nn_ = og['num_nodes'][k]
        out[k] = om.segment_mean(nn_, feat[k])[om.seg_ids(nn_)] + x
    return out, heads


def _cast(t, dt):
    if isinstance(t, dict):
        return {k: _cast(v, dt) for k, v in t.items()}
    return t.to(dt) if torch.is_tensor(t) and t.is_floating_point() else t


def _mod_params(layer):
    out = {}
    for cn in ('conv1', 'conv2'):
        for et, mod in getattr(layer, cn).mods.items():
            out[(cn, et, 'fc.weight')] = mod.fc.weight
            out[(cn, et, 'attn_l')], out[(cn, et, 'attn_r')], out[(cn, et, 'bias')] = mod.attn_l, mod.attn_r, mod.bias
    return out


class Run:
    """one oracle pass: forward now, backward once the cotangent is known"""

    def __init__(self, layer, og, x, masks, all_rels, dt, emu=False):
        self.layer, self.dt = layer, dt
        self.feat = {k: v.to(dt).clone().requires_grad_() for k, v in x.items()}
        self.out, self.heads = ref_forward(layer, og, self.feat, _cast(masks, dt), all_rels, emu)

    def backward(self, cot):
        ks = sorted(self.feat)
        ps = _mod_params(self.layer)
        names = [n for n in ps]
        loss = sum((self.out[k] * cot[k].to(self.dt)).sum() for k in ks)
        gs = torch.autograd.grad(loss, [self.feat[k] for k in ks] + [ps[n] for n in names], allow_unused=True)
        self.dx = {k: g.double() for k, g in zip(ks, gs[:len(ks)])}
        self.grads = {n: (None if g is None else g.double()) for n, g in zip(names, gs[len(ks):])}
        self.out = {k: v.detach().double() for k, v in self.out.items()}


class Reference:
    """float64 oracle + its rounding-emulated / fp32 re-runs for one case: cotangent, delta, zeroed share, yardsticks"""

    def __init__(self, layer64, og, x, masks, all_rels, route, cot_seed=9):
        self.og = og
        self.r64 = Run(layer64, og, x, masks, all_rels, torch.float64)
        if not all_rels:
            with torch.no_grad():             # the restated forward IS the oracle's
                o = layer64(og, {k: v.double() for k, v in x.items()}, _cast(masks, torch.float64))
            for k in o:
                assert torch.equal(o[k], self.r64.out[k].detach()), 'restated MSHGNN.forward differs from the oracle (type %d)' % k
        self.yard = [Run(copy.deepcopy(layer64).float(), og, x, masks, all_rels, torch.float32)]
        if route != 'fp32':
            self.yard.insert(0, Run(copy.deepcopy(layer64), og, x, masks, all_rels, torch.float64, emu=True))
        # delta from the route's own rounding (yard[0]: the bf16 emulation, or the fp32 run on the exact route)
        diff, cells, zeroed = 0.0, 0, 0
        for k, hv in self.r64.heads.items():
            if hv is not None:
                diff = max(diff, float((self.yard[0].heads[k].detach().double() - hv.detach()).abs().max()))
        self.head_err, self.delta = diff, ARGMAX_MULT * diff
        gen = torch.Generator().manual_seed(cot_seed)
        self.cot = {}
        for k, hv in self.r64.heads.items():
            c = torch.randn(self.r64.out[k].shape, generator=gen, dtype=torch.float64)
            if hv is not None:
                top = hv.detach().topk(2, dim=1)[0]
                contested = (top[:, 0] - top[:, 1]) < self.delta
                c = torch.where(contested, torch.zeros_like(c), c)
                cells += contested.numel()
                zeroed += int(contested.sum())
            self.cot[k] = c
        self.cells, self.share = cells, (zeroed / cells if cells else 0.0)
        for r in [self.r64] + self.yard:
            r.backward(self.cot)

    def logit_spread(self, layer64, x):
        """std of the raw edge logits el[src] + er[dst] over every edge of conv1 (float64, no masks)"""
        vals = []
        with torch.no_grad():
            for (s, et, d_), r in self.og['rel'].items():
                if len(r['src']) == 0:
                    continue
                mod = layer64.conv1.mods[et]
                ps, pd = mod.fc(x[s].double()).view(-1, H, mod._out_feats), mod.fc(x[d_].double()).view(-1, H, mod._out_feats)
                vals.append(((ps * mod.attn_l).sum(-1)[r['src'].long()] + (pd * mod.attn_r).sum(-1)[r['dst'].long()]).reshape(-1))
        return float(torch.cat(vals).std()) if vals else None


def row_err(got, ref):
    """max over rows of |got_row - ref_row| / (|ref_row| + floor), floor = 0.1 x the mean row norm of the reference: a row
    that is legitimately (near) zero is judged on the scale of a typical row instead of dividing by nothing"""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    if ref.numel() == 0:
        return 0.0
    nr = ref.norm(dim=1)
    floor = 0.1 * float(nr.mean())
    if floor == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float('inf')
    return float(((got - ref).norm(dim=1) / (nr + floor)).max())


def elem_err(got, ref, floor=0.0):
    """max |got - ref| / max(max |ref|, floor): the small [H D] gradients, element-wise against the tensor's scale"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    sc = max(float(ref.abs().max()), floor)
    if sc == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float('inf')
    return float((got - ref).abs().max()) / sc


def _cat(d):
    return torch.cat([d[k] for k in sorted(d)], 0)


def tensors_of(run):
    t = {'out': _cat(run.out), 'dx': _cat(run.dx)}
    for n, g in run.grads.items():
        if g is not None:
            t['/'.join(n)] = g
    return t


def kind_scales(want):
    """largest |element| over the reference tensors of one kind (attn_l, attn_r, bias of all modules)"""
    sc = {}
    for n, t in want.items():
        kind = n.split('/')[-1]
        sc[kind] = max(sc.get(kind, 0.0), float(t.abs().max()) if t.numel() else 0.0)
    return sc


def err_of(name, got, ref, scales):
    """row-wise for out, d x and the fc weight gradients; element-wise for the [H D] vectors - against the tensor's own scale,
    but not below 1e-3 of the scale of its kind over all modules: the attention vectors of a module whose destinations all have
    ONE in-edge get an exactly zero gradient in exact arithmetic and 1e-17 of noise in float64"""
    if name in ('out', 'dx') or name.endswith('fc.weight'):
        return row_err(got, ref)
    return elem_err(got, ref, 1e-3 * scales[name.split('/')[-1]])


# the product stores every result as fp32: half an ulp of the tensor's scale is the least any bound can ask for (a sum whose
# float64 and emulated values coincide, such as a bias gradient, has a reference error of exactly zero)
FP32_HALF_ULP = 2.0 ** -24


def bound_of(name, yard, want, scales):
    return MARGIN * max(max(err_of(name, y[name], want[name], scales) for y in yard), FP32_HALF_ULP)


# ------------------------------------------------------------------------------------------------------------ product side
def collate(samples, padded):
    c = pkg('collate')
    caps = c.default_caps(len(samples), 20) if padded else None
    (mg,), _ = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=caps)(samples)
    assert bool(mg.meta.get('padded')) == bool(padded)
    return mg


def type_rows(mg):
    """[(first stacked row, live rows, capacity)] per node type"""
    out, r = [], 0
    for k in range(1, K + 1):
        out.append((r, mg.count('N%d' % k), mg.meta['ncap'][k]))
        r += mg.meta['ncap'][k]
    return out, r


def stack(mg, per_type, fill=0.0):
    rows, NT = type_rows(mg)
    d = per_type[1].shape[1]
    t = torch.full((NT, d), fill, dtype=torch.float32)
    for k, (r0, n, _) in enumerate(rows, 1):
        t[r0:r0 + n] = per_type[k].float()
    return t


def live_rows(mg, t):
    rows, _ = type_rows(mg)
    return torch.cat([t[r0:r0 + n] for r0, n, _ in rows], 0)


def dead_rows(mg, t):
    rows, _ = type_rows(mg)
    return torch.cat([t[r0 + n:r0 + cap] for r0, n, cap in rows], 0)


def oracle_masks(mg, tap, d, all_rels):
    """the product's tapped masks ('ms' [2, NT, D] per (conv, stacked row), 'mk' per relation instance in plan.insts order:
    conv1's live relations, then conv2's) in the oracle's format"""
    rows, _ = type_rows(mg)
    ms = tap['ms'].cpu().double()
    live = [tuple(key) for key, nm in mg.meta['rels'] if all_rels or mg.count('E_' + nm) > 0]
    ne = {tuple(key): mg.count('E_' + nm) for key, nm in mg.meta['rels']}
    out, i = {}, 0
    for c, cn in enumerate(('conv1', 'conv2')):
        feat = {k: ms[c, r0:r0 + n] for k, (r0, n, _) in enumerate(rows, 1)}
        attn = {}
        for key in live:
            if tap['mk'] is not None:
                attn[key] = tap['mk'][i].cpu().double().view(-1, H)[:ne[key]]
            else:
                attn[key] = torch.ones(ne[key], H, dtype=torch.float64)
            i += 1
        out[cn] = dict(feat=feat, attn=attn)
    assert tap['mk'] is None or i == len(tap['mk'])
    return out


class Spy:
    """which product route a call took: counts the calls of the three product families inside ops"""

    def __init__(self, monkeypatch):
        ops = pkg('ops')
        self.n = dict(gemm16=0, gemm_group=0, gemm_nt=0)
        for nm in self.n:
            monkeypatch.setattr(ops, nm, self._wrap(nm, getattr(ops, nm)))

    def _wrap(self, nm, fn):
        def f(*a, **kw):
            self.n[nm] += 1
            return fn(*a, **kw)
        return f

    def route(self):
        live = sorted(k for k, v in self.n.items() if v)
        return {('gemm_nt',): 'fp32', ('gemm_group',): 'grouped', ('gemm16',): 'gemm16', (): 'none'}.get(tuple(live), tuple(live))


def param_names(layer, params):
    ids = {id(p): n for n, p in _mod_params(layer).items()}
    return [ids[id(p)] for p in params]


def run_layer(dev, layer, mg, x, cot, drop, all_rels, tap, seed=21, strided=False):
    """one forward + backward of ops.hgat_layer -> (out, dx, {param name: grad}, tapped masks or None).  cot: callable
    (out, tap) -> stacked cotangent (the reference needs the masks of THIS call first) or a tensor.  strided: the same rows
    as a column slice of a [NT, 2 d] matrix (unit inner stride, row stride 2 d)"""
    ops = pkg('ops')
    plan, params = layer.plan(mg, x.shape[1], all_rels)
    names = param_names(layer, params)
    ps = [p.detach().clone().requires_grad_() for p in params]
    xr = x.to(dev)
    if strided:
        xr = torch.cat([torch.zeros_like(xr), xr], 1)[:, x.shape[1]:].detach()
        assert xr.stride() == (2 * x.shape[1], 1)
    xr.requires_grad_()
    ops.DROP_TAP = [] if tap else None
    try:
        reseed(seed)
        out = ops.hgat_layer(xr, plan, ps, drop)
        taps = ops.DROP_TAP
    finally:
        ops.DROP_TAP = None
    tapped = None
    if tap and drop is not None:
        assert len(taps) == 1
        tapped = taps[0]
    g = cot(out.detach().cpu(), tapped) if callable(cot) else cot
    gs = torch.autograd.grad(out, [xr] + ps, g.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), gs[0].cpu(), {n: g_.cpu() for n, g_ in zip(names, gs[1:])}, tapped


# ------------------------------------------------------------------------------------------------------------ the cases
# (route, d, batch, drop, padded, all_rels, rounded).  Every width, batch, dropout setting, layout and relation setting on every
# route; d = 256 / gemm16 / dropout / padded / 512 sessions together is the configuration bench.py times.
CASES = [
    ('fp32', 32, 's32', None, False, False, False),
    ('fp32', 40, 'edge', (0.3, 0.3), False, False, False),
    ('fp32', 64, 'big', (0.3, 0.0), True, False, False),
    ('fp32', 40, 's32', (0.0, 0.3), True, False, False),
    ('fp32', 32, 'short2212', None, False, False, False),
    ('fp32', 64, 'short231', None, False, True, False),
    ('grouped', 40, 's32', None, False, False, True),
    ('grouped', 72, 'edge', (0.3, 0.3), True, False, True),
    ('grouped', 72, 'big', (0.3, 0.0), False, False, True),
    ('grouped', 40, 's32', (0.0, 0.3), False, False, False),
    ('grouped', 40, 'short2212', None, False, False, True),
    ('grouped', 72, 'short231', None, False, True, True),
    ('gemm16', 64, 's32', None, False, False, True),
    ('gemm16', 128, 'edge', (0.3, 0.3), False, False, True),
    ('gemm16', 256, 'big', (0.3, 0.3), True, False, True),
    ('gemm16', 128, 'big', (0.3, 0.0), False, False, False),
    ('gemm16', 64, 's32', (0.0, 0.3), True, False, True),
    ('gemm16', 64, 'short2212', None, False, False, True),
    ('gemm16', 128, 'short231', None, False, True, True),
    ('gemm16', 256, 's32', None, True, False, False),
]


def case_id(c):
    route, d, batch, drop, padded, all_rels, rounded = c
    return '-'.join([route, 'd%d' % d, batch, 'nodrop' if drop is None else 'drop%g_%g' % drop, 'padded' if padded else 'exact',
                     'allrels' if all_rels else 'liverels', 'bf16in' if rounded else 'fp32in'])


def check_reference(ref, layer64, x, what):
    """what must hold of the reference alone (also run without a GPU): the zeroed share and the logit spread"""
    assert ref.share <= MAX_ZEROED, '%s: %.2f %% of the cells zeroed at delta %.3e (cap 5 %%)' % (what, 100 * ref.share, ref.delta)
    spread = ref.logit_spread(layer64, x)
    assert spread is None or 0.3 < spread < 3.0, '%s: edge-logit spread %.3f is not of order 1' % (what, spread)
    return spread


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_hgat_layer_against_the_float64_oracle(dev, case, monkeypatch):
    route, d, batch, drop, padded, all_rels, rounded = case
    ops = pkg('ops')
    what = case_id(case)
    model, layer64, samples, og = make_case(d, batch, rounded)
    layer = model.to(dev).layers[0]
    mg = collate(samples, padded).to(dev)
    xt = make_x(og, d, rounded)
    x = stack(mg, xt)
    box = {}

    def cot(out, tap):
        # the reference of this case, once: with the masks of the (first) product call
        if 'ref' not in box:
            masks = oracle_masks(mg, tap, d, all_rels) if tap is not None else None
            box['ref'] = Reference(layer64, og, xt, masks, all_rels, route)
        return stack(mg, box['ref'].cot)

    spy = Spy(monkeypatch)
    ops.set_precision('fp32' if route == 'fp32' else 'bf16')
    try:
        runs = {'tapped' if drop is not None else 'plain': run_layer(dev, layer, mg, x, cot, drop, all_rels, tap=True)}
        took = spy.route()
        if drop is not None:
            # the production path keeps no mask tensor: same nonce, same device counter -> the same masks from the hash, and the
            # backward finishes d x in srec_hg_pre_merge instead of srec_hg_drop_merge
            runs['untapped'] = run_layer(dev, layer, mg, x, cot, drop, all_rels, tap=False)
            with torch.no_grad():
                plain = ops.hgat_layer(x.to(dev), *layer.plan(mg, d, all_rels), None).cpu()
    finally:
        ops.set_precision('fp32')
    assert took == route, '%s: the call took %r' % (what, took)
    ref = box['ref']
    spread = check_reference(ref, layer64, xt, what)
    print('\nHGAT %s: cells %d zeroed %.2f%% delta %.3e (head err %.3e) logit spread %s'
          % (what, ref.cells, 100 * ref.share, ref.delta, ref.head_err, 'n/a' if spread is None else '%.2f' % spread))
    if drop is not None:
        ms = runs['tapped'][3]['ms']
        if drop[0] > 0:
            assert abs(float((live_rows(mg, ms[0].cpu()) == 0).float().mean()) - drop[0]) < 0.05
        assert (live_rows(mg, plain) - live_rows(mg, runs['tapped'][0])).abs().max() > 1e-3, 'dropout changes nothing'
        assert torch.equal(runs['untapped'][0], runs['tapped'][0]), 'the replayed masks differ from the tapped ones'
    want = tensors_of(ref.r64)
    yard = [tensors_of(r) for r in ref.yard]
    scales = kind_scales(want)
    failures = []
    for tag, (out, dx, grads, _) in runs.items():
        got = {'out': live_rows(mg, out), 'dx': live_rows(mg, dx)}
        got.update({'/'.join(n): g for n, g in grads.items()})
        assert set(got) == set(want), (sorted(set(got) ^ set(want)))
        # rows past a type's live count: exact zeros in out (hgat.hip hg_agg_node_kernel / hg_agg_kernel: `o[x] = 0.f` for a
        # row that is not live) and in d x (hg_pre_kernel writes o = 0 for such a row; the backward-data GEMMs write zeros past
        # the live count, gemm16.hip `!g.keep_dead && (C16 || beta == 0)`, or skip the rows)
        assert float(dead_rows(mg, out).abs().max() if padded else 0.0) == 0.0, '%s %s: padded rows of out' % (what, tag)
        assert float(dead_rows(mg, dx).abs().max() if padded else 0.0) == 0.0, '%s %s: padded rows of dx' % (what, tag)
        worst = {}
        for n in sorted(got):
            e = err_of(n, got[n].reshape(want[n].shape), want[n], scales)
            bound = bound_of(n, yard, want, scales)
            kind = n.split('/')[-1]
            if kind not in worst or e / bound > worst[kind][0] / worst[kind][1]:
                worst[kind] = (e, bound)
            if not e <= bound:
                failures.append('%s %s %s: error %.3e > bound %.3e (%g x the reference\'s own error)' % (what, tag, n, e, bound, MARGIN))
        print('HGAT %s %s: ' % (what, tag) + '  '.join('%s %.2e/%.2e' % (k_, v[0], v[1]) for k_, v in sorted(worst.items()))
              + '   (worst error / bound per tensor kind)')
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------------------ padded layout
PADDED = [('fp32', 32, 's32', None), ('fp32', 32, 's32', (0.3, 0.3)), ('grouped', 40, 's32', None),
          ('grouped', 72, 'edge', (0.3, 0.3)), ('gemm16', 64, 's32', None), ('gemm16', 256, 'big', (0.3, 0.3))]


@pytest.mark.parametrize('route,d,batch,drop', PADDED, ids=lambda v: str(v).replace(' ', ''))
def test_padded_rows_are_never_read_and_stay_zero(dev, route, d, batch, drop, monkeypatch):
    """The capacity-padded layout of the layer alone.
    (a) dropout-free: live rows of out, d x and every parameter gradient equal the exact-layout call's at the fp32
        accumulation-order level: element-wise rtol 1e-4, as test_padded_layout_equals_exact.  (With dropout the masks are keyed
        by the element's position in the stacked matrix, so the two layouts draw different masks: nothing to compare.)
    (b) 'rows past a type's live count are never read' (ops.py, at the forward gemm16 call): the padded rows of x filled with
        zeros and with a large FINITE sentinel give bit-identical results in every live row and every parameter gradient - a
        leak shows as a wrong number in identifiable rows.
    (c) the padded rows of out and d x are exact zeros (hgat.hip: hg_agg_node_kernel writes `o[x] = 0.f` for a row that is not
        live, hg_pre_kernel leaves `o` at zero for it; the backward-data GEMMs write zeros past the live count or skip)."""
    ops = pkg('ops')
    model, layer64, samples, og = make_case(d, batch, rounded=True)
    layer = model.to(dev).layers[0]
    mg_e, mg_p = collate(samples, False).to(dev), collate(samples, True).to(dev)
    xt = make_x(og, d, rounded=True)
    gen = torch.Generator().manual_seed(4)
    cot = {k: torch.randn(v.shape, generator=gen) for k, v in xt.items()}
    spy = Spy(monkeypatch)
    ops.set_precision('fp32' if route == 'fp32' else 'bf16')
    try:
        exact = run_layer(dev, layer, mg_e, stack(mg_e, xt), stack(mg_e, cot), drop, False, tap=False)
        zero = run_layer(dev, layer, mg_p, stack(mg_p, xt), stack(mg_p, cot), drop, False, tap=False)
        sent = run_layer(dev, layer, mg_p, stack(mg_p, xt, fill=3.0e4), stack(mg_p, cot), drop, False, tap=False)
    finally:
        ops.set_precision('fp32')
    assert spy.route() == route, spy.route()
    for tag, r in (('zero fill', zero), ('sentinel', sent)):
        assert float(dead_rows(mg_p, r[0]).abs().max()) == 0.0, '%s: padded rows of out' % tag
        assert float(dead_rows(mg_p, r[1]).abs().max()) == 0.0, '%s: padded rows of dx' % tag
    for nm, a, b in [('out', zero[0], sent[0]), ('dx', zero[1], sent[1])] + [('/'.join(n), zero[2][n], sent[2][n]) for n in zero[2]]:
        bad = (a != b).reshape(a.shape[0], -1).any(1).nonzero().view(-1) if a.dim() > 1 and a.shape[0] > 1 else (a != b).nonzero()
        assert bad.numel() == 0, '%s: %d rows depend on the padded rows of x, first %r' % (nm, bad.shape[0], bad[:8].tolist())
    if drop is None:
        pairs = [('out', live_rows(mg_p, zero[0]), exact[0]), ('dx', live_rows(mg_p, zero[1]), exact[1])]
        pairs += [('/'.join(n), zero[2][n], exact[2][n]) for n in exact[2]]
        assert set(zero[2]) == set(exact[2])
        for nm, a, b in pairs:
            close(a, b, rtol=1e-4, atol=1e-7, what='padded vs exact ' + nm)


def test_row_strided_input_equals_the_contiguous_call(dev):
    """bf16 mode, D = 64, node types of 5 / 3 / 2 rows, dropout (0.3, 0.3): x given as a column slice of a [10, 128] matrix
    (_ld(x) != D) against the same call on x.contiguous().  The GEMM strategy is chosen once per call (hgat.gemm_strategy): the
    contiguous call takes gemm16, the strided one the per-module products, and the dropout prep writes its bf16 operand copy
    only for the former - same masks (same nonce, keyed by the element's position), same kernels around the GEMMs.  Both calls
    are bf16-route evaluations of the same function, so they must agree as closely as this file asks a bf16-route result to agree
    with the float64 oracle: err_of against the contiguous call <= bound_of of the gemm16 route (MARGIN x the rounding-emulated
    oracle run's own error), out, d x and every parameter gradient; contested arg-max cells carry no cotangent, as in the
    oracle test.  Both calls run untapped (the production path: masks recomputed, d x finished by srec_hg_pre_merge)."""
    ops = pkg('ops')
    d, drop = 64, (0.3, 0.3)
    model, layer64, samples, og = make_case(d, 'rows532', rounded=True)
    layer = model.to(dev).layers[0]
    mg = collate(samples, False).to(dev)
    assert [n for _, n, _ in type_rows(mg)[0]] == [5, 3, 2]
    xt = make_x(og, d, rounded=True)
    x = stack(mg, xt)
    box = {}

    def cot(out, tap):
        if 'ref' not in box:
            box['ref'] = Reference(layer64, og, xt, oracle_masks(mg, tap, d, False), False, 'gemm16')
        return stack(mg, box['ref'].cot)

    ops.set_precision('bf16')
    try:
        run_layer(dev, layer, mg, x, cot, drop, False, tap=True)            # (the masks of this seed, for the cotangent)
        runs = [run_layer(dev, layer, mg, x, cot, drop, False, tap=False, strided=st) for st in (False, True)]
    finally:
        ops.set_precision('fp32')
    ref = box['ref']
    want, yard = tensors_of(ref.r64), [tensors_of(r) for r in ref.yard]
    scales = kind_scales(want)
    cont, strd = [dict({'out': out, 'dx': dx}, **{'/'.join(n): g for n, g in grads.items()}) for out, dx, grads, _ in runs]
    assert set(cont) == set(strd) == set(want)
    failures = []
    for n in sorted(want):
        e, bound = err_of(n, strd[n].reshape(want[n].shape), cont[n].reshape(want[n].shape), scales), bound_of(n, yard, want, scales)
        print('HGAT strided vs contiguous %s: %.3e / %.3e' % (n, e, bound))
        if not e <= bound:
            failures.append('%s: strided vs contiguous %.3e > bound %.3e' % (n, e, bound))
    assert not failures, '\n'.join(failures)


def test_a_plan_without_modules_in_bf16_mode(dev, monkeypatch):
    """Sessions of one click: no relation has an edge, so the plan has no GAT module and the layer is out = x's session mean per
    row (msgifsr.py:86-89).  D = 64 in bf16 mode is where the gemm16 route would be taken if there were anything to multiply:
    hgat.gemm_strategy answers 'plain' for a module-less plan and no GEMM wrapper is called.  out and d x against the float64
    oracle at the file's bf16-route bound (no product is involved: the errors are fp32 summation order)."""
    ops, d = pkg('ops'), 64
    model, layer64, samples, og = make_case(d, 'single111', rounded=True)
    layer = model.to(dev).layers[0]
    mg = collate(samples, False).to(dev)
    plan, params = layer.plan(mg, d, False)
    assert len(plan.modules) == 0 and len(params) == 0
    xt = make_x(og, d, rounded=True)
    ref = Reference(layer64, og, xt, None, False, 'gemm16')
    spy = Spy(monkeypatch)
    ops.set_precision('bf16')
    try:
        out, dx, grads, _ = run_layer(dev, layer, mg, stack(mg, xt), stack(mg, ref.cot), None, False, tap=False)
    finally:
        ops.set_precision('fp32')
    assert spy.route() == 'none' and grads == {}
    want, yard = tensors_of(ref.r64), [tensors_of(r) for r in ref.yard]
    assert set(want) == {'out', 'dx'}
    for n, got in (('out', out), ('dx', dx)):
        e, bound = err_of(n, got, want[n], {}), bound_of(n, yard, want, {})
        print('HGAT no modules %s: %.3e / %.3e' % (n, e, bound))
        assert e <= bound, '%s: error %.3e > bound %.3e' % (n, e, bound)
