"""float64 oracles of the graph kernels that carry LESSR, SRGNN and NISER (csrc/sgat.hip, the read-out core and the weighted-mean
aggregation of csrc/segops.hip, csrc/gruseq.hip), the seeded graphs and sessions they are tested on, the case tables and the
row-wise comparator.  CPU only; nothing here imports the product.

The oracles are plain torch built from the helpers of oracle/models_ref.py (edge_softmax, segment_softmax, segment_sum,
SRGNNLayer._wmean); autograd supplies every gradient; tests/test_graph_oracle_cpu.py pins each of them to the oracle MODULE it
restates (SGAT, AttnReadout, EOPA).  Every oracle takes `dtype` - float64 is the reference, float32 the yardstick - and
`order='reversed'`, which visits the in-edges / session nodes in reversed order inside every sum and soft-max (and the columns of
W_hh inside the GRU's mat-vec, whose EDGE order is part of the operation): the same values, another rounding.

Tolerance rule (`rows_close`): row by row - a pooled norm cannot see one wrong row.  E[row] is the largest absolute error of
the fp32 oracle against the float64 one in that row; a row of the kernel's result passes when its largest absolute error
against float64 is at most margin * max(E[row], median(E)).  No floor relative to the row's own magnitude: gradients such as
dK are cancelling sums whose fp32 error is 3e-4 of the row and more.  The median term covers the rows both oracle runs
compute exactly (in-degree 0 and 1, padded rows: E = 0).  The two attention ops have FOUR fp32 yardsticks, E being the largest
error of the four per row: the oracle as it is, the oracle with the kernels' sigmoid, 1 / (1 + __expf(-x)) (_KernelSigmoid), and
the oracle with every logit displaced by one ulp up / down in alternating directions (_nudged).  Why: alpha = exp(e - max) / sum
turns the ABSOLUTE rounding error of a logit e (a dot product over the hidden columns; half an ulp of |e| ~ 4 is 2.4e-7, of the
85 that peaked logits reach 3.8e-6) into a RELATIVE error of every row that alpha scales (dX_i = alpha_i dout, dU_i through
alpha_i (dalpha_i - s)).  One fp32 run samples that error once per row, on the host's own BLAS and vector paths, and among 1200
node rows a few come out 20 - 50 x smaller than another correct run's: measured on an MI355X against the plain fp32 run alone,
single rows of dU / dX of seg_attn (1 - 8 of 1226) reached ratios of 20 - 40 (110 with peaked logits) and one row of dQ of
sgat_attn 19, at errors of 0.6 - 1 ulp of the row's logits; the fp32 oracle with nothing changed but the sigmoid reaches 20 - 55
on the same cases on the CPU (the rounding of -x log2(e) ahead of the hardware 2^t costs several ulp per sigmoid, so the
kernels' logits carry 3 - 4 x torch's error), and order='reversed' cannot show it because it leaves every logit's own sum alone.
Both are the arithmetic the kernels state, not a summation defect, so they belong in the yardstick: what one ulp of every
logit is worth in each row, instead of one sample of it.  The margin stays.  MARGIN = 16 is the factor tests/test_models_gpu.py already grants
the kernels' sequential accumulation against torch's pairwise sums; the ratios measured on the GPU stand in
tests/test_graph_ops_gpu.py and DESIGN.md.  Nothing is masked or skipped: every row of every case is compared.
"""
import collections
import functools
import zlib

import torch

from oracle.models_ref import SRGNNLayer, edge_softmax, segment_softmax, segment_sum

F64, F32 = torch.float64, torch.float32
MARGIN = 16.0

# in-degrees of edge_graph: every lane-trip boundary of `for j = lane; j < deg; j += 64` up to the LDS budget of 256
EDGE_DEGREES = [0, 1, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256] + [4] * 40
# session lengths: the 4-wave x 4-row grouping (16 nodes), the 8-row unroll tails and the 64-lane soft-max trips up to 256
SESSION_LENS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 255, 256]
GRU_DEGREES = [0, 1, 2, 3, 9, 64, 130] + [2] * 20
WMEAN_DEGREES = [300, 0, 1, 2, 5, 64, 65] + [3] * 30


# ------------------------------------------------------------------------------------------------------------ the oracles
def _flip(order, *ts):
    assert order in (None, 'reversed'), order
    return [t.flip(0) for t in ts] if order == 'reversed' else list(ts)


class _KernelSigmoid(torch.autograd.Function):
    """sigmoidf_ of csrc/common.h restated in fp32 torch: 1 / (1 + __expf(-x)), where __expf(y) is the hardware's 2^t on
    t = y * log2(e) ROUNDED to fp32 - the rounding of t moves the result by up to |x| 2^-24 relative, several ulp for the
    arguments met here, where torch.sigmoid stays within one.  The backward is s (1 - s) on the same s, as the kernels
    recompute it.  (2^t itself is taken exactly and rounded once.)"""

    @staticmethod
    def forward(ctx, x):
        assert x.dtype == F32, x.dtype
        t = (-x) * torch.tensor(1.4426950408889634, dtype=F32)
        s = 1.0 / (1.0 + torch.exp2(t.double()).float())
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return g * s * (1.0 - s)


def _sigmoid(kind, dtype):
    assert kind in ('torch', 'kernel'), kind
    return _KernelSigmoid.apply if kind == 'kernel' and dtype == F32 else torch.sigmoid


def _nudged(e, nudge):
    """the fp32 logits e [n, 1] displaced by nudge (+1 / -1) ulp, in alternating directions from one logit to the next (a
    common shift would cancel in the soft-max): what the resolution of an fp32 logit alone does to everything behind it"""
    if not nudge:
        return e
    assert e.dtype == F32 and nudge in (1, -1), (e.dtype, nudge)
    a = e.detach().abs()
    ulp = torch.nextafter(a, torch.full_like(a, float('inf'))) - a
    sign = 1.0 - 2.0 * (torch.arange(e.shape[0]) % 2).to(F32).reshape(e.shape)
    return e + nudge * sign * ulp


def sgat_ref(Q, K, we, Vf, src, dst, dtype=F64, order=None, keep=None, sigmoid='torch', nudge=0):
    """e_uv = fc_e(sigmoid(q_u + k_v)); a = softmax over the in-edges of v; out_v = sum_u a_uv v_u (oracle SGAT after its
    fc_q / fc_k / fc_v).  Q, K, Vf [n, .] (rows no edge touches give zero rows), we [1, Hh] -> out [n, Do].
    keep: a dict that receives the logits `e` with their gradient retained;  sigmoid='kernel' (fp32 only): the kernels'
    formulation of the sigmoid (_KernelSigmoid) instead of torch's;  nudge=+1 / -1 (fp32 only): every logit displaced by one ulp
    (_nudged)"""
    Q, K, we, Vf = (t.to(dtype) for t in (Q, K, we, Vf))
    src, dst = _flip(order, src, dst)
    n = Q.shape[0]
    e = _nudged(_sigmoid(sigmoid, dtype)(Q[src] + K[dst]) @ we.reshape(-1, 1), nudge)
    if keep is not None:
        e.retain_grad()
        keep['e'] = e
    a = edge_softmax(dst, e, n)
    return torch.zeros(n, Vf.shape[1], dtype=dtype).index_add_(0, dst, Vf[src] * a)


def seg_attn_ref(U, Vq, we, X, lens, dtype=F64, order=None, sigmoid='torch', nudge=0):
    """e_i = fc_e(sigmoid(u_i + v_b)); alpha = softmax over the session; out_b = sum_i alpha_i x_i (oracle AttnReadout
    after fc_u / fc_v).  lens [B] int64, one entry per row of Vq (0 for a dead session); the rows of U and X behind
    sum(lens) are padding -> out [B, D]"""
    U, Vq, we, X = (t.to(dtype) for t in (U, Vq, we, X))
    n = int(lens.sum())
    U, X = U[:n], X[:n]
    if order == 'reversed':             # all nodes back to front: the segments stay contiguous, every session is reversed
        U, X, Vq, lens = U.flip(0), X.flip(0), Vq.flip(0), lens.flip(0)
    sid = torch.repeat_interleave(torch.arange(len(lens)), lens)
    e = _nudged(_sigmoid(sigmoid, dtype)(U + Vq[sid]) @ we.reshape(-1, 1), nudge)
    alpha = segment_softmax(lens, e)
    out = segment_sum(lens, X * alpha)
    return out.flip(0) if order == 'reversed' else out


def gru_seq_ref(GI, Whh, bhh, src, dst, dtype=F64, order=None):
    """per node, a GRU cell stepped over the node's in-edges in edge-id order on the precomputed input projections GI[src],
    h0 = 0 -> the last hidden state [n, D] (zero rows for in-degree 0).  Runs on the device of its arguments."""
    assert order in (None, 'reversed'), order
    GI, Whh, bhh = (t.to(dtype) for t in (GI, Whh, bhh))
    n, D = GI.shape[0], Whh.shape[1]
    ins = [[] for _ in range(n)]
    for e, v in enumerate(dst.tolist()):
        ins[v].append(e)
    src = src.tolist()
    rows = []
    for v in range(n):
        h = torch.zeros(D, dtype=dtype, device=GI.device)
        for e in ins[v]:
            gi = GI[src[e]]
            gh = (Whh.flip(1) @ h.flip(0) if order == 'reversed' else Whh @ h) + bhh
            r = torch.sigmoid(gi[:D] + gh[:D])
            z = torch.sigmoid(gi[D:2 * D] + gh[D:2 * D])
            c = torch.tanh(gi[2 * D:] + r * gh[2 * D:])
            h = (1 - z) * c + z * h
        rows.append(h)
    return torch.stack(rows)


def wmean_ref(x, src, dst, w, dtype=F64, order=None, reverse=False):
    """SRGNNLayer._wmean: out_v = sum_{e into v} w_e x_src(e) / sum_{e into v} w_e (zero rows for in-degree 0);
    reverse=True: the same over the reversed graph (the layer's second aggregation)"""
    if reverse:
        src, dst = dst, src
    src, dst, w = _flip(order, src, dst, w)
    return SRGNNLayer._wmean(x.to(dtype), src, dst, w, x.shape[0])


def evaluate(fn, inputs, gout, dtype, **kw):
    """runs an oracle on fresh leaves of `inputs` (a dict of float tensors, fn's first arguments in order) and its backward
    on gout -> {'out': ..., 'd<name>': ...}, all CPU tensors of `dtype`"""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in inputs.items()}
    out = fn(*leaves.values(), dtype=dtype, **kw)
    out.backward(gout.to(dtype))
    res = {'out': out.detach()}
    res.update({'d' + k: t.grad for k, t in leaves.items()})
    return res


# ------------------------------------------------------------------------------------------------------------ the comparator
def rows_close(hip, ref64, yard32, what, margin=MARGIN, info=None, one_row=False):
    """asserts the rule of the module docstring for every row; yard32: the fp32 oracle's result, or several (E is then the
    larger error per row); info = (label, per-row values) names the failing row's
    in-degree / session length; one_row: the whole tensor is one row (d fc_e, d W_hh, d b_hh) -> the largest ratio
    error / max(E[row], median(E)) over the rows (what the GPU tests record)"""
    yards = list(yard32) if isinstance(yard32, (list, tuple)) else [yard32]
    hip, ref64, *yards = (torch.as_tensor(t).detach().to('cpu', F64) for t in [hip, ref64] + yards)
    assert all(t.shape == ref64.shape for t in [hip] + yards), (what, hip.shape, ref64.shape, [t.shape for t in yards])
    rows = 1 if one_row or hip.dim() < 2 else hip.shape[0]
    hip, ref64, *yards = (t.reshape(rows, -1) for t in [hip, ref64] + yards)
    if hip.numel() == 0:
        return 0.0
    E = torch.stack([(y - ref64).abs().amax(1) for y in yards]).amax(0)
    unit = torch.maximum(E, E.median())
    err = (hip - ref64).abs().amax(1)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float('inf')))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / unit)        # (an error over a zero unit: inf)
    bad = torch.nonzero(~(err <= margin * unit)).flatten()
    if len(bad):
        r = int(bad[ratio[bad].argmax()])
        where = '' if info is None else ', %s %d' % (info[0], int(info[1][r]))
        raise AssertionError('%s: row %d%s: max abs error %.3e against float64, the fp32 oracle has %.3e here (median over the '
                             'rows %.3e): ratio %.1f > %g; %d of %d rows fail'
                             % (what, r, where, float(err[r]), float(E[r]), float(E.median()), float(ratio[r]), margin,
                                len(bad), len(err)))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------ the graphs
Graph = collections.namedtuple('Graph', 'n n_cap E src dst deg in_ptr in_idx out_ptr out_idx')


def _csr(key, n, n_cap):
    """edge ids grouped by key in edge-id order; the entries of ptr behind the live count repeat the last live value, as
    batch.FlatBatch pads them"""
    order = torch.sort(key, stable=True).indices
    ptr = torch.zeros(n_cap + 1, dtype=torch.int64)
    ptr[1:n + 1] = torch.cumsum(torch.bincount(key, minlength=n), 0)
    ptr[n + 1:] = ptr[n]
    return ptr, order


def _graph(degrees, seed, cap_extra, hub=None, hub_edges=0, no_out=None):
    """a graph with exactly the in-degrees `degrees`, edge ids shuffled over the destinations, sources drawn from every node
    but `no_out`, `hub_edges` edges re-pointed to the source `hub`, `cap_extra` padded nodes behind the live ones"""
    g = torch.Generator().manual_seed(seed)
    deg = torch.tensor(degrees, dtype=torch.int64)
    n, E = len(degrees), int(deg.sum())
    dst = torch.repeat_interleave(torch.arange(n), deg)[torch.randperm(E, generator=g)]
    pool = torch.tensor([v for v in range(n) if v != no_out])
    src = pool[torch.randint(0, len(pool), (E,), generator=g)]
    if hub_edges:
        src[torch.randperm(E, generator=g)[:hub_edges]] = hub
    in_ptr, in_idx = _csr(dst, n, n + cap_extra)
    out_ptr, out_idx = _csr(src, n, n + cap_extra)
    return Graph(n, n + cap_extra, E, src, dst, deg, in_ptr, in_idx, out_ptr, out_idx)


@functools.lru_cache(maxsize=None)
def edge_graph(seed=0, cap_extra=0):
    """53 live nodes, 1254 edges, in-degrees EDGE_DEGREES; node 0 is the source of >= 300 edges, node 1 of none"""
    return _graph(EDGE_DEGREES, 100 + seed, cap_extra, hub=0, hub_edges=300, no_out=1)


@functools.lru_cache(maxsize=None)
def gru_graph(seed=0, cap_extra=5):
    """27 live nodes with in-degrees GRU_DEGREES (249 GRU steps, the longest chain 130), 5 padded nodes"""
    return _graph(GRU_DEGREES, 200 + seed, cap_extra)


@functools.lru_cache(maxsize=None)
def wmean_graph(seed=0, cap_extra=0):
    """37 live nodes: node 0 has in-degree 300, node 1 in-degree 0, node 2 out-degree 0"""
    return _graph(WMEAN_DEGREES, 300 + seed, cap_extra, no_out=2)


Sessions = collections.namedtuple('Sessions', 'B B_cap N N_cap lens seg')


@functools.lru_cache(maxsize=None)
def session_lens(dead=False):
    """the sessions SESSION_LENS; dead=True: 3 dead sessions and 11 padded node rows behind them (seg repeats its last live
    value).  lens has one entry per row of the batch (0 for the dead ones)"""
    B, N = len(SESSION_LENS), sum(SESSION_LENS)
    B_cap, N_cap = (B + 3, N + 11) if dead else (B, N)
    lens = torch.tensor(SESSION_LENS + [0] * (B_cap - B), dtype=torch.int64)
    seg = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    return Sessions(B, B_cap, N, N_cap, lens, seg)


# ------------------------------------------------------------------------------------------------------------ the cases
# A case is a hashable record; inputs(case) draws its tensors (padded rows hold random values the kernels must ignore),
# reference(case) evaluates the float64 oracle and the fp32 yardstick once per process.
SgatCase = collections.namedtuple('SgatCase', 'Hh Do scale cap_extra strided seed', defaults=(1.0, 0, False, 0))
SegCase = collections.namedtuple('SegCase', 'h D scale dead strided seed', defaults=(1.0, False, False, 0))
GruCase = collections.namedtuple('GruCase', 'D seed', defaults=(0,))
WmeanCase = collections.namedtuple('WmeanCase', 'D cap_extra seed', defaults=(0, 0))

SGAT_CASES = ([SgatCase(Hh, Do, 1.0, cap) for Hh, Do in ((32, 32), (1, 4), (64, 256), (65, 260), (130, 260), (100, 516))
               for cap in (0, 7)]
              + [SgatCase(32, 32, 8.0, 0), SgatCase(130, 260, 8.0, 7), SgatCase(65, 260, 1.0, 7, True)])
# seg_attn: the error of the session-wide sums (the soft-max denominator, sum_i alpha_i dalpha_i) is shared by all rows of a
# session and can exceed a row's own E by the square root of the session length, so a sequential fp32 sum in ANOTHER order
# passes the rule only for some draws of a case with 255- and 256-node sessions.  A case's seed is the first one at which the
# reversed-order fp32 oracle stays within 12 of the plain fp32 run's E alone (test_graph_oracle_cpu.py requires 16, with all
# yardsticks): chosen on the CPU from oracle runs, never from a kernel's output.
SEG_CASES = ([SegCase(h, D) for h, D in ((4, 4), (32, 128), (48, 96), (100, 400))]
             + [SegCase(256, 1024, seed=4), SegCase(260, 260), SegCase(512, 516, seed=6),
                SegCase(32, 128, 1.0, True), SegCase(260, 260, 1.0, True), SegCase(48, 96, 1.0, True, True),
                SegCase(100, 400, 8.0, True, seed=4)])
# (33: the first width on the streaming kernels, forward only - the backward's launchers take multiples of 4; 36: the first such)
GRU_CASES = [GruCase(D) for D in (8, 32, 33, 36, 64, 96, 100, 256)]
WMEAN_CASES = [WmeanCase(D, cap) for D in (4, 32, 100, 260) for cap in (0, 6)]


def case_id(c):
    return '-'.join('%s%g' % (k, v) for k, v in zip(c._fields, c) if not isinstance(v, bool) or v)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def inputs(case):
    """-> (oracle function, {input name: fp32 CPU tensor}, gout, keyword arguments of the oracle, graph or sessions)"""
    return _inputs(type(case).__name__, case)       # (records of two kinds with equal fields are equal tuples)


@functools.lru_cache(maxsize=None)
def _inputs(kind, case):
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    if isinstance(case, SgatCase):
        G = edge_graph(0, case.cap_extra)
        x = dict(Q=_randn(g, G.n_cap, case.Hh), K=_randn(g, G.n_cap, case.Hh), we=_randn(g, 1, case.Hh) * case.scale,
                 Vf=_randn(g, G.n_cap, case.Do))
        return sgat_ref, x, _randn(g, G.n_cap, case.Do), dict(src=G.src, dst=G.dst), G
    if isinstance(case, SegCase):
        S = session_lens(case.dead)
        x = dict(U=_randn(g, S.N_cap, case.h), Vq=_randn(g, S.B_cap, case.h), we=_randn(g, 1, case.h) * case.scale,
                 X=_randn(g, S.N_cap, case.D))
        return seg_attn_ref, x, _randn(g, S.B_cap, case.D), dict(lens=S.lens), S
    if isinstance(case, GruCase):
        G, D = gru_graph(), case.D
        x = dict(GI=_randn(g, G.n_cap, 3 * D), Whh=_randn(g, 3 * D, D) / D ** 0.5, bhh=_randn(g, 3 * D) * 0.1)
        return gru_seq_ref, x, _randn(g, G.n_cap, D), dict(src=G.src, dst=G.dst), G
    assert isinstance(case, WmeanCase), case
    G = wmean_graph(0, case.cap_extra)
    w = torch.randint(1, 10, (G.E,), generator=g)
    return wmean_ref, dict(x=_randn(g, G.n_cap, case.D)), _randn(g, G.n_cap, case.D), dict(src=G.src, dst=G.dst, w=w), G


def run(case, dtype, **kw):
    fn, x, gout, args, _ = inputs(case)
    return evaluate(fn, x, gout, dtype, **args, **kw)


def reference(case, reverse=False):
    """(float64 results, fp32 results, [every fp32 yardstick of the case]) computed once and shared: treat them as read-only.
    The attention ops have four yardsticks: the oracle as it is, with the kernels' sigmoid, with the logits displaced by one
    ulp either way (module docstring).
    reverse: the second aggregation of a WmeanCase"""
    return _reference(type(case).__name__, case, reverse)


@functools.lru_cache(maxsize=None)
def _reference(kind, case, reverse):
    kw = dict(reverse=True) if reverse else {}
    yards = [run(case, F32, **kw)]
    if kind in ('SgatCase', 'SegCase'):
        yards += [run(case, F32, sigmoid='kernel'), run(case, F32, nudge=1), run(case, F32, nudge=-1)]
    return run(case, F64, **kw), yards[0], yards


def row_info(case, name):
    """(label, per-row values) for rows_close's message: the in-degree of a node row / the length of a session row"""
    _, x, _, _, G = inputs(case)
    if isinstance(case, SegCase):
        if name in ('dU', 'dX'):
            lens = torch.repeat_interleave(G.lens, G.lens)
            return 'session length', torch.cat([lens, torch.zeros(G.N_cap - G.N, dtype=torch.int64)])
        return 'session length', G.lens
    return 'in-degree', torch.cat([G.deg, torch.zeros(G.n_cap - G.n, dtype=torch.int64)])


ONE_ROW = ('dwe', 'dWhh', 'dbhh')


def compare(case, got, names=None, reverse=False, live_only=()):
    """rows_close of every quantity in `got` (a dict like evaluate's) against reference(case) -> {name: largest ratio}.
    live_only: quantities whose padded rows the op leaves unwritten by contract (compared on the live rows)"""
    ref64, _, yards = reference(case, reverse)
    G = inputs(case)[4]
    out = {}
    for k in names or sorted(ref64):
        a, r, y = got[k], ref64[k], [yd[k] for yd in yards]
        label, vals = row_info(case, k)
        if k in live_only:
            a, r, y, vals = a[:G.n], r[:G.n], [t[:G.n] for t in y], vals[:G.n]
        one = k in ONE_ROW
        out[k] = rows_close(a, r, y, '%s %s' % (case_id(case), k), MARGIN, None if one else (label, vals), one_row=one)
    return out
