"""The graph kernels of LESSR, SRGNN and NISER at operator level, row by row against the float64 oracles of
tests/graph_oracle.py: ops.sgat_attn (csrc/sgat.hip), ops.seg_attn (csrc/segops.hip), ops.gru_seq (csrc/gruseq.hip) and
ops.edge_coef + ops.edge_agg as gnn.srgnn_layer calls them - forward and every input gradient, at in-degrees and session lengths
on both sides of every lane trip up to the LDS budgets (in-degree 256, 256-node sessions), widths on both sides of the 64-lane
and 256-column trips, peaked soft-max logits, row-strided operands, capacity padding with a device live count.

Every row of every quantity is held to graph_oracle.rows_close at margin 16 (error against float64 <= 16 x the larger of the
fp32 oracle's own error in that row and its median over the rows; the attention ops take the largest of four fp32 runs, see
graph_oracle's docstring for the measurement behind that); padded / dead rows must be exactly zero where the op promises it;
every result is finite although the allocator hands the backward a block of NaNs; a second run is bit-identical.

Largest ratio error / max(E[row], median(E)) measured on an MI355X per op and quantity, over all cases of the op (bound: 16):
    sgat_attn   out 3.03  dQ 11.73  dK 6.98  dVf 10.11  dwe 0.84   (logits x 8: dQ, dK, dVf; moderate logits 4.18 / 2.93 / 2.66)
    seg_attn    out 2.57  dU 11.03  dVq 1.96  dX 12.55  dwe 0.79   (logits x 8: dU, dX; moderate logits 7.53 / 7.48)
    gru_seq     out 3.03  dGI 3.96  dWhh 1.58  dbhh 1.70
    edge_agg    out 4.67  dx 2.44                                  (edge_coef's weights inside; both directions)
Each test prints its ratios (pytest -s).
"""
import pytest
import torch

import graph_oracle as go
from util import pkg

pytestmark = pytest.mark.gpu


def _dev_graph(G, dev):
    return tuple(t.to(torch.int32).to(dev) for t in (G.in_ptr, G.in_idx, G.out_ptr, G.out_idx, G.src, G.dst))


def _dyn(n, dev):
    return torch.tensor([n], dtype=torch.int32, device=dev)


def _leaf(t, dev, strided=False):
    """a leaf on the device; strided: a column slice of a wider tensor (row stride > width, a multiple of 4, 16-byte aligned
    start) that ops._rows hands to the kernels as a view"""
    if not strided:
        return t.to(dev).requires_grad_()
    wide = torch.randn(t.shape[0], (t.shape[1] + 3) // 4 * 4 + 12, device=dev)
    wide[:, 4:4 + t.shape[1]] = t.to(dev)
    v = wide[:, 4:4 + t.shape[1]].detach().requires_grad_()
    r = pkg('ops')._rows(v)
    assert r.data_ptr() == v.data_ptr() and r.stride() == v.stride() and v.stride(0) > v.shape[1]
    return v


def _poison(dev):
    """freed blocks of NaNs, one per pool of the caching allocator: what the next torch.empty of a backward gets"""
    for n in (200_000, 6_000_000):
        t = torch.full((n,), float('nan'), device=dev)
        del t


def _backward(out, leaves, gout, dev):
    _poison(dev)
    grads = torch.autograd.grad(out, list(leaves.values()), gout.to(dev))
    res = {'out': out.detach().cpu()}
    res.update({'d' + k: g.cpu() for k, g in zip(leaves, grads)})
    return res


def _check(case, run, zero, live_only=(), reverse=False):
    """run() -> results on the CPU; zero: {quantity: first row that must be exactly zero}"""
    got, again = run(), run()
    G = go.inputs(case)[4]
    for k, v in got.items():
        w = again[k]
        if k in live_only:                                   # (rows behind the live count: unwritten by contract)
            v, w = v[:G.n], w[:G.n]
        assert bool(torch.isfinite(v).all()), '%s %s: not finite' % (go.case_id(case), k)
        assert torch.equal(v, w), '%s %s: two runs differ' % (go.case_id(case), k)
    for k, first in zero.items():
        assert first == len(got[k]) or float(got[k][first:].abs().max()) == 0.0, \
            '%s %s: rows behind the live count are not zero' % (go.case_id(case), k)
    ratios = go.compare(case, got, names=sorted(got), live_only=live_only, reverse=reverse)
    print('RATIO %s %s %s' % (type(case).__name__, go.case_id(case), ' '.join('%s=%.2f' % kv for kv in sorted(ratios.items()))))
    return got


@pytest.mark.parametrize('case', go.SGAT_CASES, ids=go.case_id)
def test_sgat_attn_rows_match_the_float64_oracle(dev, case):
    ops = pkg('ops')
    _, x, gout, _, G = go.inputs(case)
    graph = _dev_graph(G, dev)
    dyn = _dyn(G.n, dev) if case.cap_extra else None

    def run():
        leaves = {k: _leaf(t, dev, case.strided and k != 'we') for k, t in x.items()}
        out = ops.sgat_attn(leaves['Q'], leaves['K'], leaves['we'], leaves['Vf'], graph, dyn)
        return _backward(out, leaves, gout, dev)
    _check(case, run, dict(out=G.n, dQ=G.n, dK=G.n, dVf=G.n))


@pytest.mark.parametrize('case', go.SEG_CASES, ids=go.case_id)
def test_seg_attn_rows_match_the_float64_oracle(dev, case):
    ops = pkg('ops')
    _, x, gout, _, S = go.inputs(case)
    seg = S.seg.to(torch.int32).to(dev)
    dynB = _dyn(S.B, dev) if case.dead else None

    def run():
        leaves = {k: _leaf(t, dev, case.strided and k in ('U', 'X')) for k, t in x.items()}
        out = ops.seg_attn(leaves['U'], leaves['Vq'], leaves['we'], leaves['X'], seg, dynB)
        return _backward(out, leaves, gout, dev)
    _check(case, run, dict(out=S.B, dVq=S.B, dX=S.N, dU=S.N))


def _gru_run(ops, case, dev):
    _, x, gout, _, G = go.inputs(case)
    graph = _dev_graph(G, dev)
    dyn, dynE = _dyn(G.n, dev), _dyn(G.E, dev)

    def run(backward=True):
        leaves = {k: _leaf(t, dev) for k, t in x.items()}
        out = ops.gru_seq(leaves['GI'], leaves['Whh'], leaves['bhh'], graph, dyn, dynE)
        return _backward(out, leaves, gout, dev) if backward else {'out': out.detach().cpu()}
    return run, G


@pytest.mark.parametrize('case', go.GRU_CASES, ids=go.case_id)
def test_gru_seq_rows_match_the_float64_oracle(dev, case):
    """D <= 32: the register-resident kernels; 33 .. 64: one lane trip of the streaming kernels; 96, 100: two; 256: MAXD"""
    run, G = _gru_run(pkg('ops'), case, dev)
    if case.D % 4:
        # the backward sums the per-edge records with the 16-byte row kernels and takes the weight gradients as exact-fp32
        # GEMMs over them; both take widths that are multiples of 4 (as every linear layer of the models does): the forward
        # runs at such a width, the backward is refused by the first launcher, cleanly
        _check(case, lambda: run(False), dict(out=G.n))
        with pytest.raises(RuntimeError, match=r'srec_\w+ failed with status 1001 \(bad argument'):
            run()
        torch.cuda.synchronize()
        return
    _check(case, run, dict(out=G.n), live_only=('dGI',))


def test_gru_seq_refuses_a_width_beyond_its_lds_rows(dev):
    ops = pkg('ops')
    assert ops.GRU_SEQ_MAXD == 256
    run, _ = _gru_run(ops, go.GruCase(ops.GRU_SEQ_MAXD + 1), dev)
    with pytest.raises(RuntimeError, match=r'srec_gru_seq_fwd failed with status 1001 \(bad argument'):
        run(False)
    torch.cuda.synchronize()


@pytest.mark.parametrize('case', go.WMEAN_CASES, ids=go.case_id)
def test_edge_coef_and_edge_agg_rows_match_the_float64_oracle(dev, case):
    """both aggregations of gnn.srgnn_layer: over the in-edges with w / (sum of w into the destination), over the out-edges
    with w / (sum of w out of the source); the backward of each is the same kernel on the other CSR"""
    ops = pkg('ops')
    _, x, gout, args, G = go.inputs(case)
    in_ptr, in_idx, out_ptr, out_idx, esrc, edst = _dev_graph(G, dev)
    ew = args['w'].to(torch.int32).to(dev)
    dyn = _dyn(G.n, dev) if case.cap_extra else None
    in_csr, out_csr = (in_ptr, in_idx, esrc), (out_ptr, out_idx, edst)

    for reverse in (False, True):
        def run():
            leaves = {'x': _leaf(x['x'], dev)}
            if reverse:
                coef = ops.edge_coef(out_ptr, out_idx, ew, G.n_cap, dyn)
                out = ops.edge_agg(leaves['x'], coef, out_csr, in_csr, dyn)
            else:
                coef = ops.edge_coef(in_ptr, in_idx, ew, G.n_cap, dyn)
                out = ops.edge_agg(leaves['x'], coef, in_csr, out_csr, dyn)
            return _backward(out, leaves, gout, dev)
        got = _check(case, run, dict(out=G.n, dx=G.n), reverse=reverse)
        assert float(got['out'][2 if reverse else 1].abs().max()) == 0.0          # no out-edge / no in-edge: a zero row


def test_widths_off_the_16_byte_rows_are_refused_by_the_launchers(dev):
    """Do, h or D that is no multiple of 4: the bad-argument status of the launcher, not a misaligned access"""
    ops = pkg('ops')
    G = go.edge_graph(0, 0)
    graph = _dev_graph(G, dev)
    r = lambda *s: torch.randn(*s, device=dev)
    with pytest.raises(RuntimeError, match=r'srec_sgat_fwd failed with status 1001 \(bad argument'):
        ops.sgat_attn(r(G.n, 8), r(G.n, 8), r(1, 8), r(G.n, 6), graph)
    S = go.session_lens(False)
    seg = S.seg.to(torch.int32).to(dev)
    for h, D in ((6, 8), (8, 6)):
        with pytest.raises(RuntimeError, match=r'srec_seg_attn_fwd failed with status 1001 \(bad argument'):
            ops.seg_attn(r(S.N, h), r(S.B, h), r(1, h), r(S.N, D), seg)
    W = go.wmean_graph(0, 0)
    in_ptr, in_idx, out_ptr, out_idx, esrc, edst = _dev_graph(W, dev)
    coef = ops.edge_coef(in_ptr, in_idx, torch.ones(W.E, dtype=torch.int32, device=dev), W.n)
    with pytest.raises(RuntimeError, match=r'srec_edge_agg failed with status 1001 \(bad argument'):
        ops.edge_agg(r(W.n, 6), coef, (in_ptr, in_idx, esrc), (out_ptr, out_idx, edst))
    torch.cuda.synchronize()
