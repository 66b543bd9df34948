"""tests/graph_oracle.py checked on the CPU: each float64 oracle equals the oracle MODULE it restates (models_ref.SGAT,
AttnReadout, EOPA, SRGNNLayer._wmean); the bound of rows_close is not too tight - for every case of
tests/test_graph_ops_gpu.py the fp32 oracle with every sum in reversed order passes it at the margin the kernels get - and
tight enough: seeded defects of the kind a kernel would have (a dropped in-edge at a lane-trip / LDS-budget boundary, a skipped
session node, missing trailing columns, a wrong GRU edge order, a dirty padded row, a missing factor in one row of dK) are
each rejected; the generators produce exactly the degrees and lengths they declare, up to the kernels' static budgets."""
import pytest
import torch

import graph_oracle as go
from graph_oracle import F32, F64
from oracle import models_ref as om
from util import pkg

ALL_CASES = go.SGAT_CASES + go.SEG_CASES + go.GRU_CASES + go.WMEAN_CASES


# ------------------------------------------------------------------------------------------------------------ anchoring
def test_sgat_oracle_equals_the_oracle_module():
    G = go.edge_graph(0, 0)
    torch.manual_seed(1)
    m = om.SGAT(24, 20, 12, batch_norm=False).double()
    feat = torch.randn(G.n, 24, dtype=F64)
    want = m({'src': G.src, 'dst': G.dst}, feat)
    got = go.sgat_ref(m.fc_q(feat), m.fc_k(feat), m.fc_e.weight, m.fc_v(feat), G.src, G.dst)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-15)
    rev = go.sgat_ref(m.fc_q(feat), m.fc_k(feat), m.fc_e.weight, m.fc_v(feat), G.src, G.dst, order='reversed')
    assert torch.allclose(rev, want, rtol=1e-12, atol=1e-14) and not torch.equal(rev, want)


def test_seg_attn_oracle_equals_the_oracle_module():
    S = go.session_lens(True)
    torch.manual_seed(2)
    m = om.AttnReadout(16, 12, 16, batch_norm=False).double()
    feat = torch.randn(S.N, 16, dtype=F64)
    last = S.seg[1:S.B + 1] - 1
    want = m({'num_nodes': S.lens[:S.B]}, feat, last)
    pad = torch.randn(S.N_cap - S.N, 16, dtype=F64)                      # padded node rows / dead sessions: ignored, zero rows
    X = torch.cat([feat, pad])
    Vq = torch.cat([m.fc_v(feat[last]), torch.randn(S.B_cap - S.B, 12, dtype=F64)])
    for order in (None, 'reversed'):
        got = go.seg_attn_ref(m.fc_u(X), Vq, m.fc_e.weight, X, S.lens, order=order)
        assert torch.allclose(got[:S.B], want, rtol=1e-12, atol=1e-14)
        assert got.shape == (S.B_cap, 16) and float(got[S.B:].detach().abs().max()) == 0.0


def test_gru_seq_oracle_equals_the_oracle_module():
    G = go.gru_graph(0, 0)
    torch.manual_seed(3)
    D = 10
    m = om.EOPA(D, D, batch_norm=False).double()
    with torch.no_grad():                                                # the module's output = the neighbour state
        m.fc_self.weight.zero_()
        m.fc_neigh.weight.copy_(torch.eye(D))
    feat = torch.randn(G.n, D, dtype=F64)
    want = m({'src': G.src, 'dst': G.dst}, feat)
    GI = feat @ m.gru.weight_ih_l0.t() + m.gru.bias_ih_l0
    for order in (None, 'reversed'):
        got = go.gru_seq_ref(GI, m.gru.weight_hh_l0, m.gru.bias_hh_l0, G.src, G.dst, order=order)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    assert float(got[0].detach().abs().max()) == 0.0                     # in-degree 0


def test_wmean_oracle_equals_the_oracle_layer():
    G = go.wmean_graph(0, 0)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(G.n, 8, generator=g, dtype=F64)
    w = torch.randint(1, 10, (G.E,), generator=g)
    assert torch.equal(go.wmean_ref(x, G.src, G.dst, w), om.SRGNNLayer._wmean(x, G.src, G.dst, w, G.n))
    assert torch.equal(go.wmean_ref(x, G.src, G.dst, w, reverse=True), om.SRGNNLayer._wmean(x, G.dst, G.src, w, G.n))
    rev = go.wmean_ref(x, G.src, G.dst, w, order='reversed')
    assert torch.allclose(rev, go.wmean_ref(x, G.src, G.dst, w), rtol=1e-13, atol=1e-15)
    assert float(go.wmean_ref(x, G.src, G.dst, w)[1].abs().max()) == 0.0            # in-degree 0
    assert float(go.wmean_ref(x, G.src, G.dst, w, reverse=True)[2].abs().max()) == 0.0   # out-degree 0


# ------------------------------------------------------------------------------------------------------------ the generators
def test_generators_produce_the_declared_degrees_and_lengths():
    for cap in (0, 7):
        G = go.edge_graph(0, cap)
        assert (G.n, G.n_cap, G.E) == (53, 53 + cap, 1254)
        assert torch.bincount(G.dst, minlength=G.n).tolist() == go.EDGE_DEGREES
        out_deg = torch.bincount(G.src, minlength=G.n)
        assert int(out_deg[0]) >= 300 and int(out_deg[1]) == 0
        assert not torch.equal(G.in_idx, torch.arange(G.E))                          # shuffled edge ids
        for ptr, idx, key in ((G.in_ptr, G.in_idx, G.dst), (G.out_ptr, G.out_idx, G.src)):
            assert len(ptr) == G.n_cap + 1 and int(ptr[G.n]) == G.E and bool((ptr[G.n:] == G.E).all())
            assert sorted(idx.tolist()) == list(range(G.E))
            for v in range(G.n):
                mine = idx[ptr[v]:ptr[v + 1]]
                assert bool((key[mine] == v).all()) and bool((mine[1:] > mine[:-1]).all())    # edge-id order
    G = go.gru_graph()
    assert torch.bincount(G.dst, minlength=G.n).tolist() == go.GRU_DEGREES and G.n_cap == G.n + 5
    for cap in (0, 6):
        G = go.wmean_graph(0, cap)
        ind, outd = torch.bincount(G.dst, minlength=G.n), torch.bincount(G.src, minlength=G.n)
        assert ind.tolist() == go.WMEAN_DEGREES and int(ind[0]) == 300 and int(ind[1]) == 0 and int(outd[2]) == 0
    S, Sd = go.session_lens(False), go.session_lens(True)
    assert S.lens.tolist() == go.SESSION_LENS and (S.B, S.B_cap, S.N_cap) == (18, 18, S.N)
    assert Sd.lens.tolist() == go.SESSION_LENS + [0, 0, 0] and (Sd.B_cap, Sd.N_cap) == (21, Sd.N + 11)
    assert Sd.seg.tolist()[-4:] == [Sd.N] * 4 and len(Sd.seg) == Sd.B_cap + 1


def test_generators_reach_the_kernels_budgets_exactly():
    """the largest in-degree of edge_graph is the SGAT kernels' LDS budget, the longest session the read-out's"""
    try:
        L = pkg('ops').limits()
    except (OSError, RuntimeError) as e:
        pytest.skip('libsrec_hip.so is not built: %s' % e)
    assert max(go.EDGE_DEGREES) == L['sgat_deg'] and max(go.SESSION_LENS) == L['nodes']


# ------------------------------------------------------------------------------------------------------------ the bound
@pytest.mark.parametrize('case', ALL_CASES, ids=go.case_id)
def test_the_bound_admits_another_summation_order(case):
    """a correct fp32 implementation that sums in another order stays inside the bound the kernels are held to"""
    got = go.run(case, F32, order='reversed')
    ratios = go.compare(case, got)
    assert len(ratios) == len(go.inputs(case)[1]) + 1 and max(ratios.values()) <= go.MARGIN
    if isinstance(case, go.WmeanCase):
        go.compare(case, go.run(case, F32, order='reversed', reverse=True), reverse=True)


def _rejected(case, got, name):
    yard32 = go.reference(case)[1]
    with pytest.raises(AssertionError, match=name):
        go.compare(case, got, names=[name])
    go.compare(case, yard32, names=[name])                                # (the unharmed run passes)


def _moderate(cases, **kw):
    c = [c for c in cases if c.scale == 1.0 and all(getattr(c, k) == v for k, v in kw.items())]
    return c[0]


@pytest.mark.parametrize('pos', [64, 128, 255])
def test_a_dropped_in_edge_is_rejected(pos):
    """the in-edge at position 64 / 128 / 255 of a node's list: what a wrong lane-trip bound or an LDS budget one too small
    would lose"""
    case = _moderate(go.SGAT_CASES, Hh=130, Do=260, cap_extra=0)
    fn, x, gout, args, G = go.inputs(case)
    v = go.EDGE_DEGREES.index(pos + 1)
    e = int(G.in_idx[G.in_ptr[v] + pos])
    keep = torch.arange(G.E) != e
    got = go.evaluate(fn, x, gout, F32, src=G.src[keep], dst=G.dst[keep])
    _rejected(case, got, 'out')
    _rejected(case, got, 'dK')
    with pytest.raises(AssertionError, match='row %d, in-degree %d' % (v, pos + 1)):
        go.compare(case, got, names=['out'])


def test_a_skipped_session_node_is_rejected():
    case = _moderate(go.SEG_CASES, h=48, D=96, dead=False)
    fn, x, gout, args, S = go.inputs(case)
    b = go.SESSION_LENS.index(33)
    row = int(S.seg[b]) + 16                                             # the 17th node: the first of the second 16-node group
    keep = torch.arange(S.N_cap) != row
    lens = S.lens.clone()
    lens[b] -= 1
    out = fn(x['U'][keep], x['Vq'], x['we'], x['X'][keep], lens, dtype=F32)
    _rejected(case, {'out': out}, 'out')
    with pytest.raises(AssertionError, match='row %d, session length 33' % b):
        go.compare(case, {'out': out}, names=['out'])


def test_missing_trailing_columns_are_rejected():
    """columns 256 .. 259 of a 260-wide row: the second trip of `for c = lane * 4; c < D; c += 256`"""
    for case in (_moderate(go.SGAT_CASES, Hh=65, Do=260, cap_extra=0), _moderate(go.SEG_CASES, h=260, D=260, dead=False),
                 go.WmeanCase(260, 0)):
        got = {k: v.clone() for k, v in go.reference(case)[1].items()}
        got['out'][:, 256:] = 0
        _rejected(case, got, 'out')
    case = _moderate(go.SEG_CASES, h=260, D=260, dead=False)
    got = {k: v.clone() for k, v in go.reference(case)[1].items()}
    got['dU'][:, 256:] = 0
    _rejected(case, got, 'dU')


def test_a_wrong_gru_edge_order_is_rejected():
    case = go.GruCase(96)
    fn, x, gout, args, G = go.inputs(case)
    v = go.GRU_DEGREES.index(9)
    mine = G.in_idx[G.in_ptr[v]:G.in_ptr[v + 1]]
    src = G.src.clone()
    a, b = int(mine[3]), int(mine[4])
    assert int(src[a]) != int(src[b])
    src[a], src[b] = G.src[b], G.src[a]                                  # the two edges visited in swapped order
    got = go.evaluate(fn, x, gout, F32, src=src, dst=G.dst)
    _rejected(case, got, 'out')
    with pytest.raises(AssertionError, match='row %d, in-degree 9' % v):
        go.compare(case, got, names=['out'])


def test_a_dirty_padded_row_is_rejected():
    for case, name, live in ((_moderate(go.SGAT_CASES, Hh=32, Do=32, cap_extra=7), 'dK', 12),
                             (_moderate(go.SEG_CASES, h=32, D=128, dead=True), 'dX', 2),
                             (_moderate(go.SEG_CASES, h=32, D=128, dead=True), 'out', 2), (go.GruCase(33), 'out', 2),
                             (go.WmeanCase(32, 6), 'out', 2)):
        got = {k: v.clone() for k, v in go.reference(case)[1].items()}
        assert float(got[name][-1].abs().max()) == 0.0 and float(got[name][live].abs().max()) > 0.0
        got[name][-1] = got[name][live]                                  # a live row's values behind the live count
        _rejected(case, got, name)


def test_a_missing_factor_in_one_row_of_dk_is_rejected():
    """dK_v = sum_j de_j we sg (1 - sg): without the sg (1 - sg) factor in the row of one node"""
    case = _moderate(go.SGAT_CASES, Hh=32, Do=32, cap_extra=0)
    fn, x, gout, args, G = go.inputs(case)
    keep = {}
    leaves = {k: t.clone().requires_grad_() for k, t in x.items()}
    fn(*leaves.values(), dtype=F32, keep=keep, **args).backward(gout)
    got = {'dK': leaves['K'].grad.clone()}
    go.compare(case, got, names=['dK'])
    v = go.EDGE_DEGREES.index(65)
    de = keep['e'].grad[G.dst == v]                                      # [65, 1]
    got['dK'][v] = (de * x['we']).sum(0)
    _rejected(case, got, 'dK')
