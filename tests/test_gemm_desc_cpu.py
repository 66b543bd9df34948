"""The problem table of a gemm16 launch (ops.gemm16_desc -> srec_gemm16_group, include/srec_hg.h) as the named problem record
ops.GemmProb fills it.  CPU only: `ptr` is pointed at Tensor.data_ptr and nothing is launched."""
import ctypes

import pytest
import torch

from util import pkg


@pytest.fixture
def ops(monkeypatch):
    o = pkg('ops')
    monkeypatch.setattr(o, 'ptr', lambda t: None if t is None else t.data_ptr())
    return o


def _problem(M=5, N=16, K=32):
    A, B, C = torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(N, K, dtype=torch.bfloat16), torch.zeros(M, N)
    return (M, N, K, [(A, B)], C, torch.zeros(1, dtype=torch.int32))


def _bytes(g):
    return ctypes.string_at(ctypes.addressof(g), ctypes.sizeof(g))


def test_tuple_and_record_fill_the_same_struct(ops):
    tup = _problem()
    a = ops.gemm16_desc([tup], 32, 32, 16, beta=1.0)
    b = ops.gemm16_desc([ops.GemmProb(*tup)], 32, 32, 16, beta=1.0)
    assert _bytes(a) == _bytes(b)
    assert (a.np, a.lda, a.ldb, a.ldc, a.beta, a.c16) == (1, 32, 32, 16, 1.0, 0)
    assert (a.M[0], a.N[0], a.K[0], a.nseg[0]) == (5, 16, 32, 1)
    assert (a.A[0][0], a.B[0][0], a.C[0], a.dyn[0]) == (tup[3][0][0].data_ptr(), tup[3][0][1].data_ptr(), tup[4].data_ptr(),
                                                       tup[5].data_ptr())
    # the defaults
    assert (a.koff[0], a.nsplit[0], a.lda_p[0], a.ldb_p[0], a.ldc_p[0], a.mhint[0]) == (0, 1, 0, 0, 0, 0)


def test_optional_fields_land_in_their_problem_slot(ops):
    plain, other = _problem(), _problem(7, 8, 64)
    g = ops.gemm16_desc([plain, ops.GemmProb(*other, nsplit=3, koff=64, ld=(40, 48, 56), mhint=77), plain], 32, 32, 16)
    assert g.np == 3
    assert (g.koff[1], g.nsplit[1], g.lda_p[1], g.ldb_p[1], g.ldc_p[1], g.mhint[1]) == (64, 3, 40, 48, 56, 77)
    assert (g.M[1], g.N[1], g.K[1], g.C[1]) == (7, 8, 64, other[4].data_ptr())
    for p in (0, 2):
        assert (g.koff[p], g.nsplit[p], g.lda_p[p], g.ldb_p[p], g.ldc_p[p], g.mhint[p]) == (0, 1, 0, 0, 0, 0)
    assert all(g.nsplit[p] == 0 and g.M[p] == 0 for p in range(3, ops.G16_MAXP))      # unused slots stay zero


def test_flag_bits_are_the_headers(ops):
    C = ops.CONST
    assert ops.gemm16_desc([_problem()], 32, 32, 16, c16=True, keep_dead=True).c16 == C['SREC_G16_KEEP_DEAD'] | C['SREC_G16_C_BF16']
    assert ops.gemm16_desc([_problem()], 32, 32, 16, c16=True).c16 == C['SREC_G16_C_BF16']
    assert ops.gemm16_desc([_problem()], 32, 32, 16, keep_dead=True).c16 == C['SREC_G16_KEEP_DEAD']
    assert (C['SREC_G16_C_BF16'], C['SREC_G16_KEEP_DEAD']) == (1, 2)
    assert [C['SREC_HG_' + n] for n in ('P16_BF16', 'SKIP_DEAD_DP', 'LATE_DX', 'FOLDED')] == [1, 2, 4, 8]


def test_too_many_problems_assert(ops):
    ops.gemm16_desc([_problem()] * ops.G16_MAXP, 32, 32, 16)
    with pytest.raises(AssertionError):
        ops.gemm16_desc([_problem()] * (ops.G16_MAXP + 1), 32, 32, 16)
    with pytest.raises(AssertionError):
        ops.gemm16_desc([], 32, 32, 16)
