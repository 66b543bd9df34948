"""srec_gemm16_tn2 (csrc/gemm16.hip): two problem families in ONE launch against one srec_gemm16_tn launch per family on the same
operands, byte for byte.  Only which workgroup carries a tile differs between the two, so nothing here needs a tolerance: every C
buffer starts from a sentinel, is followed by guard rows and carries guard columns (ldc > N in some problems), and the whole
buffers are compared."""
import ctypes
import itertools

import pytest
import torch

from util import pkg

SENT = -777.0
SHAPES = [(8, 8), (136, 128), (256, 264)]              # (M, N): one tile; two row tiles, the last 8 rows high; 2 x 3 tiles
KS = [1, 63, 64, 65, 200]                              # reduction rows around the 64-row stage
DYNS = ['0', 'K-1', 'K', '>K', 'null']                 # live count of the operand, relative to koff + K
NSPLITS = [1, 3]
KOFFS = [0, 64]
FAMILIES = [(1, 1), (12, 4), (15, 1), (1, 15)]
VARIANTS = list(itertools.product(SHAPES, KS, DYNS, NSPLITS, KOFFS))          # 300


def _tiles(v):
    (M, N), _, _, nsplit, _ = v
    return -(-M // 128) * -(-N // 128) * nsplit


class Problem:
    """one tn problem with private operands; variant i of a launch pads its leading dimensions by 8 (i % 3) / 8 (i % 2) / 4 (i % 4)"""

    def __init__(self, dev, v, i, gen):
        ops = pkg('ops')
        (M, N), K, dyn, nsplit, koff = v
        lda, ldb, self.ldc = M + 8 * (i % 3), N + 8 * (i % 2), N + 4 * (i % 4)
        rnd = lambda *s: (torch.randn(*s, device=dev, generator=gen) * 0.5).bfloat16()
        self.A, self.B = rnd(koff + K, lda), rnd(koff + K, ldb)              # the problem reduces rows koff .. koff + K
        live = {'0': 0, 'K-1': koff + K - 1, 'K': koff + K, '>K': koff + K + 70, 'null': None}[dyn]
        self.dyn = None if live is None else torch.tensor([live], device=dev, dtype=torch.int32)
        self.rows, self.guard = nsplit * M, 3
        self.mk = lambda C: ops.GemmProb(M, N, K, [(self.A[koff:, :M], self.B[koff:, :N])], C, self.dyn, koff=koff, nsplit=nsplit,
                                         ld=(lda, ldb, self.ldc))

    def fresh(self, dev):
        return torch.full((self.rows + self.guard, self.ldc), SENT, device=dev)


def _run(dev, fam_a, fam_b, b_first):
    """-> (C buffers of the two-family launch, C buffers of the two single-family launches), families concatenated"""
    ops, L = pkg('ops'), pkg('_lib')
    both = fam_a + fam_b
    want = [q.fresh(dev) for q in both]
    for fam, Cs in ((fam_a, want[:len(fam_a)]), (fam_b, want[len(fam_a):])):
        ops.gemm16('tn', [q.mk(C) for q, C in zip(fam, Cs)], 8, 8, 8)       # (group leading dimensions: overridden per problem)
    got = [q.fresh(dev) for q in both]
    ga = ops.gemm16_desc([q.mk(C) for q, C in zip(fam_a, got)], 8, 8, 8)
    gb = ops.gemm16_desc([q.mk(C) for q, C in zip(fam_b, got[len(fam_a):])], 8, 8, 8)
    L.lib.srec_gemm16_tn2(ctypes.addressof(ga), ctypes.addressof(gb), int(b_first), L.stream())
    torch.cuda.synchronize()
    return got, want


def _check(probs, got, want, what):
    for i, (q, g, w) in enumerate(zip(probs, got, want)):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (what, i, 'differs from the launch of its own')
        assert bool((g[q.rows:] == SENT).all()), (what, i, 'guard rows written')
        assert not bool((g[:q.rows, :8] == SENT).any()), (what, i, 'output not written')


def test_variants_cover_what_they_should():
    """no GPU: the tile counts the family cases below rely on"""
    assert len(VARIANTS) == 300
    assert {_tiles(v) for v in VARIANTS} == {1, 2, 3, 6, 18}
    for nA, nB in FAMILIES:
        a, b = _family_variants(nA, nB)
        ta, tb = sum(map(_tiles, a)), sum(map(_tiles, b))
        assert len(a) == nA and len(b) == nB
        if (nA, nB) == (1, 1):
            assert ta < 8 and tb < 8                                       # a family with fewer than 8 tiles
        else:
            assert ta % 8 or tb % 8                                        # a family that does not fill its last run
            assert max(ta, tb) > 8                                         # ... and more than one tile per XCD


def _family_variants(nA, nB):
    """a fixed pick of nA + nB variants: every 19th of the 300, so shapes, K, dyn, nsplit and koff all move inside one launch"""
    pick = [VARIANTS[(7 + 19 * i * (nA + 2 * nB)) % 300] for i in range(nA + nB)]
    return pick[:nA], pick[nA:]


@pytest.mark.gpu
@pytest.mark.parametrize('b_first', [0, 1], ids=['order_a', 'order_b'])
@pytest.mark.parametrize('nA,nB', FAMILIES)
def test_two_families_equal_two_launches(dev, nA, nB, b_first):
    gen = torch.Generator(device=dev)
    gen.manual_seed(100 * nA + nB)
    va, vb = _family_variants(nA, nB)
    fam_a = [Problem(dev, v, i, gen) for i, v in enumerate(va)]
    fam_b = [Problem(dev, v, nA + i, gen) for i, v in enumerate(vb)]
    got, want = _run(dev, fam_a, fam_b, b_first)
    _check(fam_a + fam_b, got, want, (nA, nB, b_first))


@pytest.mark.gpu
def test_every_variant_in_some_family(dev):
    """all 300 (shape, K, dyn, nsplit, koff) combinations, 16 per launch, the family sizes and orders taking turns"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    for c, i0 in enumerate(range(0, len(VARIANTS), 16)):
        vs = VARIANTS[i0:i0 + 16]
        nA = min(FAMILIES[c % 4][0], len(vs) - 1)
        probs = [Problem(dev, v, i0 + i, gen) for i, v in enumerate(vs)]
        got, want = _run(dev, probs[:nA], probs[nA:], c % 2)
        _check(probs, got, want, ('chunk', c))


def test_more_than_one_problem_table_is_refused():
    """no GPU: the argument checks run ahead of any launch and follow no pointer"""
    ops, L = pkg('ops'), pkg('_lib')
    fn = L.lib.load().srec_gemm16_tn2

    def desc(n):
        g = ops.GemmGroup16()
        g.np, g.lda, g.ldb, g.ldc = n, 8, 8, 8
        for p in range(n):
            g.M[p], g.N[p], g.K[p], g.nseg[p], g.C[p] = 8, 8, 64, 1, 0x4000
            g.A[p][0], g.B[p][0] = 0x1000, 0x2000
        return g
    for nA, nB in ((9, 8), (16, 1), (1, 16)):
        ga, gb = desc(nA), desc(nB)
        assert fn(ctypes.addressof(ga), ctypes.addressof(gb), 0, None) == L.CONST['SREC_BAD_ARG'], (nA, nB)
    ga, gb = desc(4), desc(4)
    assert fn(ctypes.addressof(ga), None, 0, None) == L.CONST['SREC_BAD_ARG']          # no second family
    gb.beta = 1.0
    assert fn(ctypes.addressof(ga), ctypes.addressof(gb), 0, None) == L.CONST['SREC_BAD_ARG']   # one beta per launch
