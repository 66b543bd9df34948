"""Host side of the normalisation folds around the MSHGNN layer (no GPU): the predicate's decisions, the switch parsing, and the one
property of the collated batch the exit folds rely on - cat_inv is the inverse of cat_perm on the live rows."""
import numpy as np
import pytest

from util import load_golden, pkg

A, B, C, D = 1, 2, 4, 8


def _bits(mask=15, H=8, Dm=256, per_type=(5, 4, 5), entry=True, exit_=True, pf=0.1, pa=0.1, tap=False):
    return pkg('hgat').norm_fold_bits(mask, H, Dm, list(per_type), entry, exit_, pf, pa, tap)


def test_predicate_decisions():
    hg = pkg('hgat')
    assert (hg.FOLD_A, hg.FOLD_B, hg.FOLD_C, hg.FOLD_D) == (A, B, C, D)
    built = hg.FOLDS_BUILT
    assert _bits() == 15 & built
    for m in range(16):                                             # the mask only ever takes folds away
        assert _bits(mask=m) == m & built
    assert _bits(entry=False) == (B | C) & built and _bits(exit_=False) == (A | D) & built
    assert _bits(pf=0.0, pa=0.0) == (B | C) & built                 # no dropout launch: the entry folds have no host
    assert _bits(pf=0.0, pa=0.1) & A == A & built                   # (attention dropout alone still launches the dropout pass)
    assert _bits(tap=True) & D == 0 and _bits(tap=True) & A == A & built     # stored masks: d x is not written in one pass
    assert _bits(H=4) == 0 and _bits(Dm=260) == 0 and _bits(Dm=512) == 0 and _bits(Dm=252) == 0      # not the node kernels
    assert _bits(per_type=(9, 1, 1)) == 0 and _bits(per_type=()) == 0 and _bits(per_type=(0, 0)) == 0
    assert _bits(Dm=64) == 15 & built and _bits(per_type=(8, 8)) == 15 & built


def test_switch_parsing():
    parse = pkg('ops').parse_norm_fold
    assert parse(None) == 15 and parse('') == 15 and parse(' ') == 15
    assert [parse(str(m)) for m in (0, 1, 2, 4, 8, 15)] == [0, 1, 2, 4, 8, 15]
    assert parse('0xf') == 15 and parse('0b101') == 5
    for bad in ('16', '-1', 'on'):
        with pytest.raises(ValueError):
            parse(bad)


@pytest.mark.parametrize('native', [False, True], ids=['python', 'native'])
@pytest.mark.parametrize('K', [2, 3])
@pytest.mark.parametrize('padded', [False, True], ids=['exact', 'padded'])
def test_cat_inv_inverts_cat_perm_on_the_live_rows(K, native, padded, monkeypatch):
    """both collate builders, the sample split and a hand batch with a one-click session: every live stacked row r has
    cat_perm[cat_inv[r]] == r with cat_inv[r] below the live concatenated count, every other stacked row has cat_inv = -1"""
    c = pkg('collate')
    if native:
        assert c._native() is not None, 'the native collate (csrc/collate.cpp) is not built'

    else:
        monkeypatch.setattr(c, '_NATIVE', False)
    samples = [([5], 3), ([1, 2, 1, 2, 3], 4)] + list(load_golden('msgifsr_K3_edge')[1])
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'datasets', 'sample', 'train.txt')
    with open(root) as f:
        for line in list(f)[:40]:
            seq = [int(t) for t in line.replace(',', ' ').split()]
            if len(seq) >= 2:
                samples.append((seq[:-1][-19:], seq[-1]))
    caps = c.default_caps(len(samples) + 3, 20) if padded else None
    (mg,), _ = c.collate_fn_factory_ccs((c.seq_to_ccs_graph,), K, caps=caps)(samples)
    perm, inv = mg.field('cat_perm').numpy().astype(np.int64), mg.field('cat_inv').numpy().astype(np.int64)
    ncap, NT = mg.meta['ncap'], mg.count('NT')
    assert inv.shape[0] == sum(ncap[k] for k in range(1, K + 1))
    r0, live = 0, []
    for k in range(1, K + 1):
        live += list(range(r0, r0 + mg.count('N%d' % k)))
        r0 += ncap[k]
    live = np.asarray(live)
    assert len(live) == NT and mg.count('N%d' % K) < mg.count('N1')
    assert (inv[live] >= 0).all() and (inv[live] < NT).all()
    assert (perm[inv[live]] == live).all()
    assert sorted(inv[live].tolist()) == list(range(NT))
    dead = np.setdiff1d(np.arange(inv.shape[0]), live)
    assert (inv[dead] == -1).all()
