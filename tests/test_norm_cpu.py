"""CPU half of the renormalisation of the served scores: the float64 oracle (tests/norm_oracle.py) against a brute-force
loop and its -inf rules, the argument checks of ops.score_norm on CPU tensors (pure torch ahead of any launch), the C ABI of
srec_score_norm / srec_score_norm_ws (declared with the descriptor of srec_score_select, exported, bad arguments refused
without a launch), dist.lse_fold, and --renormalize of the two launchers."""
import math
import os
import sys

import pytest
import torch

import served_abi
from item_bias_oracle import NINF, exact_bias
from norm_oracle import eligible, lse_pair64, norm64
from select_oracle import drop_mask
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')


# ------------------------------------------------------------------------------------------- oracle against a loop
def test_oracle_against_a_brute_force_loop_on_3_by_20():
    g = torch.Generator().manual_seed(5)
    B, V = 3, 20
    s = torch.randint(-8, 9, (B, V), generator=g).double() / 4
    bias = exact_bias(V, 2, off_share=0.3, off_ranges=())
    bias[1, 5:] = NINF
    group = torch.tensor([0, 1, 0])
    listed = torch.tensor([[0, 3], [1, -1], [19, 2]])
    for b_, g_ in ((None, None), (bias[0], None), (bias, group)):
        for drop in (None, drop_mask(listed, V)):
            got = norm64(s, b_, g_, drop)
            assert got.dtype == torch.float64 and got.shape == (B,)
            for b in range(B):
                tot = 0.0
                for v in range(V):
                    bb = 0.0 if b_ is None else float(b_[v] if b_.dim() == 1 else b_[g_[b], v])
                    if bb == NINF or (drop is not None and bool(drop[b, v])):
                        continue
                    tot += math.exp(float(s[b, v]) + bb)
                assert abs(float(got[b]) - math.log(tot)) < 1e-12, (b, b_ is None, drop is None)
    # two row ranges with id_lo and the GLOBAL bias combine by log-sum-exp to the whole
    dm = drop_mask(listed, V)
    lo = norm64(s[:, :8], bias, group, dm[:, :8], 0)
    hi = norm64(s[:, 8:], bias, group, dm[:, 8:], 8)
    assert float((lse_pair64(lo, hi) - norm64(s, bias, group, dm)).abs().max()) < 1e-12
    assert int(eligible(B, V, bias, group, dm).sum()) < int(eligible(B, V, bias, group).sum()) < B * V


def test_oracle_minus_infinity_rules():
    B, V = 3, 6
    s = torch.zeros(B, V, dtype=torch.float64)
    none = torch.full((V,), NINF)
    z = norm64(s, none)
    assert z.tolist() == [NINF] * B and not bool(torch.isnan(z).any())
    bias3 = torch.stack([torch.zeros(V), none, torch.zeros(V)])
    z = norm64(s, bias3, torch.tensor([0, 1, 2]))
    assert z[1] == NINF and abs(float(z[0]) - math.log(V)) < 1e-12 and z[0] == z[2]
    z = norm64(s, None, None, torch.ones(B, V, dtype=torch.bool))           # everything dropped
    assert z.tolist() == [NINF] * B
    s2 = s.clone()
    s2[0] = NINF                                                            # eligible items that all score -inf
    z = norm64(s2)
    assert z[0] == NINF and not bool(torch.isnan(z).any()) and abs(float(z[1]) - math.log(V)) < 1e-12
    # one item far ahead: Z is its score
    s3 = torch.full((1, V), -800.0, dtype=torch.float64)
    s3[0, 4] = 0.25
    assert norm64(s3).tolist() == [0.25]
    assert lse_pair64(torch.tensor([NINF, 0.0]), torch.tensor([NINF, NINF])).tolist() == [NINF, 0.0]


def test_lse_fold_is_safe_against_empty_rows_and_columns():
    D = pkg('dist')
    z = torch.tensor([[NINF, 0.5, NINF, 1.0], [NINF, NINF, -2.0, 1.0]])
    out = D.lse_fold(z)
    assert out.dtype == torch.float32 and not bool(torch.isnan(out).any())
    assert out[0] == NINF and out[1] == 0.5 and out[2] == -2.0 and abs(float(out[3]) - (1.0 + math.log(2.0))) < 1e-6
    assert torch.equal(D.lse_fold(z[:1]), z[0])


# ------------------------------------------------------------------------------------------- ops.score_norm argument checks
def test_score_norm_refuses_bad_arguments_on_cpu_tensors():
    """anything that reached the library would raise RuntimeError (CPU tensors) instead"""
    ops, score = pkg('ops'), pkg('score')
    assert ops.score_norm is score.score_norm
    B, V = 4, 10
    sr, E = torch.zeros(B, 8), torch.zeros(V, 8)
    grp = torch.zeros(B, dtype=torch.int64)
    for kw, msg in ((dict(bias=torch.zeros(V + 1)), 'bias has 11 columns for 10 table rows'),
                    (dict(bias=torch.zeros(3, V)), 'a bias of 3 rows needs group'),
                    (dict(bias=torch.zeros(V), group=grp), r'group needs a 2-D bias \[G, V\]'),
                    (dict(group=grp), 'group is given without a bias'),
                    (dict(bias=torch.zeros(V, dtype=torch.int64)), 'must be a floating tensor'),
                    (dict(bias=torch.zeros(3, V), group=grp[:3]), 'group must hold 4 integer row ids'),
                    (dict(listed=torch.zeros(B, 65, dtype=torch.int64)), r'65 listed items per session; csrc/score_norm\.hip takes at most 64')):
        with pytest.raises(ValueError, match='^score_norm: .*' + msg):
            ops.score_norm(sr, E, None, **kw)
    out = ops.score_norm(torch.zeros(0, 8), E, None, bias=torch.zeros(V))   # no sessions: nothing is launched
    assert out.shape == (0,) and out.dtype == torch.float32
    with pytest.raises(RuntimeError, match='need GPU'):                    # good arguments reach the library: no fallback
        ops.score_norm(sr, E, None, bias=torch.zeros(V))


# ------------------------------------------------------------------------------------------- C ABI
TAIL = [('float*', 'out'), ('void*', 'ws'), ('void*', 'stream')]


def test_header_declares_both_entry_points():
    L = pkg('_lib')
    protos = L.parse_header()
    # the descriptor srec_score_select takes, then out where that call has K, floor, val and idx
    assert protos['srec_score_norm'] == protos['srec_score_select'][:1] + TAIL == [('const void*', 'served')] + TAIL
    assert L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS
    assert protos['srec_score_norm_ws'] == [('int', 'B'), ('int', 'V'), ('int', 'd'), ('int', 'C'), ('int', 'L'), ('long*', 'bytes')]
    dll = L.lib.load()                                  # binds every declared symbol: a missing export raises here
    assert len(dll.srec_score_norm.argtypes) == 4


def test_c_entries_refuse_bad_arguments_without_a_launch():
    import ctypes
    dll = pkg('_lib').lib.load()
    good = dict(sr=0x1000, ld_sr=32, comp_stride=0, E=0x2000, ld_e=32, cs=None, off_ex=None, off_in=None, listed=None, L=0,
                listed_mode=0, id_lo=0, B=2, V=10, d=32, C=1, bias=0x6000, ld_bias=10, group=0x7000, G=3, out=0x4000, ws=0x8000,
                stream=None)
    rest = [n for _, n in TAIL]
    for change in (dict(G=0), dict(group=None), dict(ld_bias=9), dict(bias=0x6002), dict(group=0x7001), dict(d=30), dict(d=1028),
                   dict(C=5), dict(C=0), dict(L=65), dict(listed_mode=2), dict(out=None), dict(ws=None), dict(id_lo=-1),
                   dict(id_lo=2 ** 31 - 5), dict(E=0x2004), dict(ld_e=30), dict(bias=None, group=None, G=2)):
        assert served_abi.call(dll.srec_score_norm, rest, {**good, **change}) == 1001, change
    assert served_abi.call(dll.srec_score_norm, rest, {**good, 'B': 0, 'G': 0}) == 0        # no sessions: nothing to do
    assert served_abi.call(dll.srec_score_norm, rest, good, null=True) == 1001              # no descriptor
    n = ctypes.c_long(-1)
    assert dll.srec_score_norm_ws(512, 37484, 256, 3, 20, ctypes.addressof(n)) == 0 and n.value > 0 and n.value % 8 == 0
    small = ctypes.c_long(-1)
    assert dll.srec_score_norm_ws(5, 1, 32, 1, 0, ctypes.addressof(small)) == 0 and small.value == 5 * 8   # one range
    for B, V, d, C, Lm in ((0, 10, 32, 1, 0), (2, 0, 32, 1, 0), (2, 10, 30, 1, 0), (2, 10, 32, 5, 0), (2, 10, 32, 1, 65)):
        assert dll.srec_score_norm_ws(B, V, d, C, Lm, ctypes.addressof(n)) == 1001
    assert dll.srec_score_norm_ws(2, 10, 32, 1, 0, None) == 1001


# ------------------------------------------------------------------------------------------- launchers
def test_both_launchers_accept_renormalize(tmp_path):
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
        import rerank as rr
    finally:
        sys.path.remove(SCRIPTS)
    data = tmp_path / 'data'
    data.mkdir()
    (data / 'num_items.txt').write_text('50\n')
    deny = str(tmp_path / 'deny.txt')
    open(deny, 'w').write('2\n')
    base = {rec: ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--dataset-dir', str(data)],
            rr: ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--candidates', 'c.txt', '--dataset-dir', str(data)]}
    for mod in (rec, rr):
        assert mod.parse(base[mod]).renormalize is False
        args = mod.parse(base[mod] + ['--renormalize', '--deny', deny, '--exclude-seen'])
        assert args.renormalize is True and args.catalog == dict(deny=[2]) and args.exclude_seen
        assert '--renormalize' in mod.parser('SRGNN').format_help()


def test_models_take_the_keyword_and_log_mass_checks_the_bias_first():
    import inspect
    mixin = pkg('srgnn')._ScoringMixin
    for fn in ('recommend', 'score_items', 'rerank'):
        p = inspect.signature(getattr(mixin, fn)).parameters['renormalize']
        assert p.default is False and p.kind is p.KEYWORD_ONLY, fn
        assert 'NO renormalisation' not in getattr(mixin, fn).__doc__, fn
    assert 'CATALOGUE' in mixin.score_items.__doc__ and 'CATALOGUE' in mixin.rerank.__doc__
    model = pkg().SRGNN(50, 32, 1).train()
    with pytest.raises(ValueError, match=r'log_mass: item_bias must be a floating tensor \[50\]'):
        model.log_mass(None, item_bias=torch.zeros(51))
    with pytest.raises(ValueError, match='log_mass: item_group is given without an item_bias'):
        model.log_mass(None, item_group=torch.zeros(2, dtype=torch.int64))
    assert model.training
