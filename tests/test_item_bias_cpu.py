"""CPU half of the per-item bias of the serving calls: the bias normaliser of ops.score_select / ops.score_items
(score._bias_args), ops.catalog_bias, the launchers' catalogue readers and parser errors, the C ABI of the bias in the two serving
entry points (the members of the srec_served descriptor both take, exported, bad arguments refused without a launch) and the float64 oracle (tests/item_bias_oracle.py) against a brute-force loop."""
import os
import sys

import pytest
import torch

import served_abi
from item_bias_oracle import NINF, bias_rows, exact_bias, items_biased64, select_biased64
from select_oracle import drop_mask
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')


# ------------------------------------------------------------------------------------------- _bias_args
def test_bias_args_accepts_rows_groups_and_column_slices_as_they_are():
    score = pkg('score')
    B, V = 4, 10
    assert score._bias_args('score_select', None, None, B, V) == score.BiasArgs(None, 0, None, 1)
    b1 = torch.arange(V, dtype=torch.float32)
    a = score._bias_args('score_select', b1, None, B, V)
    assert a.bias.data_ptr() == b1.data_ptr() and a.group is None and a.G == 1 and a.ld_bias == V
    wide = torch.arange(3 * 2 * V, dtype=torch.float32).reshape(3, 2 * V)
    grp = torch.tensor([2, 0, 1, 1])
    sl = wide[:, V:]                                    # a column slice: unit column stride, row stride 2 V - taken as it is
    a = score._bias_args('score_items', sl, grp, B, V)
    assert a.bias.data_ptr() == sl.data_ptr() and a.ld_bias == 2 * V and a.G == 3
    assert a.group.dtype == torch.int32 and a.group.tolist() == [2, 0, 1, 1] and a.group.is_contiguous()
    # one row as [1, V]: no group needed, a given one is not passed on
    a = score._bias_args('score_select', wide[:1, :V], None, B, V)
    assert a.G == 1 and a.group is None and a.bias.data_ptr() == wide.data_ptr()
    assert score._bias_args('score_select', wide[:1, :V], torch.zeros(B, dtype=torch.int64), B, V).group is None
    # anything else is made contiguous fp32: a column stride of 2, another dtype
    a = score._bias_args('score_select', wide[:, ::2], grp, B, V)
    assert a.bias.is_contiguous() and a.ld_bias == V and torch.equal(a.bias, wide[:, ::2])
    a = score._bias_args('score_select', b1.double(), None, B, V)
    assert a.bias.dtype == torch.float32 and torch.equal(a.bias, b1)
    a = score._bias_args('score_select', b1.half(), None, B, V)
    assert a.bias.dtype == torch.float32
    # group ids of any integer dtype and shape [B, 1]
    assert score._bias_args('x', wide[:, :V], grp.to(torch.int16).reshape(B, 1), B, V).group.shape == (B,)


def test_bias_args_refusals_in_the_words_of_the_caller():
    score = pkg('score')
    B, V = 4, 10
    ok, grp = torch.zeros(3, V), torch.zeros(B, dtype=torch.int64)
    for who in ('score_select', 'score_items'):
        for bias, group, msg in ((torch.zeros(V + 1), None, 'bias has 11 columns for 10 table rows'),
                                 (torch.zeros(3, V - 1), grp, 'bias has 9 columns for 10 table rows'),
                                 (torch.zeros(2, 3, V), grp, 'got 3 dimensions'),
                                 (torch.zeros(()), None, 'got 0 dimensions'),
                                 (torch.zeros(V, dtype=torch.int64), None, 'must be a floating tensor'),
                                 (torch.zeros(V, dtype=torch.bool), None, 'must be a floating tensor'),
                                 (torch.zeros(V), grp, r'group needs a 2-D bias \[G, V\]'),
                                 (None, grp, 'group is given without a bias'),
                                 (ok, None, 'a bias of 3 rows needs group'),
                                 (ok, grp[:3], 'group must hold 4 integer row ids'),
                                 (ok, torch.zeros(B + 1, dtype=torch.int32), 'group must hold 4 integer row ids'),
                                 (ok, torch.zeros(B), 'group must hold 4 integer row ids'),
                                 (torch.zeros(0, V), grp, 'bias has no rows')):
            with pytest.raises(ValueError, match='^' + who + ': .*' + msg):
                score._bias_args(who, bias, group, B, V)
    # through the public calls, with CPU tensors: anything that reached the library would raise RuntimeError instead
    ops = pkg('ops')
    sr, E = torch.zeros(B, 8), torch.zeros(V, 8)
    with pytest.raises(ValueError, match='score_select: bias has 11 columns'):
        ops.score_select(sr, E, None, 3, bias=torch.zeros(V + 1))
    with pytest.raises(ValueError, match='score_items: a bias of 3 rows needs group'):
        ops.score_items(sr, E, None, torch.tensor([1, 2]), bias=ok)
    assert pkg('score')._mixture_args.__code__.co_argcount == 6         # the shared normaliser keeps its signature


# ------------------------------------------------------------------------------------------- catalog_bias
def test_catalog_bias_combines_allow_deny_and_boost():
    ops = pkg('ops')
    b = ops.catalog_bias(8)
    assert b.dtype == torch.float32 and b.tolist() == [0.0] * 8
    assert ops.catalog_bias(6, allow=[1, 2, 3]).tolist() == [NINF, 0, 0, 0, NINF, NINF]
    assert ops.catalog_bias(6, deny=torch.tensor([0, 5])).tolist() == [NINF, 0, 0, 0, 0, NINF]
    assert ops.catalog_bias(6, boost=([4, 1], [0.5, -2.0])).tolist() == [0, -2.0, 0, 0, 0.5, 0]
    # all three: a boost on a filtered item stays -inf; deny wins over allow; an id boosted twice adds up
    b = ops.catalog_bias(6, allow=[1, 2, 3], deny=[2], boost=(torch.tensor([1, 5, 2, 1]), torch.tensor([0.5, 1.0, 3.0, 0.25])))
    assert b.tolist() == [NINF, 0.75, NINF, 0.0, NINF, NINF]
    assert ops.catalog_bias(4, allow=[], deny=[]).tolist() == [NINF] * 4
    assert ops.catalog_bias(4, allow=torch.tensor([3, 3], dtype=torch.int32)).tolist() == [NINF, NINF, NINF, 0.0]


def test_catalog_bias_refusals():
    ops = pkg('ops')
    for kw, msg in ((dict(allow=[0, 6]), r'allow id 6; ids are in \[0, 6\)'), (dict(deny=[-1]), 'deny id -1'),
                    (dict(boost=([7], [1.0])), 'boost id 7'), (dict(boost=([1, 2], [1.0])), 'boost has 2 ids and 1 values'),
                    (dict(allow=torch.tensor([1.0])), 'allow ids must be integers')):
        with pytest.raises(ValueError, match='catalog_bias: ' + msg):
            ops.catalog_bias(6, **kw)


# ------------------------------------------------------------------------------------------- launchers
def _scripts():
    sys.path.insert(0, SCRIPTS)
    try:
        import common
        import recommend
        import rerank
    finally:
        sys.path.remove(SCRIPTS)
    return common, recommend, rerank


def test_catalogue_file_readers(tmp_path):
    common, _, _ = _scripts()
    (tmp_path / 'ids.txt').write_text('3\n\n 17 \n0\n')
    assert common.read_id_file(str(tmp_path / 'ids.txt')) == [3, 17, 0]
    (tmp_path / 'bias.txt').write_text('3:0.5\n4\t-2\n\n 9:1e-1\n')
    assert common.read_bias_file(str(tmp_path / 'bias.txt')) == ([3, 4, 9], [0.5, -2.0, 0.1])
    (tmp_path / 'bad.txt').write_text('3\nx7\n')
    with pytest.raises(ValueError, match=r'bad\.txt line 2: `x7` is no item id'):
        common.read_id_file(str(tmp_path / 'bad.txt'))
    for text, msg in (('3:0.5\n4;1\n', 'line 2: `4;1` is not `id:value`'), ('3:0.5:1\n', 'line 1'), ('a:1\n', 'line 1'),
                      ('3:inf\n', 'line 1: the value of item 3 is not finite'), ('1:0\n2\tnan\n', 'line 2: the value of item 2'),
                      ('5:-inf\n', 'not finite')):
        (tmp_path / 'b.txt').write_text(text)
        with pytest.raises(ValueError, match=msg):
            common.read_bias_file(str(tmp_path / 'b.txt'))


def test_launchers_parse_catalogue_flags_and_refuse_before_a_model_is_built(tmp_path, capsys):
    _, rec, rr = _scripts()
    data = tmp_path / 'data'
    data.mkdir()
    (data / 'num_items.txt').write_text('50\n')
    allow, deny, bias, empty = (str(tmp_path / n) for n in ('allow.txt', 'deny.txt', 'bias.txt', 'empty.txt'))
    open(allow, 'w').write('1\n2\n49\n')
    open(deny, 'w').write('2\n')
    open(bias, 'w').write('1:0.5\n7\t-1.25\n')
    open(empty, 'w').write('\n\n')
    base = {rec: ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--dataset-dir', str(data)],
            rr: ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--candidates', 'c.txt', '--dataset-dir', str(data)]}
    for mod in (rec, rr):
        assert mod.parse(base[mod]).catalog is None
        args = mod.parse(base[mod] + ['--allow', allow, '--deny', deny, '--item-bias', bias])
        assert args.catalog == dict(allow=[1, 2, 49], deny=[2], boost=([1, 7], [0.5, -1.25]))
        want = pkg('ops').catalog_bias(50, **args.catalog)
        assert want[1] == 0.5 and want[2] == NINF and want[49] == 0 and want[7] == NINF and int((want > NINF).sum()) == 2
        assert mod.parse(base[mod] + ['--deny', deny]).catalog == dict(deny=[2])
        open(str(tmp_path / 'far.txt'), 'w').write('3\n50\n')
        open(str(tmp_path / 'nan.txt'), 'w').write('3:nan\n')
        open(str(tmp_path / 'neg.txt'), 'w').write('-1:0.5\n')
        for flags, msg in ((['--allow', str(tmp_path / 'far.txt')], r'--allow: item id 50; ids are in [0, 50)'),
                           (['--deny', str(tmp_path / 'far.txt')], '--deny: item id 50'),
                           (['--item-bias', str(tmp_path / 'neg.txt')], '--item-bias: item id -1'),
                           (['--item-bias', str(tmp_path / 'nan.txt')], 'is not finite'),
                           (['--allow', empty], 'names no item'),
                           (['--allow', str(tmp_path / 'missing.txt')], 'missing.txt')):
            capsys.readouterr()
            with pytest.raises(SystemExit) as e:
                mod.parse(base[mod] + flags)
            assert e.value.code == 2 and msg in capsys.readouterr().err, (flags, msg)


# ------------------------------------------------------------------------------------------- C ABI
SELECT = [('int', 'K'), ('const float*', 'floor'), ('float*', 'out_val'), ('int*', 'out_idx'), ('void*', 'ws'), ('void*', 'stream')]
ITEMS = [('const int*', 'items'), ('long', 'ld_items'), ('int', 'M'), ('float*', 'out'), ('void*', 'stream')]


def test_header_declares_the_biased_entry_points_beside_the_unchanged_ones():
    """the bias is a member of the descriptor every serving entry point takes: one entry point each, no _biased variant"""
    L = pkg('_lib')
    protos = L.parse_header()
    assert protos['srec_score_select'] == [('const void*', 'served')] + SELECT
    assert protos['srec_score_items'] == [('const void*', 'served')] + ITEMS
    assert L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS
    assert [n for n, _ in served_abi.MEMBERS[-4:]] == ['bias', 'ld_bias', 'group', 'G']      # behind the unbiased operands
    assert not {'srec_score_select_biased', 'srec_score_items_biased'} & set(protos)
    dll = L.lib.load()                                  # binds every declared symbol: a missing export raises here
    assert len(dll.srec_score_select.argtypes) == 1 + len(SELECT)
    assert len(dll.srec_score_items.argtypes) == 1 + len(ITEMS)


def test_biased_c_entries_refuse_bad_arguments_without_a_launch():
    """every refusal happens ahead of the launch, so it can be provoked on a machine without a GPU with pointers that are
    never followed"""
    dll = pkg('_lib').lib.load()
    common = dict(sr=0x1000, ld_sr=32, comp_stride=0, E=0x2000, ld_e=32, cs=None, off_ex=None, off_in=None, listed=None, L=0,
                  listed_mode=0, id_lo=0, B=2, V=10, d=32, C=1, bias=0x6000, ld_bias=10, group=0x7000, G=3, stream=None)
    sel = dict(common, K=5, floor=None, out_val=0x4000, out_idx=0x5000, ws=0x8000)
    itm = dict(common, items=0x3000, ld_items=7, M=7, out=0x4000)
    bad = [dict(G=0), dict(G=-1), dict(group=None), dict(ld_bias=9), dict(bias=0x6002), dict(group=0x7001),
           dict(bias=None, group=None, G=2), dict(bias=None, G=0), dict(d=30), dict(C=5)]
    # select: without a floor and with an aligned one (the two entry points this one replaced)
    for fn, good, rest in ((dll.srec_score_select, sel, [n for _, n in SELECT]),
                           (dll.srec_score_select, dict(sel, floor=0xa000), [n for _, n in SELECT]),
                           (dll.srec_score_items, itm, [n for _, n in ITEMS])):
        for change in bad:
            assert served_abi.call(fn, rest, {**good, **change}) == 1001, (fn, change)
        assert served_abi.call(fn, rest, {**good, 'B': 0, 'G': 0}) == 0         # no sessions: nothing to do
        assert served_abi.call(fn, rest, good, null=True) == 1001              # no descriptor
    assert served_abi.call(dll.srec_score_select, [n for _, n in SELECT], {**sel, 'K': 129}) == 1001
    assert served_abi.call(dll.srec_score_select, [n for _, n in SELECT], {**sel, 'floor': 0xa002}) == 1001   # floor misaligned


# ------------------------------------------------------------------------------------------- oracle against a loop
def test_oracle_against_a_brute_force_loop_on_3_by_20():
    g = torch.Generator().manual_seed(5)
    B, V, K = 3, 20, 8
    s = (torch.randint(-8, 9, (B, V), generator=g).double() / 4)          # many ties
    bias = exact_bias(V, 2, off_share=0.3, off_ranges=())
    bias[1, 5:] = NINF                                                    # group 1: five eligible items, fewer than K
    group = torch.tensor([0, 1, 0])
    listed = torch.tensor([[0, 3], [1, -1], [19, 2]])
    items = torch.tensor([[0, 19, -1, 4, 4, 25], [1, 2, 3, -1, 0, 7], [19, 2, 5, 5, -1, 30]])
    rows = bias_rows(bias, group, B)
    assert rows.shape == (B, V) and torch.equal(rows[1], bias[1].double()) and torch.equal(rows[2], bias[0].double())
    for drop in (None, drop_mask(listed, V)):
        val, idx = select_biased64(s, K, bias, group, drop)
        got = items_biased64(s, items, bias, group, 0, drop)
        for b in range(B):
            bb = bias[group[b]].double()
            elig = [v for v in range(V) if bb[v] != NINF and not (drop is not None and bool(drop[b, v]))]
            best = sorted(elig, key=lambda v: (-float(s[b, v] + bb[v]), v))[:K]
            want_i = best + [-1] * (K - len(best))
            want_v = [float(s[b, v] + bb[v]) for v in best] + [NINF] * (K - len(best))
            assert idx[b].tolist() == want_i and val[b].tolist() == want_v, (b, drop is not None)
            for m, i in enumerate(items[b].tolist()):
                if i < 0:
                    w = NINF
                elif i >= V:
                    w = 0.0
                elif i not in elig:
                    w = NINF
                else:
                    w = float(s[b, i] + bb[i])
                assert float(got[b, m]) == w, (b, m, i)
        assert idx[1].tolist()[5:] == [-1] * (K - 5) or drop is not None
    # shards: columns [0, 8) and [8, 20) with id_lo; a foreign id gives 0 whatever its bias
    lo = items_biased64(s[:, :8], items, bias, group, 0)
    hi = items_biased64(s[:, 8:], items, bias, group, 8)
    whole = items_biased64(s, items, bias, group)
    inside = (items >= 0) & (items < V)
    assert torch.equal((lo + hi)[inside | (items < 0)], whole[inside | (items < 0)])
    assert bool((lo[items >= 8] == 0).all()) and bool((hi[(items >= 0) & (items < 8)] == 0).all())
    # one shared row
    v1, i1 = select_biased64(s, K, bias[0])
    v2, i2 = select_biased64(s, K, bias[:1], torch.zeros(B, dtype=torch.long))
    assert torch.equal(v1, v2) and torch.equal(i1, i2)
