"""The operands of the served score as ONE record and ONE host struct: score._served_args on CPU tensors (pure torch: every
form of the operands is checked without a GPU or a library call), the layout of srec_served, and what every entry point that
takes it refuses ahead of any launch (fake pointers, never followed)."""
import ctypes

import pytest
import torch

import served_abi
from util import pkg

B, D, V = 3, 8, 10


def _args(srs=None, table=None, cs=None, off_ex=None, off_in=None, listed=None, drop_listed=False, id_lo=0, bias=None, group=None,
          who='score_select'):
    srs = torch.zeros(B, D) if srs is None else srs
    table = torch.zeros(V, D) if table is None else table
    return pkg('score')._served_args(who, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias, group)


def test_the_record_has_the_members_of_the_struct_in_its_order():
    score, L = pkg('score'), pkg('_lib')
    tensors = {'sr': 'srs', 'comp_stride': 'comp', 'E': 'table'}            # E and ld_e: the table and its row stride
    assert [tensors.get(n, n) for n, _ in served_abi.MEMBERS if n != 'ld_e'] == list(score.ServedArgs._fields)
    assert L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS and ctypes.sizeof(L.STRUCTS['srec_served']) == 136
    a = _args()
    assert (a.B, a.V, a.d, a.C, a.L, a.G, a.id_lo) == (B, V, D, 1, 0, 1, 0)
    assert a.listed_mode == L.CONST['SREC_LISTED_SCORE'] and a.bias is None and a.group is None and a.listed is None
    assert a.off_ex is None and a.off_in is None and a.cs is None


def test_drop_listed_sets_the_mode_and_ignores_off_in():
    L = pkg('_lib')
    off = torch.arange(B, dtype=torch.float32)
    listed = torch.tensor([[1, -1], [2, 3], [-1, -1]])
    a = _args(off_ex=off, off_in=off + 1, listed=listed, drop_listed=True)
    assert a.listed_mode == L.CONST['SREC_LISTED_DROP'] and a.off_in is None
    assert a.off_ex.tolist() == [off.tolist()] and a.L == 2 and a.listed.dtype == torch.int32 and a.listed.tolist() == listed.tolist()
    a = _args(off_ex=off, off_in=off + 1, listed=listed, drop_listed=False)
    assert a.listed_mode == L.CONST['SREC_LISTED_SCORE'] and a.off_in.tolist() == [(off + 1).tolist()]


def test_bias_forms_rows_groups_and_column_slices():
    b1 = torch.arange(V, dtype=torch.float32)
    a = _args(bias=b1[None])                                                # [1, V]: no group needed
    assert a.bias.data_ptr() == b1.data_ptr() and a.G == 1 and a.group is None
    grp = torch.tensor([2, 0, 1])
    b3 = torch.arange(3 * V, dtype=torch.float32).reshape(3, V)
    a = _args(bias=b3, group=grp)
    assert a.bias.data_ptr() == b3.data_ptr() and (a.G, a.ld_bias) == (3, V)
    assert a.group.dtype == torch.int32 and a.group.tolist() == [2, 0, 1]
    wide = torch.arange(2 * 2 * V, dtype=torch.float32).reshape(2, 2 * V)
    sl = wide[:, 3:3 + V]                                                   # a column slice: its row stride is kept, no copy
    a = _args(bias=sl, group=torch.tensor([1, 0, 1]))
    assert a.bias.data_ptr() == sl.data_ptr() and (a.G, a.ld_bias) == (2, 2 * V)
    with pytest.raises(ValueError, match='^score_norm: a bias of 3 rows needs group'):
        _args(bias=b3, who='score_norm')


def test_session_vectors_lists_and_id_lo():
    wide = torch.arange(B * 2 * D, dtype=torch.float32).reshape(B, 2 * D)
    view = wide[:, D:]                                                      # a row-strided view is taken as it is
    a = _args(srs=view, id_lo=1000)
    assert a.srs.data_ptr() == view.data_ptr() and (a.ld_sr, a.comp, a.C, a.id_lo) == (2 * D, 0, 1, 1000)
    parts = [torch.full((B, D), float(c)) for c in range(3)]
    a = _args(srs=parts)                                                    # a list of C tensors: one [C, B, d] block
    assert (a.C, a.ld_sr, a.comp) == (3, D, B * D) and torch.equal(a.srs, torch.stack(parts))
    a = _args(listed=torch.zeros(B, 0, dtype=torch.int64))                  # an empty list is no list
    assert a.listed is None and a.L == 0
    with pytest.raises(ValueError, match=r'^score_cutoff: 65 listed items per session; csrc/score_cutoff\.hip'):
        _args(listed=torch.zeros(B, 65, dtype=torch.int64), who='cutoff_passes')      # (the generator speaks as score_cutoff)
    with pytest.raises(RuntimeError, match='need GPU'):                     # the struct is filled through ptr(): no fallback
        _args().struct()


# ------------------------------------------------------------------------------------------- C ABI
GOOD = dict(sr=0x1000, ld_sr=32, comp_stride=0, E=0x2000, ld_e=32, cs=None, off_ex=None, off_in=None, listed=None, L=0,
            listed_mode=0, id_lo=0, B=2, V=10, d=32, C=1, stream=None)
ENTRIES = {      # name: what follows the descriptor, with values that are fine
    'srec_score_rank': dict(labels=0x3000, target=0x4000, target_given=0, rank=0x5000, ws=0x8000),
    'srec_score_select': dict(K=5, floor=None, out_val=0x4000, out_idx=0x5000, ws=0x8000),
    'srec_score_sample': dict(K=5, inv_temperature=1.0, seed=7, session_keys=None, floor=None, out_key=0x4000, out_idx=0x5000,
                              ws=0x8000),
    'srec_score_items': dict(items=0x3000, ld_items=7, M=7, out=0x4000),
    'srec_score_norm': dict(out=0x4000, ws=0x8000),
    'srec_score_cutoff_hist': dict(inv_temperature=1.0, top_k=5, top_p=0.9, **{'pass': 0}, top=0x4000, state=0x9000, hist=0xa000),
    'srec_score_cutoff_tail': dict(inv_temperature=1.0, top=0x4000, floor=0x5000, hist=0xa000),
    'srec_score_cutoff': dict(inv_temperature=1.0, top_k=5, top_p=0.9, min_gap=1.0, floor=0x5000, count=0x6000, log_kept=0x7000,
                              top=0x4000, ws=0x8000),
}


def _call(name, args, **kw):
    L = pkg('_lib')
    rest = [n for _, n in L.lib.protos[name][1:]]
    assert L.lib.protos[name][0] == ('const void*', 'served') and set(rest) == set(ENTRIES[name]) | {'stream'}, name
    return served_abi.call(getattr(L.lib.load(), name), rest, args, **kw)


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_every_entry_point_refuses_a_null_descriptor_and_a_bad_one(name):
    good = {**GOOD, **ENTRIES[name]}
    assert _call(name, good, null=True) == 1001
    nothing = {n: (0.0 if isinstance(v, float) else None if v is None or v >= 0x1000 else 0) for n, v in good.items()}
    assert _call(name, nothing, null=True) == 1001                          # also with nothing else valid
    for change in (dict(d=30), dict(C=5), dict(L=65), dict(sr=0x1004), dict(E=0x2008), dict(ld_e=30), dict(id_lo=-1),
                   dict(listed_mode=2), dict(G=0), dict(G=2), dict(group=0x7001), dict(bias=0x6002)):
        assert _call(name, {**good, **change}) == 1001, change
    assert _call(name, {**good, 'B': 0, 'd': 30, 'G': 0}) == 0               # no sessions: nothing to do, ahead of the checks
    if name != 'srec_score_rank':                                            # (the rank never forms a global id as an int)
        assert _call(name, {**good, 'id_lo': 2 ** 31 - 5}) == 1001


def test_the_binding_refuses_another_number_of_arguments_ahead_of_the_call():
    """a caller of the positional prototypes would hand its first pointer to `const void* served`, which is followed: the
    binding takes exactly the declared arguments, so such a call never reaches the library"""
    dll = pkg('_lib').lib.load()
    old_items = [0x1000, 32, 0, 0x2000, 32, None, None, None, None, 0, 0, 0x3000, 7, 7, 0, 2, 10, 32, 1, 0x4000, None]
    with pytest.raises(TypeError, match='takes exactly 6 arguments'):
        dll.srec_score_items(*old_items)
    with pytest.raises(TypeError, match='takes exactly 4 arguments'):
        dll.srec_score_norm(0x1000, 32, 0, 0x2000, 32)
    with pytest.raises(TypeError):
        dll.srec_score_norm(None, None, None)                                # one short
    assert dll.srec_score_norm(None, None, None, None) == 1001 and isinstance(dll.srec_score_norm.argtypes, list)


def test_rank_prototype_and_its_refusal_of_a_bias_and_of_listed_drop():
    L = pkg('_lib')
    assert L.lib.protos['srec_score_rank'] == [('const void*', 'served'), ('const int*', 'labels'), ('float*', 'target'),
                                               ('int', 'target_given'), ('int*', 'rank'), ('void*', 'ws'), ('void*', 'stream')]
    good = {**GOOD, **ENTRIES['srec_score_rank']}
    for change in (dict(bias=0x6000), dict(bias=0x6000, ld_bias=10, group=0x7000, G=3), dict(listed_mode=L.CONST['SREC_LISTED_DROP']),
                   dict(labels=None), dict(target=None), dict(rank=None, target_given=1)):
        assert _call('srec_score_rank', {**good, **change}) == 1001, change
