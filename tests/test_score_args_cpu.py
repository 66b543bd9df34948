"""The argument conventions score_rank and score_select share (score._mixture_args) on CPU tensors: it is pure torch, so
every form of `srs`, the offsets, the listed items and the refusals are checked without a GPU or a library call."""
import pytest
import torch

from util import pkg

B, D, V = 3, 8, 10


def _args(srs, off_ex=None, off_in=None, listed=None, who='score_rank'):
    return pkg('score')._mixture_args(who, srs, torch.zeros(V, D), off_ex, off_in, listed)


def test_every_form_of_srs():
    g = torch.Generator().manual_seed(0)
    one, three = torch.randn(B, D, generator=g), torch.randn(3, B, D, generator=g)
    for srs, C, comp, want in [(one, 1, 0, one), (one[None], 1, 0, one), (three, 3, B * D, three),
                               ([three[0], three[1], three[2]], 3, B * D, three), ([one], 1, 0, one)]:
        a = _args(srs)
        assert (a.C, a.B, a.d, a.ld_sr, a.comp) == (C, B, D, D, comp)
        assert a.srs.dtype == torch.float32 and torch.equal(a.srs, want)
        assert (a.V, tuple(a.table.shape)) == (V, (V, D))
        assert (a.off_ex, a.off_in, a.listed, a.L) == (None, None, None, 0)
    assert _args(one).srs.data_ptr() == one.data_ptr() and _args(three).srs.data_ptr() == three.data_ptr()


def test_a_row_strided_view_is_taken_as_it_is():
    big = torch.randn(B, 12, generator=torch.Generator().manual_seed(1))
    a = _args(big[:, :D])
    assert (a.C, a.B, a.d, a.ld_sr, a.comp) == (1, B, D, 12, 0)
    assert a.srs.data_ptr() == big.data_ptr() and a.srs.stride() == (12, 1)          # no copy


def test_offsets_and_listed_items():
    srs = torch.zeros(3, B, D)
    off = torch.arange(3 * B, dtype=torch.float64).reshape(3, B) / 4
    a = _args(srs, off_ex=off, off_in=None)
    assert a.off_in is None
    assert a.off_ex.dtype == torch.float32 and a.off_ex.shape == (3, B) and a.off_ex.is_contiguous()
    assert torch.equal(a.off_ex.double(), off)
    a = _args(srs, off_ex=None, off_in=off.t().contiguous().t())                     # a [C, B] view with strides (1, C)
    assert a.off_ex is None and a.off_in.is_contiguous() and torch.equal(a.off_in.double(), off)
    for listed in (None, torch.zeros(B, 0, dtype=torch.int64)):
        a = _args(srs, listed=listed)
        assert (a.listed, a.L) == (None, 0)
    listed = torch.arange(B * 5).reshape(B, 5) - 1
    a = _args(srs, listed=listed)
    assert a.L == 5 and a.listed.dtype == torch.int32 and a.listed.shape == (B, 5) and a.listed.is_contiguous()
    assert torch.equal(a.listed.long(), listed)
    assert _args(srs, listed=torch.zeros(B, 64, dtype=torch.int64)).L == 64


def test_both_public_functions_refuse_65_listed_items_in_their_own_words():
    ops = pkg('ops')
    sr, E = torch.zeros(B, D), torch.zeros(V, D)         # CPU tensors: anything that reached the library would raise RuntimeError
    listed = torch.zeros(B, 65, dtype=torch.int32)
    with pytest.raises(ValueError) as e:
        ops.score_rank(sr, E, None, torch.zeros(B, dtype=torch.int64), listed=listed)
    assert str(e.value) == ('score_rank: 65 listed items per session; the fix-up pass of csrc/rank.hip takes at most 64 '
                            '(evaluate such sessions with method="topk")')
    for drop in (False, True):
        with pytest.raises(ValueError) as e:
            ops.score_select(sr, E, None, 5, listed=listed, drop_listed=drop)
        assert str(e.value) == 'score_select: 65 listed items per session; csrc/recommend.hip takes at most 64'


def test_score_select_refuses_k_out_of_range():
    ops, maxk = pkg('ops'), pkg('_lib').CONST['SREC_SELECT_MAXK']
    for k in (0, maxk + 1):
        with pytest.raises(ValueError) as e:
            ops.score_select(torch.zeros(B, D), torch.zeros(V, D), None, k)
        assert str(e.value) == ('score_select: k = %d; the selection kernel of csrc/recommend.hip keeps between 1 and %d items '
                                'per session' % (k, maxk))


def test_ops_re_exports_the_scoring_module():
    ops, score = pkg('ops'), pkg('score')
    for name in ('CEWorkspace', 'TableBF16', 'ScoreCE', 'ScoreStats', 'ScoreLogProb', 'score_ce', 'score_stats', 'score_logp',
                 'score_topk', 'score_rank', 'score_select', 'use_bf16_scoring', '_bf16_dim_ok', '_prepare_sr', '_ce_fwd',
                 '_ce_bwd', '_pad_rows', '_mixture_args', '_byte_ws', '_logp_cols', 'finish_table_grad', 'sr16_written',
                 'sr16_claim'):
        assert getattr(ops, name) is getattr(score, name), name
    ops.PRECISION['matmul'] = 'bf16'                     # read through the module at call time, never a copied value
    try:
        assert score.use_bf16_scoring(64) and not score.use_bf16_scoring(258)
    finally:
        ops.PRECISION['matmul'] = 'fp32'
    assert not score.use_bf16_scoring(64)
