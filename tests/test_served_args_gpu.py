"""The host plumbing of the served score on the GPU: the srec_served that score._served_args(...).struct() fills names exactly
the tensors it was given - pointers, strides, counts - for contiguous inputs, a row-strided view of the session vectors and
a column slice of a wider bias.  A wrong stride or pointer here is what no kernel would notice by itself; the calls at the
end must therefore return the same bits for the views as for contiguous copies of them."""
import pytest
import torch

from util import pkg

pytestmark = pytest.mark.gpu

B, V, D = 3, 10, 32


def _inputs(dev, C, L, strided):
    g = torch.Generator().manual_seed(11 + 7 * C + L)
    wide = torch.randn(C, B, 2 * D, generator=g).to(dev)
    srs = wide[:, :, D:] if strided else wide[:, :, D:].contiguous()
    srs = srs[0] if C == 1 else list(srs)                       # C = 1: a [B, d] view, row stride 2 d; else a list of C tensors
    table = torch.randn(V, D, generator=g).to(dev)
    cs = (torch.rand(V, generator=g) + 0.5).to(dev)
    off_ex, off_in = torch.randn(C, B, generator=g).to(dev), torch.randn(C, B, generator=g).to(dev)
    listed = torch.tensor([[1001, -1], [1004, 1009], [-1, 5]], dtype=torch.int32)[:, :L].to(dev) if L else None
    bias_wide = torch.randn(2, 2 * V, generator=g).to(dev)
    bias = bias_wide[:, 3:3 + V] if strided else bias_wide[:, 3:3 + V].contiguous()
    group = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    return srs, table, cs, off_ex, off_in, listed, bias, group


@pytest.mark.parametrize('strided', [False, True])
@pytest.mark.parametrize('L', [0, 2])
@pytest.mark.parametrize('C', [1, 3])
def test_the_struct_names_the_tensors_it_was_given(dev, C, L, strided):
    score, lib = pkg('score'), pkg('_lib')
    srs, table, cs, off_ex, off_in, listed, bias, group = _inputs(dev, C, L, strided)
    a = score._served_args('score_select', srs, table, cs, off_ex, off_in, listed, False, 1000, bias, group)
    s = a.struct()
    assert type(s) is lib.STRUCTS['srec_served']
    if C == 1:                                                  # taken as it is: the caller's memory, the view's row stride
        assert s.sr == srs.data_ptr() and (s.ld_sr, s.comp_stride) == (srs.stride(0), 0) == (2 * D if strided else D, 0)
    else:                                                       # stacked: the record's own block
        assert s.sr == a.srs.data_ptr() and (s.ld_sr, s.comp_stride) == (D, B * D) and torch.equal(a.srs, torch.stack(srs))
    assert s.E == table.data_ptr() and s.ld_e == table.stride(0) == D and s.cs == cs.data_ptr()
    assert s.off_ex == off_ex.data_ptr() and s.off_in == off_in.data_ptr()
    assert (s.listed, s.L) == ((listed.data_ptr(), 2) if L else (None, 0))
    assert (s.listed_mode, s.id_lo) == (lib.CONST['SREC_LISTED_SCORE'], 1000) and (s.B, s.V, s.d, s.C) == (B, V, D, C)
    assert s.bias == bias.data_ptr() and s.ld_bias == bias.stride(0) == (2 * V if strided else V)
    assert s.group == group.data_ptr() and s.G == 2
    d = score._served_args('score_select', srs, table, cs, off_ex, off_in, listed, True, 1000, None, None).struct()
    assert (d.listed_mode, d.off_in) == (lib.CONST['SREC_LISTED_DROP'], None)          # off_in is ignored under drop_listed
    assert (d.bias, d.ld_bias, d.group, d.G) == (None, 0, None, 1)                     # no bias: the plain call


@pytest.mark.parametrize('L', [0, 2])
@pytest.mark.parametrize('C', [1, 3])
def test_views_and_contiguous_copies_give_the_same_bits(dev, C, L):
    ops = pkg('ops')
    out = []
    for strided in (False, True):
        srs, table, cs, off_ex, off_in, listed, bias, group = _inputs(dev, C, L, strided)
        kw = dict(off_ex=off_ex, off_in=off_in, listed=listed, id_lo=1000, bias=bias, group=group)
        val, idx = ops.score_select(srs, table, cs, 4, **kw)
        items = ops.score_items(srs, table, cs, torch.arange(1000, 1000 + V, device=dev), **kw)
        out.append((val, idx, items, ops.score_norm(srs, table, cs, **kw)))
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert bool(torch.isfinite(out[0][2]).all()) and bool((out[0][1] >= 1000).all())
