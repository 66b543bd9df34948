"""Ensembles without a GPU: the float64 oracle of the multi-table score (tests/ensemble_oracle.py) against the single-table one,
the argument checks of ops.ens_select / ops.ens_ahead and of Ensemble (ValueError before anything is launched), the EM of
Ensemble.fit_weights, and the --members lines of src/scripts/ensemble.py."""
import importlib
import os
import sys

import pytest
import torch

from ensemble_oracle import exact_mixture, random_mixture, scores64_multi
from rank_oracle import scores64
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')


def _script(name):
    sys.path.insert(0, SCRIPTS)
    try:
        return importlib.import_module(name)
    finally:
        sys.path.remove(SCRIPTS)


# ------------------------------------------------------------------------------------------- 1) the oracle
@pytest.mark.parametrize('C', [1, 3])
def test_multi_table_oracle_is_the_single_table_oracle_when_the_tables_agree(C):
    g = torch.Generator().manual_seed(C)
    B, V, d = 7, 50, 16
    srs = torch.randn(C, B, d, generator=g)
    E, cs = torch.randn(V, d, generator=g), torch.rand(V, generator=g) + 0.5
    off, off_in = torch.randn(C, B, generator=g), torch.randn(C, B, generator=g)
    listed = torch.stack([torch.randperm(V + 10, generator=g)[:4] + 5 for _ in range(B)])
    listed[:, 3] = -1
    comps = [(srs[c], E, cs) for c in range(C)]
    for lst, oi, id_lo in ((None, None, 0), (listed, off_in, 0), (listed, off_in, 5)):
        a = scores64_multi(comps, off, oi, lst, id_lo)
        b = scores64(srs, E, cs, off, oi, lst, id_lo)
        assert a.dtype == torch.float64 and torch.equal(a, b)
    assert torch.equal(scores64_multi([(srs[0], E, None)]), scores64(srs[0], E))


def test_oracle_takes_a_table_per_component():
    comps, off, _, _ = random_mixture((8, 12), 3, 20, seed=0)
    s = scores64_multi(comps, off)
    ref = torch.logsumexp(torch.stack([scores64(sr, E, cs, off[c:c + 1]) for c, (sr, E, cs) in enumerate(comps)], 0), 0)
    assert torch.allclose(s, ref, rtol=0, atol=1e-12)


def test_exact_mixture_is_exact_in_fp32():
    comps, off, off_in, listed = exact_mixture((32, 100), 37, 700, seed=1)
    s = scores64_multi(comps, off, off_in, listed)
    assert torch.equal(s.float().double(), s)


# ------------------------------------------------------------------------------------------- 2) the launchers' checks
def _comps(C=2, B=4, V=10, d=8):
    return [(torch.zeros(B, d), torch.zeros(V, d), None) for _ in range(C)]


@pytest.mark.parametrize('fn', ['ens_select', 'ens_ahead'])
def test_launchers_refuse_bad_arguments_before_any_launch(fn):
    ops = pkg('ops')
    B, V = 4, 10

    def call(comps, off_ex=None, **kw):
        off_ex = torch.zeros(len(comps), B) if off_ex is None else off_ex
        if fn == 'ens_select':
            return ops.ens_select(comps, 3, off_ex, **kw)
        return ops.ens_ahead(comps, torch.zeros(B, dtype=torch.int32), torch.zeros(B), off_ex, **kw)

    with pytest.raises(ValueError, match='0 components'):
        call([])
    with pytest.raises(ValueError, match='9 components'):
        call(_comps(9))
    bad = _comps()
    bad[1] = (torch.zeros(B + 1, 8), bad[1][1], None)
    with pytest.raises(ValueError, match='component 1 has 5 sessions'):
        call(bad)
    bad = _comps()
    bad[1] = (bad[1][0], torch.zeros(V + 2, 8), None)
    with pytest.raises(ValueError, match='component 1 scores 12 items'):
        call(bad)
    bad = _comps()
    bad[0] = (bad[0][0].double(), bad[0][1], None)
    with pytest.raises(ValueError, match='component 0: sr must be a float32'):
        call(bad)
    bad = _comps()
    bad[1] = (bad[1][0], bad[1][1], torch.zeros(V, dtype=torch.float64))
    with pytest.raises(ValueError, match='component 1: cs must be a float32'):
        call(bad)
    bad = _comps()
    bad[1] = (bad[1][0].to('meta'), bad[1][1], None)
    with pytest.raises(ValueError, match='component 1: sr is on meta'):
        call(bad)
    bad = _comps()
    bad[1] = (torch.zeros(B, 6), torch.zeros(V, 6), None)
    with pytest.raises(ValueError, match='component 1: width 6'):
        call(bad)
    bad = _comps()
    bad[0] = (torch.zeros(B, 8), torch.zeros(V, 12), None)
    with pytest.raises(ValueError, match='component 0: sr has 8 columns, its table 12'):
        call(bad)
    with pytest.raises(ValueError, match=r'off_ex must be \[2, 4\]'):
        call(_comps(), torch.zeros(1, B))
    with pytest.raises(ValueError, match=r'off_in must be \[2, 4\]'):
        call(_comps(), off_in=torch.zeros(B, 2))
    with pytest.raises(ValueError, match='65 listed items'):
        call(_comps(), listed=torch.zeros(B, 65, dtype=torch.int32))
    with pytest.raises(ValueError, match='bias has 9 columns'):
        call(_comps(), bias=torch.zeros(V - 1))
    if fn == 'ens_select':
        for k in (0, 129):
            with pytest.raises(ValueError, match='k = %d' % k):
                ops.ens_select(_comps(), k, torch.zeros(2, B))
    else:
        with pytest.raises(ValueError, match='labels must hold 4'):
            ops.ens_ahead(_comps(), torch.zeros(B + 1, dtype=torch.int32), torch.zeros(B), torch.zeros(2, B))
        with pytest.raises(ValueError, match='target must hold 4'):
            ops.ens_ahead(_comps(), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), torch.zeros(2, B))


def test_descriptor_struct_holds_eight_components():
    lib = pkg('_lib')
    s = lib.ENS_STRUCTS['srec_served_multi']
    assert lib.ENS_CONST == {'SREC_ENS_MAXCOMP': 8} and 'srec_served_multi' not in lib.STRUCTS
    fields = dict(s._fields_)
    for name in ('sr', 'E', 'cs', 'ld_sr', 'ld_e', 'd'):
        assert fields[name]._length_ == 8, name
    assert [n for n, _ in s._fields_][6:] == ['C', 'off_ex', 'off_in', 'listed', 'L', 'listed_mode', 'id_lo', 'B', 'V', 'bias',
                                             'ld_bias', 'group', 'G']
    for name in ('srec_ens_select', 'srec_ens_select_ws', 'srec_ens_ahead', 'srec_ens_ahead_ws'):
        assert name in lib.lib.protos


def test_descriptor_layout_equals_the_compilers(tmp_path):
    """sizeof, every member's offset and size, and element [0] of every array member of srec_served_multi as g++ lays out
    include/srec.h (which includes include/srec_ens.h), against the class _lib binds from include/srec_ens.h"""
    import ctypes
    import subprocess
    lib = pkg('_lib')
    cls = lib.ENS_STRUCTS['srec_served_multi']
    want = {'sizeof': ctypes.sizeof(cls)}
    lines = ['printf("sizeof %zu\\n", sizeof(srec_served_multi));']
    for f, ty in cls._fields_:
        lines.append('printf("off.%s %%zu\\n", offsetof(srec_served_multi, %s));' % (f, f))
        lines.append('printf("size.%s %%zu\\n", sizeof(((srec_served_multi*)0)->%s));' % (f, f))
        want['off.' + f], want['size.' + f] = getattr(cls, f).offset, getattr(cls, f).size
        if issubclass(ty, ctypes.Array):
            lines.append('printf("row.%s %%zu\\n", sizeof(((srec_served_multi*)0)->%s[0]));' % (f, f))
            want['row.' + f] = ctypes.sizeof(ty._type_)
    src = tmp_path / 'layout.cpp'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "srec.h"\nint main() {\n%s\nreturn 0;\n}\n' % '\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.run(['g++', '-I', os.path.join(ROOT, 'include'), str(src), '-o', exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    got = {k: int(v) for k, v in zip(out[::2], out[1::2])}
    assert got == want and len(want) == 1 + 2 * 19 + 6, sorted(k for k in want if got.get(k) != want[k])


# ------------------------------------------------------------------------------------------- 3) Ensemble's checks
class _Stub:
    """what Ensemble's constructor looks at"""

    def __init__(self, n=10, shard=None, order=1, fusion=False, device='cpu'):
        self.n, self.shard, self.order, self.fusion, self.device = n, shard, order, fusion, device

    def _num_items(self):
        return self.n

    def _table(self):
        return torch.empty(0, device=self.device)


def test_ensemble_constructor_checks():
    Ensemble = pkg('ensemble').Ensemble
    assert pkg().Ensemble is Ensemble
    e = Ensemble([_Stub(), _Stub()])
    assert e.weights == [0.5, 0.5]
    e = Ensemble([_Stub(), _Stub(), _Stub()], weights=(1, 1, 2))
    assert e.weights == [0.25, 0.25, 0.5]
    with pytest.raises(ValueError, match='no members'):
        Ensemble([])
    with pytest.raises(ValueError, match='member 1 has 11 items, member 0 has 10'):
        Ensemble([_Stub(), _Stub(n=11)])
    with pytest.raises(ValueError, match='member 1 is on meta'):
        Ensemble([_Stub(), _Stub(device='meta')])
    with pytest.raises(ValueError, match='member 0 is row-sharded'):
        Ensemble([_Stub(shard=object()), _Stub()])
    with pytest.raises(ValueError, match='9 soft-maxes'):
        Ensemble([_Stub(order=3, fusion=True)] * 3)
    Ensemble([_Stub(order=3, fusion=True), _Stub(order=3, fusion=True), _Stub(order=3), _Stub()])      # 3 + 3 + 1 + 1
    with pytest.raises(ValueError, match='1 weights for 2 members'):
        Ensemble([_Stub(), _Stub()], weights=[1.0])
    for w in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='weights are positive and finite'):
            Ensemble([_Stub(), _Stub()], weights=[1.0, w])
    with pytest.raises(ValueError, match='inputs for 1 members, the ensemble has 2'):
        Ensemble([_Stub(), _Stub()]).recommend([()])


# ------------------------------------------------------------------------------------------- 4) fit_weights
def _loglik(lp, w):
    return float(torch.logsumexp(lp.double() + torch.log(w)[None, :], 1).mean())


def test_fit_weights_never_lowers_the_likelihood():
    Ensemble = pkg('ensemble').Ensemble
    g = torch.Generator().manual_seed(0)
    lp = -3.0 + torch.randn(400, 3, generator=g) * 1.5
    lp[:, 1] += 0.5
    prev = _loglik(lp, torch.full((3,), 1 / 3, dtype=torch.float64))
    for it in range(1, 30):
        w = Ensemble.fit_weights(lp, iters=it)
        assert w.dtype == torch.float64 and abs(float(w.sum()) - 1.0) < 1e-12 and bool((w >= 0).all())
        ll = _loglik(lp, w)
        assert ll >= prev - 1e-12, (it, ll, prev)
        prev = ll
    assert abs(Ensemble.mean_log_likelihood(lp, w) - prev) < 1e-12
    # the fixed point of EM: the gradient of the likelihood on the simplex vanishes (mean responsibility / weight == 1)
    w = Ensemble.fit_weights(lp, iters=2000)
    r = torch.softmax(lp.double() + torch.log(w)[None, :], 1).mean(0)
    assert torch.allclose(r, w, atol=1e-9)


def test_fit_weights_drops_a_uniformly_worse_member_and_keeps_identical_ones_uniform():
    Ensemble = pkg('ensemble').Ensemble
    g = torch.Generator().manual_seed(1)
    a = -3.0 + torch.randn(200, generator=g)
    w = Ensemble.fit_weights(torch.stack([a, a - 2.0], 1))
    assert float(w[1]) < 0.01 and float(w[0]) > 0.99
    w = Ensemble.fit_weights(torch.stack([a, a, a], 1))
    assert torch.allclose(w, torch.full((3,), 1 / 3, dtype=torch.float64), atol=1e-12)
    # an example nobody gives any probability is left out; float32 input is computed in float64
    lp = torch.stack([a, a - 2.0], 1)
    lp[5] = float('-inf')
    assert float(Ensemble.fit_weights(lp)[1]) < 0.01
    with pytest.raises(ValueError, match=r'\[N, M\]'):
        Ensemble.fit_weights(a)


# ------------------------------------------------------------------------------------------- 5) --members lines
def test_members_lines_parse_as_recommend_flags(tmp_path):
    ens = _script('ensemble')
    m = ens.parse_member('--model SRGNN --checkpoint a.pt --weight 0.4')
    assert (m.model, m.checkpoint, m.weight, m.embedding_dim, m.num_layers) == ('SRGNN', 'a.pt', 0.4, 64, 2)
    assert m.dataset_dir is None and not hasattr(m, 'order')
    m = ens.parse_member('--model MSGIFSR --order 3 --fusion --checkpoint "b c.pt" --embedding-dim 32  # strong')
    assert (m.model, m.order, m.fusion, m.extra, m.checkpoint, m.weight, m.embedding_dim) == ('MSGIFSR', 3, True, False, 'b c.pt', None, 32)
    m = ens.parse_member('--checkpoint c.pt --dataset-dir ../x')
    assert (m.model, m.dataset_dir) == ('SRGNN', '../x')
    for line, why in (('--model SRGNN', 'checkpoint'), ('--model SRGNN --checkpoint a.pt --fusion', 'unrecognized'),
                      ('--model GRU4REC --checkpoint a.pt', 'invalid choice'), ('--checkpoint a.pt --weight 0', 'positive'),
                      ('--checkpoint a.pt --weight x', 'invalid float')):
        with pytest.raises(ValueError, match=why):
            ens.parse_member(line)
    f = tmp_path / 'members.txt'
    f.write_text('# two members\n--model SRGNN --checkpoint a.pt --weight 0.4\n\n--model NISER --checkpoint b.pt\n')
    ms = ens.read_members(str(f))
    assert [(m.model, m.weight) for m in ms] == [('SRGNN', 0.4), ('NISER', None)]
    f.write_text('--model SRGNN --checkpoint a.pt\n--model SRGNN\n')
    with pytest.raises(ValueError, match='line 2'):
        ens.read_members(str(f))
    f.write_text('# nothing\n')
    with pytest.raises(ValueError, match='names no member'):
        ens.read_members(str(f))
    (tmp_path / 'm2.txt').write_text('--model SRGNN --checkpoint a.pt\n--model MSGIFSR --checkpoint b.pt --dataset-dir ../y\n')
    args = ens.parse(['--members', str(tmp_path / 'm2.txt'), '--sessions', 's.txt', '--dataset-dir', '../z', '--top', '7'])
    assert [m.dataset_dir for m in args.member_list] == ['../z', '../y'] and args.top == 7 and args.catalog is None
    with pytest.raises(SystemExit):
        ens.parse(['--members', str(tmp_path / 'm2.txt')])
