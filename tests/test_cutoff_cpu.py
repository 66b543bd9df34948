"""The cutoff oracle (tests/cutoff_oracle.py) against a brute-force sort, the facts about the shared cases that keep the GPU
tests from becoming vacuous, and the host-side argument checks of truncated sampling.  No GPU."""
import os
import random
import subprocess
import sys

import pytest
import torch

import cutoff_oracle as co
from select_oracle import scores64
from util import ROOT, pkg

NINF = float('-inf')


# ------------------------------------------------------------------------------------------- the oracle
def test_oracle_equals_a_brute_force_sort_on_tiny_inputs():
    rnd = random.Random(5)
    g = torch.Generator().manual_seed(5)
    for trial in range(60):
        B, V = 4, rnd.choice([1, 2, 7, 12])
        s = torch.randint(-6, 7, (B, V), generator=g).double() / 4             # many ties
        s[torch.rand(B, V, generator=g) < 0.15] = NINF                         # eligible rows that score -inf
        s[0, 0] = -0.0
        dm = torch.rand(B, V, generator=g) < 0.25
        if trial % 5 == 0:
            dm[1] = True                                                       # a session with nothing eligible
        if trial % 7 == 0:
            s[2] = NINF                                                        # ... and one whose rows all score -inf
        T = rnd.choice([1.0, 0.5, 2.0])
        crit = dict(top_k=rnd.choice([None, 1, 3, V, V + 2]), top_p=rnd.choice([None, 0.3, 0.62, 0.9, 1.0]),
                    min_p=rnd.choice([None, 1.0, 0.5, 0.01]))
        f = co.floor64(s, dm, T, **crit)
        n = co.count64(s, dm, f)
        lk = co.kept64(s, dm, T, f)
        m = co.weights64(s, dm, T)[1]
        for b in range(B):
            bf, bn, blk, bm = co.brute(s[b].tolist(), (~dm[b]).tolist(), T, **crit)
            assert (float(f[b]), int(n[b]), float(m[b])) == (bf, bn, bm), (trial, b, crit)
            assert float(lk[b]) == blk or abs(float(lk[b]) - blk) < 1e-12, (trial, b, crit, float(lk[b]), blk)
        assert not bool(torch.isnan(f).any() | torch.isnan(lk).any())


def test_oracle_edge_cases():
    s = torch.tensor([[1.0, 1.0, 0.0, NINF], [NINF, NINF, NINF, NINF], [2.0, 1.0, 0.0, -1.0]], dtype=torch.float64)
    dm = torch.tensor([[False] * 4, [False, False, True, True], [True] * 4])
    f = co.floor64(s, dm, 1.0, top_p=0.3)
    assert f.tolist() == [1.0, NINF, NINF]                                     # the tie at the boundary is inside
    assert co.count64(s, dm, f).tolist() == [2, 2, 0]
    assert co.kept64(s, dm, 1.0, f).tolist()[1:] == [0.0, NINF]
    assert co.floor64(s, dm, 1.0, top_k=4).tolist() == [NINF, NINF, NINF]
    assert co.count64(s, dm, co.floor64(s, dm, 1.0, top_k=4)).tolist() == [4, 2, 0]
    assert co.floor64(s, dm, 1.0, min_p=1.0).tolist() == [1.0, NINF, NINF]
    assert co.floor64(s, dm, 1.0).tolist() == [NINF] * 3


# ------------------------------------------------------------------------------------------- the shared cases
@pytest.mark.parametrize('B,V,d,least', [(33, 5000, 96, 30), (37, 1300, 64, 35), (40, 3429, 64, 39)])
def test_exact_cases_are_exact_and_mostly_decided(B, V, d, least):
    sr, E, cs = co.exact_inputs(B, V, d)
    s64 = scores64(sr, E, cs)
    assert torch.equal(torch.matmul(sr, (E * cs[:, None]).t()).double(), s64)
    assert torch.equal(torch.matmul(sr, E.t()) * cs[None, :], s64.float())
    sizes, ties = [], []
    for T in co.EXACT_TS:
        for p in co.EXACT_PS:
            dec = co.decided(s64, None, T, p)
            t = co.tau_p64(s64, None, T, p)
            sizes += co.count64(s64, None, t).tolist()
            ties += (s64 == t[:, None]).sum(1).tolist()
            assert int(dec.sum()) >= least and float(dec.double().mean()) >= 0.85, (T, p, int(dec.sum()))
    print((B, V, d), 'nuclei of %d .. %d items, up to %d tied at the boundary' % (min(sizes), max(sizes), max(ties)))
    assert min(sizes) >= 1 and max(sizes) > 128          # (past the selection kernel's pool)


@pytest.mark.parametrize('scale', [1.0, 3.0])
def test_random_cases_have_a_narrow_tolerant_interval(scale):
    sr, E, cs = co.random_inputs(scale)
    s64 = scores64(sr, E, cs)
    for T in co.EXACT_TS:
        for p in co.EXACT_PS:
            n_lo, n_hi = co.top_p_interval(s64, None, T, p)
            w = n_hi - n_lo
            exact = co.count64(s64, None, co.tau_p64(s64, None, T, p))
            assert bool(((n_lo <= exact) & (exact <= n_hi)).all())
            print('x%g T %.1f p %.1f: interval width max %d at counts %d .. %d' % (scale, T, p, int(w.max()), int(exact.min()), int(exact.max())))
            assert int(w.max()) <= 16


# ------------------------------------------------------------------------------------------- checks
@pytest.mark.parametrize('bad', [dict(top_k=0), dict(top_k=-3), dict(top_k=1.5), dict(top_k=True), dict(top_k=2 ** 31), dict(top_k='4'),
                                 dict(top_p=0), dict(top_p=0.0), dict(top_p=-0.2), dict(top_p=float('nan')), dict(top_p=1e-60),
                                 dict(top_p='x'), dict(top_p=True),
                                 dict(min_p=0), dict(min_p=-1.0), dict(min_p=1.01), dict(min_p=float('nan')), dict(min_p=float('inf')),
                                 dict(min_p='x'),
                                 dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('inf')),
                                 dict(temperature=float('nan')), dict(temperature='hot'), dict(temperature=1e-39)])
def test_cutoff_scalars_rejects_bad_values_in_the_callers_words(bad):
    ops = pkg('ops')
    kw = dict(top_k=None, top_p=None, min_p=None, temperature=1.0)
    kw.update(bad)
    with pytest.raises(ValueError, match='^someone: '):
        ops.cutoff_scalars('someone', **kw)


def test_cutoff_scalars_values():
    ops = pkg('ops')
    assert ops.cutoff_scalars('w', None, None, None, 1.0) == (0, 1.0, float('inf'), 1.0)
    assert ops.cutoff_scalars('w', 10 ** 6, 1.0, 1.0, 2.0) == (10 ** 6, 1.0, 0.0, 0.5)
    assert ops.cutoff_scalars('w', None, 1.5, None, 1.0)[1] == 1.0
    assert ops.cutoff_scalars('w', None, 1.0 - 1e-12, None, 1.0)[1] == 1.0          # rounds to 1 in fp32: no criterion
    k, p, gap, inv_t = ops.cutoff_scalars('w', 7, 0.9, 1e-3, 0.5)
    assert (k, inv_t) == (7, 2.0) and p == float(torch.tensor(0.9, dtype=torch.float32)) and gap == co.gap32(0.5, 1e-3)


def test_score_cutoff_checks_before_any_launch():
    """bad scalars raise on CPU tensors: nothing was launched and the library was not called"""
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(5, 8)
    for bad in (dict(top_k=0), dict(top_p=0.0), dict(min_p=2.0), dict(temperature=0.0)):
        with pytest.raises(ValueError, match='^score_cutoff: '):
            ops.score_cutoff(sr, E, None, **bad)
    with pytest.raises(ValueError, match='^score_cutoff: 65 listed'):
        ops.score_cutoff(sr, E, None, listed=torch.zeros(3, 65, dtype=torch.int64), top_k=2)
    with pytest.raises(ValueError, match='^score_select: floor'):
        ops.score_select(sr, E, None, 2, floor=torch.zeros(4))
    with pytest.raises(ValueError, match='^score_sample: floor'):
        ops.score_sample(sr, E, None, 2, floor=torch.zeros(3, dtype=torch.int64))


def test_header_declares_what_the_library_exports_for_the_cutoff():
    L = pkg('_lib')
    want = {'srec_score_cutoff_ws', 'srec_score_cutoff_hist', 'srec_score_cutoff_advance', 'srec_score_cutoff_tail',
            'srec_score_cutoff_finish', 'srec_score_cutoff', 'srec_score_select', 'srec_score_sample'}
    protos = L.lib.protos
    assert want <= set(protos)
    # the floor is an operand of the selection and of the draw themselves: no _floor variants
    assert not {'srec_score_select_floor', 'srec_score_sample_floor'} & set(protos)
    assert ('const float*', 'floor') in protos['srec_score_select'] and ('const float*', 'floor') in protos['srec_score_sample']
    served, t = [('const void*', 'served')], ('float', 'inv_temperature')
    assert protos['srec_score_cutoff_hist'] == served + [t, ('int', 'top_k'), ('float', 'top_p'), ('int', 'pass'), ('const float*', 'top'),
                                                         ('const long long*', 'state'), ('long long*', 'hist'), ('void*', 'stream')]
    assert protos['srec_score_cutoff_tail'] == served + [t, ('const float*', 'top'), ('const float*', 'floor'), ('long long*', 'hist'),
                                                         ('void*', 'stream')]
    assert protos['srec_score_cutoff'] == served + [t, ('int', 'top_k'), ('float', 'top_p'), ('float', 'min_gap'), ('float*', 'floor'),
                                                    ('int*', 'count'), ('float*', 'log_kept'), ('float*', 'top'), ('void*', 'ws'),
                                                    ('void*', 'stream')]
    assert L.CONST['SREC_CUTOFF_PASSES'] == 4 and L.CONST['SREC_CUTOFF_STATE'] == 8
    if os.path.exists(L.LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln and ln.split()[-1].startswith('srec_')}
        assert exported == set(L.lib.protos), sorted(exported ^ set(L.lib.protos))


def test_recommend_launcher_rejects_the_cutoff_flags_without_sample(tmp_path):
    script = os.path.join(ROOT, 'src', 'scripts', 'recommend.py')
    for flag, val in (('--sample-top-k', '5'), ('--sample-top-p', '0.9'), ('--sample-min-p', '0.1')):
        r = subprocess.run([sys.executable, script, '--model', 'SRGNN', '--dataset-dir', os.path.join(ROOT, 'datasets', 'sample'),
                            '--checkpoint', str(tmp_path / 'missing.pt'), '--sessions', str(tmp_path / 'missing.txt'), flag, val],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and flag in r.stderr and '--sample' in r.stderr, (flag, r.stderr[-500:])
        assert 'missing.pt' not in r.stderr, 'the checkpoint was looked for before the flags were checked'
