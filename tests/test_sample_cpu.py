"""CPU half of drawing from the served distribution: the oracle's noise (tests/sample_oracle.py) against the library's host
restatement srec_sample_uniform and against ops.sample_noise, bit for bit; the C ABI of srec_score_sample (declared in the
order of srec_score_select, exported, bad arguments refused without a launch); the argument checks of
ops.score_sample and model.sample on CPU tensors; the launcher's flags; and the yardstick itself - the oracle's own draws
pass the statistical cases of tests/test_sample_gpu.py at their thresholds, and the seeds chosen there leave lists that
round-off cannot reorder."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import sample_oracle as so
import served_abi
from select_oracle import window_count
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
SEEDS = (0, 1, (7 << 32) | 5)
KEYS = np.array([0, 1, 2, -1, -77, 2 ** 31 - 1, -2 ** 31, 4095], dtype=np.int32)
IDS = np.array([0, 1, 37483, 2 ** 31 - 1, 2, 3, 1299, 5000], dtype=np.int32)


def _uniform(seed, keys, ids):
    dll = pkg('_lib').lib.load()
    keys, ids = np.ascontiguousarray(keys, dtype=np.int32), np.ascontiguousarray(ids, dtype=np.int32)
    h = np.full((len(keys), len(ids)), 0xdeadbeef, dtype=np.uint32)
    w = np.full((len(keys), len(ids)), -1.0, dtype=np.float32)
    assert dll.srec_sample_uniform(seed, keys.ctypes.data, len(keys), ids.ctypes.data, len(ids), h.ctypes.data, w.ctypes.data) == 0
    return h, w


# ------------------------------------------------------------------------------------------- the noise, three restatements
@pytest.mark.parametrize('seed', SEEDS)
def test_host_hash_and_uniform_equal_the_oracle_bit_for_bit(seed):
    h, w = _uniform(seed, KEYS, IDS)
    ho, wo = so.hash_hw(seed, KEYS, IDS)
    assert h.dtype == ho.dtype and np.array_equal(h, ho), (seed, h[0, :4], ho[0, :4])
    assert np.array_equal(w.view(np.uint32), wo.view(np.uint32)), seed
    assert float(w.min()) > 0.0 and float(w.max()) < 1.0
    # for a fixed session the hash is a bijection of the id: 4096 consecutive ids, 4096 values
    hh, _ = _uniform(seed, KEYS[:2], np.arange(4096))
    assert all(len(set(row.tolist())) == 4096 for row in hh)


def test_null_keys_and_ids_are_the_indices_and_bad_arguments_are_refused():
    dll = pkg('_lib').lib.load()
    h = np.zeros((3, 5), dtype=np.uint32)
    w = np.zeros((3, 5), dtype=np.float32)
    assert dll.srec_sample_uniform(9, None, 3, None, 5, h.ctypes.data, w.ctypes.data) == 0
    ho, wo = so.hash_hw(9, np.arange(3), np.arange(5))
    assert np.array_equal(h, ho) and np.array_equal(w, wo)
    h2 = np.zeros((3, 5), dtype=np.uint32)
    assert dll.srec_sample_uniform(9, None, 3, None, 5, h2.ctypes.data, None) == 0 and np.array_equal(h2, ho)
    assert dll.srec_sample_uniform(9, None, 3, None, 5, None, None) == 1001
    assert dll.srec_sample_uniform(9, None, -1, None, 5, h.ctypes.data, None) == 1001


def test_uniform_of_the_extreme_hashes_stays_inside_the_open_interval():
    """the clamp: h = 0xffffffff rounds to 2^32 as a float and w would be 1.0; h = 0 gives 2^-33, not 0"""
    h = np.array([0, 1, 127, 128, 2 ** 31, 2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1], dtype=np.uint32)
    w = so.w_of(h)
    assert w.dtype == np.float32 and float(w[0]) == 2.0 ** -33 and float(w[-1]) == 1.0 - 2.0 ** -24 == float(w[-2])
    assert float(w[-3]) < 1.0 and bool((np.diff(w.astype(np.float64)) >= 0).all())
    g = so.gumbel_of_w(w)
    assert np.isfinite(g).all() and abs(g[0] - 33 * np.log(2.0)) < 1e-9 and -2.82 < g[-1] < -2.80
    # the same through the library: the hash is a bijection of the id, so invert it for the hashes that clamp
    M = 0xffffffff

    def unhash(x):
        x ^= x >> 16
        x = x * pow(0x846ca68b, -1, 2 ** 32) & M
        x ^= (x >> 15) ^ (x >> 30)
        x = x * pow(0x7feb352d, -1, 2 ** 32) & M
        return x ^ (x >> 16)
    seed, q = (7 << 32) | 5, -77
    skey = int(so.hash_hw(seed, [q], [0])[0][0, 0])                      # h at gid 0 is h32(skey ^ 0x7F4A7C15)
    skey = unhash(skey) ^ 0x7F4A7C15
    want = [2 ** 32 - 1, 2 ** 32 - 128, 2 ** 32 - 129, 0]
    gids = [(((unhash(hv) ^ skey) - 0x7F4A7C15) & M) * pow(0x9E3779B1, -1, 2 ** 32) & M for hv in want]
    ids = np.array(gids, dtype=np.uint32).view(np.int32)                 # ids past 2^31 travel as their bit pattern here
    hh, ww = _uniform(seed, [q], ids)
    assert hh[0].tolist() == want and np.array_equal(ww, so.w_of(hh))
    assert ww[0].tolist() == [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, float(np.float32(1.0 - 2.0 ** -24)), 2.0 ** -33]
    assert np.array_equal(so.hash_hw(seed, [q], ids)[0], hh)


@pytest.mark.parametrize('seed', SEEDS)
def test_ops_sample_noise_equals_the_oracle_exactly(seed):
    ops = pkg('ops')
    ids = np.concatenate([IDS, np.arange(3000)])
    g = ops.sample_noise(seed, torch.from_numpy(KEYS), torch.from_numpy(ids))
    go = so.gumbel64(seed, KEYS, ids)
    assert g.dtype == torch.float64 and g.shape == (len(KEYS), len(ids))
    assert torch.equal(g, go), float((g - go).abs().max())
    assert torch.equal(ops.sample_noise(seed, KEYS.tolist(), ids.tolist()), go)       # plain sequences too
    # the arithmetic-only logarithm both use, against the library logarithms: last-place differences only
    w = so.hash_hw(seed, KEYS, ids)[1].astype(np.float64)
    ref = -np.log(-np.log1p(-w))
    assert float(np.abs(go.numpy() - ref).max()) < 1e-14
    assert float(go.min()) > -2.82 and float(go.max()) < 22.9
    with pytest.raises(ValueError, match=r'^sample_noise: seed must be an integer in \[0, 2\^64\)'):
        ops.sample_noise(-1, KEYS, ids)


# ------------------------------------------------------------------------------------------- C ABI
HEAD = [('const void*', 'served'), ('int', 'K')]
NOISE = [('float', 'inv_temperature'), ('unsigned long long', 'seed'), ('const int*', 'session_keys')]
TAIL = [('const float*', 'floor'), ('float*', 'out_key'), ('int*', 'out_idx'), ('void*', 'ws'), ('void*', 'stream')]


def test_header_declares_the_entry_points_in_the_order_of_select_biased():
    """srec_score_select with the noise operands between K and floor"""
    L = pkg('_lib')
    protos = L.parse_header()
    sel = protos['srec_score_select']
    n = len(HEAD)
    assert sel[:n] == HEAD and L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS
    assert protos['srec_score_sample'] == HEAD + NOISE + TAIL
    assert [t for t, _ in sel[n:]] == [t for t, _ in TAIL]
    assert protos['srec_score_sample_ws'] == protos['srec_score_select_ws']
    assert protos['srec_sample_uniform'] == [('unsigned long long', 'seed'), ('const int*', 'session_keys'), ('int', 'n_b'),
                                             ('const int*', 'ids'), ('int', 'n_v'), ('unsigned*', 'h_out'), ('float*', 'w_out')]
    dll = L.lib.load()                                  # binds every declared symbol: a missing export raises here
    assert len(dll.srec_score_sample.argtypes) == n + len(NOISE) + len(TAIL)
    assert dll.srec_score_sample.argtypes[n:n + 2] == [ctypes.c_float, ctypes.c_ulonglong]


def test_c_entry_refuses_bad_arguments_without_a_launch():
    dll = pkg('_lib').lib.load()
    good = dict(sr=0x1000, ld_sr=32, comp_stride=0, E=0x2000, ld_e=32, cs=None, off_ex=None, off_in=None, listed=None, L=0,
                listed_mode=0, id_lo=0, B=2, V=10, d=32, C=1, K=5, bias=0x6000, ld_bias=10, group=0x7000, G=3, inv_temperature=1.0,
                seed=7, session_keys=0x9000, floor=None, out_key=0x4000, out_idx=0x5000, ws=0x8000, stream=None)
    rest = [a for _, a in HEAD[1:] + NOISE + TAIL]
    inf = float('inf')
    for change in (dict(K=129), dict(K=0), dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=inf),
                   dict(inv_temperature=float('nan')), dict(session_keys=0x9002),
                   dict(floor=0xa002),
                   # ... and everything srec_score_select refuses
                   dict(G=0), dict(group=None), dict(ld_bias=9), dict(bias=0x6002), dict(group=0x7001), dict(d=30), dict(d=1028),
                   dict(C=5), dict(C=0), dict(L=65), dict(listed_mode=2), dict(out_key=None), dict(out_idx=None), dict(ws=None),
                   dict(id_lo=-1), dict(id_lo=2 ** 31 - 5), dict(E=0x2004), dict(ld_e=30), dict(bias=None, group=None, G=2)):
        assert served_abi.call(dll.srec_score_sample, rest, {**good, **change}) == 1001, change
        assert served_abi.call(dll.srec_score_sample, rest, {**good, 'floor': 0xa000, **change}) == 1001, change   # (was _floor)
    assert served_abi.call(dll.srec_score_sample, rest, {**good, 'B': 0}) == 0              # no sessions: nothing to do
    assert served_abi.call(dll.srec_score_sample, rest, good, null=True) == 1001            # no descriptor
    n, m = ctypes.c_long(-1), ctypes.c_long(-2)
    assert dll.srec_score_sample_ws(512, 37484, 256, 3, 20, 100, ctypes.addressof(n)) == 0 and n.value > 0
    assert dll.srec_score_select_ws(512, 37484, 256, 3, 20, 100, ctypes.addressof(m)) == 0 and m.value == n.value
    assert dll.srec_score_sample_ws(2, 10, 32, 1, 0, 129, ctypes.addressof(n)) == 1001
    assert dll.srec_score_sample_ws(2, 10, 32, 1, 0, 5, None) == 1001


# ------------------------------------------------------------------------------------------- ops.score_sample argument checks
def test_score_sample_refuses_bad_arguments_on_cpu_tensors():
    """anything that reached the library would raise RuntimeError (CPU tensors) instead"""
    ops, score = pkg('ops'), pkg('score')
    assert ops.score_sample is score.score_sample and ops.sample_noise is score.sample_noise
    B, V = 4, 10
    sr, E = torch.zeros(B, 8), torch.zeros(V, 8)
    for kw, msg in ((dict(k=0), 'k = 0; the selection kernel .* keeps between 1 and 128'),
                    (dict(k=129), 'k = 129'),
                    (dict(temperature=0.0), r'temperature = 0\.0; it must be positive and finite'),
                    (dict(temperature=-0.5), 'temperature = -0.5'),
                    (dict(temperature=float('inf')), 'temperature = inf'),
                    (dict(temperature=float('nan')), 'temperature = nan'),
                    (dict(temperature=1e-40), 'it must be positive and finite'),          # 1 / T is not a finite fp32
                    (dict(temperature='hot'), 'temperature must be a number'),
                    (dict(seed=-1), r'seed must be an integer in \[0, 2\^64\), got -1'),
                    (dict(seed=2 ** 64), 'seed must be an integer'),
                    (dict(seed=1.5), 'seed must be an integer'),
                    (dict(session_keys=torch.zeros(B + 1, dtype=torch.int64)), 'session_keys must hold 4 integers'),
                    (dict(session_keys=torch.zeros(B)), 'session_keys must hold 4 integers'),
                    (dict(bias=torch.zeros(V + 1)), 'bias has 11 columns for 10 table rows'),
                    (dict(group=torch.zeros(B, dtype=torch.int64)), 'group is given without a bias'),
                    (dict(listed=torch.zeros(B, 65, dtype=torch.int64)), r'65 listed items per session; csrc/recommend\.hip takes at most 64')):
        kw = dict(dict(k=3), **kw)
        with pytest.raises(ValueError, match='^score_sample: .*' + msg):
            ops.score_sample(sr, E, None, **kw)
    key, idx = ops.score_sample(torch.zeros(0, 8), E, None, 3, seed=2 ** 64 - 1)          # no sessions: nothing is launched
    assert key.shape == idx.shape == (0, 3) and key.dtype == torch.float32 and idx.dtype == torch.int32
    with pytest.raises(RuntimeError, match='need GPU'):                                  # good arguments reach the library: no fallback
        ops.score_sample(sr, E, None, 3, temperature=0.5, seed=5, session_keys=torch.arange(B))
    assert 'sample' not in {k[0] for k in score._BYTE_WS} and isinstance(score._SAMPLE_WS, dict)


def test_model_sample_takes_the_keywords_and_checks_before_the_model_runs():
    import inspect
    mixin = pkg('srgnn')._ScoringMixin
    sig = inspect.signature(mixin.sample).parameters
    want = dict(k=1, temperature=1.0, seed=0, session_keys=None, exclude_seen=False, item_bias=None, item_group=None, renormalize=False)
    for name, default in want.items():
        assert sig[name].default == default and sig[name].kind is sig[name].KEYWORD_ONLY, name
    assert callable(pkg('dist').VocabParallel.sample) and callable(pkg('dist').HipLocal.sample)
    model = pkg().SRGNN(50, 32, 1).train()
    model.session_repr = None                                   # anything that ran the model would fail on this
    for kw, msg in ((dict(item_bias=torch.zeros(51)), r'sample: item_bias must be a floating tensor \[50\]'),
                    (dict(item_group=torch.zeros(2, dtype=torch.int64)), 'sample: item_group is given without an item_bias'),
                    (dict(temperature=0.0), 'sample: temperature = 0.0; it must be positive and finite'),
                    (dict(temperature=float('nan')), 'sample: temperature = nan'),
                    (dict(k=129), 'sample: k = 129'), (dict(seed=-3), 'sample: seed must be an integer')):
        with pytest.raises(ValueError, match='^' + msg):
            model.sample(None, **kw)
        assert model.training


# ------------------------------------------------------------------------------------------- launcher
def test_launcher_accepts_the_sampling_flags():
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend as rec
    finally:
        sys.path.remove(SCRIPTS)
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt']
    a = rec.parse(base)
    assert a.sample is False and a.temperature == 1.0 and a.seed == 0
    a = rec.parse(base + ['--sample', '--seed', '5', '--temperature', '0.7', '--top', '10', '--exclude-seen'])
    assert a.sample is True and a.seed == 5 and a.temperature == 0.7 and a.top == 10 and a.exclude_seen
    assert rec.parse(base + ['--sample', '--seed', str(2 ** 64 - 1)]).seed == 2 ** 64 - 1
    for bad in (['--temperature', '0'], ['--temperature', '-1'], ['--temperature', 'inf'], ['--temperature', 'nan'],
                ['--seed', '-1'], ['--seed', str(2 ** 64)]):
        with pytest.raises(SystemExit):
            rec.parse(base + ['--sample'] + bad)
    helptext = rec.parser('SRGNN').format_help()
    assert all(f in helptext for f in ('--sample', '--temperature', '--seed'))


# ------------------------------------------------------------------------------------------- the yardstick on its own
@pytest.mark.parametrize('T', so.LIST_TS)
def test_oracle_draws_pass_the_statistical_cases_at_their_thresholds(T):
    """the draws of the oracle itself (seed STAT_SEED, keys 0 .. 4095): first-draw counts against softmax(s' / T) over the six
    eligible items, ordered pairs against Plackett-Luce - and the positive control: counts drawn at T = 0.5 fail against the
    T = 1 probabilities"""
    first = so.oracle_draw(8, 1, T)[:, 0]
    c1 = so.chi2_first(first, so.stat_probs(8, T))
    pairs = so.oracle_draw(5, 2, T)
    c2 = so.chi2_pairs(pairs, so.stat_probs(5, T))
    print('T %.1f: first-draw chi-square %.2f (5 dof, < %.2f), ordered pairs %.2f (19 dof, < %.2f)' % (T, c1, so.CHI2_5, c2, so.CHI2_19))
    assert c1 < so.CHI2_5 and c2 < so.CHI2_19
    assert int(so.stat_probs(8, T).gt(0).sum()) == 6 and int(so.stat_probs(5, T).gt(0).sum()) == 5
    if T == 0.5:
        assert so.chi2_first(first, so.stat_probs(8, 1.0)) > 10 * so.CHI2_5
        assert so.chi2_pairs(pairs, so.stat_probs(5, 1.0)) > 10 * so.CHI2_19


def test_oracle_statistics_hold_for_other_seeds_and_neighbours_are_uncorrelated():
    for seed in (0, 1, (7 << 32) | 5):
        c1 = so.chi2_first(so.oracle_draw(8, 1, 1.0, seed)[:, 0], so.stat_probs(8, 1.0))
        c2 = so.chi2_pairs(so.oracle_draw(5, 2, 1.0, seed), so.stat_probs(5, 1.0))
        assert c1 < so.CHI2_5 and c2 < so.CHI2_19, (seed, c1, c2)
        _, w = so.hash_hw(seed, np.arange(512), np.arange(512))
        w = w.astype(np.float64) - 0.5
        for a, b in ((w[:-1], w[1:]), (w[:, :-1], w[:, 1:])):                    # adjacent sessions, adjacent items
            assert abs(float((a * b).mean() / w.var())) < 0.02, seed
        assert abs(float(w.mean())) < 0.005


def test_chosen_seeds_leave_lists_round_off_cannot_blur():
    """the GPU tests' conditions against vacuity, checked where there is no GPU: the noise-only case is decided beyond twice
    the noise tolerance; every list case keeps at most 4 keys within 2 tol of its K-th best"""
    B, V, d, K = so.NOISE_SHAPE
    gap = so.min_gap(so.key64(torch.zeros(B, V, dtype=torch.float64), 1.0, so.NOISE_SEED), K)
    print('noise-only case: smallest gap among the %d best keys %.2e' % (K + 1, gap))
    assert gap > 2 * so.TOL_NOISE
    worst = 0
    for (B, V, d) in so.LIST_SHAPES:
        for kind in so.LIST_KINDS:
            for mode in ('row', 'groups'):
                s, dm = so.biased64(*so.list_case(B, V, d, kind, mode))
                assert int((~dm).sum(1).min()) > so.LIST_K
                for T in so.LIST_TS:
                    near = int(window_count(so.key64(s, T, so.LIST_SEED), so.LIST_K, so.tol_key(T), dm).max())
                    worst = max(worst, near)
                    assert near <= 4, (B, V, d, kind, mode, T, near)
    print('list cases: at most %d keys within 2 tol of the K-th best' % worst)
