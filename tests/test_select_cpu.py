"""CPU half of the top-N serving path: the float64 selection oracle against brute force, the C ABI of
srec_score_select, the argument checks of ops.score_select that fire before any GPU call, and the launcher's parser and
session-file reader."""
import os
import subprocess
import sys

import pytest
import torch

import served_abi
from select_oracle import drop_mask, merge_lists, select64
from util import GOLDEN, ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')


def _brute(s, k, dropped, id_lo):
    """python loops: eligible columns sorted by (-value, id)"""
    out_v, out_i = [], []
    for b, row in enumerate(s.tolist()):
        cols = sorted((c for c in range(len(row)) if c + id_lo not in dropped[b]), key=lambda c: (-row[c], c))[:k]
        out_v.append([row[c] for c in cols] + [float('-inf')] * (k - len(cols)))
        out_i.append([c + id_lo for c in cols] + [-1] * (k - len(cols)))
    return torch.tensor(out_v, dtype=torch.float64), torch.tensor(out_i)


@pytest.mark.parametrize('k', [1, 4, 9, 12])
@pytest.mark.parametrize('id_lo', [0, 100])
def test_oracle_selection_equals_brute_force_with_ties_drops_and_short_lists(k, id_lo):
    g = torch.Generator().manual_seed(5)
    s = torch.randint(-3, 4, (6, 9), generator=g).double() / 2          # 7 distinct values in 9 columns: ties everywhere
    s[2] = 1.0                                                          # a session whose columns all tie
    listed = torch.tensor([[id_lo + 1, -1, id_lo + 4], [-1, -1, -1], [id_lo, id_lo + 8, 5000], [id_lo + 3, id_lo + 3, -1],
                           [id_lo + 2, id_lo + 5, id_lo + 7], [7000, -1, id_lo + 6]])
    dropped = [set(x for x in row if x >= 0) for row in listed.tolist()]
    val, idx = select64(s, k, drop_mask(listed, 9, id_lo), id_lo)
    bv, bi = _brute(s, k, dropped, id_lo)
    assert torch.equal(val, bv) and torch.equal(idx, bi)
    # no list: nothing dropped; k > columns ends in (-inf, -1)
    val, idx = select64(s, k, None, id_lo)
    bv, bi = _brute(s, k, [set()] * 6, id_lo)
    assert torch.equal(val, bv) and torch.equal(idx, bi)
    if k > 9:
        assert bool((idx[:, 9:] == -1).all()) and bool(torch.isinf(val[:, 9:]).all())


def test_oracle_merge_of_shard_lists_equals_the_whole_selection():
    g = torch.Generator().manual_seed(6)
    s = torch.randint(-3, 4, (5, 30), generator=g).double() / 2
    listed = torch.randint(0, 30, (5, 4), generator=g)
    whole = select64(s, 12, drop_mask(listed, 30))
    a = select64(s[:, :13], 12, drop_mask(listed, 13, 0), 0)
    b = select64(s[:, 13:], 12, drop_mask(listed, 17, 13), 13)
    val, idx = merge_lists([a[0], b[0]], [a[1], b[1]], 12)
    assert torch.equal(val, whole[0]) and torch.equal(idx, whole[1])


def test_header_declares_both_functions_and_the_library_binds_them():
    L = pkg('_lib')
    protos = L.lib.protos
    assert [t for t, _ in protos['srec_score_select_ws']] == ['int'] * 6 + ['long*']
    assert protos['srec_score_select'] == [('const void*', 'served'), ('int', 'K'), ('const float*', 'floor'), ('float*', 'out_val'),
                                           ('int*', 'out_idx'), ('void*', 'ws'), ('void*', 'stream')]
    assert L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS      # the operands ahead of K, in the order they always had
    assert L.CONST['SREC_SELECT_MAXK'] == 128 and L.CONST['SREC_LISTED_SCORE'] == 0 and L.CONST['SREC_LISTED_DROP'] == 1
    dll = L.lib.load()                                  # binds every declared symbol: a missing export raises here
    assert len(dll.srec_score_select.argtypes) == 7 and len(dll.srec_score_select_ws.argtypes) == 7


def test_score_select_refuses_bad_arguments_before_any_gpu_call():
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(200, 8)      # CPU tensors: anything that reached the library would raise RuntimeError
    for k in (129, 0, -1):
        with pytest.raises(ValueError, match='score_select: k'):
            ops.score_select(sr, E, None, k)
    with pytest.raises(ValueError, match='65 listed items per session'):
        ops.score_select(sr, E, None, 20, listed=torch.zeros(3, 65, dtype=torch.int32), drop_listed=True)
    assert callable(getattr(pkg().SRGNN, 'recommend')) and callable(getattr(pkg('dist').VocabParallel, 'select'))


def test_recommend_launcher_help_parses():
    for model in ('SRGNN', 'MSGIFSR'):
        r = subprocess.run([sys.executable, os.path.join(SCRIPTS, 'recommend.py'), '--model', model, '--help'],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for flag in ('--checkpoint', '--sessions', '--top', '--exclude-seen', '--batch-size', '--output', '--embedding-dim'):
            assert flag in r.stdout, flag
        assert ('--fusion' in r.stdout) == (model == 'MSGIFSR')


def _launcher():
    sys.path.insert(0, SCRIPTS)
    try:
        import recommend
    finally:
        sys.path.remove(SCRIPTS)
    return recommend


def test_launcher_parser_bounds_and_session_capacity():
    rec = _launcher()
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt']
    args = rec.parse(base + ['--model', 'MSGIFSR', '--extra', '--top', '128'])
    assert args.model == 'MSGIFSR' and args.top == 128 and args.extra and not args.exclude_seen and args.embedding_dim == 256
    assert rec.parse(base).top == 20 and rec.parse(base).model == 'SRGNN'
    with pytest.raises(SystemExit):
        rec.parse(base + ['--top', '129'])
    with pytest.raises(SystemExit):
        rec.parse(['--sessions', 's.txt'])              # --checkpoint is required
    lim = dict(nodes=256, deg=128, sgat_deg=256)
    assert rec.session_capacity(lim) == 128 and rec.session_capacity(lim, order=3) == 85
    assert rec.session_capacity(lim, order=3, listed=True) == 64


def test_session_file_reader_round_trips_the_sample(tmp_path):
    rec = _launcher()
    path = os.path.join(GOLDEN, 'sample_test.txt')
    sessions = rec.read_session_file(path)
    assert len(sessions) > 40 and all(len(s) >= 1 and all(isinstance(i, int) for i in s) for s in sessions)
    assert [list(s) for s in pkg('dataset').read_sessions(path)] == sessions
    out = tmp_path / 'again.txt'
    out.write_text(rec.format_sessions(sessions))
    assert rec.read_session_file(str(out)) == sessions
    assert out.read_text().split() == open(path).read().split()
    ids, vals = rec.parse_line(rec.format_line([7, 3, -1], [-0.5, -1.25, float('-inf')]) + '\n')
    assert ids == [7, 3] and vals == [-0.5, -1.25]
