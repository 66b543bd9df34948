"""CPU half of scoring given items: the float64 oracle against a hand-written case, the C ABI of srec_score_items (declared,
exported, bad arguments refused without a launch), the argument checks of ops.score_items that fire before any library
call, and the re-ranking launcher's parser, candidate padding and output format."""
import os
import subprocess
import sys

import pytest
import torch

import served_abi
from items_oracle import drop_mask, items64, order64
from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')
INF = float('inf')


# ------------------------------------------------------------------------------------------- oracle, by hand
S = torch.tensor([[0.5, -1.0, 2.0, 2.0, 0.25],
                  [1.0, 1.0, -3.0, 0.0, 4.0]], dtype=torch.float64)


def test_oracle_gathers_pads_and_leaves_foreign_ids_to_their_shard():
    items = torch.tensor([[2, -1, 0, 2, 4], [4, 4, 3, -1, 1]])
    want = torch.tensor([[2.0, -INF, 0.5, 2.0, 0.25], [4.0, 4.0, 0.0, -INF, 1.0]], dtype=torch.float64)
    assert torch.equal(items64(S, items), want)
    # a shared list
    assert torch.equal(items64(S, torch.tensor([3, -1, 0])), torch.tensor([[2.0, -INF, 0.5], [0.0, -INF, 1.0]], dtype=torch.float64))
    # two shards, columns [0, 2) and [2, 5): what one does not own is 0, padding is -inf on both, and the sum is the whole
    lo, hi = items64(S[:, :2], items, 0), items64(S[:, 2:], items, 2)
    assert torch.equal(lo, torch.tensor([[0.0, -INF, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, -INF, 1.0]], dtype=torch.float64))
    assert torch.equal(hi, torch.tensor([[2.0, -INF, 0.0, 2.0, 0.25], [4.0, 4.0, 0.0, -INF, 0.0]], dtype=torch.float64))
    assert torch.equal(lo + hi, want)
    # dropped lists: -inf on the owner only
    listed = torch.tensor([[2, -1], [1, 4]])
    wd = torch.tensor([[-INF, -INF, 0.5, -INF, 0.25], [-INF, -INF, 0.0, -INF, -INF]], dtype=torch.float64)
    assert torch.equal(items64(S, items, 0, drop_mask(listed, 5)), wd)
    lo, hi = items64(S[:, :2], items, 0, drop_mask(listed, 2, 0)), items64(S[:, 2:], items, 2, drop_mask(listed, 3, 2))
    assert float(lo[0, 0]) == 0.0 and float(hi[0, 0]) == -INF and float(lo[1, 4]) == -INF and float(hi[1, 4]) == 0.0
    assert torch.equal(lo + hi, wd)


def test_oracle_order_by_value_then_id_with_unfilled_slots_last():
    items = torch.tensor([[2, -1, 0, 3, 4], [4, 4, 3, -1, 1]])
    val, ids = order64(items64(S, items), items)
    assert ids.tolist() == [[2, 3, 0, 4, -1], [4, 4, 1, 3, -1]]          # 2.0 twice: id 2 before id 3; a repeated id twice
    assert val.tolist() == [[2.0, 2.0, 0.5, 0.25, -INF], [4.0, 4.0, 1.0, 0.0, -INF]]
    val, ids = order64(items64(S, items), items, k=2)
    assert ids.tolist() == [[2, 3], [4, 4]] and val.tolist() == [[2.0, 2.0], [4.0, 4.0]]


# ------------------------------------------------------------------------------------------- C ABI
REST = ['items', 'ld_items', 'M', 'out', 'stream']               # what follows the descriptor


def test_header_declares_score_items_and_the_library_exports_it():
    L = pkg('_lib')
    assert L.lib.protos['srec_score_items'] == [('const void*', 'served'), ('const int*', 'items'), ('long', 'ld_items'), ('int', 'M'),
                                                ('float*', 'out'), ('void*', 'stream')]
    assert L.STRUCTS['srec_served']._fields_ == served_abi.MEMBERS          # (id_lo among them, a long)
    dll = L.lib.load()                                  # binds every declared symbol: a missing export raises here
    assert len(dll.srec_score_items.argtypes) == 1 + len(REST)
    assert callable(pkg('ops').score_items) and pkg('ops').score_items is pkg('score').score_items


def test_c_entry_refuses_bad_arguments_without_a_launch():
    """every refusal happens ahead of the launch, so it can be provoked on a machine without a GPU with pointers that are
    never followed"""
    dll = pkg('_lib').lib.load()
    good = dict(sr=0x1000, ld_sr=32, comp_stride=0, E=0x2000, ld_e=32, cs=None, off_ex=None, off_in=None, listed=None, L=0,
                listed_mode=0, items=0x3000, ld_items=7, M=7, id_lo=0, B=2, V=10, d=32, C=1, out=0x4000, stream=None)
    bad = [dict(sr=0x1004), dict(E=0x2008), dict(d=30), dict(d=1028, ld_sr=1028, ld_e=1028), dict(C=0), dict(C=5),
           dict(L=65, listed=0x5000), dict(M=0), dict(id_lo=-1), dict(ld_items=3), dict(listed_mode=2), dict(items=None),
           dict(out=None), dict(ld_e=30), dict(ld_sr=34)]
    for change in bad:
        assert served_abi.call(dll.srec_score_items, REST, {**good, **change}) == 1001, change
    assert served_abi.call(dll.srec_score_items, REST, {**good, 'B': 0, 'd': 30}) == 0        # no sessions: nothing to do
    assert served_abi.call(dll.srec_score_items, REST, good, null=True) == 1001               # no descriptor


# ------------------------------------------------------------------------------------------- ops.score_items, before the library
def test_mixture_args_refuses_65_listed_items_in_score_items_words():
    score = pkg('score')
    with pytest.raises(ValueError, match=r'score_items: 65 listed items per session; csrc/score_items\.hip takes at most 64'):
        score._mixture_args('score_items', torch.zeros(3, 8), torch.zeros(20, 8), None, None, torch.zeros(3, 65, dtype=torch.int64))
    a = score._mixture_args('score_items', torch.zeros(3, 8), torch.zeros(20, 8), None, None, torch.zeros(3, 64, dtype=torch.int64))
    assert (a.L, a.C, a.B, a.d, a.V) == (64, 1, 3, 8, 20)


def test_score_items_refuses_bad_ids_before_any_library_call():
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(200, 8)      # CPU tensors: anything that reached the library would raise RuntimeError
    for items in (torch.tensor([[1, 2], [3, -2], [0, 0]]), torch.tensor([5, -7], dtype=torch.int32)):
        with pytest.raises(ValueError, match='score_items: item id -[27]'):
            ops.score_items(sr, E, None, items)
    with pytest.raises(ValueError, match='65 listed items per session'):
        ops.score_items(sr, E, None, torch.tensor([1]), listed=torch.zeros(3, 65, dtype=torch.int32), drop_listed=True)
    with pytest.raises(ValueError, match='2 rows for 3 sessions'):
        ops.score_items(sr, E, None, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.score_items(sr, E, None, torch.zeros(3, 4))
    # nothing to score: an empty result, no launch (CPU tensors again)
    assert ops.score_items(sr, E, None, torch.zeros(3, 0, dtype=torch.int64)).shape == (3, 0)
    assert ops.score_items(sr[:0], E, None, torch.tensor([1, 2])).shape == (0, 2)
    for cls, names in ((pkg().SRGNN, ('score_items', 'rerank')), (pkg().MSGIFSR, ('score_items', 'rerank', '_score_items')),
                       (pkg('dist').VocabParallel, ('score_items',)), (pkg('dist').HipLocal, ('score_items',))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


# ------------------------------------------------------------------------------------------- launcher
def _launcher():
    sys.path.insert(0, SCRIPTS)
    try:
        import rerank
    finally:
        sys.path.remove(SCRIPTS)
    return rerank


def test_rerank_launcher_help_parses():
    for model in ('SRGNN', 'MSGIFSR'):
        r = subprocess.run([sys.executable, os.path.join(SCRIPTS, 'rerank.py'), '--model', model, '--help'],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        for flag in ('--checkpoint', '--sessions', '--candidates', '--top', '--exclude-seen', '--batch-size', '--output',
                     '--precision', '--embedding-dim'):
            assert flag in r.stdout, flag
        assert ('--fusion' in r.stdout) == (model == 'MSGIFSR')


def test_rerank_launcher_parser_padding_and_line_count_error(capsys):
    rr = _launcher()
    base = ['--checkpoint', 'c.pt', '--sessions', 's.txt', '--candidates', 'c.txt']
    args = rr.parse(base)
    assert args.top is None and not args.exclude_seen and args.model == 'SRGNN' and args.candidates == 'c.txt'
    args = rr.parse(base + ['--model', 'MSGIFSR', '--extra', '--top', '500', '--exclude-seen'])
    assert args.top == 500 and args.extra and args.exclude_seen          # no limit of 128 here
    for wrong in (base + ['--top', '0'], base[:4], base + ['--batch-size', '0']):
        with pytest.raises(SystemExit):
            rr.parse(wrong)
    assert rr.pad_candidates([[5, 6, 7], [1], []]) == [[5, 6, 7], [1, -1, -1], [-1, -1, -1]]
    assert rr.pad_candidates([[4, 4]]) == [[4, 4]] and rr.pad_candidates([[], []]) == [[], []]
    p = rr.parser('SRGNN')
    sessions = [[1, 2], [3], [4, 5, 6]]
    assert rr.match_candidates(p, sessions, [[9, 8]]) == [[9, 8]] * 3                 # a single line serves every session
    assert rr.match_candidates(p, sessions, [[1], [2, 3], [4]]) == [[1], [2, 3], [4]]
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        rr.match_candidates(p, sessions, [[1], [2]])
    assert e.value.code == 2 and '--candidates has 2 lines for 3 sessions' in capsys.readouterr().err


def test_rerank_output_format_round_trip():
    rr, rec = _launcher(), __import__('recommend')
    assert rr.format_line is rec.format_line and rr.parse_line is rec.parse_line and rr.read_session_file is rec.read_session_file
    ids, vals = rr.parse_line(rr.format_line([7, 7, 3, -1], [-0.5, -0.5, -11.25, float('-inf')]) + '\n')
    assert ids == [7, 7, 3] and vals == [-0.5, -0.5, -11.25]
    assert rr.parse_line(rr.format_line([-1, -1], [float('-inf')] * 2)) == ([], [])
