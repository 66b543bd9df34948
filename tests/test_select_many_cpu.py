"""CPU side of the long top-N route (csrc/select_many.hip): the constants and entries of the C ABI, and the argument checks of
ops.score_select_many, model.recommend_many and the candidates.py launcher, which must raise before anything is loaded or
launched; the --ids-only line format against rerank.py's reader.  No GPU."""
import os
import subprocess
import sys

import pytest
import torch

from util import ROOT, pkg

SCRIPTS = os.path.join(ROOT, 'src', 'scripts')


def _script(name):
    sys.path.insert(0, SCRIPTS)
    try:
        return __import__(name)
    finally:
        sys.path.remove(SCRIPTS)


def test_constants_and_entries_of_the_header_and_the_library():
    L = pkg('_lib')
    assert L.CONST['SREC_SELECT_MANY_MAXK'] == 4096 and L.CONST['SREC_SELECT_MANY_SORT'] == 8192
    assert L.CONST['SREC_SELECT_MAXK'] == 128                        # (the selection kernel's limit stays)
    protos = L.lib.protos
    assert protos['srec_score_select_many_collect'] == [
        ('const void*', 'served'), ('const float*', 'floor'), ('int', 'cap'), ('float*', 'buf_val'), ('int*', 'buf_idx'),
        ('int*', 'n'), ('void*', 'stream')]
    assert protos['srec_score_select_many_order'] == [
        ('int', 'B'), ('int', 'cap'), ('const int*', 'n'), ('const float*', 'buf_val'), ('const int*', 'buf_idx'), ('int', 'K'),
        ('float*', 'out_val'), ('int*', 'out_idx'), ('void*', 'stream')]
    assert os.path.exists(L.LIB_PATH), 'the library is not built'
    out = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    assert {'srec_score_select_many_collect', 'srec_score_select_many_order'} <= exported


def test_score_select_many_checks_before_any_launch():
    """bad arguments raise ValueError on CPU tensors: nothing was launched and the library was not called"""
    ops = pkg('ops')
    sr, E = torch.zeros(3, 8), torch.zeros(5, 8)
    for k in (0, -1, 4097):
        with pytest.raises(ValueError, match='^score_select_many: k = '):
            ops.score_select_many(sr, E, None, k)
    with pytest.raises(ValueError, match='^score_select_many: floor must hold 3'):
        ops.score_select_many(sr, E, None, 200, floor=torch.zeros(4), cap=5)
    with pytest.raises(ValueError, match='^score_select_many: floor and cap come together'):
        ops.score_select_many(sr, E, None, 200, floor=torch.zeros(3))
    with pytest.raises(ValueError, match='^score_select_many: floor and cap come together'):
        ops.score_select_many(sr, E, None, 200, cap=5)
    with pytest.raises(ValueError, match='^score_select_many: cap = 0'):
        ops.score_select_many(sr, E, None, 200, floor=torch.zeros(3), cap=0)
    with pytest.raises(ValueError, match='^score_select_many: 65 listed'):
        ops.score_select_many(sr, E, None, 200, listed=torch.zeros(3, 65, dtype=torch.int64))
    assert ops.select_many_k('t', 1) == 1 and ops.select_many_k('t', 4096) == 4096
    # no sessions: empty lists, still no launch
    val, idx = ops.score_select_many(sr[:0], E, None, 200)
    assert val.shape == idx.shape == (0, 200) and val.dtype == torch.float32 and idx.dtype == torch.int32
    # good arguments on CPU tensors get as far as the launch, which has no fallback
    with pytest.raises(RuntimeError, match='GPU|libsrec'):
        ops.score_select_many(sr, E, None, 200, floor=torch.zeros(3), cap=5)


def test_recommend_many_checks_its_arguments_before_the_model_runs():
    from test_diversify_cpu import _cpu_model
    m = _cpu_model()
    for kw in (dict(k=0), dict(k=4097), dict(k=200, item_bias=torch.zeros(7)),
               dict(k=200, item_group=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError, match='^recommend_many: '):
            m.recommend_many(None, **kw)
    assert m._ROUTES['select_many'] == ('score_select_many', {})
    assert m._ROUTES['select'] == ('score_select', {})


def test_candidates_launcher_checks_top_and_keeps_recommends_limit(tmp_path):
    cand = _script('candidates')
    data = os.path.join(ROOT, 'datasets', 'sample')
    base = ['--model', 'SRGNN', '--dataset-dir', data, '--checkpoint', str(tmp_path / 'missing.pt'), '--sessions',
            str(tmp_path / 'missing.txt')]
    for top in ('0', '4097'):
        with pytest.raises(SystemExit):
            cand.parse(base + ['--top', top])
    args = cand.parse(base)
    assert args.top == 1000 and not args.ids_only and not args.exclude_seen and not args.renormalize
    args = cand.parse(base + ['--top', '4096', '--ids-only', '--exclude-seen', '--renormalize', '--batch-size', '7'])
    assert args.top == 4096 and args.ids_only and args.exclude_seen and args.renormalize and args.batch_size == 7
    rec = _script('recommend')
    with pytest.raises(SystemExit):
        rec.parse(base + ['--top', '129'])


def test_ids_only_lines_round_trip_through_reranks_reader(tmp_path):
    cand, rr = _script('candidates'), _script('rerank')
    lists = [[5, 3, 900, -1, -1], [7], [-1, -1], list(range(4096))]
    path = tmp_path / 'cands.txt'
    path.write_text(''.join(cand.format_ids(ids) + '\n' for ids in lists))
    back = rr.read_session_file(str(path))
    assert back == [[5, 3, 900], [7], [-1], list(range(4096))]      # a session without an item: rerank.py's padding id
    assert rr.pad_candidates(back[:3]) == [[5, 3, 900], [7, -1, -1], [-1, -1, -1]]
