"""CPU side of the full-catalog target-rank evaluation: the metric arithmetic (train.metrics_from_ranks), the rank path
of train.evaluate on a materialising model, the shard additivity of dist.VocabParallel.target_rank over gloo (plain-torch
stand-in for the kernels, as tests/test_dist_cpu.py) and the launcher flags."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rank_oracle import ranks_exact, scores64
from test_dist_cpu import FakeModel, TorchLocal, _free_port
from util import GOLDEN, ROOT, pkg

from oracle import collate_ref as oc
from oracle import models_ref as om


def test_metrics_from_ranks_hand_values():
    train = pkg('train')
    # ranks: best item, the last one inside @5, the first one outside @5, no label, last inside @20, first outside @20
    m = train.metrics_from_ranks(torch.tensor([0, 4, 5, -1, 19, 20]), (5, 20))
    n = 5.0
    exp = {
        'hit@5': 2 / n, 'mrr@5': (1 + 1 / 5) / n, 'ndcg@5': (1 + 1 / math.log2(6)) / n,
        'hit@20': 4 / n, 'mrr@20': (1 + 1 / 5 + 1 / 6 + 1 / 20) / n,
        'ndcg@20': (1 + 1 / math.log2(6) + 1 / math.log2(7) + 1 / math.log2(21)) / n,
    }
    assert set(m) == set(exp)
    for k, v in exp.items():
        assert abs(m[k] - v) < 1e-12, (k, m[k], v)
    # only label-less sessions: nothing to average, no division by zero
    assert train.metrics_from_ranks(torch.tensor([-1, -1]), (10,)) == {'hit@10': 0.0, 'mrr@10': 0.0, 'ndcg@10': 0.0}


class _Wrap:
    def __init__(self, x):
        self.x = x

    def to(self, device):
        return self.x


def _evaluate_fixture(n_batches=10):
    z = np.load(os.path.join(GOLDEN, 'srgnn_evaluate.npz'))
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('init/')}
    model = om.SRGNN(3429, 32, 1)
    model.load_state_dict(init)
    ds = pkg('dataset')
    data = ds.AugmentedDataset(ds.read_sessions(os.path.join(ROOT, 'tests', 'golden', 'sample_test.txt')))
    fn = oc.collate_fn_factory(oc.seq_to_session_graph)
    batches = []
    for b in range(n_batches):
        inp, lab = fn([data[i] for i in range(b * 32, b * 32 + 32)])
        batches.append(([_Wrap(om.to_torch(x)) for x in inp], torch.from_numpy(lab)))
    return z, model, batches


def test_evaluate_rank_method_on_a_cpu_model_equals_topk_method():
    train = pkg('train')
    z, model, batches = _evaluate_fixture()
    cpu = torch.device('cpu')
    mrr0, hit0 = train.evaluate(model, batches, cpu)
    mrr1, hit1 = train.evaluate(model, batches, cpu, method='rank')
    assert hit1 == hit0 and abs(mrr1 - mrr0) < 1e-7, (mrr1, hit1, mrr0, hit0)
    assert abs(mrr1 - float(z['mrr'])) < 1e-7 and abs(hit1 - float(z['hit'])) < 1e-9
    m = train.evaluate(model, batches, cpu, method='rank', cutoffs=(5, 10, 20))
    assert m['mrr@20'] == mrr1 and m['hit@20'] == hit1
    assert m['hit@5'] <= m['hit@10'] <= m['hit@20'] and m['mrr@5'] <= m['ndcg@5'] <= m['hit@5']
    # the top-k method reports the same cutoffs from the 20 best items
    mt = train.evaluate(model, batches, cpu, cutoffs=(5, 10, 20))
    for k in m:
        assert abs(mt[k] - m[k]) < 1e-12, (k, mt[k], m[k])


# ------------------------------------------------------------------------------------------- shard additivity (gloo, W = 2)
class RankLocal(TorchLocal):
    """TorchLocal + the `rank` entry of dist.HipLocal: ops.score_rank's contract on one row shard, in float64 throughout
    (the summed target too: a float32 round trip would break the exact ties this test plants)"""

    def rank(self, srs, table, cs, labels, off_ex, off_in, listed, id_lo, target=None, target_only=False):
        s = scores64(srs, table, cs, off_ex, off_in, listed, id_lo)
        lab = labels.long()
        n = table.shape[0]
        if target is None:
            own = (lab >= id_lo) & (lab < id_lo + n)
            target = torch.where(own, s.gather(1, (lab - id_lo).clamp(0, n - 1)[:, None])[:, 0], torch.zeros(len(lab)).double())
        if target_only:
            return None, target
        return ranks_exact(s, lab, target, id_lo).to(torch.int32), target


def _rank_case():
    g = torch.Generator().manual_seed(11)
    V, d, B, C, L = 150, 16, 8, 2, 4
    eighth = lambda *shape: torch.randint(-8, 9, shape, generator=g).float() / 8      # exact products and sums
    table = eighth(V, d)
    table[130] = table[7]                                 # an exact tie across the two shards ...
    table[9] = table[8]                                   # ... and inside one
    srs = eighth(C, B, d)
    srs[:, 1], srs[:, 3] = srs[:, 0], srs[:, 2]          # sessions 0 / 1 and 2 / 3: same vectors, the two labels of a tied pair
    labels = torch.randint(0, V, (B,), generator=g)
    labels[0], labels[1], labels[2], labels[3], labels[4] = 130, 7, 9, 8, -1     # 130: owned by rank 1
    listed = torch.randint(0, V, (B, L), generator=g)
    listed[:, 0] = torch.arange(B) * 3 + 20               # distinct ids per row ...
    listed[:, 1] = torch.arange(B) * 3 + 100
    listed[:, 2] = torch.arange(B) * 3 + 21
    listed[:, 3] = -1
    listed[0, 1] = 130                                    # the label itself is listed (owner: rank 1)
    listed[1, 0] = 5                                      # a listed item owned by rank 0 ...
    off_ex = -eighth(C, B).abs()
    off_in = off_ex + 4.0                                 # ... that jumps ahead of everything once it is "in"
    return table, srs, labels, listed, off_ex, off_in


def _rank_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        D = pkg('dist')
        table, srs, labels, listed, off_ex, off_in = _rank_case()
        model = FakeModel(table)
        vp = D.VocabParallel(model, local=RankLocal())
        shard = model._table().detach()
        with torch.no_grad():
            mix = vp.target_rank(list(srs), shard, None, labels, off_ex, off_in, listed)
            one = vp.target_rank([srs[0]], shard, None, labels)
            n = labels.numel() // world
            sl = slice(rank * n, (rank + 1) * n)
            dp = vp.target_rank([s[sl] for s in srs], shard, None, labels[sl], off_ex[:, sl], off_in[:, sl], listed[sl],
                                data_parallel=True)
        q.put((rank, vp.lo, vp.hi, mix.tolist(), one.tolist(), dp.tolist()))
    finally:
        dist.destroy_process_group()


def test_sharded_target_rank_two_ranks_equal_unsharded():
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    table, srs, labels, listed, off_ex, off_in = _rank_case()
    ref_mix = ranks_exact(scores64(srs, table, None, off_ex, off_in, listed), labels)
    ref_one = ranks_exact(scores64(srs[0], table), labels)
    assert int(ref_mix[4]) == -1 and int(ref_one[4]) == -1
    # the duplicated rows tie exactly: the lower id of a pair is ahead of the higher one, never the other way round
    # (ids 8 and 9 are neighbours: exactly one more item ahead; between 7 and 130 other exact ties may sit as well)
    assert int(ref_one[0]) > int(ref_one[1]) and int(ref_one[2]) == int(ref_one[3]) + 1
    n = labels.numel() // world
    for rank, lo, hi, mix, one, dp in res:
        assert (lo <= 130 < hi) == (rank == 1) and (lo <= 5 < hi) == (rank == 0)
        assert mix == ref_mix.tolist(), (rank, mix, ref_mix.tolist())
        assert one == ref_one.tolist(), (rank, one, ref_one.tolist())
        assert dp == ref_mix[rank * n:(rank + 1) * n].tolist(), (rank, dp)


def test_cutoffs_beyond_the_topk_kernel_need_the_rank_method(monkeypatch):
    """the fused top-K keeps 32 items: --eval-cutoffs 50 with the top-K method is refused when the options are read, not
    after the first epoch"""
    train = pkg('train')
    sys.path.insert(0, ROOT)
    from src.scripts import common
    with pytest.raises(ValueError):
        train.check_eval_options('topk', (5, 50))
    train.check_eval_options('rank', (5, 50, 100))
    train.check_eval_options('topk', (5, 32))
    with pytest.raises(ValueError):
        train.TrainRunner('sample', torch.nn.Linear(2, 2), [], [], torch.device('cpu'), eval_cutoffs=(50,))
    monkeypatch.setattr(sys, 'argv', ['main_srgnn.py', '--eval-cutoffs', '5,50'])
    with pytest.raises(SystemExit):
        common.parse('SRGNN')
    monkeypatch.setattr(sys, 'argv', ['main_srgnn.py', '--eval-cutoffs', '5,50,100', '--eval-method', 'rank'])
    assert common.parse('SRGNN').eval_cutoffs == (5, 50, 100)


# ------------------------------------------------------------------------------------------- launcher flags
def _runner(monkeypatch, argv):
    sys.path.insert(0, ROOT)
    from src.scripts import common
    train = pkg('train')
    monkeypatch.setattr(sys, 'argv', ['main_srgnn.py'] + argv)
    args = common.parse('SRGNN')
    _, model, batches = _evaluate_fixture(n_batches=2)
    torch.manual_seed(0)
    events = []
    runner = train.TrainRunner('sample', model, batches[:1], batches, torch.device('cpu'), lr=args.lr, hooks=[events.append],
                               **common.eval_options(args))
    return runner, events


def test_launcher_eval_flags_reach_the_runner_and_leave_the_epoch_line_alone(monkeypatch, capsys):
    plain, ev0 = _runner(monkeypatch, [])
    assert plain.eval_method == 'topk' and plain.eval_cutoffs is None
    capsys.readouterr()
    plain.train(1)
    out0 = capsys.readouterr().out.splitlines()
    flagged, ev1 = _runner(monkeypatch, ['--eval-method', 'rank', '--eval-cutoffs', '5,10,20'])
    assert flagged.eval_method == 'rank' and flagged.eval_cutoffs == (5, 10, 20)
    capsys.readouterr()
    flagged.train(1)
    out1 = capsys.readouterr().out.splitlines()
    line0 = [l for l in out0 if l.startswith('Epoch 0:')]
    line1 = [l for l in out1 if l.startswith('Epoch 0:')]
    # same weights, same data: the reference's epoch line is byte-identical with and without the options ...
    assert len(line0) == 1 and line0 == line1, (line0, line1)
    assert line0[0].startswith('Epoch 0: MRR = ') and ', Hit = ' in line0[0] and line0[0].endswith('%')
    assert not any('@' in l for l in out0)
    # ... and the extra cutoffs follow it on a line of their own and ride in the epoch event
    extra = out1[out1.index(line1[0]) + 1]
    assert all(('%s@%d = ' % (n, k)) in extra for n in ('HR', 'MRR', 'NDCG') for k in (5, 10, 20)), extra
    e0 = [e for e in ev0 if e['kind'] == 'epoch'][0]
    e1 = [e for e in ev1 if e['kind'] == 'epoch'][0]
    assert set(e0) == {'kind', 'epoch', 'mrr', 'hit'}
    assert set(e1['metrics']) == {'%s@%d' % (n, k) for n in ('hit', 'mrr', 'ndcg') for k in (5, 10, 20)}
    assert abs(e1['mrr'] - e0['mrr']) < 1e-7 and e1['hit'] == e0['hit'] == e1['metrics']['hit@20']
