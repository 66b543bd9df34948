"""Worker side of tests/test_cap_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/norm_gpu_worker.py, whose identity model and exact-input case it shares).  Every rank cuts its row shard out of the same
table and serves capped lists through model.recommend_capped over the sharded table - replicated and data-parallel, from the
128-item pool, an explicit pool beyond 128 and the 4096-item fallback, the latter also data-parallel under a rule that sends
only ONE rank's sessions there - and through dist.VocabParallel.cap_select itself."""
import os

import torch
import torch.distributed as dist

from norm_gpu_worker import identity_model
from select_gpu_worker import sharded_case
from util import pkg

K = 30


def case_rule(V):
    """(category [V], caps [40]): forty categories over the global ids, at most two of each (the first never shown); every
    tenth item has none"""
    category = torch.arange(V) % 40
    category[::10] = -1
    caps = torch.full((40,), 2)
    caps[1] = 0
    return category, caps


def tight_rule(V):
    """five categories, two of each: ten items whatever the pool - the 128-item pool is incomplete and the fallback runs"""
    return torch.arange(V) % 5, torch.full((5,), 2)


def split_rule(pool_ids, V, b=16):
    """(category [V], caps [1]) that binds for ONE rank's sessions only: the 128-item pool of session b (the first session of
    rank 1 of two) shares category 0 with cap 2 and no other item has a category - session b keeps 2 of its pool, the
    sessions of rank 0 find their K in theirs"""
    category = torch.full((V,), -1)
    category[pool_ids[b, :128].long()] = 0
    return category, torch.tensor([2])


def run_rank(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device('cuda:0')
        D, ops = pkg('dist'), pkg('ops')
        sr, E, _, _ = sharded_case()
        V = E.shape[0]
        model = identity_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        sr = sr.to(dev)
        rule = ops.cap_rule(V, *case_rule(V), device=dev)
        tight = ops.cap_rule(V, *tight_rule(V), device=dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        vp.eval_data_parallel = False
        pv, pi = model.recommend(sr, k=128)
        out['pool'] = [pv.cpu(), pi.cpu()]
        out['capped'] = [t.cpu() for t in model.recommend_capped(sr, k=K, rule=rule)]
        out['capped_many'] = [t.cpu() for t in model.recommend_capped(sr, k=K, rule=rule, pool=300)]
        out['capped_fallback'] = [t.cpu() for t in model.recommend_capped(sr, k=20, rule=tight, return_complete=True)]
        with torch.no_grad():
            out['route'] = [t.cpu() for t in vp.cap_select(pi, pv, rule, K)]
            out['route_dp'] = [t.cpu() for t in vp.cap_select(pi[mine], pv[mine], rule, K, data_parallel=True)]
        vp.eval_data_parallel = True
        sent = D.STATS['count']
        out['capped_dp'] = [t.cpu() for t in model.recommend_capped(sr[mine], k=K, rule=rule)]
        out['collectives_dp'] = D.STATS['count'] - sent
        # only rank 1 holds a session whose 128-item pool runs short: both ranks must go on to the 4096-item pool together
        split = ops.cap_rule(V, *split_rule(out['pool'][1], V), device=dev)
        sent = D.STATS['count']
        out['capped_dp_split'] = [t.cpu() for t in model.recommend_capped(sr[mine], k=K, rule=split, return_complete=True)]
        out['collectives_dp_split'] = D.STATS['count'] - sent
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
