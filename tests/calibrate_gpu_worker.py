"""Worker side of tests/test_calibrate_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/cap_gpu_worker.py, whose identity model and exact-input case it shares).  Every rank cuts its row shard out of the same
table and serves calibrated slates through model.recommend_calibrated over the sharded table - fed as replicated sessions
and as data-parallel ones - and through dist.VocabParallel.calibrate itself."""
import os

import torch
import torch.distributed as dist

from norm_gpu_worker import identity_model
from select_gpu_worker import sharded_case
from util import pkg

K, POOL, WEIGHT = 20, 100, 0.7


def case_target(B, V):
    """(category int32 [V] over the global ids: 23 categories, every ninth item none; tcat [B, 5], tw [B, 5]: a sparse target
    per session with an empty pair and a duplicate)"""
    category = (torch.arange(V) * 31 % 23).to(torch.int32)
    category[::9] = -1
    g = torch.Generator().manual_seed(17)
    tcat = torch.randint(0, 23, (B, 5), generator=g)
    tcat[:, 3] = tcat[:, 0]
    tcat[:, 4] = -1
    return category, tcat, torch.rand(B, 5, generator=g) + 0.1


def run_rank(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device('cuda:0')
        D = pkg('dist')
        sr, E, _, _ = sharded_case()
        V = E.shape[0]
        model = identity_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        sr = sr.to(dev)
        category, tcat, tw = [t.to(dev) for t in case_target(sr.shape[0], V)]
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        kw = dict(k=K, weight=WEIGHT, item_category=category, pool=POOL, return_kl=True)
        vp.eval_data_parallel = False
        pv, pi = model.recommend(sr, k=POOL)
        out['pool'] = [pv.cpu(), pi.cpu()]
        out['calibrated'] = [t.cpu() for t in model.recommend_calibrated(sr, target=(tcat, tw), **kw)]
        with torch.no_grad():
            out['route'] = [t.cpu() for t in vp.calibrate(pi, pv, category, K, WEIGHT, tcat.to(torch.int32), tw, 0.01)]
        vp.eval_data_parallel = True
        sent = D.STATS['count']
        out['calibrated_dp'] = [t.cpu() for t in model.recommend_calibrated(sr[mine], target=(tcat[mine], tw[mine]), **kw)]
        out['collectives_dp'] = D.STATS['count'] - sent
        sent = D.STATS['count']
        model.recommend(sr[mine], k=POOL)
        out['collectives_pool_dp'] = D.STATS['count'] - sent
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
