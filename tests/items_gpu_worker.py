"""Worker side of tests/test_items_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/select_gpu_worker.py, whose exact-input case and table-only model it shares).  Every rank cuts its row shard out of
the same table and scores the same candidates through dist.VocabParallel.score_items - with the same sessions on every
rank, and with its own slice of them."""
import os

import torch
import torch.distributed as dist

from select_gpu_worker import sharded_case, table_only_model
from util import pkg

M = 70


def candidates():
    """int64 [B, M]: ids of both shards in every list, among them -1 slots, a repeated id, ids 0 and V - 1 and two of the
    session's listed ids - the same on every rank and in the parent"""
    sr, E, _, listed = sharded_case()
    B, V = sr.shape[0], E.shape[0]
    g = torch.Generator().manual_seed(13)
    items = torch.randint(0, V, (B, M), generator=g)
    items[:, 0], items[:, 1], items[:, 2] = 0, V - 1, -1
    items[:, 3] = items[:, 4]
    items[:, 5:7] = listed[:, :2]
    items[torch.arange(B), torch.randint(7, M, (B,), generator=g)] = -1
    return items


def run_rank(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device('cuda:0')
        D = pkg('dist')
        sr, E, cs, listed = sharded_case()
        model = table_only_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        cs_loc = torch.ones(vp.per)
        cs_loc[:vp.n_live] = cs[vp.lo:vp.hi]
        sr, cs_loc, listed, items = sr.to(dev), cs_loc.to(dev), listed.to(dev), candidates().to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        with torch.no_grad():
            out['replicated'] = vp.score_items([sr], table, cs_loc, items).cpu()
            out['routed'] = model._run(pkg('serving').Query([sr], cs_loc, None, None, None), 'score_items', items).cpu()    # the model's own route
            out['replicated_shared'] = vp.score_items([sr], table, cs_loc, items[0]).cpu()
            out['replicated_drop'] = vp.score_items([sr], table, cs_loc, items, listed=listed, drop_listed=True).cpu()
            out['data_parallel_drop'] = vp.score_items([sr[mine]], table, cs_loc, items[mine], listed=listed[mine, :4 + rank],
                                                       drop_listed=True, data_parallel=True).cpu()
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
