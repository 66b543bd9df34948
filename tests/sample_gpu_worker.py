"""Worker side of tests/test_sample_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/select_gpu_worker.py, whose inputs it reuses).  Every rank cuts its row shard out of the same table and draws through
dist.VocabParallel.sample - with the same sessions on every rank, and with its own slice of them (default keys: the global
row index; given keys: gathered with the sessions)."""
import os

import torch
import torch.distributed as dist

from select_gpu_worker import sharded_case, table_only_model
from util import pkg

K, SEED, T = 50, 9, 0.7


def session_keys(B):
    """caller-given keys that are not the row index (a negative one among them)"""
    return (torch.arange(B, dtype=torch.int64) * 7919 - 5) % 100003 - 17


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
        sr, cs_loc, listed = sr.to(dev), cs_loc.to(dev), listed.to(dev)
        B = sr.shape[0]
        n = B // world
        mine = slice(rank * n, (rank + 1) * n)
        q = session_keys(B).to(dev)
        kw = dict(temperature=T, seed=SEED)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        with torch.no_grad():
            out['replicated'] = [t.cpu() for t in vp.sample([sr], table, cs_loc, K, **kw)]
            out['replicated_drop_keys'] = [t.cpu() for t in vp.sample([sr], table, cs_loc, K, listed=listed, drop_listed=True,
                                                                      session_keys=q, **kw)]
            out['data_parallel'] = [t.cpu() for t in vp.sample([sr[mine]], table, cs_loc, K, data_parallel=True, **kw)]
            out['data_parallel_drop_keys'] = [t.cpu() for t in vp.sample([sr[mine]], table, cs_loc, K, listed=listed[mine, :4 + rank],
                                                                         drop_listed=True, data_parallel=True,
                                                                         session_keys=q[mine], **kw)]
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
