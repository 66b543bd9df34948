"""Worker side of tests/test_diversify_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/select_gpu_worker.py).  Every rank cuts its row shard out of the same table, takes the pool through
dist.VocabParallel.select and re-ranks it through dist.VocabParallel.diversify - with the same sessions on every rank, and
with its own slice of them."""
import os

import torch
import torch.distributed as dist

from select_gpu_worker import table_only_model
from util import pkg

SHAPE = (32, 4999, 96)       # sessions (two equal slices), catalog rows (odd: the last shard ends in a padding row), width
POOL, K, THETA = 40, 12, 0.75


def sharded_case():
    """(session vectors, table): a catalogue of near-duplicates around 300 directions - the same on every rank and in the parent"""
    B, V, d = SHAPE
    g = torch.Generator().manual_seed(23)
    sr = torch.randn(B, d, generator=g) * 0.3
    E = (torch.randn(300, d, generator=g)[torch.randint(0, 300, (V,), generator=g)] + 0.3 * torch.randn(V, d, generator=g)) * 0.2
    return sr, E


def run_rank(rank, world, port, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device('cuda:0')
        D = pkg('dist')
        sr, E = sharded_case()
        model = table_only_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        sr = sr.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        with torch.no_grad():
            val, ids = vp.select([sr], table, None, POOL)
            out['pool'] = [val.cpu(), ids.cpu()]
            out['replicated'] = [t.cpu() for t in vp.diversify(table, ids, val, K, THETA)]
            val, ids = vp.select([sr[mine]], table, None, POOL, data_parallel=True)
            out['data_parallel'] = [t.cpu() for t in vp.diversify(table, ids, val, K, THETA, data_parallel=True)]
            # the model-level route (the mixin's dispatch) over the shard
            vp.eval_data_parallel = False
            out['list_diversity'] = model.list_diversity(out['pool'][1][:, :K]).cpu()
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
