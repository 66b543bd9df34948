"""Worker side of tests/test_select_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/rank_gpu_worker.py).  Every rank cuts its row shard out of the same exact-input table and selects through
dist.VocabParallel.select - with the same sessions on every rank, and with its own slice of them."""
import os

import torch
import torch.distributed as dist

from select_oracle import exact_case
from util import pkg

SHAPE = (32, 4999, 96)       # sessions (two equal slices), catalog rows (odd: the last shard ends in a padding row), width
K = 50


def sharded_case():
    """(session vectors, table, column scale, listed ids [B, 6] with empty slots) - the same on every rank and in the parent"""
    B, V, d = SHAPE
    sr, E, cs = exact_case(B, V, d)
    g = torch.Generator().manual_seed(11)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    listed[:, 5] = -1
    listed[:, 0] = torch.arange(B) % 2 * 2500 + 3          # ids on both shards, among them the duplicated rows' scores
    return sr, E, cs, listed


def table_only_model(E):
    """the least a VocabParallel attaches to: the scoring mixin over an item table"""
    class TableOnly(pkg('srgnn')._ScoringMixin, torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.embedding = torch.nn.Embedding.from_pretrained(E.clone(), freeze=False)
    return TableOnly()


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
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        with torch.no_grad():
            out['replicated'] = [t.cpu() for t in vp.select([sr], table, cs_loc, K)]
            out['replicated_drop'] = [t.cpu() for t in vp.select([sr], table, cs_loc, K, listed=listed, drop_listed=True)]
            out['data_parallel_drop'] = [t.cpu() for t in vp.select([sr[mine]], table, cs_loc, K, listed=listed[mine, :4 + rank],
                                                                    drop_listed=True, data_parallel=True)]
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
