"""Worker side of tests/test_item_bias_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/select_gpu_worker.py, whose exact-input case and table-only model it shares, and tests/items_gpu_worker.py, whose
candidates it shares).  Every rank cuts its row shard out of the same table, takes its columns of the same GLOBAL bias and
runs dist.VocabParallel.select and .score_items with it - with the same sessions on every rank, and with its own slice of
them (the group ids are then gathered with the sessions)."""
import os

import torch
import torch.distributed as dist

from item_bias_oracle import exact_bias
from items_gpu_worker import candidates
from select_gpu_worker import K, sharded_case, table_only_model
from util import pkg

G = 3


def sharded_bias():
    """(bias fp32 [G, V] over global ids, group int64 [B]): multiples of 1/8, about 30 % -inf, -inf on one whole chunk and
    across the boundary between the two shards (rows 2400 .. 2599) - the same on every rank and in the parent"""
    sr, E, _, _ = sharded_case()
    bias = exact_bias(E.shape[0], G, seed=3, off_ranges=((128, 256), (2400, 2600)))
    return bias, torch.arange(sr.shape[0]) % G


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
        bias, group = sharded_bias()
        model = table_only_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        cs_loc = torch.ones(vp.per)
        cs_loc[:vp.n_live] = cs[vp.lo:vp.hi]
        sr, cs_loc, listed, items = sr.to(dev), cs_loc.to(dev), listed.to(dev), candidates().to(dev)
        bias, group = bias.to(dev), group.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        cpu = lambda r: [t.cpu() for t in r] if isinstance(r, (tuple, list)) else r.cpu()
        with torch.no_grad():
            out['select'] = cpu(vp.select([sr], table, cs_loc, K, bias=bias, group=group))
            out['select_shared'] = cpu(vp.select([sr], table, cs_loc, K, bias=bias[1]))
            out['select_routed'] = cpu(model._run(pkg('serving').Query([sr], cs_loc, None, None, None, False, dict(bias=bias, group=group)),
                                                  'select', K))
            out['select_drop'] = cpu(vp.select([sr], table, cs_loc, K, listed=listed, drop_listed=True, bias=bias, group=group))
            out['select_dp_drop'] = cpu(vp.select([sr[mine]], table, cs_loc, K, listed=listed[mine, :4 + rank], drop_listed=True,
                                                  data_parallel=True, bias=bias, group=group[mine]))
            out['items'] = cpu(vp.score_items([sr], table, cs_loc, items, bias=bias, group=group))
            out['items_shared'] = cpu(vp.score_items([sr], table, cs_loc, items[0], bias=bias[1]))
            out['items_routed'] = cpu(model._run(pkg('serving').Query([sr], cs_loc, None, None, None, False, dict(bias=bias, group=group)),
                                                 'score_items', items))
            out['items_drop'] = cpu(vp.score_items([sr], table, cs_loc, items, listed=listed, drop_listed=True, bias=bias, group=group))
            out['items_dp_drop'] = cpu(vp.score_items([sr[mine]], table, cs_loc, items[mine], listed=listed[mine, :4 + rank],
                                                      drop_listed=True, data_parallel=True, bias=bias, group=group[mine]))
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
