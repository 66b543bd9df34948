"""Worker side of tests/test_rank_many_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/rank_served_gpu_worker.py, whose exact-input case, labels and seen_model it shares).  Every rank cuts its row shard out
of the same table, takes its columns of the same GLOBAL bias and runs dist.VocabParallel.ahead_many - with the same sessions on
every rank, and with its own slice of them - and model.rank_items over the sharded table."""
import os

import torch
import torch.distributed as dist

from item_bias_gpu_worker import sharded_bias
from rank_served_gpu_worker import TOP_K, seen_model, sharded_labels
from select_gpu_worker import sharded_case
from util import pkg

M = 6


def sharded_items():
    """int64 [B, M]: column 0 = sharded_labels() (one -1, one its own session lists, the first and the last row of the table),
    the rest random distinct ids on both shards, one more empty slot"""
    _, E, _, _ = sharded_case()
    labels = sharded_labels()
    g = torch.Generator().manual_seed(29)
    items = torch.stack([torch.randperm(E.shape[0], generator=g)[:M] for _ in range(labels.numel())])
    items[:, 1:] = torch.where(items[:, 1:] == labels[:, None], torch.full_like(items[:, 1:], -1), items[:, 1:])
    items[:, 0] = labels
    items[4, 2] = -1
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
        bias, group = sharded_bias()
        items = sharded_items()
        model = seen_model(E, listed).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        cs_loc = torch.ones(vp.per)
        cs_loc[:vp.n_live] = cs[vp.lo:vp.hi]
        sr, cs_loc, listed, items = sr.to(dev), cs_loc.to(dev), listed.to(dev), items.to(dev)
        bias, group = bias.to(dev), group.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        kw = dict(listed=listed, drop_listed=True, bias=bias, group=group)
        with torch.no_grad():
            target = vp.score_items([sr], table, cs_loc, items, **kw)
            floor = vp.cutoff([sr], table, cs_loc, top_k=TOP_K, **kw)[0]
            out['target'], out['floor'] = target.cpu(), floor.cpu()
            out['ahead'] = vp.ahead_many([sr], table, cs_loc, items, target, **kw).cpu()
            out['ahead_floor'] = vp.ahead_many([sr], table, cs_loc, items, target, floor=floor, **kw).cpu()
            out['ahead_routed'] = model._run(pkg('serving').Query([sr], cs_loc, None, None, listed, True, dict(bias=bias, group=group)),
                                            'ahead_many', items, target).cpu()
            out['ahead_dp'] = vp.ahead_many([sr[mine]], table, cs_loc, items[mine], target[mine], listed=listed[mine, :4 + rank],
                                            drop_listed=True, data_parallel=True, bias=bias, group=group[mine],
                                            floor=floor[mine]).cpu()
        out['ranks'] = model.rank_items(sr, items=items, exclude_seen=True, item_bias=bias, item_group=group).cpu()
        out['ranks_top_k'] = model.rank_items(sr, items=items, exclude_seen=True, item_bias=bias, item_group=group, top_k=TOP_K).cpu()
        vp.eval_data_parallel = True        # every rank feeds its own slice of the batch (no exclude_seen: seen_model's lists are the batch's)
        out['ranks_dp'] = model.rank_items(sr[mine], items=items[mine], item_bias=bias, item_group=group[mine], top_k=TOP_K).cpu()
        vp.eval_data_parallel = False
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
