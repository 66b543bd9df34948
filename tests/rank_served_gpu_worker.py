"""Worker side of tests/test_rank_served_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/norm_gpu_worker.py, whose exact-input case, table-only model and global bias it shares).  Every rank cuts its row shard
out of the same table, takes its columns of the same GLOBAL bias and runs dist.VocabParallel.ahead - with the same sessions
on every rank, and with its own slice of them - and model.served_rank over the sharded table."""
import os

import torch
import torch.distributed as dist

from item_bias_gpu_worker import sharded_bias
from select_gpu_worker import sharded_case, table_only_model
from util import pkg

TOP_K = 40


def sharded_labels():
    """int64 [B]: labels on both shards, one session without a label, one whose label its own list holds"""
    sr, E, _, listed = sharded_case()
    g = torch.Generator().manual_seed(23)
    labels = torch.randint(0, E.shape[0], (sr.shape[0],), generator=g)
    labels[0], labels[1], labels[2], labels[3] = -1, listed[1, 0], 3, E.shape[0] - 1
    return labels


def seen_model(E, listed):
    """table_only_model whose session vectors are its input, whose own items are the rows of `listed` (exclude_seen) and
    whose soft-max normaliser is taken as 0: the served value is the raw logit plus the bias, the same bits on one device and
    on any number of shards - what is compared is the route (items, cutoff and count over the shards), not the statistics
    pass"""
    model = table_only_model(E)
    cls = type(model)
    cls.session_repr = lambda self, sr: sr
    cls._session_items = staticmethod(lambda sr: listed.to(sr.device)[:sr.shape[0]].to(torch.int32))
    cls._lse = lambda self, sr, cs, inv_scale, st, labels=None: torch.zeros(sr.shape[0], device=sr.device)
    return model


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
        labels = sharded_labels()
        model = seen_model(E, listed).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        cs_loc = torch.ones(vp.per)
        cs_loc[:vp.n_live] = cs[vp.lo:vp.hi]
        sr, cs_loc, listed, labels = sr.to(dev), cs_loc.to(dev), listed.to(dev), labels.to(dev)
        bias, group = bias.to(dev), group.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        kw = dict(listed=listed, drop_listed=True, bias=bias, group=group)
        with torch.no_grad():
            target = vp.score_items([sr], table, cs_loc, labels[:, None], **kw)[:, 0]
            floor = vp.cutoff([sr], table, cs_loc, top_k=TOP_K, **kw)[0]
            out['target'], out['floor'] = target.cpu(), floor.cpu()
            out['ahead'] = vp.ahead([sr], table, cs_loc, labels, target, **kw).cpu()
            out['ahead_floor'] = vp.ahead([sr], table, cs_loc, labels, target, floor=floor, **kw).cpu()
            out['ahead_routed'] = model._run(pkg('serving').Query([sr], cs_loc, None, None, listed, True, dict(bias=bias, group=group)),
                                            'ahead', labels, target).cpu()
            out['ahead_dp'] = vp.ahead([sr[mine]], table, cs_loc, labels[mine], target[mine], listed=listed[mine, :4 + rank],
                                       drop_listed=True, data_parallel=True, bias=bias, group=group[mine], floor=floor[mine]).cpu()
        out['served'] = model.served_rank(sr, labels=labels, exclude_seen=True, item_bias=bias, item_group=group).cpu()
        out['served_top_k'] = model.served_rank(sr, labels=labels, exclude_seen=True, item_bias=bias, item_group=group,
                                                top_k=TOP_K).cpu()
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
