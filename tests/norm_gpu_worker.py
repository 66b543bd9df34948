"""Worker side of tests/test_norm_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/item_bias_gpu_worker.py, whose exact-input case, table-only model and global bias it shares).  Every rank cuts its row
shard out of the same table, takes its columns of the same GLOBAL bias and runs dist.VocabParallel.norm - with the same
sessions on every rank, and with its own slice of them - and model.recommend(renormalize=True) over the sharded table."""
import os

import torch
import torch.distributed as dist

from item_bias_gpu_worker import sharded_bias
from select_gpu_worker import K, sharded_case, table_only_model
from util import pkg


def identity_model(E):
    """table_only_model whose session vectors are its input: the least model.recommend() runs on"""
    model = table_only_model(E)
    type(model).session_repr = lambda self, sr: sr
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
        model = identity_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        cs_loc = torch.ones(vp.per)
        cs_loc[:vp.n_live] = cs[vp.lo:vp.hi]
        sr, cs_loc, listed = sr.to(dev), cs_loc.to(dev), listed.to(dev)
        bias, group = bias.to(dev), group.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        with torch.no_grad():
            out['norm'] = vp.norm([sr], table, cs_loc, bias=bias, group=group).cpu()
            out['norm_plain'] = vp.norm([sr], table, cs_loc).cpu()
            out['norm_routed'] = model._run(pkg('serving').Query([sr], cs_loc, None, None, None, False, dict(bias=bias, group=group)),
                                            'norm').cpu()
            out['norm_drop'] = vp.norm([sr], table, cs_loc, listed=listed, drop_listed=True, bias=bias, group=group).cpu()
            out['norm_dp'] = vp.norm([sr[mine]], table, cs_loc, data_parallel=True, bias=bias, group=group[mine]).cpu()
            out['norm_dp_drop'] = vp.norm([sr[mine]], table, cs_loc, listed=listed[mine, :4 + rank], drop_listed=True,
                                          data_parallel=True, bias=bias, group=group[mine]).cpu()
        out['recommend'] = [t.cpu() for t in model.recommend(sr, k=K, item_bias=bias, item_group=group, renormalize=True)]
        out['log_mass'] = model.log_mass(sr, item_bias=bias, item_group=group).cpu()
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
