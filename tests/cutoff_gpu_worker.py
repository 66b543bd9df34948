"""Worker side of tests/test_cutoff_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/sample_gpu_worker.py, whose inputs and keys it reuses).  Every rank cuts its row shard out of the same table, finds the
cutoff through dist.VocabParallel.cutoff and draws inside it through dist.VocabParallel.sample - with the same sessions on
every rank, and with its own slice of them."""
import os

import torch
import torch.distributed as dist

from sample_gpu_worker import K, SEED, T, session_keys
from select_gpu_worker import sharded_case, table_only_model
from util import pkg

CRIT = dict(top_k=300, top_p=0.8, min_p=0.01, temperature=T)
NARROW = dict(top_k=30, temperature=T)          # fewer kept items than K: the lists end in (-inf, -1) slots
SMALL_CRITS = (dict(top_k=30, top_p=0.8, min_p=0.01), dict(top_k=7), dict(top_p=0.6), dict(min_p=0.2), dict())
SMALL = (34, 60, 32)                            # (B, V, d) of a table whose rows all live on rank 0 (shards are whole 64-row
#                                                 tiles): rank 1 has no live row


def small_case():
    from select_oracle import exact_case
    sr, E, cs = exact_case(*SMALL)
    return sr / 8, E, cs


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

        def both(name, srs, crit, **more):
            """the cutoff, and the draw inside it"""
            dp = {k: v for k, v in more.items() if k in ('listed', 'drop_listed', 'data_parallel')}
            cut = vp.cutoff(srs, table, cs_loc, **crit, **dp)
            draw = vp.sample(srs, table, cs_loc, K, floor=cut[0], **kw, **more)
            out[name] = [t.cpu() for t in cut] + [t.cpu() for t in draw]
        with torch.no_grad():
            both('replicated', [sr], CRIT)
            both('replicated_narrow', [sr], NARROW)
            both('replicated_drop_keys', [sr], CRIT, listed=listed, drop_listed=True, session_keys=q)
            both('data_parallel', [sr[mine]], CRIT, data_parallel=True)
            both('data_parallel_drop_keys', [sr[mine]], NARROW, listed=listed[mine, :4 + rank], drop_listed=True,
                 data_parallel=True, session_keys=q[mine])
            # a table of 60 rows: the last rank owns none of them - it launches no pass and joins every collective
            sr2, E2, cs2 = small_case()
            model2 = table_only_model(E2).to(dev)
            vp2 = D.VocabParallel(model2)
            out['small_n_live'] = vp2.n_live
            cs2_loc = torch.ones(vp2.per)
            cs2_loc[:vp2.n_live] = cs2[vp2.lo:vp2.hi]
            sr2, cs2_loc = sr2.to(dev), cs2_loc.to(dev)
            n2 = sr2.shape[0] // world
            for name, srs, dp in (('small', [sr2], {}), ('small_dp', [sr2[rank * n2:(rank + 1) * n2]], dict(data_parallel=True))):
                for i, crit in enumerate(SMALL_CRITS):
                    cut = vp2.cutoff(srs, model2._table(), cs2_loc, temperature=T, **crit, **dp)
                    draw = vp2.sample(srs, model2._table(), cs2_loc, 20, floor=cut[0], **kw, **dp)
                    out[name, i] = [t.cpu() for t in cut] + [t.cpu() for t in draw]
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
