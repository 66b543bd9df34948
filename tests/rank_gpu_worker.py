"""Worker side of tests/test_rank_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/dist_gpu_worker.py, whose case factory this reuses).  Every rank cuts its row shard out of the same weights and
evaluates model.target_rank over the sharded table - once with the same sessions on every rank, once with its own slice."""
import os

import torch
import torch.distributed as dist

from dist_gpu_worker import make_case, rank_slice
from util import pkg


def run_rank(rank, world, port, case, outdir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device('cuda:0')
        D = pkg('dist')
        build, collate, samples, V = make_case(case)
        model = build().to(dev)
        vp = D.VocabParallel(model)
        model.eval()
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live)

        def ranks(part, data_parallel):
            inputs, labels = collate(None)(part)
            vp.eval_data_parallel = data_parallel
            return model.target_rank(*[x.to(dev) for x in inputs], labels=labels.to(dev)).cpu()
        out['replicated'] = ranks(samples, False)
        out['data_parallel'] = ranks(rank_slice(samples, world, rank, False)[0], True)
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
