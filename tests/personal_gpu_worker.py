"""Worker side of tests/test_personal_gpu.py's sharded case: W processes, one per rank, all on cuda:0, talking over gloo (as
tests/cap_gpu_worker.py, whose identity model and exact-input case it shares).  Every rank cuts its row shard out of the same
table and serves personalised lists through model.recommend_personal over the sharded table - replicated and data-parallel,
from the pool of k + M items, an explicit pool beyond 128 and both stages of the pool policy, the latter data-parallel under
lists that send only ONE rank's sessions to the second stage - and through dist.VocabParallel.personal_merge itself."""
import os

import torch
import torch.distributed as dist

import personal_oracle as po
from norm_gpu_worker import identity_model
from select_gpu_worker import sharded_case
from util import pkg

K = 30


def case_lists(pool_ids, V):
    """(items int64 [B, 60], bias fp32 [B, 60]): per session 25 of the first 40 items of its 128-item pool and 30 items from
    outside it, shuffled, five padding slots; biases from the oracle's set"""
    g = torch.Generator().manual_seed(21)
    B = pool_ids.shape[0]
    items = torch.full((B, 60), -1, dtype=torch.int64)
    for b in range(B):
        inside = pool_ids[b, torch.randperm(40, generator=g)[:25]].long()
        rest = torch.ones(V, dtype=torch.bool)
        rest[pool_ids[b].long().clamp(min=0)] = False
        rest = rest.nonzero().flatten()
        outside = rest[torch.randperm(rest.numel(), generator=g)[:30]]
        items[b, torch.randperm(60, generator=g)[:55]] = torch.cat([inside, outside])
    bias = torch.tensor(po.BIASES)[torch.randint(0, len(po.BIASES), (B, 60), generator=g)]
    return items, bias


def split_lists(pool_ids, world):
    """items int64 [B, 110] that send ONE rank's sessions to the second stage: the sessions of the last rank hide the first
    110 items of their 128-item pool (18 survivors for a list of 30), the others the first five of theirs"""
    B = pool_ids.shape[0]
    n = B // world
    items = torch.full((B, 110), -1, dtype=torch.int64)
    items[:B - n, :5] = pool_ids[:B - n, :5].long()
    items[B - n:] = pool_ids[B - n:, :110].long()
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
        sr, E, _, _ = sharded_case()
        V = E.shape[0]
        model = identity_model(E).to(dev)
        vp = D.VocabParallel(model)
        table = model._table()
        sr = sr.to(dev)
        n = sr.shape[0] // world
        mine = slice(rank * n, (rank + 1) * n)
        out = dict(rank=rank, lo=vp.lo, hi=vp.hi, n_live=vp.n_live, rows=table.shape[0])
        vp.eval_data_parallel = False
        pv, pi = model.recommend(sr, k=128)
        out['pool'] = [pv.cpu(), pi.cpu()]
        items, bias = case_lists(out['pool'][1], V)
        items, bias = items.to(dev), bias.to(dev)
        M = items.shape[1]
        pv, pi = model.recommend(sr, k=K + M)
        out['pool_kM'] = [pv.cpu(), pi.cpu()]
        base = model.score_items(sr, items=items)
        out['base'] = base.cpu()
        out['personal'] = [t.cpu() for t in model.recommend_personal(sr, k=K, personal_items=items, personal_bias=bias)]
        out['personal_hide'] = [t.cpu() for t in model.recommend_personal(sr, k=K, personal_items=items)]
        out['personal_many'] = [t.cpu() for t in model.recommend_personal(sr, k=K, personal_items=items, personal_bias=bias, pool=300)]
        it32 = items.to(torch.int32)
        with torch.no_grad():
            out['route'] = [t.cpu() for t in vp.personal_merge(pi, pv, it32, base, bias, K)]
            out['route_dp'] = [t.cpu() for t in vp.personal_merge(pi[mine], pv[mine], it32[mine], base[mine], bias[mine], K,
                                                                  data_parallel=True)]
        vp.eval_data_parallel = True
        sent = D.STATS['count']
        out['personal_dp'] = [t.cpu() for t in model.recommend_personal(sr[mine], k=K, personal_items=items[mine],
                                                                        personal_bias=bias[mine])]
        out['collectives_dp'] = D.STATS['count'] - sent
        # only the last rank holds sessions whose 128-item pool runs short: all ranks must go on to the larger pool together
        split = split_lists(out['pool'][1], world).to(dev)
        sent = D.STATS['count']
        out['personal_dp_split'] = [t.cpu() for t in model.recommend_personal(sr[mine], k=K, personal_items=split[mine],
                                                                              return_complete=True)]
        out['collectives_dp_split'] = D.STATS['count'] - sent
        torch.cuda.synchronize()
        torch.save(out, os.path.join(outdir, 'rank%d.pt' % rank))
        dist.barrier()
    finally:
        dist.destroy_process_group()
