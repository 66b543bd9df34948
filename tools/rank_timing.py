"""Timing of the full-catalog target-rank evaluation against the top-K evaluation it stands beside, at the benchmarked
shape (B 512, V 37 484, d 256): median of N device-event timed calls after warm-up, the two sides of a comparison
alternating call by call.
  (i)  ops.score_rank (one soft-max, C = 1)             vs  ops.score_topk(k = 20)
  (ii) MSGIFSR order 3 extra + fusion: model.target_rank vs  model.topk (forward(): one (B, V) matrix per order + torch.topk)
Prints one JSON line per comparison; `flops_share` is 2 B V d C over the call time over the fp32 MFMA peak (157.3 TFLOP/s) -
the whole call (target, count and fix-up launches), so a lower bound of the count kernel's own share.
usage (GPU box; every GPU step under its own time limit, a later step only after the earlier one ended well):
  timeout -k 10 300 python tools/rank_timing.py --out profiles/rank_timing.jsonl && \
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o rank -- python tools/rank_timing.py --only kernel
(the plain run gives the medians, the traced run of its own the per-kernel times; options: --calls N >= 30, --only kernel|model)"""
import argparse
import importlib
import json
import os
import statistics
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import torch

PEAK_FP32_MFMA = 157.3e12


def timed(fns, calls, warmup=5):
    """fns: {name: callable}; -> {name: [us per call]} with the callables alternating inside every round"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(calls):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3)
    return out


def summary(us):
    s = sorted(us)
    return dict(median_us=round(statistics.median(s), 1), p10_us=round(s[len(s) // 10], 1), p90_us=round(s[(9 * len(s)) // 10], 1))


def synth_samples(n, V, seed):
    """n prefix samples of the benchmark's synthetic sessions (bench.synth_sessions)"""
    import bench
    sessions = bench.synth_sessions(n, V, 6.2, 20, np.random.default_rng(seed))
    return [(s[:e], int(s[e])) for s in sessions for e in range(1, len(s))][:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--only', choices=['kernel', 'model'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'rank_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    sp = importlib.import_module('sessionrec-pytorch_amd')
    col = importlib.import_module('sessionrec-pytorch_amd.collate')
    dev = torch.device('cuda:0')
    B, V, d = 512, 37484, 256
    lines = []
    if args.only in (None, 'kernel'):
        torch.manual_seed(1)
        sr = torch.randn(B, d, device=dev) * 0.3
        E = torch.randn(V, d, device=dev) * 0.2
        cs = torch.rand(V, device=dev) + 0.5
        labels = torch.randint(0, V, (B,), device=dev, dtype=torch.int32)
        t = timed({'score_rank': lambda: ops.score_rank(sr, E, cs, labels), 'score_topk': lambda: ops.score_topk(sr, E, cs, 20)},
                  args.calls)
        r = dict(what='kernel', B=B, V=V, d=d, C=1, calls=args.calls, score_rank=summary(t['score_rank']),
                 score_topk_k20=summary(t['score_topk']))
        r['flops_share'] = round(2.0 * B * V * d / (r['score_rank']['median_us'] * 1e-6) / PEAK_FP32_MFMA, 3)
        # the two answers agree: the label is in the top 20 exactly where fewer than 20 items are ahead of it
        rank = ops.score_rank(sr, E, cs, labels)[0]
        top = ops.score_topk(sr, E, cs, 20)[1]
        r['agree'] = bool(torch.equal((top == labels[:, None]).any(1), (rank < 20)))
        lines.append(r)
    if args.only in (None, 'model'):
        torch.manual_seed(2)
        K = 3
        model = sp.MSGIFSR(V, 'synthetic', d, 1, dropout=0.0, order=K, extra=True, fusion=True).to(dev).eval()
        (mg,), labels = col.collate_fn_factory_ccs((col.seq_to_ccs_graph,), K)(synth_samples(B, V, 123))
        mg, labels = mg.to(dev), labels.to(dev)
        t = timed({'target_rank': lambda: model.target_rank(mg, labels=labels), 'topk': lambda: model.topk(mg, k=20)}, args.calls)
        r = dict(what='msgifsr order 3 extra+fusion', B=B, V=V, d=d, C=K, calls=args.calls, target_rank=summary(t['target_rank']),
                 topk_k20_materialised=summary(t['topk']))
        rank = model.target_rank(mg, labels=labels)
        top = model.topk(mg, k=20)[1]
        r['agree_share'] = round(float(((top == labels[:, None]).any(1) == (rank < 20)).float().mean()), 4)
        lines.append(r)
    text = '\n'.join(json.dumps(r) for r in lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
