"""Timing of the per-item bias of the serving calls (csrc/recommend.hip, csrc/score_items.hip: ops.score_select /
ops.score_items with bias=, group=) beside the unbiased calls and beside what a user had before for the same job, at the
benchmarked shape (B 512, V 37 484, d 256): median of N device-event timed calls after warm-up, all rows alternating call by
call, p10 / p90 as the spread.
  select C = 1 K = 20 and C = 3 K = 100, each: no bias | zero bias [V] | half the catalogue -inf | [4, V] with random groups
  score_items M = 100 and M = 1000, C = 1: no bias | bias [V] with half the catalogue -inf | [4, V] with random groups
  before: score_logp(...) + bias, topk(20) for C = 1; the three-matrix mixture + bias, topk(100) for C = 3
  the model-level check of item_bias / item_group (serving.ServingMixin._item_bias: one pass over the bias, one device-to-host read)
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/item_bias_timing.py --out profiles/item_bias_timing.md"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'item_bias_timing needs the GPU: there is nothing to fall back to'
    sp = importlib.import_module('sessionrec-pytorch_amd')
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d, C, G = 512, 37484, 256, 3, 4
    torch.manual_seed(1)
    srs = torch.randn(C, B, d, device=dev) * 0.3
    E = torch.randn(V, d, device=dev) * 0.2
    cs = torch.rand(V, device=dev) + 0.5
    off_ex = -2.0 * torch.rand(C, B, device=dev)
    sr = srs[0].contiguous()
    ws = ops.CEWorkspace(B, V, d, dev)
    zero = torch.zeros(V, device=dev)
    half = ops.catalog_bias(V, deny=torch.randperm(V, device=dev)[:V // 2], device=dev)
    grouped = torch.randn(G, V, device=dev)
    grouped[torch.rand(G, V, device=dev) < 0.5] = float('-inf')
    group = torch.randint(0, G, (B,), device=dev, dtype=torch.int32)
    items = {M: torch.randint(0, V, (B, M), device=dev, dtype=torch.int32) for M in (100, 1000)}
    model = sp.SRGNN(V, 32, 1).to(dev).eval()            # (the check reads the catalogue size off the model's table only)

    def logp_topk():
        # one soft-max before this feature: the (B, V) log-probabilities, the bias added to them, torch.topk
        return (ops.score_logp(sr, E, cs, ws, 1.0) + half).topk(20)

    def mixture_topk():
        # forward() of a fusion model: one (B, V) log-prob matrix per order, their logsumexp, the bias, torch.topk
        s = torch.logsumexp(torch.stack([ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0)
        return (s + grouped[group.long()]).topk(100)
    fns = {}
    for name, a, k, off in (('select C=1 K=20', sr, 20, None), ('select C=3 K=100', srs, 100, off_ex)):
        fns[name + ', no bias'] = lambda a=a, k=k, off=off: ops.score_select(a, E, cs, k, off)
        fns[name + ', zero bias [V]'] = lambda a=a, k=k, off=off: ops.score_select(a, E, cs, k, off, bias=zero)
        fns[name + ', half the catalogue -inf'] = lambda a=a, k=k, off=off: ops.score_select(a, E, cs, k, off, bias=half)
        fns[name + ', bias [4, V], random groups'] = lambda a=a, k=k, off=off: ops.score_select(a, E, cs, k, off, bias=grouped, group=group)
    for M, it in items.items():
        fns['score_items C=1 M=%d, no bias' % M] = lambda it=it: ops.score_items(sr, E, cs, it, checked=True)
        fns['score_items C=1 M=%d, half the catalogue -inf' % M] = lambda it=it: ops.score_items(sr, E, cs, it, checked=True, bias=half)
        fns['score_items C=1 M=%d, bias [4, V], random groups' % M] = lambda it=it: ops.score_items(sr, E, cs, it, checked=True, bias=grouped,
                                                                                                group=group)
    fns['before: score_logp + bias [V], topk(20), C=1'] = logp_topk
    fns['before: three-matrix mixture + bias[group], topk(100), C=3'] = mixture_topk
    fns['model check of item_bias [V] (one device-to-host read)'] = lambda: model._item_bias('recommend', half, None)
    fns['model check of item_bias [4, V] and item_group'] = lambda: model._item_bias('recommend', grouped, group)
    with torch.no_grad():
        t = timed(fns, args.calls)
        v0, i0 = ops.score_select(sr, E, cs, 20)
        v1, i1 = ops.score_select(sr, E, cs, 20, bias=zero)
        same = torch.equal(i0, i1) and bool((v0 == v1).all())
    rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
    for k in fns:
        s = summary(t[k])
        rows.append('| %s | %.1f | %.1f | %.1f |' % (k, s['median_us'], s['p10_us'], s['p90_us']))
    text = '\n'.join(['B %d, V %d, d %d; %d timed calls per row after 5 warm-up rounds, rows alternating call by call; zero bias '
                      'returns the unbiased ids and values: %s' % (B, V, d, args.calls, same), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
