"""Timing of the draw from the served distribution (csrc/recommend.hip NOISE instances, ops.score_sample) beside the selection
it extends (ops.score_select at the same C and K) and beside the route it replaces - the (B, V) log-probabilities (one
matrix, or the three-matrix mixture), + bias, torch Gumbel noise of the same size, topk - at the benchmarked shape
(B 512, V 37 484, d 256): median of N device-event timed calls after warm-up, all candidates alternating call by call,
p10 / p90 as the spread.
  C = 1, K = 1 | C = 1, K = 20 | C = 3, K = 100 with a 20-item list (scored), each with a [V] bias
`sample / select` is what the hash and the two logarithms per (session, item) pair cost on top of the selection.
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/sample_timing.py --out profiles/score_sample_timing.md"""
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
    assert torch.cuda.is_available(), 'sample_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d, C, L = 512, 37484, 256, 3, 20
    torch.manual_seed(1)
    srs = torch.randn(C, B, d, device=dev) * 0.3
    E = torch.randn(V, d, device=dev) * 0.2
    cs = torch.rand(V, device=dev) + 0.5
    off_ex = -2.0 * torch.rand(C, B, device=dev)
    off_in = off_ex + torch.rand(C, B, device=dev) * 3 - 1.0
    listed = torch.stack([torch.randperm(V, device=dev)[:L] for _ in range(B)]).to(torch.int32)
    bias = torch.randn(V, device=dev)
    bias[torch.rand(V, device=dev) < 0.1] = float('-inf')
    sr = srs[0].contiguous()
    ws = ops.CEWorkspace(B, V, d, dev)

    def gumbel_topk(s, k):
        return (s + bias[None] - torch.log(-torch.log(torch.rand_like(s)))).topk(k)

    def mat1(k):
        return lambda: gumbel_topk(ops.score_logp(sr, E, cs, ws, 1.0), k)

    def mat3():
        # forward() of a fusion model: one (B, V) log-prob matrix per order, their logsumexp (the list's offsets left out: the
        # materialised route is only cheaper for it)
        s = torch.logsumexp(torch.stack([ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0)
        return gumbel_topk(s, 100)
    rows3 = dict(off_ex=off_ex, off_in=off_in, listed=listed, bias=bias)
    groups = [
        ('C=1 K=1', lambda: ops.score_sample(sr, E, cs, 1, bias=bias, seed=3), lambda: ops.score_select(sr, E, cs, 1, bias=bias), mat1(1)),
        ('C=1 K=20', lambda: ops.score_sample(sr, E, cs, 20, bias=bias, seed=3), lambda: ops.score_select(sr, E, cs, 20, bias=bias),
         mat1(20)),
        ('C=3 K=100, 20 listed', lambda: ops.score_sample(srs, E, cs, 100, seed=3, temperature=0.7, **rows3),
         lambda: ops.score_select(srs, E, cs, 100, **rows3), mat3),
    ]
    fns = {}
    for name, smp, sel, mat in groups:
        fns['sample ' + name], fns['select ' + name], fns['materialised ' + name] = smp, sel, mat
    with torch.no_grad():
        t = timed(fns, args.calls)
    rows = ['| case | score_sample us (p10 / p90) | score_select us (p10 / p90) | sample / select | logp + bias + torch Gumbel + topk us (p10 / p90) | materialised / sample |',
            '|---|---|---|---|---|---|']
    for name, _, _, _ in groups:
        a, b, c = (summary(t[p + name]) for p in ('sample ', 'select ', 'materialised '))
        rows.append('| %s | %.1f (%.1f / %.1f) | %.1f (%.1f / %.1f) | %.2f | %.1f (%.1f / %.1f) | %.2f |' % (
            name, a['median_us'], a['p10_us'], a['p90_us'], b['median_us'], b['p10_us'], b['p90_us'], a['median_us'] / b['median_us'],
            c['median_us'], c['p10_us'], c['p90_us'], c['median_us'] / a['median_us']))
    text = '\n'.join(['B %d, V %d, d %d, a [V] bias (a tenth of it -inf); %d timed calls per entry after 5 warm-up rounds, all nine '
                      'callables alternating call by call; medians, p10 / p90 in brackets' % (B, V, d, args.calls), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
