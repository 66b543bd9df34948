"""Timing of scoring given items (csrc/score_items.hip, ops.score_items) beside the materialising route the project had
before it, at the benchmarked shape (B 512, V 37 484, d 256) for M candidates per session: median of N device-event timed
calls after warm-up, all candidates of one M alternating call by call, p10 / p90 as the spread.
  one soft-max:   ops.score_items(off_ex = -lse)  |  the lse pass (ops.score_stats) + ops.score_items: what model.score_items
                  pays  |  ops.score_logp(...).gather(1, items): the (B, V) log-probabilities, then a gather
  C = 3 mixture:  ops.score_items with a 20-item scored list  |  forward().gather: three (B, V) log-prob matrices, their
                  logsumexp, then a gather
ops.score_items is timed as callers get it, with its id check (one device-to-host read), and with checked=True (the launch
alone).  `GB/s gathered` is B M d 4 bytes per median call of the launch alone; the rows come from a 38 MB table, so most of
them are served by the caches.  Prints one JSON line per M and the crossover; --out also writes the text.
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/score_items_timing.py --out profiles/score_items_timing.txt"""
import argparse
import importlib
import json
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
    ap.add_argument('--m', type=int, nargs='+', default=[20, 100, 1000, 2000, 4000])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'score_items_timing needs the GPU: there is nothing to fall back to'
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
    sr = srs[0].contiguous()
    ws = ops.CEWorkspace(B, V, d, dev)
    tg = ops.TableGrad(E)
    zeros = torch.zeros(B, device=dev, dtype=torch.int32)

    def lse():
        return ops.score_stats(sr, E, cs, zeros, ws, tg, None, 1.0, None)[0]

    lines = []
    with torch.no_grad():
        neg_lse = -lse().unsqueeze(0)
        for M in args.m:
            items = torch.randint(0, V, (B, M), device=dev)
            items[:, :L // 2] = listed[:, :L // 2]                 # some of every session's listed ids among its candidates
            i32 = items.to(torch.int32)
            fns = {
                'score_items C=1': lambda: ops.score_items(sr, E, cs, i32, neg_lse),
                'score_items C=1 launch alone': lambda: ops.score_items(sr, E, cs, i32, neg_lse, checked=True),
                'lse + score_items C=1': lambda: ops.score_items(sr, E, cs, i32, -lse().unsqueeze(0), checked=True),
                'score_logp.gather C=1': lambda: ops.score_logp(sr, E, cs, ws, 1.0).gather(1, items),
                'score_items C=3 launch alone': lambda: ops.score_items(srs, E, cs, i32, off_ex, off_in, listed, checked=True),
                'forward().gather C=3': lambda: torch.logsumexp(torch.stack(
                    [ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0).gather(1, items),
            }
            t = {k: summary(v) for k, v in timed(fns, args.calls).items()}
            err = float((fns['score_items C=1']() - fns['score_logp.gather C=1']()).abs().max())
            gbs = {k: round(B * M * d * 4 / (t[k]['median_us'] * 1e-6) / 1e9, 1) for k in t if 'launch alone' in k}
            lines.append(json.dumps(dict(B=B, V=V, d=d, M=M, calls=args.calls, us=t, gathered_GBps=gbs, max_abs_diff_c1=err)))
            print(lines[-1], flush=True)
    rec = [json.loads(x) for x in lines]
    for a, b in (('lse + score_items C=1', 'score_logp.gather C=1'), ('score_items C=3 launch alone', 'forward().gather C=3')):
        lost = [r['M'] for r in rec if r['us'][a]['median_us'] > r['us'][b]['median_us']]
        lines.append('%s vs %s: %s' % (a, b, 'the materialising route is the faster one from M = %d of %s' % (lost[0], args.m)
                                       if lost else 'score_items is the faster one at every M of %s' % args.m))
        print(lines[-1])
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
