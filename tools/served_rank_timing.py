"""Timing of the served-rank count (ops.score_ahead, csrc/rank_served.hip) against the rank evaluation it stands beside
(ops.score_rank, csrc/rank.hip - unchanged), at the benchmarked shape (B 512, V 37 484, d 256): median of N device-event timed
calls after warm-up, the rows of a group alternating call by call (the conventions of tools/rank_timing.py).  Both sides are
given the labels' scores (target=), so both run one pass over the table: score_rank its target kernel (which only initialises
the ranks then), the count kernel and, with a list, the fix-up kernel; score_ahead a 2 KB memset and its count kernel.
  C = 1 and C = 3:  plain (no bias, no list)   vs  score_rank at the same C
                    a [V] bias, a [4, V] bias  vs  the same score_rank (it takes no bias)
                    20 listed ids, dropped     vs  score_rank with the same 20 ids scored through off_in (it cannot drop)
Prints one JSON line per row and writes a markdown table with --out.
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/served_rank_timing.py --out profiles/served_rank_timing.md"""
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
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'served_rank_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d, L, G = 512, 37484, 256, 20, 4
    rows, agree = [], []
    for C in (1, 3):
        torch.manual_seed(C)
        srs = torch.randn(C, B, d, device=dev) * 0.3
        E = torch.randn(V, d, device=dev) * 0.2
        cs = torch.rand(V, device=dev) + 0.5
        labels = torch.randint(0, V, (B,), device=dev, dtype=torch.int32)
        off_ex = -2.0 * torch.rand(C, B, device=dev)
        off_in = off_ex + 1.0
        listed = torch.stack([torch.randperm(V, device=dev)[:L] for _ in range(B)]).to(torch.int32)
        bias1 = torch.randn(V, device=dev) * 0.5
        bias1[torch.rand(V, device=dev) < 0.1] = float('-inf')
        biasG = torch.randn(G, V, device=dev) * 0.5
        group = torch.randint(0, G, (B,), device=dev, dtype=torch.int32)
        target = ops.score_items(srs, E, cs, labels[:, None], off_ex)[:, 0].contiguous()
        t_in = ops.score_items(srs, E, cs, labels[:, None], off_ex, off_in, listed)[:, 0].contiguous()
        fns = {
            'score_rank plain': lambda: ops.score_rank(srs, E, cs, labels, off_ex, target=target),
            'score_ahead plain': lambda: ops.score_ahead(srs, E, cs, labels, target, off_ex),
            'score_ahead bias [V]': lambda: ops.score_ahead(srs, E, cs, labels, target, off_ex, bias=bias1),
            'score_ahead bias [4, V]': lambda: ops.score_ahead(srs, E, cs, labels, target, off_ex, bias=biasG, group=group),
            'score_rank 20 listed, scored': lambda: ops.score_rank(srs, E, cs, labels, off_ex, off_in, listed, target=t_in),
            'score_ahead 20 listed, scored': lambda: ops.score_ahead(srs, E, cs, labels, t_in, off_ex, off_in, listed),
            'score_ahead 20 listed, dropped': lambda: ops.score_ahead(srs, E, cs, labels, target, off_ex, None, listed, True),
        }
        t = timed(fns, args.calls)
        base = {k: summary(v) for k, v in t.items()}
        for k, s in base.items():
            ref = base['score_rank 20 listed, scored' if 'listed' in k else 'score_rank plain']['median_us']
            rows.append(dict(call=k, C=C, B=B, V=V, d=d, calls=args.calls, **s, ratio_to_score_rank=round(s['median_us'] / ref, 3)))
        # the two kernels agree where they compute the same thing (the plain count; the scored list up to the fix-up's clamp)
        r_plain = ops.score_rank(srs, E, cs, labels, off_ex, target=target)[0]
        a_plain = ops.score_ahead(srs, E, cs, labels, target, off_ex)
        r_in = ops.score_rank(srs, E, cs, labels, off_ex, off_in, listed, target=t_in)[0].clamp(min=0)
        a_in = ops.score_ahead(srs, E, cs, labels, t_in, off_ex, off_in, listed)
        agree.append(dict(C=C, plain_equal=bool(torch.equal(r_plain, a_plain)),
                          listed_max_abs_diff=int((r_in - a_in).abs().max())))
    for r in rows:
        print(json.dumps(r))
    print(json.dumps(dict(agree=agree)))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('| call | C | median us | p10 us | p90 us | ratio to score_rank |\n|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| %s | %d | %.1f | %.1f | %.1f | %.3f |\n' % (r['call'], r['C'], r['median_us'], r['p10_us'], r['p90_us'],
                                                                        r['ratio_to_score_rank']))
            f.write('\nagreement: %s\n' % json.dumps(agree))


if __name__ == '__main__':
    main()
