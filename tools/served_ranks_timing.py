"""Timing of the many-targets served rank (ops.score_ahead_many, csrc/rank_served_many.hip: ONE pass over the table for M given
items per session) against the M calls of the single-label count it replaces (ops.score_ahead, csrc/rank_served.hip -
unchanged), at the benchmarked shape (B 512, V 37 484, d 256), C = 1 and 3: median of N device-event timed calls after warm-up,
the two rows of a pair alternating call by call (the conventions of tools/served_rank_timing.py).  Both sides are given the
items' scores (score_items, outside the timed region).
  M in {1, 2, 4, 16, 64}, two placements of the targets:
    uniform   ids drawn uniformly from the catalogue - their ranks spread over everything, so nearly every (session, row) score
              falls between the best and the worst threshold: the worst case for the bucket path
    top100    ids drawn from each session's 100 best - nearly every score is behind all thresholds and does nothing
What must hold: at every M >= 4, in both placements, the one call is faster than the M single calls ("holds" column); M = 1 and
2 are reported without a requirement (model.rank_items routes M = 1 to the single-label kernel).
Prints one JSON line per row and writes a markdown table with --out.
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/served_ranks_timing.py --out profiles/served_ranks_timing.md"""
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

MS = (1, 2, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'served_ranks_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d = 512, 37484, 256
    rows = []
    for C in (1, 3):
        torch.manual_seed(C)
        srs = torch.randn(C, B, d, device=dev) * 0.3
        E = torch.randn(V, d, device=dev) * 0.2
        cs = torch.rand(V, device=dev) + 0.5
        off_ex = -2.0 * torch.rand(C, B, device=dev)
        best = ops.score_select(srs, E, cs, 100, off_ex)[1]
        for place in ('uniform', 'top100'):
            for M in MS:
                if place == 'uniform':
                    items = torch.stack([torch.randperm(V, device=dev)[:M] for _ in range(B)]).to(torch.int32)
                else:
                    items = best.gather(1, torch.stack([torch.randperm(100, device=dev)[:M] for _ in range(B)])).contiguous()
                target = ops.score_items(srs, E, cs, items, off_ex).contiguous()
                cols = [(items[:, j].contiguous(), target[:, j].contiguous()) for j in range(M)]

                def singles():
                    return [ops.score_ahead(srs, E, cs, lab, t, off_ex) for lab, t in cols]
                t = timed({'many': lambda: ops.score_ahead_many(srs, E, cs, items, target, off_ex), 'singles': singles}, args.calls)
                many, single = summary(t['many']), summary(t['singles'])
                got = ops.score_ahead_many(srs, E, cs, items, target, off_ex)
                differ = int((got != torch.stack(singles(), 1)).sum())      # (targets within round-off of each other may)
                rows.append(dict(C=C, placement=place, M=M, B=B, V=V, d=d, calls=args.calls,
                                 many=many, singles=single, speedup=round(single['median_us'] / many['median_us'], 2),
                                 holds=(None if M < 4 else bool(many['median_us'] < single['median_us'])),
                                 slots_differing_from_singles=differ, mean_rank=round(float(got.float().mean()), 1)))
    for r in rows:
        print(json.dumps(r))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('ops.score_ahead_many (one call) beside M calls of ops.score_ahead on the same operands; B %d, V %d, d %d; median '
                    '(p10 - p90) of %d timed calls, microseconds.  holds: one call is faster than the M calls it replaces (required '
                    'at M >= 4).\n\n' % (B, V, d, args.calls))
            f.write('| C | placement | M | one call us | M single calls us | speed-up | holds | mean rank |\n|---|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write('| %d | %s | %d | %.1f (%.1f - %.1f) | %.1f (%.1f - %.1f) | %.2f | %s | %.1f |\n' % (
                    r['C'], r['placement'], r['M'], r['many']['median_us'], r['many']['p10_us'], r['many']['p90_us'],
                    r['singles']['median_us'], r['singles']['p10_us'], r['singles']['p90_us'], r['speedup'],
                    '-' if r['holds'] is None else ('yes' if r['holds'] else 'NO'), r['mean_rank']))
            bad = [r for r in rows if r['holds'] is False]
            f.write('\nrows where the condition fails: %s\n' % (json.dumps([(r['C'], r['placement'], r['M']) for r in bad]) if bad else 'none'))
            f.write('slots differing from the single calls (targets of a session within round-off of each other): %s\n'
                    % json.dumps({'C%d %s M%d' % (r['C'], r['placement'], r['M']): r['slots_differing_from_singles'] for r in rows
                                  if r['slots_differing_from_singles']}))


if __name__ == '__main__':
    main()
