"""Timing of the top-N selection (csrc/recommend.hip, ops.score_select) beside what the project had before it, at the
benchmarked shape (B 512, V 37 484, d 256): median of N device-event timed calls after warm-up, all candidates
alternating call by call, p10 / p90 as the spread.
  select C = 1, K = 20 | select C = 1, K = 100 | select C = 3, K = 100 with a 20-item list, scored and dropped
  ops.score_topk(k = 20) on the C = 1 inputs | materialised mixture: three (B, V) log-prob matrices, logsumexp, topk(100)
Prints a markdown table (and writes it with --out); `floor` is 2 B V d C flop at the fp32 MFMA peak (157.3 TFLOP/s).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/select_timing.py --out profiles/score_select_timing.md"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import PEAK_FP32_MFMA, summary, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'select_timing needs the GPU: there is nothing to fall back to'
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

    def materialised():
        # forward() of a fusion model: one (B, V) log-prob matrix per order, their logsumexp, torch.topk
        s = torch.logsumexp(torch.stack([ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0)
        return s.topk(100)
    fns = {
        'select C=1 K=20': (1, lambda: ops.score_select(sr, E, cs, 20)),
        'select C=1 K=100': (1, lambda: ops.score_select(sr, E, cs, 100)),
        'select C=3 K=100, 20 listed scored': (3, lambda: ops.score_select(srs, E, cs, 100, off_ex, off_in, listed)),
        'select C=3 K=100, 20 listed dropped': (3, lambda: ops.score_select(srs, E, cs, 100, off_ex, None, listed, drop_listed=True)),
        'score_topk C=1 K=20 (topk.hip)': (1, lambda: ops.score_topk(sr, E, cs, 20)),
        'materialised C=3 mixture, topk(100)': (3, materialised),
    }
    with torch.no_grad():
        t = timed({k: f for k, (_, f) in fns.items()}, args.calls)
        same = torch.equal(ops.score_select(sr, E, cs, 20)[1], ops.score_topk(sr, E, cs, 20)[1])
    rows = ['| call | median us | p10 us | p90 us | fp32 MFMA floor us | floor / median |', '|---|---|---|---|---|---|']
    for k, (c, _) in fns.items():
        s = summary(t[k])
        floor = 2.0 * B * V * d * c / PEAK_FP32_MFMA * 1e6
        rows.append('| %s | %.1f | %.1f | %.1f | %.1f | %.2f |' % (k, s['median_us'], s['p10_us'], s['p90_us'], floor, floor / s['median_us']))
    text = '\n'.join(['B %d, V %d, d %d; %d timed calls per row after 5 warm-up rounds, rows alternating call by call; '
                      'select K=20 ids equal score_topk ids: %s' % (B, V, d, args.calls, same), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
