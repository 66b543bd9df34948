"""Timing of the diversified top-N (csrc/diversify.hip, ops.diversify) at the serving shape - B 512 sessions, a pool of
M 128 of a table of V 37 484 rows of d 256, K 20 picks - beside what a caller had to write before and beside the selection
that makes the pool: median of N device-event timed calls after warm-up, the candidates alternating call by call, p10 / p90
as the spread.
  (a) ops.diversify on the table and the pool's ids (one launch)
  (b) the composition in PyTorch: gather [B, M, d], normalise, bmm to a [B, M, M] Gram matrix, K steps of argmax / maximum
  (c) ops.score_select(k=128) alone: the pool
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/diversify_timing.py --out FILE"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, timed


def torch_mmr(E, ids, val, k, theta):
    """the composition ops.diversify replaces (every slot filled): (val [B,k], pick [B,k], ild [B])"""
    x = torch.nn.functional.normalize(E[ids.long()], dim=-1, eps=1e-12)
    sim = torch.bmm(x, x.transpose(1, 2))
    B, M = val.shape
    ar = torch.arange(B, device=val.device)
    pen = torch.zeros_like(val)
    taken = torch.zeros_like(val, dtype=torch.bool)
    picks = []
    for t in range(k):
        m = (val - theta * pen if t else val).masked_fill(taken, float('-inf'))
        p = m.argmax(1)
        picks.append(p)
        taken[ar, p] = True
        pen = sim[ar, p] if t == 0 else torch.maximum(pen, sim[ar, p])
    pick = torch.stack(picks, 1)
    sub = sim.gather(1, pick[:, :, None].expand(B, k, M)).gather(2, pick[:, None, :].expand(B, k, k))
    ild = 1 - (sub.sum((1, 2)) - sub.diagonal(dim1=1, dim2=2).sum(1)) / (k * (k - 1))
    return val.gather(1, pick), pick, ild


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'diversify_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d, M, K, theta = 512, 37484, 256, 128, 20, 0.5
    torch.manual_seed(1)
    sr = torch.randn(B, d, device=dev) * 0.3
    # a catalogue with near-duplicates: 4 000 directions, every row close to one of them
    E = (torch.randn(4000, d, device=dev)[torch.randint(0, 4000, (V,), device=dev)] + 0.3 * torch.randn(V, d, device=dev)) * 0.2
    with torch.no_grad():
        val, ids = ops.score_select(sr, E, None, M)
        got = ops.diversify(E, ids, val, K, theta, checked=True)
        ref = torch_mmr(E, ids, val, K, theta)
        same = float((got[1].long() == ref[1]).float().mean())
        fns = {
            '(a) ops.diversify, K=20 of M=128 (one launch)': lambda: ops.diversify(E, ids, val, K, theta, checked=True),
            '(a\') ops.diversify with its row check (one device-to-host read)': lambda: ops.diversify(E, ids, val, K, theta),
            '(b) PyTorch: gather, normalise, bmm, 20 x (argmax, maximum)': lambda: torch_mmr(E, ids, val, K, theta),
            '(c) ops.score_select k=128 alone (the pool)': lambda: ops.score_select(sr, E, None, M),
            'ops.score_select k=20 (the plain top 20)': lambda: ops.score_select(sr, E, None, K),
        }
        t = timed(fns, args.calls)
    rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
    med = {}
    for name in fns:
        s = summary(t[name])
        med[name[:3]] = s['median_us']
        rows.append('| %s | %.1f | %.1f | %.1f |' % (name, s['median_us'], s['p10_us'], s['p90_us']))
    text = '\n'.join(['B %d, V %d, d %d, pool M %d, K %d, diversity %.2f; %d timed calls per row after 5 warm-up rounds, rows '
                      'alternating call by call; picks equal to the PyTorch composition\'s: %.4f of all slots; mean ild %.4f '
                      '(first %d slots: %.4f)' % (B, V, d, M, K, theta, args.calls, same, float(got[3].mean()), K,
                                                  float(ops.diversify(E, ids[:, :K].contiguous(), val[:, :K].contiguous(), K, 0.0)[3].mean())),
                      ''] + rows +
                     ['', '(b) / (a) = %.2f; (a) / (c) = %.3f' % (med['(b)'] / med['(a)'], med['(a)'] / med['(c)'])])
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
