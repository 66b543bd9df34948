"""Timing of the log-normaliser over the eligible catalogue (csrc/score_norm.hip: ops.score_norm) beside what was there
before for the same number - the materialised (B, V) log-probabilities (score_logp, or the three-matrix mixture of a fusion
model's forward()) plus the bias, then torch.logsumexp - at the benchmarked shape (B 512, V 37 484, d 256): median of N
device-event timed calls after warm-up, all rows alternating call by call, p10 / p90 as the spread.
  C = 1, no bias (also beside the fused statistics pass score_stats, the `_lse` of the models)
  C = 1, bias [V] with half the entries -inf
  C = 3, bias [4, V] with random groups
  C = 3 with a 20-item list per session, scored (off_in) and dropped
Every pair is also compared value by value (the largest difference is printed with the table).
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/score_norm_timing.py --out profiles/score_norm_timing.md"""
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
    assert torch.cuda.is_available(), 'score_norm_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d, C, G, L = 512, 37484, 256, 3, 4, 20
    torch.manual_seed(1)
    srs = torch.randn(C, B, d, device=dev) * 0.3
    E = torch.randn(V, d, device=dev) * 0.2
    cs = torch.rand(V, device=dev) + 0.5
    off_ex = -2.0 * torch.rand(C, B, device=dev)
    off_in = off_ex + torch.rand(C, B, device=dev) * 3 - 1.0
    sr = srs[0].contiguous()
    ws = ops.CEWorkspace(B, V, d, dev)
    tg = ops.TableGrad(E)
    zeros = torch.zeros(B, device=dev, dtype=torch.int32)
    half = ops.catalog_bias(V, deny=torch.randperm(V, device=dev)[:V // 2], device=dev)
    grouped = torch.randn(G, V, device=dev)
    grouped[torch.rand(G, V, device=dev) < 0.5] = float('-inf')
    group = torch.randint(0, G, (B,), device=dev, dtype=torch.int32)
    listed = torch.stack([torch.randperm(V, device=dev)[:L] for _ in range(B)]).to(torch.int32)
    inside = torch.zeros(B, V, dtype=torch.bool, device=dev).scatter_(1, listed.long(), True)

    def logp(c, off=None):
        # (B, V) log-probabilities of one soft-max, as forward() forms them; + a per-session offset for a mixture component
        z = ops.score_logp(srs[c], E, cs, ws, 1.0)
        return z if off is None else z + off[c][:, None]

    def mixture(listed_mode=None):
        # forward() of a fusion model: one (B, V) matrix per order, their logsumexp; the session's own items through off_in
        ex = torch.logsumexp(torch.stack([logp(c, off_ex) for c in range(C)], 0), 0)
        if listed_mode is None:
            return ex
        if listed_mode == 'drop':
            return ex.masked_fill(inside, float('-inf'))
        return torch.where(inside, torch.logsumexp(torch.stack([logp(c, off_in) for c in range(C)], 0), 0), ex)

    def lse_raw():
        # what score_logp subtracts: the statistics pass alone gives the plain normaliser of one soft-max
        return ops.score_stats(sr, E, cs, zeros, ws, tg, None, 1.0, None)[0]
    # the mixture's offsets as the models pass them: minus every component's own lse, so that the score is forward()'s
    lse_c = torch.stack([ops.score_stats(srs[c].contiguous(), E, cs, zeros, ws, tg, None, 1.0, None)[0] for c in range(C)], 0)
    nex, nin = (off_ex - lse_c).contiguous(), (off_in - lse_c).contiguous()
    # (name, the new call, what was there before, what the comparison of their values adds to `before`: score_logp returns
    # z - lse, score_norm at C = 1 sums the raw logits)
    pairs = [
        ('C=1, no bias', lambda: ops.score_norm(sr, E, cs), lambda: torch.logsumexp(logp(0), 1), lse_raw),
        ('C=1, bias [V], half the catalogue -inf', lambda: ops.score_norm(sr, E, cs, bias=half),
         lambda: torch.logsumexp(logp(0) + half, 1), lse_raw),
        ('C=3, bias [4, V], random groups', lambda: ops.score_norm(srs, E, cs, nex, bias=grouped, group=group),
         lambda: torch.logsumexp(mixture() + grouped[group.long()], 1), None),
        ('C=3, 20 listed items scored with off_in', lambda: ops.score_norm(srs, E, cs, nex, nin, listed),
         lambda: torch.logsumexp(mixture('score'), 1), None),
        ('C=3, 20 listed items dropped', lambda: ops.score_norm(srs, E, cs, nex, None, listed, drop_listed=True),
         lambda: torch.logsumexp(mixture('drop'), 1), None),
    ]
    fns = {}
    for name, new, old, _ in pairs:
        fns['score_norm ' + name] = new
        fns['before: materialised + logsumexp, ' + name] = old
    fns['score_stats (the `_lse` pass), C=1, no bias'] = lse_raw
    with torch.no_grad():
        t = timed(fns, args.calls)
        diffs = ['%s: %.1e' % (name, float((new() - (old() if fix is None else old() + fix())).abs().max())) for name, new, old, fix in pairs]
        diffs.append('score_stats against score_norm, C=1, no bias: %.1e' % float((lse_raw() - ops.score_norm(sr, E, cs)).abs().max()))
    rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
    for k in fns:
        s = summary(t[k])
        rows.append('| %s | %.1f | %.1f | %.1f |' % (k, s['median_us'], s['p10_us'], s['p90_us']))
    text = '\n'.join(['B %d, V %d, d %d; %d timed calls per row after 5 warm-up rounds, rows alternating call by call.' % (B, V, d, args.calls),
                      'Largest |score_norm - before| per pair: ' + '; '.join(diffs), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
