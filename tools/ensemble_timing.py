"""Timing of the multi-table selection (csrc/ensemble.hip, ops.ens_select) beside the two routes a user had before it, at the
benchmarked shape (B 512, V 37 484, d 256), K 20 and 100: median of N device-event timed calls after warm-up, all candidates
alternating call by call, p10 / p90 as the spread.
  two single-soft-max members (C = 2, a table each) | a single-soft-max member and a three-component one (C = 4, two tables)
  ens_select | materialised: one fp32 (B, V) log-prob matrix per component, logsumexp, torch.topk | the members' separate
  ops.score_select calls summed (the cost of the tile products plus one selection each; it does not give the blend)
Prints a markdown table (and writes it with --out); `floor` is 2 B V d C flop at the fp32 MFMA peak (157.3 TFLOP/s).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/ensemble_timing.py --out profiles/ensemble_timing.md"""
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
    assert torch.cuda.is_available(), 'ensemble_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    dev = torch.device('cuda:0')
    B, V, d = 512, 37484, 256
    torch.manual_seed(1)
    tables = [torch.randn(V, d, device=dev) * 0.2 for _ in range(2)]
    css = [torch.rand(V, device=dev) + 0.5 for _ in range(2)]
    srs = torch.randn(4, B, d, device=dev) * 0.3
    logw = -8.0 + 4.0 * torch.rand(4, B, device=dev)
    ws = ops.CEWorkspace(B, V, d, dev)
    table_of = [0, 1, 1, 1]
    # the fused route scores raw logits: its offsets carry -lse of every component, as a member's Query does; the
    # materialised route adds the same logw to score_logp's log-probabilities - the two compute one blend
    lse = torch.stack([torch.logsumexp((srs[c] @ tables[t].T) * css[t][None, :], 1) for c, t in enumerate(table_of)], 0)
    off = (logw - lse).contiguous()
    # members as (table index, components): C = 2 is two single soft-maxes, C = 4 is 1 + 3 components
    layouts = {'C=2 (1 + 1)': [(0, [0]), (1, [1])], 'C=4 (1 + 3)': [(0, [0]), (1, [1, 2, 3])]}

    def comps_of(layout):
        return [(srs[c], tables[t], css[t]) for t, cs_ in layout for c in cs_]

    def offs_of(layout):
        return torch.stack([off[c] for _, cs_ in layout for c in cs_], 0).contiguous()

    def fused(layout, k):
        comps, o = comps_of(layout), offs_of(layout)
        return lambda: ops.ens_select(comps, k, o)

    def materialised(layout, k):
        def run():
            z = [ops.score_logp(srs[c], tables[t], css[t], ws, 1.0) + logw[c][:, None] for t, cs_ in layout for c in cs_]
            return torch.logsumexp(torch.stack(z, 0), 0).topk(k)
        return run

    def separate(layout, k):
        members = [(srs[cs_].contiguous() if len(cs_) > 1 else srs[cs_[0]], tables[t], css[t], off[cs_].contiguous())
                   for t, cs_ in layout]

        def run():
            return [ops.score_select(s, E, cs, k, o) for s, E, cs, o in members]
        return run
    fns, flops = {}, {}
    for name, layout in layouts.items():
        C = sum(len(cs_) for _, cs_ in layout)
        for k in (20, 100):
            for what, make in (('ens_select', fused), ('materialised + topk', materialised), ('separate score_select, summed', separate)):
                key = '%s K=%d %s' % (name, k, what)
                fns[key], flops[key] = make(layout, k), C
    with torch.no_grad():
        t = timed(fns, args.calls)
        v, i = fns['C=4 (1 + 3) K=20 ens_select']()
        mv, mi = fns['C=4 (1 + 3) K=20 materialised + topk']()
        same = float((i == mi.to(torch.int32)).float().mean())
        err = float((v - mv).abs().max())
    rows = ['| call | median us | p10 us | p90 us | fp32 MFMA floor us | floor / median |', '|---|---|---|---|---|---|']
    for k in fns:
        s = summary(t[k])
        floor = 2.0 * B * V * d * flops[k] / PEAK_FP32_MFMA * 1e6
        rows.append('| %s | %.1f | %.1f | %.1f | %.1f | %.2f |' % (k, s['median_us'], s['p10_us'], s['p90_us'], floor, floor / s['median_us']))
    text = '\n'.join(['B %d, V %d, d %d; %d timed calls per row after 5 warm-up rounds, rows alternating call by call; C=4 K=20: '
                      'share of ens_select ids equal to the materialised topk ids %.4f, max |value difference| %.1e'
                      % (B, V, d, args.calls, same, err), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
