"""Timing of the per-session hide / boost lists (csrc/personal.hip, ops.personal_merge, model.recommend_personal) at the serving
shape - B 512 sessions, a table of V 37 484 rows of d 256 - beside the calls it is built from: median of N device-event timed
calls after warm-up, the candidates alternating call by call, p10 / p90 as the spread.
  (a) ops.personal_merge alone, k 20, at the pools the model call takes for lists of M = 20, 108, 300 and 1024 items: hide-only
      (no bias) and with finite biases
  (b) the calls it is built from: recommend(k=20), recommend(k=128), recommend_many(k=20 + M), score_items of M items
  (c) SRGNN recommend_personal(k=20) end to end for those M: lists drawn uniformly from the catalogue (beyond k + M = 128 the
      128-item pool of stage 1 suffices), hide-only and with finite biases, and lists holding the session's own top-M items,
      which send the batch to recommend_many(k + M)
and how often stage 1 suffices for 300-item lists (uniform over the catalogue, and drawn from the session's own top-1000).
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 400 python tools/personal_timing.py --out profiles/personal_timing.md"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, synth_samples, timed

K = 20
LISTS = (20, 108, 300, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'personal_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    sp = importlib.import_module('sessionrec-pytorch_amd')
    col = importlib.import_module('sessionrec-pytorch_amd.collate')
    dev = torch.device('cuda:0')
    B, V, d = 512, 37484, 256
    torch.manual_seed(1)
    g = torch.Generator().manual_seed(2)
    model = sp.SRGNN(V, d, 1).to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)(synth_samples(B, V, 123))
    mg = inputs[0].to(dev)
    fns, notes = {}, []
    with torch.no_grad():
        top = model.recommend_many(mg, k=1024)[1]
        fns['(b) recommend k=20'] = lambda: model.recommend(mg, k=K)
        fns['(b) recommend k=128 (the pool of stage 1)'] = lambda: model.recommend(mg, k=128)
        for M in LISTS:
            uniform = torch.stack([torch.randperm(V, generator=g)[:M] for _ in range(B)]).to(dev)
            bias = (torch.rand(B, M, generator=g) * 4 - 2).to(dev)
            head = top[:, :M].contiguous()
            P = K + M
            fns['(b) recommend_many k=%d (the pool k + M)' % P] = lambda P=P: model.recommend_many(mg, k=P)
            fns['(b) score_items of M=%d items' % M] = lambda it=uniform: model.score_items(mg, items=it)
            for P1 in sorted({min(P, 128), P}):
                pv, pi = model.recommend_many(mg, k=P1)
                base = model.score_items(mg, items=uniform)
                it32 = uniform.to(torch.int32)
                fns['(a) ops.personal_merge M=%d, P=%d, hide' % (M, P1)] = \
                    lambda pi=pi, pv=pv, it=it32, base=base: ops.personal_merge(pi, pv, it, base, None, K, checked=True)
                fns['(a) ops.personal_merge M=%d, P=%d, biases' % (M, P1)] = \
                    lambda pi=pi, pv=pv, it=it32, base=base, bs=bias: ops.personal_merge(pi, pv, it, base, bs, K, checked=True)
            fns['(c) recommend_personal k=20, M=%d uniform, hide' % M] = \
                lambda it=uniform: model.recommend_personal(mg, k=K, personal_items=it)
            fns['(c) recommend_personal k=20, M=%d uniform, biases' % M] = \
                lambda it=uniform, bs=bias: model.recommend_personal(mg, k=K, personal_items=it, personal_bias=bs)
            fns['(c) recommend_personal k=20, M=%d = the session\'s own top-M, hide' % M] = \
                lambda it=head: model.recommend_personal(mg, k=K, personal_items=it)
            if M == 300:
                near = torch.stack([top[b, torch.randperm(1000, generator=g)[:M].to(dev)] for b in range(B)])
                for what, it in (('uniform over the catalogue', uniform), ('drawn from the session\'s own top-1000', near)):
                    hit = ops.personal_merge(*reversed(model.recommend(mg, k=128)), it.to(torch.int32),
                                             model.score_items(mg, items=it), None, K, checked=True)[3]
                    done = hit <= 128 - K
                    notes.append('300-item lists %s: %d of %d sessions complete after stage 1 (mean hit %.1f, largest %d) - the '
                                 'batch %s' % (what, int(done.sum()), B, float(hit.float().mean()), int(hit.max()),
                                               'ends there' if bool(done.all()) else 'goes on to recommend_many(320)'))
        t = timed(fns, args.calls)
    rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
    for name in fns:
        s = summary(t[name])
        rows.append('| %s | %.1f | %.1f | %.1f |' % (name, s['median_us'], s['p10_us'], s['p90_us']))
    text = '\n'.join(['B %d, V %d, d %d, SRGNN, k %d; %d timed calls per row after 5 warm-up rounds, rows alternating call by call.'
                      % (B, V, d, K, args.calls), ''] + notes + [''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
