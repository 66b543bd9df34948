"""Timing of the cutoff of truncated sampling (csrc/score_cutoff.hip: ops.score_cutoff) beside the log-mass pass at the same
shape (ops.score_norm: what ONE pass over the table costs at least) and beside the route it replaces - the materialised (B, V)
scores, torch.sort and a cumulative sum - at the benchmarked shape (B 512, V 37 484, d 256): median of N device-event timed
calls after warm-up, all rows alternating call by call, p10 / p90 as the spread.
  C = 1, no bias, no list
  C = 3 mixture, bias [4, V] with random groups, a 20-item list per session, dropped
Per configuration: the maximum (the K = 1 selection), each histogram pass (both searches, and the top_p search alone), the
advance step, the tail pass, the finish step, and the whole score_cutoff for top_k alone, top_p alone and both.
--big adds the per-rank shard shape of a 10 M item catalogue on 8 ranks (V 1 250 000), C = 1.
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 400 python tools/score_cutoff_timing.py --out profiles/score_cutoff_timing.md"""
import argparse
import ctypes
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, timed

TOP_K, TOP_P, T = 1000, 0.9, 1.0


def pieces(ops, sc, L, srs, E, cs, off_ex, listed, drop, bias, group):
    """{row name: callable} of the single launches of one score_cutoff(top_k, top_p) call, each on the state the call itself
    would hand it (the passes are run once, the state ahead of every pass is kept)"""
    k_, p_, gap, inv_t = ops.cutoff_scalars('timing', TOP_K, TOP_P, None, T)
    a = sc._served_args('score_cutoff', srs, E, cs, off_ex, None, listed, drop, 0, bias, group)
    B, dev = a.B, a.srs.device
    desc = a.struct()
    served = ctypes.addressof(desc)
    lib, st = L.lib, L.stream
    n = ctypes.c_long()
    lib.srec_score_select_ws(B, a.V, a.d, a.C, a.L, 1, ctypes.addressof(n))
    ws = torch.empty(n.value, device=dev, dtype=torch.uint8)
    top = torch.empty(B, device=dev)
    ids = torch.empty(B, device=dev, dtype=torch.int32)
    floor = torch.empty(B, device=dev)
    count = torch.empty(B, device=dev, dtype=torch.int32)
    lk = torch.empty(B, device=dev)
    hist = torch.zeros(B, 3, 256, device=dev, dtype=torch.int64)
    state = torch.zeros(B, 8, device=dev, dtype=torch.int64)
    lib.srec_score_select(served, 1, None, L.ptr(top), L.ptr(ids), L.ptr(ws), st())
    before, hists = [], []
    for j in range(4):
        before.append(state.clone())
        lib.srec_score_cutoff_hist(served, inv_t, k_, p_, j, L.ptr(top), L.ptr(state), L.ptr(hist), st())
        hists.append(hist.clone())
        lib.srec_score_cutoff_advance(B, j, k_, p_, gap, L.ptr(hist), L.ptr(state), L.ptr(top), L.ptr(floor), st())
    scratch = torch.zeros_like(state)
    keep = (a, desc, ws, before, hists)                    # the operands behind the pointers

    def hist_pass(j, k, p):
        return lambda: lib.srec_score_cutoff_hist(served, inv_t, k, p, j, L.ptr(top), L.ptr(before[j]), L.ptr(hist), st())

    def advance():
        scratch.copy_(before[1])
        lib.srec_score_cutoff_advance(B, 1, k_, p_, gap, L.ptr(hists[1]), L.ptr(scratch), L.ptr(top), L.ptr(floor), st())
    fns = {'maximum (K = 1 selection)': lambda: lib.srec_score_select(served, 1, None, L.ptr(top), L.ptr(ids), L.ptr(ws), st())}
    for j in range(4):
        fns['histogram pass %d, top_k + top_p' % j] = hist_pass(j, k_, p_)
    for j in range(4):
        fns['histogram pass %d, top_p alone' % j] = hist_pass(j, 0, p_)
    for j in range(4):
        fns['histogram pass %d, top_k alone' % j] = hist_pass(j, k_, 1.0)
    fns['advance step (with a 4 KB state copy)'] = advance
    fns['tail pass'] = lambda: lib.srec_score_cutoff_tail(served, inv_t, L.ptr(top), L.ptr(floor), L.ptr(hist), st())
    fns['finish step'] = lambda: lib.srec_score_cutoff_finish(B, L.ptr(hist), L.ptr(count), L.ptr(lk), st())
    return fns, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--big', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'score_cutoff_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    sc = importlib.import_module('sessionrec-pytorch_amd.score')
    L = importlib.import_module('sessionrec-pytorch_amd._lib')
    dev = torch.device('cuda:0')
    B, d, C, G, NL = 512, 256, 3, 4, 20
    text = []
    for V in [37484] + ([1250000] if args.big else []):
        torch.manual_seed(1)
        srs = torch.randn(C, B, d, device=dev) * 0.3
        E = torch.randn(V, d, device=dev) * 0.2
        cs = torch.rand(V, device=dev) + 0.5
        off_ex = -2.0 * torch.rand(C, B, device=dev)
        sr = srs[0].contiguous()
        ws = ops.CEWorkspace(B, V, d, dev)
        grouped = torch.randn(G, V, device=dev)
        grouped[torch.rand(G, V, device=dev) < 0.5] = float('-inf')
        group = torch.randint(0, G, (B,), device=dev, dtype=torch.int32)
        listed = torch.stack([torch.randperm(V, device=dev)[:NL] for _ in range(B)]).to(torch.int32)
        tg = ops.TableGrad(E)
        zeros = torch.zeros(B, device=dev, dtype=torch.int32)
        # the mixture's offsets as the models pass them: minus every component's own lse, so that the score is forward()'s
        lse_c = torch.stack([ops.score_stats(srs[c].contiguous(), E, cs, zeros, ws, tg, None, 1.0, None)[0] for c in range(C)], 0)
        nex = (off_ex - lse_c).contiguous()

        def nucleus(s):
            # the route the kernel replaces, given the (B, V) scores: sort, soft-max, cumulative sum, the boundary value
            v, _ = s.sort(dim=1, descending=True)
            cum = torch.softmax(v / T, 1).cumsum(1)
            n = (cum < TOP_P).sum(1).clamp(max=V - 1)
            return v.gather(1, n[:, None])[:, 0], n + 1

        def materialised1():
            return nucleus(ops.score_logp(sr, E, cs, ws, 1.0))

        def materialised3():
            z = torch.logsumexp(torch.stack([ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0)
            z = z + grouped[group.long()]
            return nucleus(z.scatter(1, listed.long(), float('-inf')))
        configs = [('C=1', (sr, E, cs, None, None, False, None, None), materialised1)]
        if V < 100000:
            configs.append(('C=3, bias [4, V], 20 listed items dropped', (srs, E, cs, nex, listed, True, grouped, group), materialised3))
        for name, (s_, E_, cs_, off_, lst_, drop_, bias_, grp_), before in configs:
            kw = dict(off_ex=off_, listed=lst_, drop_listed=drop_, bias=bias_, group=grp_, temperature=T)
            fns, keep = pieces(ops, sc, L, s_, E_, cs_, off_, lst_, drop_, bias_, grp_)
            fns = {'%s: %s' % (name, k): f for k, f in fns.items()}
            fns['%s: score_cutoff, top_k = %d' % (name, TOP_K)] = lambda: ops.score_cutoff(s_, E_, cs_, top_k=TOP_K, **kw)
            fns['%s: score_cutoff, top_p = %.1f' % (name, TOP_P)] = lambda: ops.score_cutoff(s_, E_, cs_, top_p=TOP_P, **kw)
            fns['%s: score_cutoff, top_k + top_p' % name] = lambda: ops.score_cutoff(s_, E_, cs_, top_k=TOP_K, top_p=TOP_P, **kw)
            fns['%s: score_cutoff, min_p = 0.01 alone (no search)' % name] = lambda: ops.score_cutoff(s_, E_, cs_, min_p=0.01, **kw)
            fns['%s: score_norm (one log-mass pass)' % name] = lambda: ops.score_norm(s_, E_, cs_, off_ex=off_, listed=lst_, drop_listed=drop_,
                                                                                       bias=bias_, group=grp_)
            fns['%s: before: materialised scores + sort + cumsum (top_p)' % name] = before
            with torch.no_grad():
                t = timed(fns, args.calls)
                floor, count, _, _ = ops.score_cutoff(s_, E_, cs_, top_p=TOP_P, **kw)
                ref_floor, ref_count = before()
            agree = 'largest |count - materialised count| %d at counts %d .. %d' % (
                int((count.long() - ref_count).abs().max()), int(count.min()), int(count.max()))
            rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
            for k in fns:
                s = summary(t[k])
                rows.append('| %s | %.1f | %.1f | %.1f |' % (k, s['median_us'], s['p10_us'], s['p90_us']))
            text += ['B %d, V %d, d %d, %s; %d timed calls per row after 5 warm-up rounds, rows alternating call by call; %s.'
                     % (B, V, d, name, args.calls, agree), ''] + rows + ['']
            del fns, keep
        del E, grouped, ws, tg
        torch.cuda.empty_cache()
    text = '\n'.join(text)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
