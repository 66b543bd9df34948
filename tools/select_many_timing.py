"""Timing and peak memory of top-N lists beyond 128 items (csrc/select_many.hip: ops.score_select_many = the top_k cutoff + the
collect pass + the order kernel) beside the route it replaces - the materialised (B, V) scores and torch.topk(k) - at the
benchmarked shape (B 512, V 37 484, d 256), k in {256, 1000, 4096}: median of N device-event timed calls after warm-up, all
rows alternating call by call, p10 / p90 as the spread; peak memory = the rise of torch.cuda.max_memory_allocated over one
call after the warm-up (scratch that the calls cache is allocated by then and is reported beside it).
  C = 1, no bias, no list
  C = 3 mixture, bias [4, V] with random groups, a 20-item list per session, dropped
Per configuration and k: the whole score_select_many, its collect pass and its order kernel alone (on the floor and the buffer
the call itself produced), and the materialised route.
--big adds the per-rank shard shape of a 10 M item catalogue on 8 ranks (V 1 250 000), C = 1.
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 500 python tools/select_many_timing.py --big --out profiles/select_many_timing.md"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, timed

KS = (256, 1000, 4096)


def peak_rise(fn):
    """bytes by which one call raises the allocator's peak over what is allocated going in (the call has run before: cached
    scratch does not count)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--big', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'select_many_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    sc = importlib.import_module('sessionrec-pytorch_amd.score')
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

        def materialised1(k):
            return lambda: ops.score_logp(sr, E, cs, ws, 1.0).topk(k)

        def materialised3(k):
            def run():
                z = torch.logsumexp(torch.stack([ops.score_logp(srs[c], E, cs, ws, 1.0) + off_ex[c][:, None] for c in range(C)], 0), 0)
                z = z + grouped[group.long()]
                return z.scatter(1, listed.long(), float('-inf')).topk(k)
            return run
        configs = [('C=1', (sr, E, cs, None, None, False, None, None), materialised1)]
        if V < 100000:
            configs.append(('C=3, bias [4, V], 20 listed items dropped', (srs, E, cs, nex, listed, True, grouped, group), materialised3))
        for name, (s_, E_, cs_, off_, lst_, drop_, bias_, grp_), before in configs:
            kw = dict(off_ex=off_, listed=lst_, drop_listed=drop_, bias=bias_, group=grp_)
            a = sc._served_args('timing', s_, E_, cs_, off_, None, lst_, drop_, 0, bias_, grp_)
            fns, mem, agree = {}, {}, []
            for k in KS:
                with torch.no_grad():
                    floor, count, _, _ = ops.score_cutoff(s_, E_, cs_, top_k=k, **kw)
                    cap = int(count.max())
                    bv, bi, n, capq = sc._collect_many(a, floor, cap)
                    bv, bi, n = bv.clone(), bi.clone(), n.clone()       # (the timed calls reuse the scratch these are views of)
                    val, idx = ops.score_select_many(s_, E_, cs_, k, **kw)
                    rv, ri = before(k)()
                agree.append('k %d: counts %d .. %d, %d of %d ids equal to topk\'s' % (
                    k, int(count.min()), int(count.max()), int((idx.long() == ri).sum()), idx.numel()))
                many = lambda k=k: ops.score_select_many(s_, E_, cs_, k, **kw)
                fns['%s, k %d: score_select_many' % (name, k)] = many
                fns['%s, k %d: collect pass alone' % (name, k)] = lambda floor=floor, cap=cap: sc._collect_many(a, floor, cap)
                fns['%s, k %d: order kernel alone' % (name, k)] = lambda bv=bv, bi=bi, n=n, capq=capq, k=k: sc._order_many(bv, bi, n, capq, k)
                fns['%s, k %d: before: materialised scores + torch.topk' % (name, k)] = before(k)
                with torch.no_grad():
                    many()
                    mem['%s, k %d: score_select_many' % (name, k)] = peak_rise(many)
                    mem['%s, k %d: before: materialised scores + torch.topk' % (name, k)] = peak_rise(before(k))
            with torch.no_grad():
                t = timed(fns, args.calls)
            rows = ['| call | median us | p10 us | p90 us | peak memory MB |', '|---|---|---|---|---|']
            for key in fns:
                s = summary(t[key])
                rows.append('| %s | %.1f | %.1f | %.1f | %s |' % (key, s['median_us'], s['p10_us'], s['p90_us'],
                                                                   '%.1f' % (mem[key] / 2 ** 20) if key in mem else ''))
            cached = sum(w.numel() for w in sc._MANY_WS.values()) + sum(w.numel() for w in sc._CUTOFF_WS.values())
            text += ['B %d, V %d, d %d, %s; %d timed calls per row after 5 warm-up rounds, rows alternating call by call; %s.  '
                     'Peak memory: the rise of the allocator\'s peak over one call; the scratch score_select_many caches between '
                     'calls (collect buffers, cutoff workspace) holds %.1f MB more by now; one (B, V) fp32 matrix is %.1f MB.'
                     % (B, V, d, name, args.calls, '; '.join(agree), cached / 2 ** 20, B * V * 4 / 2 ** 20), ''] + rows + ['']
            del fns
        del E, grouped, ws, tg
        torch.cuda.empty_cache()
    text = '\n'.join(text)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
