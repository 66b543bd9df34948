"""Timing of the calibrated re-rank (csrc/calibrate.hip, ops.calibrate, model.recommend_calibrated) at the serving shape - B 512
sessions, pools of M 128 slots, K 20 picks, T 12 target pairs, a table of V 37 484 rows of d 256 - beside a composition of the
same greedy in PyTorch and beside the selection that makes the pool: median of N device-event timed calls after warm-up, the
candidates alternating call by call, p10 / p90 as the spread.
  (a) ops.calibrate alone (one launch), k 20 and k 128, weight 0.5
  (b) the composition in PyTorch on the same pools: float64, a host loop of k rounds over [B, M, T] temporaries
  (c) SRGNN end to end: recommend(k=pool) beside recommend_calibrated(k=20) of the same pool, the target being the session's
      own items
Prints a markdown table (and writes it with --out).
usage (GPU box, under its own time limit):  timeout -k 10 300 python tools/calibrate_timing.py --out profiles/calibrate_timing.md"""
import argparse
import importlib
import os
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, 'tools'))
import torch

from rank_timing import summary, synth_samples, timed


def torch_calibrated(ids, val, category, tcat, tw, k, weight, alpha):
    """the composition ops.calibrate replaces: (val [B,k], pick [B,k], kl [B]) - the same greedy, float64, k rounds of small
    launches.  The calibration term is formed once per target pair (the first pair of a category stands for it)"""
    B, M = ids.shape
    n_items = category.numel()
    w, a = float(torch.tensor(weight, dtype=torch.float32)), float(torch.tensor(alpha, dtype=torch.float32))
    filled = (ids >= 0) & (ids < n_items)
    cat = torch.where(filled, category[ids.clamp(0, n_items - 1).long()].long(), torch.full_like(ids, -1, dtype=torch.long))
    valid = (tcat >= 0) & (tw > 0)
    twd = torch.where(valid, tw.double(), torch.zeros_like(tw, dtype=torch.float64))
    same = (tcat[:, :, None] == tcat[:, None, :]) & valid[:, :, None] & valid[:, None, :]          # [B, T, T]
    P = (same * twd[:, None, :]).sum(2)
    first = valid & ~torch.tril(same, -1).any(2)                                                    # one pair per category of S
    W = twd.sum(1, keepdim=True)
    target = W > 0
    p = torch.where(first & target, P / W.clamp(min=1e-300), torch.zeros_like(P))                  # [B, T], 0: not a class
    match = (cat[:, :, None] == tcat[:, None, :].long()) & (p > 0)[:, None, :]                     # [B, M, T]
    s = val.double()
    n = torch.zeros_like(p)
    N = torch.zeros(B, 1, dtype=torch.float64, device=ids.device)
    avail = filled.clone()
    pos = torch.arange(M, device=ids.device)[None].expand(B, M)
    ninf = torch.full_like(s, float('-inf'))

    def term(n, D):
        return torch.where(p > 0, p * torch.log(p.clamp(min=1e-300) / ((1.0 - a) * n / D + a * p).clamp(min=1e-300)), torch.zeros_like(p))
    picks = []
    for _ in range(k):
        t_out = term(n, N + 1)
        kl_none, kl_out = term(n, N.clamp(min=1)).sum(1, keepdim=True), t_out.sum(1, keepdim=True)
        delta = term(n + 1, N + 1) - t_out
        kl = torch.where(cat < 0, kl_none, kl_out + (match * delta[:, None, :]).sum(2))
        m = s if w == 0 else torch.where(s == float('-inf'), ninf, (1.0 - w) * s - w * kl)
        m = torch.where(avail, m, ninf)
        best = m.max(1, keepdim=True).values
        i = torch.where(avail & (m == best), pos, torch.full_like(pos, M)).min(1).values          # the lower slot of equals
        got = i < M
        i = i.clamp(max=M - 1)
        picks.append(torch.where(got, i, torch.full_like(i, -1)))
        hit = torch.zeros_like(avail).scatter_(1, i[:, None], got[:, None])
        avail = avail & ~hit
        n = n + (match & hit[:, :, None]).sum(1)
        N = N + (hit & (cat >= 0)).sum(1, keepdim=True)
    pick = torch.stack(picks, 1)
    out = torch.where(pick < 0, torch.full_like(val[:, :k], float('-inf')), val.gather(1, pick.clamp(min=0)))
    return out, pick.to(torch.int32), term(n, N.clamp(min=1)).sum(1).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=31)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.calls >= 30, 'the median of at least 30 timed calls'
    assert torch.cuda.is_available(), 'calibrate_timing needs the GPU: there is nothing to fall back to'
    ops = importlib.import_module('sessionrec-pytorch_amd.ops')
    sp = importlib.import_module('sessionrec-pytorch_amd')
    col = importlib.import_module('sessionrec-pytorch_amd.collate')
    dev = torch.device('cuda:0')
    B, V, d, G, T = 512, 37484, 256, 40, 12
    torch.manual_seed(1)
    g = torch.Generator().manual_seed(2)
    category = torch.randint(-1, G, (V,), generator=g).to(torch.int32).to(dev)
    tcat = torch.randint(-1, 10, (B, T), generator=g).to(torch.int32).to(dev)
    tw = (torch.rand(B, T, generator=g) + 0.05).to(dev)
    model = sp.SRGNN(V, d, 1).to(dev).eval()
    inputs, _ = col.collate_fn_factory(col.seq_to_session_graph)(synth_samples(B, V, 123))
    mg = inputs[0].to(dev)
    with torch.no_grad():
        v128, i128 = model.recommend(mg, k=128)
        same = []
        for k in (20, 128):
            got, ref = ops.calibrate(i128, v128, category, k, 0.5, tcat, tw, checked=True), torch_calibrated(i128, v128, category, tcat, tw, k, 0.5, 0.01)
            same.append('%d of %d sessions' % (int((got[1] == ref[1]).all(1).sum()), B))
        plain = model.recommend(mg, k=20)[1]
        slate, kl = model.recommend_calibrated(mg, k=20, weight=0.5, item_category=category, return_kl=True)[1:]
        kl_plain = model.list_calibration(mg, item_ids=plain, item_category=category)
        fns = {
            '(a) ops.calibrate k=20 of M=128, T=12': lambda: ops.calibrate(i128, v128, category, 20, 0.5, tcat, tw, checked=True),
            '(a) ops.calibrate k=128 of M=128, T=12': lambda: ops.calibrate(i128, v128, category, 128, 0.5, tcat, tw, checked=True),
            '(a\') ops.calibrate k=20 with its checks (one device-to-host read)': lambda: ops.calibrate(i128, v128, category, 20, 0.5, tcat, tw),
            '(b) PyTorch composition k=20 of M=128, T=12': lambda: torch_calibrated(i128, v128, category, tcat, tw, 20, 0.5, 0.01),
            '(c) SRGNN recommend k=20': lambda: model.recommend(mg, k=20),
            '(c) SRGNN recommend k=80 (the default pool of k=20)': lambda: model.recommend(mg, k=80),
            '(c) SRGNN recommend_calibrated k=20 (pool 80, target: the session\'s items)':
                lambda: model.recommend_calibrated(mg, k=20, weight=0.5, item_category=category),
            '(c) SRGNN recommend k=128': lambda: model.recommend(mg, k=128),
            '(c) SRGNN recommend_calibrated k=20, pool=128': lambda: model.recommend_calibrated(mg, k=20, weight=0.5, item_category=category, pool=128),
        }
        t = timed(fns, args.calls)
        slow = {'(b) PyTorch composition k=128 of M=128, T=12': lambda: torch_calibrated(i128, v128, category, tcat, tw, 128, 0.5, 0.01)}
        t.update(timed(slow, args.calls, warmup=2))
        fns.update(slow)
    rows = ['| call | median us | p10 us | p90 us |', '|---|---|---|---|']
    for name in fns:
        s = summary(t[name])
        rows.append('| %s | %.1f | %.1f | %.1f |' % (name, s['median_us'], s['p10_us'], s['p90_us']))
    text = '\n'.join(['B %d, V %d, d %d, %d categories, weight 0.5, alpha 0.01; %d timed calls per row after warm-up rounds, rows '
                      'alternating call by call (the k=128 composition in a round of its own); kernel picks equal to the float64 '
                      'PyTorch composition at k=20 / k=128: %s / %s; sessions whose calibrated top 20 differs from the plain one: '
                      '%d of %d; mean KL to the session\'s own mix: plain %.4f, calibrated %.4f'
                      % (B, V, d, G, args.calls, same[0], same[1], int((slate != plain).any(1).sum()), B, float(kl_plain.mean()),
                         float(kl.mean())), ''] + rows)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
