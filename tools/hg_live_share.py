"""share of the MSHGNN layer's projected (module, row) pairs that some edge reads as its source, over bench.py's batches (CPU):
python tools/hg_live_share.py [n_batches]   - what the row lists of the 'g16' forward projections keep"""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

sp = importlib.import_module('sessionrec-pytorch_amd')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
batches, _ = bench.make_batches('MSGIFSR', 3, n, 512, 37484, 20, 123, padded=True)
layer = sp.MSGIFSR(37484, 'x', 64, 1, dropout=0.0, order=3, extra=False, fusion=False).layers[0]
tot_live = tot_listed = 0
for i, ((mg,), _) in enumerate(batches):
    plan, _ = layer.plan(mg, 64)
    live = listed = 0
    for bi, (m, t) in enumerate(plan.blocks):
        src = set()
        for (_, sb, _, gr) in plan.insts:
            if sb == bi:
                src |= set(gr[4][:int(gr[0].max())].tolist())
        live += mg.count('N%d' % (t + 1))
        listed += len(src)
    print('batch %2d: projected (block, live row) pairs %6d, with an out-edge %6d (%.3f)' % (i, live, listed, listed / live))
    tot_live, tot_listed = tot_live + live, tot_listed + listed
print('total: %d projected, %d listed: %.3f kept, %.3f skipped' % (tot_live, tot_listed, tot_listed / tot_live, 1 - tot_listed / tot_live))
