"""bench.py's plain run: exactly --steps timed steps, the headline fields only, and --dump-outputs writing what the last
timed step computed - the same arrays in two runs of the same arguments (seeded inputs and weights, deterministic kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import ROOT

pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_bench_line_and_dumped_outputs(dev, tmp_path):
    runs = []
    for tag in ('a', 'b'):
        out = _bench(['--gpus', '1', '--steps', '4', '--warmup', '2', '--dump-outputs', str(tmp_path / tag)])
        runs.append((out, _load(str(tmp_path / tag))))
    out, arrs = runs[0]
    assert out['steps'] == 4 and out['warmup'] == 2 and out['full'] is False
    assert len(out['repeats_ms_per_step']) == 1 and out['ms_per_step'] == out['repeats_ms_per_step'][0] > 0
    assert out['value'] == pytest.approx(512 / (out['ms_per_step'] * 1e-3), rel=1e-9)
    assert out['unit'] == 'sessions/s' and out['higher_is_better'] is True and out['dtype'].startswith('bf16')
    assert all(out[k] is None for k in ('roofline', 'cpu_baseline', 'fp32', 'end_to_end', 'quality'))
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
    assert arrs['loss'].shape == (1,) and float(arrs['loss'][0]) == np.float32(out['config']['final_loss'])
    assert arrs['param.embeddings.weight.rows_sample'].shape == (8192, 256)
    assert len(arrs) > 50                                  # the loss and every parameter of the MSGIFSR step
    out_b, arrs_b = runs[1]
    assert sorted(arrs_b) == sorted(arrs)
    for k, a in arrs.items():
        assert np.array_equal(a, arrs_b[k]), k
