"""CPU side of the sharded long top-N route: dist.VocabParallel.select_many over gloo with 2 ranks and a plain-torch stand-in
for the kernels built from the float64 oracle (the pattern of tests/test_cutoff_dist_cpu.py) must give select64 of the WHOLE
table - replicated and data-parallel, listed items scored and dropped, with a grouped bias, and on a rank without live rows,
which has to join the cutoff's collectives and contribute unfilled lists."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from select_oracle import select64
from test_cutoff_dist_cpu import CutoffLocal
from test_dist_cpu import FakeModel, _free_port
from test_serve_dist_cpu import B, _case
from util import pkg

KS = {300: 200, 40: 130}            # V -> k: above the selection kernel's 128; V = 40: more than the catalogue holds


class ManyLocal(CutoffLocal):
    """CutoffLocal + the select_many entry of dist.HipLocal: select64 among this shard's rows at or above the floor.  cap must
    be the largest count of the cutoff over the whole table: no shard may find more pairs than that in a session."""

    def select_many(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, floor, cap, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        out = self._floored(s, dm, floor)
        assert isinstance(cap, int) and cap >= 1 and int((~out).sum(1).max()) <= cap, (cap, (~out).sum(1).tolist())
        val, idx = select64(s.float(), k, out, id_lo)
        return val.float(), idx.to(torch.int32)


def _routes(call, k, srs, off_ex, off_in, listed, bias, group, **kw):
    srs = list(srs)
    return {(drop, biased): [t.tolist() for t in call(srs, k, off_ex, off_in, listed, drop, bias=bias if biased else None,
                                                      group=group if biased else None, **kw)]
            for drop in (False, True) for biased in (False, True)}


def _worker(rank, world, port, V, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, srs, off_ex, off_in, listed, bias, group, items, keys = _case(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=ManyLocal(V))
        shard = model._table().detach()
        call = lambda srs, *a, **kw: vp.select_many(srs, shard, None, *a, **kw)
        n = B // world
        sl = slice(rank * n, (rank + 1) * n)
        with torch.no_grad():
            out = {False: _routes(call, KS[V], srs, off_ex, off_in, listed, bias, group),
                   True: _routes(call, KS[V], srs[:, sl], off_ex[:, sl], off_in[:, sl], listed[sl], bias, group[sl],
                                 data_parallel=True)}
        q.put((rank, vp.n_live, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('V', [300, 40])
def test_sharded_select_many_two_ranks_equal_select64_of_the_whole_table(V):
    world, k = 2, KS[V]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, V, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    table, srs, off_ex, off_in, listed, bias, group, items, keys = _case(V)
    local = ManyLocal(V)

    def whole(srs, k, off_ex, off_in, listed, drop, bias=None, group=None):     # select64 of the whole table, no floor at all
        kw = {} if bias is None else dict(bias=bias, group=group)
        s, dm = local._scored(srs, table, None, off_ex, off_in, listed, drop, 0, **kw)
        val, idx = select64(s.float(), k, dm, 0)
        return val.float(), idx.to(torch.int32)
    ref = _routes(whole, k, srs, off_ex, off_in, listed, bias, group)
    if V == 300:                       # the floor is felt: full lists without a bias, and lists cut by ties or by the bias
        assert all(-1 not in row for row in ref[False, False][1])
    assert any(-1 in row for row in ref[True, True][1])
    n = B // world
    for rank, n_live, out in res:
        assert n_live == {300: (192, 108), 40: (40, 0)}[V][rank]
        for key, r in ref.items():
            assert out[False][key] == r, (V, rank, key, 'replicated')
            assert out[True][key] == [x[rank * n:(rank + 1) * n] for x in r], (V, rank, key, 'data_parallel')
