"""CPU side of the sharded cutoff: dist.VocabParallel.cutoff, and the floor it hands to select / sample, over gloo with 2 ranks
and a plain-torch stand-in for the kernels built from the float64 oracle (the pattern of tests/test_serve_dist_cpu.py) must
give what ONE call on the whole table gives - replicated and data-parallel, listed items scored and dropped, with a grouped
bias, and on a rank without live rows, which has to join every collective."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import cutoff_oracle as co
from select_oracle import select64
from test_dist_cpu import FakeModel, _free_port
from test_serve_dist_cpu import B, K, SEED, T, ServeLocal, _case
from sample_oracle import key64
from util import pkg

CRITS = (dict(top_k=3), dict(top_p=0.6), dict(min_p=0.2), dict(top_k=30, top_p=0.8, min_p=0.05), dict())


class CutoffLocal(ServeLocal):
    """ServeLocal + the cutoff entry of dist.HipLocal and the floor of select / sample.  The stand-in's partials are not the
    kernel's histograms: every shard writes the fp32 bits of its scores and an eligibility flag into its columns of a zeroed
    [B, V, 2] integer tensor, ONE reduce_sum completes it on every rank (x + 0 is exact), and the oracle runs on the whole.
    The maxima go through reduce_max and must agree with it - so both collectives carry what the result depends on, and a
    rank that skipped one would hang or fail."""

    def __init__(self, V):
        self.V = V

    def cutoff(self, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, crit, reduce_max, reduce_sum, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        Bn, n = s.shape
        elig = torch.ones(Bn, n, dtype=torch.bool) if dm is None else ~dm
        s32 = s.float()
        own = torch.where(elig, s32, torch.full_like(s32, co.NINF))
        top = own.max(1).values if n > 0 else torch.full((Bn,), co.NINF)
        top = reduce_max(top.clone())
        full = torch.zeros(Bn, self.V, 2, dtype=torch.int64)
        full[:, id_lo:id_lo + n, 0] = s32.contiguous().view(torch.int32).long()
        full[:, id_lo:id_lo + n, 1] = elig.long()
        full = reduce_sum(full)
        s_all = full[..., 0].to(torch.int32).view(torch.float32).double()
        dm_all = full[..., 1] == 0
        Tq = crit['temperature']
        w, m = co.weights64(s_all, dm_all, Tq)
        assert torch.equal(m.float() + 0.0, top + 0.0), 'the MAX all-reduce did not carry the maxima'
        kw = {k: v for k, v in crit.items() if k != 'temperature'}
        floor = co.floor64(s_all, dm_all, Tq, **kw)
        return (floor.float(), co.count64(s_all, dm_all, floor).to(torch.int32), co.kept64(s_all, dm_all, Tq, floor).float(),
                top + 0.0)

    def _floored(self, s, dm, floor):
        below = s.float() < floor.float()[:, None]
        return below if dm is None else dm | below

    def select(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, floor=None, **bias):
        if floor is None:
            return super().select(srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        val, idx = select64(s.float(), k, self._floored(s, dm, floor), id_lo)
        return val.float(), idx.to(torch.int32)

    def sample(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, temperature, seed, session_keys, floor=None,
               **bias):
        if floor is None:
            return super().sample(srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, temperature, seed, session_keys,
                                  **bias)
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        val, idx = select64(key64(s.float(), temperature, seed, session_keys, id_lo).float(), k, self._floored(s, dm, floor), id_lo)
        return val.float(), idx.to(torch.int32)


def _routes(call, srs, off_ex, off_in, listed, bias, group, keys, drop, **kw):
    """{(criteria index, route): lists}: the cutoff, and a selection and a draw inside it"""
    srs, out = list(srs), {}
    for i, crit in enumerate(CRITS):
        cut = call('cutoff', srs, off_ex, off_in, listed, drop, bias=bias, group=group, temperature=T, **crit, **kw)
        out[i, 'cutoff'] = [t.tolist() for t in cut]
        out[i, 'select'] = [t.tolist() for t in call('select', srs, K, off_ex, off_in, listed, drop, bias=bias, group=group,
                                                     floor=cut[0], **kw)]
        out[i, 'sample'] = [t.tolist() for t in call('sample', srs, K, off_ex, off_in, listed, drop, bias=bias, group=group,
                                                     temperature=T, seed=SEED, session_keys=keys, floor=cut[0], **kw)]
    return out


def _worker(rank, world, port, V, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, srs, off_ex, off_in, listed, bias, group, items, keys = _case(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=CutoffLocal(V))
        shard = model._table().detach()
        call = lambda name, srs, *a, **kw: getattr(vp, name)(srs, shard, None, *a, **kw)
        n = B // world
        sl = slice(rank * n, (rank + 1) * n)
        out = {}
        with torch.no_grad():
            for drop in (False, True):
                out[drop, False] = _routes(call, srs, off_ex, off_in, listed, bias, group, keys, drop)
                out[drop, True] = _routes(call, srs[:, sl], off_ex[:, sl], off_in[:, sl], listed[sl], bias, group[sl], keys[sl],
                                          drop, data_parallel=True)
        q.put((rank, vp.n_live, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('V', [150, 40])
def test_sharded_cutoff_two_ranks_equal_unsharded(V):
    world = 2
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
    local = CutoffLocal(V)
    same = lambda t: t

    def whole(name, srs, *a, **kw):                                  # one call on the whole table, id_lo 0
        if name == 'cutoff':
            crit = {k: kw.pop(k) for k in ('top_k', 'top_p', 'min_p', 'temperature') if k in kw}
            return local.cutoff(srs, table, None, *a, 0, crit, same, same, **kw)
        return getattr(local, name)(srs, table, None, *a, 0, **kw)
    n = B // world
    for rank, n_live, out in res:
        assert n_live == {150: (128, 22), 40: (40, 0)}[V][rank]
        for drop in (False, True):
            ref = _routes(whole, srs, off_ex, off_in, listed, bias, group, keys, drop)
            counts = ref[1, 'cutoff'][1]
            assert 0 < min(counts) and max(counts) < V - 5, 'the nucleus of the case keeps nothing or everything'
            assert any(-1 in row for row in ref[0, 'select'][1]), 'no kept set is smaller than K: the floor is not felt'
            for key, r in ref.items():
                assert out[drop, False][key] == r, (V, rank, drop, key, 'replicated')
                assert out[drop, True][key] == [x[rank * n:(rank + 1) * n] for x in r], (V, rank, drop, key, 'data_parallel')
