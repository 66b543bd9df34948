"""CPU side of the sharded serving routes: dist.VocabParallel.select / sample / score_items / norm over gloo with 2 ranks
(plain-torch stand-in for the kernels, as tests/test_rank_cpu.py) must give what ONE call on the whole table gives -
replicated and data-parallel, listed items scored and dropped, with a grouped bias, and on a rank without live rows (the
neutral branch of every route)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from item_bias_oracle import NINF, bias_rows
from items_oracle import items64
from norm_oracle import norm64
from sample_oracle import key64
from select_oracle import drop_mask, scores64, select64
from test_dist_cpu import FakeModel, TorchLocal, _free_port
from util import pkg

D, B, C, L, M, K, T, SEED = 16, 8, 2, 4, 6, 5, 0.5, 9
ROUTES = ('select', 'sample', 'items', 'items1d', 'norm')
TOL_NORM = 1e-5             # fewer than ten fp32 roundings of values below 16: 10 * 16 * 2^-24


class ServeLocal(TorchLocal):
    """TorchLocal + the select / sample / score_items / norm entries of dist.HipLocal, from the float64 oracles.  Scores and
    sampled keys are rounded to fp32 BEFORE selection: two values that round together tie here as they do in
    VocabParallel._merge_lists, on a shard and on the whole table alike."""

    def _scored(self, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, bias=None, group=None):
        """(s float64 [B, n] with the bias added, ineligible bool [B, n] or None); bias: this shard's columns"""
        n = table.shape[0]
        if drop_listed:
            s, dm = scores64(srs, table, cs, off_ex, None, None, id_lo), drop_mask(listed, n, id_lo)
        else:
            s, dm = scores64(srs, table, cs, off_ex, off_in, listed, id_lo), None
        if bias is not None:
            rows = bias_rows(bias, group, s.shape[0], 0, n)
            s = s + rows
            dm = (rows == NINF) if dm is None else dm | (rows == NINF)
        return s, dm

    def select(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        val, idx = select64(s.float(), k, dm, id_lo)
        return val.float(), idx.to(torch.int32)

    def sample(self, srs, table, cs, k, off_ex, off_in, listed, drop_listed, id_lo, temperature, seed, session_keys, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        val, idx = select64(key64(s.float(), temperature, seed, session_keys, id_lo).float(), k, dm, id_lo)
        return val.float(), idx.to(torch.int32)

    def score_items(self, srs, table, cs, items, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias)
        return items64(s.float(), items, id_lo, dm).float()

    def norm(self, srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo, **bias):
        s, dm = self._scored(srs, table, cs, off_ex, off_in, listed, drop_listed, id_lo)
        return norm64(s.float(), bias.get('bias'), bias.get('group'), dm).float()


def _case(V):
    g = torch.Generator().manual_seed(31 + V)
    eighth = lambda *shape: torch.randint(-8, 9, shape, generator=g).float() / 8      # exact products and sums
    table, srs = eighth(V, D), eighth(C, B, D)
    off_ex = -eighth(C, B).abs()
    off_in = off_ex + 0.5
    listed = torch.randint(0, V, (B, L), generator=g)
    listed[:, 3] = -1
    bias = eighth(2, V) * 2
    bias[0, ::5] = NINF
    bias[1, 1::3] = NINF
    group = torch.arange(B) % 2
    items = torch.randint(-1, V, (B, M), generator=g)
    keys = torch.arange(B) * 7 + 3
    return table, srs, off_ex, off_in, listed, bias, group, items, keys


def _routes(call, srs, off_ex, off_in, listed, bias, group, items, shared, keys, drop, **kw):
    """the routes through `call(name, *args)`: {route: result}; shared: the 1-D item list every session (and rank) scores;
    kw: data_parallel for the sharded calls"""
    srs = list(srs)
    return {
        'select': call('select', srs, K, off_ex, off_in, listed, drop, bias=bias, group=group, **kw),
        'sample': call('sample', srs, K, off_ex, off_in, listed, drop, bias=bias, group=group, temperature=T, seed=SEED,
                       session_keys=keys, **kw),
        'items': call('score_items', srs, items, off_ex, off_in, listed, drop, bias=bias, group=group, **kw),
        'items1d': call('score_items', srs, shared, off_ex, off_in, listed, drop, bias=bias, group=group, **kw),
        'norm': call('norm', srs, off_ex, off_in, listed, drop, bias=bias, group=group, **kw),
    }


def _lists(res):
    return {k: [t.tolist() for t in v] if isinstance(v, tuple) else v.tolist() for k, v in res.items()}


def _worker(rank, world, port, V, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        table, srs, off_ex, off_in, listed, bias, group, items, keys = _case(V)
        model = FakeModel(table)
        vp = pkg('dist').VocabParallel(model, local=ServeLocal())
        shard = model._table().detach()
        call = lambda name, srs, *a, **kw: getattr(vp, name)(srs, shard, None, *a, **kw)
        n = B // world
        sl = slice(rank * n, (rank + 1) * n)
        out = {}
        with torch.no_grad():
            for drop in (False, True):
                out[drop, False] = _lists(_routes(call, srs, off_ex, off_in, listed, bias, group, items, items[0], keys, drop))
                out[drop, True] = _lists(_routes(call, srs[:, sl], off_ex[:, sl], off_in[:, sl], listed[sl], bias, group[sl],
                                                 items[sl], items[0], keys[sl], drop, data_parallel=True))
        q.put((rank, vp.n_live, out))
    finally:
        dist.destroy_process_group()


def _assert_route(route, got, ref, what):
    if route != 'norm':
        assert got == ref, (what, got, ref)                    # bit for bit, ids included
        return
    got, ref = torch.tensor(got, dtype=torch.float64), torch.tensor(ref, dtype=torch.float64)
    off = ref == NINF
    assert torch.equal(got == NINF, off), (what, got, ref)
    err = float((got - ref)[~off].abs().max()) if not bool(off.all()) else 0.0
    assert err <= TOL_NORM, (what, err)


@pytest.mark.parametrize('V', [150, 40])
def test_sharded_serving_routes_two_ranks_equal_unsharded(V):
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
    local = ServeLocal()
    whole = lambda name, srs, *a, **kw: getattr(local, name)(srs, table, None, *a, 0, **kw)      # one call, id_lo 0
    n = B // world
    for rank, n_live, out in res:
        assert n_live == {150: (128, 22), 40: (40, 0)}[V][rank]
        for drop in (False, True):
            ref = _lists(_routes(whole, srs, off_ex, off_in, listed, bias, group, items, items[0], keys, drop))
            if drop:
                assert any(v == NINF for row in ref['items'] for v in row)
            for route in ROUTES:
                r = ref[route]
                _assert_route(route, out[drop, False][route], r, (V, rank, drop, route, 'replicated'))
                cut = [x[rank * n:(rank + 1) * n] for x in r] if route in ('select', 'sample') else r[rank * n:(rank + 1) * n]
                _assert_route(route, out[drop, True][route], cut, (V, rank, drop, route, 'data_parallel'))
