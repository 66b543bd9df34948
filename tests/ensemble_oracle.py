"""float64 restatement of the multi-table served score of csrc/ensemble.hip (include/srec_ens.h: srec_served_multi), shared by
tests/test_ensemble_cpu.py and tests/test_ensemble_gpu.py.  Everything is materialised: this is the yardstick, not the
product.  Selection, ranks and the list checks are those of select_oracle / rank_oracle over these scores."""
import torch


def scores64_multi(comps, off_ex=None, off_in=None, listed=None, id_lo=0):
    """(B, n) float64: logsumexp_c(cs_c[v] <sr_c[b], E_c[v]> + off[c, b]) over comps = [(sr [B, d_c], table [n, d_c], cs [n] or
    None), ...] - off_in for the items of listed[b, :] (global ids, -1 = empty), off_ex elsewhere; one component: z + off,
    no exp / log (rank_oracle.scores64 with a table per component)"""
    C = len(comps)
    B, n = comps[0][0].shape[0], comps[0][1].shape[0]
    z = []
    for sr, E, cs in comps:
        zc = sr.detach().double().cpu() @ E.detach().double().cpu().T
        if cs is not None:
            zc = zc * cs.detach().double().cpu()[None, :]
        z.append(zc)
    z = torch.stack(z, 0)
    zero = torch.zeros(C, B, dtype=torch.float64)
    oe = zero if off_ex is None else off_ex.detach().double().cpu().reshape(C, B)
    oi = zero if off_in is None else off_in.detach().double().cpu().reshape(C, B)
    inside = torch.zeros(B, n + 1, dtype=torch.bool)
    if listed is not None:
        lst = listed.detach().long().cpu()
        loc = lst - id_lo
        loc = torch.where((lst >= 0) & (loc >= 0) & (loc < n), loc, torch.full_like(loc, n))
        inside.scatter_(1, loc, True)
    inside = inside[:, :n]
    z = z + torch.where(inside[None], oi[:, :, None], oe[:, :, None])
    return z[0] if C == 1 else torch.logsumexp(z, dim=0)


def exact_tables(ds, B, V, seed):
    """comps with entries that are multiples of 1/8 in [-1, 1] and column scales in {0.5, 1, 2}: a different table per
    component, rows 3 / 17 duplicated in every table (equal scores: the tie rule decides)"""
    g = torch.Generator().manual_seed(seed)
    comps = []
    for d in ds:
        sr = torch.randint(-8, 9, (B, d), generator=g).float() / 8
        E = torch.randint(-8, 9, (V, d), generator=g).float() / 8
        cs = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (V,), generator=g)]
        E[17], cs[17] = E[3], cs[3]
        comps.append((sr, E, cs))
    return comps


def exact_mixture(ds, B, V, seed):
    """(comps, off, off_in, listed): the inputs of an EXACT mixture - session b's component b % C carries an offset that is a
    multiple of 1/8 and the others -1e5 (exp() of the difference is exactly 0 in fp32 and in float64, whatever the fold
    order); off_in = off + 2 on the live component; listed: 4 items and an empty slot per session"""
    C = len(ds)
    comps = exact_tables(ds, B, V, seed)
    g = torch.Generator().manual_seed(seed + 1)
    b = torch.arange(B)
    off = torch.full((C, B), -1.0e5)
    off[b % C, b] = -torch.randint(0, 9, (B,), generator=g).float() / 8
    off_in = off.clone()
    off_in[b % C, b] += 2.0
    listed = torch.stack([torch.randperm(V, generator=g)[:5] for _ in range(B)])
    listed[:, 4] = -1
    return comps, off, off_in, listed


def exact_bias(V, seed):
    """bias [2, V]: finite entries multiples of 1/8, a few -inf"""
    g = torch.Generator().manual_seed(seed + 2)
    bias = torch.randint(-8, 9, (2, V), generator=g).float() / 8
    bias[0, torch.randperm(V, generator=g)[:7]] = float('-inf')
    bias[1, torch.randperm(V, generator=g)[:7]] = float('-inf')
    return bias


def random_mixture(ds, B, V, seed):
    """random inputs at the project's scaling: sessions randn * 0.3, tables randn * 0.2, offsets in [-8, -4]"""
    g = torch.Generator().manual_seed(seed)
    C = len(ds)
    comps = [(torch.randn(B, d, generator=g) * 0.3, torch.randn(V, d, generator=g) * 0.2,
              (0.5 + torch.rand(V, generator=g)) if c % 2 else None) for c, d in enumerate(ds)]
    off = -4.0 - 4.0 * torch.rand(C, B, generator=g)
    off_in = off + torch.rand(C, B, generator=g)
    listed = torch.stack([torch.randperm(V, generator=g)[:6] for _ in range(B)])
    listed[:, 5] = -1
    return comps, off, off_in, listed
