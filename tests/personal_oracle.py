"""The per-session list merge of csrc/personal.hip (ops.personal_merge) as a plain Python loop, and the random cases the CPU
and GPU tests share.  Everything is compared with `==`: the values are copied, or formed by one fp32 add (torch.float32 here,
so that the bits compare)."""
import torch

NINF = float('-inf')
BIASES = [NINF, -3.0, -0.5, 0.0, 0.5, 4.0]


def new_values(base, bias):
    """t [B, M] fp32: base + bias in fp32, -inf everywhere without a bias"""
    base = base.to(torch.float32)
    return torch.full_like(base, NINF) if bias is None else base + bias.to(torch.float32)


def merge(pool_ids, pool_val, items, base, bias, k):
    """(val fp32 [B,k], ids int32 [B,k], src int32 [B,k], hit [B], kept [B]) of the contract in include/srec.h: integer
    tensors of ids (a slot is filled iff id >= 0), fp32 values, bias fp32 or None; on the CPU"""
    B, P = pool_ids.shape
    M = items.shape[1]
    t = new_values(base, bias)
    val = torch.full((B, k), NINF, dtype=torch.float32)
    ids = torch.full((B, k), -1, dtype=torch.int32)
    src = torch.full((B, k), -1, dtype=torch.int32)
    hit, kept = [], []
    pid, pv, it, tv = pool_ids.tolist(), pool_val.tolist(), items.tolist(), t.tolist()
    for b in range(B):
        first = {}
        for j in range(M):
            if it[b][j] >= 0:
                first.setdefault(it[b][j], j)
        survivors = [(-pv[b][i], pid[b][i], i) for i in range(P) if pid[b][i] >= 0 and pid[b][i] not in first]
        hit.append(sum(1 for i in range(P) if pid[b][i] >= 0 and pid[b][i] in first))
        candidates = [(-tv[b][j], v, P + j) for v, j in first.items() if tv[b][j] > NINF]
        out = sorted(survivors + candidates, key=lambda e: (e[0] + 0.0, e[1]))[:k]
        kept.append(len(out))
        for r, (_, v, s) in enumerate(out):
            ids[b, r], src[b, r] = v, s
            val[b, r] = pool_val[b, s] if s < P else t[b, s - P]
    return val, ids, src, torch.tensor(hit, dtype=torch.int32), torch.tensor(kept, dtype=torch.int32)


def complete(hit, pool_ids, k):
    """bool [B]: the rule under which the merge is the exact top-k of the adjusted catalogue"""
    return (hit.long() <= pool_ids.shape[1] - k) | (pool_ids[:, -1] < 0)


def random_case(B, P, M, seed=0, bias=True):
    """(pool_ids int64 [B,P], pool_val fp32 [B,P], items int64 [B,M], base fp32 [B,M], bias fp32 [B,M] or None): ordered pools
    with holes in the middle and at the end (equal values in every other session), lists drawn mostly from the pool's head,
    shuffled, with -1 padding, the base of a pool item being its pool value, biases from BIASES"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * P + M)
    n = P + M + 50
    pool_ids = torch.full((B, P), -1, dtype=torch.int64)
    pool_val = torch.full((B, P), 7.0)                           # (the value of an unfilled slot is never looked at)
    items = torch.full((B, M), -1, dtype=torch.int64)
    base = torch.randn(B, M, generator=g) - 1.0
    for b in range(B):
        f = P if P < 3 else int(torch.randint((P + 1) // 2, P + 1, (1,), generator=g))
        ident = torch.randperm(n, generator=g)[:f]
        v = torch.randn(f, generator=g)
        if b % 2:
            v = (v * 2).round() / 2                              # ties (and -0.0 beside +0.0)
        order = sorted(range(f), key=lambda i: (-float(v[i]) + 0.0, int(ident[i])))
        at = torch.randperm(P, generator=g)[:f].sort().values
        pool_ids[b, at] = ident[order]
        pool_val[b, at] = v[order]
        m = M if M < 3 else int(torch.randint(M // 2, M + 1, (1,), generator=g))
        head = ident[order][:min(f, 2 * M)]
        inside = head[torch.randperm(head.numel(), generator=g)][:max(1, (3 * m) // 4)]
        rest = torch.tensor(sorted(set(range(n)) - set(ident.tolist())))
        outside = rest[torch.randperm(rest.numel(), generator=g)][:m - inside.numel()]
        chosen = torch.cat([inside, outside])
        chosen = chosen[torch.randperm(chosen.numel(), generator=g)]
        slots = torch.randperm(M, generator=g)[:chosen.numel()]
        items[b, slots] = chosen
        where = {int(i): float(x) for i, x in zip(ident[order], v[order])}
        for j in slots.tolist():
            if int(items[b, j]) in where:
                base[b, j] = where[int(items[b, j])]
        if M > 3:
            base[b, slots[0]] = NINF                             # (a seen / filtered item: out whatever its bias)
    bs = torch.tensor(BIASES)[torch.randint(0, len(BIASES), (B, M), generator=g)] if bias else None
    return pool_ids, pool_val, items, base, bs


def dense_top(row, n):
    """([ids], [values]) of the n best entries > -inf of a dense fp32 row by (value descending, id ascending)"""
    vals = row.tolist()
    order = sorted((i for i in range(len(vals)) if vals[i] > NINF), key=lambda i: (-vals[i] + 0.0, i))[:n]
    return order, [vals[i] for i in order]
