"""The capped top-k by hand: a plain Python loop over the slots of an ordered pool with a dict of counts per category - what
csrc/cap_select.hip (ops.cap_select, model.recommend_capped) must equal with `==`.  Also the random pools the CPU and GPU
tests share."""
import torch

NINF = float('-inf')


def capped(ids, category, caps, k):
    """(pick [B][k], kept [B], scanned [B]) as Python lists.  ids: [B][P] item ids (filled iff 0 <= id < len(category));
    category: [num_items] with c < 0 or c >= len(caps) = no category (always accepted); caps: [G].  A slot with a category is
    accepted iff fewer than caps[c] EARLIER filled slots of the session have that category; the walk stops behind the k-th
    accepted slot."""
    ids = ids.tolist() if torch.is_tensor(ids) else ids
    category = category.tolist() if torch.is_tensor(category) else category
    caps = caps.tolist() if torch.is_tensor(caps) else caps
    n, G = len(category), len(caps)
    picks, kept, scanned = [], [], []
    for row in ids:
        seen, pick, used = {}, [], len(row)
        for i, v in enumerate(row):
            if not 0 <= v < n:
                continue
            c = category[v]
            if 0 <= c < G:
                before = seen.get(c, 0)
                seen[c] = before + 1
                if before >= caps[c]:
                    continue
            pick.append(i)
            if len(pick) == k:
                used = i + 1
                break
        kept.append(len(pick))
        scanned.append(used)
        picks.append(pick + [-1] * (k - len(pick)))
    return picks, kept, scanned


def capped_lists(val, ids, category, caps, k):
    """(values [B, k], item ids [B, k]) of the pool (val, ids) under the caps: the pool's own numbers at the picks, (-inf, -1)
    in the tail - what model.recommend_capped returns for that pool"""
    pick = torch.tensor(capped(ids, category, caps, k)[0], dtype=torch.long).view(ids.shape[0], k)
    got = pick >= 0
    v = torch.where(got, val.gather(1, pick.clamp(min=0)), torch.full((), NINF, dtype=val.dtype))
    i = torch.where(got, ids.long().gather(1, pick.clamp(min=0)), torch.full((), -1, dtype=torch.long))
    return v, i.to(torch.int32)


def random_pool(B, P, G, n_items=None, seed=0, garbage=False):
    """(ids int64 [B, P], val fp32 [B, P] descending, category int32 [n_items], caps int32 [G]): categories skewed so that
    caps bind (half of the items share the first few), caps drawn from 0 .. 3, about 10 % of the items without a category,
    unfilled slots (-1) in the middle and at the end; garbage=True: some of them hold ids >= n_items and < -1 instead"""
    g = torch.Generator().manual_seed(1000 * seed + B + P + G)
    n_items = max(2 * P, 64) if n_items is None else n_items
    skew = torch.randint(0, min(G, 3), (n_items,), generator=g)
    flat = torch.randint(0, G, (n_items,), generator=g)
    category = torch.where(torch.rand(n_items, generator=g) < 0.5, skew, flat)
    category[torch.rand(n_items, generator=g) < 0.1] = -1
    if n_items > 1:
        category[1] = G - 1                                  # the last category is present
    caps = torch.randint(0, 4, (G,), generator=g)
    ids = torch.stack([torch.randperm(n_items, generator=g)[:P] if n_items >= P else torch.randint(0, n_items, (P,), generator=g)
                       for _ in range(B)])
    hole = torch.rand(B, P, generator=g) < 0.05
    hole[:, P - P // 16:] = True                             # ... and a run of them at the end
    hole[0] = hole[0] & (P == 1)                             # (session 0 has none, unless the pool is one slot)
    fill = torch.full_like(ids, -1)
    if garbage:
        junk = torch.randint(0, 4, (B, P), generator=g)
        fill = torch.where(junk == 0, torch.full_like(ids, n_items), fill)
        fill = torch.where(junk == 1, torch.full_like(ids, 2 ** 31 - 1), fill)
        fill = torch.where(junk == 2, torch.full_like(ids, -7), fill)
    ids = torch.where(hole, fill, ids)
    val = torch.sort(torch.randn(B, P, generator=g), 1, descending=True).values
    return ids, val, category.to(torch.int32), caps.to(torch.int32)
