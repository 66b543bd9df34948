"""Training / evaluation harness - host-side mirror of /root/reference/src/utils/train.py:
fix_weight_decay :12-23, prepare_batch :26-32, evaluate :36-55 (returns (MRR@k, HR@k) in that
order), TrainRunner :56-127 (Adam + StepLR(3, 0.1), log strings, early stop when BOTH metrics drop).

On a GPU model the step goes through `model.fused_loss` (scoring GEMM + softmax-CE fused, logits
never materialised) and FusedAdam; the reference-style path `nll_loss(model(*inputs), labels)`
still works on the same modules (forward() returns (B, num_items) log-probabilities).
"""
import time

import torch as th
from torch import nn, optim


def fix_weight_decay(model):
    decay, no_decay = [], []
    for name, param in model.named_parameters():
        if not param.requires_grad:
            continue
        if any(tag in name for tag in ('bias', 'batch_norm', 'activation')):
            no_decay.append(param)
        else:
            decay.append(param)
    return [{'params': decay}, {'params': no_decay, 'weight_decay': 0}]


def prepare_batch(batch, device):
    inputs, labels = batch
    return [x.to(device) for x in inputs], labels.to(device, non_blocking=labels.is_pinned())


def metrics_from_ranks(ranks, cutoffs):
    """{'hit@k', 'mrr@k', 'ndcg@k' for k in cutoffs} from the labels' ranks (0 = the label is the best item): hit = rank < k,
    mrr = 1 / (rank + 1) and ndcg = 1 / log2(rank + 2) inside the cutoff, 0 outside, averaged over the sessions.  A rank of
    -1 (a session without a label) is left out of numerator and denominator."""
    r = th.as_tensor(ranks).detach().reshape(-1).to('cpu', th.float64)
    r = r[r >= 0]
    n = max(int(r.numel()), 1)
    out = {}
    for k in cutoffs:
        k = int(k)
        inside = r < k
        out['hit@%d' % k] = float(inside.sum()) / n
        out['mrr@%d' % k] = float((1.0 / (r[inside] + 1.0)).sum()) / n
        out['ndcg@%d' % k] = float((1.0 / th.log2(r[inside] + 2.0)).sum()) / n
    return out


def ranks_from_scores(scores, labels):
    """the labels' ranks in a materialised (B, V) score matrix under the rule of the fused kernels: an item is ahead of the
    label if it scores higher, or the same with a lower id; the label itself never counts; label < 0 -> -1"""
    lab = labels.long()
    safe = lab.clamp(min=0)
    t = scores.gather(1, safe.unsqueeze(1))
    ids = th.arange(scores.shape[1], device=scores.device).unsqueeze(0)
    ahead = (scores > t) | ((scores == t) & (ids < safe.unsqueeze(1)))
    ahead &= ids != safe.unsqueeze(1)
    return th.where(lab >= 0, ahead.sum(1), th.full_like(lab, -1))


def metrics_from_served_ranks(ranks, cutoffs):
    """metrics_from_ranks for the ranks of model.served_rank: the same keys plus 'shown', the share of the labelled sessions
    whose label COULD be shown (rank >= 0).  A rank of -2 (the label is filtered out: seen, denied, below the truncation
    floor) is a miss at every cutoff and stays in the denominator; -1 (no label) is left out of both."""
    r = th.as_tensor(ranks).detach().reshape(-1).to('cpu', th.float64)
    r = r[r != -1]
    n = max(int(r.numel()), 1)
    shown = r >= 0
    out = {}
    for k in cutoffs:
        k = int(k)
        inside = shown & (r < k)
        out['hit@%d' % k] = float(inside.sum()) / n
        out['mrr@%d' % k] = float((1.0 / (r[inside] + 1.0)).sum()) / n
        out['ndcg@%d' % k] = float((1.0 / th.log2(r[inside] + 2.0)).sum()) / n
    out['shown'] = float(shown.sum()) / n
    return out


def served_ranks_from_scores(scores, labels, item_bias=None, item_group=None, seen=None, top_k=None, top_p=None, min_p=None,
                             temperature=1.0):
    """model.served_rank from a materialised (B, V) score matrix (a CPU model's forward()): int64 [B] with its -1 / -2
    convention.  item_bias [V] or [G, V] (item_group [B]) is added to the scores, -inf = not in the catalogue; seen [B, L] item
    ids (-1 = empty) are not eligible; top_k / top_p / min_p at `temperature` as model.cutoff() defines them, on the eligible
    rows.  Ties go towards the lower id (ranks_from_scores)."""
    return item_ranks_from_scores(scores, labels.reshape(-1, 1), item_bias, item_group, seen, top_k, top_p, min_p, temperature)[:, 0]


def _seen_items(who, model, inputs, kw):
    """the materialised routes' `seen`: exclude_seen taken OUT of the keywords kw; when set, the model's own view of every
    session's items (model._session_items), None otherwise"""
    if not kw.pop('exclude_seen', False):
        return None
    if not hasattr(model, '_session_items'):
        raise ValueError('%s: exclude_seen on the materialised route needs model._session_items' % who)
    return model._session_items(inputs[0])


def evaluate_served(model, data_loader, device, cutoffs=(20,), **served):
    """metrics_from_served_ranks over a data loader: HR / MRR / NDCG @cutoffs and 'shown' of what users are SHOWN - under
    served = the keywords of model.served_rank (exclude_seen, item_bias, item_group, top_k, top_p, min_p, temperature).  On the
    GPU every batch is model.served_rank (fused passes, no (B, V) tensor, sharded table included); a CPU model takes the
    materialised route: forward() plus bias and masks, served_ranks_from_scores (exclude_seen then needs the model's
    _session_items).  item_group, being per session, may be a callable (inputs, labels) -> [B] row ids.  With no keywords the
    metrics are those of evaluate(method='rank', cutoffs=cutoffs).  evaluate() is unchanged."""
    model.eval()
    group_of = served.get('item_group')
    ranks = []
    with th.no_grad():
        for batch in data_loader:
            inputs, labels = prepare_batch(batch, device)
            kw = dict(served)
            if callable(group_of):
                kw['item_group'] = group_of(inputs, labels)
            if hasattr(model, 'served_rank') and labels.is_cuda:
                r = model.served_rank(*inputs, labels=labels, **kw)
            else:
                seen = _seen_items('evaluate_served', model, inputs, kw)
                r = served_ranks_from_scores(model(*inputs), labels, seen=seen, **kw)
            ranks.append(r.long().cpu())
    ranks = th.cat(ranks) if ranks else th.zeros(0, dtype=th.long)
    return metrics_from_served_ranks(ranks, [int(k) for k in cutoffs])


def _served_scores(scores, item_bias, item_group, seen, top_k, top_p, min_p, temperature):
    """(s float64 [B, V], eligible bool [B, V], floor float64 [B, 1]) of the materialised routes: the biased score, the rows
    that can be shown (bias > -inf, not seen, not below the truncation floor) and that floor (-inf without one)"""
    ninf = float('-inf')
    s = scores.double()
    B, V = s.shape
    elig = th.ones(B, V, dtype=th.bool, device=s.device)
    if item_bias is not None:
        b = item_bias.to(s.device).double()
        b = b[item_group.to(s.device).long()] if (b.dim() == 2 and item_group is not None) else b.reshape(-1, V)
        s = s + b
        elig &= b != ninf
    if seen is not None:
        sl = seen.to(s.device).long()
        drop = th.zeros(B, V + 1, dtype=th.bool, device=s.device)
        drop.scatter_(1, th.where(sl < 0, th.full_like(sl, V), sl), True)
        elig &= ~drop[:, :V]
    floor = th.full((B, 1), ninf, dtype=th.float64, device=s.device)
    if top_k is not None or top_p is not None or min_p is not None:
        se = th.where(elig, s, th.full_like(s, ninf))
        top = se.max(1, keepdim=True).values
        srt = se.sort(1, descending=True).values
        if top_k is not None:
            kth = srt[:, int(top_k) - 1:int(top_k)] if int(top_k) <= V else floor
            few = elig.sum(1, keepdim=True) < int(top_k)
            floor = th.maximum(floor, th.where(few, th.full_like(kth, ninf), kth))
        if top_p is not None and float(top_p) < 1.0:
            w = th.where(srt > ninf, th.exp((srt - top) / float(temperature)), th.zeros_like(srt))
            cum = w.cumsum(1)
            first = (cum >= float(top_p) * cum[:, -1:]).double().argmax(1, keepdim=True)
            floor = th.maximum(floor, srt.gather(1, first))
        if min_p is not None:
            import math
            floor = th.maximum(floor, top + float(temperature) * math.log(float(min_p)))
        elig = elig & ~(s < floor)
    return s, elig, floor


def item_ranks_from_scores(scores, items, item_bias=None, item_group=None, seen=None, top_k=None, top_p=None, min_p=None,
                           temperature=1.0):
    """model.rank_items from a materialised (B, V) score matrix (a CPU model's forward()): int64 [B, M] with its -1 / -2
    convention, beside served_ranks_from_scores and with its keywords.  items: [B, M] or [M] item ids, -1 = empty slot, every id
    at most once per row.  An item that can be shown is ranked among ALL items that can (its session's other targets
    included), by (value descending, id ascending): the contract of ops.score_ahead_many on exact scores."""
    ninf = float('-inf')
    s, elig, _ = _served_scores(scores, item_bias, item_group, seen, top_k, top_p, min_p, temperature)
    B, V = s.shape
    it = th.as_tensor(items).to(s.device).long()
    it = it.expand(B, it.shape[-1]) if it.dim() == 1 else it
    safe = it.clamp(min=0)
    t = s.gather(1, safe)                                                     # [B, M]
    shown = elig.gather(1, safe) & (t > ninf)
    se = th.where(elig, s, th.full_like(s, float('nan')))                     # (a NaN is ahead of nothing)
    ids = th.arange(V, device=s.device).view(1, 1, V)
    ahead = (se[:, None, :] > t[:, :, None]) | ((se[:, None, :] == t[:, :, None]) & (ids < safe[:, :, None]))
    r = th.where(shown, ahead.sum(2), th.full_like(it, -2))
    return th.where(it >= 0, r, th.full_like(it, -1))


def metrics_from_item_ranks(ranks, cutoffs):
    """Rest-of-session metrics from the ranks of model.rank_items ([n, M]; -1 = empty slot, -2 = a target that could not be
    shown): a CASE is a row with at least one slot != -1, n its number of such slots (a -2 stays in n), hits = #{0 <= r < k}.
    Per cutoff k, means over the cases of  hit@k = [hits > 0];  recall@k = hits / n;  precision@k = hits / k;
    mrr@k = 1 / (1 + min r) if that minimum is < k, else 0;  map@k = (1 / min(n, k)) * sum over the hits j of
    #{i : 0 <= r_i <= r_j} / (r_j + 1);  ndcg@k = sum over the hits of 1 / log2(r_j + 2), divided by the ideal
    sum_{i < min(n, k)} 1 / log2(i + 2).  'shown': the share of the live slots with r >= 0.  No cases: all zeros.  With one
    target per case hit = recall, and hit / mrr / ndcg / shown are metrics_from_served_ranks'."""
    r = th.as_tensor(ranks).detach().to('cpu', th.int64)
    r = r.reshape(-1, r.shape[-1]) if r.dim() >= 2 else r.reshape(-1, 1)
    live = r != -1
    r, live = r[live.any(1)], live[live.any(1)]
    cases = int(r.shape[0])
    out = {}
    ok = r >= 0
    if cases == 0:
        for k in cutoffs:
            out.update({'%s@%d' % (m, int(k)): 0.0 for m in ('hit', 'recall', 'precision', 'mrr', 'map', 'ndcg')})
        out['shown'] = 0.0
        return out
    n = live.sum(1).double()
    rd = r.double()
    # for MAP: the number of the case's shown targets ranked at or before each target
    upto = (ok[:, None, :] & ok[:, :, None] & (r[:, None, :] <= r[:, :, None])).sum(2).double()      # [case, j]
    big = th.where(ok, r, th.full_like(r, 2 ** 62)).min(1).values
    for k in cutoffs:
        k = int(k)
        hit = ok & (r < k)
        hits = hit.sum(1).double()
        lim = th.minimum(n, th.full_like(n, float(k)))
        ideal = th.cumsum(1.0 / th.log2(th.arange(int(lim.max())).double() + 2.0), 0)[(lim - 1).long()]
        zero = th.zeros_like(rd)
        out['hit@%d' % k] = float((hits > 0).double().mean())
        out['recall@%d' % k] = float((hits / n).mean())
        out['precision@%d' % k] = float((hits / k).mean())
        out['mrr@%d' % k] = float(th.where(big < k, 1.0 / (big.double() + 1.0), th.zeros_like(n)).mean())
        out['map@%d' % k] = float((th.where(hit, upto / (rd + 1.0), zero).sum(1) / lim).mean())
        out['ndcg@%d' % k] = float((th.where(hit, 1.0 / th.log2(rd.clamp(min=0) + 2.0), zero).sum(1) / ideal).mean())
    out['shown'] = float(ok.sum()) / float(live.sum())
    return out


def evaluate_rest(model, dataset, collate_fn, device, batch_size, cutoffs=(20,), max_targets=64, **served):
    """Rest-of-session evaluation, the second standard protocol of the session-based literature: every prefix is judged
    against ALL distinct items its session still contains (dataset.rest_items; the next-item label is one of them) -
    metrics_from_item_ranks (hit / recall / precision / mrr / map / ndcg @cutoffs, 'shown') plus 'truncated', the number of
    prefixes with more than max_targets remaining items (they keep the first max_targets).  dataset: an AugmentedDataset,
    walked sequentially in batches of batch_size through collate_fn.  served: the keywords of model.rank_items (exclude_seen,
    item_bias, item_group - also a callable (inputs, labels) -> [B] - top_k, top_p, min_p, temperature).  On the GPU every
    batch is ONE model.rank_items call (one counting pass for all targets, no (B, V) tensor, sharded table included); a CPU
    model takes the materialised route, item_ranks_from_scores.  evaluate() and evaluate_served() are unchanged."""
    model.eval()
    group_of = served.get('item_group')
    ranks, truncated, width = [], 0, 1
    with th.no_grad():
        for lo in range(0, len(dataset), batch_size):
            idx = list(range(lo, min(lo + batch_size, len(dataset))))
            inputs, labels = prepare_batch(collate_fn([dataset[i] for i in idx]), device)
            items, cut = dataset.rest_items(idx, max_targets)
            truncated += cut
            items = th.from_numpy(items).to(device)
            kw = dict(served)
            if callable(group_of):
                kw['item_group'] = group_of(inputs, labels)
            if hasattr(model, 'rank_items') and labels.is_cuda:
                r = model.rank_items(*inputs, items=items, **kw)
            else:
                seen = _seen_items('evaluate_rest', model, inputs, kw)
                r = item_ranks_from_scores(model(*inputs), items, seen=seen, **kw)
            ranks.append(r.long().cpu())
            width = max(width, r.shape[1])
    pad = [th.cat([r, r.new_full((r.shape[0], width - r.shape[1]), -1)], 1) for r in ranks]
    ranks = th.cat(pad) if pad else th.zeros(0, 1, dtype=th.long)
    out = metrics_from_item_ranks(ranks, [int(k) for k in cutoffs])
    out['truncated'] = int(truncated)
    return out


def evaluate(model, data_loader, device, cutoff=20, method='topk', cutoffs=None):
    """(MRR@cutoff, HR@cutoff) as the reference (train.py:36-55).  method='rank': from the label's rank among ALL items
    (model.target_rank on the GPU: one fused pass, no (B, V) tensor, mixtures of soft-maxes included; a CPU model's
    materialised forward() output otherwise) instead of the `cutoff` best items.  cutoffs: return the metrics_from_ranks
    dict for these cutoffs instead of the pair."""
    assert method in ('topk', 'rank'), method
    check_eval_options(method, cutoffs)
    if method == 'rank' or cutoffs is not None:
        return _evaluate_ranks(model, data_loader, device, cutoff, method, cutoffs)
    model.eval()
    mrr, hit, num_samples = 0.0, 0, 0
    with th.no_grad():
        for batch in data_loader:
            inputs, labels = prepare_batch(batch, device)
            if hasattr(model, 'topk') and labels.is_cuda:
                topk = model.topk(*inputs, k=cutoff)[1].long()    # fused: no (B, V) score matrix
                num_samples += topk.size(0)
            else:
                logits = model(*inputs)
                num_samples += logits.size(0)
                topk = logits.topk(k=cutoff)[1]
            hit_ranks = th.where(topk == labels.unsqueeze(-1))[1] + 1
            hit += hit_ranks.numel()
            mrr += hit_ranks.float().reciprocal().sum().item()
    return mrr / num_samples, hit / num_samples


TOPK_MAX = 32        # srec_score_topk keeps at most 32 items per session (include/srec.h)


def check_eval_options(method, cutoffs):
    """cutoffs beyond the fused top-K kernel's limit need the rank method - said before training starts, not after an epoch"""
    if method == 'topk' and cutoffs and max(cutoffs) > TOPK_MAX:
        raise ValueError('evaluation cutoffs above %d need method="rank" (--eval-method rank): the top-K evaluation keeps '
                         'at most %d items per session' % (TOPK_MAX, TOPK_MAX))


def _evaluate_ranks(model, data_loader, device, cutoff, method, cutoffs):
    model.eval()
    kmax = max([int(cutoff)] + [int(k) for k in (cutoffs or ())])
    ranks = []
    with th.no_grad():
        for batch in data_loader:
            inputs, labels = prepare_batch(batch, device)
            if method == 'rank':
                if hasattr(model, 'target_rank') and labels.is_cuda:
                    r = model.target_rank(*inputs, labels=labels)
                else:
                    r = ranks_from_scores(model(*inputs), labels)
            else:       # the `kmax` best items: a label outside them is a miss at every cutoff
                if hasattr(model, 'topk') and labels.is_cuda:
                    topk = model.topk(*inputs, k=kmax)[1].long()
                else:
                    topk = model(*inputs).topk(k=kmax)[1]
                found = topk == labels.unsqueeze(-1)
                r = th.where(found.any(1), found.float().argmax(1), th.full_like(labels, kmax))
            ranks.append(r.long().cpu())
    ranks = th.cat(ranks) if ranks else th.zeros(0, dtype=th.long)
    if cutoffs is not None:
        return metrics_from_ranks(ranks, cutoffs)
    m = metrics_from_ranks(ranks, (cutoff,))
    return m['mrr@%d' % cutoff], m['hit@%d' % cutoff]


class TrainRunner:
    def __init__(self, dataset, model, train_loader, test_loader, device, lr=1e-3, weight_decay=0, patience=3,
                 checkpoint=None, resume=True, hooks=(), graph='auto', shard=None, eval_method='topk', eval_cutoffs=None):
        """Same positional surface as the reference (train.py:57-69).  Additions (the reference has
        neither): `checkpoint` = path written after every epoch (model, optimizer incl. Adam moments and step counts,
        scheduler, epoch / batch counters, best metrics) and, with `resume`, read back at the start of train();
        `hooks` = callables hook(event: dict) invoked after every logged interval and every epoch (the reference's
        wandb calls sit at the same two places).  `graph` ('auto' | False): on the GPU, batches that arrive
        capacity-padded (collate_fn_factory*(..., caps=...)) replay ONE captured hipGraph of the whole step (forward,
        backward, FusedAdam) instead of ~120 eager launches; a batch with another layout or relation pattern runs
        eagerly, with the same result.  `shard` (dist.VocabParallel, multi-GPU): the item table is row-sharded over the
        ranks and every rank feeds its slice of each batch (dataset.RankSliceBatchSampler); the replicated encoder
        gradients are all-reduced after backward, evaluation merges per-shard top-k lists, only rank 0 prints.
        `eval_method` ('topk' | 'rank') and `eval_cutoffs` (e.g. (5, 10, 20)): see evaluate(); the extra cutoffs' HR / MRR / NDCG
        are printed on a line of their own after the reference's epoch line and ride in the 'epoch' hook event as `metrics`."""
        assert eval_method in ('topk', 'rank'), eval_method
        self.eval_method = eval_method
        self.eval_cutoffs = tuple(int(k) for k in eval_cutoffs) if eval_cutoffs else None
        check_eval_options(self.eval_method, self.eval_cutoffs)
        self.shard = shard
        self.rank = shard.rank if shard is not None else 0
        self.replicated = ([p for p in model.parameters() if p is not model._table() and p.requires_grad]
                           if shard is not None else None)
        self.graph = graph
        self._gstep = None
        self.graph_steps = self.eager_steps = 0
        self.checkpoint = checkpoint
        self.resume = resume
        self.hooks = list(hooks)
        self.best = (0, 0, 0)            # max_mrr, max_hit, bad_counter
        self.dataset = dataset
        self.model = model
        params = fix_weight_decay(model) if weight_decay > 0 else model.parameters()
        self.fused = th.device(device).type == 'cuda' and hasattr(model, 'fused_loss')
        if self.fused:
            from .optim import FusedAdam
            self.optimizer = FusedAdam(params, lr=lr, weight_decay=weight_decay, model=model, fuse_projection=True)
        else:
            self.optimizer = optim.Adam(params, lr=lr, weight_decay=weight_decay)
        self.scheduler = optim.lr_scheduler.StepLR(self.optimizer, step_size=3, gamma=0.1)
        self.train_loader = train_loader
        self.test_loader = test_loader
        self.device = device
        self.epoch = 0
        self.batch = 0
        self.patience = patience
        self.loss_trace = []

    def _graph_step(self, inputs, labels):
        """replay of the captured step, or None when this batch has to run eagerly"""
        if not (self.graph and self.fused and getattr(self.model, 'graph_capable', False)):
            return None
        if not all(getattr(x, 'meta', None) is not None and x.meta.get('padded') for x in inputs):
            return None
        from .graph import GraphedTrainStep, capture_agreed
        if self._gstep is None:
            dev_in = [x.to(self.device) for x in inputs]
            dev_lab = labels.to(self.device)
            agree = None
            if self.shard is not None and self.shard.world > 1:
                # the ranks decide TOGETHER (graph.capture_agreed): a rank whose capture failed retries with all the others
                # (the constructor's warm-up steps issue the step's collectives), and after the last attempt either all
                # replay or all launch eagerly
                import torch.distributed as dist
                from .dist import all_reduce_

                def agree(x):
                    ok = th.tensor([x], device=self.device)
                    all_reduce_(ok, dist.ReduceOp.MIN, self.shard.group)
                    return ok.item()
            # (a refused capture: the constructor has put parameters, buffers and optimizer state back - same trajectory)
            self._gstep, self.capture_attempts, err = capture_agreed(
                lambda: GraphedTrainStep(self.model, self.optimizer, dev_in, dev_lab,
                                         after_backward=self._sync_grads if self.shard is not None else None),
                agree, retries=1, log=print)
            if self._gstep is None:
                print('hipGraph capture failed (%s); eager launches' % (('%s: %s' % (type(err).__name__, err)) if err is not None
                                                                        else 'on another rank'))
                self.graph = False
            if self._gstep is None:
                return None
        try:
            return self._gstep(inputs, labels)
        except RuntimeError as e:
            if 'differs from the captured one' not in str(e):
                raise
            return None

    def _sync_grads(self):
        self.shard.sync_replicated_grads(self.replicated, self.optimizer)

    def _print(self, *a):
        if self.rank == 0:
            print(*a)

    def _loss_handle(self, loss):
        """what the training loop keeps of a step's loss until it reads the values back in bulk: a replayed step overwrites
        its static loss tensor - its value waits in the captured step's device ring (graph.LOSS_RING slots, index = the
        step's count), no copy command between two graph launches; an eager step's loss is a tensor of its own"""
        g = self._gstep
        if g is not None and loss is g.loss:
            if g.loss_ring is not None:
                return int(g.last_T)
            return loss.detach().clone()
        return loss.detach()

    def train_step(self, inputs, labels):
        """inputs / labels as the collate function returned them (host, pinned) or already on the device.  A replayed step
        takes a host batch in through a side-stream copy that overlaps the replays still in flight (GraphedTrainStep._post);
        an eager step moves it to the device here."""
        loss = self._graph_step(inputs, labels)
        if loss is not None:
            self.graph_steps += 1
            return loss
        self.eager_steps += 1
        if th.device(self.device).type == 'cuda' and any(getattr(x, 'buf', None) is not None and not x.buf.is_cuda for x in inputs):
            inputs, labels = prepare_batch((inputs, labels), self.device)
        self.optimizer.zero_grad()
        if self.fused:
            loss = self.model.fused_loss(*inputs, labels)
        else:
            scores = self.model(*inputs)
            assert not th.isnan(scores).any()
            loss = nn.functional.nll_loss(scores, labels)
        loss.backward()
        if self.shard is not None:
            self._sync_grads()
        self.optimizer.step()
        return loss

    # ------------------------------------------------------------------ checkpoint / hooks (not in the reference)
    def state_dict(self):
        """plain tensors, numbers, strings, lists and dicts only: loadable with torch.load(weights_only=True).  RNG states
        ride along so that a resumed dropout / shuffled run continues the uninterrupted trajectory."""
        rng = dict(torch=th.get_rng_state())
        if th.cuda.is_available() and th.device(self.device).type == 'cuda':
            rng['cuda'] = th.cuda.get_rng_state(self.device)
        if self.fused:
            # the private generators the run draws from: the dropout nonces of the HIP path (ops._nonce) and the samplers'
            # shuffles (src/scripts/common.py: RandomSampler(generator=...)) - neither is part of torch's global state
            from . import ops
            if ops._NONCE['gen'] is not None:
                rng['nonce'] = ops._NONCE['gen'].get_state()
                rng['nonce_seed'] = int(ops._NONCE['seed'])
        gens = self._loader_generators()
        if gens:
            rng['samplers'] = [g.get_state() for g in gens]
        return dict(model=self.model.state_dict(), optimizer=self.optimizer.state_dict(),
                    scheduler=self.scheduler.state_dict(), epoch=self.epoch, batch=self.batch, best=list(self.best),
                    rng=rng)

    def load_state_dict(self, sd):
        self.model.load_state_dict(sd['model'])
        self.optimizer.load_state_dict(sd['optimizer'])
        self.scheduler.load_state_dict(sd['scheduler'])
        self.epoch, self.batch, self.best = sd['epoch'], sd['batch'], tuple(sd['best'])
        rng = sd.get('rng') or {}
        if 'torch' in rng:
            th.set_rng_state(rng['torch'].cpu())
        if 'cuda' in rng and th.cuda.is_available() and th.device(self.device).type == 'cuda':
            th.cuda.set_rng_state(rng['cuda'].cpu(), self.device)
        if 'nonce' in rng and self.fused:
            from . import ops
            ops.seed_dropout()
            ops._NONCE['gen'].set_state(rng['nonce'].cpu())
            ops._NONCE['seed'] = th.initial_seed()          # (keyed by the seed in effect now: no implicit restart at the next draw)
        for g, st in zip(self._loader_generators(), rng.get('samplers') or []):
            g.set_state(st.cpu())
        self._gstep = None                 # optimizer state tensors were replaced: a captured step would use stale ones
        if self.fused:
            from . import ops
            ops.weights_changed()          # cached bf16 copies / column scales belong to the old weights
            self.model.__dict__.pop('_srec_state', None)
            if hasattr(self.model, 'table_written'):
                self.model.table_written() # notes about rows prepared / copies written by the old optimizer's row pass

    def _loader_generators(self):
        """the torch.Generators that shuffle the training loader (sampler / batch sampler and what they wrap), in a fixed order"""
        out, seen, todo = [], set(), [self.train_loader]
        while todo:
            o = todo.pop(0)
            if o is None or id(o) in seen:
                continue
            seen.add(id(o))
            g = getattr(o, 'generator', None)
            if isinstance(g, th.Generator) and all(g is not h for h in out):
                out.append(g)
            for name in ('sampler', 'batch_sampler', 'base', 'base_sampler'):
                todo.append(getattr(o, name, None))
        return out

    def _ckpt_path(self, path=None):
        """with a row-sharded table every rank owns different rows (and Adam moments): one file per rank"""
        path = path or self.checkpoint
        if self.shard is not None and self.shard.world > 1:
            path = '%s.rank%dof%d' % (path, self.shard.rank, self.shard.world)
        return path

    def save_checkpoint(self, path=None):
        import os
        path = self._ckpt_path(path)
        tmp = path + '.tmp'
        th.save(self.state_dict(), tmp)
        os.replace(tmp, path)              # a crash mid-write never leaves a truncated checkpoint behind

    def load_checkpoint(self, path=None):
        # weights_only=True: a checkpoint is data (tensors / numbers / containers), never pickled code
        self.load_state_dict(th.load(self._ckpt_path(path), map_location=self.device, weights_only=True))

    def _emit(self, **event):
        for h in self.hooks:
            h(event)

    def train(self, epochs, log_interval=100):
        import os
        done = 0
        if self.checkpoint and self.resume and os.path.exists(self._ckpt_path()):
            self.load_checkpoint()
            done = self.epoch                # `epochs` is the total of the interrupted run
            self._print(f'Resumed from {self._ckpt_path()}: epoch {self.epoch}, batch {self.batch}')
        max_mrr, max_hit, bad_counter = self.best
        t = time.time()
        mean_loss = 0
        evaluate(self.model, self.test_loader, self.device)
        for _ in range(epochs - done):
            self.model.train()
            pending = []                  # device-side loss values not read back yet

            def flush():
                # The reference reads loss.item() after every step (train.py:99-104), which drains the GPU queue each time.
                # Same numbers, same NaN check, same running mean - read back in one go where they are needed (the log
                # line, the end of the epoch), so the host prepares batch i+1 while the GPU runs step i.
                nonlocal mean_loss
                if pending:
                    ring = None
                    if any(isinstance(v, int) for v in pending):                # replayed steps: slots of the device loss ring
                        ring = self._gstep.loss_ring.tolist()
                        self._gstep.check()                 # (the host is synchronised here anyway: batch-intake fault flag)
                    eager = [v for v in pending if not isinstance(v, int)]
                    eager = iter(th.stack(eager).tolist()) if eager else iter(())
                    for v in pending:
                        v = ring[v % len(ring)] if isinstance(v, int) else next(eager)
                        assert v == v, 'loss is NaN'
                        self.loss_trace.append(v)
                        mean_loss += v / log_interval
                    pending.clear()
            for batch in self.train_loader:
                inputs, labels = batch                   # (host batches: train_step moves / stages them as its path needs)
                if not self.fused:
                    inputs, labels = prepare_batch(batch, self.device)
                pending.append(self._loss_handle(self.train_step(inputs, labels)))
                if (self.batch > 0 and self.batch % log_interval == 0) or len(pending) >= 256:
                    flush()
                if self.batch > 0 and self.batch % log_interval == 0:
                    self._print(f'Batch {self.batch}: Loss = {mean_loss:.4f}, Time Elapsed = {time.time() - t:.2f}s')
                    self._emit(kind='interval', batch=self.batch, loss=mean_loss, seconds=time.time() - t)
                    t = time.time()
                    mean_loss = 0
                self.batch += 1
            flush()
            if self._gstep is not None:
                self._gstep.check()            # end of the epoch: also a run / tail shorter than a flush interval is checked
            self.scheduler.step()
            metrics = None
            if self.eval_cutoffs:
                metrics = evaluate(self.model, self.test_loader, self.device, method=self.eval_method,
                                   cutoffs=sorted(set(self.eval_cutoffs) | {20}))
                mrr, hit = metrics['mrr@20'], metrics['hit@20']
            else:
                mrr, hit = evaluate(self.model, self.test_loader, self.device, method=self.eval_method)
            self._print(f'Epoch {self.epoch}: MRR = {mrr * 100:.3f}%, Hit = {hit * 100:.3f}%')
            if metrics is not None:
                self._print('         ' + ', '.join(f'{n}@{k} = {metrics["%s@%d" % (key, k)] * 100:.3f}%' for k in self.eval_cutoffs
                                                   for n, key in (('HR', 'hit'), ('MRR', 'mrr'), ('NDCG', 'ndcg'))))
                self._emit(kind='epoch', epoch=self.epoch, mrr=mrr, hit=hit, metrics=metrics)
            else:
                self._emit(kind='epoch', epoch=self.epoch, mrr=mrr, hit=hit)
            stop = False
            if mrr < max_mrr and hit < max_hit:
                bad_counter += 1
                stop = bad_counter == self.patience
            else:
                bad_counter = 0
            if stop:
                break
            max_mrr = max(max_mrr, mrr)
            max_hit = max(max_hit, hit)
            self.epoch += 1
            self.best = (max_mrr, max_hit, bad_counter)
            if self.checkpoint:
                self.save_checkpoint()
        return max_mrr, max_hit
