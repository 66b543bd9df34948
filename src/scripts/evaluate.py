"""(not in the reference) HR / MRR / NDCG of what a trained model SHOWS its users, on the test split of a dataset:

    python scripts/evaluate.py --model SRGNN --checkpoint run.pt --dataset-dir ../datasets/sample --cutoffs 5,10,20 \\
        --exclude-seen --deny blocked.txt

--checkpoint is what `--checkpoint` of the training launchers writes (TrainRunner: its `model` entry is read); the model
flags must be those of the training run.  <dataset-dir>/test.txt is evaluated as the launchers evaluate it (every prefix of
every session predicts its next item: AugmentedDataset).  Without a filter the metrics are those of `--eval-method rank`.
--exclude-seen, --allow FILE / --deny FILE (one item id per line) and --item-bias FILE (`id:value` or `id<TAB>value` per line)
are the serving controls of scripts/recommend.py: the label's rank is then taken among the items recommend.py could print
with the same flags, by log-probability + bias (model.served_rank: the label's value from the gather kernel, one fused
counting pass over the item table - csrc/rank_served.hip - no (B, V) score matrix).  --sample-top-k K / --sample-top-p P /
--sample-min-p Q at --temperature additionally keep only the items a truncated draw (recommend.py --sample) could return.
A label that cannot be shown - the session's own item under --exclude-seen, a denied item, an item outside the truncated
set - is a miss at every cutoff; `shown` is the share of the test cases whose label could be shown at all.
Output: ONE JSON line - {"metrics": {"hit@k", "mrr@k", "ndcg@k" per cutoff, "shown"}, "sessions": n, "flags": {...}}.
--protocol rest is the second standard protocol of the session-based literature: every prefix is judged against ALL distinct
items its session still contains (at most --max-targets of them, in order of first occurrence), under the same serving
controls - hit / recall / precision / mrr / map / ndcg per cutoff and "shown" (train.evaluate_rest: model.rank_items ranks all
targets of a batch in one counting pass, csrc/rank_served_many.hip).  Its line carries "truncated", the number of prefixes
with more than --max-targets remaining items, and the flags "protocol" and "max_targets"."""
import argparse
import json
import sys

from common import DEFAULTS, _cutoffs, build_model, catalog_flags, model_flags, read_catalog, variant_flags


def parser(model):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description=__doc__.split('\n\n')[0])
    p.add_argument('--model', default=model, choices=sorted(DEFAULTS), help='the model class of the checkpoint')
    model_flags(p, model)
    variant_flags(p, model)
    p.add_argument('--checkpoint', required=True, help='a checkpoint of the training launchers (its `model` entry is read)')
    p.add_argument('--cutoffs', type=_cutoffs, default=(5, 10, 20), metavar='K1,K2,...', help='report HR / MRR / NDCG at these cutoffs')
    p.add_argument('--exclude-seen', action='store_true', help="an item of the session itself is never shown")
    catalog_flags(p)
    p.add_argument('--sample-top-k', type=int, default=None, metavar='K',
                   help='only the K most probable eligible items are shown (any K >= 1; ties with the K-th are kept)')
    p.add_argument('--sample-top-p', type=float, default=None, metavar='P',
                   help='only the smallest set of most probable items holding probability P (0 < P < 1) at the --temperature')
    p.add_argument('--sample-min-p', type=float, default=None, metavar='Q',
                   help='only items at least Q times as probable as the best one (0 < Q <= 1)')
    p.add_argument('--temperature', type=float, default=1.0, help='the temperature --sample-top-p / --sample-min-p are taken at')
    p.add_argument('--batch-size', type=int, default=DEFAULTS[model]['batch_size'], help='sessions per launch')
    p.add_argument('--protocol', default='next', choices=['next', 'rest'],
                   help='next: the next item is the one relevant item; rest: every item the session still contains is relevant')
    p.add_argument('--max-targets', type=int, default=64, metavar='M',
                   help='--protocol rest: at most M distinct remaining items per prefix (1 .. 64), the first M are kept')
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'], help='operand precision of the encoder')
    return p


def parse(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--model', default='SRGNN', choices=sorted(DEFAULTS))
    model = pre.parse_known_args(argv)[0].model
    p = parser(model)
    args = p.parse_args(argv)
    if args.batch_size < 1:
        p.error('--batch-size must be positive')
    if not (0.0 < args.temperature < float('inf')):
        p.error('--temperature must be positive and finite')
    if args.sample_top_k is not None and not 1 <= args.sample_top_k < 2 ** 31:
        p.error('--sample-top-k must be an integer >= 1')
    if args.sample_top_p is not None and not 0.0 < args.sample_top_p < 1.0:
        p.error('--sample-top-p must be a probability mass in (0, 1)')
    if args.sample_min_p is not None and not 0.0 < args.sample_min_p <= 1.0:
        p.error('--sample-min-p must be in (0, 1]')
    if not 1 <= args.max_targets <= 64:
        p.error('--max-targets must be in 1 .. 64')
    args.catalog = read_catalog(p, args)
    return args


def served_keywords(args, item_bias):
    """the keywords of model.served_rank / train.evaluate_served the flags stand for"""
    return dict(exclude_seen=args.exclude_seen, item_bias=item_bias, top_k=args.sample_top_k, top_p=args.sample_top_p,
                min_p=args.sample_min_p, temperature=args.temperature)


def report(metrics, sessions, args):
    """the one JSON line (--protocol next: exactly the keys it always had)"""
    flags = {k: getattr(args, k) for k in ('model', 'checkpoint', 'dataset_dir', 'exclude_seen', 'allow', 'deny', 'item_bias',
                                           'sample_top_k', 'sample_top_p', 'sample_min_p', 'temperature', 'batch_size', 'precision')}
    flags['cutoffs'] = list(args.cutoffs)
    if getattr(args, 'protocol', 'next') != 'rest':
        return json.dumps({'metrics': metrics, 'sessions': sessions, 'flags': flags})
    metrics = dict(metrics)
    flags.update(protocol='rest', max_targets=args.max_targets)
    return json.dumps({'metrics': metrics, 'sessions': sessions, 'truncated': metrics.pop('truncated', 0), 'flags': flags})


def main(argv=None):
    args = parse(argv)
    import torch as th
    from importlib import import_module
    from pathlib import Path
    from torch.utils.data import DataLoader
    if not th.cuda.is_available():
        sys.exit('evaluate.py needs a GPU: the models run on HIP kernels only')
    device = th.device('cuda', th.cuda.current_device())
    ops = import_module('sessionrec-pytorch_amd.ops')
    train = import_module('sessionrec-pytorch_amd.train')
    ds = import_module('sessionrec-pytorch_amd.dataset')
    ops.set_precision(args.precision)
    with open(Path(args.dataset_dir) / 'num_items.txt') as f:
        num_items = int(f.readline())
    model, collate_fn, _ = build_model(args.model, args, num_items, device)
    state = th.load(args.checkpoint, map_location='cpu', weights_only=True)
    model.load_state_dict(state['model'])
    model = model.to(device).eval()
    ops.weights_changed()
    model.table_written()
    item_bias = None if args.catalog is None else ops.catalog_bias(num_items, device=device, **args.catalog)
    test_set = ds.AugmentedDataset(ds.read_sessions(str(Path(args.dataset_dir) / 'test.txt')))
    if args.protocol == 'rest':
        metrics = train.evaluate_rest(model, test_set, collate_fn, device, args.batch_size, args.cutoffs, args.max_targets,
                                      **served_keywords(args, item_bias))
    else:
        loader = DataLoader(test_set, batch_size=args.batch_size, shuffle=False, collate_fn=collate_fn)
        metrics = train.evaluate_served(model, loader, device, args.cutoffs, **served_keywords(args, item_bias))
    print(report(metrics, len(test_set), args))


if __name__ == '__main__':
    main()
