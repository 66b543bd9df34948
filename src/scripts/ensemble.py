"""(not in the reference) serve and evaluate an ENSEMBLE of trained models - the probability-averaged blend of their next-item
distributions (sessionrec-pytorch_amd/ensemble.py: Ensemble; one fused pass over the members' item tables, csrc/ensemble.hip):

    python scripts/ensemble.py --members members.txt --sessions sessions.txt --top 50 --exclude-seen
    python scripts/ensemble.py --members members.txt --evaluate --dataset-dir ../datasets/sample --cutoffs 5,10,20
    python scripts/ensemble.py --members members.txt --fit-weights --evaluate --dataset-dir ../datasets/sample

--members FILE holds one member per line, written as the model flags of scripts/recommend.py plus --weight W (default 1; the
weights are normalised to sum to one), e.g.

    --model SRGNN --checkpoint a.pt --weight 0.4
    --model MSGIFSR --order 3 --fusion --checkpoint b.pt

(blank lines and lines that start with # are skipped; a member's --dataset-dir defaults to this script's).  All members share
the catalogue of --dataset-dir; together they may mix at most 8 soft-maxes (an MSGIFSR order-k --fusion member counts k).
Serving: --sessions FILE (one session per line, as scripts/recommend.py) prints one line of `id:logprob` pairs per session, best
first - the values are log sum_m w_m p_m(item) (+ bias), not renormalised.  --exclude-seen, --allow / --deny / --item-bias,
--batch-size and --output as in scripts/recommend.py.  Every member's sessions are cut to ITS OWN per-session capacity.
--evaluate prints ONE JSON line instead: HR / MRR / NDCG at --cutoffs and `shown` on <dataset-dir>/test.txt under the same
serving controls (Ensemble.served_rank, train.metrics_from_served_ranks), with the weights used.
--fit-weights first fits the weights on the labels of <dataset-dir>/test.txt (Ensemble.fit_weights: EM on the members'
log-probabilities of the labels), prints them to the standard error stream and uses them instead of --weight."""
import argparse
import json
import shlex
import sys

from common import DEFAULTS, _cutoffs, build_model, catalog_flags, model_flags, read_catalog, variant_flags
from recommend import MAX_TOP, format_line, read_session_file, session_capacity


class _LineParser(argparse.ArgumentParser):
    """argparse for one line of --members: a mistake raises ValueError instead of leaving the process"""

    def error(self, message):
        raise ValueError(message)


def member_parser(model):
    """the flags of one --members line: recommend.py's model and variant flags, --checkpoint and --weight"""
    p = _LineParser(add_help=False, allow_abbrev=False)
    p.add_argument('--model', default=model, choices=sorted(DEFAULTS))
    model_flags(p, model)
    variant_flags(p, model)
    p.add_argument('--checkpoint', required=True)
    p.add_argument('--weight', type=float, default=None)
    p.set_defaults(dataset_dir=None)
    return p


def parse_member(line):
    """one --members line -> argparse.Namespace (model, its flags, checkpoint, weight or None); ValueError for a bad line"""
    try:
        argv = shlex.split(line, comments=True)
    except ValueError as e:
        raise ValueError('cannot split the line: %s' % e) from None
    pre = _LineParser(add_help=False, allow_abbrev=False)
    pre.add_argument('--model', default='SRGNN', choices=sorted(DEFAULTS))
    model = pre.parse_known_args(argv)[0].model
    m = member_parser(model).parse_args(argv)
    if m.weight is not None and not (0.0 < m.weight < float('inf')):
        raise ValueError('--weight must be positive and finite')
    return m


def read_members(path):
    """[Namespace, ...] of a --members file; ValueError names the line"""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip() or line.lstrip().startswith('#'):
                continue
            try:
                out.append(parse_member(line))
            except ValueError as e:
                raise ValueError('%s, line %d: %s' % (path, n, e)) from None
    if not out:
        raise ValueError('%s names no member' % path)
    return out


def parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description=__doc__.split('\n\n')[0])
    p.add_argument('--members', required=True, metavar='FILE', help='one member per line: recommend.py\'s model flags plus --weight W')
    p.add_argument('--dataset-dir', default='../datasets/sample', help='the dataset directory (the catalogue; the test split)')
    p.add_argument('--sessions', default=None, help='serving: one session per line, item ids separated by commas')
    p.add_argument('--top', type=int, default=20, help='items per session (at most %d)' % MAX_TOP)
    p.add_argument('--exclude-seen', action='store_true', help='never recommend / show an item of the session itself')
    catalog_flags(p)
    p.add_argument('--evaluate', action='store_true', help='print HR / MRR / NDCG of the blend on <dataset-dir>/test.txt as one JSON line')
    p.add_argument('--cutoffs', type=_cutoffs, default=(5, 10, 20), metavar='K1,K2,...', help='--evaluate: report at these cutoffs')
    p.add_argument('--fit-weights', action='store_true',
                   help='fit the weights on the labels of <dataset-dir>/test.txt first; replaces --weight')
    p.add_argument('--batch-size', type=int, default=128, help='sessions per launch')
    p.add_argument('--output', default=None, help='serving: write here instead of the standard output')
    return p


def parse(argv=None):
    p = parser()
    args = p.parse_args(argv)
    if not 1 <= args.top <= MAX_TOP:
        p.error('--top must be between 1 and %d (the selection kernel keeps at most %d items per session)' % (MAX_TOP, MAX_TOP))
    if args.batch_size < 1:
        p.error('--batch-size must be positive')
    if args.sessions is None and not args.evaluate and not args.fit_weights:
        p.error('give --sessions (serving), --evaluate or --fit-weights')
    try:
        args.member_list = read_members(args.members)
    except (OSError, ValueError) as e:
        p.error('--members: %s' % e)
    for m in args.member_list:
        if m.dataset_dir is None:
            m.dataset_dir = args.dataset_dir
    args.catalog = read_catalog(p, args)
    return args


class Member:
    """a loaded member: the model on the device, its collate function and the session length its kernels take"""

    def __init__(self, flags, num_items, device, ops, exclude_seen):
        import torch as th
        self.flags = flags
        model, self.collate_fn, _ = build_model(flags.model, flags, num_items, device)
        state = th.load(flags.checkpoint, map_location='cpu', weights_only=True)
        model.load_state_dict(state['model'])
        self.model = model.to(device).eval()
        self.model.table_written()
        self.cap = session_capacity(ops.limits(), getattr(flags, 'order', 1), exclude_seen or getattr(flags, 'extra', False))

    def cut(self, sessions, who):
        """the sessions as this member takes them (their last `cap` clicks), with recommend.py's warning"""
        n = sum(len(s) > self.cap for s in sessions)
        if n:
            print('warning: %s: %d sessions are longer than %d clicks (the per-session capacity of the kernels) and were cut to '
                  'their last %d clicks' % (who, n, self.cap, self.cap), file=sys.stderr)
            return [s[-self.cap:] for s in sessions]
        return sessions

    def inputs(self, samples, device):
        inputs, _ = self.collate_fn(samples)
        return tuple(x.to(device) for x in inputs)


def main(argv=None):
    args = parse(argv)
    import torch as th
    from importlib import import_module
    from pathlib import Path
    if not th.cuda.is_available():
        sys.exit('ensemble.py needs a GPU: the models run on HIP kernels only')
    device = th.device('cuda', th.cuda.current_device())
    ops = import_module('sessionrec-pytorch_amd.ops')
    train = import_module('sessionrec-pytorch_amd.train')
    ds = import_module('sessionrec-pytorch_amd.dataset')
    Ensemble = import_module('sessionrec-pytorch_amd.ensemble').Ensemble
    ops.set_precision('fp32')
    with open(Path(args.dataset_dir) / 'num_items.txt') as f:
        num_items = int(f.readline())
    members = [Member(m, num_items, device, ops, args.exclude_seen) for m in args.member_list]
    ops.weights_changed()
    weights = [1.0 if m.flags.weight is None else m.flags.weight for m in members]
    item_bias = None if args.catalog is None else ops.catalog_bias(num_items, device=device, **args.catalog)
    served = dict(exclude_seen=args.exclude_seen, item_bias=item_bias)

    def batches(samples):
        """(per-member inputs, labels) per batch of (session, label) samples, every member's sessions cut to its capacity"""
        cut = [m.cut([s for s, _ in samples], 'member %d' % i) for i, m in enumerate(members)]
        for b in range(0, len(samples), args.batch_size):
            labels = th.tensor([l for _, l in samples[b:b + args.batch_size]], dtype=th.int64, device=device)
            yield [m.inputs([(s, 0) for s in c[b:b + args.batch_size]], device) for m, c in zip(members, cut)], labels

    test = None
    if args.evaluate or args.fit_weights:
        test_set = ds.AugmentedDataset(ds.read_sessions(str(Path(args.dataset_dir) / 'test.txt')))
        test = [test_set[i] for i in range(len(test_set))]
        test = [(list(s), int(l)) for s, l in test]
    if args.fit_weights:
        logp = []
        for inputs, labels in batches(test):
            logp.append(th.stack([m.model.score_items(*inp, items=labels[:, None])[:, 0] for m, inp in zip(members, inputs)], 1))
        weights = Ensemble.fit_weights(th.cat(logp, 0)).tolist()
        print('fitted weights: %s' % ' '.join('%.6f' % w for w in weights), file=sys.stderr)
    ens = Ensemble([m.model for m in members], weights)

    if args.evaluate:
        ranks = [ens.served_rank(inputs, labels, **served).long().cpu() for inputs, labels in batches(test)]
        ranks = th.cat(ranks) if ranks else th.zeros(0, dtype=th.long)
        metrics = train.metrics_from_served_ranks(ranks, [int(k) for k in args.cutoffs])
        flags = {k: getattr(args, k) for k in ('members', 'dataset_dir', 'exclude_seen', 'allow', 'deny', 'item_bias', 'batch_size')}
        flags['cutoffs'] = list(args.cutoffs)
        print(json.dumps({'metrics': metrics, 'sessions': len(test), 'weights': list(ens.weights), 'flags': flags}))
    if args.sessions is not None:
        sessions = read_session_file(args.sessions)
        out = open(args.output, 'w') if args.output else sys.stdout
        try:
            for inputs, _ in batches([(s, 0) for s in sessions]):
                val, idx = ens.recommend(inputs, k=args.top, **served)
                for ids, vals in zip(idx.cpu().tolist(), val.cpu().tolist()):
                    out.write(format_line(ids, vals) + '\n')
        finally:
            if out is not sys.stdout:
                out.close()


if __name__ == '__main__':
    main()
