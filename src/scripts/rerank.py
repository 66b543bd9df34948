"""(not in the reference) re-rank given candidate items for a file of sessions with a trained model:

    python scripts/rerank.py --model SRGNN --checkpoint run.pt --sessions sessions.txt --candidates candidates.txt --top 50

--checkpoint, --sessions and the model flags are those of recommend.py.  --candidates holds the candidate item ids of session
i on line i, separated by commas (lines may differ in length); a file of ONE line serves every session.  Output: one line
per input session, in input order - `id:logprob` pairs separated by tabs, best first, in recommend.py's format.  The values
are the model's full-catalog log-probabilities of the candidates (model.rerank: one gather pass over the candidates' rows,
no (B, V) score matrix, any number of candidates); candidates that cannot be returned (--exclude-seen, --allow / --deny) are left out.  --allow / --deny / --item-bias as in
recommend.py: the values are then log-probability + bias.  --renormalize as in recommend.py: over the eligible CATALOGUE, not
over the candidates."""
import argparse
import sys

from common import DEFAULTS, build_model, catalog_flags, model_flags, read_catalog, variant_flags
from recommend import format_line, parse_line, read_session_file, session_capacity  # noqa: F401  (one format, one reader)


def parser(model):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description=__doc__.split('\n\n')[0])
    p.add_argument('--model', default=model, choices=sorted(DEFAULTS), help='the model class of the checkpoint')
    model_flags(p, model)
    variant_flags(p, model)
    p.add_argument('--checkpoint', required=True, help='a checkpoint of the training launchers (its `model` entry is read)')
    p.add_argument('--sessions', required=True, help='one session per line, item ids separated by commas')
    p.add_argument('--candidates', required=True, help='candidate item ids of session i on line i (one line: for every session)')
    p.add_argument('--top', type=int, default=None, help='items per session (default: every candidate)')
    p.add_argument('--exclude-seen', action='store_true', help="never return an item of the session itself")
    catalog_flags(p)
    p.add_argument('--renormalize', action='store_true',
                   help='print log-probabilities renormalised over the eligible catalogue (--exclude-seen, --allow / --deny, '
                        '--item-bias): per session they sum to one over the items that can be shown')
    p.add_argument('--batch-size', type=int, default=DEFAULTS[model]['batch_size'], help='sessions per launch')
    p.add_argument('--output', default=None, help='write here instead of the standard output')
    p.add_argument('--precision', default='fp32', choices=['fp32', 'bf16'], help='operand precision of the encoder')
    return p


def parse(argv=None):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--model', default='SRGNN', choices=sorted(DEFAULTS))
    model = pre.parse_known_args(argv)[0].model
    p = parser(model)
    args = p.parse_args(argv)
    if args.top is not None and args.top < 1:
        p.error('--top must be positive')
    if args.batch_size < 1:
        p.error('--batch-size must be positive')
    args.catalog = read_catalog(p, args)
    return args


def match_candidates(parser_, sessions, candidates):
    """one candidate list per session: a single line serves all; any other difference in line counts is a usage error"""
    if len(candidates) == 1:
        return candidates * len(sessions)
    if len(candidates) != len(sessions):
        parser_.error('--candidates has %d lines for %d sessions (one line per session, or a single line for all)'
                      % (len(candidates), len(sessions)))
    return candidates


def pad_candidates(lists):
    """[[id, ...], ...] of one batch -> rows of equal length, short ones filled with -1 (padding slots score -inf)"""
    width = max((len(c) for c in lists), default=0)
    return [list(c) + [-1] * (width - len(c)) for c in lists]


def main(argv=None):
    args = parse(argv)
    sessions = read_session_file(args.sessions)
    candidates = match_candidates(parser(args.model), sessions, read_session_file(args.candidates))
    import torch as th
    from importlib import import_module
    from pathlib import Path
    if not th.cuda.is_available():
        sys.exit('rerank.py needs a GPU: the models run on HIP kernels only')
    device = th.device('cuda', th.cuda.current_device())
    ops = import_module('sessionrec-pytorch_amd.ops')
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

    cap = session_capacity(ops.limits(), getattr(args, 'order', 1), args.exclude_seen or getattr(args, 'extra', False))
    cut = sum(len(s) > cap for s in sessions)
    if cut:
        print('warning: %d sessions are longer than %d clicks (the per-session capacity of the kernels) and were cut to '
              'their last %d clicks' % (cut, cap, cap), file=sys.stderr)
        sessions = [s[-cap:] for s in sessions]
    out = open(args.output, 'w') if args.output else sys.stdout
    try:
        for b in range(0, len(sessions), args.batch_size):
            inputs, _ = collate_fn([(s, 0) for s in sessions[b:b + args.batch_size]])
            items = th.tensor(pad_candidates(candidates[b:b + args.batch_size]), dtype=th.int64)
            val, idx = model.rerank(*[x.to(device) for x in inputs], items=items.to(device), k=args.top,
                                    exclude_seen=args.exclude_seen, item_bias=item_bias, renormalize=args.renormalize)
            for ids, vals in zip(idx.cpu().tolist(), val.cpu().tolist()):
                out.write(format_line(ids, vals) + '\n')
    finally:
        if out is not sys.stdout:
            out.close()


if __name__ == '__main__':
    main()
