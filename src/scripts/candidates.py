"""(not in the reference) long candidate lists of a trained model for a file of sessions - the first stage of a two-stage set-up:

    python scripts/candidates.py --model SRGNN --checkpoint cheap.pt --sessions sessions.txt --top 1000 --ids-only > cands.txt
    python scripts/rerank.py --model MSGIFSR --checkpoint strong.pt --sessions sessions.txt --candidates cands.txt --top 50

--checkpoint, --sessions, the model flags, --exclude-seen, --allow / --deny / --item-bias, --renormalize, --batch-size,
--precision and --output are those of recommend.py.  --top N: 1 <= N <= 4096 items per session (recommend.py stops at 128:
model.recommend_many finds every session's N-th best score by radix search, collects the items at or above it and orders
them, csrc/select_many.hip - no (B, V) score matrix).  Output: one line per input session, in input order - recommend.py's
`id:logprob` pairs separated by tabs, best first; --ids-only: the ids alone, separated by commas, the file rerank.py
--candidates reads (a session without a single eligible item gives the line `-1`, rerank.py's padding id)."""
import argparse
import sys

from common import DEFAULTS, build_model, catalog_flags, model_flags, read_catalog, variant_flags
from recommend import format_line, parse_line, read_session_file, session_capacity  # noqa: F401  (one format, one reader)

MAX_TOP = 4096          # SREC_SELECT_MANY_MAXK (include/srec.h)


def format_ids(ids):
    """the ids of one session separated by commas, unfilled slots (id -1) left out - a line read_session_file reads back;
    no id at all: `-1`, the padding id of rerank.py (an empty line would not count as a session there)"""
    return ','.join(str(i) for i in ids if i >= 0) or '-1'


def parser(model):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description=__doc__.split('\n\n')[0])
    p.add_argument('--model', default=model, choices=sorted(DEFAULTS), help='the model class of the checkpoint')
    model_flags(p, model)
    variant_flags(p, model)
    p.add_argument('--checkpoint', required=True, help='a checkpoint of the training launchers (its `model` entry is read)')
    p.add_argument('--sessions', required=True, help='one session per line, item ids separated by commas')
    p.add_argument('--top', type=int, default=1000, help='items per session (at most %d)' % MAX_TOP)
    p.add_argument('--ids-only', action='store_true',
                   help='write the ids alone, separated by commas: the file rerank.py --candidates reads')
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
    if not 1 <= args.top <= MAX_TOP:
        p.error('--top must be between 1 and %d (the order kernel returns at most %d items per session)' % (MAX_TOP, MAX_TOP))
    if args.batch_size < 1:
        p.error('--batch-size must be positive')
    args.catalog = read_catalog(p, args)
    return args


def main(argv=None):
    args = parse(argv)
    import torch as th
    from importlib import import_module
    from pathlib import Path
    if not th.cuda.is_available():
        sys.exit('candidates.py needs a GPU: the models run on HIP kernels only')
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

    sessions = read_session_file(args.sessions)
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
            val, idx = model.recommend_many(*[x.to(device) for x in inputs], k=args.top, exclude_seen=args.exclude_seen,
                                            item_bias=item_bias, renormalize=args.renormalize)
            for ids, vals in zip(idx.cpu().tolist(), val.cpu().tolist()):
                out.write((format_ids(ids) if args.ids_only else format_line(ids, vals)) + '\n')
    finally:
        if out is not sys.stdout:
            out.close()


if __name__ == '__main__':
    main()
