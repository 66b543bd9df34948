"""(not in the reference) top-N recommendations of a trained model for a file of sessions:

    python scripts/recommend.py --model SRGNN --checkpoint run.pt --sessions sessions.txt --top 50 --exclude-seen

--checkpoint is what `--checkpoint` of the training launchers writes (TrainRunner: its `model` entry is read); the model
flags must be those of the training run.  --sessions holds one session per line in the format of datasets/*/test.txt
(item ids separated by commas); the WHOLE line is the prefix whose next item is wanted.  Output: one line per input
session, in input order - `id:logprob` pairs separated by tabs, best first (model.recommend: one fused selection pass over
the item table, no (B, V) score matrix).  --allow FILE / --deny FILE (one item id per line) restrict the catalogue for this
run and --item-bias FILE (`id:value` or `id<TAB>value` per line) is added to the log-probabilities before ranking; the printed
values are then log-probability + bias (ops.catalog_bias combines the three, the selection kernel applies them).
--renormalize prints them renormalised over the items that remain eligible (model.recommend(renormalize=True): one more
fused pass, csrc/score_norm.hip).
--sample DRAWS the --top items of every session from the model's distribution instead of taking the most probable ones
(model.sample: without replacement, in draw order; --temperature sharpens or flattens it, --seed fixes the draw).  The
session key of the noise is the 0-based number of the session in the file (blank lines are not counted), so the output does
not depend on --batch-size.  The printed values are still the items' log-probabilities, not the sampled keys.
--sample-top-k K / --sample-top-p P / --sample-min-p Q truncate the distribution before the draw (model.sample(top_k=, top_p=,
min_p=): among the K most probable items, inside the nucleus of mass P at the --temperature, among the items at least Q times
as probable as the best one; several flags: the smallest set - csrc/score_cutoff.hip finds the cutoff without the score
matrix).  A session that keeps fewer than --top items prints fewer pairs.  Only with --sample.
--diversity THETA re-ranks the --pool M most probable items of every session (default min(128, max(4 top, top))) into a slate
of --top items that trades probability for coverage (model.recommend_diverse: greedy MMR on the cosine of the item rows, one
more kernel, csrc/diversify.hip); the output has the same format, in PICK order, with the items' own values.  Not together
with --sample.
--categories FILE (`id:category` per line; an unlisted item has no category) with --max-per-category N prints the first --top
items of the served order that hold at most N items of one category (model.recommend_capped: one more kernel over the ordered
pool, csrc/cap_select.hip); --category-caps FILE (`category:cap` per line) sets the cap of the categories it names instead of
N.  --pool M (--top <= M <= 4096) fixes the pool the list is taken from; by default the 128 most probable items, and the 4096
most probable ones for a batch in which some session's list runs short.  Same output format, served order.  Not together with
--sample or --diversity.
--calibrate W (in [0, 1]) with --categories FILE re-ranks the --pool M most probable items (--top <= M <= 128, default
min(128, max(4 top, top))) into a slate whose category mix follows that of the session's own items (model.recommend_calibrated:
greedy on (1 - W) * value - W * KL(target, list), one more kernel, csrc/calibrate.hip); --calibrate-smooth A (default 0.01)
is the smoothing of the KL term.  Same output format, in PICK order, with the items' own values.  Not together with --sample,
--diversity, --max-per-category or --category-caps.
--hide FILE names the items every session must NOT be shown: line i holds those of session i (ONE line: of every session),
separated by commas or tabs, each `id` or `id:anything` - an output file of this script is one, so page 2 is

    python scripts/recommend.py ... --top 10 --output page1.txt ;  python scripts/recommend.py ... --top 10 --hide page1.txt

--session-bias FILE (the same layout, `id:value` entries) adds the value to the log-probability of that item for that session
before ranking; an id in both files is hidden (model.recommend_personal: the --top + M most probable items merged with the M
listed ones re-scored, one more kernel, csrc/personal.hip - no dense per-session bias).  --pool M (--top <= M <= 4096) fixes
the pool the list is taken from.  Same output format, served order.  Not together with --sample, --diversity, the cap flags,
--calibrate or --renormalize."""
import argparse
import sys

from common import (DEFAULTS, build_model, calibrate_flags, cap_flags, catalog_flags, model_flags, personal_flags,
                    read_calibration, read_caps, read_catalog, read_personal, variant_flags)

MAX_TOP = 128           # SREC_SELECT_MAXK (include/srec.h)
MAX_CAP_POOL = 4096     # SREC_CAP_MAXP


def read_session_file(path):
    """[[item id, ...], ...]: one session per non-empty line, ids separated by commas (datasets/*/test.txt)"""
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line:
                out.append([int(x) for x in line.split(',')])
    return out


def format_sessions(sessions):
    """the text read_session_file reads back"""
    return ''.join(','.join(str(i) for i in s) + '\n' for s in sessions)


def format_line(ids, vals):
    """`id:logprob` pairs separated by tabs; unfilled slots (id -1: fewer eligible items than --top) are left out"""
    return '\t'.join('%d:%.7f' % (i, v) for i, v in zip(ids, vals) if i >= 0)


def parse_line(line):
    """-> ([ids], [log-probabilities]) of one output line"""
    pairs = [p.split(':') for p in line.rstrip('\n').split('\t') if p]
    return [int(i) for i, _ in pairs], [float(v) for _, v in pairs]


def session_capacity(limits, order=1, listed=False):
    """the longest session (in clicks) that fits the per-session kernels whatever it holds: at most limits['nodes'] read-out
    nodes (all n-gram orders together: <= order * clicks), node degrees <= limits['deg'] (<= clicks), and - where the
    session's own items travel as a list (--exclude-seen, --extra) - at most 64 distinct items"""
    cap = min(limits['nodes'] // max(order, 1), limits['deg'])
    return min(cap, 64) if listed else cap


def parser(model):
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description=__doc__.split('\n\n')[0])
    p.add_argument('--model', default=model, choices=sorted(DEFAULTS), help='the model class of the checkpoint')
    model_flags(p, model)
    variant_flags(p, model)
    p.add_argument('--checkpoint', required=True, help='a checkpoint of the training launchers (its `model` entry is read)')
    p.add_argument('--sessions', required=True, help='one session per line, item ids separated by commas')
    p.add_argument('--top', type=int, default=20, help='items per session (at most %d)' % MAX_TOP)
    p.add_argument('--exclude-seen', action='store_true', help="never recommend an item of the session itself")
    catalog_flags(p)
    p.add_argument('--renormalize', action='store_true',
                   help='print log-probabilities renormalised over the eligible catalogue (--exclude-seen, --allow / --deny, '
                        '--item-bias): per session they sum to one over the items that can be shown')
    p.add_argument('--sample', action='store_true',
                   help='draw the --top items from the distribution (without replacement, in draw order) instead of taking '
                        'the most probable ones')
    p.add_argument('--temperature', type=float, default=1.0, help='--sample: draw from softmax(log-probability / temperature)')
    p.add_argument('--seed', type=int, default=0, help='--sample: seed of the draw, in [0, 2^64)')
    p.add_argument('--sample-top-k', type=int, default=None, metavar='K',
                   help='--sample: draw among the K most probable eligible items (any K >= 1; ties with the K-th are kept)')
    p.add_argument('--sample-top-p', type=float, default=None, metavar='P',
                   help='--sample: draw inside the smallest set of most probable items holding probability P (0 < P < 1) at '
                        'the --temperature')
    p.add_argument('--sample-min-p', type=float, default=None, metavar='Q',
                   help='--sample: never draw an item less than Q times as probable as the best one (0 < Q <= 1)')
    p.add_argument('--diversity', type=float, default=None, metavar='THETA',
                   help='re-rank the --pool most probable items into a diversified slate: each pick maximises value - THETA * '
                        '(largest cosine to the items picked so far); finite, >= 0; printed in pick order')
    p.add_argument('--pool', type=int, default=None, metavar='M',
                   help='--diversity: items per session the slate is picked from, --top <= M <= %d (default: min(%d, 4 * top)); '
                        '--categories: the pool the capped list is taken from, --top <= M <= %d (default: %d, then %d); '
                        '--calibrate: as for --diversity; --hide / --session-bias: the pool the listed items are merged '
                        'into, --top <= M <= %d (default: --top + the longest list)'
                        % (MAX_TOP, MAX_TOP, MAX_CAP_POOL, MAX_TOP, MAX_CAP_POOL, MAX_CAP_POOL))
    cap_flags(p)
    calibrate_flags(p)
    personal_flags(p)
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
        p.error('--top must be between 1 and %d (the selection kernel keeps at most %d items per session)' % (MAX_TOP, MAX_TOP))
    if args.batch_size < 1:
        p.error('--batch-size must be positive')
    if not (0.0 < args.temperature < float('inf')):
        p.error('--temperature must be positive and finite')
    if not 0 <= args.seed < 2 ** 64:
        p.error('--seed must be in [0, 2^64)')
    for flag, val in (('--sample-top-k', args.sample_top_k), ('--sample-top-p', args.sample_top_p), ('--sample-min-p', args.sample_min_p)):
        if val is not None and not args.sample:
            p.error('%s truncates the distribution --sample draws from: it goes with --sample' % flag)
    if args.sample_top_k is not None and not 1 <= args.sample_top_k < 2 ** 31:
        p.error('--sample-top-k must be an integer >= 1')
    if args.sample_top_p is not None and not 0.0 < args.sample_top_p < 1.0:
        p.error('--sample-top-p must be a probability mass in (0, 1)')
    if args.sample_min_p is not None and not 0.0 < args.sample_min_p <= 1.0:
        p.error('--sample-min-p must be in (0, 1]')
    personal = args.hide is not None or args.session_bias is not None
    if personal:
        for flag, given in (('--sample', args.sample), ('--diversity', args.diversity is not None),
                            ('--categories / --max-per-category / --category-caps',
                             args.categories is not None or args.max_per_category is not None or args.category_caps is not None),
                            ('--calibrate', args.calibrate is not None), ('--renormalize', args.renormalize)):
            if given:
                p.error('--hide / --session-bias merge per-session lists into the most probable items: not together with %s' % flag)
        if args.pool is not None and not args.top <= args.pool <= MAX_CAP_POOL:
            p.error('--pool must be between --top and %d' % MAX_CAP_POOL)
    if args.diversity is not None:
        if args.sample:
            p.error('--diversity re-ranks the most probable items and --sample draws them: give one of the two')
        if not (0.0 <= args.diversity < float('inf')):
            p.error('--diversity must be finite and >= 0')
        if args.pool is not None and not args.top <= args.pool <= MAX_TOP:
            p.error('--pool must be between --top and %d' % MAX_TOP)
    elif args.pool is not None and args.categories is None and not personal:
        p.error('--pool goes with --diversity or --categories (or --hide / --session-bias)')
    if args.calibrate is not None:
        if args.sample:
            p.error('--calibrate re-ranks the most probable items and --sample draws them: give one of the two')
        if args.diversity is not None:
            p.error('--calibrate and --diversity are two re-ranks of the same pool: give one of the two')
        if args.pool is not None and not args.top <= args.pool <= MAX_TOP:
            p.error('--pool must be between --top and %d' % MAX_TOP)
    elif args.categories is not None:
        if args.sample or args.diversity is not None:
            p.error('--categories caps the most probable items in served order: not together with --sample or --diversity')
        if args.pool is not None and not args.top <= args.pool <= MAX_CAP_POOL:
            p.error('--pool must be between --top and %d' % MAX_CAP_POOL)
    args.calibration = read_calibration(p, args)
    args.caps = None if args.calibration is not None else read_caps(p, args)
    args.catalog = read_catalog(p, args)
    args.personal = None
    if personal:
        try:
            n_sessions = len(read_session_file(args.sessions))
        except (OSError, ValueError) as e:
            p.error('--sessions: %s' % e)
        args.personal = read_personal(p, args, n_sessions)
    return args


def main(argv=None):
    args = parse(argv)
    import torch as th
    from importlib import import_module
    from pathlib import Path
    if not th.cuda.is_available():
        sys.exit('recommend.py needs a GPU: the models run on HIP kernels only')
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
    rule = None if args.caps is None else ops.cap_rule(num_items, device=device, **args.caps)
    calibration = args.calibration
    if calibration is not None:           # (the category vector goes to the device once, as int32: no read per batch)
        calibration = dict(calibration, item_category=th.tensor(calibration['item_category'], dtype=th.int32, device=device))

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
            n = len(sessions[b:b + args.batch_size])
            if args.personal is not None:
                mine = {key: rows if rows is None or len(rows) == 1 else rows[b:b + n] for key, rows in args.personal.items()}
                val, idx = model.recommend_personal(*[x.to(device) for x in inputs], k=args.top, pool=args.pool,
                                                    exclude_seen=args.exclude_seen, item_bias=item_bias, **mine)
            elif args.sample:
                val, idx = model.sample(*[x.to(device) for x in inputs], k=args.top, temperature=args.temperature,
                                        seed=args.seed, session_keys=th.arange(b, b + n, dtype=th.int32),
                                        exclude_seen=args.exclude_seen, item_bias=item_bias, renormalize=args.renormalize,
                                        top_k=args.sample_top_k, top_p=args.sample_top_p, min_p=args.sample_min_p)
            elif args.diversity is not None:
                val, idx = model.recommend_diverse(*[x.to(device) for x in inputs], k=args.top, diversity=args.diversity,
                                                   pool=args.pool, exclude_seen=args.exclude_seen, item_bias=item_bias,
                                                   renormalize=args.renormalize)
            elif calibration is not None:
                val, idx = model.recommend_calibrated(*[x.to(device) for x in inputs], k=args.top, pool=args.pool,
                                                      exclude_seen=args.exclude_seen, item_bias=item_bias,
                                                      renormalize=args.renormalize, **calibration)
            elif rule is not None:
                val, idx = model.recommend_capped(*[x.to(device) for x in inputs], k=args.top, rule=rule, pool=args.pool,
                                                  exclude_seen=args.exclude_seen, item_bias=item_bias,
                                                  renormalize=args.renormalize)
            else:
                val, idx = model.recommend(*[x.to(device) for x in inputs], k=args.top, exclude_seen=args.exclude_seen,
                                           item_bias=item_bias, renormalize=args.renormalize)
            for ids, vals in zip(idx.cpu().tolist(), val.cpu().tolist()):
                out.write(format_line(ids, vals) + '\n')
    finally:
        if out is not sys.stdout:
            out.close()


if __name__ == '__main__':
    main()
