"""Shared driver of the four launcher scripts.  Flag names, defaults and printed strings follow the
reference CLIs (main_lessr.py:7-53, main_niser.py:7-53, main_msgifsr.py:35-112); main_srgnn.py is the
script start.sh:6 expects but the reference never shipped.  GPU selection is ROCm
aware (HIP_VISIBLE_DEVICES / first device) instead of shelling out to nvidia-smi (quirk 4)."""
import argparse
import os
import random
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
sys.path.insert(0, str(HERE.parents[2]))
sys.path.insert(0, str(HERE.parents[1]))

DEFAULTS = {
    'LESSR': dict(embedding_dim=32, num_layers=3, feat_drop=0.2, batch_size=512, patience=2, num_workers=0),
    'NISER': dict(embedding_dim=64, num_layers=2, feat_drop=0.5, batch_size=128, patience=2, num_workers=4),
    'SRGNN': dict(embedding_dim=64, num_layers=2, feat_drop=0.5, batch_size=128, patience=2, num_workers=4),
    'MSGIFSR': dict(embedding_dim=256, num_layers=1, feat_drop=0.1, batch_size=512, patience=3, num_workers=4),
}


def _cutoffs(text):
    ks = tuple(int(k) for k in text.split(',') if k.strip())
    if not ks or min(ks) < 1:
        raise argparse.ArgumentTypeError('expected positive cutoffs separated by commas, e.g. 5,10,20')
    return ks


def eval_options(args):
    """the TrainRunner keywords of --eval-method / --eval-cutoffs"""
    return dict(eval_method=args.eval_method, eval_cutoffs=args.eval_cutoffs)


def model_flags(p, model):
    """the flags every model is built from (shared with scripts/recommend.py)"""
    d = DEFAULTS[model]
    p.add_argument('--dataset-dir', default='../datasets/sample', help='the dataset directory')
    p.add_argument('--embedding-dim', type=int, default=d['embedding_dim'], help='the embedding size')
    p.add_argument('--num-layers', type=int, default=d['num_layers'], help='the number of layers')
    p.add_argument('--feat-drop', type=float, default=d['feat_drop'], help='the dropout ratio for features')


def variant_flags(p, model):
    """... and the ones only MSGIFSR has"""
    if model == 'MSGIFSR':
        p.add_argument('--order', type=int, default=3, help='order of msg')
        p.add_argument('--reducer', type=str, default='mean', help='method for reducer')
        p.add_argument('--norm', type=bool, default=True, help='whether use l2 norm')
        p.add_argument('--extra', action='store_true', help='whether use REnorm.')
        p.add_argument('--fusion', action='store_true', help='whether use IFR.')


def catalog_flags(p):
    """the catalogue controls of scripts/recommend.py and scripts/rerank.py (ops.catalog_bias combines them)"""
    p.add_argument('--allow', default=None, metavar='FILE', help='only these items may be returned: one item id per line')
    p.add_argument('--deny', default=None, metavar='FILE', help='these items are never returned: one item id per line')
    p.add_argument('--item-bias', default=None, metavar='FILE',
                   help='added to the log-probabilities before ranking: one `id:value` or `id<TAB>value` per line, unnamed items get 0')


def read_id_file(path):
    """[item id, ...]: one id per non-empty line; ValueError names the line that is none"""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if line:
                try:
                    out.append(int(line))
                except ValueError:
                    raise ValueError('%s line %d: `%s` is no item id' % (path, n, line)) from None
    return out


def read_bias_file(path):
    """([item id, ...], [value, ...]): one `id:value` or `id<TAB>value` per non-empty line; ValueError names the line that is
    malformed or whose value is not finite"""
    import math
    ids, vals = [], []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split('\t') if '\t' in line else line.split(':')
            try:
                if len(parts) != 2:
                    raise ValueError
                i, v = int(parts[0]), float(parts[1])
            except ValueError:
                raise ValueError('%s line %d: `%s` is not `id:value` or `id<TAB>value`' % (path, n, line)) from None
            if not math.isfinite(v):
                raise ValueError('%s line %d: the value of item %d is not finite (use --deny to remove an item)' % (path, n, i))
            ids.append(i)
            vals.append(v)
    return ids, vals


def read_catalog(p, args):
    """the keywords of ops.catalog_bias from --allow / --deny / --item-bias, or None when none is given.  Read and checked
    against <dataset-dir>/num_items.txt before any model is built; p.error() for a file that cannot be read, an id outside the
    catalogue, a value that is not finite and an --allow that names nothing."""
    if args.allow is None and args.deny is None and args.item_bias is None:
        return None
    kw = {}
    try:
        with open(Path(args.dataset_dir) / 'num_items.txt') as f:
            num_items = int(f.readline())
        if args.allow is not None:
            kw['allow'] = read_id_file(args.allow)
            if not kw['allow']:
                p.error('--allow %s names no item: nothing could be returned' % args.allow)
        if args.deny is not None:
            kw['deny'] = read_id_file(args.deny)
        if args.item_bias is not None:
            kw['boost'] = read_bias_file(args.item_bias)
    except (OSError, ValueError) as e:
        p.error(str(e))
    for flag, ids in (('--allow', kw.get('allow', [])), ('--deny', kw.get('deny', [])), ('--item-bias', kw.get('boost', ([], []))[0])):
        bad = [i for i in ids if not 0 <= i < num_items]
        if bad:
            p.error('%s: item id %d; ids are in [0, %d)' % (flag, bad[0], num_items))
    return kw


def cap_flags(p):
    """the per-category caps of scripts/recommend.py (ops.cap_rule builds the rule, model.recommend_capped applies it)"""
    p.add_argument('--categories', default=None, metavar='FILE',
                   help='the category (brand, seller) of the items: one `id:category` per line, categories are integers >= 0; '
                        'an unlisted item has none and is never capped')
    p.add_argument('--max-per-category', type=int, default=None, metavar='N',
                   help='--categories: at most N items of one category in every printed list (0: none at all)')
    p.add_argument('--category-caps', default=None, metavar='FILE',
                   help='--categories: one `category:cap` per line, instead of N for the categories it names')


def read_pair_file(path, what):
    """([first, ...], [second, ...]): one `first:second` pair of integers per non-empty line (`what` names the format);
    ValueError names the line that is none"""
    a, b = [], []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            parts = line.split(':')
            try:
                if len(parts) != 2:
                    raise ValueError
                a.append(int(parts[0]))
                b.append(int(parts[1]))
            except ValueError:
                raise ValueError('%s line %d: `%s` is not `%s`' % (path, n, line, what)) from None
    return a, b


MAX_CATEGORIES = 16384      # SREC_CAP_MAXG (include/srec.h)


def read_caps(p, args):
    """the keywords item_category / max_per_category of model.recommend_capped from --categories / --max-per-category /
    --category-caps, or None when none is given.  Read and checked against <dataset-dir>/num_items.txt before any model is
    built; p.error() for a cap flag without --categories, --categories without a cap, a file that cannot be read, an item
    outside the catalogue, an item named twice, a category outside [0, MAX_CATEGORIES) and a negative cap.  A category without
    a cap of its own (--category-caps alone) is not capped."""
    if args.categories is None:
        if args.max_per_category is not None or args.category_caps is not None:
            p.error('--max-per-category / --category-caps cap the categories of --categories: give the file')
        return None
    if args.max_per_category is None and args.category_caps is None:
        p.error('--categories goes with --max-per-category N or --category-caps FILE')
    if args.max_per_category is not None and args.max_per_category < 0:
        p.error('--max-per-category must be >= 0')
    try:
        with open(Path(args.dataset_dir) / 'num_items.txt') as f:
            num_items = int(f.readline())
        ids, cats = read_pair_file(args.categories, 'id:category')
        named = read_pair_file(args.category_caps, 'category:cap') if args.category_caps is not None else ([], [])
    except (OSError, ValueError) as e:
        p.error(str(e))
    item_category = [-1] * num_items
    for i, c in zip(ids, cats):
        if not 0 <= i < num_items:
            p.error('--categories: item id %d; ids are in [0, %d)' % (i, num_items))
        if not 0 <= c < MAX_CATEGORIES:
            p.error('--categories: category %d of item %d; categories are in [0, %d)' % (c, i, MAX_CATEGORIES))
        if item_category[i] >= 0:
            p.error('--categories: item %d is named twice' % i)
        item_category[i] = c
    for c, m in zip(*named):
        if not 0 <= c < MAX_CATEGORIES:
            p.error('--category-caps: category %d; categories are in [0, %d)' % (c, MAX_CATEGORIES))
        if m < 0:
            p.error('--category-caps: the cap %d of category %d; a cap is >= 0' % (m, c))
    caps = [2 ** 31 - 1 if args.max_per_category is None else min(args.max_per_category, 2 ** 31 - 1)] * (max(cats + named[0] + [0]) + 1)
    for c, m in zip(*named):
        caps[c] = min(m, 2 ** 31 - 1)
    return dict(item_category=item_category, max_per_category=caps)


def calibrate_flags(p):
    """the calibrated slates of scripts/recommend.py (model.recommend_calibrated)"""
    p.add_argument('--calibrate', type=float, default=None, metavar='W',
                   help='--categories: re-rank the --pool most probable items into a slate whose category mix follows the '
                        'session\'s own: each pick maximises (1 - W) * value - W * KL(target, list so far); W in [0, 1]; printed '
                        'in pick order')
    p.add_argument('--calibrate-smooth', type=float, default=None, metavar='A',
                   help='--calibrate: the smoothing of the KL term, 0 < A < 1 (default: 0.01)')


def read_calibration(p, args):
    """the keywords item_category / weight / alpha of model.recommend_calibrated from --calibrate / --calibrate-smooth /
    --categories, or None without --calibrate.  Read and checked against <dataset-dir>/num_items.txt before any model is
    built; p.error() for --calibrate-smooth alone, --calibrate without --categories or with a cap flag, a number out of
    range, a file that cannot be read, an item outside the catalogue, an item named twice and a category outside
    [0, 2^31)."""
    if args.calibrate is None:
        if args.calibrate_smooth is not None:
            p.error('--calibrate-smooth smooths the term of --calibrate W: give the weight')
        return None
    if args.categories is None:
        p.error('--calibrate follows the category mix of the session: give --categories FILE (`id:category` per line)')
    if args.max_per_category is not None or args.category_caps is not None:
        p.error('--calibrate is the soft counterpart of --max-per-category / --category-caps: give one of the two')
    if not 0.0 <= args.calibrate <= 1.0:
        p.error('--calibrate must be in [0, 1]')
    alpha = 0.01 if args.calibrate_smooth is None else args.calibrate_smooth
    if not 0.0 < alpha < 1.0:
        p.error('--calibrate-smooth must be in (0, 1)')
    try:
        with open(Path(args.dataset_dir) / 'num_items.txt') as f:
            num_items = int(f.readline())
        ids, cats = read_pair_file(args.categories, 'id:category')
    except (OSError, ValueError) as e:
        p.error(str(e))
    item_category = [-1] * num_items
    for i, c in zip(ids, cats):
        if not 0 <= i < num_items:
            p.error('--categories: item id %d; ids are in [0, %d)' % (i, num_items))
        if not 0 <= c < 2 ** 31:
            p.error('--categories: category %d of item %d; categories are in [0, 2^31)' % (c, i))
        if item_category[i] >= 0:
            p.error('--categories: item %d is named twice' % i)
        item_category[i] = c
    return dict(item_category=item_category, weight=args.calibrate, alpha=alpha)


def personal_flags(p):
    """the per-session hide / boost lists of scripts/recommend.py (model.recommend_personal)"""
    p.add_argument('--hide', default=None, metavar='FILE',
                   help='items a session is never shown: line i holds those of session i, separated by commas or tabs (`id` or '
                        '`id:anything`, so an output file of this script is one: page 2 is --hide page1.txt); ONE line serves all '
                        'sessions; -1 or an empty line: none')
    p.add_argument('--session-bias', default=None, metavar='FILE',
                   help='added to the log-probability of the named items of a session before ranking: the layout of --hide with '
                        '`id:value` entries; an id in both files is hidden')


MAX_PERSONAL = 1024         # SREC_PERSONAL_MAXM (include/srec.h)


def read_personal_file(path, valued):
    """[{item id: value}, ...], one dict per line of the file (an empty line: an empty dict): entries separated by commas or
    tabs, `id` or `id:anything` (valued: `id:value`, the value a number that is neither NaN nor +inf); -1 names nothing.
    ValueError names the line that is malformed or names an id twice"""
    out = []
    with open(path) as f:
        for n, line in enumerate(f.read().splitlines(), 1):
            row = {}
            for entry in filter(None, (e.strip() for e in line.replace('\t', ',').split(','))):
                head, sep, tail = entry.partition(':')
                try:
                    i = int(head)
                    v = float(tail) if valued else float('-inf')
                    if valued and (not sep or v != v or v == float('inf')):
                        raise ValueError
                except ValueError:
                    raise ValueError('%s line %d: `%s` is not `%s`' % (path, n, entry, 'id:value' if valued else 'id` or `id:anything')) from None
                if i == -1:
                    continue
                if i in row:
                    raise ValueError('%s line %d: item %d is named twice' % (path, n, i))
                row[i] = v
            out.append(row)
    return out


def read_personal(p, args, n_sessions):
    """the keywords personal_items / personal_bias of model.recommend_personal from --hide / --session-bias, as Python lists
    with one row per session or ONE row for all of them (personal_bias None with --hide alone), or None when neither is given.
    Read and checked against <dataset-dir>/num_items.txt and the number of sessions before any model is built; p.error() for
    a file that cannot be read, a malformed entry, an id outside the catalogue or twice on a line, more than MAX_PERSONAL
    entries on a line and a line count that is neither 1 nor the number of sessions.  An id in both files is hidden."""
    if args.hide is None and args.session_bias is None:
        return None
    try:
        with open(Path(args.dataset_dir) / 'num_items.txt') as f:
            num_items = int(f.readline())
        files = [(flag, read_personal_file(path, valued)) for flag, path, valued in
                 (('--session-bias', args.session_bias, True), ('--hide', args.hide, False)) if path is not None]
    except (OSError, ValueError) as e:
        p.error(str(e))
    for flag, rows in files:
        if len(rows) not in (1, n_sessions):
            p.error('%s: %d lines for %d sessions; one line per session, or ONE line for all of them' % (flag, len(rows), n_sessions))
        for n, row in enumerate(rows, 1):
            bad = [i for i in row if not 0 <= i < num_items]
            if bad:
                p.error('%s line %d: item id %d; ids are in [0, %d), or -1 for none' % (flag, n, bad[0], num_items))
    merged = [{} for _ in range(max(len(rows) for _, rows in files))]
    for _, rows in files:                           # (--hide last: an id in both files is hidden)
        for n, m in enumerate(merged):
            m.update(rows[n if len(rows) > 1 else 0])
    for n, m in enumerate(merged, 1):
        if len(m) > MAX_PERSONAL:
            p.error('--hide / --session-bias line %d: %d items; at most %d per session' % (n, len(m), MAX_PERSONAL))
    items = [sorted(m) or [-1] for m in merged]
    bias = None if args.session_bias is None else [[m.get(i, 0.0) for i in row] for row, m in zip(items, merged)]
    return dict(personal_items=items, personal_bias=bias)


def build_model(model_name, args, num_items, device, caps=None):
    """(model on the CPU, evaluation collate_fn, training collate_fn) of a launcher's flags (run, scripts/recommend.py)"""
    from src.models import LESSR, MSGIFSR, NISER, SRGNN
    from src.utils.data.collate import (collate_fn_factory, collate_fn_factory_ccs, seq_to_ccs_graph,
                                        seq_to_eop_multigraph, seq_to_session_graph, seq_to_shortcut_graph)
    if model_name == 'LESSR':
        fns = (seq_to_eop_multigraph, seq_to_shortcut_graph) if args.num_layers > 1 else (seq_to_eop_multigraph,)
        collate_fn = collate_fn_factory(*fns)
        train_collate_fn = collate_fn_factory(*fns, caps=caps)
        model = LESSR(num_items, args.embedding_dim, args.num_layers, feat_drop=args.feat_drop)
    elif model_name == 'MSGIFSR':
        collate_fn = collate_fn_factory_ccs((seq_to_ccs_graph,), order=args.order)
        train_collate_fn = collate_fn_factory_ccs((seq_to_ccs_graph,), order=args.order, caps=caps)
        model = MSGIFSR(num_items, args.dataset_dir, args.embedding_dim, args.num_layers, dropout=args.feat_drop,
                        reducer=args.reducer, order=args.order, norm=args.norm, extra=args.extra, fusion=args.fusion,
                        device=device)
    else:
        collate_fn = collate_fn_factory(seq_to_session_graph)
        train_collate_fn = collate_fn_factory(seq_to_session_graph, caps=caps)
        cls = NISER if model_name == 'NISER' else SRGNN
        model = cls(num_items, args.embedding_dim, args.num_layers, feat_drop=args.feat_drop)
    return model, collate_fn, train_collate_fn


def parse(model):
    d = DEFAULTS[model]
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    model_flags(p, model)
    p.add_argument('--lr', type=float, default=1e-3, help='the learning rate')
    p.add_argument('--batch-size', type=int, default=d['batch_size'], help='the batch size for training')
    p.add_argument('--epochs', type=int, default=30, help='the number of training epochs')
    p.add_argument('--weight-decay', type=float, default=1e-4, help='the parameter for L2 regularization')
    p.add_argument('--patience', type=int, default=d['patience'],
                   help='the number of epochs that the performance does not improves after which the training stops')
    p.add_argument('--num-workers', type=int, default=d['num_workers'],
                   help='the number of processes to load the input graphs')
    p.add_argument('--valid-split', type=float, default=None, help='the fraction for the validation set')
    p.add_argument('--log-interval', type=int, default=100, help='print the loss after this number of iterations')
    p.add_argument('--precision', default=os.environ.get('SREC_PRECISION', 'fp32'), choices=['fp32', 'bf16'],
                   help='(not in the reference) fp32: results match the reference to fp32 round-off; bf16: bf16 MFMA operands '
                        'with fp32 accumulation and master weights (BASELINE config C3), ~2x faster, metrics within 0.03 pt')
    p.add_argument('--no-graph', action='store_true',
                   help='(not in the reference) eager launches instead of replaying one captured hipGraph per training step')
    p.add_argument('--checkpoint', default=None,
                   help='(not in the reference) write a resumable checkpoint here after every epoch; resume from it if present')
    p.add_argument('--loader', default='ring', choices=['ring', 'torch'],
                   help='(not in the reference) ring: worker processes collate straight into a shared pinned ring '
                        '(sessionrec-pytorch_amd/loader.py); torch: torch.utils.data.DataLoader as in the reference')
    p.add_argument('--metrics-log', default=None, help='(not in the reference) append one JSON line per logged interval / epoch')
    p.add_argument('--gpus', type=int, default=int(os.environ.get('SREC_GPUS', '1')),
                   help='(not in the reference) train on this many GPUs of the node: item table row-sharded over them (RCCL), '
                        'encoder replicated, every rank encoding its slice of each --batch-size batch (same loss as one GPU)')
    p.add_argument('--eval-method', default='topk', choices=['topk', 'rank'],
                   help='(not in the reference) topk: the reference evaluation (MRR@20 / HR@20 from the 20 best items); rank: the '
                        "label's rank among ALL items in one fused pass - any cutoff, and no (B, V) score matrix for --extra / "
                        '--fusion either (with --extra: sessions of at most 64 distinct items)')
    p.add_argument('--eval-cutoffs', type=_cutoffs, default=None, metavar='K1,K2,...',
                   help='(not in the reference) also report HR / MRR / NDCG at these cutoffs after every epoch, e.g. 5,10,20')
    variant_flags(p, model)
    args = p.parse_args()
    if args.eval_method == 'topk' and args.eval_cutoffs and max(args.eval_cutoffs) > 32:
        p.error('--eval-cutoffs above 32 need --eval-method rank (the top-K evaluation keeps at most 32 items per session)')
    if int(os.environ.get('RANK', '0')) == 0:
        print(args)
    return args


def seed_all(seed=123):
    import numpy as np
    import torch
    random.seed(seed)
    os.environ['PYTHONHASHSEED'] = str(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


def _jsonl(path):
    import json

    def hook(event):
        with open(path, 'a') as f:
            f.write(json.dumps(event) + '\n')
    return hook


def _launch_ranks(n):
    """`--gpus N` outside a torchrun environment: re-execute this launcher under torch.distributed.run, one rank per GPU"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '8')
    env.pop('HIP_VISIBLE_DEVICES', None)          # start.sh pins one device for the single-GPU case
    cmd = [sys.executable, '-u', '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(sys.argv[0])] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def run(model_name):
    args = parse(model_name)
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        _launch_ranks(args.gpus)
    seed_all(123)
    import torch as th
    from torch.utils.data import DataLoader, SequentialSampler
    from src.utils.data.dataset import AugmentedDataset, read_dataset
    from src.utils.train import TrainRunner

    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    sharded = world > 1 or bool(os.environ.get('SREC_FORCE_COLLECTIVES'))
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29544')
        dist.init_process_group('nccl' if th.cuda.is_available() else 'gloo', rank=rank, world_size=world)
        if th.cuda.is_available():
            th.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        if rank != 0:
            sys.stdout = open(os.devnull, 'w')            # one log, rank 0's
    device = th.device('cuda', th.cuda.current_device()) if th.cuda.is_available() else th.device('cpu')
    if device.type == 'cuda':
        from importlib import import_module
        import_module('sessionrec-pytorch_amd.ops').set_precision(args.precision)
        if args.precision == 'fp32':
            print('precision fp32 (reference numerics); --precision bf16 runs the same step about twice as fast')
    print('reading dataset')
    train_sessions, test_sessions, num_items = read_dataset(Path(args.dataset_dir))
    if args.valid_split is not None:
        num_valid = int(len(train_sessions) * args.valid_split)
        test_sessions = train_sessions[-num_valid:]
        train_sessions = train_sessions[:-num_valid]
    train_set, test_set = AugmentedDataset(train_sessions), AugmentedDataset(test_sessions)
    caps = None
    shuffled = model_name in ('NISER', 'SRGNN')
    per_rank = (args.batch_size + world - 1) // world        # sessions one rank encodes per step
    if sharded:
        # every rank must present the SAME padded layout sizes to the collectives in every step: capacities are mandatory
        # and must never overflow - exact maxima of the epoch for the sequential loaders, worst case for the shuffled ones
        from src.utils.data.collate import default_caps, estimate_caps
        max_len = int(train_set.index[:, 1].max()) if len(train_set) else 1
        caps = (default_caps(per_rank, max_len) if shuffled else
                estimate_caps(train_set, per_rank, headroom=1.0, slices=(args.batch_size, world)))
        if model_name == 'LESSR':
            caps = dict(caps, E=caps['N'] * max(7, max_len))
    elif device.type == 'cuda' and not args.no_graph and not getattr(args, 'extra', False):
        from src.utils.data.collate import estimate_caps, measure_caps
        # capacity-padded training batches -> whole-step hipGraph replay.  MSGIFSR / SRGNN / NISER: capacities MEASURED on the
        # epoch's largest batches (tight: kernels whose grid follows the capacity pay for slack); LESSR: the click-count bound
        if model_name == 'LESSR':
            caps = estimate_caps(train_set, args.batch_size, shuffled=shuffled)
            caps = dict(caps, E=caps['N'] * 7)               # shortcut graphs: up to L(L+1)/2 edges per session
        else:
            caps = measure_caps(train_set, args.batch_size, 'ccs' if model_name == 'MSGIFSR' else 'session',
                                getattr(args, 'order', 1), shuffled=shuffled)
    print(len(train_set))
    print(len(test_set))
    model, collate_fn, train_collate_fn = build_model(model_name, args, num_items, device, caps)
    pin = device.type == 'cuda'          # pinned batches: asynchronous H2D copies

    def ring(batch_sampler):
        # single-graph capacity-padded training batches: built by the workers INSIDE a shared pinned ring (no pickling, no
        # pinning pass in this process); anything else keeps the DataLoader
        if args.loader != 'ring' or device.type != 'cuda' or (model_name == 'LESSR' and args.num_layers > 1):
            return None
        from importlib import import_module
        kind = {'MSGIFSR': 'ccs', 'LESSR': 'eop'}.get(model_name, 'session')
        return import_module('sessionrec-pytorch_amd.loader').ring_loader_or_none(
            train_set, batch_sampler, kind, getattr(args, 'order', 1), caps, args.num_workers)
    pw = args.num_workers > 0            # keep the loader processes across epochs (a respawn costs seconds per epoch)
    # reference loaders: LESSR / MSGIFSR train in time order (SequentialSampler), NISER shuffles; test shuffles
    if sharded:
        # the reference's batches (order and membership), each rank collating its contiguous slice of every batch
        from importlib import import_module
        from torch.utils.data import RandomSampler
        RankSlice = import_module('sessionrec-pytorch_amd.dataset').RankSliceBatchSampler
        base = (RandomSampler(train_set, generator=th.Generator().manual_seed(123)) if shuffled
                else SequentialSampler(train_set))
        slices = RankSlice(base, args.batch_size, rank, world, prefix_len=train_set.index[:, 1],
                           need_len=(args.order + 1) if model_name == 'MSGIFSR' else None)
        train_loader = ring(slices) or DataLoader(train_set, batch_sampler=slices, num_workers=args.num_workers,
                                                  collate_fn=train_collate_fn, pin_memory=pin, persistent_workers=pw)
        # evaluation: every rank scores the same sessions against its rows (order does not enter the metrics)
        test_loader = DataLoader(test_set, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                                 collate_fn=collate_fn, persistent_workers=pw)
    elif model_name in ('LESSR', 'MSGIFSR'):
        from torch.utils.data import BatchSampler
        train_loader = (ring(BatchSampler(SequentialSampler(train_set), args.batch_size, drop_last=False)) or
                        DataLoader(train_set, batch_size=args.batch_size, num_workers=args.num_workers, collate_fn=train_collate_fn,
                                   sampler=SequentialSampler(train_set), pin_memory=pin, persistent_workers=pw))
        test_loader = None
    else:
        from torch.utils.data import BatchSampler, RandomSampler
        # (the shuffle has its own seeded generator: the batch order of a run does not depend on what else draws from
        #  torch's global stream)
        shuffle = RandomSampler(train_set, generator=th.Generator().manual_seed(123))
        train_loader = (ring(BatchSampler(shuffle, args.batch_size, drop_last=False)) or
                        DataLoader(train_set, batch_size=args.batch_size, sampler=shuffle, num_workers=args.num_workers,
                                   collate_fn=train_collate_fn, pin_memory=pin, persistent_workers=pw))
        test_loader = None
    if test_loader is None:
        test_loader = DataLoader(test_set, batch_size=args.batch_size, shuffle=True, num_workers=args.num_workers,
                                 collate_fn=collate_fn, persistent_workers=pw)
    model = model.to(device)
    print(model)
    shard = None
    if sharded:
        from importlib import import_module
        shard = import_module('sessionrec-pytorch_amd.dist').VocabParallel(model, idx_cap=caps['U'])
        print(f'item table row-sharded over {world} ranks ({shard.per} rows each), {per_rank} sessions per rank and step')
    runner = TrainRunner(args.dataset_dir, model, train_loader, test_loader, device=device, lr=args.lr,
                         weight_decay=args.weight_decay, patience=args.patience, checkpoint=args.checkpoint,
                         hooks=[_jsonl(args.metrics_log)] if args.metrics_log and rank == 0 else (),
                         graph=False if args.no_graph else 'auto', shard=shard, **eval_options(args))
    print('start training')
    mrr, hit = runner.train(args.epochs, args.log_interval)
    if runner.graph_steps:
        print(f'training steps: {runner.graph_steps} hipGraph replays, {runner.eager_steps} eager')
    if sharded and getattr(slices, 'short_batches', 0):
        print(f'note: {slices.short_batches} global batches had no session of {slices.need_len} clicks - on those the row-sharded '
              'step keeps the residual / bias of relations without edges (single-device skips them: dataset.RankSliceBatchSampler)')
    print('MRR@20\tHR@20')
    print(f'{mrr * 100:.3f}%\t{hit * 100:.3f}%')
    if sharded:
        sys.stdout.flush()
        dist.barrier()
        dist.destroy_process_group()
