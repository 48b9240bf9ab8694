"""Layer-restore sweep: the counterpart of the reference's ``layerwise_quant_compare.py`` (:120-231), which scores the all-4-bit model
and then ``[4] * L`` with a few layers restored to 8 bits, and appends both kinds of line to ``restore_{K}_layers.txt`` (the logs
BASELINE.md cites).

The reference runs one pass over the validation set per combination.  Here all combinations are scored in ONE pass
(``harness.validate_many``): each batch goes to the device once and, on a fused ViT / DeiT model, through one engine call that runs
what the lists share once - everything in front of the first restored layer is shared with the baseline (``FrozenPlan.forward_many``).

    python -m diff_vit_amd.restore --model deit_small --restore 1
    python -m diff_vit_amd.restore --model deit_small --restore 4 --max-combos 100 --seed 0
    python -m diff_vit_amd.restore --model deit_small --combos my_combinations.json

Differences the build owns: the reference hard-codes its combinations per K (layerwise_quant_compare.py:22-117, drawn once with
``random.sample``); here they are every K-subset when there are at most ``--max-combos`` of them, else a seeded sample of distinct
sorted subsets, or the caller's own list (``--combos``).  ``Time`` of a line is the sweep's wall time divided by the number of lists,
since no list has a pass of its own.
"""
import itertools
import json
import math
import random
import time

import torch

from . import harness


def enumerate_combinations(n_layers, k, max_combos=200, seed=0):
    """the index lists of a ``--restore k`` sweep over ``n_layers`` layers: every k-subset in lexicographic order when there are at most
    ``max_combos`` of them, else ``max_combos`` distinct sorted subsets drawn with ``random.Random(seed)``, in the order drawn"""
    if not 0 <= k <= n_layers:
        raise ValueError('--restore %d: the model has %d layers' % (k, n_layers))
    if max_combos < 1:
        raise ValueError('--max-combos must be positive')
    if math.comb(n_layers, k) <= max_combos:
        return [list(c) for c in itertools.combinations(range(n_layers), k)]
    rng, seen = random.Random(seed), {}
    while len(seen) < max_combos:
        seen.setdefault(tuple(sorted(rng.sample(range(n_layers), k))))
    return [list(c) for c in seen]


def restored_list(n_layers, indices, base=4, restored=8):
    bc = [base] * n_layers
    for i in indices:
        if not 0 <= int(i) < n_layers:
            raise ValueError('restore index %r outside 0 ... %d' % (i, n_layers - 1))
        bc[int(i)] = restored
    return bc


def restore_sweep(args, loader, model, device, combinations, base=4, restored=8):
    """[(indices, loss, top1, top5), ...]: first the baseline ``[base] * L`` with empty indices, then ``[base] * L`` with the layers of
    every entry of ``combinations`` at ``restored`` bits, in input order; one pass over ``loader`` (``harness.validate_many``)."""
    n = model.bit_config_length() if harness._is_swin(model) else 4 * model.arch['depth'] + 2
    combos = [[]] + [[int(i) for i in c] for c in combinations]
    res = harness.validate_many(args, loader, model, device, [restored_list(n, c, base, restored) for c in combos])
    return [(c,) + tuple(r) for c, r in zip(combos, res)]


def schedule_counts(model, combinations, base=4, restored=8):
    """(blocks the shared schedule runs, blocks of a per-list loop) for the sweep's distinct lists on a frozen ViT / DeiT model, else None"""
    plan = getattr(model, '_plan', None)
    if plan is None or not hasattr(plan, 'forward_many_plan'):
        return None
    n = plan.n_layers
    lists = list(dict.fromkeys(tuple(restored_list(n, c, base, restored)) for c in [[]] + list(combinations)))
    return plan.forward_many_plan(lists)['blocks'], len(lists) * plan.depth


def format_line(indices, top1, top5, seconds):
    """the reference's two line shapes (layerwise_quant_compare.py:171-172,222-223)"""
    if not indices:
        return ' * Restore Index: nothing, Prec@1 {0:.3f} Prec@5 {1:.3f} Time {2:.3f}'.format(top1, top5, seconds)
    return ' *Restore Indices: {0}, Prec@1 {1:.3f} Prec@5 {2:.3f} Time {3:.3f}'.format(list(indices), top1, top5, seconds)


def build_parser():
    p = harness.build_parser()
    p.description = 'layer-restore sweep: [4] * L with a few layers restored to 8 bits (layerwise_quant_compare.py)'
    p.add_argument('--restore', default=1, type=int, metavar='K', help='layers restored per list')
    p.add_argument('--combos', default='', metavar='FILE.json', help='a JSON list of index lists to sweep instead of the K-subsets')
    p.add_argument('--max-combos', default=200, type=int, help='all K-subsets when there are at most this many, else a seeded sample of this size')
    p.add_argument('--out-dir', default='.', help='where restore_{K}_layers.txt is appended to')
    return p


def main(argv=None):
    import argparse
    import os
    args = build_parser().parse_args(argv)
    harness.seed(args.seed)
    device = torch.device(args.device)
    model, loader, train_loader = harness.build_model_and_loaders(args, device)
    harness.calibrate_model(model, harness.calibration_data(args, model, train_loader, device), where=args.calib_on)
    n = model.bit_config_length() if harness._is_swin(model) else 4 * model.arch['depth'] + 2
    if args.combos:
        with open(args.combos) as f:
            combos = [sorted(int(i) for i in c) for c in json.load(f)]
        label = str(len(combos[0])) if combos and len({len(c) for c in combos}) == 1 else 'custom'
    else:
        combos, label = enumerate_combinations(n, args.restore, args.max_combos, args.seed), str(args.restore)
    quiet = argparse.Namespace(**{**vars(args), 'print_freq': 10 ** 9})
    t0 = time.time()
    rows = restore_sweep(quiet, loader, model, device, combos)
    per_list = (time.time() - t0) / len(rows)
    path = os.path.join(args.out_dir, 'restore_%s_layers.txt' % label)
    with open(path, 'a') as f:
        for indices, loss, top1, top5 in rows:
            line = format_line(indices, top1, top5, per_list)
            print(line)
            f.write(line + '\n')
    counts = schedule_counts(model, combos)
    if counts:
        print(' * blocks executed: %d instead of %d (%d lists x depth %d)' % (counts + (counts[1] // model.arch['depth'], model.arch['depth'])))
    print('Results for %s restored layers have been saved to %s' % (label, path))
    return rows


if __name__ == '__main__':
    main()
