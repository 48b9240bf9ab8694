"""Many bit lists in one call against the per-list loop, on DeiT-S at batch 256 (profiles/forward_many.txt).

    python tools/bench_forward_many.py [--out profiles/forward_many.txt] [--batch 256] [--rounds 5]

Workloads: (a) the 51-list single-restore sweep ([4] * 50 and its 50 single restores); (b) every population that
``harness --mixed --device-metrics --model deit_small --seed 0`` hands to ``validate_many`` (recorded from a run of the harness on a small
synthetic validation set; the distinct lists of each call, as validate_many forwards them).

Legs, alternated within every round, a device synchronisation around each, median of the rounds:
    loop          ``plan.forward`` per list on one stream
    loop/streams  ``plan.forward_streams`` per list (3 side streams): what ``model(x, bc)`` runs at this batch, the per-list path of
                  validate_many before the many-list call
    many          ``plan.forward_many`` on one stream
    many/streams  ``plan.forward_many`` sliced over the same streams: what ``model.forward_many`` runs at this batch
The counted schedule (``forward_many_plan``) stands next to every time, and the logits of both paths are compared for equality."""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import diff_vit_amd as dva  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure(plan, x, lists, rounds):
    B, nc = x.shape[0], plan.arch['num_classes']
    outs = [torch.empty(B, nc, device=x.device) for _ in lists]
    legs = {
        'loop': lambda: [plan.forward(x, bc, out=o) for bc, o in zip(lists, outs)],
        'loop/streams': lambda: [plan.forward_streams(x, bc, o, 3) for bc, o in zip(lists, outs)],
        'many': lambda: plan.forward_many(x, lists),
        'many/streams': lambda: plan.forward_many(x, lists, n_streams=3),
    }
    for fn in legs.values():                       # warm-up: workspaces, streams, the first launch of every kernel
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn)[0])
    ref = torch.stack(legs['loop']())
    same = all(torch.equal(ref, torch.stack(list(legs[k]())) if k.startswith('loop') else legs[k]()) for k in legs)
    return {k: statistics.median(v) for k, v in ms.items()}, ms, same


def report(w, tag, plan, x, lists, rounds):
    lists = [list(k) for k in dict.fromkeys(tuple(l) for l in lists)]
    c = plan.forward_many_plan(lists)
    med, raw, same = measure(plan, x, lists, rounds)
    w('%s: %d distinct lists; blocks %d of %d, stems %d, norms %d, heads %d, x copies %d, snapshot slots %d; logits %s' % (
        tag, len(lists), c['blocks'], len(lists) * plan.depth, c['stems'], c['norms'], c['heads'], c['copies'], c['snapshots'],
        'byte-equal on all four legs' if same else 'DIFFER'))
    for k in med:
        w('    %-13s %8.2f ms  [%s]' % (k, med[k], ' '.join('%.2f' % v for v in raw[k])))
    w('    many / loop %.3f, many/streams / loop/streams %.3f (blocks ratio %.3f)' % (
        med['many'] / med['loop'], med['many/streams'] / med['loop/streams'], c['blocks'] / (len(lists) * plan.depth)))
    return med, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forward_many.txt'))
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--n-val', type=int, default=64, help='synthetic validation images of the recorded harness run')
    a = ap.parse_args()
    assert a.rounds >= 3
    H = dva.harness
    recorded, real = [], H.validate_many
    H.validate_many = lambda args, loader, model, device, cfgs: (recorded.append([list(c) for c in cfgs]), real(args, loader, model, device, cfgs))[1]
    models, build = [], H.build_model_and_loaders
    H.build_model_and_loaders = lambda *x: (lambda r: (models.append(r[0]), r)[1])(build(*x))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            H.main(['--model', 'deit_small', '--seed', '0', '--quant', '--mixed', '--device-metrics', '--n-val', str(a.n_val), '--val-batchsize',
                    str(a.n_val), '--calib-batchsize', '8'])
    finally:
        H.validate_many, H.build_model_and_loaders = real, build
    model = models[0]
    plan = model._plan
    x = dva.synth.images(5, a.batch, plan.arch['img_size']).to(plan.device)
    lines = []

    def w(s):
        print(s, flush=True)
        lines.append(s)
    w('bench_forward_many: deit_small (seeded synthetic weights, calibrated by the harness), batch %d, %d rounds, median; torch %s, %s' % (
        a.batch, a.rounds, torch.__version__, torch.cuda.get_device_name(0)))
    n = plan.n_layers
    sweep = [[4] * n] + [[8 if j == i else 4 for j in range(n)] for i in range(n)]
    report(w, '(a) single-restore sweep', plan, x, sweep, a.rounds)
    tot = {k: 0.0 for k in ('loop', 'loop/streams', 'many', 'many/streams')}
    blocks = [0, 0]
    w('(b) harness --mixed --device-metrics --model deit_small --seed 0: %d calls of validate_many' % len(recorded))
    for i, cfgs in enumerate(recorded):
        med, c = report(w, '  call %d' % i, plan, x, cfgs, a.rounds)
        for k in tot:
            tot[k] += med[k]
        blocks[0] += c['blocks']
        blocks[1] += len(dict.fromkeys(tuple(l) for l in cfgs)) * plan.depth
    w('(b) all calls, one batch each: loop %.1f ms, loop/streams %.1f ms, many %.1f ms, many/streams %.1f ms; blocks %d of %d' % (
        tot['loop'], tot['loop/streams'], tot['many'], tot['many/streams'], blocks[0], blocks[1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
