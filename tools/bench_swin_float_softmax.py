"""GPU: Config(ptf=True, lis=False) of Swin-B on the engine next to the default configuration and next to the module graph (before
p2v_window_softmax_attention the only way to run it), and - with --parent DIR, a built tree of the parent commit - the check that the
default benchmark did not move: bench.py and bench.py --model swin_base from both trees in turn, throughput and the md5 of the dumped logits.

    python tools/bench_swin_float_softmax.py [--steps 10] [--repeats 5] [--parent DIR]  ->  stdout (profiles/swin_float_softmax.txt is one run)

Per geometry the two models are built once and their timed loops ALTERNATE, so that drift of the device hits both alike; every figure is
the median of the repeats with their smallest and largest value.  The per-launch time of the window-attention kernel of either
configuration comes from p2v_run_ops_profile (HIP events around every launch of one single-stream forward at the whole batch)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diff_vit_amd as dva              # noqa: E402
from diff_vit_amd import swin           # noqa: E402

CASES = (('Swin-B 224^2 / window 7', swin.swin_base_patch4_window7_224, 224, 256, 16),
         ('Swin-B 384^2 / window 12', swin.swin_base_patch4_window12_384, 384, 64, 4))       # (name, factory, image, batch, module-graph batch)


def timed(run, n, warm=1):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def build(factory, img, lis):
    m = factory(cfg=dva.Config(True, lis, 'minmax'))
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, img).cuda())
    return m


def window_launch_us(plan, x):
    us = [1e3 * ms for kind, _, ms in plan.profile(x) if kind in ('window_attention', 'window_softmax_attention')]
    return sum(us) / len(us), len(us)


def engine_cases(steps, repeats):
    for name, factory, img, batch, gb in CASES:
        x = dva.synth.images(5, batch, img, offset=100).cuda()
        models = {lis: build(factory, img, lis) for lis in (True, False)}
        rates, launch = {True: [], False: []}, {True: [], False: []}
        with torch.no_grad():
            for m in models.values():
                m(x)
            for _ in range(repeats):
                for lis, m in models.items():
                    rates[lis].append(batch / timed(lambda: m(x), steps))
            for _ in range(repeats):
                for lis, m in models.items():
                    launch[lis].append(window_launch_us(m._plan, x))
            scales = sorted({float(b['wa'].s_q2) for st in models[False]._plan.stages for b in st['blocks']})
            print('%s, batch %d, 8 bit, %d repeats of %d steps, the two configurations alternating (median [min .. max]); qact2 scales %s'
                  % (name, batch, repeats, steps, scales), flush=True)
            for lis in (True, False):
                r, l = spread(rates[lis]), spread([u for u, _ in launch[lis]])
                print('  Config(ptf=True, lis=%-5s): %9.1f img/s [%9.1f .. %9.1f]; %s %7.1f us per launch [%7.1f .. %7.1f], %d launches'
                      % (lis, r[0], r[1], r[2], 'k_window_attention%s       ' % ('_wide' if img == 384 else '     ') if lis else
                         'k_window_softmax_attention', l[0], l[1], l[2], launch[lis][0][1]), flush=True)
            m = models[False]
            ref = m(x[:gb])
            graph = lambda: m.act_out(m.head(m.forward_features(x[:gb]), m.global_distance))      # noqa: E731  the module graph, layer by layer
            g = spread([gb / timed(graph, 1) for _ in range(3)])
            d = torch.round((graph() - ref) / m._plan.s_out).abs()
            print('  module graph under (True, False), batch %d: %8.1f img/s [%8.1f .. %8.1f]; engine / graph %.0fx; logit codes engine != graph: '
                  '%d of %d (max %d)' % (gb, g[0], g[1], g[2], spread(rates[False])[0] / g[0], int((d > 0).sum()), d.numel(), int(d.max())), flush=True)
        del models, x
        torch.cuda.empty_cache()


def parent_check(parent, steps, warmup, repeats):
    """bench.py of the parent's tree and of this one, a fresh process each, in turn"""
    trees = (('parent', os.path.abspath(parent)), ('this', ROOT))
    for extra in ([], ['--model', 'swin_base']):
        vals, md5 = {'parent': [], 'this': []}, {'parent': set(), 'this': set()}
        for _ in range(repeats):
            for tag, tree in trees:
                with tempfile.TemporaryDirectory() as d:
                    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup), '--no-cpu-baseline',
                                          '--dump-outputs', d] + extra, cwd=tree, check=True, capture_output=True, text=True, timeout=900).stdout
                    vals[tag].append(json.loads(out.strip().splitlines()[-1])['value'])
                    with open(os.path.join(d, 'logits.npy'), 'rb') as f:
                        md5[tag].add(hashlib.md5(f.read()).hexdigest())
        p, t = spread(vals['parent']), spread(vals['this'])
        same = md5['parent'] == md5['this'] and len(md5['this']) == 1
        print('bench.py %-18s parent %9.1f img/s [%9.1f .. %9.1f]   this %9.1f img/s [%9.1f .. %9.1f]   logits md5 %s (%s)'
              % (' '.join(extra) or '(default)', p[0], p[1], p[2], t[0], t[1], t[2], 'equal' if same else 'DIFFER', sorted(md5['this'])[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also run bench.py from both trees in turn')
    ap.add_argument('--bench-steps', type=int, default=30)
    ap.add_argument('--bench-warmup', type=int, default=5)
    ap.add_argument('--bench-repeats', type=int, default=3, help='bench.py runs per tree and model')
    args = ap.parse_args()
    engine_cases(args.steps, args.repeats)
    if args.parent:
        torch.cuda.empty_cache()
        parent_check(args.parent, args.bench_steps, args.bench_warmup, args.bench_repeats)


if __name__ == '__main__':
    main()
