"""The entropy term of the data-free calibration images (diff_vit_amd.psaq): fused HIP operator against the torch composition the
reference runs, on one GPU, in one process, alternating, three repeats.  -> profiles/psaq.txt

    python tools/bench_psaq.py [--batch 32] [--repeats 3] [--steps 3]

  1. one loss evaluation: value and gradient of the term over every block, on random ``attn @ v`` tensors of the model's shapes
     (DeiT-S: 12 blocks of [32, 6, 197, 64]; Swin-T: 2 + 2 + 6 + 2 blocks of 64 / 16 / 4 / 1 windows of 49 tokens, head_dim 32) -
     wall time between two synchronisations (what a step pays, host work included) and torch.cuda.max_memory_allocated above the inputs
  2. one ``generate_data`` step on DeiT-S (float forward, loss, backward, Adam) with each loss: how much of a step the term is"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diff_vit_amd as dva  # noqa: E402

SHAPES = {'deit_small': [(1, 6, 197, 64)] * 12,
          'swin_tiny': [(64, 3, 49, 32)] * 2 + [(16, 6, 49, 32)] * 2 + [(4, 12, 49, 32)] * 6 + [(1, 24, 49, 32)] * 2}


def loss_eval(avs, groups, fn):
    for a in avs:
        a.grad = None
    total = 0
    for a, g in zip(avs, groups):
        total = total - fn(a, g)
    total.backward()
    return total.detach()


def timed(fn, n=3):
    """(seconds per call, peak bytes above what was allocated before)"""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, torch.cuda.max_memory_allocated() - base


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--batch', default=32, type=int)
    p.add_argument('--repeats', default=3, type=int)
    p.add_argument('--steps', default=3, type=int, help='generate_data steps per epoch in part 2')
    args = p.parse_args(argv)
    dev = torch.device('cuda')
    print('device: %s, batch %d' % (torch.cuda.get_device_name(0), args.batch))
    fns = (('fused op', dva.psaq.patch_similarity_entropy), ('torch composition', dva.psaq.patch_similarity_entropy_torch))
    for model, shapes in SHAPES.items():
        gen = torch.Generator().manual_seed(1)
        avs = [torch.randn(args.batch * g, h, n, d, generator=gen).to(dev).requires_grad_(True) for g, h, n, d in shapes]
        groups = [s[0] for s in shapes]
        vals = {name: float(loss_eval(avs, groups, fn)) for name, fn in fns}
        print('%s: %d blocks, loss %s' % (model, len(shapes), ', '.join('%s %.6f' % kv for kv in vals.items())))
        rows = {name: [] for name, _ in fns}
        for r in range(args.repeats):
            for name, fn in fns:
                rows[name].append(timed(lambda: loss_eval(avs, groups, fn)))
        for name, _ in fns:
            ms = [t * 1e3 for t, _ in rows[name]]
            print('  %-18s %s ms per loss evaluation (min %.3f, spread %.3f); peak memory %.1f MiB'
                  % (name, ' '.join('%8.3f' % m for m in ms), min(ms), max(ms) - min(ms), max(b for _, b in rows[name]) / 2 ** 20))
        a, b = [t for t, _ in rows['fused op']], [t for t, _ in rows['torch composition']]
        print('  fused op faster by %.2fx (slowest fused %.3f ms against fastest composition %.3f ms)' % (min(b) / min(a), max(a) * 1e3, min(b) * 1e3))
        del avs
        torch.cuda.empty_cache()
    m = dva.deit_small_patch16_224(cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(m.arch, 0), strict=False)
    m = m.to(dev).eval()
    print('generate_data on deit_small, batch %d, 2 x %d steps:' % (args.batch, args.steps))
    for r in range(args.repeats):
        for name, loss in (('engine', 'engine'), ('torch', 'torch')):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            dva.generate_data(m, args.batch, iterations=args.steps, seed=1, loss=loss)
            torch.cuda.synchronize()
            print('  loss=%-7s %8.2f ms per step, peak memory %.0f MiB' % (name, (time.perf_counter() - t0) / (2 * args.steps) * 1e3,
                                                                          torch.cuda.max_memory_allocated() / 2 ** 20))


if __name__ == '__main__':
    main()
