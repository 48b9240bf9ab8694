"""GPU: Config(ptf=False) of Swin-T and Swin-B on the engine next to the three configurations the Swin plans served before, the per-launch
time of the float LayerNorm at every Swin width (up to 2048 channels a row per wave, k_float_layernorm; beyond that a row per workgroup,
k_float_layernorm_xwide), and - with --parent DIR, a built tree of the parent commit - the check that nothing else moved: bench.py and
bench.py --model swin_base from both trees in turn (throughput and the md5 of the dumped logits), and tools/kernel_resources.py --digest of
both libraries (every kernel of the parent present with the same name, resources and code hash; the added kernels listed).

    python tools/bench_swin_float_ln.py [--steps 10] [--repeats 5] [--parent DIR]  ->  stdout (profiles/swin_float_ln.txt is one run)

The four models of a geometry are built once and their timed loops ALTERNATE, so that drift of the device hits all alike; every figure is
the median of the repeats with their smallest and largest value."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diff_vit_amd as dva              # noqa: E402
from diff_vit_amd import engine as E    # noqa: E402
from diff_vit_amd import swin           # noqa: E402
from bench_swin_float_softmax import parent_check, spread, timed      # noqa: E402

CASES = (('Swin-T', swin.swin_tiny_patch4_window7_224), ('Swin-B', swin.swin_base_patch4_window7_224))
CONFIGS = ((True, True), (True, False), (False, True), (False, False))
# stage widths and 4 * C merge widths of Swin-T/S (96 ...), Swin-B (128 ...) and Swin-L (192 ...)
WIDTHS = (96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072)
ROWS = 256 * 49          # the rows of the last merge norm / the final norm at batch 256


def build(factory, cfg):
    m = factory(cfg=dva.Config(cfg[0], cfg[1], 'minmax'))
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
    return m


def engine_cases(batch, steps, repeats):
    x = dva.synth.images(5, batch, 224, offset=100).cuda()
    for name, factory in CASES:
        models = {cfg: build(factory, cfg) for cfg in CONFIGS}
        rates = {cfg: [] for cfg in CONFIGS}
        with torch.no_grad():
            for m in models.values():
                m(x)
            for _ in range(repeats):
                for cfg, m in models.items():
                    rates[cfg].append(batch / timed(lambda: m(x), steps))
            print('%s 224^2, batch %d, 8 bit, %d repeats of %d steps, the four configurations alternating (median [min .. max])'
                  % (name, batch, repeats, steps), flush=True)
            for cfg in CONFIGS:
                r = spread(rates[cfg])
                agg = {}
                for kind, _, ms in models[cfg]._plan.profile(x):
                    n_, t_ = agg.get(kind, (0, 0.0))
                    agg[kind] = (n_ + 1, t_ + ms)
                norms = '  '.join('%s %d launches %.3f ms' % (k, agg[k][0], agg[k][1]) for k in ('layernorm', 'ln_gemm', 'float_layernorm') if k in agg)
                print('  Config(ptf=%-5s, lis=%-5s): %9.1f img/s [%9.1f .. %9.1f]; one single-stream forward %.3f ms, of it %s'
                      % (cfg[0], cfg[1], r[0], r[1], r[2], sum(t_ for _, t_ in agg.values()), norms), flush=True)
        del models
        torch.cuda.empty_cache()


def launch_times(repeats, launches=50):
    """HIP events around `launches` back-to-back launches of p2v_float_layernorm on ROWS rows"""
    L = E.lib()
    print('p2v_float_layernorm, %d rows (batch 256 x 49 tokens), dense rows, no tap: us per launch (median [min .. max] of %d x %d launches)'
          % (ROWS, repeats, launches), flush=True)
    for C_ in WIDTHS:
        gen = torch.Generator().manual_seed(C_)
        x = torch.clamp(torch.round(torch.randn(ROWS, C_, generator=gen) * 30.0), -128, 127).to(torch.int8).cuda()
        out = torch.empty_like(x)
        gamma, beta = (torch.rand(C_, generator=gen) + 0.5).cuda(), (torch.randn(C_, generator=gen) * 0.1).cuda()
        g = torch.full((C_,), 16.0).cuda()
        ln = E.FloatLn(2.0 ** -4, 1e-5, E.ptr(gamma), E.ptr(beta), E.ptr(g))
        st = E.stream_ptr()

        def run():
            E.check(L.p2v_float_layernorm(E.ptr(x), C_, ROWS, C_, C.byref(ln), E.ptr(out), C_, None, st))
        us = []
        for _ in range(repeats):
            run()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                run()
            b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b) / launches)
        m = spread(us)
        print('  C %4d (%s): %7.1f us [%7.1f .. %7.1f]   %6.1f GB/s read + written'
              % (C_, 'k_float_layernorm_xwide' if C_ > 2048 else 'k_float_layernorm      ', m[0], m[1], m[2], 2 * ROWS * C_ / m[0] * 1e-3), flush=True)


def digest_check(parent):
    """tools/kernel_resources.py --digest of the parent's library and of this one (host side: reads the code objects)"""
    tool = os.path.join(ROOT, 'tools', 'kernel_resources.py')
    lib = os.path.join('diff-vit_amd', 'csrc', 'libp2vit_hip.so')
    out = {}
    for tag, tree in (('parent', os.path.abspath(parent)), ('this', ROOT)):
        txt = subprocess.run([sys.executable, tool, os.path.join(tree, lib), '--digest'], check=True, capture_output=True, text=True).stdout
        out[tag] = [l for l in txt.splitlines() if l.strip()]
    old, new = set(out['parent']), set(out['this'])
    print('kernel_resources.py --digest: parent %d kernels, this %d; parent lines missing from this build (name, resources or code hash changed): %d'
          % (len(old), len(new), len(old - new)), flush=True)
    for l in sorted(old - new):
        print('  CHANGED OR GONE: ' + l, flush=True)
    for l in sorted(new - old):
        print('  added: ' + l, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also bench.py from both trees in turn and the kernel digests')
    ap.add_argument('--bench-steps', type=int, default=30)
    ap.add_argument('--bench-warmup', type=int, default=5)
    ap.add_argument('--bench-repeats', type=int, default=3, help='bench.py runs per tree and model')
    args = ap.parse_args()
    engine_cases(args.batch, args.steps, args.repeats)
    launch_times(args.repeats)
    if args.parent:
        torch.cuda.empty_cache()
        digest_check(args.parent)
        parent_check(args.parent, args.bench_steps, args.bench_warmup, args.bench_repeats)


if __name__ == '__main__':
    main()
