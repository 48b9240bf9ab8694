"""GPU: what CKA over the stage list costs.  One process, one stream, alternating repeats, median [min .. max] of three.  DeiT-S, all
layers 8 bit, n = 50 images:
  (a) the plain forward
  (b) the CKA update of the quantized side as it was: forward_linear_taps (fp32 taps of the 4 * depth + 2 linear outputs) + cka_grams
  (c) forward_grams, engine stages (5 * depth + 3)      (d) FULL stages (9 * depth + 7)      (e) engine stages + the linear outputs
  and cka_centre on the Grams of (c);
  the Gram launches of (c) alone: ONE p2v_code_grams call over the 62 int8 stage shapes (per-channel stages with their shift bytes): ms, bytes
  of codes per second, useful int8 OP/s (2 n^2 F per stage) and what the MFMAs execute (2 * tiles * 32 * 32 * F, twice for a shifted stage),
  and their share of (c).
Expected before the first run: a stage offers tiles x chunks = 3 x (10 ... 37) workgroups of 4 waves to 256 CUs, reads 3.8 ... 15 MB
once and contracts them with ~1 % of the int8 MFMA rate: neither the copy rate nor the MFMA roof is in reach, the two launches per stage
and the latency of a workgroup's 16 dependent load rounds are; so ~10 us a stage, ~0.6 ms on top of the forward for (c).
With --parent DIR (a built tree of the parent commit): bench.py and bench.py --model swin_base from both trees in turn, three runs.
python tools/bench_stage_grams.py [--parent DIR]  ->  stdout (profiles/stage_grams.txt is one run of it)"""
import argparse, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tools'))
import diff_vit_amd as dva
from diff_vit_amd import engine as E
from bench_stage_stats import HBM, alternate, event_ms, parent_check, show, spread

PEAK_INT8 = 5.0e15     # dense int8 MFMA OP/s of the device (bench.py: PEAK_INT8_TOPS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--parent', default=None, help='a built tree of the parent commit: also run bench.py from both trees in turn')
    ap.add_argument('--bench-steps', type=int, default=30)
    ap.add_argument('--bench-warmup', type=int, default=5)
    args = ap.parse_args()
    n = args.n
    with torch.no_grad():
        arch = dva.synth.ARCHS['deit_small']
        m = dva.deit_small_patch16_224(cfg=dva.Config())
        m.load_state_dict(dva.synth.vit_state_dict(arch, 5), strict=False)
        m = m.cuda().eval()
        dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
        m.freeze('cuda')
        plan, bits = m._plan, [8] * 50
        x = dva.synth.images(5, n, 224, offset=100).cuda()
        raw = plan.forward_grams(x, bits)[2]

        def taps_and_grams():
            _, bufs = plan.forward_linear_taps(x, bits)
            return torch.ops.p2vit.cka_grams(list(bufs), [])
        cases = {'(a) forward (one stream)': lambda: plan.forward(x, bits),
                 '(b) forward_linear_taps + cka_grams (50 layers)': taps_and_grams,
                 '(c) forward_grams engine (63 stages)': lambda: plan.forward_grams(x, bits),
                 '(c) + cka_centre': lambda: torch.ops.p2vit.cka_centre(plan.forward_grams(x, bits)[2]),
                 '(d) forward_grams full (115 stages)': lambda: plan.forward_grams(x, bits, stages='full'),
                 '(e) forward_grams engine + linear (112 stages)': lambda: plan.forward_grams(x, bits, with_linear=True),
                 'cka_centre alone (63 Grams)': lambda: torch.ops.p2vit.cka_centre(raw)}
        res = alternate(cases, args.repeats)
        show('DeiT-S, %d images, [8] * 50; median of %d alternating repeats' % (n, args.repeats), res, '(a) forward (one stream)')
        taps = sum(t.numel() for t in plan.forward_linear_taps(x, bits)[1]) * 4
        print('  fp32 taps (b) writes and reads back: %.1f MB; (c) writes %d x %d x %d fp64 = %.2f MB' % (taps / 1e6, raw.shape[0], n, n, raw.numel() * 8 / 1e6))

        # the Gram launches of (c) alone: the stage shapes of the engine list in ONE p2v_code_grams call
        T, D = plan.tokens, plan.D
        shapes = [(T, D, True)]
        for _ in range(plan.depth):
            shapes += [(T, 3 * D, False), (T, D, False), (T, D, True), (T, 4 * D, False), (T, D, True)]
        shapes += [(1, D, False)]                      # qact2 (the class rows); act_out is an fp32 stage of 1000 values, left out here
        lays = (E.GramLayer * len(shapes))()
        keep = []
        shift = torch.randint(0, 4, (D,), dtype=torch.uint8, device='cuda')
        F_total = useful = executed = 0
        tiles = ((n + 31) // 32) * ((n + 31) // 32 + 1) // 2
        for k, (rows, cols, sh) in enumerate(shapes):
            buf = torch.randint(-128, 128, (n, rows, cols), dtype=torch.int8, device='cuda')
            keep.append(buf)
            d = lays[k]
            d.base, d.shift, d.sample_stride, d.row_stride, d.rows, d.cols, d.dtype = buf.data_ptr(), shift.data_ptr() if sh else None, rows * cols, cols, rows, cols, E.GRAM_I8
            F_total += n * rows * cols
            useful += 2 * n * n * rows * cols
            executed += 2 * tiles * 1024 * rows * cols * (2 if sh else 1)
        L = E.lib()
        need = L.p2v_code_grams_workspace_bytes(lays, len(shapes), n)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        out = torch.empty(len(shapes), n, n, dtype=torch.float64, device='cuda')
        run = lambda: E.check(L.p2v_code_grams(lays, len(shapes), n, E.ptr(out), E.ptr(ws), need, E.stream_ptr()))
        run()
        torch.cuda.synchronize()
        ms, lo, hi = spread([event_ms(run, 5) for _ in range(args.repeats)])
        c_ms = res['(c) forward_grams engine (63 stages)'][0]
        print('the Gram launches of (c) alone (%d int8 stages, 2 launches each, one p2v_code_grams call): %.3f ms [%.3f .. %.3f] = %.1f us a stage' % (len(shapes), ms, lo, hi, 1e3 * ms / len(shapes)))
        print('  %.1f MB of codes: %.3f TB/s = %.1f %% of the copy rate; useful %.2f TOP/s, executed by the MFMAs %.2f TOP/s = %.2f %% of the int8 peak'
              % (F_total / 1e6, F_total / (ms * 1e-3) / 1e12, 100 * F_total / (ms * 1e-3) / HBM, useful / (ms * 1e-3) / 1e12, executed / (ms * 1e-3) / 1e12,
                 100 * executed / (ms * 1e-3) / PEAK_INT8))
        print('  share of (c): %.1f %% (%.3f of %.3f ms); (c) - (a) = %.3f ms' % (100 * ms / c_ms, ms, c_ms, c_ms - res['(a) forward (one stream)'][0]))
        # one large stage by itself, where the grid fills the device: n = 512
        big = torch.randint(-128, 128, (512, T, 4 * D), dtype=torch.int8, device='cuda')
        one = (E.GramLayer * 1)()
        one[0].base, one[0].sample_stride, one[0].row_stride, one[0].rows, one[0].cols, one[0].dtype = big.data_ptr(), T * 4 * D, 4 * D, T, 4 * D, E.GRAM_I8
        need1 = L.p2v_code_grams_workspace_bytes(one, 1, 512)
        ws1 = torch.empty(need1, dtype=torch.uint8, device='cuda')
        out1 = torch.empty(1, 512, 512, dtype=torch.float64, device='cuda')
        run1 = lambda: E.check(L.p2v_code_grams(one, 1, 512, E.ptr(out1), E.ptr(ws1), need1, E.stream_ptr()))
        run1()
        torch.cuda.synchronize()
        ms1, lo1, hi1 = spread([event_ms(run1, 3) for _ in range(args.repeats)])
        ex1 = 2 * 136 * 1024 * T * 4 * D
        print('one stage of 512 x [197][1536] codes (136 tiles x 37 chunks = 5032 workgroups, %.0f MB of partials): %.3f ms [%.3f .. %.3f], %.1f TOP/s executed = %.1f %% of the int8 peak, '
              '%.2f TB/s of operand loads (each row is loaded by 16 tiles; L2 serves the repeats)' % (need1 / 1e6, ms1, lo1, hi1, ex1 / (ms1 * 1e-3) / 1e12, 100 * ex1 / (ms1 * 1e-3) / PEAK_INT8,
                                                                                                  136 * 64 * T * 4 * D / (ms1 * 1e-3) / 1e12))
        del m, plan, keep, big
    if args.parent:
        torch.cuda.empty_cache()
        parent_check(args.parent, args.bench_steps, args.bench_warmup, 3)


if __name__ == '__main__':
    main()
