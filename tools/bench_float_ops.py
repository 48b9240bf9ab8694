"""GPU: the four Config(ptf, lis) configurations of DeiT-S on the engine, next to the module graph on the same GPU (before the float
LayerNorm / table softmax operators the only way to run ptf=False, and lis=False did not run at all), with the per-kind launch times of
one single-stream forward: float LayerNorm against the int kernel (unfused: ln_gemm = 0), table-softmax attention against k_lis_attention.
python tools/bench_float_ops.py [batch] [steps]  ->  stdout (profiles/float_ops.txt is one run of it)"""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva
from diff_vit_amd import engine as E

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
arch = dva.synth.ARCHS['deit_small']
sd = dva.synth.vit_state_dict(arch, 5)
x = dva.synth.images(5, batch, 224, offset=100).cuda()
bits = [8] * 50


def timed(run, n, warm=2):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def kinds(plan):
    agg, cnt = {}, {}
    for kind, ms in plan.profile(x, bits):
        agg[kind] = agg.get(kind, 0.0) + ms
        cnt[kind] = cnt.get(kind, 0) + 1
    return agg, cnt


print('DeiT-S, batch %d, all layers 8 bit, %d timed steps per figure' % (batch, steps), flush=True)
per_kind = {}
for ptf, lis in ((True, True), (True, False), (False, True), (False, False)):
    m = dva.deit_small_patch16_224(cfg=dva.Config(ptf, lis, 'minmax'))
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, 224).cuda())
    with torch.no_grad():
        assert m._fused()
        ref = m(x, bits)[0]
        dt = timed(lambda: m(x, bits), steps)
        one = timed(lambda: m._plan.forward(x, bits), steps)
        agg, cnt = kinds(m._plan)
        per_kind[(ptf, lis)] = (agg, cnt)
        m._fused = lambda: False                      # the module graph, layer by layer
        dg = timed(lambda: m(x, bits), 2, warm=1)
        graph = m(x, bits)[0]
        del m._fused
    s_o = m._plan.s_out
    d = torch.round((graph - ref) / s_o).abs()
    print('Config(ptf=%s, lis=%s): engine %9.1f img/s sliced (%7.3f ms), %9.1f img/s one stream (%7.3f ms); module graph %8.1f img/s (%8.2f ms); '
          'engine / graph %.1fx; logit codes engine != graph: %d of %d (max %d)'
          % (ptf, lis, batch / dt, dt * 1e3, batch / one, one * 1e3, batch / dg, dg * 1e3, dg / dt, int((d > 0).sum()), d.numel(), int(d.max())), flush=True)
    if ptf and lis:                                   # the int LayerNorm as launches of its own, for the per-kind comparison
        E.check(E.lib().p2v_set_tuning(b'ln_gemm', 0))
        per_kind['int, unfused'] = kinds(m._plan)
        E.check(E.lib().p2v_set_tuning(b'ln_gemm', 1))
    del m
    torch.cuda.empty_cache()

print('per-kind launch times of one single-stream forward (HIP events between launches; ms total / launches / us per launch):')
for key, (agg, cnt) in per_kind.items():
    tot = sum(v for k, v in agg.items() if k != 'event_gap')
    print('  %-22s total %.3f ms   ' % (key if isinstance(key, str) else 'ptf=%s lis=%s' % key, tot) +
          '  '.join('%s %.3f/%d/%.1f' % (k, v, cnt[k], 1e3 * v / cnt[k]) for k, v in sorted(agg.items(), key=lambda kv: -kv[1]) if k != 'event_gap'), flush=True)
