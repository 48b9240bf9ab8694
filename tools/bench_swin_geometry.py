"""GPU: the patch 4 / window 12 / 384^2 Swin geometry next to 224^2 / window 7 in ONE call: sliced int8 forward rate as bench_swin runs
it (warm-up, then timed loops bracketed by synchronisation), the rate per number of stream slices, and the per-kind launch times of
SwinPlan.profile (window attention, GEMMs, LayerNorm; the stand-alone LayerNorm launches of 1024 channels and more one by one) at the slice size.
python tools/bench_swin_geometry.py [BATCH=64] [STEPS=10] [MODELS=swin_base_384,swin_base]"""
import collections, contextlib, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
names = (sys.argv[3] if len(sys.argv) > 3 else 'swin_base_384,swin_base').split(',')
WARMUP, REPEATS, STREAMS = 3, 3, 3


def timed(run):
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    loops = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(STEPS):
            run()
        torch.cuda.synchronize()
        loops.append((time.perf_counter() - t0) / STEPS)
    return sorted(loops)


rates = {}
for name in names:
    with contextlib.redirect_stdout(sys.stderr):
        model = dva.harness.str2model(name)(cfg=dva.Config(True, True, 'minmax'))
    model.load_state_dict(dva.synth.swin_state_dict(model.state_dict(), 1))
    model = model.cuda().eval()
    S = model.arch['img_size']
    tokens = (S // model.arch['patch_size']) ** 2
    with torch.no_grad():
        t0 = time.perf_counter()
        dva.harness.calibrate_model(model, dva.synth.images(1, 2, S).cuda())
        t_cal = time.perf_counter() - t0
    plan = model.freeze('cuda')
    base = dva.synth.images(5, min(B, 16), S, offset=100).cuda()
    x = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:B].contiguous()
    print('== %s: %dx%d, window %d, %d tokens per image, batch %d, int8, calibration %.1f s (host)' % (
        name, S, S, model.arch['window_size'], tokens, B, t_cal), flush=True)
    for k in (STREAMS, 1, 2):
        if k > 1 and B < 16 * k:
            continue
        loops = timed(lambda: plan.forward(x, n_streams=k))
        med = loops[len(loops) // 2]
        print('  %d stream slice%s: %8.1f img/s  %8.2f ms per step  (loops of %d steps: %s ms)' % (
            k, ' ' if k == 1 else 's', B / med, 1e3 * med, STEPS, ' / '.join('%.2f' % (1e3 * v) for v in loops)), flush=True)
        if k == STREAMS:
            rates[name] = (B / med, tokens)
    # per-kind launch times of one slice on one stream (HIP events around every launch: the launches do not overlap here)
    n_sl = STREAMS if B >= 16 * STREAMS else 1
    Bl = (B + n_sl - 1) // n_sl
    prof = plan.profile(x[:Bl]); prof = plan.profile(x[:Bl])
    rec = plan._recorded[(Bl, 0, True)]
    kinds, detail, norms = collections.OrderedDict(), collections.OrderedDict(), collections.OrderedDict()
    for i, (kind, e, ms) in enumerate(prof):
        o = rec['ops'][i]
        a = kinds.setdefault(kind, [0, 0.0]); a[0] += 1; a[1] += ms
        if kind == 'window_attention':
            d = detail.setdefault('window_attention T=%d heads=%d ws=%d' % (o.i1, o.i2, o.wa.ws), [0, 0.0]); d[0] += 1; d[1] += ms
        if kind == 'layernorm' and o.N >= 1024:            # the stand-alone LayerNorms of the wide stages and of the merges, by (channels, rows)
            d = norms.setdefault((o.N, o.M), [0, 0.0]); d[0] += 1; d[1] += ms
    tot = sum(v[1] for v in kinds.values())
    print('  per-kind launch times, one slice of %d images on one stream (total %.2f ms):' % (Bl, tot))
    for k, (n, ms) in sorted(kinds.items(), key=lambda kv: -kv[1][1]):
        print('    %-18s x%3d  %8.3f ms  %5.1f %%  %8.2f us per image' % (k, n, ms, 100 * ms / tot, 1e3 * ms / Bl))
    for k, (n, ms) in detail.items():
        print('      %-40s x%3d  %8.3f ms  %7.2f ns per token and launch' % (k, n, ms, 1e6 * ms / n / (Bl * int(k.split('T=')[1].split()[0]))))
    for (C_, rows), (n, ms) in norms.items():
        print('      layernorm C=%-5d rows=%-6d              x%3d  %8.3f ms  %7.2f us per launch  %6.2f ps per row byte' % (
            C_, rows, n, ms, 1e3 * ms / n, 1e9 * ms / n / (rows * C_)))
    del plan, model, x
    torch.cuda.empty_cache()
if len(rates) == 2:
    (r_a, t_a), (r_b, t_b) = rates[names[0]], rates[names[1]]
    print('== %s: %.1f img/s; %s: %.1f img/s; token ratio %.2f -> equal efficiency would be %.1f img/s: the new geometry runs at %.2f of it' % (
        names[0], r_a, names[1], r_b, t_a / t_b, r_b * t_b / t_a, r_a / (r_b * t_b / t_a)))
