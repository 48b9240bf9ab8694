"""GPU: what per-layer bit lists and packed int4 weights cost and buy on the Swin plan, in ONE call (profiles/swin_mixed.txt):
  build   wall clock of the plan build after a warm-up build: one SwinPlan + freeze_all() (both widths of every layer, frozen by
          p2v_freeze_weights).  On a tree without freeze_all (the parent commit) the same section times SwinPlan(bits=8) + SwinPlan(bits=4),
          which is what serving both widths took there - run this file from both trees.
  pack    4-bit forward rate with packed codes (pack4=True) against int8-stored codes (pack4=False), two plans alternating.
  switch  one forward after changing the list against repeating the same list, everything frozen.
python tools/bench_swin_mixed.py [MODELS=swin_base:256,swin_large_384:64] [STEPS=10] [SECTIONS=build,pack,switch]"""
import contextlib, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import diff_vit_amd as dva
from diff_vit_amd.swin_plan import SwinPlan

models = (sys.argv[1] if len(sys.argv) > 1 else 'swin_base:256,swin_large_384:64').split(',')
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
sections = (sys.argv[3] if len(sys.argv) > 3 else 'build,pack,switch').split(',')
NEW = hasattr(SwinPlan, 'freeze_all')
WARMUP, ROUNDS = 3, 3


def loop(run, steps=STEPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        run(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def fmt(v):
    return ' / '.join('%.3f' % (1e3 * t) for t in v)


for spec in models:
    name, B = spec.split(':')
    B = int(B)
    with contextlib.redirect_stdout(sys.stderr):
        model = dva.harness.str2model(name)(cfg=dva.Config(True, True, 'minmax'))
    model.load_state_dict(dva.synth.swin_state_dict(model.state_dict(), 1))
    model = model.cuda().eval()
    S = model.arch['img_size']
    with torch.no_grad():
        dva.harness.calibrate_model(model, dva.synth.images(1, 2, S).cuda())
    sd, calib = dict(model.state_dict()), model.export_calib()
    n_w = sum(m.weight.numel() for _, m in model.linear_modules())
    print('== %s: %dx%d, batch %d, %.1f M weights in %d layers, %s tree' % (name, S, S, B, n_w / 1e6, len(model.linear_modules()),
                                                                          'this' if NEW else 'parent'), flush=True)
    mk = lambda **kw: SwinPlan(model.arch, sd, calib, device='cuda', in_chans=3, **kw)

    if 'build' in sections:
        def build():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if NEW:
                p = [mk(bits=8).freeze_all()]
            else:
                p = [mk(bits=8), mk(bits=4)]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, p
        build()                                    # warm-up: GELU tables, allocator, library
        torch.cuda.empty_cache()
        mem0 = torch.cuda.memory_allocated()       # the model itself (and the GELU tables, which the process keeps)
        ts = []
        for _ in range(2):
            t, p = build()
            ts.append(t)
            mem = torch.cuda.memory_allocated() - mem0
            del p
            torch.cuda.empty_cache()
        print('  build  %s: %s s (two builds), %.0f MB of device memory in the plan(s)' % (
            'SwinPlan + freeze_all()' if NEW else 'SwinPlan(bits=8) + SwinPlan(bits=4)', ' / '.join('%.2f' % t for t in ts), mem / 1e6), flush=True)

    if not NEW:
        continue
    base = dva.synth.images(5, min(B, 16), S, offset=100).cuda()
    x = base.repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:B].contiguous()
    L = model.bit_config_length()

    if 'pack' in sections:
        plans = {'packed (pack4=True)': mk(bits=4, pack4=True), 'int8-stored (pack4=False)': mk(bits=4, pack4=False)}
        outs, times = {}, {k: [] for k in plans}
        with torch.no_grad():
            for k, p in plans.items():
                for _ in range(WARMUP):
                    outs[k] = p.forward(x)
            for _ in range(ROUNDS):
                for k, p in plans.items():
                    times[k].append(loop(lambda i: p.forward(x)))
            p8 = plans['packed (pack4=True)']
            for _ in range(WARMUP):
                p8.forward(x, bit_config=[8] * L)
            t8 = [loop(lambda i: p8.forward(x, bit_config=[8] * L)) for _ in range(ROUNDS)]
        a, b = outs.values()
        print('  pack   4-bit forward, %d steps per loop, plans alternating; logits equal: %s' % (STEPS, bool(torch.equal(a, b))))
        for k, v in times.items():
            med = sorted(v)[len(v) // 2]
            print('         %-26s %9.1f img/s  %8.3f ms per step  (loops: %s ms)' % (k, B / med, 1e3 * med, fmt(v)))
        med = sorted(t8)[len(t8) // 2]
        print('         %-26s %9.1f img/s  %8.3f ms per step  (loops: %s ms)' % ('8-bit, same plan', B / med, 1e3 * med, fmt(t8)), flush=True)
        del plans, p8, p, outs, a, b
        torch.cuda.empty_cache()

    if 'switch' in sections:
        plan = mk(bits=8).freeze_all()
        la = [8 if i % 2 == 0 else 4 for i in range(L)]
        lb = [4 if i % 2 == 0 else 8 for i in range(L)]
        lb[0] = 8
        with torch.no_grad():
            for _ in range(WARMUP):
                plan.forward(x, bit_config=la); plan.forward(x, bit_config=lb)
            same, alt = [], []
            for _ in range(ROUNDS):
                same.append(loop(lambda i: plan.forward(x, bit_config=la)))
                alt.append(loop(lambda i: plan.forward(x, bit_config=la if i % 2 == 0 else lb)))
            # the host side alone: moving one recording from one list to the other
            r = plan._recorded[next(k for k in plan._recorded if k[2] is True)]
            ca, cb = plan.bit_config(la), plan.bit_config(lb)
            t0 = time.perf_counter()
            for i in range(100):
                plan._switch(r, cb if i % 2 == 0 else ca)
            t_sw = (time.perf_counter() - t0) / 100
        ms, ma = sorted(same)[1], sorted(alt)[1]
        print('  switch %d of %d layers change width per switch; same list %8.3f ms per step (%s), lists alternating %8.3f ms (%s): %+.3f ms per '
              'switch; rewriting one recording on the host %.1f us' % (sum(a_ != b_ for a_, b_ in zip(la, lb)), L, 1e3 * ms, fmt(same), 1e3 * ma, fmt(alt),
                                                                       1e3 * (ma - ms), 1e6 * t_sw), flush=True)
        del plan, r
        torch.cuda.empty_cache()
    del model, x, mk, sd, calib
    torch.cuda.empty_cache()
