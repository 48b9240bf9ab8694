"""Time the per-layer Hessian traces on the GPU: DeiT-S, batch 32, float model, one batch.

    python tools/bench_hessian.py [--model deit_small] [--batch 32] [--probes 8] [--rounds 3] [--out profiles/hessian.txt]

Three legs in one process, alternating round by round, early stopping disabled (tol 0) at a fixed number of probes per layer so that the
legs do the same work:
  (a) reference  the reference's loop restated in plain torch: randint_like + boolean-mask write + sum(Hv * v).cpu().item() per layer
                 and probe (hutchinson_traces(probes='layer', rng='torch'))
  (b) layer      the same double backwards with the HIP bookkeeping: one fill launch and one step per probe for all layers
  (c) joint      one double backward per probe for all layers
Per leg: the time per probe of one layer (a, b) / of all layers (c), and the share of it outside autograd - the same double backwards
timed alone, with fixed probe vectors and nothing else.  Then a full mean_hessian over the batch with the real stopping rule for (b) and
(c), the Spearman rank correlation of the two normalised vectors and their largest absolute difference: whether 'joint' may stand in
for 'layer'.  Times are host clocks around work that ends in a device synchronise.  Nothing is asserted; there is no CPU fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.nn as nn


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(np.float64), np.argsort(np.argsort(b)).astype(np.float64)
    return float(np.corrcoef(ra, rb)[0, 1])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--model', default='deit_small')
    p.add_argument('--batch', default=32, type=int)
    p.add_argument('--probes', default=8, type=int)
    p.add_argument('--rounds', default=3, type=int)
    p.add_argument('--max-iter', default=150, type=int)
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hessian.txt'))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('bench_hessian needs the GPU: a CPU time says nothing about it')
    import diff_vit_amd as dva
    H = dva.hessian
    dev = torch.device('cuda')
    model = dva.harness.str2model(args.model)(cfg=dva.Config())
    model.load_state_dict(dva.synth.vit_state_dict(model.arch, 0), strict=False)
    model = model.to(dev).eval()
    x = dva.synth.images(1, args.batch, model.arch['img_size']).to(dev)
    with torch.no_grad():
        y = model(x)[0].argmax(1)
    crit = nn.CrossEntropyLoss()
    names, params = dva.select_params(model)
    L = len(names)

    def sync():
        torch.cuda.synchronize()

    def leg(mode, rng):
        sync()
        t0 = time.perf_counter()
        out = dva.hutchinson_traces(model, crit, x, y, max_iter=args.probes, tol=0.0, probes=mode, rng=rng, seed=0, check_every=args.probes)
        sync()
        return time.perf_counter() - t0, out

    def autograd_only(mode):
        """the double backwards of a leg and nothing else: fixed probe vectors, no draw, no sum, no read"""
        loss = crit(H._forward_logits(model, x), y)
        grads = torch.autograd.grad(loss, params, create_graph=True)
        vs = [torch.ones_like(q) for q in params]
        sync()
        t0 = time.perf_counter()
        for _ in range(args.probes):
            if mode == 'joint':
                torch.autograd.grad(grads, params, grad_outputs=vs, retain_graph=True)
            else:
                for g, q, v in zip(grads, params, vs):
                    torch.autograd.grad(g, q, grad_outputs=v, retain_graph=True)
        sync()
        return time.perf_counter() - t0

    def setup_only():
        sync()
        t0 = time.perf_counter()
        loss = crit(H._forward_logits(model, x), y)
        torch.autograd.grad(loss, params, create_graph=True)
        sync()
        return time.perf_counter() - t0

    legs = (('reference', 'layer', 'torch'), ('layer', 'layer', 'counter'), ('joint', 'joint', 'counter'))
    for _, mode, rng in legs:                                   # warm-up of every shape a timed window uses
        leg(mode, rng)
    autograd_only('layer'), autograd_only('joint'), setup_only()
    times = {k: [] for k, _, _ in legs}
    auto = {'layer': [], 'joint': []}
    setup = []
    for _ in range(args.rounds):
        for k, mode, rng in legs:
            times[k].append(leg(mode, rng)[0])
        auto['layer'].append(autograd_only('layer'))
        auto['joint'].append(autograd_only('joint'))
        setup.append(setup_only())
    lines = ['bench_hessian: %s, batch %d, float, %d selected tensors (%d parameters), %d probes per layer, %d rounds, torch %s, %s'
             % (args.model, args.batch, L, sum(q.numel() for q in params), args.probes, args.rounds, torch.__version__, torch.cuda.get_device_name(0)),
             'forward + first backward with create_graph (every leg pays it once per batch): %.1f ms (median)' % (1e3 * float(np.median(setup)))]
    for k, mode, _ in legs:
        per = 1 if mode == 'joint' else L                       # double backwards per probe index
        t = float(np.median(times[k])) - float(np.median(setup))
        a = float(np.median(auto[mode]))
        lines.append('(%s) %-9s loop %.1f ms [%s]; per double backward %.3f ms; the same double backwards alone %.1f ms; outside autograd %.1f %%'
                     % ('abc'[[q[0] for q in legs].index(k)], k, 1e3 * t, ' '.join('%.1f' % (1e3 * v) for v in times[k]), 1e3 * t / (args.probes * per),
                        1e3 * a, 100.0 * max(0.0, t - a) / t))
    lines.append('per probe of ALL layers: reference %.1f ms, layer %.1f ms, joint %.1f ms'
                 % tuple(1e3 * (float(np.median(times[k])) - float(np.median(setup))) / args.probes for k, _, _ in legs))
    full = {}
    for mode in ('layer', 'joint'):
        sync()
        t0 = time.perf_counter()
        _, traces, info = dva.hutchinson_traces(model, crit, x, y, max_iter=args.max_iter, probes=mode, seed=0)
        sync()
        full[mode] = (time.perf_counter() - t0, H.normalise_traces([traces]), info)
        lines.append('full mean_hessian over one batch, real stopping rule (tol 5e-3, max_iter %d), %-5s: %.2f s, %d double backwards, probes per layer '
                     'min %d / median %d / max %d, %d of %d layers converged'
                     % (args.max_iter, mode, full[mode][0], info['hvps'], min(info['probes']), int(np.median(info['probes'])), max(info['probes']),
                        sum(info['converged']), L))
    ref_rate = (float(np.median(times['reference'])) - float(np.median(setup))) / (args.probes * L)
    lines.append('the reference loop over the same %d double backwards as the full layer run, from its measured rate: %.2f s (an estimate, not a run)'
                 % (full['layer'][2]['hvps'], ref_rate * full['layer'][2]['hvps']))
    a, b = np.asarray(full['layer'][1]), np.asarray(full['joint'][1])
    lines.append('joint against layer, normalised vectors of one batch: Spearman rank correlation %.4f, largest absolute difference %.4f (layer %s)'
                 % (spearman(a, b), float(np.abs(a - b).max()), names[int(np.abs(a - b).argmax())]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
