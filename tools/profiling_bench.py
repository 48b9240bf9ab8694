"""Times ModelDiff's black-box profiling-input search on the GPU (not bench.py): DeiT-S with synthetic weights, [8] * 50 against [4] * 50,
--n seeds, --iters iterations; three variants in ONE call, alternating, the median of --reps rounds; one JSON line.

    python tools/profiling_bench.py [--model deit_small] [--n 50] [--iters 200] [--reps 3]

  (a) reference_port   the reference's loop as it stands (dataset_utility.py:209-302) on the engine: per iteration two candidate batches,
                       each evaluated with both models twice on the WHOLE batch (once for the outputs, once inside
                       metrics_output_diversity), logits to the host, numpy distances - 8 full-batch forwards, 8 host copies.
  (b) host_loop_2img   the same decisions from the host, but each candidate's changed rows from ONE 2-image forward per model; the
                       rows go to the host, numpy updates the tables (one synchronisation per iteration).
  (c) device_loop      profiling.gen_profiling_inputs_in_blackbox: candidate builder, a 2-image forward per model, p2v_profile_step;
                       no host read before the end.
  launches             per iteration: the forwards' kernel launches (FrozenPlan.profile) plus the search's own (c: 1 + 2).
  new_launches         the three p2v_profile launches of an iteration alone (candidates + step on fixed candidate logits), ms per
                       iteration and their share of (c); forwards_2img: the two 2-image forwards alone.
All three take the same draws and must end at the same inputs (asserted)."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import diff_vit_amd as dva  # noqa: E402

P = dva.profiling


def cdist_mean(a, b=None):
    a = a.astype(np.float64)
    if b is None:
        d = a[:, None, :] - a[None, :, :]
        return float(np.mean(np.sqrt((d * d).sum(-1))))
    d = a - b.astype(np.float64)
    return float(np.mean(np.sqrt((d * d).sum(-1))))


def reference_port(plan, b1, b2, x0, eps, pos, idx):
    f = lambda x, bits: plan.forward(x, bits).cpu().numpy()
    x, n = x0.clone(), x0.shape[0]
    o01, o02 = f(x, b1), f(x, b2)

    def evaluate(xs):
        o1, o2 = f(xs, b1), f(xs, b2)
        m1, m2 = cdist_mean(f(xs, b1)), cdist_mean(f(xs, b2))          # metrics_output_diversity runs the model again
        return cdist_mean(o1, o01) * cdist_mean(o2, o02) * m1 * m2

    score = evaluate(x)
    e = torch.tensor(eps, dtype=torch.float32, device=x.device)
    for p, i in zip(pos, idx):
        mut = torch.zeros_like(x)
        mut.view(n, -1)[i, p] = e
        right, left = x + mut, x - mut
        sr, sl = evaluate(right), evaluate(left)
        if sr <= score and sl <= score:
            continue
        x, score = (right, sr) if sr > sl else (left, sl)
    return x


def host_loop_2img(plan, b1, b2, x0, eps, pos, idx):
    x, n = x0.clone(), x0.shape[0]
    O = [plan.forward(x, b).cpu().numpy() for b in (b1, b2)]
    O0 = [o.copy() for o in O]

    def value(tabs):
        return cdist_mean(tabs[0], O0[0]) * cdist_mean(tabs[1], O0[1]) * cdist_mean(tabs[0]) * cdist_mean(tabs[1])

    score = value(O)
    e = torch.tensor(eps, dtype=torch.float32, device=x.device)
    stage = torch.empty((2,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    for p, i in zip(pos, idx):
        stage[0] = x[i]
        stage[1] = x[i]
        stage.view(2, -1)[0, p] += e
        stage.view(2, -1)[1, p] -= e
        rows = [plan.forward(stage, b).cpu().numpy() for b in (b1, b2)]
        cands = []
        for c in range(2):
            tabs = [o.copy() for o in O]
            for m in range(2):
                tabs[m][i] = rows[m][c]
            cands.append(tabs)
        sr, sl = value(cands[0]), value(cands[1])
        if sr <= score and sl <= score:
            continue
        c = 0 if sr > sl else 1
        O, score = cands[c], (sr, sl)[c]
        x.view(n, -1)[i, p] = stage.view(2, -1)[c, p]
    return x


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--model', default='deit_small')
    p.add_argument('--n', type=int, default=50)
    p.add_argument('--iters', type=int, default=200)
    p.add_argument('--reps', type=int, default=3)
    a = p.parse_args()
    dev = torch.device('cuda:0')
    with contextlib.redirect_stdout(sys.stderr):
        m = dva.harness.str2model(a.model)(cfg=dva.Config(True, True, 'minmax'))
    m.load_state_dict(dva.synth.vit_state_dict(m.arch, 0), strict=False)
    m = m.to(dev).eval()
    S = m.arch['img_size']
    dva.harness.calibrate_model(m, dva.synth.images(1, 10, S).to(dev))
    L = 4 * m.depth + 2
    b1, b2 = [8] * L, [4] * L
    plan = m._plan or m.freeze(dev)
    x0 = dva.synth.images(2, a.n, S).to(dev)
    eps = float(np.float32(0.2))
    pos, idx = P.draw_mutations(3 * S * S, a.n, a.iters, np.random.RandomState(0))
    variants = {'reference_port': lambda: reference_port(plan, b1, b2, x0, eps, pos, idx),
                'host_loop_2img': lambda: host_loop_2img(plan, b1, b2, x0, eps, pos, idx),
                'device_loop': lambda: P.gen_profiling_inputs_in_blackbox(m, b1, m, b2, x0, epsilon=0.2, max_iterations=a.iters,
                                                                          rng=np.random.RandomState(0))}
    short = P.draw_mutations(3 * S * S, a.n, 2, np.random.RandomState(0))
    reference_port(plan, b1, b2, x0, eps, *short)           # warm-up: plans, workspaces, allocator
    host_loop_2img(plan, b1, b2, x0, eps, *short)
    P.gen_profiling_inputs_in_blackbox(m, b1, m, b2, x0, max_iterations=2, rng=np.random.RandomState(0))
    times, ends = {k: [] for k in variants}, {}
    for _ in range(a.reps):
        for k, fn in variants.items():                       # alternating
            ms, ends[k] = wall(fn)
            times[k].append(ms / a.iters)
    same = all(torch.equal(ends['device_loop'], v) for v in ends.values())
    assert same, 'the three variants ended at different inputs'

    # the search's own launches alone, and the two 2-image forwards alone
    E = dva.engine
    lib = E.lib()
    n, elems, classes = a.n, 3 * S * S, m.num_classes
    nbytes = lib.p2v_profile_state_bytes(n, classes)
    state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    o = [plan.forward(x0, b) for b in (b1, b2)]
    stage = torch.empty(2, 3, S, S, device=dev)
    cand = [torch.empty(2, classes, device=dev) for _ in range(2)]
    rows = torch.empty(a.iters, 4, dtype=torch.float64, device=dev)
    x = x0.clone()
    st = E.stream_ptr(dev)
    E.check(lib.p2v_profile_init(E.ptr(state), nbytes, n, classes, E.ptr(o[0]), E.ptr(o[1]), st))
    lib.p2v_profile_candidates(E.ptr(x), n, elems, 0, 0, eps, E.ptr(stage), st)
    for c, b in zip(cand, (b1, b2)):
        plan.forward(stage, b, out=c)

    def own():
        for it in range(a.iters):
            E.check(lib.p2v_profile_candidates(E.ptr(x), n, elems, idx[it], pos[it], eps, E.ptr(stage), st))
            E.check(lib.p2v_profile_step(E.ptr(state), nbytes, n, classes, E.ptr(cand[0]), E.ptr(cand[1]), E.ptr(stage), E.ptr(x), elems,
                                         idx[it], pos[it], C.c_void_p(rows.data_ptr() + 32 * it), st))

    def fwd():
        for it in range(a.iters):
            plan.forward(stage, b1, out=cand[0])
            plan.forward(stage, b2, out=cand[1])

    t_own = float(np.median([wall(own)[0] for _ in range(a.reps)])) / a.iters
    t_fwd = float(np.median([wall(fwd)[0] for _ in range(a.reps)])) / a.iters
    k_full = len(plan.profile(x0, b1)) - 1                   # (the last entry is the event gap, no launch)
    k_two = len(plan.profile(stage, b1)) - 1
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({'model': a.model, 'n': a.n, 'iters': a.iters, 'reps': a.reps, 'same_final_inputs': same,
                      'ms_per_iteration': {k: round(v, 4) for k, v in med.items()},
                      'all_rounds_ms_per_iteration': {k: [round(t, 4) for t in v] for k, v in times.items()},
                      'launches_per_iteration': {'reference_port': 8 * k_full, 'host_loop_2img': 2 * k_two + 6, 'device_loop': 2 * k_two + 3},
                      'launches_per_forward': {'full_batch': k_full, 'two_images': k_two},
                      'speedup_device_over_reference_port': round(med['reference_port'] / med['device_loop'], 2),
                      'speedup_device_over_host_2img': round(med['host_loop_2img'] / med['device_loop'], 2),
                      'new_launches': {'ms_per_iteration': round(t_own, 4), 'share_of_device_loop': round(t_own / med['device_loop'], 3)},
                      'forwards_2img': {'ms_per_iteration': round(t_fwd, 4), 'share_of_device_loop': round(t_fwd / med['device_loop'], 3)}}),
          flush=True)


if __name__ == '__main__':
    main()
