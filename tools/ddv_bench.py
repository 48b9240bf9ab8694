"""Times a DDV of the quantized model on the GPU (not bench.py): n clean + n perturbed images, [8] * L, median of --reps, one JSON line
per model.

    python tools/ddv_bench.py [--n 50] [--reps 10] [--models deit_small,vit_base]

  (a)  forward_ms                 FrozenPlan.forward of the 2n images (one stream; the last block on the class rows only)
       forward_all_rows_ms        the same with the switch cls_rows = 0: every row of the last block, what every tap entry point computes
  (b)  ddv_int8_ms                FrozenPlan.forward_ddv: the 5 * depth + 3 stages reduced from the live int8 buffers
  (c)  ddv_linear_ms              forward_ddv(with_linear=True): + the 4 * depth + 1 linear outputs through ONE fp32 tap buffer
  (d)  taps_torch_ms              what there was before: forward_linear_taps (all fp32 taps resident) + torch cosine_similarity per tap
       reduction                  bytes the reductions of (b) read (both operands of every stage), the time they add to the all-rows
                                  forward, and the rate; `standalone`: ONE grouped p2v_pair_cosine over buffers of the same shapes,
                                  ~0.9 GB that no launch has just written.  HBM: 8.0 TB/s peak, 6.29 TB/s measured for a float4 copy
                                  (MI355X_MICROARCH.md); the live buffers of (b) mostly sit in the 256 MiB Infinity Cache."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np  # noqa: E402

import diff_vit_amd as dva  # noqa: E402
import p2vit_oracle as O  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def run(model, n, reps):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', model + '.npz'))
    arch = dva.synth.ARCHS[model]
    sd = dva.synth.vit_state_dict(arch, int(g['seed']))
    calib = O.unflatten_calib({k[len('calib/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('calib/')})
    plan = dva.FrozenPlan(arch, sd, calib, device=torch.device('cuda:0'))
    L = 4 * arch['depth'] + 2
    bits = [8] * L
    x = dva.synth.images(1, 2 * n, 224).cuda()
    lib = dva.engine.lib()
    t_fwd = timed(lambda: plan.forward(x, bits), reps)
    cls_rows = int(os.environ.get('P2V_CLS_ROWS', '1') != '0')        # what the process started with (the library reads it once)
    lib.p2v_set_tuning(b'cls_rows', 0)
    t_all = timed(lambda: plan.forward(x, bits), reps)
    lib.p2v_set_tuning(b'cls_rows', cls_rows)
    t_b = timed(lambda: plan.forward_ddv(x, bits, False), reps)
    t_c = timed(lambda: plan.forward_ddv(x, bits, True), reps)

    def taps_torch():
        logits, taps = plan.forward_linear_taps(x, bits, want=set(range(1, L)))
        return [F.cosine_similarity(t[:n].reshape(n, -1), t[n:].reshape(n, -1), dim=1) for t in taps[1:]] + \
               [F.cosine_similarity(logits[:n], logits[n:], dim=1)]
    t_d = timed(taps_torch, reps)
    T, D, Hd = plan.tokens, plan.D, plan.hidden
    per_block = [(T, 3 * D), (T, D), (T, D), (T, Hd), (T, D)]
    shapes = [(T, D)] + per_block * arch['depth'] + [(1, D)]
    nbytes = 2.0 * n * sum(r * c for r, c in shapes) + 2.0 * n * arch['num_classes'] * 4
    a = [torch.randint(-128, 128, (n, r, c), dtype=torch.int8, device='cuda') for r, c in shapes]
    b = [torch.randint(-128, 128, (n, r, c), dtype=torch.int8, device='cuda') for r, c in shapes]
    t_alone = timed(lambda: torch.ops.p2vit.pair_cosine(a, b, [None] * len(a)), reps)
    tap_bytes = sum(int(np.prod(s)) for s in plan.tap_shapes(2 * n)[1:]) * 4
    return {'model': model, 'n': n, 'images': 2 * n, 'stages_int8': 5 * arch['depth'] + 3, 'stages_linear': 9 * arch['depth'] + 4,
            'forward_ms': round(t_fwd, 3), 'forward_all_rows_ms': round(t_all, 3), 'ddv_int8_ms': round(t_b, 3),
            'ddv_linear_ms': round(t_c, 3), 'taps_torch_ms': round(t_d, 3),
            'ddv_int8_over_forward': round(t_b / t_fwd, 3), 'ddv_linear_over_taps_torch': round(t_c / t_d, 3),
            'fp32_activation_MB': {'ddv_linear': round(plan.ddv_tap_bytes(n) / 1e6, 1), 'taps_torch': round(tap_bytes / 1e6, 1)},
            'reduction': {'MB_read': round(nbytes / 1e6, 1), 'added_ms': round(t_b - t_all, 3),
                          'TBps_in_forward': round(nbytes / max(t_b - t_all, 1e-6) / 1e9, 2),
                          'standalone_ms': round(t_alone, 3), 'standalone_TBps': round(2.0 * n * sum(r * c for r, c in shapes) / t_alone / 1e9, 2),
                          'hbm_TBps': {'peak': 8.0, 'measured_copy': 6.29}}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=50)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--models', default='deit_small,vit_base')
    a = p.parse_args()
    for m in a.models.split(','):
        print(json.dumps(run(m, a.n, a.reps)), flush=True)


if __name__ == '__main__':
    main()
