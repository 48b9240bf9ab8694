"""Times the pieces of a CKA update on the GPU (not bench.py): the tapped forward (p2v_forward_linear_taps, all 4*depth+2 linear outputs)
against the plain forward, the grouped Gram kernels (torch.ops.p2vit.cka_grams) and the HSIC update (hsic_accumulate) against the
plain-torch restatement (diff_vit_amd.cka.gram_matrix + matmul) on the same GPU in the same process.  One JSON line per model.

    python tools/cka_bench.py [--n 50] [--reps 10] [--models deit_small,vit_base]

Roofline figures: bytes = every tap element read once (n * sum F * 4); mfma_flop = the padded triangle-tile work the kernel issues
(sum over layers of tiles * 32 * 32 * 2 * F).  Peaks: ~6 TB/s achievable HBM, 155 TF fp32 MFMA (MI355X_MICROARCH.md)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np  # noqa: E402

import diff_vit_amd as dva  # noqa: E402
import p2vit_oracle as O  # noqa: E402

GOLD = {'deit_small': 'deit_small', 'vit_base': 'vit_base'}


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
    g = np.load(os.path.join(ROOT, 'tests', 'golden', GOLD[model] + '.npz'))
    arch = dva.synth.ARCHS[model]
    sd = dva.synth.vit_state_dict(arch, int(g['seed']))
    calib = O.unflatten_calib({k[len('calib/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('calib/')})
    plan = dva.FrozenPlan(arch, sd, calib, device=torch.device('cuda:0'))
    L = 4 * arch['depth'] + 2
    bits = [8] * L
    x = dva.synth.images(1, n, 224).cuda()
    t_fwd = timed(lambda: plan.forward(x, bits), reps)
    t_tap = timed(lambda: plan.forward_linear_taps(x, bits), reps)
    _, taps = plan.forward_linear_taps(x, bits)
    feats = [t[0].numel() for t in taps]
    T = (n + 31) // 32
    tiles = T * (T + 1) // 2
    nbytes = 4.0 * n * sum(feats)
    mfma_flop = sum(tiles * 32 * 32 * 2.0 * ((f + 31) // 32 * 32) for f in feats)
    t_gram = timed(lambda: torch.ops.p2vit.cka_grams(taps, []), reps)
    t_gram_torch = timed(lambda: torch.stack([dva.cka.gram_matrix(t) for t in taps]), reps)
    grams = torch.ops.p2vit.cka_grams(taps, [])
    acc = torch.zeros(L, L, device='cuda')
    t_hsic = timed(lambda: torch.ops.p2vit.hsic_accumulate(grams, grams, acc, None, None), reps)
    g2d = grams.reshape(L, -1)
    t_hsic_torch = timed(lambda: acc.add_(g2d @ g2d.t()), reps)
    cka = dva.MinibatchCKA(L)
    t_upd = timed(lambda: cka.update_state(taps), reps)

    def torch_update():
        gg = torch.stack([dva.cka.gram_matrix(t) for t in taps])     # [L, n*n]
        acc.add_(gg @ gg.t())
    t_upd_torch = timed(torch_update, reps)
    return {'model': model, 'n': n, 'layers': L, 'features_per_image': sum(feats),
            'forward_ms': round(t_fwd, 3), 'tapped_forward_ms': round(t_tap, 3),
            'grams_ms': round(t_gram, 3), 'grams_torch_ms': round(t_gram_torch, 3),
            'grams_TBps': round(nbytes / t_gram / 1e9, 2), 'grams_TFLOPs': round(mfma_flop / t_gram / 1e9, 1),
            'grams_roofline_ms': {'hbm_6TBps': round(nbytes / 6e12 * 1e3, 3), 'mfma_155TF': round(mfma_flop / 155e12 * 1e3, 3)},
            'hsic_ms': round(t_hsic, 3), 'hsic_torch_ms': round(t_hsic_torch, 3),
            'update_ms': round(t_upd, 3), 'update_torch_ms': round(t_upd_torch, 3), 'update_speedup': round(t_upd_torch / t_upd, 2)}


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
