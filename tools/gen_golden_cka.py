"""tests/golden/cka_kat.npz from the REAL reference's CKA tooling (efficient_CKA.MinibatchCKA, DDV_CKA.MinibatchAdvCKA and the hook selection
of cka_utility.get_activations).  Runs where the reference tree is importable (oracle/gen_golden.py::import_reference); stores results
only.  The tests rebuild the inputs from the counter-based generator of diff-vit_amd/synth.py with the recorded seeds.

    python tools/gen_golden_cka.py

Activations of update u, layer l (n images, F features): ``kat_acts(seed, tag, u, [F...], n)`` below - a part shared by all layers
plus a per-layer part, so that the heat maps are neither all ones nor all zeros."""
import os
import sys
from functools import partial  # noqa: F401

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as GG  # noqa: E402

synth = GG.synth
OUT = os.path.join(ROOT, 'tests', 'golden', 'cka_kat.npz')

SEED = 21
NS = (4, 12, 50)
FS = (1, 63, 4097, 300)         # ragged feature counts of the layers (4097: one feature past a chunk of the device kernel)
FS2 = (63, 1, 200)              # the second model's layers (across models / adversarial)
UPDATES = 3


def kat_acts(seed, tag, u, fs, n):
    base = synth.normal(seed, '%s/base/u%d' % (tag, u), (n, max(fs)))
    return [base[:, :F] * (0.25 * l) + synth.normal(seed, '%s/u%d/l%d' % (tag, u, l), (n, F)) for l, F in enumerate(fs)]


def main():
    GG.import_reference()
    import efficient_CKA
    import DDV_CKA
    import models as ref_models
    from models.vit_fquant import Attention, Mlp
    out = {'seed': np.int64(SEED), 'ns': np.array(NS), 'fs': np.array(FS), 'fs2': np.array(FS2), 'updates': np.int64(UPDATES)}
    for n in NS:
        c = efficient_CKA.MinibatchCKA(len(FS))
        x = efficient_CKA.MinibatchCKA(len(FS), len(FS2), across_models=True)
        a = DDV_CKA.MinibatchAdvCKA(len(FS), len(FS2))
        for u in range(UPDATES):
            a1, a2 = kat_acts(SEED, 'm1', u, FS, n), kat_acts(SEED, 'm2', u, FS2, n)
            adv1, adv2 = kat_acts(SEED, 'adv1', u, FS, n), kat_acts(SEED, 'adv2', u, FS2, n)
            c.update_state(a1)
            x.update_state_across_models(a1, a2)
            a.update_state(a1, adv1, a2, adv2)
        out['internal/n%d' % n] = c.result().detach().numpy()
        out['across/n%d' % n] = x.result().detach().numpy()
        out['adv/n%d' % n] = a.result().detach().numpy()
        print('n=%d: internal diag %s' % (n, np.diag(out['internal/n%d' % n])))

    # hook selection of cka_utility.get_activations (lines 63-71) on the micro-ViT, float (bit_config None) and [8] * 10, and the
    # float vs [8] * 10 heat map on the micro_vit.npz weights, calibration batch and evaluation images
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'micro_vit.npz'))
    arch = synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}

    def selected(model, bit_config, x):
        kinds = [ref_models.QConv2d, ref_models.QLinear] + ([Attention, Mlp] if bit_config is None else [])
        acts, info, hooks = [], [], []

        def mk(index, name):
            def hook(m, inp, o):
                acts.append(m.qkv_output if isinstance(m, Attention) else m.fc1_output if isinstance(m, Mlp) else o)
                info.append((index, name))
            return hook
        for index, (name, layer) in enumerate(model.named_modules()):
            if type(layer) in kinds:
                hooks.append(layer.register_forward_hook(mk(index, name)))
        with torch.no_grad():
            model(x, bit_config=bit_config, plot=False)
        for h in hooks:
            h.remove()
        order = sorted(range(len(info)), key=lambda k: info[k][0])
        return [acts[i].detach() for i in order], [info[i][1] for i in order]

    x_cal, x_ev = torch.from_numpy(g['x_cal']), torch.from_numpy(g['x_ev'])
    fp = GG.build_ref(arch, sd, GG.import_reference())
    a_fp, names_fp = selected(fp, None, x_ev)
    q = GG.build_ref(arch, sd, GG.import_reference())
    with torch.no_grad():
        q.model_open_calibrate()
        q.model_open_last_calibrate()
        q(x_cal, plot=False)
        q.model_close_calibrate()
        q.model_quant()
    a_q, names_q = selected(q, [8] * 10, x_ev)
    out['micro/names_fp'] = np.array(names_fp)
    out['micro/names_q8'] = np.array(names_q)
    out['micro/shapes_fp'] = np.array([list(t.shape) + [0] * (4 - t.dim()) for t in a_fp], dtype=np.int64)
    out['micro/shapes_q8'] = np.array([list(t.shape) + [0] * (4 - t.dim()) for t in a_q], dtype=np.int64)
    cka = efficient_CKA.MinibatchCKA(len(a_fp), len(a_q), across_models=True)
    cka.update_state_across_models(a_fp, a_q)
    out['micro/heatmap_fp_q8'] = cka.result().detach().numpy()
    print('micro: %d float layers, %d quantized layers; heat map diag %s' % (len(a_fp), len(a_q), np.diag(out['micro/heatmap_fp_q8'])[:4]))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
