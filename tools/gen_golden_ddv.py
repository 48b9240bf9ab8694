"""tests/golden/ddv_micro.npz from the REAL reference's DDV tooling (modeldiff_p2.gen_adv_inputs, compute_ddv,
calculate_and_print_similarities) on the micro-ViT of tests/golden/micro_vit.npz (same weights and calibration batch,
Config(True, True, 'minmax')).  Runs where the reference tree is importable (oracle/gen_golden.py::import_reference); stores inputs and
results only.

    python tools/gen_golden_ddv.py

modeldiff_p2 imports torchvision for its ImageFolder loader, which nothing here calls: empty stand-in modules are enough.

    x, x_adv          eight seeded images in [0, 1] and their perturbed twins (gen_adv_inputs on the float model, torch.manual_seed(SEED))
    keys, keys/<run>  the hook names the float run fills (the order of `printed`), and those of every run
    ddv32/{fp,q8,q4}/<key>  fp32 [8]: compute_ddv of the float model and of the quantized model at [8] * 10 and [4] * 10
    ddv64/{fp,q8,q4}/<key>  the same quantity recomputed here in numpy fp64 from the very same hook outputs
    fp32_dev          max |ddv32 - ddv64| over everything: the reference's own fp32 rounding
    printed/{q8,q4}   [keys] what calculate_and_print_similarities prints for (float, quantized)"""
import contextlib
import io
import os
import re
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import gen_golden as GG  # noqa: E402

synth = GG.synth
OUT = os.path.join(ROOT, 'tests', 'golden', 'ddv_micro.npz')
SEED = 33
N = 8


def ddv64(normal, adv):
    out = []
    for ya, yb in zip(normal, adv):
        ya = ya.detach().numpy().astype(np.float64).ravel()
        yb = yb.detach().numpy().astype(np.float64).ravel()
        out.append(np.dot(ya, yb) / (np.sqrt(np.dot(ya, ya)) * np.sqrt(np.dot(yb, yb))))
    out = np.array(out)
    norm = np.sqrt(np.dot(out, out))
    return out / norm if norm != 0 else out


def main():
    ref = GG.import_reference()
    for name in ('torchvision', 'torchvision.datasets', 'torchvision.transforms'):
        sys.modules.setdefault(name, types.ModuleType(name))
    import modeldiff_p2 as MD
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'micro_vit.npz'))
    arch = synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    fp = GG.build_ref(arch, sd, ref)
    q = GG.build_ref(arch, sd, ref)
    with torch.no_grad():
        q.model_open_calibrate()
        q.model_open_last_calibrate()
        q(torch.from_numpy(g['x_cal']), plot=False)
        q.model_close_calibrate()
        q.model_quant()
    x = synth.uniform(SEED, 'ddv/x', (N, 3, arch['img_size'], arch['img_size']))
    torch.manual_seed(SEED)
    x_adv = MD.gen_adv_inputs(fp, x, None)
    assert float(x_adv.min()) >= 0 and float(x_adv.max()) <= 1 and float((x_adv - x).abs().max()) <= 0.3 + 1e-6

    def run(model, call):
        outputs = {}
        MD.add_hooks(model, outputs)
        with torch.no_grad():
            d32 = MD.compute_ddv(call, x, x_adv, outputs)
            call(x)
            normal = {k: v.clone() for k, v in outputs.items()}
            call(x_adv)
            adv = {k: v.clone() for k, v in outputs.items()}
        for m in model.modules():
            m._forward_hooks.clear()
        return d32, {k: ddv64(normal[k], adv[k]) for k in normal}

    runs = {'fp': run(fp, fp), 'q8': run(q, lambda t: q(t, [8] * 10)), 'q4': run(q, lambda t: q(t, [4] * 10))}
    # the float pass fires no hook on attn.qkv / mlp.fc1 (the SmoothQuant branch calls F.linear itself there), the quantized passes do
    keys = list(runs['fp'][0].keys())
    out = {'seed': np.int64(SEED), 'x': x.numpy(), 'x_adv': x_adv.numpy(), 'keys': np.array(keys)}
    dev = 0.0
    for tag, (d32, d64) in runs.items():
        out['keys/' + tag] = np.array(list(d32.keys()))
        for k in d32:                       # (qact_pos sees the position embedding, a batch of one: the rows differ in length)
            out['ddv32/%s/%s' % (tag, k)] = np.asarray(d32[k], dtype=np.float32)
            out['ddv64/%s/%s' % (tag, k)] = d64[k]
            dev = max(dev, float(np.max(np.abs(out['ddv32/%s/%s' % (tag, k)].astype(np.float64) - d64[k]))))
    out['fp32_dev'] = np.float64(dev)
    for tag in ('q8', 'q4'):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            MD.calculate_and_print_similarities(runs['fp'][0], runs[tag][0])
        printed = dict(re.findall(r'^(\S+) layer similarity: (\S+)%$', buf.getvalue(), flags=re.M))
        out['printed/' + tag] = np.array([float(printed[k]) for k in keys])
        print(tag, 'printed similarities', out['printed/' + tag])
    print('%d keys, fp32_dev %.3g' % (len(keys), dev))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
