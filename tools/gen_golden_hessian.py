"""Generate tests/golden/hessian_micro.npz by RUNNING THE REAL REFERENCE's Hutchinson loop (pyhessian/hessian.py ``hessian.trace``) on
the reference's own micro-ViT, on the CPU, and the normalisation of its driver (test_quant.py, the statements between the trace loop and
the ``***Trace`` print).

Run once where the reference tree is present:   python tools/gen_golden_hessian.py [path of the reference tree]

Nothing of the reference's text is stored: it is imported / compiled when this recipe runs.  Stored are the inputs' seeds and what the
loop did: the selected names, every per-probe value (``group_product`` is wrapped at run time), the probe counts, the traces, the
``mean_hessian`` vector, ``torch.__version__`` and the first 64 signs of the first probe (so that a changed generator stream of torch
is reported as that).

- ``Tensor.cuda`` is a process-local identity, as in oracle/gen_golden.py (the reference's forward hard-codes ``.cuda()``).
- ``pyhessian/hessian.py`` and ``utils.py`` are loaded through a stub package: the package's ``__init__`` pulls in ``ddv_hessian`` and
  with it ``cka_utility``, which this recipe does not need.
- The micro-ViT, its weights and the images come from ``diff_vit_amd.synth`` like the other micro fixtures: 2 batches of 8.
- The seed is the first for which every stop decision of the reference's run lies at least 1 % of ``tol`` away from ``tol``; the
  smallest margin is asserted and stored.  (The reference's ``np.mean`` is pairwise, ``stop_scan`` sequential: they may differ in the
  last ulp, which matters only for a decision that sits on ``tol``.)
"""
import ast
import importlib.util
import os
import sys
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TOL, MAX_ITER, BATCH, N_BATCHES, WEIGHT_SEED, IMAGE_SEED = 5e-3, 150, 8, 2, 7, 21


def import_reference():
    torch.Tensor.cuda = lambda self, *a, **k: self      # process-local; see module docstring
    sys.path.insert(0, REF)
    import config as ref_config                           # noqa
    import models as ref_models                           # noqa
    from models import vit_fquant                         # noqa
    pkg = types.ModuleType('pyhessian')
    pkg.__path__ = [os.path.join(REF, 'pyhessian')]
    sys.modules['pyhessian'] = pkg
    mods = {}
    for name in ('utils', 'hessian'):
        spec = importlib.util.spec_from_file_location('pyhessian.' + name, os.path.join(REF, 'pyhessian', name + '.py'))
        m = importlib.util.module_from_spec(spec)
        sys.modules['pyhessian.' + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return ref_config, ref_models, vit_fquant, mods['hessian'], mods['utils']


def build_ref(arch, sd, ref_config, ref_models, vit_fquant):
    cfg = ref_config.Config(True, True, 'minmax')
    m = vit_fquant.VisionTransformer(img_size=arch['img_size'], patch_size=arch['patch_size'], embed_dim=arch['embed_dim'], depth=arch['depth'],
                                     num_heads=arch['num_heads'], num_classes=arch['num_classes'], mlp_ratio=arch['mlp_ratio'], qkv_bias=True,
                                     norm_layer=partial(ref_models.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    return m.eval()


def normalisation_block():
    """code object of the driver's statements from ``new_global_hessian_track = []`` up to the ``***Trace`` print"""
    path = os.path.join(REF, 'test_quant.py')
    with open(path) as f:
        src = f.read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.If) and 'from pyhessian import hessian' in (ast.get_source_segment(src, node) or ''):
            body = node.body
            start = [i for i, s in enumerate(body) if isinstance(s, ast.Assign) and getattr(s.targets[0], 'id', '') == 'new_global_hessian_track']
            if len(start) == 1:
                return compile(ast.fix_missing_locations(ast.Module(body=body[start[0]:], type_ignores=[])), path, 'exec')
    raise AssertionError('the normalisation block was not found')


def margins(values, tol):
    """the reference's decisions over one layer's values with its own np.mean: relative distance of every gap from tol"""
    out, trace = [], 0.0
    for i in range(len(values)):
        gap = abs(np.mean(values[:i + 1]) - trace) / (abs(trace) + 1e-6)
        out.append(abs(gap - tol) / tol)
        if gap < tol:
            break
        trace = np.mean(values[:i + 1])
    return out


def run(seed, model, batches, H, U):
    """hessian.trace() of the reference on every batch under torch.manual_seed(seed): per batch names, traces and the values"""
    per_batch = []
    real = U.group_product
    torch.manual_seed(seed)
    for x, y in batches:
        seen = []

        def spy(xs, ys):
            r = real(xs, ys)
            seen.append(float(r))
            return r
        H.group_product = spy
        try:
            model.zero_grad()
            comp = H.hessian(model, torch.nn.CrossEntropyLoss(), data=(x, y), cuda=False)
            state = torch.get_rng_state()
            first = torch.randint_like(comp.params[0], high=2).reshape(-1)[:64] * 2 - 1
            torch.set_rng_state(state)
            names, traces = comp.trace(maxIter=MAX_ITER, tol=TOL)
        finally:
            H.group_product = real
        assert len(traces) == len(names), 'a layer converged on an exact zero: the reference appended it twice'
        # split the flat record by the stopping rule itself: a layer's run ends where the reference's rule stopped it
        seqs, pos = [], 0
        for t in traces:
            trace, k = 0.0, 0
            while True:
                k += 1
                m = np.mean(seen[pos:pos + k])
                if abs(m - trace) / (abs(trace) + 1e-6) < TOL or k == MAX_ITER:
                    break
                trace = m
            seqs.append(seen[pos:pos + k])
            pos += k
        assert pos == len(seen), (pos, len(seen))
        per_batch.append(dict(names=list(names), traces=[float(t) for t in traces], values=seqs, first=first.numpy().astype(np.float32)))
    return per_batch


def main():
    import diff_vit_amd as dva
    ref_config, ref_models, vit_fquant, H, U = import_reference()
    arch = dva.synth.ARCHS['micro']
    sd = dva.synth.vit_state_dict(arch, WEIGHT_SEED)
    model = build_ref(arch, sd, ref_config, ref_models, vit_fquant)
    batches = []
    for b in range(N_BATCHES):
        x = dva.synth.images(IMAGE_SEED, BATCH, arch['img_size'], offset=b * BATCH)
        y = torch.tensor([(3 * i + 5 * b + 1) % arch['num_classes'] for i in range(BATCH)])
        batches.append((x, y))
    for seed in range(64):
        res = run(seed, model, batches, H, U)
        margin = min(min(margins(s, TOL)) for r in res for s in r['values'])
        print('seed %d: probes %s, smallest margin %.4f of tol' % (seed, [sum(len(s) for s in r['values']) for r in res], margin))
        if margin >= 0.01:
            break
    assert margin >= 0.01, 'no seed keeps every stop decision 1 % of tol away from tol'
    env = dict(trace_list=[r['traces'] for r in res], mean_hessian=[], name=res[0]['names'], print=lambda *a, **k: None)
    exec(normalisation_block(), env)
    out = dict(seed=np.int64(seed), weight_seed=np.int64(WEIGHT_SEED), image_seed=np.int64(IMAGE_SEED), batch=np.int64(BATCH),
               n_batches=np.int64(N_BATCHES), tol=np.float64(TOL), max_iter=np.int64(MAX_ITER), margin=np.float64(margin),
               torch_version=np.asarray(torch.__version__), names=np.asarray(res[0]['names']),
               mean_hessian=np.asarray(env['mean_hessian'], np.float64))
    for b, (r, (x, y)) in enumerate(zip(res, batches)):
        assert r['names'] == res[0]['names']
        out['b%d/labels' % b] = y.numpy()
        out['b%d/traces' % b] = np.asarray(r['traces'], np.float64)
        out['b%d/counts' % b] = np.asarray([len(s) for s in r['values']], np.int64)
        out['b%d/values' % b] = np.asarray([v for s in r['values'] for v in s], np.float64)
        out['b%d/first_signs' % b] = r['first']
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, 'hessian_micro.npz')
    np.savez_compressed(path, **out)
    print('hessian_micro: %d layers, probes per batch %s, margin %.4f, %d bytes' % (len(res[0]['names']), [int(out['b%d/counts' % b].sum()) for b in range(N_BATCHES)],
                                                                                  margin, os.path.getsize(path)))


if __name__ == '__main__':
    main()
