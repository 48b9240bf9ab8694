"""tests/golden/psaq_kat.npz from the REAL reference's data-generation functions (generate_data.py, utils/kde.py), run on the CPU where
the reference tree is present; stores inputs and results only.

    python tools/gen_golden_psaq.py <reference root>

utils/kde.py needs numpy and torch alone and is loaded by its path.  generate_data.py does ``from utils import *`` (timm, torchvision): a
stand-in ``utils`` module in ``sys.modules`` that exposes that very ``KernelDensityEstimator`` is enough for the functions called here
(``differential_entropy``, ``get_image_prior_losses``, ``clip``, ``lr_cosine_policy``).  The entropy term itself stands inline in the
reference's loop (generate_data.py:102-112): those five lines - head mean, ``torch.cosine_similarity``, the estimator on
``sims.view(batch, -1)``, ``linspace(min, max, 10)`` - are applied here around the reference's estimator and ``differential_entropy``.

    <case>/av                     fp32 input [images * groups, heads, tokens, head_dim]; <case>/groups
    <case>/value32, grad32        the reference's value and its autograd gradient in fp32, as it runs
    <case>/value64, grad64        the same lines on the fp64 input with torch's default dtype set to fp64 (so that the reference's
                                  ``linspace`` and its ``torch.tensor(2 pi h^2)`` are fp64 too)
    tv/x, tv/value                get_image_prior_losses
    clip/x, clip/out              clip (the ImageNet statistics it hard-codes)
    lr/args, lr/values            lr_cosine_policy(base_lr, warmup, epochs) at every step of one epoch

The 197-token cases of the GPU test are seeded in the test, not stored."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'psaq_kat.npz')
CASES = {'ragged': (2, 1, 2, 17, 8), 'tile': (1, 1, 1, 33, 4), 'windows': (2, 3, 2, 10, 8), 'minimum': (1, 1, 1, 3, 128),
         'correlated': (2, 1, 3, 21, 16)}


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference(ref_root):
    kde = load(os.path.join(ref_root, 'utils', 'kde.py'), 'ref_kde')
    stand_in = types.ModuleType('utils')
    stand_in.KernelDensityEstimator = kde.KernelDensityEstimator
    stand_in.__all__ = ['KernelDensityEstimator']
    sys.modules['utils'] = stand_in
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            t = types.ModuleType('tqdm')
            t.tqdm = lambda it, *a, **k: it
            sys.modules['tqdm'] = t
    return load(os.path.join(ref_root, 'generate_data.py'), 'ref_generate_data')


def entropy(G, attention, batch_size):
    """generate_data.py:102-112 around the reference's estimator and differential_entropy (no .cuda())"""
    attention_p = attention.mean(dim=1)[:, 1:, :]
    sims = torch.cosine_similarity(attention_p.unsqueeze(1), attention_p.unsqueeze(2), dim=3)
    kde = G.KernelDensityEstimator(sims.view(batch_size, -1))
    start_p, end_p = sims.min().item(), sims.max().item()
    x_plot = torch.linspace(start_p, end_p, steps=10).repeat(batch_size, 1)
    return G.differential_entropy(kde(x_plot), x_plot)


def value_and_grad(G, av, batch_size):
    leaf = av.clone().requires_grad_(True)
    v = entropy(G, leaf, batch_size)
    g, = torch.autograd.grad(v, leaf)
    return v.detach().numpy(), g.numpy()


def case_input(name, shape):
    B, Gr, H, N, hd = shape
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    av = torch.randn(B * Gr, H, N, hd, generator=gen)
    if name == 'correlated':
        av = torch.randn(B * Gr, H, 1, hd, generator=gen) + 0.6 * av
    return av


def main(ref_root):
    G = import_reference(ref_root)
    out = {}
    for name, shape in CASES.items():
        av = case_input(name, shape)
        out[name + '/av'], out[name + '/groups'] = av.numpy(), np.int64(shape[1])
        out[name + '/value32'], out[name + '/grad32'] = value_and_grad(G, av, shape[0])
        torch.set_default_dtype(torch.float64)
        try:
            out[name + '/value64'], out[name + '/grad64'] = value_and_grad(G, av.double(), shape[0])
        finally:
            torch.set_default_dtype(torch.float32)
        print('%-10s %s value %.9g (fp32 %.9g) |grad| %.3g' % (name, shape, out[name + '/value64'], out[name + '/value32'],
                                                             np.linalg.norm(out[name + '/grad64'])))
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 9, 11, generator=gen)
    out['tv/x'], out['tv/value'] = x.numpy(), G.get_image_prior_losses(x).numpy()
    x = 3.0 * torch.randn(2, 3, 5, 6, generator=gen)
    out['clip/x'] = x.numpy().copy()
    out['clip/out'] = G.clip(x.clone()).numpy()

    class Opt:
        param_groups = [{'lr': None}]
    args = (0.25, 5, 12)
    policy = G.lr_cosine_policy(*args)
    values = []
    for it in range(args[2]):
        policy(Opt, it, it)
        values.append(float(Opt.param_groups[0]['lr']))
    out['lr/args'], out['lr/values'] = np.array(args, dtype=np.float64), np.array(values, dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
