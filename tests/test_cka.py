"""CPU: the CKA model diff (diff_vit_amd.cka) against the REAL reference's CKA tooling (tests/golden/cka_kat.npz, tools/gen_golden_cka.py),
the hook selection of get_activations, and the argument checks of the new C entry points (made before any HIP call)."""
import ctypes
import os
from functools import partial

import numpy as np
import pytest
import torch

from _cka_ref import centre_restatement, small_integers
from conftest import ROOT, load_golden


def _kat_acts(synth, seed, tag, u, fs, n):
    # tools/gen_golden_cka.py::kat_acts (that module imports the reference tree, so it is restated here)
    base = synth.normal(seed, '%s/base/u%d' % (tag, u), (n, max(fs)))
    return [base[:, :F] * (0.25 * l) + synth.normal(seed, '%s/u%d/l%d' % (tag, u, l), (n, F)) for l, F in enumerate(fs)]


def _run_kat(cka, g, n, synth, device='cpu'):
    seed, fs, fs2 = int(g['seed']), [int(v) for v in g['fs']], [int(v) for v in g['fs2']]
    c = cka.MinibatchCKA(len(fs))
    x = cka.MinibatchCKA(len(fs), len(fs2), across_models=True)
    a = cka.MinibatchAdvCKA(len(fs), len(fs2))
    for u in range(int(g['updates'])):
        a1 = [v.to(device) for v in _kat_acts(synth, seed, 'm1', u, fs, n)]
        a2 = [v.to(device) for v in _kat_acts(synth, seed, 'm2', u, fs2, n)]
        adv1 = [v.to(device) for v in _kat_acts(synth, seed, 'adv1', u, fs, n)]
        adv2 = [v.to(device) for v in _kat_acts(synth, seed, 'adv2', u, fs2, n)]
        c.update_state(a1)
        x.update_state_across_models(a1, a2)
        a.update_state(a1, adv1, a2, adv2)
    return c.result(), x.result(), a.result()


def test_cpu_restatement_matches_reference_kat(synth):
    import diff_vit_amd as dva
    g = load_golden('cka_kat')
    for n in [int(v) for v in g['ns']]:
        got = _run_kat(dva.cka, g, n, synth)
        for kind, t in zip(('internal', 'across', 'adv'), got):
            ref = g['%s/n%d' % (kind, n)]
            assert t.device.type == 'cpu' and t.shape == ref.shape
            assert np.abs(t.numpy() - ref).max() <= 1e-6, (kind, n, np.abs(t.numpy() - ref).max())


def _micro_float(dva, synth):
    a = synth.ARCHS['micro']
    g = load_golden('micro_vit')
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    return m.eval(), g


def test_get_activations_layer_selection_matches_reference(synth):
    """names, order and shapes of cka_utility.get_activations on the micro-ViT module graph: float (QConv2d / QLinear / Attention / Mlp
    hooked) and with a bit_config (QConv2d / QLinear only)."""
    import diff_vit_amd as dva
    m, g = _micro_float(dva, synth)
    k = load_golden('cka_kat')
    x = torch.from_numpy(g['x_ev'])
    # with a bit_config the hooks go on every QConv2d / QLinear; the quantized forward that fires all of them runs on the GPU
    # (tests/test_cka_gpu.py): here the selection itself
    hooked = [n for n, mod in m.named_modules() if type(mod) in (dva.QConv2d, dva.QLinear)]
    assert hooked == [str(s) for s in k['micro/names_q8']] == [n for n, mod in m.named_modules() if mod in m.linear_modules()]
    for bits, tag in ((None, 'fp'),):
        acts = dva.cka.get_activations(x, m, bits, 'cpu')
        # layer_info through a layer_indices call of every index (the reference's return form)
        names = []
        for i in range(len(acts)):
            a_i, info = dva.cka.get_activations(x, m, bits, 'cpu', layer_indices=i)
            assert len(a_i) == 1 and torch.equal(a_i[0], acts[i])
            names.append(info[0]['name'])
        assert names == [str(s) for s in k['micro/names_' + tag]], tag
        shapes = [[d for d in row if d] for row in k['micro/shapes_' + tag]]
        assert [list(t.shape) for t in acts] == shapes, tag
    normed = dva.cka.get_activations(x, m, None, 'cpu', normalize_act=True)
    assert all(t.dim() == 2 and torch.allclose(t.norm(dim=1), torch.ones(t.shape[0]), atol=1e-5) for t in normed)


def test_cka_entry_points_refuse_bad_arguments_without_gpu():
    import diff_vit_amd as dva
    E = dva.engine
    L = E.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value            # a non-null pointer that no check dereferences
    lay = (E.CkaLayer * 1)()
    lay[0].x, lay[0].features, lay[0].ldx = p, 100, 100
    assert L.p2v_cka_workspace_bytes(lay, 1, 8) > 0
    assert L.p2v_cka_workspace_bytes(lay, 1, 3) == 0 and L.p2v_cka_workspace_bytes(lay, 1, 257) == 0
    with pytest.raises(AssertionError):
        E.check(L.p2v_cka_grams(lay, 1, 3, p, p, 1 << 30, None))          # n < 4
    with pytest.raises(AssertionError):
        E.check(L.p2v_cka_grams(lay, 1, 257, p, p, 1 << 30, None))        # n > 256
    with pytest.raises(E.P2VError, match='workspace'):
        E.check(L.p2v_cka_grams(lay, 1, 8, p, p, 16, None))               # short workspace
    with pytest.raises(E.P2VError):
        E.check(L.p2v_cka_grams(lay, 1, 8, None, p, 1 << 30, None))       # null grams
    with pytest.raises(E.P2VError):
        E.check(L.p2v_cka_grams(None, 1, 8, p, p, 1 << 30, None))         # null layers
    bad = (E.CkaLayer * 1)()
    bad[0].x, bad[0].features, bad[0].ldx = None, 100, 100
    with pytest.raises(E.P2VError):
        E.check(L.p2v_cka_grams(bad, 1, 8, p, p, 1 << 30, None))          # null x
    bad[0].x, bad[0].ldx = p, 50
    with pytest.raises(E.P2VError):
        E.check(L.p2v_cka_grams(bad, 1, 8, p, p, 1 << 30, None))          # row stride < F
    with pytest.raises(E.P2VError):
        E.check(L.p2v_hsic_accumulate(None, 1, p, 1, 8, p, None, None, 0, None))
    with pytest.raises(AssertionError):
        E.check(L.p2v_hsic_accumulate(p, 1, p, 1, 2, p, None, None, 0, None))
    with pytest.raises(AssertionError):
        E.check(L.p2v_hsic_accumulate(p, 1, p, 1, 300, p, None, None, 0, None))
    with pytest.raises(E.P2VError):
        E.check(L.p2v_hsic_accumulate(p, 1, p, 1, 8, p, None, None, 2, None))    # dtype
    with pytest.raises(E.P2VError):
        E.check(L.p2v_forward_linear_taps(None, None, 1, None, 10, None, None, 0, None, None))


def test_new_prototypes_declared_and_exported():
    import diff_vit_amd as dva
    src = open(os.path.join(ROOT, 'include', 'p2vit.h')).read()
    lib = ctypes.CDLL(dva.engine.LIB_PATH)
    for name in ('p2v_forward_linear_taps', 'p2v_cka_workspace_bytes', 'p2v_cka_grams', 'p2v_hsic_accumulate'):
        assert (name + '(') in src and hasattr(lib, name), name
    assert dva.engine.P2V_ABI_VERSION == 6 == dva.engine.lib().p2v_abi_version()
    for op in ('cka_grams', 'hsic_accumulate'):
        assert hasattr(torch.ops.p2vit, op)
    with pytest.raises(NotImplementedError):
        torch.ops.p2vit.cka_grams([torch.zeros(4, 8)], [])               # no CPU kernel behind the op


@pytest.mark.parametrize('n,F', [(4, 1), (5, 33), (33, 1025), (65, 4097), (256, 8193)])
def test_centre_restatement_against_gram_matrix(n, F):
    """the reference of the exact GPU test is itself checked: against cka.gram_matrix in fp64 (torch's own summation orders) cast to fp32,
    within one fp32 ulp of the entry - the two differ at most in the last fp64 bits of the means, which the cast can turn into one fp32 step"""
    import diff_vit_amd as dva
    x, y = small_integers(n * 31 + F, (n, F)), small_integers(n * 37 + F, (n, F))
    assert float((x.abs() @ y.abs().t()).max()) < 2.0 ** 24 and float((x.abs() @ x.abs().t()).max()) < 2.0 ** 24
    for yy in (None, y):
        got = centre_restatement(x, yy).numpy()
        ref = dva.cka.gram_matrix(x.double(), None if yy is None else yy.double(), torch.float64).reshape(n, n).float().numpy()
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)), (n, F, yy is None)
        if yy is None:
            assert np.array_equal(got, got.T)
