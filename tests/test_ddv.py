"""CPU: the DDV model diff (diff_vit_amd.ddv) against the REAL reference's modeldiff_p2 (tests/golden/ddv_micro.npz, written by
tools/gen_golden_ddv.py): the cosine / normalisation formula on the float micro-ViT, the two similarity metrics, the PGD attack through
its properties, and the CPU twin of torch.ops.p2vit.pair_cosine."""
from functools import partial

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def micro_model(dva, synth, g):
    a = synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    return m.eval()


def shared_keys(dva, k, run, ours):
    """reference hook keys of ``run`` that ``REFERENCE_KEYS`` maps onto a stage of ``ours``"""
    return [r for r in (str(v) for v in k['keys/' + run]) if dva.ddv.REFERENCE_KEYS.get(r) in ours]


def test_float_ddv_matches_reference(dva, synth):
    """fp64 sums over F <= 2^20 features in two orders differ by at most 2 F 2^-53 = 2.3e-10 relative to sqrt(aa bb); the float pass is
    bit-equal to the reference's on one host (test_oracle_golden).  Against the reference's own fp32 output the allowance is its
    measured fp32 rounding, twice: it normalises before the dot product, the restatement after it."""
    k = load_golden('ddv_micro')
    m = micro_model(dva, synth, load_golden('micro_vit'))
    d = dva.compute_ddv(m, torch.from_numpy(k['x']), torch.from_numpy(k['x_adv']))
    assert list(d) == dva.ddv.stage_names(2, True) and all(v.dtype == torch.float64 and v.shape == (8,) for v in d.values())
    keys = shared_keys(dva, k, 'fp', d)
    assert len(keys) == 2 * 4 + 4                          # proj, qact2, fc2, qact4 per block; pos_drop, final_qact2, head, act_out
    dev = float(k['fp32_dev'])
    assert 0 < dev < 1e-6
    for r in keys:
        got = d[dva.ddv.REFERENCE_KEYS[r]].numpy()
        e64 = float(np.abs(got - k['ddv64/fp/' + r]).max())
        e32 = float(np.abs(got - k['ddv32/fp/' + r].astype(np.float64)).max())
        print(r, e64, e32)
        assert e64 <= 1e-9, (r, e64)
        assert e32 <= 2 * dev + 1e-9, (r, e32)
    # qkv / fc1 of a float pass: the tensors Attention / Mlp keep for the analysis scripts (no reference hook fires there)
    assert all(torch.isfinite(v).all() for v in d.values())
    d0 = dva.compute_ddv(m, torch.from_numpy(k['x']), torch.from_numpy(k['x_adv']), with_linear=False)
    assert list(d0) == dva.ddv.stage_names(2, False)
    for nm, v in d0.items():
        assert torch.equal(v, d[nm])


def test_quantized_module_graph_ddv_matches_reference(dva, synth):
    """a calibrated model in the model_quant() state on the CPU has no engine: compute_ddv runs its module graph (QAct hooks fire
    there) and reduces with pair_cosine_cpu; the fake-quantised activations are the reference's, so 1e-9 holds as for the float pass."""
    k = load_golden('ddv_micro')
    g = load_golden('micro_vit')
    m = micro_model(dva, synth, g)
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']))
    assert m._fused()
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10)):
        d = dva.compute_ddv(m, torch.from_numpy(k['x']), torch.from_numpy(k['x_adv']), bits)
        keys = shared_keys(dva, k, tag, d)
        assert len(keys) == 2 * 6 + 4
        for r in keys:
            err = float(np.abs(d[dva.ddv.REFERENCE_KEYS[r]].numpy() - k['ddv64/%s/%s' % (tag, r)]).max())
            assert err <= 1e-9, (tag, r, err)


def test_similarity_metrics(dva):
    k = load_golden('ddv_micro')
    keys = [str(v) for v in k['keys']]
    fp = {r: torch.from_numpy(k['ddv32/fp/' + r]) for r in keys}
    for tag in ('q8', 'q4'):
        q = {r: torch.from_numpy(k['ddv32/%s/%s' % (tag, r)]) for r in keys}
        got = dva.ddv.reference_similarity(fp, q)
        assert list(got) == keys
        assert np.allclose([got[r] for r in keys], k['printed/' + tag], rtol=0, atol=1e-6, equal_nan=True)
        s = dva.ddv.similarity(fp, q)
        assert all(-1 - 1e-12 <= s[r] <= 1 + 1e-12 for r in keys)
    d = {r: torch.from_numpy(k['ddv64/fp/' + r]) for r in keys}
    assert all(abs(v - 1) <= 1e-12 for v in dva.ddv.similarity(d, d).values())
    assert dva.ddv.reference_similarity({'a': torch.tensor([0.5, -0.5, 0.1, 0.2])}, {'a': torch.tensor([0.5, 0.5, 0.3, -0.1])}) == {'a': 0.0}


def test_pgd_properties(dva, synth):
    """bit equality with the reference's twins is not asked for (a sign flip where a gradient is ~0 depends on the summation order);
    the attack's contract is: inside [0, 1] and the epsilon ball, repeatable under a seed, and it ascends its objective."""
    k = load_golden('ddv_micro')
    m = micro_model(dva, synth, load_golden('micro_vit'))
    x = torch.from_numpy(k['x'])
    eps = 0.3
    torch.manual_seed(5)
    adv = dva.gen_adv_inputs(m, x)
    assert adv.shape == x.shape and not adv.requires_grad
    assert float(adv.min()) >= 0 and float(adv.max()) <= 1
    assert float((adv - x).abs().max()) <= eps + 1e-6                        # (x +- eps in fp32)
    torch.manual_seed(5)
    assert torch.equal(adv, dva.gen_adv_inputs(m, x))
    y = dva.ddv.pgd_targets(m, x)
    torch.manual_seed(5)
    start = dva.AttackPGD(m, eps, 0.01, 50).random_start(x)
    with torch.no_grad():
        f0 = float(dva.ddv.pgd_objective(m(start)[0], y))
        f1 = float(dva.ddv.pgd_objective(m(adv)[0], y))
    print('objective at the random start %.6g, after 50 steps %.6g' % (f0, f1))
    assert f1 > f0
    torch.manual_seed(5)
    few = dva.gen_adv_inputs(m, x, epsilon=0.05, step_size=0.01, num_steps=3)
    assert float((few - x).abs().max()) <= 0.05 + 1e-6


def test_pair_cosine_cpu_exact_and_nan(dva):
    gen = torch.Generator().manual_seed(9)
    a = torch.randint(-128, 128, (5, 17, 48), generator=gen, dtype=torch.int8)
    b = torch.randint(-128, 128, (5, 17, 48), generator=gen, dtype=torch.int8)
    a[3] = 0
    an, bn = a.numpy().astype(np.int64).reshape(5, -1), b.numpy().astype(np.int64).reshape(5, -1)
    want = np.stack([(an * bn).sum(1), (an * an).sum(1), (bn * bn).sum(1)], 1)
    for aa, bb in ((a, b), (a.float(), b.float()), (a.double(), b.double())):
        got = dva.ddv.pair_cosine_cpu([aa], [bb])
        assert got.dtype == torch.float64 and got.shape == (1, 5, 3)
        assert np.array_equal(got[0].numpy(), want.astype(np.float64))
    cos = dva.ddv.cosines(got[0])
    assert torch.isnan(cos[3]) and torch.isfinite(cos[[0, 1, 2, 4]]).all()
    assert torch.isnan(dva.ddv.ddv_from_sums(got)).all()                    # NaN / NaN for the whole vector, as numpy gives
    # per-channel scales: powers of two keep every product exact
    sc = torch.tensor([2.0 ** (i % 5 - 2) for i in range(48)])
    got = dva.ddv.pair_cosine_cpu([a], [b], [sc])[0].numpy()
    av, bv = a.double().numpy() * sc.double().numpy(), b.double().numpy() * sc.double().numpy()
    want = np.stack([(av * bv).reshape(5, -1).sum(1), (av * av).reshape(5, -1).sum(1), (bv * bv).reshape(5, -1).sum(1)], 1)
    assert np.array_equal(got, want)
    same = dva.ddv.cosines(dva.ddv.pair_cosine_cpu([b], [b]))
    assert float((same - 1).abs().max()) <= 1e-15


def test_refusals_without_gpu(dva):
    import ctypes
    E = dva.engine
    L = E.lib()
    with pytest.raises(NotImplementedError):
        dva.compute_ddv(torch.nn.Linear(2, 2), torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    d = E.CosLayer(16, 32, None, 64, 16, 4, 16, E.COS_I8)
    assert L.p2v_pair_cosine_workspace_bytes((E.CosLayer * 1)(d), 1, 3) > 0
    for field, bad in (('a', 17), ('b', 40), ('row_stride', 24), ('sample_stride', 72)):
        e = E.CosLayer(16, 32, None, 64, 16, 4, 16, E.COS_I8)
        setattr(e, field, bad)
        assert L.p2v_pair_cosine((E.CosLayer * 1)(e), 1, 3, ctypes.c_void_p(256), ctypes.c_void_p(256), 1 << 20, None) == E.E_ARG, field
    f = E.CosLayer(16, 32, None, 18, 6, 3, 6, E.COS_F32)                    # 24-byte rows of floats
    assert L.p2v_pair_cosine((E.CosLayer * 1)(f), 1, 3, ctypes.c_void_p(256), ctypes.c_void_p(256), 1 << 20, None) == E.E_ARG
    assert b'16 bytes' in L.p2v_last_error()
    assert 'pair_cosine' in dva.ops.OPS
    with pytest.raises(NotImplementedError):                                # the op has no CPU kernel: pair_cosine_cpu is its twin
        torch.ops.p2vit.pair_cosine([torch.zeros(2, 16)], [torch.zeros(2, 16)], [None])
