"""GPU: the CKA model diff on the MI355X - every linear-layer tap of p2v_forward_linear_taps against the oracle, forward hooks on the
fused path, the grouped Gram / HSIC kernels against fp64 restatements, and the micro-ViT heat map against the REAL reference's."""
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_calib, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _micro_model(dva, synth, g):
    a = synth.ARCHS['micro']
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('w/')}
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    return m.eval(), sd


def _rebuild_taps(O, arch, W, c, x, bits):
    """every QConv2d / QLinear output rebuilt with oracle.qgemm from the oracle's integer taps, in bit_config order."""
    orc = O.OracleViT(arch, W)
    orc.calib = c
    taps = {}
    orc.quant_forward(x, bits, taps)
    P, D = arch['patch_size'], arch['embed_dim']
    out = []
    s_in = c['qact_input']
    cols = F.unfold(taps['qact_input'].float(), kernel_size=P, stride=P).transpose(1, 2)
    s_w = c['patch_embed.proj']['int%d' % bits[0]]
    wq = O.weight_codes(W['patch_embed.proj.weight'], None, s_w, bits[0])
    out.append(O.qgemm(cols.reshape(-1, cols.shape[-1]), s_in, wq, s_w.reshape(-1), W['patch_embed.proj.bias']))
    BP = O.BIT_POOL
    for i in range(arch['depth']):
        p = 'blocks.%d.' % i
        b = bits[1 + 4 * i: 5 + 4 * i]
        for nm, tin, kind, bit in (('attn.qkv', 'attn.qact0', 'attn', b[0]), ('attn.proj', 'attn.qact2', 'attn.proj', b[1]),
                                   ('mlp.fc1', 'mlp.qact0', 'mlp', b[2]), ('mlp.fc2', 'mlp.qact1', 'mlp.fc2', b[3])):
            if kind in ('attn', 'mlp'):
                bi = BP.index(bit)
                s_x, cs = c[p + kind + '.best_act_scale'][bi], c[p + kind + '.best_scale'][bi]
                s_w = c[p + kind + '.best_weight_scale'][bi]['int%d' % bit]
            else:
                s_x, cs = c[p + tin], None
                s_w = c[p + kind]['int%d' % bit]
            wq = O.weight_codes(W[p + nm + '.weight'], cs, s_w, bit)
            xin = taps[p + tin].float()
            out.append(O.qgemm(xin.reshape(-1, xin.shape[-1]), s_x, wq, s_w.reshape(-1), W[p + nm + '.bias']))
    s_w = c['head']['int%d' % bits[-1]]
    wq = O.weight_codes(W['head.weight'], None, s_w, bits[-1])
    out.append(O.qgemm(taps['qact2'].float(), c['qact2'], wq, s_w.reshape(-1), W['head.bias']))
    return out


def _check_plan_taps(dva, O, plan, arch, W, c, x, bits):
    logits, taps = plan.forward_linear_taps(x.cuda(), bits)
    assert torch.equal(logits, plan.forward(x.cuda(), bits))
    ref = _rebuild_taps(O, arch, W, c, x, bits)
    B, D = x.shape[0], arch['embed_dim']
    g = arch['img_size'] // arch['patch_size']
    assert taps[0].shape == (B, D, g, g)
    for k, (t, r) in enumerate(zip(taps, ref)):
        got = (t.permute(0, 2, 3, 1) if k == 0 else t).reshape(r.shape).cpu()
        assert torch.equal(got, r), (bits, k, float((got - r).abs().max()))
    t2 = {}
    plan.forward(x.cuda(), bits, taps=t2)
    for i in range(arch['depth']):
        assert torch.equal(t2['qkv_output'][i], taps[1 + 4 * i]) and torch.equal(t2['fc1_output'][i], taps[3 + 4 * i])
    return taps


def test_linear_taps_micro_vit_bit_equal_to_oracle(dva, oracle, synth):
    g = load_golden('micro_vit')
    m, sd = _micro_model(dva, synth, g)
    m = m.cuda()
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']).cuda())
    x = torch.from_numpy(g['x_ev'])
    m(x.cuda(), [8] * 10, False)                               # freezes the plan
    c = m.export_calib()
    mixed = [int(b) for b in g['bit_qmix']]
    taps8 = None
    for bits in ([8] * 10, [4] * 10, mixed):
        t = _check_plan_taps(dva, oracle, m._plan, synth.ARCHS['micro'], sd, c, x, bits)
        taps8 = t if bits == [8] * 10 else taps8
    # forward hooks on the fused model: fire once each, in module order, with these tensors; the logits are unchanged
    seen = []
    hooks = [mod.register_forward_hook(lambda mod_, inp, out, name=name: seen.append((name, inp, out)))
             for name, mod in m.named_modules() if type(mod) in (dva.QConv2d, dva.QLinear)]
    out = m(x.cuda(), [8] * 10, False)[0]
    assert torch.equal(out, m._plan.forward(x.cuda(), [8] * 10))
    names = [n for n, mod in m.named_modules() if type(mod) in (dva.QConv2d, dva.QLinear)]
    assert [s[0] for s in seen] == names and all(s[1] == () for s in seen)
    for (_, _, t), r in zip(seen, taps8):
        assert torch.equal(t, r)
    # get_activations on the fused model: the reference's names (tests/golden/cka_kat.npz) and one engine call
    acts, info = dva.get_activations(x, m, [8] * 10, 'cuda', layer_indices=3)
    assert info[0]['name'] == 'blocks.0.mlp.fc1' and torch.equal(acts[0], taps8[3])
    k = load_golden('cka_kat')
    acts = dva.get_activations(x, m, [8] * 10, 'cuda')
    shapes = [[d for d in row if d] for row in k['micro/shapes_q8']]
    assert [list(a.shape) for a in acts] == shapes
    for h in hooks:
        h.remove()
    h = m.head.register_forward_hook(lambda mod_, inp, out: out * 2)
    with pytest.raises(RuntimeError, match='replacement'):
        m(x.cuda(), [8] * 10, False)
    h.remove()


def test_linear_taps_deit_small_packed_int4(dva, oracle, synth):
    g = load_golden('deit_small')
    arch = synth.ARCHS['deit_small']
    sd = synth.vit_state_dict(arch, int(g['seed']))
    c = golden_calib(g, oracle)
    plan = dva.FrozenPlan(arch, sd, c, device=torch.device('cuda:0'))
    x = synth.images(int(g['seed']), 2, 224, offset=1000)
    L = 4 * arch['depth'] + 2
    for bits in ([4] * L, [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]):
        _check_plan_taps(dva, oracle, plan, arch, sd, c, x, bits)


def _gram64(x, y):
    n = x.shape[0]
    x = x.reshape(n, -1).double()
    y = x if y is None else y.reshape(n, -1).double()
    gram = x @ y.t()
    gram.diagonal().fill_(0)
    means = gram.sum(0) / (n - 2)
    means -= means.sum() / (2 * (n - 1))
    gram -= means.unsqueeze(0)
    gram -= means.unsqueeze(1)
    gram.diagonal().fill_(0)
    bound = x.abs() @ y.abs().t()
    return gram, float(bound.max())


def test_cka_grams_against_fp64(dva):
    gen = torch.Generator(device='cuda').manual_seed(5)
    cases = [(4, 1), (5, 63), (50, 4097), (64, 8192), (65, 300), (256, 605184), (50, 605184)]
    for n, Fn in cases:
        xs = [torch.randn(n, Fn, device='cuda', generator=gen), (torch.randn(n, Fn + 3, device='cuda', generator=gen) + 0.5)[:, 1:Fn + 1]]
        ys = [torch.randn(n, Fn, device='cuda', generator=gen) * 0.5 + xs[0], torch.randn(n, Fn, device='cuda', generator=gen)]
        for yy in (None, ys):
            got = torch.ops.p2vit.cka_grams(xs, yy if yy is not None else [])
            again = torch.ops.p2vit.cka_grams(xs, yy if yy is not None else [])
            assert torch.equal(got, again), (n, Fn)
            assert got.shape == (2, n, n)
            for l in range(2):
                ref, bound = _gram64(xs[l], None if yy is None else yy[l])
                err = float((got[l].double() - ref).abs().max())
                assert err <= 4e-6 * bound, (n, Fn, l, yy is None, err, bound)
                if yy is None:
                    assert torch.equal(got[l], got[l].t())
        del xs, ys


def test_device_cka_matches_cpu_restatement(dva, synth):
    from test_cka import _run_kat
    g = load_golden('cka_kat')
    for n in [int(v) for v in g['ns']]:
        dev = _run_kat(dva.cka, g, n, synth, 'cuda')
        cpu = _run_kat(dva.cka, g, n, synth, 'cpu')
        for kind, d, c in zip(('internal', 'across', 'adv'), dev, cpu):
            assert d.is_cuda
            assert float((d.cpu() - c).abs().max()) <= 1e-5, (kind, n)
        assert float((torch.diagonal(dev[0]).cpu() - 1).abs().max()) <= 1e-5
    # fp64 accumulators
    acts = [torch.randn(12, 300, device='cuda'), torch.randn(12, 77, device='cuda')]
    c64 = dva.MinibatchCKA(2, dtype=torch.float64)
    c64.update_state(acts)
    r = c64.result()
    assert r.dtype == torch.float64 and float((torch.diagonal(r) - 1).abs().max()) <= 1e-12


def test_micro_vit_heatmap_matches_reference(dva, synth):
    g = load_golden('micro_vit')
    k = load_golden('cka_kat')
    fp, _ = _micro_model(dva, synth, g)
    q, _ = _micro_model(dva, synth, g)
    fp, q = fp.cuda(), q.cuda()
    dva.harness.calibrate_model(q, torch.from_numpy(g['x_cal']).cuda())
    x = torch.from_numpy(g['x_ev'])
    hm = dva.compute_cka(fp, q, [x], None, [8] * 10)
    ref = k['micro/heatmap_fp_q8']
    assert hm.shape == ref.shape
    assert float(np.abs(hm.cpu().numpy() - ref).max()) <= 1e-4
