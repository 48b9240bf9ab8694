"""CPU: Config(ptf=False) / Config(lis=False) - the canonical float LayerNorm and table softmax of tests/_float_ops_ref.py against the REAL
reference (tests/golden/micro_vit_float_ops.npz, tools/gen_golden_float_ops.py), the module surface's calibration under the three
configurations, and the two flags through a plan file."""
import numpy as np
import pytest
import torch

import _float_ops_ref as R

TAGS = sorted(R.CONFIGS)


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def world(dva, oracle):
    g = R.fixture()
    arch = dva.synth.ARCHS['micro']
    seed = int(g['seed'])
    return dict(g=g, arch=arch, sd=dva.synth.vit_state_dict(arch, seed), x_cal=dva.synth.images(seed, int(g['n_calib']), arch['img_size']),
                x_ev=dva.synth.images(seed, int(g['n_eval']), arch['img_size'], offset=1000))


@pytest.mark.parametrize('tag', TAGS)
def test_calibration_equals_reference(dva, world, tag):
    """the module surface under Config(ptf, lis) reproduces every calibrated tensor of the reference; with ptf=False every QAct scale is one
    power of two (what lets the integer kernels run these configurations unchanged)"""
    g = world['g']
    m = R.make_model(dva, world['arch'], world['sd'], tag)
    dva.harness.calibrate_model(m, world['x_cal'])
    flat = dva.calib_io.flatten(m.export_calib())
    pre = tag + '/calib/'
    assert len(flat) == sum(1 for k in g.files if k.startswith(pre))
    for k, v in flat.items():
        assert np.array_equal(v.numpy().reshape(g[pre + k].shape), g[pre + k]), (tag, k)
    if not R.CONFIGS[tag][0]:
        for k, v in flat.items():
            if 'qact' in k or k == 'act_out':
                mant, _ = torch.frexp(v.reshape(-1))
                assert v.numel() == 1 and float(mant[0]) == 0.5, (tag, k)


def _stage_inputs(world, oracle, tag):
    g, arch = world['g'], world['arch']
    c = R.fixture_calib(g, tag, oracle)
    taps = {k[len(tag + '/taps/'):]: g[k] for k in g.files if k.startswith(tag + '/taps/')}
    return c, taps, arch['embed_dim'], arch['num_heads'], arch['depth']


@pytest.mark.parametrize('tag', [t for t in TAGS if not R.CONFIGS[t][0]])
def test_float_layernorm_against_reference(world, oracle, tag):
    """the canonical LayerNorm on the reference's INPUT codes of every norm: its output codes differ from the reference's (fp32
    F.layer_norm) by at most 1, in at most 1 code per 1 000 per stage - and in exactly the counts the generator measured"""
    g, W = world['g'], world['sd']
    c, taps, D, H, depth = _stage_inputs(world, oracle, tag)
    cap = int(g['cap_per_1000'])
    prev, s_prev = 'qact1', c['qact1']
    stages = []
    for i in range(depth):
        p = 'blocks.%d.' % i
        for nm, src, s_src, cs, s0 in ((p + 'attn.qact0', prev, s_prev, c[p + 'attn.best_scale'][1], c[p + 'attn.best_act_scale'][1]),
                                       (p + 'mlp.qact0', p + 'qact2', c[p + 'qact2'], c[p + 'mlp.best_scale'][1], c[p + 'mlp.best_act_scale'][1])):
            norm = 'norm1' if nm.endswith('attn.qact0') else 'norm2'
            q0, _ = R.float_layernorm(torch.from_numpy(taps[src].astype(np.int64)), float(s_src.reshape(-1)[0]), W[p + norm + '.weight'],
                                      W[p + norm + '.bias'], 1e-6, 1.0 / (cs * s0).reshape(-1).expand(D))
            stages.append((nm, q0.numpy(), taps[nm]))
        prev, s_prev = p + 'qact4', c[p + 'qact4']
    qf, _ = R.float_layernorm(torch.from_numpy(taps[prev].astype(np.int64))[:, 0], float(s_prev.reshape(-1)[0]), W['norm.weight'], W['norm.bias'],
                              1e-6, (1.0 / c['qact2']).reshape(-1).expand(D))
    stages.append(('qact2', qf.numpy(), taps['qact2']))
    for nm, got, want in stages:
        d = got.reshape(want.shape).astype(np.int64) - want.astype(np.int64)
        nd, mx = int((d != 0).sum()), int(np.abs(d).max())
        print(tag, nm, '%d of %d codes differ, max %d' % (nd, d.size, mx))
        assert mx <= 1 and nd * 1000 <= cap * d.size, (tag, nm, nd, d.size, mx)
        assert [nd, d.size, mx] == [int(v) for v in g['%s/stage_diff/q8/%s' % (tag, nm)]], (tag, nm)


@pytest.mark.parametrize('tag', [t for t in TAGS if not R.CONFIGS[t][1]])
def test_softmax_attention_against_reference(world, oracle, tag):
    """the table softmax on the reference's score and value codes: attn.qact2 within the same cap; the table equals the fixture's"""
    g = world['g']
    c, taps, D, H, depth = _stage_inputs(world, oracle, tag)
    cap = int(g['cap_per_1000'])
    for i in range(depth):
        p = 'blocks.%d.' % i
        tab = R.softmax_table(c[p + 'attn.qact_attn1'])
        assert np.array_equal(tab, g['%s/softmax_table/%d' % (tag, i)].astype(np.int64))
        assert int(tab.max()) < 1 << 21 and int(tab[0]) == (1 << 21) - 1
        q1 = torch.from_numpy(taps[p + 'attn.qact1'].astype(np.int64))
        Bn, N = q1.shape[0], q1.shape[1]
        v = q1.reshape(Bn, N, 3, H, D // H).permute(2, 0, 3, 1, 4)[2]
        sc = torch.from_numpy(taps[p + 'attn.qact_attn1'].astype(np.int64))
        q2 = R.softmax_attention(sc, v, tab, float(c[p + 'attn.qact1'] / c[p + 'attn.qact2'])).transpose(1, 2).reshape(Bn, N, D).numpy()
        want = taps[p + 'attn.qact2']
        d = q2 - want.astype(np.int64)
        nd, mx = int((d != 0).sum()), int(np.abs(d).max())
        print(tag, p + 'attn.qact2', '%d of %d codes differ, max %d' % (nd, d.size, mx))
        assert mx <= 1 and nd * 1000 <= cap * d.size, (tag, i, nd, mx)
        assert [nd, d.size, mx] == [int(x) for x in g['%s/stage_diff/q8/%sattn.qact2' % (tag, p)]]


@pytest.mark.parametrize('tag', TAGS)
def test_whole_model_runs_the_three_configurations(world, oracle, tag):
    """the helper's whole model under every configuration and bit list: as far from the reference's logits as the generator recorded
    (no cap on this figure; DESIGN records it), and its taps carry the score codes the softmax consumed"""
    g, arch = world['g'], world['arch']
    c = R.fixture_calib(g, tag, oracle)
    ptf, lis = R.CONFIGS[tag]
    s_o = float(c['act_out'].reshape(-1)[0])
    for name, bits in R.bit_lists(g, 4 * arch['depth'] + 2).items():
        taps = {}
        out = R.quant_forward(oracle, arch, world['sd'], c, world['x_ev'], bits, ptf, lis, taps=taps)
        d = np.abs(np.rint((out.numpy() - g['%s/logits/%s' % (tag, name)]) / s_o))
        print(tag, name, '%d of %d logit codes differ from the reference, max %d' % (int((d > 0).sum()), d.size, int(d.max())))
        assert [int((d > 0).sum()), d.size, int(d.max())] == [int(v) for v in g['%s/logit_codes_differ/%s' % (tag, name)]]
        assert 'blocks.0.attn.qact_attn1' in taps and 'qact2' in taps


def test_helper_equals_oracle_under_the_integer_configuration(micro, oracle):
    """(True, True) through the helper's whole model is the oracle's quant_forward, bit for bit: the restatement changed nothing else"""
    orc = oracle.OracleViT(micro['arch'], micro['sd'])
    orc.calib = micro['calib']
    for bits in ([8] * 10, [4] * 10):
        assert torch.equal(R.quant_forward(oracle, micro['arch'], micro['sd'], micro['calib'], micro['x_ev'], bits, True, True),
                           orc.quant_forward(micro['x_ev'], bits))


def test_layernorm_edge_rows():
    """a constant row has variance 0 exactly (integer statistics): y = beta; saturating rows stay finite"""
    C = 64
    gamma, beta, g = torch.linspace(0.5, 1.5, C), torch.linspace(-1, 1, C), torch.full((C,), 16.0)
    q = torch.stack([torch.full((C,), 37), torch.full((C,), -128), torch.full((C,), 127), torch.tensor([-128, 127] * (C // 2))])
    codes, y = R.float_layernorm(q, 0.125, gamma, beta, 1e-6, g)
    assert torch.equal(y[0], beta) and torch.equal(y[1], beta) and torch.equal(y[2], beta)
    assert torch.equal(codes[0], torch.clamp(torch.round(beta.double() * 16), -128, 127).long())
    assert bool(torch.isfinite(y[3]).all()) and int(codes[3].abs().max()) <= 128


@pytest.mark.parametrize('tag', TAGS + ['tt'])
def test_plan_file_round_trip_of_the_flags(dva, world, tag, tmp_path):
    """calib_io.save_plan writes Config(ptf, lis) as int_norm / int_softmax; a file without the keys reads as (True, True)"""
    import json
    ptf, lis = R.CONFIGS.get(tag, (True, True))
    m = R.make_model(dva, world['arch'], world['sd'], tag) if tag in R.CONFIGS else None
    if m is None:
        from functools import partial
        a = world['arch']
        m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                                  num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                                  norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
        m.load_state_dict(world['sd'], strict=False)
        m.eval()
    dva.harness.calibrate_model(m, world['x_cal'])
    path = str(tmp_path / 'plan.npz')
    dva.calib_io.save_plan(path, m)
    assert dva.calib_io.plan_flags(path) == (ptf, lis)
    z = dict(np.load(path))
    meta = json.loads(str(z['meta']))
    for k in ('int_norm', 'int_softmax', 'ln_eps'):
        del meta[k]
    z['meta'] = np.array(json.dumps(meta))
    old = str(tmp_path / 'old.npz')
    np.savez_compressed(old, **z)
    assert dva.calib_io.plan_flags(old) == (True, True)


def test_fused_state_and_refusals_without_a_gpu(dva, world):
    """Config(ptf=False): model_quant() leaves the norms in mode 'ln' and the model still counts as fused; compute_ddv(attention=True) on
    a quantized lis=False model is refused before anything runs"""
    m = R.make_model(dva, world['arch'], world['sd'], 'ff')
    dva.harness.calibrate_model(m, world['x_cal'])
    assert all(mod.mode == 'ln' for mod in m.modules() if type(mod) is dva.QIntLayerNorm) and m._fused()
    m.blocks[0].norm1.mode = 'int'
    assert not m._fused()
    m.blocks[0].norm1.mode = 'ln'
    x = world['x_ev'][:2]
    with pytest.raises(NotImplementedError):
        dva.ddv.compute_ddv(m, x, x, [8] * 10, attention=True)
    t = R.make_model(dva, world['arch'], world['sd'], 'tf')
    dva.harness.calibrate_model(t, world['x_cal'])
    assert t._fused()
    with pytest.raises(NotImplementedError):
        dva.ddv.compute_ddv(t, x, x, [8] * 10, attention=True)
