"""CPU: Config.BIT_TYPE_S = uint3 - the canonical semantics of tests/_softmax_bits_ref.py against the REAL reference
(tests/golden/softmax_bits.npz, tools/gen_golden_softmax_bits.py), the product's calibration under uint3 against the reference's state,
how the width travels (export_calib, plan files), what ``freeze`` refuses, and the command lines."""
import json
from functools import partial

import numpy as np
import pytest
import torch

import _softmax_bits_ref as R
from conftest import load_golden


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _cfg(dva, bits):
    cfg = dva.Config(True, True, 'minmax')
    cfg.BIT_TYPE_S = dva.BIT_TYPE_DICT['uint%d' % bits]
    return cfg


def _micro_model(dva, synth, cfg, sd=None):
    a = synth.ARCHS['micro']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg)
    missing, unexpected = m.load_state_dict(sd if sd is not None else R.micro_weights(synth, a), strict=False)
    assert not missing and not unexpected
    return m.eval()


def _calibrated(dva, synth, cfg):
    g = R.fixture()
    m = _micro_model(dva, synth, cfg)
    x_cal = synth.images(int(g['micro/seed']), int(g['micro/n_calib']), synth.ARCHS['micro']['img_size'])
    with torch.no_grad():
        m.model_open_calibrate()
        m.model_open_last_calibrate()
        out = m(x_cal, plot=False)[0]
        m.model_close_calibrate()
    m.model_quant()
    return m, out


def test_helper_against_the_reference_operator():
    """QIntSoftmax(uint3) of the reference on the score vectors kat_ops.npz uses for uint4: the helper equals it on every element, as it
    does at 4 bits on the same vectors"""
    g, kat = R.fixture(), load_golden('kat_ops')
    seen = set()
    for e in range(3, 9):
        sf = torch.tensor([2.0 ** -e])
        codes = torch.from_numpy(kat['lis/%d/codes' % e].astype(np.float32))
        k3 = R.lis_int_bits(codes, sf, 3)
        assert np.array_equal(k3.numpy().astype(np.int8), g['lis3/%d/k' % e]), e
        assert np.array_equal(R.probs(R.lis_int_bits(codes, sf, 4)).numpy(), kat['lis/%d/probs' % e]), e
        assert R.exponent_classes(k3) <= set(range(8)) | {16}
        seen |= R.exponent_classes(k3)
    assert seen == set(range(8)) | {16}


def test_helper_window_attention_against_the_reference(synth):
    """the reference's WindowAttention under uint3 at 7 x 7, masked and unmasked: every tap of the helper's restatement"""
    g = R.fixture()
    dim, heads, ws = 64, 2, 7
    W = {
        'qkv.weight': synth.normal(21, 'wa/qkv.w', (3 * dim, dim), 0.09), 'qkv.bias': synth.normal(21, 'wa/qkv.b', (3 * dim,), 0.1),
        'proj.weight': synth.normal(21, 'wa/proj.w', (dim, dim), 0.08), 'proj.bias': synth.normal(21, 'wa/proj.b', (dim,), 0.05),
        'relative_position_bias_table': synth.normal(21, 'wa/table', ((2 * ws - 1) ** 2, heads), 0.6),
    }
    c = {k[len('win/scale/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('win/scale/')}
    region = torch.from_numpy(g['win/region'].astype(np.int64))
    mask = (region.unsqueeze(1) != region.unsqueeze(2)).float() * -100.0
    x = torch.from_numpy(g['win/x_ev']).float()
    for tag, msk in (('nomask', None), ('mask', mask)):
        taps, taps4 = {}, {}
        R.window_attention(x, float(g['win/s_in']), W, c, heads, ws, 3, mask=msk, taps=taps)
        R.window_attention(x, float(g['win/s_in']), W, c, heads, ws, 4, mask=msk, taps=taps4)
        for name in ('qact1', 'qact_attn1', 'qact_table', 'qact2', 'softmax_k', 'qact3', 'qact4'):
            got = taps[name].numpy().astype(np.int64)
            assert np.array_equal(got, g['win/taps/%s/%s' % (tag, name)].astype(np.int64).reshape(got.shape)), (tag, name)
        assert not torch.equal(taps['qact3'], taps4['qact3'])          # the fixture tells the widths apart


def test_helper_whole_model_against_the_reference(synth, oracle):
    """the micro ViT calibrated and run by the reference under uint3: the helper's calibration pass gives the reference's state, its
    forward the reference's logits for the three bit lists and every tap of the all-8-bit one; the uint4 oracle gives other logits"""
    g = R.fixture()
    arch = synth.ARCHS['micro']
    sd = R.micro_weights(synth, arch, int(g['micro/seed']), float(g['micro/qkv_gain']))
    x_cal = synth.images(int(g['micro/seed']), int(g['micro/n_calib']), arch['img_size'])
    x_ev = synth.images(int(g['micro/seed']), int(g['micro/n_eval']), arch['img_size'], offset=1000)
    orc, _ = R.vit_calibrate(arch, sd, x_cal, 3)
    flat = oracle.flatten_calib(orc.calib)
    keys = [k for k in g.files if k.startswith('micro/calib/')]
    assert len(flat) == len(keys)
    for k, v in flat.items():
        assert np.array_equal(v.numpy().reshape(g['micro/calib/' + k].shape), g['micro/calib/' + k]), k
    lists = R.micro_bit_lists(4 * arch['depth'] + 2)
    assert lists['qmix'] == [int(b) for b in g['micro/bit_qmix']]
    for name, bits in lists.items():
        taps = {}
        y = R.vit_forward(arch, sd, orc.calib, x_ev, bits, 3, taps)
        assert np.array_equal(y.numpy(), g['micro/logits/' + name]), name
        if name == 'q8':
            for k in g.files:
                if k.startswith('micro/taps/'):
                    got = taps[k[len('micro/taps/'):]].numpy().astype(np.int64)
                    assert np.array_equal(got.reshape(g[k].shape), g[k].astype(np.int64)), k
    o4 = oracle.OracleViT(arch, sd)
    o4.calib = orc.calib
    with torch.no_grad():
        y4 = o4.quant_forward(x_ev, lists['q8'])
    d = torch.round((y4 - torch.from_numpy(g['micro/logits/q8'])) / float(orc.calib['act_out'].reshape(-1)[0]))
    assert int((d != 0).sum()) > 0 and int(g['micro/codes_differ_from_uint4']) > 0


def test_product_calibration_under_uint3(dva, synth):
    """the module surface honours BIT_TYPE_S during calibration: the reference's state, scale for scale; export_calib adds the width"""
    g = R.fixture()
    m, out = _calibrated(dva, synth, _cfg(dva, 3))
    assert all(b.attn.log_int_softmax.bit_type.name == 'uint3' for b in m.blocks)
    assert np.abs(out.numpy() - g['micro/calib_logits']).max() <= 1e-5
    flat = dva.calib_io.flatten(m.export_calib())
    width_keys = sorted(k for k in flat if k.endswith('.log_int_softmax.bits'))
    assert width_keys == ['blocks.%d.attn.log_int_softmax.bits' % i for i in range(m.depth)]
    assert all(float(flat[k]) == 3.0 for k in width_keys)
    rest = {k: v for k, v in flat.items() if k not in width_keys}
    assert len(rest) == sum(1 for k in g.files if k.startswith('micro/calib/'))
    for k, v in rest.items():
        assert np.array_equal(v.numpy().reshape(g['micro/calib/' + k].shape), g['micro/calib/' + k]), k


def test_width_travels_with_calib_and_plan_files(dva, synth, tmp_path):
    """export_calib names the width only where it is not 4; save_plan writes it; plan_softmax_bits reads it back, per block; a file
    without the key reads as 4"""
    from diff_vit_amd.plan import calib_softmax_bits, softmax_bits_list
    m3, _ = _calibrated(dva, synth, _cfg(dva, 3))
    m4, _ = _calibrated(dva, synth, _cfg(dva, 4))
    assert not any(k.endswith('.bits') for k in m4.export_calib())
    m3.blocks[1].attn.log_int_softmax.bit_type = dva.BIT_TYPE_DICT['uint4']          # a mixed assignment
    paths = ['blocks.%d.attn' % i for i in range(m3.depth)]
    assert calib_softmax_bits(m3.export_calib(), paths) == [3, 4]
    got = {}
    for tag, m in (('m3', m3), ('m4', m4)):
        path = str(tmp_path / (tag + '.npz'))
        dva.calib_io.save_plan(path, m)
        f = np.load(path, allow_pickle=False)
        meta = json.loads(str(f['meta']))
        calib = dva.calib_io.unflatten({k[len('calib/'):]: f[k] for k in f.files if k.startswith('calib/')})
        got[tag] = dva.calib_io.plan_softmax_bits(meta, calib)
    assert got == {'m3': [3, 4], 'm4': [4, 4]}
    # the plans' argument: None, an int, one entry per attention module; anything else is refused
    assert softmax_bits_list(None, 3) == [4, 4, 4] and softmax_bits_list(3, 2) == [3, 3] and softmax_bits_list([3, 4], 2) == [3, 4]
    with pytest.raises(ValueError):
        softmax_bits_list([3, 4, 4], 2)
    for bad in (2, 5, [4, 8]):
        with pytest.raises(NotImplementedError):
            softmax_bits_list(bad, 2)
    # Swin: the same key under the window attention's module path
    from diff_vit_amd import swin
    s = swin.swin_micro_patch4_window7_56(cfg=_cfg(dva, 3), num_classes=10).eval()
    s.load_state_dict(synth.swin_state_dict(s.state_dict(), 5))
    x = synth.images(11, 2, 56)
    with torch.no_grad():
        s.model_open_calibrate(); s.model_open_last_calibrate(); s(x); s.model_close_calibrate()
    sp = ['layers.%d.blocks.%d.attn' % (li, bi) for li, d in enumerate(s.arch['depths']) for bi in range(d)]
    assert calib_softmax_bits(s.export_calib(), sp) == [3] * len(sp)
    path = str(tmp_path / 'swin.npz')
    dva.calib_io.save_plan(path, s)
    f = np.load(path, allow_pickle=False)
    calib = dva.calib_io.unflatten({k[len('calib/'):]: f[k] for k in f.files if k.startswith('calib/')})
    assert dva.calib_io.plan_softmax_bits(json.loads(str(f['meta'])), calib) == [3] * len(sp)


def test_freeze_refusals(dva, synth):
    """a log-int-softmax that is neither uint3 nor uint4 and a QAct that is not int8 are refused at freeze, naming the module; uint3, and
    uint8 under lis=False, pass the check and fail only for want of a GPU"""
    from diff_vit_amd import swin
    m = _micro_model(dva, synth, _cfg(dva, 3))
    m.blocks[1].attn.log_int_softmax.bit_type = dva.BIT_TYPE_DICT['uint8']
    with pytest.raises(NotImplementedError, match=r'blocks\.1\.attn\.log_int_softmax.*uint8'):
        m.freeze('cpu')
    cfg = dva.Config(True, True, 'minmax')
    cfg.BIT_TYPE_A = dva.BIT_TYPE_DICT['uint8']
    with pytest.raises(NotImplementedError, match=r'qact.*uint8.*int8'):
        _micro_model(dva, synth, cfg).freeze('cpu')
    s = swin.swin_micro_patch4_window7_56(cfg=_cfg(dva, 3), num_classes=10).eval()
    s.layers[0].blocks[1].attn.log_int_softmax.bit_type = dva.BIT_TYPE_DICT['int8']
    with pytest.raises(NotImplementedError, match=r'layers\.0\.blocks\.1\.attn\.log_int_softmax.*int8'):
        s.freeze('cpu')
    with pytest.raises(NotImplementedError, match=r'qact.*uint8'):
        swin.swin_micro_patch4_window7_56(cfg=cfg, num_classes=10).eval().freeze('cpu')
    # accepted configurations get as far as the plan
    for cfg_ok in (_cfg(dva, 3), dva.Config(True, False, 'minmax')):
        mm, _ = _calibrated(dva, synth, cfg_ok)
        with pytest.raises(RuntimeError, match='needs a GPU device'):
            mm.freeze('cpu')


def test_command_lines_take_the_flag(dva):
    """--softmax-bits {3,4} on harness, ddv, cka and stats sets cfg.BIT_TYPE_S before a model is built"""
    assert dva.harness.build_parser().parse_args(['--softmax-bits', '3']).softmax_bits == 3
    assert dva.harness.build_parser().parse_args([]).softmax_bits is None
    assert dva.Config().set_softmax_bits(3).BIT_TYPE_S.name == 'uint3' and dva.Config().set_softmax_bits(None).BIT_TYPE_S.name == 'uint4'
    assert dva.Config().set_softmax_bits(4).BIT_TYPE_S.name == 'uint4'
    for tool in (dva.harness, dva.ddv, dva.cka, dva.stats):
        with pytest.raises(SystemExit):                       # argparse: not one of the choices
            tool.main(['--model', 'deit_tiny', '--softmax-bits', '5'])
        # the flag reaches the configuration in front of the model: the float softmax has no width
        with pytest.raises(NotImplementedError, match='--softmax-bits'):
            tool.main(['--model', 'deit_tiny', '--softmax-bits', '3', '--no-lis', '--device', 'cpu'])
