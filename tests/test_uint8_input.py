"""uint8 input (CPU): the lookup tables against the loader's own op sequence, the uint8 transform against the fp32 one, the unfused
forward_uint8 against forward, and the refusals."""
from functools import partial

import numpy as np
import pytest
import torch
from PIL import Image

import diff_vit_amd as dva
from diff_vit_amd import data as D


@pytest.mark.parametrize('family', ['deit', 'vit', 'swin'])
def test_lut_f32_equals_normalize_uint8(family):
    mean, std, _ = D.MODEL_STATS[family]
    lut = D.uint8_lut(mean, std)
    # every byte in every channel, in both layouts and at a size where the vectorised and the tail loops of the CPU kernels both run
    v = torch.arange(256, dtype=torch.uint8)
    img = torch.stack([v.roll(7 * c) for c in range(3)], -1).reshape(1, 16, 16, 3).repeat(3, 1, 1, 1)
    ref = D.normalize_uint8(img, mean, std, 'NHWC')
    for c in range(3):
        assert torch.equal(ref[:, c], lut[c][img[..., c].long()]), c
    ref_nchw = D.normalize_uint8(img.permute(0, 3, 1, 2).contiguous(), mean, std, 'NCHW')
    assert torch.equal(ref_nchw, ref)
    # the op sequence itself: ToTensor's division, then Normalize with fp32 tensors
    x = img.permute(0, 3, 1, 2).float().div(255.0)
    want = (x - torch.tensor(mean, dtype=torch.float32).reshape(3, 1, 1)) / torch.tensor(std, dtype=torch.float32).reshape(3, 1, 1)
    assert torch.equal(ref.view(torch.int32), want.view(torch.int32))
    assert torch.equal(D.expand_uint8(img, lut, 'NHWC'), ref)


def test_reciprocal_multiplication_would_not_be_exact():
    """the reason the kernels gather from a table instead of computing: v * (1/255) is not v / 255"""
    v = torch.arange(256, dtype=torch.float32)
    assert int((v / 255.0 != v * (1.0 / 255.0)).sum()) > 100


@pytest.mark.parametrize('log2_s', [-7, -6, -4, -3, 0])
def test_lut_i8_equals_the_input_quantizer(log2_s):
    mean, std, _ = D.MODEL_STATS['deit']
    lut = D.uint8_lut(mean, std)
    s = torch.tensor([2.0 ** log2_s])
    m = dva.VisionTransformer(img_size=32, patch_size=8, embed_dim=64, depth=1, num_heads=2, num_classes=10, input_quant=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), cfg=dva.Config())
    q = m.qact_input.quantizer
    want = q.quant(lut.reshape(1, 3, 1, 256), scale=s, zero_point=torch.zeros(1)).reshape(3, 256)
    got = D.uint8_lut_i8(lut, 1.0 / float(s))
    assert got.dtype == torch.int8
    assert torch.equal(got.float(), want)
    if log2_s <= -6:
        assert int(got.min()) == -128 or int(got.max()) == 127        # codes saturate at the small scales


def _photo(seed, w, h):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
    img = Image.fromarray(base).resize((w, h), Image.BILINEAR)
    return Image.fromarray(np.clip(np.asarray(img).astype(np.int16) + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8))


@pytest.mark.parametrize('family', ['deit', 'vit'])
def test_uint8_transform_matches_the_fp32_transform(family):
    mean, std, crop = D.MODEL_STATS[family]
    tf = D.build_transform(mean=mean, std=std, crop_pct=crop)
    tf8 = D.build_transform(mean=mean, std=std, crop_pct=crop, to_uint8=True)
    for seed, (w, h) in enumerate([(300, 240), (224, 224), (180, 400)]):
        img = _photo(seed, w, h)
        u8 = tf8(img)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (224, 224, 3)
        assert torch.equal(tf(img), D.normalize_uint8(u8, mean, std, 'NHWC'))


def _float_micro():
    a = dva.synth.ARCHS['micro']
    m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                              num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(a, 3), strict=False)
    return m.eval()


@pytest.mark.parametrize('layout', ['NHWC', 'NCHW'])
def test_unfused_forward_uint8_equals_forward(layout):
    m = _float_micro()
    mean, std, _ = D.MODEL_STATS['deit']
    u8 = dva.synth.images_uint8(4, 3, 32)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (3, 32, 32, 3)
    assert torch.equal(u8[1:], dva.synth.images_uint8(4, 2, 32, offset=1))           # counter based
    x = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        ref, f_ref, _ = m(D.normalize_uint8(x, mean, std, layout), [8] * 10)
        out, f_out, _ = m.forward_uint8(x, [8] * 10, mean, std, layout)
    assert torch.equal(out, ref) and f_out == f_ref
    assert len(set(ref.argmax(1).tolist())) > 1


def test_refusals():
    m = _float_micro()
    mean, std, _ = D.MODEL_STATS['deit']
    u8 = dva.synth.images_uint8(0, 2, 32)
    with pytest.raises(AssertionError, match='uint8'):
        m.forward_uint8(u8.float(), [8] * 10, mean, std)
    with pytest.raises(AssertionError, match='layout'):
        m.forward_uint8(u8, [8] * 10, mean, std, 'HWC')
    with pytest.raises(AssertionError, match='4-D'):
        m.forward_uint8(u8[0], [8] * 10, mean, std)
    with pytest.raises(AssertionError, match='channels'):
        m.forward_uint8(u8, [8] * 10, mean, std, 'NCHW')                        # an NHWC batch named NCHW: 32 "channels"
    with pytest.raises(AssertionError, match='channels'):
        m.forward_uint8(u8[..., :2].contiguous(), [8] * 10, mean, std)
    with pytest.raises(ValueError, match='mean / std'):
        m.forward_uint8(u8, [8] * 10, mean[:2], std)
    with pytest.raises(ValueError, match='mean / std'):
        D.normalize_uint8(u8, mean, std[:1])
    with pytest.raises(ValueError, match='uint8'):
        D.normalize_uint8(u8.float(), mean, std)
    with pytest.raises(ValueError, match='layout'):
        D.normalize_uint8(u8, mean, std, 'nhwc')
    from diff_vit_amd import swin
    sm = swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    with pytest.raises(ValueError, match='mean / std'):
        sm.forward_uint8(dva.synth.images_uint8(0, 1, 56), 8, mean[:2], std[:2])


def test_harness_flag_and_uint8_loader(tmp_path):
    args = dva.harness.build_parser().parse_args(['--uint8-input', '--model', 'vit_base'])
    assert args.uint8_input and dva.harness.uint8_stats(args) == D.MODEL_STATS['vit'][:2]
    assert dva.harness.uint8_stats(dva.harness.build_parser().parse_args([])) is None
    for c in ('a', 'b'):
        (tmp_path / 'val' / c).mkdir(parents=True)
        _photo(ord(c), 260, 250).save(tmp_path / 'val' / c / 'x.png')
    val, _ = D.build_loaders(str(tmp_path), 'deit_small', 2, 2, uint8=True)
    x, y = next(iter(val))
    assert x.dtype == torch.uint8 and tuple(x.shape) == (2, 224, 224, 3) and y.tolist() == [0, 1]
    val32, _ = D.build_loaders(str(tmp_path), 'deit_small', 2, 2)
    mean, std, _ = D.MODEL_STATS['deit']
    assert torch.equal(next(iter(val32))[0], D.normalize_uint8(x, mean, std))
