"""GPU: uint8 input - p2v_u8_patchify against p2v_quantize_patchify on the normalised images, and forward_uint8 against forward on the
CPU-normalised batch (fused ViT single and sliced, input_quant=False, Swin, every fallback, the prefetching loader), all bit for bit."""
import ctypes as C
from functools import partial

import pytest
import torch

import diff_vit_amd as dva
from diff_vit_amd import data as D
from diff_vit_amd import engine as E

pytestmark = pytest.mark.gpu

MEAN, STD, _ = D.MODEL_STATS['deit']


def _patchify_pair(u8_nhwc, P, C_, inv_s, k_pad, layout):
    B, S = u8_nhwc.shape[0], u8_nhwc.shape[1]
    mean, std = MEAN[:C_], STD[:C_]
    lut = D.uint8_lut(mean, std)
    x32 = D.normalize_uint8(u8_nhwc, mean, std).cuda()
    img = (u8_nhwc if layout == 'NHWC' else u8_nhwc.permute(0, 3, 1, 2).contiguous()).cuda()
    rows = B * (S // P) ** 2
    ref = torch.full((rows, k_pad), 77, dtype=torch.int8, device='cuda')
    got = torch.full((rows, k_pad), -77, dtype=torch.int8, device='cuda')
    L = E.lib()
    E.check(L.p2v_quantize_patchify(E.ptr(x32), B, C_, S, S, P, inv_s, E.ptr(ref), k_pad, E.stream_ptr()))
    li8 = D.uint8_lut_i8(lut, inv_s).cuda()
    E.check(L.p2v_u8_patchify(E.ptr(img), E.LAYOUTS[layout], E.ptr(li8), B, C_, S, S, P, E.ptr(got), k_pad, E.stream_ptr()))
    torch.cuda.synchronize()
    return ref.cpu(), got.cpu()


@pytest.mark.parametrize('layout', ['NHWC', 'NCHW'])
def test_u8_patchify_equals_fp32_patchify(layout):
    cases = [(4, 56, 3, 3), (4, 32, 1, 1), (8, 32, 3, 5), (8, 40, 3, 3), (16, 224, 3, 3), (16, 384, 3, 1), (16, 224, 1, 3),
             (16, 48, 3, 7), (8, 64, 1, 3), (12, 36, 3, 3)]
    for P, S, C_, B in cases:
        u8 = dva.synth.images_uint8(P * S + C_, B, S, C_)
        for inv_s, k_pad in ((32.0, (C_ * P * P + 63) // 64 * 64), (64.0, C_ * P * P + 4)):   # 64 saturates; k_pad % 16 != 0: dword stores
            ref, got = _patchify_pair(u8, P, C_, inv_s, k_pad, layout)
            assert torch.equal(ref, got), (P, S, C_, B, k_pad, int((ref != got).sum()))
    assert int(ref.min()) == -128 or int(ref.max()) == 127


def test_u8_patchify_refusals():
    L = E.lib()
    u8 = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device='cuda')
    out = torch.zeros(16, 256, dtype=torch.int8, device='cuda')
    lut = torch.zeros(3, 256, dtype=torch.int8, device='cuda')
    assert L.p2v_u8_patchify(E.ptr(u8), 1, None, 1, 3, 32, 32, 8, E.ptr(out), 256, E.stream_ptr()) == E.E_ARG
    assert L.p2v_u8_patchify(E.ptr(u8), 2, E.ptr(lut), 1, 3, 32, 32, 8, E.ptr(out), 256, E.stream_ptr()) == E.E_ARG
    assert L.p2v_u8_patchify(E.ptr(u8), 1, E.ptr(lut), 1, 3, 32, 32, 6, E.ptr(out), 256, E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_u8_patchify(E.ptr(u8), 1, E.ptr(lut), 1, 3, 30, 30, 8, E.ptr(out), 256, E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_u8_patchify(E.ptr(u8), 1, E.ptr(lut), 1, 3, 32, 32, 8, E.ptr(out), 96, E.stream_ptr()) == E.E_ARG
    cfg = (C.c_int8 * 10)(*[8] * 10)
    assert L.p2v_forward_u8(None, E.ptr(u8), 1, None, 1, cfg, 10, None, None, 0, -1, None) == E.E_ARG


def _vit(arch, seed, input_quant=True):
    m = dva.VisionTransformer(img_size=arch['img_size'], patch_size=arch['patch_size'], embed_dim=arch['embed_dim'], depth=arch['depth'],
                              num_heads=arch['num_heads'], num_classes=arch['num_classes'], mlp_ratio=arch['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=input_quant, cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(arch, seed), strict=False)
    return m.cuda().eval()


def _calibrated(arch, seed, input_quant=True, n_cal=8):
    m = _vit(arch, seed, input_quant)
    cal = D.normalize_uint8(dva.synth.images_uint8(seed + 100, n_cal, arch['img_size']), MEAN, STD).cuda()
    dva.harness.calibrate_model(m, cal)
    return m


def _fp32_logits(m, u8, bits, layout='NHWC'):
    with torch.no_grad():
        out = m(D.normalize_uint8(u8, MEAN, STD, layout).cuda(), bits)[0]
    torch.cuda.synchronize()
    return out.cpu()


def _u8_logits(m, u8, bits, layout='NHWC'):
    with torch.no_grad():
        out = m.forward_uint8(u8.cuda(), bits, MEAN, STD, layout)[0]
    torch.cuda.synchronize()
    return out.cpu()


def test_deit_small_forward_uint8_bit_equal():
    arch = dva.synth.ARCHS['deit_small']
    m = _calibrated(arch, 11)
    n = 4 * arch['depth'] + 2
    mixed = [8 if (i * 7) % 3 else 4 for i in range(n)]
    u8_small = dva.synth.images_uint8(21, 4, 224)
    u8_big = dva.synth.images_uint8(22, 32, 224).repeat(8, 1, 1, 1)
    u8_big[:4] = u8_small
    for bits in ([8] * n, [4] * n, mixed):
        for layout in ('NHWC', 'NCHW'):
            x = u8_small if layout == 'NHWC' else u8_small.permute(0, 3, 1, 2).contiguous()
            ref = _fp32_logits(m, x, bits, layout)
            assert torch.equal(_u8_logits(m, x, bits, layout), ref), (bits[:3], layout)
            # the patch matrix after the first launch
            plan = m._plan                                       # (frozen by the first quantized forward)
            x32 = D.normalize_uint8(x, MEAN, STD, layout).cuda()
            lut = plan.__dict__['_u8_luts'][D.uint8_lut(MEAN, STD).numpy().tobytes()]
            rows, k_pad = 4 * plan.patches, (3 * 16 * 16 + 63) // 64 * 64
            plan.forward(x32, bits, stop_after=1)
            torch.cuda.synchronize()
            p_ref = plan.view(4, 'patches', rows, k_pad).clone()
            plan.forward_uint8(x.cuda(), lut, bits, layout, stop_after=1)
            torch.cuda.synchronize()
            assert torch.equal(plan.view(4, 'patches', rows, k_pad), p_ref)
        big = _u8_logits(m, u8_big, bits)                        # 256 images: the sliced streams
        assert torch.equal(big, _fp32_logits(m, u8_big, bits))
        assert torch.equal(big[:4], _u8_logits(m, u8_small, bits)) and torch.equal(big[4], big[36])
    assert len(set(ref.argmax(1).tolist())) > 1


def test_micro_vit_without_input_quant():
    arch = dva.synth.ARCHS['micro']
    m = _calibrated(arch, 5, input_quant=False)
    u8 = dva.synth.images_uint8(6, 5, 32)
    for layout in ('NHWC', 'NCHW'):
        x = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()
        for bits in ([8] * 10, [4] * 10):
            assert torch.equal(_u8_logits(m, x, bits, layout), _fp32_logits(m, x, bits, layout)), (layout, bits[0])
    assert m._plan.inv_s_input == 0.0


def _swin(factory, seed, **kw):
    m = factory(cfg=dva.Config(True, True, 'minmax'), **kw).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), seed))
    S = m.arch['img_size']
    cal = D.normalize_uint8(dva.synth.images_uint8(seed + 1, 2, S), MEAN, STD)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(cal); m.model_close_calibrate()
        m.model_quant()
    return m.cuda()


def test_swin_forward_uint8_bit_equal():
    from diff_vit_amd import swin
    m = _swin(swin.swin_micro_patch4_window7_56, 5, num_classes=10)
    u8 = dva.synth.images_uint8(7, 5, 56)
    for layout in ('NHWC', 'NCHW'):
        x = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()
        for bits in (8, 4):
            with torch.no_grad():
                ref = m(D.normalize_uint8(x, MEAN, STD, layout).cuda(), bits).cpu()
                got = m.forward_uint8(x.cuda(), bits, MEAN, STD, layout).cpu()
            assert torch.equal(got, ref), (layout, bits)
    t = _swin(swin.swin_tiny_patch4_window7_224, 8)
    u8 = dva.synth.images_uint8(9, 16, 224).repeat(3, 1, 1, 1)       # 48 images: three slices on the side streams
    with torch.no_grad():
        ref = t(D.normalize_uint8(u8, MEAN, STD).cuda()).cpu()
        got = t.forward_uint8(u8.cuda(), 8, MEAN, STD).cpu()
    assert torch.equal(got, ref) and torch.equal(got[0], got[16])
    assert len(set(ref.argmax(1).tolist())) > 1


def test_fallbacks_equal_the_fp32_path():
    arch = dva.synth.ARCHS['micro']
    u8 = dva.synth.images_uint8(12, 3, 32)
    # calibration with uint8 input (expanded through the fp32 table) == calibration with the normalised batch
    a, b = _vit(arch, 13), _vit(arch, 13)
    cal = dva.synth.images_uint8(14, 6, 32)
    with torch.no_grad():
        for m, go in ((a, lambda m: m.forward_uint8(cal.cuda(), None, MEAN, STD)),
                      (b, lambda m: m(D.normalize_uint8(cal, MEAN, STD).cuda(), None))):
            m.model_open_calibrate(); m.model_open_last_calibrate()
            go(m)
            m.model_close_calibrate(); m.model_quant()
    bits = [8] * 10
    assert torch.equal(_u8_logits(a, u8, bits), _fp32_logits(b, u8, bits))
    # a forward hook on a QLinear: the hook sees the same output
    seen = []
    h = a.blocks[0].mlp.fc1.register_forward_hook(lambda mod, i, o: seen.append(o.detach().cpu()))
    hb = b.blocks[0].mlp.fc1.register_forward_hook(lambda mod, i, o: seen.append(o.detach().cpu()))
    try:
        assert torch.equal(_u8_logits(a, u8, bits), _fp32_logits(b, u8, bits))
    finally:
        h.remove(); hb.remove()
    assert len(seen) == 2 and torch.equal(seen[0], seen[1])
    # a -1 entry (partly float model; flips the block's norm to float for good, so it comes last)
    fp = [8] * 10
    fp[3] = -1
    assert torch.equal(_u8_logits(a, u8, fp), _fp32_logits(b, u8, fp))


def test_prefetcher_feeds_forward_uint8():
    arch = dva.synth.ARCHS['micro']
    m = _calibrated(arch, 15)
    batches = [(dva.synth.images_uint8(16, 6, 32, offset=6 * i).pin_memory(), torch.arange(6)) for i in range(3)]
    bits = [8] * 10
    outs = []
    with torch.no_grad():
        for data, _ in dva.harness.DevicePrefetcher(batches, 'cuda'):
            assert data.dtype == torch.uint8 and data.is_cuda
            outs.append(m.forward_uint8(data, bits, MEAN, STD)[0].clone())
    torch.cuda.synchronize()
    resident = _u8_logits(m, torch.cat([b for b, _ in batches]), bits)
    assert torch.equal(torch.cat(outs).cpu(), resident)
    assert torch.equal(resident, _fp32_logits(m, torch.cat([b for b, _ in batches]), bits))
