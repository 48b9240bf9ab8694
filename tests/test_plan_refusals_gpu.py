"""GPU: what the plan layer refuses before it hands a pointer to the C ABI - entry point, bad call, exception class, exact message - for
``FrozenPlan`` (micro ViT) and ``SwinPlan`` (micro Swin), and the sliced forwards at the smallest shapes that take every scheduling
branch, byte-equal to the unsliced forward."""
import types

import pytest
import torch

import diff_vit_amd as dva
from diff_vit_amd import data as D
from diff_vit_amd import engine as E

pytestmark = pytest.mark.gpu

MEAN, STD, _ = D.MODEL_STATS['deit']
BITS = [8, 4, 8, 8, 4, 8, 4, 4, 8, 8]


def _common(plan, size, n, seed):
    """a plan with good arguments of ``n`` images and the bad ones the tables below draw from"""
    v = types.SimpleNamespace(plan=plan, dev=plan.device, S=size, n=n)
    v.x = dva.synth.images(seed, n, size).cuda()
    v.u8 = dva.synth.images_uint8(seed + 1, n, size).cuda()
    v.lut = plan.input_lut(D.uint8_lut(MEAN, STD))
    v.x_size = torch.zeros(n, 3, size + 8, size + 8, device='cuda')
    v.x_chan = torch.zeros(n, 1, size, size, device='cuda')
    v.x_cpu = v.x.cpu()
    v.x_cpu_size = torch.zeros(n, 3, size + 8, size + 8)
    v.x_empty = torch.zeros(0, 3, size, size, device='cuda')
    v.u8_size = torch.zeros(n, size + 8, size + 8, 3, dtype=torch.uint8, device='cuda')
    v.u8_chan = torch.zeros(n, size, size, 1, dtype=torch.uint8, device='cuda')
    v.u8_cpu = v.u8.cpu()
    v.u8_empty = torch.zeros(0, size, size, 3, dtype=torch.uint8, device='cuda')
    v.u8_float = v.u8.float()
    v.lut_dtype = v.lut.to(torch.int16)
    v.lut_shape = torch.zeros(4, 256, dtype=torch.int8, device='cuda')
    v.lut_strided = torch.zeros(256, 3, dtype=torch.int8, device='cuda').t()
    v.out = torch.empty(n, 10, device='cuda')
    v.out_bad = torch.empty(n - 1, 10, device='cuda')
    return v


@pytest.fixture(scope='module')
def vit(micro):
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    v = _common(plan, 32, 8, 31)
    v.ref = plan.forward(v.x, BITS).clone()
    v.ref_u8 = plan.forward_uint8(v.u8, v.lut, BITS).clone()
    torch.cuda.synchronize()
    return v


@pytest.fixture(scope='module')
def swin():
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    from diff_vit_amd import swin as swin_models
    m = swin_models.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    cal = dva.synth.images(12, 2, 56)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(cal); m.model_close_calibrate()
        m.model_quant()
        m.cuda()
        m(cal[:1].cuda())                                           # freezes the plan
    v = _common(m._plan, 56, 9, 41)
    v.model = m
    return v


SIZE = "Input image size (%d*%d) doesn't match model (%d*%d)."
ON_GPU = 'the quantized forward runs on the HIP engine only: move the input to the GPU'
LAYOUT = "layout must be 'NHWC' or 'NCHW', got 'NWHC'"
NOT_U8 = 'forward_uint8 takes uint8 images, got torch.float32 (fp32 images go to forward)'
U8_SHAPE = 'uint8 images in layout NHWC must be [B, %d, %d, 3], got %s'

# FrozenPlan entry points that take fp32 images: name -> call(v, images, bit_config)
VIT_F32 = {'forward': lambda v, x, bc: v.plan.forward(x, bc),
           'forward_streams': lambda v, x, bc: v.plan.forward_streams(x, bc, v.out),
           'forward_linear_taps': lambda v, x, bc: v.plan.forward_linear_taps(x, bc),
           'forward_ddv': lambda v, x, bc: v.plan.forward_ddv(x, bc),
           'profile': lambda v, x, bc: v.plan.profile(x, bc),
           'profile_streams': lambda v, x, bc: v.plan.profile_streams(x, bc)}
# ... and uint8 images: name -> call(v, images, lut, bit_config, layout)
VIT_U8 = {'forward_uint8': lambda v, x, lut, bc, lay: v.plan.forward_uint8(x, lut, bc, lay),
          'forward_uint8_streams': lambda v, x, lut, bc, lay: v.plan.forward_uint8_streams(x, lut, bc, v.out, lay)}


def _vit_cases():
    cases = []
    for name, call in VIT_F32.items():
        cases += [
            (name, 'size', lambda v, c=call: c(v, v.x_size, BITS), AssertionError, lambda v: SIZE % (40, 40, 32, 32)),
            (name, 'channels', lambda v, c=call: c(v, v.x_chan, BITS), AssertionError, lambda v: 'expected 3 input channels'),
            (name, 'cpu', lambda v, c=call: c(v, v.x_cpu, BITS), RuntimeError, lambda v: ON_GPU),
            (name, 'empty', lambda v, c=call: c(v, v.x_empty, BITS), AssertionError, lambda v: 'empty batch'),
            (name, 'bit_config_none', lambda v, c=call: c(v, v.x, None), ValueError, lambda v: 'None is not in list'),
        ]
    for name, call in VIT_U8.items():
        lut_msg = lambda v: 'lut must be a contiguous torch.int8 [3, 256] tensor on %s (FrozenPlan.input_lut)' % v.dev
        cases += [
            (name, 'layout', lambda v, c=call: c(v, v.u8, v.lut, BITS, 'NWHC'), AssertionError, lambda v: LAYOUT),
            (name, 'not_uint8', lambda v, c=call: c(v, v.u8_float, v.lut, BITS, 'NHWC'), AssertionError, lambda v: NOT_U8),
            (name, 'size', lambda v, c=call: c(v, v.u8_size, v.lut, BITS, 'NHWC'), AssertionError, lambda v: U8_SHAPE % (32, 32, (8, 40, 40, 3))),
            (name, 'channels', lambda v, c=call: c(v, v.u8_chan, v.lut, BITS, 'NHWC'), AssertionError, lambda v: U8_SHAPE % (32, 32, (8, 32, 32, 1))),
            (name, 'cpu', lambda v, c=call: c(v, v.u8_cpu, v.lut, BITS, 'NHWC'), RuntimeError, lambda v: ON_GPU),
            (name, 'empty', lambda v, c=call: c(v, v.u8_empty, v.lut, BITS, 'NHWC'), AssertionError, lambda v: 'empty batch'),
            (name, 'lut_dtype', lambda v, c=call: c(v, v.u8, v.lut_dtype, BITS, 'NHWC'), AssertionError, lut_msg),
            (name, 'lut_shape', lambda v, c=call: c(v, v.u8, v.lut_shape, BITS, 'NHWC'), AssertionError, lut_msg),
            (name, 'lut_strided', lambda v, c=call: c(v, v.u8, v.lut_strided, BITS, 'NHWC'), AssertionError, lut_msg),
            (name, 'bit_config_none', lambda v, c=call: c(v, v.u8, v.lut, None, 'NHWC'), ValueError, lambda v: 'None is not in list'),
            # two faults: the layout is looked at before the dtype, the device before the table
            (name, 'layout+not_uint8', lambda v, c=call: c(v, v.u8_float, v.lut, BITS, 'NWHC'), AssertionError, lambda v: LAYOUT),
            (name, 'cpu+lut', lambda v, c=call: c(v, v.u8_cpu, v.lut_shape, BITS, 'NHWC'), RuntimeError, lambda v: ON_GPU),
        ]
    out_msg = lambda v: 'out must be a contiguous fp32 [8, 10] tensor on %s' % v.dev
    cover = lambda v: 'slices [3, 3] do not cover a batch of 8'
    cases += [
        # two faults: the geometry is looked at before the device
        ('forward', 'cpu+size', lambda v: v.plan.forward(v.x_cpu_size, BITS), AssertionError, lambda v: SIZE % (40, 40, 32, 32)),
        ('forward', 'out', lambda v: v.plan.forward(v.x, BITS, out=v.out_bad), AssertionError, out_msg),
        ('forward_streams', 'out', lambda v: v.plan.forward_streams(v.x, BITS, v.out_bad), AssertionError, out_msg),
        ('forward_uint8', 'out', lambda v: v.plan.forward_uint8(v.u8, v.lut, BITS, out=v.out_bad), AssertionError, out_msg),
        ('forward_uint8_streams', 'out', lambda v: v.plan.forward_uint8_streams(v.u8, v.lut, BITS, v.out_bad), AssertionError, out_msg),
        ('forward_linear_taps', 'out', lambda v: v.plan.forward_linear_taps(v.x, BITS, out=v.out_bad), AssertionError, out_msg),
        ('forward_streams', 'slices', lambda v: v.plan.forward_streams(v.x, BITS, v.out, slices=[3, 3]), AssertionError, cover),
        ('forward_streams', 'slices_zero', lambda v: v.plan.forward_streams(v.x, BITS, v.out, slices=[8, 0]), AssertionError,
         lambda v: 'slices [8, 0] do not cover a batch of 8'),
        ('forward_uint8_streams', 'slices', lambda v: v.plan.forward_uint8_streams(v.u8, v.lut, BITS, v.out, slices=[3, 3]), AssertionError, cover),
        ('profile_streams', 'slices', lambda v: v.plan.profile_streams(v.x, BITS, slices=[3, 3]), AssertionError, cover),
        ('forward_ddv', 'odd', lambda v: v.plan.forward_ddv(v.x[:7], BITS), AssertionError,
         lambda v: 'forward_ddv takes n clean images followed by their n perturbed twins: 7 images'),
        ('forward_ddv', 'stages', lambda v: v.plan.forward_ddv(v.x, BITS, stages='other'), ValueError,
         lambda v: "forward_ddv: stages must be 'engine' or 'full', not 'other'"),
    ]
    return cases


def _swin_cases():
    here = lambda v: 'images must live on %s' % v.dev
    cases = []
    for name in ('forward', 'forward_ddv', 'forward_linear_taps', 'profile'):
        call = lambda v, x, name=name: getattr(v.plan, name)(x)
        cases += [
            (name, 'size', lambda v, c=call: c(v, v.x_size[:2]), AssertionError, lambda v: SIZE % (64, 64, 56, 56)),
            (name, 'channels', lambda v, c=call: c(v, v.x_chan[:2]), AssertionError, lambda v: SIZE % (56, 56, 56, 56)),
            (name, 'cpu', lambda v, c=call: c(v, v.x_cpu[:2]), RuntimeError, here),
        ]
    u8 = lambda v, x, lut, lay='NHWC', **kw: v.plan.forward_uint8(x, lut, lay, **kw)
    lut_msg = lambda v: 'lut must be a contiguous int8 [3, 256] tensor on %s (SwinPlan.input_lut)' % v.dev
    cover = lambda v: 'slices [4, 4] do not cover a batch of 9'
    twins = 'forward_ddv takes n clean images followed by their n perturbed twins, got %d images'
    cases += [
        ('forward_uint8', 'layout', lambda v: u8(v, v.u8, v.lut, 'NWHC'), AssertionError, lambda v: LAYOUT),
        ('forward_uint8', 'not_uint8', lambda v: u8(v, v.u8_float, v.lut), AssertionError, lambda v: NOT_U8),
        ('forward_uint8', 'size', lambda v: u8(v, v.u8_size, v.lut), AssertionError, lambda v: U8_SHAPE % (56, 56, (9, 64, 64, 3))),
        ('forward_uint8', 'channels', lambda v: u8(v, v.u8_chan, v.lut), AssertionError, lambda v: U8_SHAPE % (56, 56, (9, 56, 56, 1))),
        ('forward_uint8', 'empty', lambda v: u8(v, v.u8_empty, v.lut), AssertionError, lambda v: U8_SHAPE % (56, 56, (0, 56, 56, 3))),
        ('forward_uint8', 'cpu', lambda v: u8(v, v.u8_cpu, v.lut), RuntimeError, here),
        ('forward_uint8', 'lut_dtype', lambda v: u8(v, v.u8, v.lut_dtype), AssertionError, lut_msg),
        ('forward_uint8', 'lut_shape', lambda v: u8(v, v.u8, v.lut_shape), AssertionError, lut_msg),
        ('forward_uint8', 'lut_strided', lambda v: u8(v, v.u8, v.lut_strided), AssertionError, lut_msg),
        ('forward_uint8', 'layout+not_uint8', lambda v: u8(v, v.u8_float, v.lut, 'NWHC'), AssertionError, lambda v: LAYOUT),
        ('forward_uint8', 'cpu+lut', lambda v: u8(v, v.u8_cpu, v.lut_shape), RuntimeError, here),
        ('forward_uint8', 'slices', lambda v: u8(v, v.u8, v.lut, n_streams=2, slices=[4, 4]), AssertionError, cover),
        ('forward', 'slices', lambda v: v.plan.forward(v.x, n_streams=2, slices=[4, 4]), AssertionError, cover),
        ('forward_ddv', 'odd', lambda v: v.plan.forward_ddv(v.x[:3]), AssertionError, lambda v: twins % 3),
        ('forward_ddv', 'empty', lambda v: v.plan.forward_ddv(v.x_empty), AssertionError, lambda v: twins % 0),
    ]
    return cases


def _refused(v, call, exc, message):
    with pytest.raises(exc) as info:
        call(v)
    assert type(info.value) is exc and str(info.value) == message(v)


VIT_CASES, SWIN_CASES = _vit_cases(), _swin_cases()


@pytest.mark.parametrize('call,exc,message', [c[2:] for c in VIT_CASES], ids=['%s-%s' % c[:2] for c in VIT_CASES])
def test_frozen_plan_refuses(vit, call, exc, message):
    _refused(vit, call, exc, message)


@pytest.mark.parametrize('call,exc,message', [c[2:] for c in SWIN_CASES], ids=['%s-%s' % c[:2] for c in SWIN_CASES])
def test_swin_plan_refuses(swin, call, exc, message):
    _refused(swin, call, exc, message)


if torch.cuda.device_count() > 1:          # (a case of the tables above that exists only where there is a second GPU)
    def test_plans_refuse_a_tensor_on_another_gpu(vit, swin):
        other = torch.device('cuda', (vit.dev.index + 1) % torch.cuda.device_count())
        msg = lambda v: 'images live on %s, the frozen plan on %s' % (other, v.dev)
        for call in VIT_F32.values():
            _refused(vit, lambda v: call(v, v.x.to(other), BITS), RuntimeError, msg)
        for call in VIT_U8.values():
            _refused(vit, lambda v: call(v, v.u8.to(other), v.lut, BITS, 'NHWC'), RuntimeError, msg)
        here = lambda v: 'images must live on %s' % v.dev
        for name in ('forward', 'forward_ddv', 'forward_linear_taps', 'profile'):
            _refused(swin, lambda v: getattr(v.plan, name)(v.x[:2].to(other)), RuntimeError, here)
        _refused(swin, lambda v: v.plan.forward_uint8(v.u8.to(other), v.lut), RuntimeError, here)


# ---- the sliced forwards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('threaded', [True, False], ids=['threads', 'one_thread'])
@pytest.mark.parametrize('slices', [[3, 2, 2, 1], [2, 2, 2, 1, 1]], ids=['caller_gets_the_4th', 'the_5th_wraps_to_side_0'])
def test_micro_vit_sliced_equals_whole(vit, monkeypatch, slices, threaded):
    """8 images on three side streams and the caller's: four slices (one per stream), and five (side stream 0 gets two calls)"""
    monkeypatch.setattr(E, 'THREADED_ENQUEUE', threaded)
    out = torch.full((8, 10), float('nan'), device='cuda')
    assert vit.plan.forward_streams(vit.x, BITS, out, slices=slices) is out
    torch.cuda.synchronize()
    assert torch.equal(out, vit.ref)
    out_u8 = torch.full((8, 10), float('nan'), device='cuda')
    assert vit.plan.forward_uint8_streams(vit.u8, vit.lut, BITS, out_u8, slices=slices) is out_u8
    torch.cuda.synchronize()
    assert torch.equal(out_u8, vit.ref_u8)


def test_micro_swin_sliced_equals_whole(swin, monkeypatch):
    """9 images as 4 + 3 on two side streams and 2 on the caller's: the first call records on the calling thread, the second one
    enqueues from the worker threads"""
    monkeypatch.setattr(E, 'THREADED_ENQUEUE', True)
    plan = swin.plan
    with torch.no_grad():
        whole = plan.forward(swin.x, n_streams=1)
        assert not any(k in plan._recorded for k in ((4, 1, True), (3, 2, True)))
        first = plan.forward(swin.x, n_streams=2, slices=[4, 3, 2])
        assert all(k in plan._recorded for k in ((4, 1, True), (3, 2, True), (2, 0, True)))
        second = plan.forward(swin.x, n_streams=2, slices=[4, 3, 2])
        whole_u8 = plan.forward_uint8(swin.u8, swin.lut, n_streams=1)
        sliced_u8 = plan.forward_uint8(swin.u8, swin.lut, n_streams=2, slices=[4, 3, 2])
    torch.cuda.synchronize()
    assert whole.shape == (9, 10)
    assert torch.equal(first, whole) and torch.equal(second, whole)
    assert torch.equal(sliced_u8, whole_u8)
