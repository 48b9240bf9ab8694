"""GPU: the log-int-softmax at the width of its module's bit type (Config.BIT_TYPE_S: uint3 / uint4) on the engine.

Every check is bit equality against the helper of tests/_softmax_bits_ref.py (whose uint3 reading equals the REAL reference:
tests/golden/softmax_bits.npz, tests/test_softmax_bits.py).  The operators run in the sentinel arenas of tests/_arena.py; the inputs of every
launch are chosen so that the helper's 4-bit result holds every exponent 0 ... 15 and the zero class, asserted on the helper before the
GPU is touched: at 3 bits the classes 8 ... 15 become zeros, which is what the launch has to show.  At width 4 the new entry points return
the bytes of the existing ones."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _softmax_bits_ref as R
from _arena import SENTINELS, Arena, twice
from _ddv_attention_ref import expected, int_sums, log2k_sums, window_taps_reference
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

ALL_CLASSES = set(range(17))
CLASSES = {4: ALL_CLASSES, 3: set(range(8)) | {16}}
S_Q1, S_AT, S_A2 = 2.0 ** -4, 2.0 ** -4, 2.0 ** -3
AT = dict(s_q1=S_Q1, s_attn=S_AT, s_q2=S_A2)


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


def _up16(v):
    return (v + 15) // 16 * 16


def _codes(gen, shape, std):
    return torch.clamp(torch.round(torch.randn(shape, generator=gen) * std), -128, 127)


# --------------------------------------------------------------------------------------------------
# 1. ViT operator: resident, class-row, packed and streaming kernels
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _vit_case(N, hd, B, H):
    """codes of std 30; query 0 and key 0 of every (image, head) all 127, key 1 all -128 (row 0 scores 127 and -128: exponent 16); in the
    last head of the last image every key but key 0 is all -128: key 0 takes the whole probability of row 0 (exponent 0)"""
    gen = torch.Generator().manual_seed(9100 + 10 * N + hd)
    qkv = _codes(gen, (B, N, 3, H, hd), 30.0)
    qkv[:, 0, 0] = 127
    qkv[:, 0, 1] = 127
    qkv[:, 1, 1] = -128
    qkv[-1, 1:, 1, -1] = -128
    qkv = qkv.reshape(B, N, 3 * H * hd)
    ref = {bits: R.attention(qkv, H, AT, bits) for bits in (3, 4)}
    return qkv, ref


def _attn_struct(E, hd, s_a2=S_A2):
    import p2vit_oracle as O
    x0, bb, cc = O.lis_consts(torch.tensor([S_AT]))
    return E.Attn(S_Q1 * S_Q1, float(np.float32(hd ** -0.5)), 1.0 / S_AT, S_Q1 / s_a2, x0, bb, cc)


def _run_vit(E, qkv, H, hd, bits, form, sentinel, rows=0, at=None):
    """form: 'plain' (no tap), 'probs' (the dense probs_k plane), 'taps' (the two pitched planes), 'rows' (the class-row entry);
    bits None: the existing entry point"""
    B, N = qkv.shape[:2]
    D = H * hd
    at = at or _attn_struct(E, hd)
    L = E.lib()
    a = Arena(B * N, 3 * D, 3 * D, torch.int8, sentinel, init=qkv.reshape(B * N, 3 * D))
    out = Arena(B * N, D, D, torch.int8, sentinel)
    pitch = _up16(N) + 16
    pk = Arena(B * H * N, N, N, torch.int8, sentinel) if form == 'probs' else None
    sc = Arena(B * H * N, N, pitch, torch.int8, sentinel) if form == 'taps' else None
    kp = Arena(B * H * N, N, pitch, torch.int8, sentinel) if form == 'taps' else None
    st = E.stream_ptr()
    if form in ('plain', 'probs'):
        pp = pk.ptr if pk else None
        rc = (L.p2v_lis_attention(a.ptr, B, N, H, hd, C.byref(at), out.ptr, pp, st) if bits is None else
              L.p2v_lis_attention_bits(a.ptr, B, N, H, hd, C.byref(at), bits, out.ptr, pp, st))
    elif form == 'taps':
        rc = (L.p2v_lis_attention_taps(a.ptr, B, N, H, hd, C.byref(at), out.ptr, sc.ptr, kp.ptr, pitch, st) if bits is None else
              L.p2v_lis_attention_taps_bits(a.ptr, B, N, H, hd, C.byref(at), bits, out.ptr, sc.ptr, kp.ptr, pitch, st))
    else:
        rc = (L.p2v_lis_attention_rows(a.ptr, B, N, H, hd, C.byref(at), rows, out.ptr, st) if bits is None else
              L.p2v_lis_attention_rows_bits(a.ptr, B, N, H, hd, C.byref(at), bits, rows, out.ptr, st))
    _sync()
    what = ('attention', B, N, H, hd, bits, form)
    a.read(('qkv', what))
    r = dict(rc=torch.tensor(rc))
    if rc == 0 and form != 'rows':
        r['out'] = out.read(('out', what)).long().reshape(B, N, D)
    else:               # a refusal writes nothing; the class-row entry writes whole 16-row blocks and nothing behind them
        r['raw'] = out.read(('out', what)).long().reshape(B, N, D)
    for nm, ar in (('probs_k', pk), ('scores', sc), ('probs_kp', kp)):
        if ar is not None:
            r[nm] = ar.read((nm, what)).long().reshape(B, H, N, N)
    return r


def _check_classes(ref):
    for bits in (3, 4):
        assert R.exponent_classes(ref[bits][2]) == CLASSES[bits], (bits, sorted(R.exponent_classes(ref[bits][2])))
    assert not torch.equal(ref[3][0], ref[4][0]), 'the case does not tell the widths apart'


@pytest.mark.parametrize('bits', [3, 4])
@pytest.mark.parametrize('N,hd', [(17, 32), (17, 64), (17, 96), (197, 32), (197, 64), (197, 96)])
def test_resident_kernel(dva, N, hd, bits):
    """k_lis_attention through the three entry points: untapped, the dense exponent plane, the pitched planes (head_dim 64: the integer
    score shift; 32 and 96: the fp32 chain)"""
    E = dva.engine
    B, H = (2, 3) if N == 17 else (1, 2)
    assert E.lib().p2v_attention_kernel(hd, N, 0) == 0 and E.lib().p2v_attention_kernel(hd, N, 1) == 0
    qkv, ref = _vit_case(N, hd, B, H)
    _check_classes(ref)
    out, sc, k = (t.long() for t in ref[bits])
    plain = twice(lambda s: _run_vit(E, qkv, H, hd, bits, 'plain', s))
    probs = twice(lambda s: _run_vit(E, qkv, H, hd, bits, 'probs', s))
    taps = twice(lambda s: _run_vit(E, qkv, H, hd, bits, 'taps', s))
    for got in (plain, probs, taps):
        assert int(got['rc']) == 0 and torch.equal(got['out'], out), (N, hd, bits, int((got['out'] != out).sum()))
    assert torch.equal(probs['probs_k'], k), (N, hd, bits, int((probs['probs_k'] != k).sum()))
    assert torch.equal(taps['probs_kp'], k) and torch.equal(taps['scores'], sc), (N, hd, bits)
    if bits == 4:        # the bytes of the existing entry points
        for form, got in (('plain', plain), ('probs', probs), ('taps', taps)):
            old = _run_vit(E, qkv, H, hd, None, form, SENTINELS[0])
            assert all(torch.equal(old[nm], got[nm]) for nm in got), (N, hd, form)


@pytest.mark.parametrize('bits', [3, 4])
def test_class_row_entry(dva, bits):
    """p2v_lis_attention_rows at the width, 17 query rows: the first two 16-row blocks hold the helper's rows, nothing behind them is
    written"""
    E = dva.engine
    N, hd, B, H = 197, 64, 2, 3
    qkv, ref = _vit_case(N, hd, B, H)
    _check_classes(ref)
    for b in (3, 4):          # ... in the rows the launch computes
        assert R.exponent_classes(ref[b][2][:, :, :17]) == CLASSES[b]
    want = ref[bits][0].long()
    for sentinel in SENTINELS:
        got = _run_vit(E, qkv, H, hd, bits, 'rows', sentinel, rows=17)
        s8 = sentinel - 256 if sentinel > 127 else sentinel
        assert int(got['rc']) == 0 and torch.equal(got['raw'][:, :32], want[:, :32]) and bool((got['raw'][:, 32:] == s8).all()), bits
    if bits == 4:
        old = _run_vit(E, qkv, H, hd, None, 'rows', SENTINELS[1], rows=17)
        assert torch.equal(old['raw'], got['raw'])


@pytest.mark.parametrize('bits', [3, 4])
@pytest.mark.parametrize('hd,form,kernel', [(64, 'plain', 1), (32, 'plain', 2), (32, 'taps', 2)])
def test_packed_and_streaming_kernels(dva, hd, form, kernel, bits):
    """609 tokens, one image, one head: k_lis_attention_packed (head_dim 64, untapped) and k_lis_attention_stream (head_dim 32, with and
    without the pitched planes)"""
    E = dva.engine
    N, B, H = 609, 1, 1
    assert E.lib().p2v_attention_kernel(hd, N, int(form == 'taps')) == kernel
    qkv, ref = _vit_case(N, hd, B, H)
    _check_classes(ref)
    out, sc, k = (t.long() for t in ref[bits])
    got = twice(lambda s: _run_vit(E, qkv, H, hd, bits, form, s))
    assert int(got['rc']) == 0 and torch.equal(got['out'], out), (hd, form, bits, int((got['out'] != out).sum()))
    if form == 'taps':
        assert torch.equal(got['probs_kp'], k) and torch.equal(got['scores'], sc)
    if bits == 4:
        old = _run_vit(E, qkv, H, hd, None, form, SENTINELS[0])
        assert all(torch.equal(old[nm], got[nm]) for nm in got), (hd, form)


# --------------------------------------------------------------------------------------------------
# 2. Swin operator
# --------------------------------------------------------------------------------------------------
WIN_SCALES = dict(qact1=2.0 ** -4, qact_attn1=2.0 ** -3, qact_table=2.0 ** -5, qact2=2.0 ** -4, qact3=2.0 ** -3)
WIN_HEADS, WIN_B = 3, 2


@functools.lru_cache(maxsize=None)
def _win_case(Hf, ws, shift):
    import diff_vit_amd
    S = diff_vit_amd.synth
    C_, T = WIN_HEADS * 32, Hf * Hf
    tag = 'smb%d_%d_%d' % (Hf, ws, shift)
    qkv = torch.clamp(torch.round(S.normal(9, 'wq' + tag, (WIN_B, T, 3 * C_), 25.0)), -128, 127)
    qkv[:, 0] = 127
    qkv[:, 1, C_:2 * C_] = -128
    tab = torch.clamp(torch.round(S.normal(9, 'wt' + tag, ((2 * ws - 1) ** 2, WIN_HEADS), 30.0)), -128, 127)
    ref = {}
    for bits in (3, 4):
        with R.patched([bits]):
            ref[bits] = window_taps_reference(qkv, tab, WIN_HEADS, Hf, ws, shift, WIN_SCALES)
    return qkv, tab, ref


def _win_struct(E, ref, ws, dev, s_q3=None):
    import p2vit_oracle as O
    c = WIN_SCALES
    lis = O.lis_consts(torch.tensor([c['qact2']]))
    return E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], s_q3 or c['qact3'], lis[0], lis[1],
                     lis[2], E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws,
                     ref['idx'].shape[0])


def _win_dev(tab, ref):
    return dict(tab=tab.to(torch.int8).contiguous().cuda(), idx=ref['idx'].to(torch.int32).contiguous().cuda(),
                reg=None if ref['region'] is None else ref['region'].to(torch.int8).contiguous().cuda())


def _run_win(E, qkv, tab, ref, ws, bits, form, sentinel, s_q3=None):
    """form: 'plain', 'probs' (dense exponent plane), 'taps' (three pitched planes), 'op' (a P2V_OP_WINATTN record, bits in i4)"""
    B, T = qkv.shape[:2]
    heads, N, nW = WIN_HEADS, ws * ws, ref['idx'].shape[0]
    dev = _win_dev(tab, ref)
    wa = _win_struct(E, ref, ws, dev, s_q3)
    pitch = _up16(N) + 16
    a = Arena(B * T, 3 * heads * 32, None, torch.int8, sentinel, init=qkv.reshape(B * T, -1))
    out = Arena(B * T, heads * 32, None, torch.int8, sentinel)
    pk = Arena(B * nW * heads * N, N, N, torch.int8, sentinel) if form == 'probs' else None
    planes = [Arena(B * nW * heads * N, N, pitch, torch.int8, sentinel) for _ in range(3)] if form == 'taps' else []
    L, st = E.lib(), E.stream_ptr()
    if form in ('plain', 'probs'):
        pp = pk.ptr if pk else None
        rc = (L.p2v_window_attention(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, pp, st) if bits is None else
              L.p2v_window_attention_bits(a.ptr, B, T, heads, 32, C.byref(wa), bits, out.ptr, pp, st))
    elif form == 'taps':
        rc = (L.p2v_window_attention_taps(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr, pitch, st)
              if bits is None else
              L.p2v_window_attention_taps_bits(a.ptr, B, T, heads, 32, C.byref(wa), bits, out.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr,
                                               pitch, st))
    else:
        o = E.Op()
        o.kind, o.inp, o.out = E.OP_WINATTN, a.ptr, out.ptr
        o.i0, o.i1, o.i2, o.i3, o.i4 = B, T, heads, 32, bits
        o.wa = wa
        rc = L.p2v_run_ops((E.Op * 1)(o), 1, st)
    _sync()
    what = ('window attention', ws, bits, form)
    a.read(('qkv', what))
    r = dict(rc=torch.tensor(rc), out=out.read(('out', what)).long().reshape(B, T, heads * 32))
    if pk:
        r['probs_k'] = pk.read(('probs_k', what)).long().reshape(B, nW, heads, N, N)
    for nm, ar in zip(('a1', 'a2', 'k'), planes):
        r[nm] = ar.read((nm, what)).long().reshape(B, nW, heads, N, N)
    return r


@pytest.mark.parametrize('bits', [3, 4])
@pytest.mark.parametrize('Hf,ws,shift', [(8, 4, 2), (14, 7, 3), (14, 7, 0), (18, 9, 4)])
def test_window_attention(dva, Hf, ws, shift, bits):
    """k_window_attention (generic at 4 x 4, the 7 x 7 form with its one-query tail block) and k_window_attention_wide (9 x 9), with
    shifted-window regions, untapped and with every plane"""
    E = dva.engine
    qkv, tab, ref = _win_case(Hf, ws, shift)
    for b in (3, 4):
        assert R.exponent_classes(ref[b]['k']) == CLASSES[b], (b, sorted(R.exponent_classes(ref[b]['k'])))
    assert (ref[4]['region'] is not None) == bool(shift) and not torch.equal(ref[3]['want'], ref[4]['want'])
    if ws == 7:          # the lone 49th query of a 7 x 7 window has rows of its own in the kernel: they hold narrow exponents too
        k49 = ref[4]['k'][:, :, :, 48]
        assert bool(((k49 >= 8) & (k49 <= 15)).any())
    want, k = ref[bits]['want'].long(), ref[bits]['k'].long()
    plain = twice(lambda s: _run_win(E, qkv, tab, ref[bits], ws, bits, 'plain', s))
    probs = twice(lambda s: _run_win(E, qkv, tab, ref[bits], ws, bits, 'probs', s))
    taps = twice(lambda s: _run_win(E, qkv, tab, ref[bits], ws, bits, 'taps', s))
    for got in (plain, probs, taps):
        assert int(got['rc']) == 0 and torch.equal(got['out'], want), (ws, shift, bits, int((got['out'] != want).sum()))
    assert torch.equal(probs['probs_k'], k) and torch.equal(taps['k'], k), (ws, shift, bits)
    assert torch.equal(taps['a1'], ref[bits]['a1'].long()) and torch.equal(taps['a2'], ref[bits]['a2'].long())
    if bits == 4:
        for form, got in (('plain', plain), ('probs', probs), ('taps', taps)):
            old = _run_win(E, qkv, tab, ref[4], ws, None, form, SENTINELS[0])
            assert all(torch.equal(old[nm], got[nm]) for nm in got), (ws, shift, form)


# --------------------------------------------------------------------------------------------------
# 3. refusals and range: all before any launch
# --------------------------------------------------------------------------------------------------
def test_widths_other_than_3_and_4_are_refused(dva):
    E = dva.engine
    qkv, _ = _vit_case(17, 64, 2, 3)
    wq, tab, wref = _win_case(14, 7, 3)
    for bits in (2, 5, 0, 8):
        for form in ('plain', 'probs', 'taps', 'rows'):
            got = _run_vit(E, qkv, 3, 64, bits, form, SENTINELS[0], rows=1)
            assert int(got['rc']) == E.E_UNSUPPORTED and bool((got['raw'] == SENTINELS[0]).all()), (bits, form)
            assert all(bool((got[nm] == SENTINELS[0]).all()) for nm in got if nm not in ('rc', 'raw'))
        for form in ('plain', 'probs', 'taps') + (('op',) if bits else ()):
            got = _run_win(E, wq, tab, wref[4], 7, bits, form, SENTINELS[0])
            assert int(got['rc']) == E.E_UNSUPPORTED, (bits, form)
            assert all(bool((got[nm] == SENTINELS[0]).all()) for nm in got if nm != 'rc'), (bits, form)


def test_av_mul_range_at_3_bits(dva):
    """the kernels fold 2^(127 - 2^bits) into av_mul: at 3 bits av_mul up to 2^7 is accepted (and exact), 2^8 is refused before the
    launch; at 4 bits both pass, as before"""
    E = dva.engine
    N, hd, B, H = 17, 64, 2, 3
    qkv, _ = _vit_case(N, hd, B, H)
    for e, rc3 in ((7, 0), (8, E.E_UNSUPPORTED)):
        s_a2 = S_Q1 * 2.0 ** -e
        at = _attn_struct(E, hd, s_a2)
        assert at.av_mul == 2.0 ** e
        for bits in (3, 4):
            want = R.attention(qkv, H, dict(AT, s_q2=s_a2), bits)[0].long()
            got = _run_vit(E, qkv, H, hd, bits, 'plain', SENTINELS[0], at=at)
            if bits == 3 and rc3:
                assert int(got['rc']) == rc3 and bool((got['raw'] == SENTINELS[0]).all())
            else:
                assert int(got['rc']) == 0 and torch.equal(got['out'], want), (e, bits)
                assert int(want.max()) == 127 and int(want.min()) == -128 and bool((want.abs() < 127).any())
    # the window entry: s_q1 / s_q3
    wq, tab, wref = _win_case(14, 7, 3)
    for e, rc3 in ((7, 0), (8, E.E_UNSUPPORTED)):
        for bits in (3, 4):
            got = _run_win(E, wq, tab, wref[bits], 7, bits, 'plain', SENTINELS[0], s_q3=WIN_SCALES['qact1'] * 2.0 ** -e)
            if bits == 3 and rc3:
                assert int(got['rc']) == rc3 and bool((got['out'] == SENTINELS[0]).all())
            else:
                with R.patched([bits]):
                    want = window_taps_reference(wq, tab, WIN_HEADS, 14, 7, 3, dict(WIN_SCALES, qact3=WIN_SCALES['qact1'] * 2.0 ** -e))['want']
                assert int(got['rc']) == 0 and torch.equal(got['out'], want.long()), (e, bits)


def test_op_records_read_the_width_from_i4(dva):
    """P2V_OP_WINATTN: i4 = 0 (every earlier record) means 4, 3 and 4 are the widths"""
    E = dva.engine
    qkv, tab, ref = _win_case(14, 7, 3)
    old = _run_win(E, qkv, tab, ref[4], 7, None, 'plain', SENTINELS[0])
    for i4, bits in ((0, 4), (4, 4), (3, 3)):
        got = twice(lambda s: _run_win(E, qkv, tab, ref[bits], 7, i4, 'op', s))
        assert int(got['rc']) == 0 and torch.equal(got['out'], ref[bits]['want'].long()), i4
        if bits == 4:
            assert torch.equal(got['out'], old['out'])


def test_plan_setter_refusals(dva, micro):
    E = dva.engine
    L = E.lib()
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    assert plan.softmax_bits == [4, 4]
    assert L.p2v_plan_set_softmax_bits(plan._handle, 0, 5) == E.E_UNSUPPORTED and L.p2v_plan_set_softmax_bits(plan._handle, 0, 2) == E.E_UNSUPPORTED
    assert L.p2v_plan_set_softmax_bits(plan._handle, 2, 3) == E.E_ARG and L.p2v_plan_set_softmax_bits(plan._handle, -1, 3) == E.E_ARG
    assert L.p2v_plan_set_softmax_bits(None, 0, 3) == E.E_ARG
    x = micro['x_ev'][:2].cuda()
    before = plan.forward(x, [8] * 10).cpu()                   # a refused call leaves the plan as it was
    assert np.array_equal(before.numpy(), micro['g']['logits/q8'][:2])
    soft = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'], int_softmax=False, softmax_bits=3)      # unused there, as in the reference
    assert L.p2v_plan_set_softmax_bits(soft._handle, 0, 3) == E.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'], softmax_bits=5)
    with pytest.raises(ValueError):
        dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'], softmax_bits=[3, 4, 4])
    # a calibration state that names widths (export_calib of a uint3 model): read when the argument is None, refused when they disagree
    named = dict(micro['calib'])
    named['blocks.1.attn.log_int_softmax.bits'] = torch.tensor(3.0)
    assert dva.FrozenPlan(micro['arch'], micro['sd'], named).softmax_bits == [4, 3]
    assert dva.FrozenPlan(micro['arch'], micro['sd'], named, softmax_bits=[4, 3]).softmax_bits == [4, 3]
    with pytest.raises(ValueError, match=r'blocks\.1\.attn'):
        dva.FrozenPlan(micro['arch'], micro['sd'], named, softmax_bits=4)


# --------------------------------------------------------------------------------------------------
# 4. whole models
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def micro3(dva):
    """the fixture's micro ViT: weights of the recipe, the REAL reference's calibration state under uint3, its logits and taps"""
    import p2vit_oracle as O
    g = R.fixture()
    synth = dva.synth
    arch = synth.ARCHS['micro']
    sd = R.micro_weights(synth, arch, int(g['micro/seed']), float(g['micro/qkv_gain']))
    calib = O.unflatten_calib({k[len('micro/calib/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('micro/calib/')})
    x_ev = synth.images(int(g['micro/seed']), int(g['micro/n_eval']), arch['img_size'], offset=1000)
    x_cal = synth.images(int(g['micro/seed']), int(g['micro/n_calib']), arch['img_size'])
    return dict(g=g, arch=arch, sd=sd, calib=calib, x_ev=x_ev, x_cal=x_cal, lists=R.micro_bit_lists(4 * arch['depth'] + 2))


def test_micro_vit_uint3_equals_the_reference(dva, micro3):
    """a plan at 3 bits from the reference's own calibration state: the reference's logits for the three bit lists, and its score codes
    and exponents through the DDV stages inside attention (one pair: the two evaluation images); every forward form agrees"""
    g, arch, sd, calib, x = (micro3[k] for k in ('g', 'arch', 'sd', 'calib', 'x_ev'))
    plan = dva.FrozenPlan(arch, sd, calib, softmax_bits=3)
    plan4 = dva.FrozenPlan(arch, sd, calib)
    assert plan.softmax_bits == [3, 3] and plan4.softmax_bits == [4, 4]
    xc = x.cuda()
    for name, bits in micro3['lists'].items():
        want = torch.from_numpy(g['micro/logits/' + name])
        got = plan.forward(xc, bits).cpu()
        assert torch.equal(got, want), (name, int((got != want).sum()))
        # the engine's own taps: the output of every linear layer, against the helper's forward at 3 bits; for the all-8-bit list also
        # against the same outputs rebuilt from the REFERENCE's stored codes
        mine = {}
        assert torch.equal(R.vit_forward(arch, sd, calib, x, bits, 3, mine), want)
        lin = R.linear_outputs(arch, sd, calib, mine, bits)
        if name == 'q8':
            stored = {k[len('micro/taps/'):]: g[k] for k in g.files if k.startswith('micro/taps/')}
            assert all(torch.equal(a, b) for a, b in zip(lin, R.linear_outputs(arch, sd, calib, stored, bits)))
        logits, ltaps = plan.forward_linear_taps(xc, bits)
        assert torch.equal(logits.cpu(), want) and len(ltaps) == len(lin) == 4 * arch['depth'] + 2
        for k, (t, r) in enumerate(zip(ltaps, lin)):
            got = (t.permute(0, 2, 3, 1) if k == 0 else t).reshape(r.shape).cpu()
            assert torch.equal(got, r), (name, k, float((got - r).abs().max()))
        taps = {}
        assert torch.equal(plan.forward(xc, bits, taps=taps).cpu(), want)
        for i in range(arch['depth']):
            assert torch.equal(taps['qkv_output'][i], ltaps[1 + 4 * i]) and torch.equal(taps['fc1_output'][i], ltaps[3 + 4 * i])
        # behind a 3-bit softmax the proj input differs from the 4-bit plan's: the taps tell the widths apart
        assert not torch.equal(plan4.forward_linear_taps(xc, bits)[1][2], ltaps[2])
        # the sliced multi-stream forward and the uint8 entry (on images that are exactly representable: the fp32 forward of the same ones)
        big = xc.repeat(4, 1, 1, 1)
        out = torch.empty(8, arch['num_classes'], device='cuda')
        plan.forward_streams(big, bits, out, n_streams=2, slices=[3, 5])
        _sync()
        assert torch.equal(out.cpu(), want.repeat(4, 1)), name
        assert not torch.equal(plan4.forward(xc, bits).cpu(), want), 'the 4-bit plan gives other logits'
    bits = micro3['lists']['q8']
    logits, names, sums = plan.forward_ddv(xc, bits, attention=True)
    assert torch.equal(logits.cpu(), torch.from_numpy(g['micro/logits/q8']))
    by = dict(zip(names, sums.cpu().numpy()))
    for i in range(arch['depth']):
        p = 'blocks.%d.attn.' % i
        sc, k = torch.from_numpy(g['micro/taps/' + p + 'qact_attn1']), torch.from_numpy(g['micro/taps/' + p + 'softmax_k'])
        assert R.exponent_classes(k) <= CLASSES[3]
        assert np.array_equal(by[p + 'qact_attn1'], int_sums(sc[:1], sc[1:])), p
        assert np.array_equal(by[p + 'log_int_softmax'], log2k_sums(k[:1], k[1:])), p
    # every other stage of the engine's list against the reference's taps of the same name
    for nm in names:
        key = 'micro/taps/' + nm
        if key in g.files and not nm.endswith(('qact_attn1', 'log_int_softmax')) and g[key].ndim == 3:
            t = torch.from_numpy(g[key].astype(np.int64))
            s = calib[nm].reshape(-1)
            if s.numel() == 1:
                assert np.array_equal(by[nm], int_sums(t[:1], t[1:])), nm             # (one scale: the sums are the codes')
    # the statistics of the same stages: no exponent byte in 8 ... 15, the zero class counted at 16
    _, st = plan.forward_stats(xc, bits, attention=True)
    for i in range(arch['depth']):
        p = 'blocks.%d.attn.' % i
        k = g['micro/taps/' + p + 'softmax_k'].astype(np.int64)
        hist = st.cpu().record(p + 'log_int_softmax')['hist'].reshape(-1).numpy()
        assert np.array_equal(hist[:17], np.bincount(k.reshape(-1), minlength=17)[:17]) and int(hist[8:16].sum()) == 0 and int(hist[16]) > 0
    # profiling runs the same launches
    assert any(kind == 'attention' for kind, _ in plan.profile(xc, bits))
    assert torch.equal(plan.forward(xc, bits).cpu(), torch.from_numpy(g['micro/logits/q8']))


def test_forward_uint8_at_3_bits(dva, micro3):
    """forward_uint8 runs the plan's widths: the fp32 forward of the normalized images, bit for bit"""
    arch, sd, calib = (micro3[k] for k in ('arch', 'sd', 'calib'))
    plan = dva.FrozenPlan(arch, sd, calib, softmax_bits=3)
    from diff_vit_amd import data
    S = arch['img_size']
    u8 = torch.randint(0, 256, (3, S, S, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    mean, std, _ = data.MODEL_STATS['deit']
    lut32 = data.uint8_lut(mean, std)
    bits = micro3['lists']['qmix']
    want = R.vit_forward(arch, sd, calib, data.normalize_uint8(u8, mean, std, 'NHWC'), bits, 3)
    got = plan.forward_uint8(u8.cuda(), plan.input_lut(lut32), bits).cpu()
    assert torch.equal(got, want), int((got != want).sum())


def test_mixed_widths_and_the_model_surface(dva, micro3):
    """block 0 at 3 bits, block 1 at 4: through FrozenPlan and through the model (freeze reads every module's own bit type; export_calib
    and a plan file carry it); the class-row last block and the every-row one agree"""
    arch, sd, x, x_cal = (micro3[k] for k in ('arch', 'sd', 'x_ev', 'x_cal'))
    from functools import partial
    cfg = dva.Config(True, True, 'minmax')
    cfg.BIT_TYPE_S = dva.BIT_TYPE_DICT['uint3']
    m = dva.VisionTransformer(img_size=arch['img_size'], patch_size=arch['patch_size'], embed_dim=arch['embed_dim'], depth=arch['depth'],
                              num_heads=arch['num_heads'], num_classes=arch['num_classes'], mlp_ratio=arch['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=cfg)
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, x_cal.cuda())
    g = micro3['g']
    for name, bits in micro3['lists'].items():              # the product's own calibration and freeze: the reference's logits
        out = m(x.cuda(), bits, False)[0]
        assert torch.equal(out.cpu(), torch.from_numpy(g['micro/logits/' + name])), name
    assert m._plan.softmax_bits == [3, 3]
    m.blocks[1].attn.log_int_softmax.bit_type = dva.BIT_TYPE_DICT['uint4']
    assert m._plan.softmax_bits == [3, 3]                    # the plan is a snapshot: a new freeze reads the change
    m.freeze()
    assert m._plan.softmax_bits == [3, 4]
    calib = m.export_calib()
    ocal = {k: v for k, v in calib.items() if not k.endswith('.bits')}
    for name, bits in micro3['lists'].items():
        want = R.vit_forward(arch, sd, ocal, x, bits, [3, 4])
        assert not torch.equal(want, R.vit_forward(arch, sd, ocal, x, bits, 3))
        assert not torch.equal(want, R.vit_forward(arch, sd, ocal, x, bits, 4))
        got = m(x.cuda(), bits, False)[0].cpu()
        assert torch.equal(got, want), (name, int((got != want).sum()))
        direct = dva.FrozenPlan(arch, sd, calib, softmax_bits=[3, 4])
        assert torch.equal(direct.forward(x.cuda(), bits).cpu(), want)
        from _tuning import tuning
        with tuning(dva.engine.lib(), cls_rows=0):
            assert torch.equal(direct.forward(x.cuda(), bits).cpu(), want)
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, 'mixed.npz')
        dva.calib_io.save_plan(path, m)
        loaded = dva.calib_io.load_plan(path)
    assert loaded.softmax_bits == [3, 4]
    bits = micro3['lists']['qmix']
    assert torch.equal(loaded.forward(x.cuda(), bits), m._plan.forward(x.cuda(), bits))


def test_uint4_model_still_equals_the_untouched_oracle(dva, oracle, micro):
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'], softmax_bits=4)
    orc = oracle.OracleViT(micro['arch'], micro['sd'])
    orc.calib = micro['calib']
    x = micro['x_ev']
    for bits in ([8] * 10, [4] * 10, [int(b) for b in micro['g']['bit_qmix']]):
        with torch.no_grad():
            want = orc.quant_forward(x, bits)
        assert torch.equal(plan.forward(x.cuda(), bits).cpu(), want)


@pytest.mark.parametrize('factory,img', [('swin_micro_patch4_window7_56', 56), ('swin_micro_patch4_window12_96', 96)])
def test_micro_swin_at_3_bits(dva, factory, img):
    """micro Swin (7 x 7 windows; 12 x 12: the wide kernel), calibrated under uint3 by the product: against the helper at a uniform weight
    width and with a bit list, with the DDV stages inside the window attention; a mixed softmax assignment; uint4 against the oracle"""
    import _swin_bits_ref as RB
    import swin_oracle as SO
    from diff_vit_amd import swin
    cfg = dva.Config(True, True, 'minmax')
    cfg.BIT_TYPE_S = dva.BIT_TYPE_DICT['uint3']
    m = getattr(swin, factory)(cfg=cfg, num_classes=10).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    x = dva.synth.images(11, 2, img)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x); m.model_close_calibrate()
    m.model_quant()
    nA = sum(m.arch['depths'])
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    calib = m.export_calib()
    want3 = R.swin_forward(m.arch, sd, calib, x, 8, 3)
    want4 = R.swin_forward(m.arch, sd, calib, x, 8, 4)
    assert not torch.equal(want3, want4), 'the model does not tell the widths apart'
    m = m.cuda()
    plan = m.freeze()
    assert plan.softmax_bits == [3] * nA
    assert torch.equal(plan.forward(x.cuda()).cpu(), want3)
    # a bit list: the helper on the substituted weights
    bl = [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(m.bit_config_length())]
    bl[0] = 8
    sd_s, calib_s = RB.substituted(m.cpu(), bl)
    m = m.cuda()
    want_bl = R.swin_forward(m.arch, sd_s, calib_s, x, 8, 3)
    assert torch.equal(plan.forward(x.cuda(), bit_config=bl).cpu(), want_bl)
    # the DDV stages inside the window attention: exponent planes without the classes 8 ... 15
    logits, names, sums = plan.forward_ddv(x.cuda(), attention=True)
    assert torch.equal(logits.cpu(), want3)
    with R.patched([3]):
        from _ddv_attention_ref import swin_attention_stages
        mc = m.cpu()
        saved = mc.export_calib
        mc.export_calib = lambda: {k: v for k, v in saved().items() if not k.endswith('.bits')}
        st, ref_logits = swin_attention_stages(mc, x, 8)
        del mc.export_calib
    m = m.cuda()
    assert torch.equal(ref_logits, want3)
    by = dict(zip(names, sums.cpu().numpy()))
    for nm, (v, kind) in st.items():
        if kind == 'log2k':
            assert R.exponent_classes(v) <= CLASSES[3]
        assert np.array_equal(by[nm], expected(v, kind)), nm
    # a mixed assignment straight on the plan, and the default width against the untouched oracle
    widths = [3 if i % 2 == 0 else 4 for i in range(nA)]
    ocal = {k: v for k, v in calib.items() if not k.endswith('.bits')}
    mixed = dva.SwinPlan(m.arch, sd, ocal, softmax_bits=widths)
    assert mixed.softmax_bits == widths
    assert torch.equal(mixed.forward(x.cuda()).cpu(), R.swin_forward(m.arch, sd, calib, x, 8, widths))
    assert dva.SwinPlan(m.arch, sd, calib).softmax_bits == [3] * nA          # the widths export_calib names
    with pytest.raises(ValueError, match='log_int_softmax'):
        dva.SwinPlan(m.arch, sd, calib, softmax_bits=widths)
    four = dva.SwinPlan(m.arch, sd, ocal)
    assert four.softmax_bits == [4] * nA
    with torch.no_grad():
        assert torch.equal(four.forward(x.cuda()).cpu(), SO.OracleSwin(m.arch, sd).quant_forward(x, ocal, 8))
