"""GPU: Swin window attention for 9 x 9 ... 12 x 12 windows (k_window_attention_wide) and the patch 4 / window 12 models built on it.

Kernel level: every softmax exponent and every output code against the oracle restatement of WindowAttention.forward (fed with qact1
codes, as tests/test_engine_gpu.py does for the 64-key kernel), with and without the probs_k tap; saturating and all-equal score rows;
the output footprint in sentinel arenas.  Model level: the engine against OracleSwin on every residual-stream tap and on the logits."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from _arena import Arena, twice
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

SCALES = dict(qact1=2.0 ** -4, qact_attn1=2.0 ** -3, qact_table=2.0 ** -5, qact2=2.0 ** -4, qact3=2.0 ** -3)


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def window_reference(qkv, tab, heads, Hf, ws, shift, c):
    """the scores / softmax / AV part of window_attention_quant on the partitioned windows, fed with qact1 codes:
    -> dict(idx, region, a1 [B*nW, heads, N, N] qact_attn1 codes, k softmax exponents, want [B, T, C] qact3 codes in natural order)"""
    import p2vit_oracle as O
    import swin_oracle as SO
    B, T = qkv.shape[:2]
    C_, N = heads * 32, ws * ws
    idx = SO.window_index(Hf, Hf, ws, shift)
    nW = idx.shape[0]
    region = mask = None
    if shift:
        mask = SO.shifted_window_mask(Hf, Hf, ws, shift)
        img = torch.zeros(Hf, Hf)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[hs, wsl] = cnt
                cnt += 1
        region = img.reshape(Hf // ws, ws, Hf // ws, ws).permute(0, 2, 1, 3).reshape(nW, N).long()
    xw = qkv[:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s1 = torch.tensor(c['qact1'])
    qs = (xw[0] * s1) * torch.tensor(32 ** -0.5, dtype=torch.float32)
    attn = (qs.double() @ (xw[1] * s1).double().transpose(-2, -1)).float()
    a1 = SO.q8(attn, c['qact_attn1'])
    bias = (tab * c['qact_table'])[SO.relative_position_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    xi = SO.q8(a1 * c['qact_attn1'] + bias.unsqueeze(0), c['qact2'])
    if mask is not None:
        xi = (xi.reshape(B, nW, heads, N, N) + torch.round(mask / c['qact2']).unsqueeze(1).unsqueeze(0)).reshape(B * nW, heads, N, N)
    k = O.lis_int(xi, torch.tensor([c['qact2']]))
    o = (O.lis_probs(k) @ (xw[2] * s1)).transpose(1, 2).reshape(B, nW * N, C_)
    want = torch.zeros(B, T, C_)
    want[:, idx.reshape(-1)] = SO.q8(o, c['qact3'])
    return dict(idx=idx, region=region, a1=a1, k=k.long().reshape(B, nW, heads, N, N), want=want)


def run_kernel(E, qkv, tab, ref, heads, ws, c, tap=True):
    """p2v_window_attention on dense operands -> (out [B, T, C] as float, probs_k [B, nW, heads, N, N] as long or None)"""
    import p2vit_oracle as O
    B, T = qkv.shape[:2]
    N, nW = ws * ws, ref['idx'].shape[0]
    lis = O.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(qkv=qkv.to(torch.int8).contiguous().cuda(), tab=tab.to(torch.int8).contiguous().cuda(),
               idx=ref['idx'].to(torch.int32).contiguous().cuda(),
               reg=None if ref['region'] is None else ref['region'].to(torch.int8).contiguous().cuda())
    wa = E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], lis[0], lis[1], lis[2],
                   E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws, nW)
    out = torch.full((B * T, heads * 32), 77, dtype=torch.int8, device='cuda')
    pk = torch.full((B, nW, heads, N, N), -1, dtype=torch.int8, device='cuda') if tap else None
    E.check(E.lib().p2v_window_attention(E.ptr(dev['qkv']), B, T, heads, 32, C.byref(wa), E.ptr(out), E.ptr(pk) if tap else None, E.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().float().reshape(B, T, heads * 32), (pk.cpu().long() if tap else None)


# ------------------------------------------------------------------------------------------------
# 1. kernel against the oracle
# ------------------------------------------------------------------------------------------------
CASES = [(3, 24, 12, 6, 2),      # masked, 9 full key blocks
         (5, 12, 12, 0, 2),      # a single window, heads not a multiple of 4
         (1, 36, 12, 6, 1),      # 9 windows
         (2, 18, 9, 4, 1),       # N = 81: one query in the last block
         (2, 27, 9, 0, 1),
         (4, 20, 10, 5, 1),      # N = 100
         (1, 22, 11, 5, 1)]      # N = 121


@functools.lru_cache(maxsize=None)
def case_inputs(heads, Hf, ws, shift, B, seed=9):
    """inputs as in test_window_attention_shifted_windows_vs_oracle (seeded normal x 25 codes with row 0 at 127, a table of normal x 30,
    the same five power-of-two scales) and the oracle's result for them: computed once per case"""
    import diff_vit_amd
    S = diff_vit_amd.synth
    C_, T = heads * 32, Hf * Hf
    tag = '%d_%d_%d' % (heads, Hf, ws)
    qkv = torch.clamp(torch.round(S.normal(seed, 'wq' + tag, (B, T, 3 * C_), 25.0)), -128, 127)
    qkv[0, 0] = 127
    tab = torch.clamp(torch.round(S.normal(seed, 'wt' + tag, ((2 * ws - 1) ** 2, heads), 30.0)), -128, 127)
    return qkv, tab, window_reference(qkv, tab, heads, Hf, ws, shift, SCALES)


def liveness(ref):
    """the conditions the comparison is worth something under, from the oracle's result alone"""
    k, want = ref['k'], ref['want']
    return dict(below16=float((k < 16).float().mean()), has16=bool((k == 16).any()), has0=bool((k == 0).any()),
                nonzero=float((want != 0).float().mean()))


@pytest.mark.parametrize('heads,Hf,ws,shift,B', CASES)
def test_window_attention_wide_vs_oracle(dva, heads, Hf, ws, shift, B):
    """every softmax exponent and every output code of the 65 ... 144-key kernel against the oracle, with and without the probs_k tap"""
    qkv, tab, ref = case_inputs(heads, Hf, ws, shift, B)
    live = liveness(ref)
    print('liveness', (heads, Hf, ws, shift, B), live)
    assert live['below16'] >= 0.40 and live['has16'] and live['has0'] and live['nonzero'] >= 0.80, live
    out, pk = run_kernel(dva.engine, qkv, tab, ref, heads, ws, SCALES, tap=True)
    out_nt, _ = run_kernel(dva.engine, qkv, tab, ref, heads, ws, SCALES, tap=False)
    assert torch.equal(pk, ref['k']), int((pk != ref['k']).sum())
    assert torch.equal(out, ref['want']), int((out != ref['want']).sum())
    assert torch.equal(out_nt, out), int((out_nt != out).sum())


# ------------------------------------------------------------------------------------------------
# 2. saturation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Hf,shift', [(12, 0), (24, 6)])
def test_window_attention_wide_all_equal_rows(dva, Hf, shift):
    """ws = 12, a constant qkv and a constant bias table: every score row is all-equal (within a region), where the sum of the probabilities
    is largest - 144 x 2^-7 = 1.125 without a mask.  v = -128 with qact3 scale = qact1 scale drives the output onto the clamp (-144 -> -128),
    with twice the scale it is -72 exactly: the P.V sum of 144 equal terms."""
    heads, ws, B = 2, 12, 1
    T = Hf * Hf
    for code, tcode in ((127, 0), (-128, 0), (3, -128), (0, 127)):
        qkv = torch.full((B, T, 3 * heads * 32), float(code))
        qkv[:, :, 2 * heads * 32:] = -128.0
        tab = torch.full(((2 * ws - 1) ** 2, heads), float(tcode))
        for s_q3 in (2.0 ** -4, 2.0 ** -3):
            c = dict(SCALES, qact3=s_q3)
            ref = window_reference(qkv, tab, heads, Hf, ws, shift, c)
            if not shift:
                assert bool((ref['k'] == 7).all())                              # round(144 / 1) -> 2^-7 each
                assert bool((ref['want'] == (-128 if s_q3 == 2.0 ** -4 else -72)).all())
            else:
                assert bool((ref['k'].min(-1)[0] < 7).any()) and bool((ref['k'] == 16).any())       # smaller regions, masked pairs
            out, pk = run_kernel(dva.engine, qkv, tab, ref, heads, ws, c)
            assert torch.equal(pk, ref['k']), (code, tcode, s_q3, int((pk != ref['k']).sum()))
            assert torch.equal(out, ref['want']), (code, tcode, s_q3, int((out != ref['want']).sum()))


@pytest.mark.parametrize('Hf,shift', [(12, 0), (24, 6)])
def test_window_attention_wide_saturating_scores(dva, Hf, shift):
    """ws = 12, q and k from {-128, 127} so that qact_attn1 clamps at both ends (asserted on the oracle's codes), v alternating 127 / -128"""
    heads, ws, B = 2, 12, 1
    T, D = Hf * Hf, heads * 32
    gen = torch.Generator().manual_seed(1700 + Hf)
    pm = lambda *shape: torch.where(torch.rand(*shape, generator=gen) < 0.5, torch.tensor(-128.0), torch.tensor(127.0))
    q = pm(T, heads, 32)
    q[0::4], q[1::4] = 127.0, -128.0
    k = pm(T, heads, 1).expand(T, heads, 32).clone()                      # a key is all 127 or all -128
    flips = torch.rand(T, heads, 32, generator=gen) < 0.05
    k[flips] = -k[flips] - 1
    par = (torch.arange(T).reshape(T, 1, 1) + torch.arange(32).reshape(1, 1, 32)) % 2
    v = torch.where(par == 0, torch.tensor(127.0), torch.tensor(-128.0)).expand(T, heads, 32)
    qkv = torch.stack([q, k, v], 1).reshape(1, T, 3 * D)
    tab = torch.clamp(torch.round(torch.randn((2 * ws - 1) ** 2, heads, generator=gen) * 30), -128, 127)
    ref = window_reference(qkv, tab, heads, Hf, ws, shift, SCALES)
    a1 = ref['a1']
    assert float((a1 == 127).float().mean()) > 0.2 and float((a1 == -128).float().mean()) > 0.2, 'qact_attn1 does not saturate'
    assert bool((ref['k'] < 16).any()) and bool((ref['k'] == 16).any())       # (many keys share the clamped maximum: no exponent 0)
    out, pk = run_kernel(dva.engine, qkv, tab, ref, heads, ws, SCALES)
    assert torch.equal(pk, ref['k']), int((pk != ref['k']).sum())
    assert torch.equal(out, ref['want']), int((out != ref['want']).sum())


# ------------------------------------------------------------------------------------------------
# 3. output footprint
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Hf,ws,shift', [(24, 12, 6), (12, 12, 0), (18, 9, 4)])
def test_window_attention_wide_footprint(dva, Hf, ws, shift):
    """three heads (96 channels), qkv_stride / out_stride dense and padded (288 -> 320, 96 -> 128) in sentinel arenas: the kernel writes the
    heads * 32 codes of a row and nothing in front of, behind or between the rows; the result does not depend on the input padding"""
    import p2vit_oracle as O
    E = dva.engine
    heads, B = 3, 2
    C_, T, N = heads * 32, Hf * Hf, ws * ws
    gen = torch.Generator().manual_seed(1800 + Hf + shift)
    qkv = torch.clamp(torch.round(torch.randn((B, T, 3 * C_), generator=gen) * 25.0), -128, 127)
    qkv[0, 0] = 127
    tab = torch.clamp(torch.round(torch.randn(((2 * ws - 1) ** 2, heads), generator=gen) * 30.0), -128, 127)
    c = SCALES
    ref = window_reference(qkv, tab, heads, Hf, ws, shift, c)
    k, nW = ref['k'], ref['idx'].shape[0]
    lis = O.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(tab=tab.to(torch.int8).cuda(), idx=ref['idx'].to(torch.int32).contiguous().cuda(),
               reg=None if ref['region'] is None else ref['region'].to(torch.int8).contiguous().cuda())

    def run(sentinel, ldq, ldo, tap):
        wa = E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], lis[0], lis[1], lis[2],
                       E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws, nW,
                       0 if ldq == 3 * C_ else ldq, 0 if ldo == C_ else ldo)
        a = Arena(B * T, 3 * C_, ldq, torch.int8, sentinel, init=qkv.reshape(B * T, 3 * C_))
        out = Arena(B * T, C_, ldo, torch.int8, sentinel)
        pk = Arena(B * nW * heads * N, N, N, torch.int8, sentinel) if tap else None
        E.check(E.lib().p2v_window_attention(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, pk.ptr if tap else None, E.stream_ptr()))
        torch.cuda.synchronize()
        what = ('window attention', Hf, ws, shift, ldq, ldo, tap)
        a.read(('qkv', what))
        res = dict(out=out.read(('out', what)).float().reshape(B, T, C_))
        if tap:
            res['probs_k'] = pk.read(('probs_k', what)).long().reshape(k.shape)
        return res

    for ldq, ldo, tap in ((320, 128, True), (320, 128, False), (3 * C_, C_, True), (3 * C_, 128, False), (320, C_, False)):
        got = twice(lambda s: run(s, ldq, ldo, tap))
        assert torch.equal(got['out'], ref['want']), (ldq, ldo, tap, int((got['out'] != ref['want']).sum()))
        assert not tap or torch.equal(got['probs_k'], k), (ldq, ldo, int((got['probs_k'] != k).sum()))
    assert (k < 16).any() and (k == 16).any()


# ------------------------------------------------------------------------------------------------
# 4. whole models: engine == OracleSwin on every residual-stream tap and on the logits
# ------------------------------------------------------------------------------------------------
def _micro(dva, img, ws, seed=5):
    from diff_vit_amd import swin
    kw = {} if (img, ws) == (96, 12) else dict(img_size=img, window_size=ws)
    m = swin.swin_micro_patch4_window12_96(cfg=dva.Config(True, True, 'minmax'), num_classes=10, **kw).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), seed))
    x = dva.synth.images(seed, 4, img)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
        m.model_quant()
    return m, x


@pytest.mark.parametrize('bits', [8, 4])
@pytest.mark.parametrize('img,ws', [(96, 12), (72, 9), (88, 11)])
def test_swin_micro_wide_windows_engine_vs_oracle(dva, img, ws, bits):
    """the micro architecture at 96^2 / window 12 (four shifted windows, then one), 72^2 / window 9 and 88^2 / window 11"""
    import swin_oracle as SO
    m, x = _micro(dva, img, ws)
    assert m.arch['window_size'] == ws and m.arch['img_size'] == img
    with torch.no_grad():
        taps_o = {}
        ref = SO.OracleSwin(m.arch, {k: v.cpu() for k, v in m.state_dict().items()}).quant_forward(x, m.export_calib(), bits, taps_o)
        m.cuda()
        out = m(x.cuda(), bits=bits)
        taps_g = {}
        m._plan.forward(x.cuda(), taps=taps_g)
        torch.cuda.synchronize()
    assert len(taps_g) >= 12
    for name, t in taps_g.items():
        want = taps_o[name].reshape(t.shape)
        assert torch.equal(t.cpu().int(), want.int()), (name, int((t.cpu().int() != want.int()).sum()), t.numel())
    assert torch.equal(out.cpu(), ref), float((out.cpu() - ref).abs().max())
    assert float((ref[0] - ref[1]).abs().max()) > 0


def test_swin_micro_window12_uint8_and_stream_slices(dva):
    """swin_micro_patch4_window12_96: forward_uint8 == forward on the normalised images, and the sliced multi-stream forward == one stream"""
    from diff_vit_amd import data as D
    m, _ = _micro(dva, 96, 12)
    m.cuda()
    mean, std = D.MODEL_STATS['swin'][:2]
    u8 = dva.synth.images_uint8(7, 5, 96)
    x = dva.synth.images(12, 33, 96).cuda()
    with torch.no_grad():
        for layout in ('NHWC', 'NCHW'):
            xu = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()
            for bits in (8, 4):
                want = m(D.normalize_uint8(xu, mean, std, layout).cuda(), bits).cpu()
                got = m.forward_uint8(xu.cuda(), bits, mean, std, layout).cpu()
                assert torch.equal(got, want), (layout, bits)
        m(x[:1])
        single = m._plan.forward(x, n_streams=1).cpu()
        sliced = m._plan.forward(x, n_streams=2).cpu()
        three = m._plan.forward(x, n_streams=2, slices=[12, 12, 9]).cpu()
        one = m(x[20:21]).cpu()
    assert single.shape == (33, 10) and torch.equal(sliced, single) and torch.equal(three, single) and torch.equal(single[20:21], one)
    assert len(set(single.argmax(1).tolist())) > 1 or float((single[0] - single[1]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------
# 5. the real geometry at real widths
# ------------------------------------------------------------------------------------------------
def test_swin_base_window12_384_engine_vs_oracle(dva):
    """Swin-B widths (128 ... 1024 channels, 4 ... 32 heads) at 384^2 / window 12 with depths (2, 2, 2, 2): feature maps of 96, 48, 24 and
    12 tokens, 64 ... 1 windows per image.  Calibrated through the drop-in surface on one image; two images at 8 bits: logits and every
    tap == OracleSwin, and image 0 gives the same logits alone and in the batch."""
    import swin_oracle as SO
    from diff_vit_amd import swin
    S = dva.synth
    m = swin.swin_base_patch4_window12_384(depths=(2, 2, 2, 2), num_classes=100, cfg=dva.Config(True, True, 'minmax')).eval()
    m.load_state_dict(S.swin_state_dict(m.state_dict(), 5))
    x = S.images(5, 2, 384)
    m.cuda()
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:1].cuda()); m.model_close_calibrate()
        m.model_quant()
        out = m(x.cuda())
        taps_g = {}
        m._plan.forward(x.cuda(), taps=taps_g)
        alone = m(x[:1].cuda())
        torch.cuda.synchronize()
        taps_o = {}
        ref = SO.OracleSwin(m.arch, {k: v.cpu() for k, v in m.state_dict().items()}).quant_forward(x, m.export_calib(), 8, taps_o)
    assert len(taps_g) >= 30
    for name, t in taps_g.items():
        want = taps_o[name].reshape(t.shape)
        assert torch.equal(t.cpu().int(), want.int()), (name, int((t.cpu().int() != want.int()).sum()), t.numel())
    assert torch.equal(out.cpu(), ref), int((out.cpu() != ref).sum())
    assert torch.equal(alone.cpu(), out[:1].cpu())
    assert float((ref[0] - ref[1]).abs().max()) > 0                  # the two images' logits differ: the comparison is not degenerate


# ------------------------------------------------------------------------------------------------
# 6. fuzz
# ------------------------------------------------------------------------------------------------
def test_fuzz_window_attention_up_to_12():
    """tools/fuzz_ops.py --max-window 12: its Swin cases over window sizes 2 ... 12 (nine cases: every size of the widened cycle once),
    random shifts, head counts, batch sizes and scales"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'fuzz_ops.py'), '7', '9', '--max-window', '12', '--only', 'winattn'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert '9 cases per op, 0 failing' in r.stdout
