"""GPU: the DDV stages inside attention - the score codes (qact_attn1; Swin: also qact2) and the log2 softmax exponents.

  operator level    p2v_lis_attention_taps (resident and streaming kernel) and p2v_window_attention_taps (both window kernels): the pitched
                    planes in sentinel arenas against the oracle, `out` byte-identical to the untapped launch
  reduction         P2V_COS_LOG2K against int64 sums computed on the host, bit for bit
  whole model       FrozenPlan.forward_ddv(attention=True) / SwinPlan.forward_ddv(attention=True) against the oracle's integer sums
                    (tests/_ddv_attention_ref.py) and against the REAL reference's taps of tests/golden/micro_vit.npz; the other stages and
                    the logits byte-identical to the call without the option; the scratch in an arena; refusals

Tolerances: every new stage is an exact integer sum - bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _arena import SENTINELS, Arena, twice
from _ddv_attention_ref import expected, int_sums, log2k_sums, swin_attention_stages, vit_attention_stages, window_taps_reference
from _tuning import tuning
from conftest import golden_calib, gpu_ok, load_golden
from test_forward_state_gpu import _cfg, _same_bits
from test_kernel_edges_gpu import _attn_reference, _codes, _gen
from test_swin_modeldiff_gpu import _calibrated, _micro7, _pairs

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


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


# --------------------------------------------------------------------------------------------------
# 1. ViT operator
# --------------------------------------------------------------------------------------------------
# tokens, head_dim, batch, heads, kernel (0 resident, 2 streaming)
VIT_SHAPES = [(1, 64, 2, 3, 0), (5, 32, 2, 3, 0), (16, 64, 2, 3, 0), (17, 64, 2, 3, 0),
              (33, 48, 2, 3, 0),                  # a multiplier that is no power of two: the fp32 score chain
              (197, 64, 1, 2, 0),                 # last 16-key block all padding
              (224, 64, 1, 2, 0),                 # no padding
              (577, 64, 1, 1, 0),                 # the 256-register form
              (384, 128, 1, 1, 0),
              (609, 64, 1, 1, 2), (385, 128, 1, 1, 2)]
S_Q1, S_AT, S_A2 = 2.0 ** -4, 2.0 ** -4, 2.0 ** -3


@functools.lru_cache(maxsize=None)
def _vit_case(N, hd, B, H):
    """codes of std 30; in every (image, head) query 0 and key 0 are all 127 and key 1 all -128, so row 0 scores 127 and -128 and key 1 gets
    no probability (exponent 16); in one head every key but key 0 is all -128: key 0 takes the whole probability of row 0 (exponent 0).
    One token: a row is one score and its exponent is 0 - the two ends of the score range sit in two heads of image 0."""
    import p2vit_oracle as O
    gen = _gen(7000 + 10 * N + hd)
    qkv = _codes(gen, (B, N, 3, H, hd), 30.0)
    qkv[:, 0, 0] = 127
    qkv[:, 0, 1] = 127
    if N > 1:
        qkv[:, 1, 1] = -128
        qkv[-1, 1:, 1, -1] = -128           # last head of the last image: every key but key 0 at the bottom, so key 0 takes all of row 0
    else:
        qkv[0, 0, 1, 1] = -128
    qkv = qkv.reshape(B, N, 3 * H * hd)
    sc, k, out = _attn_reference(O, qkv, H, hd, S_Q1, S_AT, S_A2)
    return qkv, sc, k, out


def _run_vit_taps(E, qkv, H, hd, sentinel, tap, pitch, which=(True, True)):
    import p2vit_oracle as O
    B, N = qkv.shape[:2]
    D = H * hd
    x0, bb, cc = O.lis_consts(torch.tensor([S_AT]))
    at = E.Attn(S_Q1 * S_Q1, float(np.float32(hd ** -0.5)), 1.0 / S_AT, S_Q1 / S_A2, x0, bb, cc)
    a = Arena(B * N, 3 * D, 3 * D, torch.int8, sentinel, init=qkv.reshape(B * N, 3 * D))
    out = Arena(B * N, D, D, torch.int8, sentinel)
    sc = Arena(B * H * N, N, pitch, torch.int8, sentinel) if tap and which[0] else None
    pk = Arena(B * H * N, N, pitch, torch.int8, sentinel) if tap and which[1] else None
    L = E.lib()
    if tap:
        E.check(L.p2v_lis_attention_taps(a.ptr, B, N, H, hd, C.byref(at), out.ptr, sc.ptr if sc else None, pk.ptr if pk else None, pitch,
                                         E.stream_ptr()))
    else:
        E.check(L.p2v_lis_attention(a.ptr, B, N, H, hd, C.byref(at), out.ptr, None, E.stream_ptr()))
    _sync()
    what = ('attention taps', B, N, H, hd, tap)
    a.read(('qkv', what))
    r = dict(out=out.read(('out', what)).float().reshape(B, N, D))
    if sc:
        r['scores'] = sc.read(('score_codes', what)).long().reshape(B, H, N, N)
    if pk:
        r['probs_k'] = pk.read(('probs_k', what)).long().reshape(B, H, N, N)
    return r


@pytest.mark.parametrize('N,hd,B,H,kernel', VIT_SHAPES)
def test_lis_attention_taps(dva, N, hd, B, H, kernel):
    E = dva.engine
    L = E.lib()
    qkv, sc, k, ref = _vit_case(N, hd, B, H)
    assert int(sc.max()) == 127 and int(sc.min()) == -128, (int(sc.min()), int(sc.max()))
    assert bool((k == 0).any()) and (N == 1 or bool((k == 16).any()))          # one token: the only exponent a row can hold is 0
    assert L.p2v_attention_kernel(hd, N, 1) == kernel
    pitch = _up16(N) + 16
    plain = twice(lambda s: _run_vit_taps(E, qkv, H, hd, s, False, pitch))
    got = twice(lambda s: _run_vit_taps(E, qkv, H, hd, s, True, pitch))
    assert torch.equal(got['out'], plain['out']) and torch.equal(plain['out'], ref), (N, hd)
    assert torch.equal(got['scores'], sc.long()), (N, hd, int((got['scores'] != sc.long()).sum()))
    assert torch.equal(got['probs_k'], k.long()), (N, hd, int((got['probs_k'] != k.long()).sum()))
    if N in (17, 33):      # each plane alone, the tight pitch, and the resident shapes on the streaming kernel
        one = _run_vit_taps(E, qkv, H, hd, SENTINELS[0], True, _up16(N), which=(True, False))
        two = _run_vit_taps(E, qkv, H, hd, SENTINELS[1], True, _up16(N), which=(False, True))
        assert torch.equal(one['scores'], sc.long()) and torch.equal(two['probs_k'], k.long()) and torch.equal(one['out'], two['out'])
        with tuning(L, attn_stream=1):
            st = _run_vit_taps(E, qkv, H, hd, SENTINELS[0], True, pitch)
        assert torch.equal(st['scores'], sc.long()) and torch.equal(st['probs_k'], k.long()) and torch.equal(st['out'], ref)


# --------------------------------------------------------------------------------------------------
# 2. Swin operator
# --------------------------------------------------------------------------------------------------
WIN_SCALES = dict(qact1=2.0 ** -4, qact_attn1=2.0 ** -3, qact_table=2.0 ** -5, qact2=2.0 ** -4, qact3=2.0 ** -3)
WIN_CASES = [(14, 7, 0), (14, 7, 3), (16, 8, 0), (18, 9, 4), (24, 12, 6)]      # feature map side, window side, shift: 4 windows each
WIN_HEADS, WIN_B = 3, 2


@functools.lru_cache(maxsize=None)
def _win_case(Hf, ws, shift):
    import diff_vit_amd
    S = diff_vit_amd.synth
    C_, T = WIN_HEADS * 32, Hf * Hf
    tag = 'att%d_%d_%d' % (Hf, ws, shift)
    qkv = torch.clamp(torch.round(S.normal(9, 'wq' + tag, (WIN_B, T, 3 * C_), 25.0)), -128, 127)
    qkv[:, 0] = 127                     # token 0: query and key at the top ...
    qkv[:, 1, C_:2 * C_] = -128         # ... token 1 (its neighbour: the same window and region): the key at the bottom
    tab = torch.clamp(torch.round(S.normal(9, 'wt' + tag, ((2 * ws - 1) ** 2, WIN_HEADS), 30.0)), -128, 127)
    return qkv, tab, window_taps_reference(qkv, tab, WIN_HEADS, Hf, ws, shift, WIN_SCALES)


def _run_win_taps(E, qkv, tab, ref, ws, sentinel, tap, pitch):
    import p2vit_oracle as O
    c = WIN_SCALES
    B, T = qkv.shape[:2]
    heads, N, nW = WIN_HEADS, ws * ws, ref['idx'].shape[0]
    lis = O.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(tab=tab.to(torch.int8).contiguous().cuda(), idx=ref['idx'].to(torch.int32).contiguous().cuda(),
               reg=None if ref['region'] is None else ref['region'].to(torch.int8).contiguous().cuda())
    wa = E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], lis[0], lis[1], lis[2],
                   E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws, nW)
    a = Arena(B * T, 3 * heads * 32, None, torch.int8, sentinel, init=qkv.reshape(B * T, -1))
    out = Arena(B * T, heads * 32, None, torch.int8, sentinel)
    planes = [Arena(B * nW * heads * N, N, pitch, torch.int8, sentinel) for _ in range(3)] if tap else []
    L = E.lib()
    if tap:
        E.check(L.p2v_window_attention_taps(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, planes[0].ptr, planes[1].ptr, planes[2].ptr, pitch,
                                            E.stream_ptr()))
    else:
        E.check(L.p2v_window_attention(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, None, E.stream_ptr()))
    _sync()
    what = ('window taps', ws, tap)
    a.read(('qkv', what))
    r = dict(out=out.read(('out', what)).float().reshape(B, T, heads * 32))
    for nm, ar in zip(('a1', 'a2', 'k'), planes):
        r[nm] = ar.read((nm, what)).long().reshape(B, nW, heads, N, N)
    return r


@pytest.mark.parametrize('Hf,ws,shift', WIN_CASES)
def test_window_attention_taps(dva, Hf, ws, shift):
    E = dva.engine
    qkv, tab, ref = _win_case(Hf, ws, shift)
    assert ref['idx'].shape[0] == 4 and (ref['region'] is not None) == bool(shift)
    assert int(ref['a1'].max()) == 127 and int(ref['a1'].min()) == -128 and int(ref['a2'].max()) == 127 and int(ref['a2'].min()) == -128
    assert bool((ref['k'] == 0).any()) and bool((ref['k'] == 16).any()) and bool((ref['a1'] != ref['a2']).any())
    pitch = _up16(ws * ws) + 16
    plain = twice(lambda s: _run_win_taps(E, qkv, tab, ref, ws, s, False, pitch))
    got = twice(lambda s: _run_win_taps(E, qkv, tab, ref, ws, s, True, pitch))
    assert torch.equal(got['out'], plain['out']) and torch.equal(plain['out'], ref['want']), (Hf, ws, shift)
    for nm in ('a1', 'a2', 'k'):
        assert torch.equal(got[nm], ref[nm].long()), (Hf, ws, shift, nm, int((got[nm] != ref[nm].long()).sum()))


# --------------------------------------------------------------------------------------------------
# 3. the reduction over exponent codes
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('rows,cols', [(1, 1), (3, 5), (197 * 2, 197), (49 * 4 * 3, 49)])
def test_pair_cosine_log2k(dva, rows, cols, n):
    """bytes k in 0 ... 19 (16 and beyond: probability 0) in pitched rows whose padding holds k = 0 (a probability of 1 if it were read);
    the last sample of `a` is all 16: sums 0, and its DDV entry NaN as numpy gives.  Bit-equal to int64 sums computed on the host."""
    E = dva.engine
    L = E.lib()
    gen = _gen(8100 + rows + n)
    pitch = _up16(cols) + 16
    ka = torch.randint(0, 20, (n, rows, cols), generator=gen)
    kb = torch.randint(0, 20, (n, rows, cols), generator=gen)
    ka[-1] = 16
    want = log2k_sums(ka, kb)
    assert want[-1, 0] == 0 and want[-1, 1] == 0
    buf = torch.zeros(2, n, rows, pitch, dtype=torch.int8)
    buf[0, :, :, :cols], buf[1, :, :, :cols] = ka.to(torch.int8), kb.to(torch.int8)
    dev = buf.cuda()
    lay = (E.CosLayer * 1)(E.CosLayer(E.ptr(dev[0]), E.ptr(dev[1]), None, rows * pitch, pitch, rows, cols, E.COS_LOG2K))
    nbytes = L.p2v_pair_cosine_workspace_bytes(lay, 1, n)
    assert nbytes > 0
    res = []
    for _ in range(2):
        ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        sums = torch.full((1, n, 3), -1.0, dtype=torch.float64, device='cuda')
        E.check(L.p2v_pair_cosine(lay, 1, n, E.ptr(sums), E.ptr(ws), nbytes, E.stream_ptr()))
        _sync()
        res.append(sums.cpu().numpy()[0])
    assert np.array_equal(res[0].view(np.uint64), want.view(np.uint64)), (rows, cols, n, res[0], want)
    assert np.array_equal(res[0].view(np.uint64), res[1].view(np.uint64))
    d = dva.ddv.ddv_from_sums(torch.from_numpy(res[0]).reshape(1, n, 3))[0].numpy()
    assert np.isnan(d[-1])
    # the int8 form over the same bytes is another number: the element type is honoured
    lay[0].dtype = E.COS_I8
    sums = torch.empty(1, n, 3, dtype=torch.float64, device='cuda')
    ws = torch.empty(L.p2v_pair_cosine_workspace_bytes(lay, 1, n), dtype=torch.uint8, device='cuda')
    E.check(L.p2v_pair_cosine(lay, 1, n, E.ptr(sums), E.ptr(ws), ws.numel(), E.stream_ptr()))
    _sync()
    assert np.array_equal(sums.cpu().numpy()[0], int_sums(ka, kb))
    # scales are refused
    sc = torch.ones(cols, device='cuda')
    lay[0].dtype, lay[0].scale = E.COS_LOG2K, E.ptr(sc)
    assert L.p2v_pair_cosine(lay, 1, n, E.ptr(sums), E.ptr(ws), ws.numel(), E.stream_ptr()) == E.E_ARG


# --------------------------------------------------------------------------------------------------
# 4. whole model: ViT / DeiT
# --------------------------------------------------------------------------------------------------
def _check_vit(dva, O, plan, arch, W, c, x, bits, tag, sets=(('engine', False), ('engine', True), ('full', True))):
    depth = arch['depth']
    n = x.shape[0] // 2
    xc = x.cuda()
    st, _, ref_logits = vit_attention_stages(O, arch, W, c, x, bits)
    want = {nm: expected(v, kind) for nm, (v, kind) in st.items()}
    for stages, lin in sets:
        logits0, names0, sums0 = plan.forward_ddv(xc, bits, with_linear=lin, stages=stages)
        logits, names, sums = plan.forward_ddv(xc, bits, with_linear=lin, stages=stages, attention=True)
        _sync()
        assert names0 == dva.ddv.stage_names(depth, lin, stages == 'full') and names == dva.ddv.stage_names(depth, lin, stages == 'full', True)
        assert len(names) == len(names0) + 2 * depth and tuple(sums.shape) == (len(names), n, 3)
        assert torch.equal(logits, logits0) and torch.equal(logits.cpu(), ref_logits), (tag, stages, lin)
        by = dict(zip(names, sums.cpu().numpy()))
        for k, nm in enumerate(names0):                       # every other stage: the same bytes
            assert np.array_equal(sums0[k].cpu().numpy().view(np.uint64), by[nm].view(np.uint64)), (tag, stages, lin, nm)
        for nm, w in want.items():                            # the new stages: the oracle's integer sums
            assert np.array_equal(by[nm], w), (tag, stages, lin, nm, by[nm], w)
        assert torch.equal(sums, plan.forward_ddv(xc, bits, with_linear=lin, stages=stages, attention=True)[2]), 'bitwise repeatable'
    return st


def test_forward_ddv_attention_micro_vit(dva, oracle, micro):
    """micro-ViT, 3 pairs (the halves of the fixture's 6 evaluation images): against the oracle, and against the REAL reference's taps
    stored in tests/golden/micro_vit.npz for [8] * 10 and the mixed list"""
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x, g = micro['x_ev'], micro['g']
    n = x.shape[0] // 2
    assert x.shape[0] == 6, 'the fixture holds an even number of images (3 clean / 3 twin); fewer than 2 would not allow this check'
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10), ('qmix', [int(b) for b in g['bit_qmix']])):
        st = _check_vit(dva, oracle, plan, micro['arch'], micro['sd'], micro['calib'], x, bits, tag)
        if 'taps/%s/blocks.0.attn.qact_attn1' % tag not in g.files:
            assert tag == 'q4'
            continue
        _, names, sums = plan.forward_ddv(x.cuda(), bits, attention=True)
        by = dict(zip(names, sums.cpu().numpy()))
        for i in range(2):
            p = 'blocks.%d.attn.' % i
            sc, k = torch.from_numpy(g['taps/%s/%sqact_attn1' % (tag, p)]), torch.from_numpy(g['taps/%s/%ssoftmax_k' % (tag, p)])
            assert torch.equal(sc.long(), st[p + 'qact_attn1'][0].long()) and torch.equal(k.long(), st[p + 'log_int_softmax'][0].long())
            assert np.array_equal(by[p + 'qact_attn1'], int_sums(sc[:n], sc[n:])), (tag, p)
            assert np.array_equal(by[p + 'log_int_softmax'], log2k_sums(k[:n], k[n:])), (tag, p)


def test_forward_ddv_attention_deit_small(dva, oracle, synth):
    """the DeiT-S architecture, 2 pairs of 224 x 224 (197 tokens, 6 heads: the last 16-key block of the resident kernel is padding)"""
    g = load_golden('deit_small')
    arch = synth.ARCHS['deit_small']
    sd = synth.vit_state_dict(arch, int(g['seed']))
    c = golden_calib(g, oracle)
    plan = dva.FrozenPlan(arch, sd, c, device=torch.device('cuda:0'))
    x = synth.images(int(g['seed']), 4, 224, offset=1000)
    Ln = 4 * arch['depth'] + 2
    for tag, bits in (('q8', [8] * Ln), ('qmix', [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(Ln)])):
        st = _check_vit(dva, oracle, plan, arch, sd, c, x, bits, tag, sets=(('engine', False),))
        assert any(bool((v == 16).any()) and bool((v == 0).any()) for v, kind in st.values() if kind == 'log2k')
    assert plan.ddv_attn_bytes(2) == 2 * 4 * 6 * 197 * 208


def _ddv_ex2(E, pl, x2n, bits, fill, stage_set, att=True, att_short=0, expect=0):
    """p2v_forward_ddv_ex2 with the workspace, logits, sums, tap scratch and attention scratch (exactly p2v_ddv_attn_scratch_bytes) in
    arenas -> (status, logits, sums, workspace bytes, attention scratch bytes)"""
    L = E.lib()
    n = x2n.shape[0] // 2
    ws = Arena(1, L.p2v_ddv_workspace_bytes(pl._handle, n), None, torch.uint8, fill, offset=0)
    stages = L.p2v_ddv_stage_count_ex2(pl._handle, 1, stage_set)
    out = Arena(2 * n, pl.arch['num_classes'], None, torch.float32, fill)
    sums = Arena(stages * n, 3, None, torch.float64, fill)
    tb = L.p2v_ddv_tap_scratch_bytes(pl._handle, n)
    tp = Arena(1, tb, None, torch.uint8, fill)
    ab = L.p2v_ddv_attn_scratch_bytes(pl._handle, n)
    ap = Arena(1, ab, None, torch.uint8, fill)
    rc = L.p2v_forward_ddv_ex2(pl._handle, E.ptr(x2n), n, _cfg(bits), len(bits), out.ptr, ws.ptr, ws.width, 1, stage_set, tp.ptr, tb,
                               ap.ptr if att else None, ab - att_short, sums.ptr, E.stream_ptr())
    _sync()
    assert rc == expect, (rc, L.p2v_last_error())
    what = ('forward_ddv_ex2', n, stage_set, hex(fill))
    tp.read(('tap scratch',) + what)
    return (rc, out.read(('logits',) + what), sums.read(('sums',) + what).reshape(stages, n, 3), ws.read(('workspace',) + what).numpy().reshape(-1),
            ap.read(('attention scratch',) + what).numpy().reshape(-1))


def test_forward_ddv_attention_in_arenas_and_refusals(dva, micro):
    """one call per stage set on three pairs under two fills: nothing outside the workspace, the two scratches, the sums and the logits is
    written; of the attention scratch only the columns [0, tokens) of its rows; the results do not depend on the fills.  Refusals (missing,
    short scratch) leave every output untouched."""
    E = dva.engine
    L = E.lib()
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    n = x.shape[0] // 2
    bits = [int(b) for b in micro['g']['bit_qmix']]
    T, H = plan.tokens, micro['arch']['num_heads']
    pitch = _up16(T)
    assert L.p2v_ddv_attn_scratch_bytes(plan._handle, n) == 2 * 2 * n * H * T * pitch
    for stage_set, stages in ((E.DDV_STAGES_ATTN, 'engine'), (E.DDV_STAGES_ATTN | E.DDV_STAGES_FULL, 'full')):
        _, _, plain = plan.forward_ddv(x, bits, with_linear=True, stages=stages, attention=True)
        _sync()
        for fill in SENTINELS:
            _, out, sums, _, ab = _ddv_ex2(E, plan, x, bits, fill, stage_set)
            assert _same_bits(out, torch.from_numpy(micro['g']['logits/qmix'])), hex(fill)
            assert _same_bits(sums, plain.cpu()), (stage_set, hex(fill))
            rows = ab.reshape(-1, pitch)
            assert bool((rows[:, T:] == fill).all()), 'a column behind the row was written'
    fill = SENTINELS[0]

    def untouched(res):
        _, out, sums, wsb, ab = res
        return all(bool((t == fill).all()) for t in (out.numpy().view(np.uint8), sums.numpy().view(np.uint8), wsb, ab))
    assert untouched(_ddv_ex2(E, plan, x, bits, fill, E.DDV_STAGES_ATTN, att=False, expect=E.E_ARG)) and b'attn_scratch' in L.p2v_last_error()
    assert untouched(_ddv_ex2(E, plan, x, bits, fill, E.DDV_STAGES_ATTN | 1, att_short=1, expect=E.E_WORKSPACE)) and b'attn_scratch' in L.p2v_last_error()
    # without the flag the entry is p2v_forward_ddv_ex: the scratch stays as it was
    rc, out, sums, _, ab = _ddv_ex2(E, plan, x, bits, fill, E.DDV_STAGES_ENGINE)
    assert bool((ab == fill).all()) and _same_bits(sums, plan.forward_ddv(x, bits, with_linear=True)[2].cpu())


# --------------------------------------------------------------------------------------------------
# 5. whole model: Swin
# --------------------------------------------------------------------------------------------------
def _check_swin(dva, m, n, bits):
    D = dva.ddv
    x, xa = _pairs(dva, n, m.arch['img_size'])
    x2 = torch.cat((x, xa), 0)
    with torch.no_grad():
        st, ref = swin_attention_stages(m, x2, bits)
    want = {nm: expected(v, kind) for nm, (v, kind) in st.items()}
    m.cuda()
    try:
        with torch.no_grad():
            fwd = m(x2.cuda(), bits=bits).cpu()
            plan = m._plan
            for lin in (False, True):
                logits0, names0, sums0 = plan.forward_ddv(x2.cuda(), lin)
                logits, names, sums = plan.forward_ddv(x2.cuda(), lin, attention=True)
                _sync()
                assert names0 == D.swin_stage_names(m.arch['depths'], lin) and names == D.swin_stage_names(m.arch['depths'], lin, True)
                assert len(names) == len(names0) + 3 * sum(m.arch['depths'])
                assert torch.equal(logits, logits0) and torch.equal(logits.cpu(), fwd) and torch.equal(fwd, ref)
                by = dict(zip(names, sums.cpu().numpy()))
                for k, nm in enumerate(names0):
                    assert np.array_equal(sums0[k].cpu().numpy().view(np.uint64), by[nm].view(np.uint64)), (bits, lin, nm)
                for nm, w in want.items():
                    assert np.array_equal(by[nm], w), (bits, lin, nm, by[nm], w)
            d = dva.compute_ddv(m, x.cuda(), xa.cuda(), bits, attention=True)
            assert list(d) == D.swin_stage_names(m.arch['depths'], True, True)
            assert torch.equal(d[names[5]], D.ddv_from_sums(sums)[5])
            with pytest.raises(NotImplementedError):
                dva.compute_ddv(m, x.cuda(), xa.cuda(), [8] * 10, attention=True)
    finally:
        m.cpu()


@pytest.mark.parametrize('bits', [8, 4])
def test_forward_ddv_attention_micro_swin(dva, bits):
    """swin_micro_patch4_window7_56 (shifted and unshifted blocks, one merge: the 49-key kernel with its one-query tail block), 3 pairs"""
    _check_swin(dva, _micro7(), 3, bits)


def test_forward_ddv_attention_swin_window12(dva):
    """the 12 x 12 windows of the wide kernel, 2 pairs"""
    _check_swin(dva, _calibrated(dva, dva.swin.swin_micro_patch4_window12_96, 96), 2, 8)


def test_compute_ddv_attention_on_the_engine(dva, synth, micro, monkeypatch):
    """compute_ddv(fused micro-ViT, attention=True): ONE engine call, no hooked forward, the keys of the shared list; attention=False is
    today's dict"""
    from test_ddv import micro_model
    m = micro_model(dva, synth, micro['g']).cuda()
    dva.harness.calibrate_model(m, micro['x_cal'].cuda())
    x, xa = micro['x_ev'][:3], micro['x_ev'][3:]
    calls = {'engine': 0, 'hooks': 0}
    real_ddv, real_hooks = dva.FrozenPlan.forward_ddv, dva.ddv._hooked_outputs
    monkeypatch.setattr(dva.FrozenPlan, 'forward_ddv', lambda self, *a, **kw: (calls.__setitem__('engine', calls['engine'] + 1), real_ddv(self, *a, **kw))[1])
    monkeypatch.setattr(dva.ddv, '_hooked_outputs', lambda *a, **kw: (calls.__setitem__('hooks', calls['hooks'] + 1), real_hooks(*a, **kw))[1])
    d = dva.compute_ddv(m, x, xa, [8] * 10, attention=True)
    assert calls == {'engine': 1, 'hooks': 0} and list(d) == dva.ddv.stage_names(2, True, False, True)
    assert all(v.is_cuda and v.dtype == torch.float64 and v.shape == (3,) for v in d.values())
    d0 = dva.compute_ddv(m, x, xa, [8] * 10)
    assert list(d0) == dva.ddv.stage_names(2, True) and all(torch.equal(v, d[nm]) for nm, v in d0.items())
    df = dva.compute_ddv(m, x, xa, [8] * 10, stages='full', attention=True)
    assert list(df) == dva.ddv._with_qact_pos(dva.ddv.stage_names(2, True, True, True))
    # a -1 entry leaves the fused state: hooks on the same-named modules, the same keys, values within the fp32 bound of the hooked path
    calls.update(engine=0, hooks=0)
    dm = dva.compute_ddv(m, x, xa, [8] * 9 + [-1], attention=True)
    assert calls == {'engine': 0, 'hooks': 2} and list(dm) == list(d)
    for i in range(2):
        for nm in ('qact_attn1', 'log_int_softmax'):
            key = 'blocks.%d.attn.%s' % (i, nm)
            assert float((dm[key] - d[key]).abs().max()) <= 1e-9, key
