"""GPU: Config(ptf=True, lis=False) of a Swin model on the engine, bit-equal to tests/_swin_float_ops_ref.py everywhere: the operator
p2v_window_softmax_attention in sentinel arenas over the shapes at which it can go wrong, hand-made tables, both ends of av_mul and every
refusal; the Swin plans under the configuration (fused, uint8, sliced, tapped, DDV, per-layer bit lists, the Swin-L widths) against the
helper's whole-model forward; and the default (True, True) path afterwards against the unchanged oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import _swin_bits_ref as RB
import _swin_float_ops_ref as R
from _arena import Arena, twice

pytestmark = pytest.mark.gpu

SCALES = dict(qact1=2.0 ** -4, qact_attn1=2.0 ** -3, qact_table=2.0 ** -5, qact2=2.0 ** -4, qact3=2.0 ** -3)
QK = float(np.float32(32 ** -0.5))


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def E(dva):
    from diff_vit_amd import engine
    engine.lib()
    return engine


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------
def _codes(gen, shape, std):
    return torch.clamp(torch.round(torch.randn(shape, generator=gen) * std), -128, 127)


def _regions(kind, nW, N):
    """region ids [nW, N] (None: no mask).  'two': two regions, the border moving with the window; 'alone': one token alone in its region
    (its row has den = tab[0]), another token per window"""
    if kind == 'none':
        return None
    t = torch.arange(N)
    reg = torch.zeros(nW, N, dtype=torch.long)
    for w in range(nW):
        if kind == 'two':
            reg[w] = (t >= (N // 2 + w) % max(N, 1)).long()
        else:
            reg[w, (N // 3 + 5 * w) % N] = 1
    return reg


def _case(ws, heads, B, nW, kind, seed, k_std=25.0):
    """inputs of one launch: the windows are a random partition of the image's tokens (every row is some window's token)"""
    gen = torch.Generator().manual_seed(seed)
    N, C_ = ws * ws, heads * 32
    T = nW * N
    qkv = _codes(gen, (B, T, 3 * C_), k_std)
    qkv[0, 0] = 127
    return dict(ws=ws, heads=heads, B=B, nW=nW, N=N, T=T, C=C_, qkv=qkv, tab=_codes(gen, ((2 * ws - 1) ** 2, heads), 30.0),
                idx=torch.randperm(T, generator=gen).reshape(nW, N), region=_regions(kind, nW, N))


def _reference(cs, c, table):
    """qact3 codes [B, T, C] in natural token order: swin_oracle's score path up to qact2 (tests/test_kernel_edges_gpu.py states it the same
    way), then the helper's table softmax"""
    import swin_oracle as SO
    B, nW, N, heads = cs['B'], cs['nW'], cs['N'], cs['heads']
    idx = cs['idx']
    xw = cs['qkv'][:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s1 = torch.tensor(c['qact1'])
    qs = (xw[0] * s1) * torch.tensor(32 ** -0.5, dtype=torch.float32)
    attn = (qs.double() @ (xw[1] * s1).double().transpose(-2, -1)).float()
    a1 = SO.q8(attn, c['qact_attn1'])
    bias = (cs['tab'] * c['qact_table'])[SO.relative_position_index(cs['ws']).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    a2 = SO.q8(a1 * c['qact_attn1'] + bias.unsqueeze(0), c['qact2'])
    allowed = None
    if cs['region'] is not None:
        allowed = (cs['region'].unsqueeze(1) == cs['region'].unsqueeze(2))[torch.arange(B * nW) % nW].unsqueeze(1)
    q3 = R.table_softmax_pv(a2, xw[2], allowed, table, c['qact1'] / c['qact3']).transpose(1, 2).reshape(B, nW * N, cs['C'])
    want = torch.zeros(B, cs['T'], cs['C'], dtype=torch.int64)
    want[:, idx.reshape(-1)] = q3
    return want, a2, allowed


def _wa(E, cs, c, dev, ldq=0, ldo=0):
    return E.WinAttn(c['qact1'], QK, c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], 0, 0, 0, E.ptr(dev['tab']), E.ptr(dev['idx']),
                     E.ptr(dev['reg']) if dev['reg'] is not None else None, cs['ws'], cs['nW'], ldq, ldo)


def _dev(cs, table):
    return dict(tab=cs['tab'].to(torch.int8).cuda(), idx=cs['idx'].to(torch.int32).contiguous().cuda(),
                reg=None if cs['region'] is None else cs['region'].to(torch.int8).contiguous().cuda(),
                table=torch.from_numpy(np.asarray(table, dtype=np.int64).astype(np.int32)).cuda())


def _run(E, cs, c, table, padded=False):
    """the launch in sentinel arenas, twice: -> int64 [B, T, C]; guards and the padding behind qkv_stride / out_stride rows keep their bytes"""
    dev = _dev(cs, table)
    B, T, C_ = cs['B'], cs['T'], cs['C']
    ldq, ldo = (3 * C_ + 32, C_ + 32) if padded else (3 * C_, C_)

    def run(sentinel):
        wa = _wa(E, cs, c, dev, ldq if padded else 0, ldo if padded else 0)
        a = Arena(B * T, 3 * C_, ldq, torch.int8, sentinel, init=cs['qkv'].reshape(B * T, 3 * C_))
        out = Arena(B * T, C_, ldo, torch.int8, sentinel)
        E.check(E.lib().p2v_window_softmax_attention(a.ptr, B, T, cs['heads'], 32, C.byref(wa), E.ptr(dev['table']), out.ptr, E.stream_ptr()))
        torch.cuda.synchronize()
        what = ('window softmax attention', cs['ws'], cs['heads'], B, cs['nW'], padded)
        a.read(('qkv', what))
        return dict(out=out.read(('out', what)).long().reshape(B, T, C_))
    return twice(run)['out']


# ws: N = 1; one full 16-key block; 25 (a full and a partial block); 49; exactly 64; 81, the first shape past one 64-key group; 144
@pytest.mark.parametrize('ws', [1, 2, 4, 5, 7, 8, 9, 12])
def test_operator_in_arenas(E, ws):
    """heads 1 / 3 / 4 / 5 (partial and second head groups) x batch 1 / 2 x 1 / 4 windows per image x no mask / two regions / one token
    alone in its region x dense / padded row strides, every combination (the launches are tiny): bit-equal to the helper, nothing written
    outside the heads * 32 codes of a row"""
    c = SCALES
    table = R.softmax_table(c['qact2'])
    n, seen_alone = 0, False
    for heads in (1, 3, 4, 5):
        for B in (1, 2):
            for nW in (1, 4):
                for ki, kind in enumerate(('none', 'two', 'alone')):
                    cs = _case(ws, heads, B, nW, kind, 7000 + 1000 * ws + 40 * heads + 12 * B + 3 * nW + ki)
                    want, a2, allowed = _reference(cs, c, table)
                    if kind == 'alone' and ws > 1:
                        seen_alone = seen_alone or bool((allowed.sum(-1) == 1).any())
                    for padded in (False, True):
                        got = _run(E, cs, c, table, padded)
                        assert torch.equal(got, want), (ws, heads, B, nW, kind, padded, int((got != want).sum()), int((got - want).abs().max()))
                        n += 1
    assert n == 96 and (seen_alone or ws == 1)


def test_hand_made_tables(E):
    """all entries 2^21 - 1 with v = -128 everywhere (the largest |num| and den: 144 keys); only tab[0] non-zero with several keys tied at
    the maximum (the probability is shared among the ties); the real table at s_q2 = 2^-2 and 2^-7"""
    c = dict(SCALES, qact3=SCALES['qact1'])                  # av_mul = 1
    # 1. the largest sums
    cs = _case(12, 3, 1, 2, 'none', 11)
    cs['qkv'][:, :, 2 * cs['C']:] = -128
    full = np.full(256, (1 << 21) - 1, dtype=np.int64)
    want, _, _ = _reference(cs, c, full)
    assert bool((want == -128).all())
    assert torch.equal(_run(E, cs, c, full), want)
    # 2. ties: K rows of two kinds and a zero bias table, so that keys of a kind score alike; only the row maximum counts
    only0 = np.zeros(256, dtype=np.int64)
    only0[0] = 12345
    for ws, kind in ((7, 'none'), (7, 'two'), (9, 'two'), (12, 'alone')):
        cs = _case(ws, 2, 2, 2, kind, 20 + ws)
        gen = torch.Generator().manual_seed(ws)
        kinds = _codes(gen, (2, 32), 25.0)
        pick = (torch.arange(cs['T']) % 3 == 0).long()
        for h in range(2):
            cs['qkv'][:, :, cs['C'] + 32 * h: cs['C'] + 32 * h + 32] = kinds[pick]
        cs['tab'].zero_()
        want, a2, allowed = _reference(cs, c, only0)
        a2m = a2 if allowed is None else torch.where(allowed.expand(a2.shape), a2, torch.full_like(a2, -1000))
        ties = (a2m == a2m.max(-1, keepdim=True)[0]).sum(-1)
        assert int(ties.max()) >= 3 and int(ties.min()) >= 1
        got = _run(E, cs, c, only0)
        assert torch.equal(got, want), (ws, kind, int((got != want).sum()))
    # 3. the real table at both ends of the qact2 scale (2^-2: the bound of the masked-key argument)
    for s2 in (2.0 ** -2, 2.0 ** -7):
        c2 = dict(c, qact2=s2, qact_attn1=s2 * 2, qact_table=s2 / 2)
        table = R.softmax_table(s2)
        for ws, kind in ((7, 'two'), (12, 'two'), (8, 'none')):
            cs = _case(ws, 3, 1, 2, kind, 31 + ws)
            want, _, _ = _reference(cs, c2, table)
            got = _run(E, cs, c2, table, padded=True)
            assert torch.equal(got, want), (s2, ws, kind, int((got != want).sum()))


def test_av_mul_ends(E):
    """s_q1 / s_q3 = 2^15: both saturations occur; 2^-40: every code rounds to zero"""
    table = R.softmax_table(SCALES['qact2'])
    cs = _case(7, 3, 2, 2, 'two', 41)
    hi = dict(SCALES, qact3=SCALES['qact1'] * 2.0 ** -15)
    want, _, _ = _reference(cs, hi, table)
    assert int(want.min()) == -128 and int(want.max()) == 127
    assert torch.equal(_run(E, cs, hi, table), want)
    lo = dict(SCALES, qact3=SCALES['qact1'] * 2.0 ** 40)
    want, _, _ = _reference(cs, lo, table)
    assert bool((want == 0).all())
    assert torch.equal(_run(E, cs, lo, table), want)


def test_refusals(E):
    """every refusal by its error code; they are host-side argument checks: nothing is launched"""
    L = E.lib()
    cs = _case(7, 3, 1, 2, 'two', 51)
    table = R.softmax_table(SCALES['qact2'])
    dev = _dev(cs, table)
    qkv = cs['qkv'].to(torch.int8).cuda()
    out = torch.full((cs['B'] * cs['T'] * cs['C'] + 16,), 0x5A, dtype=torch.int8, device='cuda')
    st = E.stream_ptr()

    def off(t, n):
        return C.c_void_p(t.data_ptr() + n)

    def call(c=SCALES, q=E.ptr(qkv), o=E.ptr(out), tb=E.ptr(dev['table']), hd=32, ws=None, wa_=True, edit=None):
        wa = _wa(E, cs, c, dev)
        if ws is not None:
            wa.ws = ws
        if edit is not None:
            edit(wa)
        return L.p2v_window_softmax_attention(q, cs['B'], cs['T'], cs['heads'], hd, C.byref(wa) if wa_ else None, tb, o, st)

    assert call(hd=64) == E.E_UNSUPPORTED and call(hd=16) == E.E_UNSUPPORTED
    assert b'p2v_window_softmax_attention' in L.p2v_last_error()
    assert call(c=dict(SCALES, qact2=2.0 ** -1)) == E.E_UNSUPPORTED and call(c=dict(SCALES, qact2=1.0)) == E.E_UNSUPPORTED
    assert b'2^-2' in L.p2v_last_error()
    assert call(c=dict(SCALES, qact3=SCALES['qact1'] * 2.0 ** -16)) == E.E_UNSUPPORTED            # s_q1 / s_q3 = 2^16
    assert call(c=dict(SCALES, qact3=SCALES['qact1'] * 2.0 ** 41)) == E.E_UNSUPPORTED             # 2^-41
    assert call(c=dict(SCALES, qact3=SCALES['qact1'] * 1.5)) == E.E_UNSUPPORTED                   # no power of two
    assert call(ws=0) == E.E_SHAPE and call(ws=13) == E.E_SHAPE
    assert call(q=None) == E.E_ARG and call(o=None) == E.E_ARG and call(tb=None) == E.E_ARG and call(wa_=False) == E.E_ARG

    def no_index(wa):
        wa.win_index = None

    def no_codes(wa):
        wa.table_codes = None
    assert call(edit=no_index) == E.E_ARG and call(edit=no_codes) == E.E_ARG
    assert call(q=off(qkv, 8)) == E.E_ARG and call(o=off(out, 2)) == E.E_ARG and call(tb=off(dev['table'], 2)) == E.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                          # nothing was launched
    # the recorded kind refuses the same way and names the entry point
    o = E.Op()
    o.kind, o.inp, o.out = E.OP_WINATTN_SOFTMAX, E.ptr(qkv), E.ptr(out)
    o.i0, o.i1, o.i2, o.i3 = cs['B'], cs['T'], cs['heads'], 32
    o.wa = _wa(E, cs, dict(SCALES, qact2=0.5), dev)
    o.lin.w_codes = E.ptr(dev['table'])
    assert L.p2v_run_ops(C.byref(o), 1, st) == E.E_UNSUPPORTED
    o.wa = _wa(E, cs, SCALES, dev)
    o.lin.w_codes = None
    assert L.p2v_run_ops(C.byref(o), 1, st) == E.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    o.lin.w_codes = E.ptr(dev['table'])
    assert L.p2v_run_ops(C.byref(o), 1, st) == 0 and call() == 0
    torch.cuda.synchronize()
    want, _, _ = _reference(cs, SCALES, table)
    assert torch.equal(out[:want.numel()].cpu().long().reshape(want.shape), want)


# ---- 2. the plans -------------------------------------------------------------------------------------------------------------------------
FACTORIES = {'w7': ('swin_micro_patch4_window7_56', 56), 'w12': ('swin_micro_patch4_window12_96', 96)}


@pytest.fixture(scope='module')
def world(dva, E):
    """per geometry: the micro model calibrated under Config(True, False) on the GPU with its plan, two images, the bit lists (8, 4, three
    mixed ones of _swin_bits_ref.bit_lists) and the helper's logits for each, computed once"""
    w = {}
    for tag, (factory, img) in FACTORIES.items():
        m, x = R.micro_swin(dva, factory, img, 3)
        L = m.bit_config_length()
        lists = [8, 4] + RB.bit_lists(L)[2:5]
        want = [R.quant_forward(pytest.MonkeyPatch, m.arch, m.state_dict(), m.export_calib(), x[:2], bl) if isinstance(bl, int) else
                R.mixed_forward(pytest.MonkeyPatch, m, x[:2], bl) for bl in lists]
        m.cuda()
        plan = m.freeze('cuda', bits=8)
        assert plan.int_softmax is False
        w[tag] = dict(m=m, x=x.cuda(), plan=plan, L=L, lists=lists, want=want, factory=factory, img=img)
    return w


def _attention_kinds(E, plan):
    kinds = [int(r['ops'][i].kind) for r in plan._recorded.values() for i in range(r['n'])]
    return kinds.count(E.OP_WINATTN), kinds.count(E.OP_WINATTN_SOFTMAX)


@pytest.mark.parametrize('tag', sorted(FACTORIES))
def test_plan_logits_equal_the_helper(E, world, tag):
    w = world[tag]
    m, x = w['m'], w['x'][:2]
    with torch.no_grad():
        for bl, want in zip(w['lists'], w['want']):
            got = m(x, bits=bl).cpu()
            assert torch.equal(got, want), (tag, bl, float((got - want).abs().max()))
    assert m._plan is w['plan']
    assert len({t.numpy().tobytes() for t in w['want']}) == len(w['want'])          # the lists are told apart
    old, new = _attention_kinds(E, w['plan'])
    assert old == 0 and new > 0 and new % sum(m.arch['depths']) == 0
    assert not torch.equal(w['want'][0], RB.uniform_oracle(m, x.cpu(), 8))            # and the configuration from the default one
    m(x, bits=8)


@pytest.mark.parametrize('tag', sorted(FACTORIES))
def test_uint8_sliced_and_profile(dva, E, world, tag):
    from diff_vit_amd import data
    w = world[tag]
    m, plan, img = w['m'], w['plan'], w['img']
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u8 = dva.synth.images_uint8(7, 2, img)
    bl = w['lists'][3]
    with torch.no_grad():
        for bits in (8, bl):
            assert torch.equal(m.forward_uint8(u8.cuda(), bits, mean, std, 'NHWC'), m(data.normalize_uint8(u8, mean, std, 'NHWC').cuda(), bits=bits))
        m(w['x'], bits=8)
        assert torch.equal(plan.forward(w['x'][:2]).cpu(), w['want'][0])
        xs = dva.synth.images(23, 48, img).cuda()             # 48 >= 16 * 3: three slices on three streams
        single = plan.forward(xs, n_streams=1)
        assert torch.equal(plan.forward(xs, n_streams=3), single) and torch.equal(plan.forward(xs, n_streams=3), single)
        assert torch.equal(plan.forward(xs, n_streams=3, slices=[20, 15, 13], bit_config=bl), plan.forward(xs, n_streams=1, bit_config=bl))
        assert torch.equal(single[:2].cpu(), plan.forward(xs[:2]).cpu())
        names = [k for k, _, _ in plan.profile(w['x'][:2])]
    assert 'window_softmax_attention' in names and 'window_attention' not in names
    assert _attention_kinds(E, plan)[0] == 0


@pytest.mark.parametrize('tag', sorted(FACTORIES))
def test_taps_and_ddv(dva, E, world, tag):
    """forward_linear_taps and forward_ddv (default stages) of the plan that has served the lists = those of a fresh plan, and their logits
    are the untapped ones; the attention stages are refused: the probabilities are not codes"""
    w = world[tag]
    m, plan, x = w['m'], w['plan'], w['x']
    x4 = torch.cat([x[:2], x[:2] + 0.01])
    fresh_m, _ = R.micro_swin(dva, w['factory'], w['img'], 3)
    fresh = fresh_m.cuda().freeze('cuda', bits=8)
    with torch.no_grad():
        m(x, bits=8)
        lg, names, sums = plan.forward_ddv(x4, with_linear=True)
        lg2, names2, sums2 = fresh.forward_ddv(x4, with_linear=True)
        assert names == names2 == dva.ddv.swin_stage_names(m.arch['depths'], True) and torch.equal(lg, lg2) and torch.equal(sums, sums2)
        assert torch.equal(lg, plan.forward(x4)) and torch.equal(lg[:2].cpu(), w['want'][0])
        out, taps = plan.forward_linear_taps(x)
        out2, taps2 = fresh.forward_linear_taps(x)
        assert torch.equal(out, out2) and torch.equal(out, plan.forward(x)) and len(taps) == len(taps2) == w['L']
        assert all(torch.equal(a, b) for a, b in zip(taps, taps2))
        t = {}
        assert torch.equal(plan.forward(x, taps=t), out) and len(t) > 0
        with pytest.raises(NotImplementedError):
            plan.forward_ddv(x4, attention=True)
        with pytest.raises(NotImplementedError):
            dva.ddv.compute_ddv(m, x[:2], x[:2] + 0.01, 8, attention=True)
        d = dva.ddv.compute_ddv(m, x[:2], x[:2] + 0.01, 8)
        assert list(d) == names
    assert _attention_kinds(E, plan)[0] == 0 and _attention_kinds(E, fresh)[0] == 0


def test_plan_refuses_a_qact2_scale_above_a_quarter(dva, world):
    """where the plan is created, naming the layer; the scale 2^-2 itself is accepted"""
    m = world['w7']['m']
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    name = 'layers.1.blocks.1.attn.qact2'
    calib = dict(m.export_calib())
    calib[name] = torch.tensor([0.5])
    with pytest.raises(NotImplementedError, match=name.replace('.', r'\.')):
        dva.SwinPlan(m.arch, sd, calib, device='cuda', int_softmax=False)
    calib[name] = torch.tensor([0.25])
    assert dva.SwinPlan(m.arch, sd, calib, device='cuda', int_softmax=False).int_softmax is False


def test_default_path_did_not_move(dva, E, world):
    """a plan of the (True, True) model built AFTER the float-softmax plans, in the same process: logits byte-identical to the oracle"""
    assert all(w['plan'].int_softmax is False for w in world.values())
    for factory, img in FACTORIES.values():
        m, x = RB.micro_swin(dva, factory, img, 2)
        want8, want4 = RB.uniform_oracle(m, x, 8), RB.uniform_oracle(m, x, 4)
        m.cuda()
        with torch.no_grad():
            assert torch.equal(m(x.cuda(), bits=8).cpu(), want8) and torch.equal(m(x.cuda(), bits=4).cpu(), want4)
        assert m._plan.int_softmax is True
        old, new = _attention_kinds(E, m._plan)
        assert new == 0 and old > 0


def test_large_micro_under_float_softmax(dva, E):
    """Swin-L widths (768 -> 3072 -> 1536 channels, 24 / 48 heads): the 3072-channel integer merge norm and the new op in one plan"""
    from test_swin_large import LARGE_MICRO
    m, x = R.micro_swin(dva, 'swin_large_patch4_window12_384', 32, 3, **LARGE_MICRO)
    assert m.layers[0].downsample.norm.weight.shape == (3072,)
    want = R.quant_forward(pytest.MonkeyPatch, m.arch, m.state_dict(), m.export_calib(), x, 8)
    m.cuda()
    with torch.no_grad():
        got = m(x.cuda(), bits=8).cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    old, new = _attention_kinds(E, m._plan)
    assert old == 0 and new == 2
