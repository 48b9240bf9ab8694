"""GPU: the lean LayerNorm phase of the fused LayerNorm + GEMM kernel (k_ln_gemm2 forms 3 / 4, "ln_gemm_lean" = 1) against the general form
("ln_gemm_lean" = 0), against p2v_int_layernorm + p2v_gemm_i8, and against the oracle's LayerNorm / qgemm restatement, bit for bit.  The
lean form is what a launch with pre-folded constants (p2v_ln_prefold), C = 64 * KT and no LayerNorm output selects; W4 = packed int4 weights
(p2v_linear.packed4 = 1: fragment-order copy for the fused kernels, packed tiles for the separate GEMM)."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


class lean:
    """the "ln_gemm_lean" switch for the duration of a block (tests/_tuning.py does not know it), restored to 1 on the way out"""

    def __init__(self, L, v):
        self.L, self.v = L, v

    def __enter__(self):
        assert self.L.p2v_set_tuning(b'ln_gemm_lean', self.v) == 0

    def __exit__(self, *exc):
        assert self.L.p2v_set_tuning(b'ln_gemm_lean', 1) == 0


def _codes(S, seed, name, shape, std):
    return torch.clamp(torch.round(S.normal(seed, name, shape, std)), -128, 127)


def _layer(dva, seed, C_, N, kind, pm_one, in_scale=None, w4=False):
    """constants of one LayerNorm + linear layer on the device, the LayerNorm constants pre-folded"""
    E, S = dva.engine, dva.synth
    tag = 'lean%d_%d' % (C_, N)
    if in_scale is None:
        in_scale = 0.0123 * 2.0 ** torch.floor(S.uniform(seed, tag + 'm', (C_,), 0, 3.99))
    gamma = S.uniform(seed, tag + 'g', (C_,), 0.5, 1.5) * torch.sign(S.uniform(seed, tag + 'gs', (C_,), -1, 1) + 1e-3)
    beta = S.normal(seed, tag + 'b', (C_,), 0.3)
    cs = 2.0 ** torch.floor(S.uniform(seed, tag + 'c', (C_,), -2, 2.99))
    cs_next = cs if pm_one else 2.0 ** torch.floor(S.uniform(seed, tag + 'd', (C_,), -2, 2.99))
    s_a = 2.0 ** -4
    out_scale = s_a * cs
    s1 = in_scale.min()
    k_pad = (C_ + 63) // 64 * 64
    w = _codes(S, seed, tag + 'w', (N, C_), 30.0)
    s_w = torch.full((N,), 2.0 ** -7); s_w[::3] = 2.0 ** -6
    if w4:                                                   # 4-bit codes on a scale 8 times as large
        w = torch.clamp(torch.round(w / 12.0), -8, 7)
        s_w = s_w * 8.0
    bias = S.normal(seed, tag + 'bb', (N,), 0.4)
    n_pad = (N + 127) // 128 * 128
    wp = torch.zeros(n_pad, k_pad, dtype=torch.int8); wp[:N, :C_] = w.to(torch.int8)
    csl = torch.zeros(n_pad); csl[:N] = s_a * s_w
    bp = torch.zeros(n_pad); bp[:N] = bias
    dev = [t.contiguous().cuda() for t in (torch.round(in_scale / s1), gamma, beta, 1.0 / out_scale, out_scale / cs_next / s_a, wp, csl, bp)]
    lnp = E.Ln(float(s1), *[E.ptr(t) for t in dev[:5]])
    L = E.lib()
    nb = L.p2v_ln_prefold_bytes(C_)
    buf = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
    E.check(L.p2v_ln_prefold(C.byref(lnp), C_, E.ptr(buf), nb))
    assert lnp.pre.gm and lnp.pre.pot == 1 and lnp.pre.pm_one == (1 if pm_one else 0)
    if w4:
        dev[5] = E.pack_int4_tiles(wp).cuda()
        wfrag = E.fragment_order_packed4(wp).cuda()
    else:
        wfrag = E.fragment_order(wp).cuda()
    lin = E.Linear(E.ptr(dev[5]), E.ptr(dev[6]), E.ptr(dev[7]), E.ptr(wfrag), 1 if w4 else 0)
    epi = E.Epilogue()
    s_out = 2.0 ** -3 if kind == 'requant' else 2.0 ** -5
    epi.inv_s_out = 1.0 / s_out
    if kind == 'gelu':
        epi.gelu = E.gelu_table(1.0 / s_out, 'cuda')
    return dict(C=C_, N=N, kind=kind, k_pad=k_pad, ek=E.EPI_REQUANT if kind == 'requant' else E.EPI_GELU, lnp=lnp, lin=lin, epi=epi, keep=(dev, buf, wfrag),
                in_scale=in_scale, gamma=gamma, beta=beta, out_scale=out_scale, cs_next=cs_next, s_a=s_a, s1=s1, w=w, s_w=s_w, bias=bias, s_out=s_out)


def _fused(dva, ly, x, want_ln=False):
    E, L = dva.engine, dva.engine.lib()
    M = x.shape[0]
    out = torch.full((M, ly['N']), 77, dtype=torch.int8, device='cuda')
    ln = torch.full((M, ly['C']), 99, dtype=torch.int8, device='cuda') if want_ln else None
    E.check(L.p2v_ln_gemm_i8(ly['ek'], E.ptr(x), ly['C'], M, ly['C'], C.byref(ly['lnp']), ly['N'], C.byref(ly['lin']), C.byref(ly['epi']),
                             E.ptr(out), ly['N'], E.ptr(ln) if want_ln else None, E.stream_ptr()))
    torch.cuda.synchronize()
    return out, ln


def _separate(dva, ly, x):
    E, L = dva.engine, dva.engine.lib()
    M = x.shape[0]
    ln = torch.zeros(M, ly['k_pad'], dtype=torch.int8, device='cuda')
    E.check(L.p2v_int_layernorm(E.ptr(x), ly['C'], M, ly['C'], C.byref(ly['lnp']), E.ptr(ln), ly['k_pad'], E.stream_ptr()))
    out = torch.zeros(M, ly['N'], dtype=torch.int8, device='cuda')
    E.check(L.p2v_gemm_i8(ly['ek'], E.ptr(ln), ly['k_pad'], M, ly['k_pad'], ly['N'], C.byref(ly['lin']), C.byref(ly['epi']), E.ptr(out), ly['N'], None,
                          E.stream_ptr()))
    torch.cuda.synchronize()
    return out, ln[:, :ly['C']]


def _oracle(oracle, ly, codes):
    ln = oracle.int_layernorm((codes * ly['in_scale'].reshape(1, -1)).unsqueeze(0), ly['in_scale'], ly['gamma'], ly['beta'], ly['out_scale'])
    q0 = torch.clamp(torch.round((ln * ly['out_scale'].reshape(1, 1, -1)) / ly['cs_next'].reshape(1, 1, -1) / ly['s_a']), -128, 127)[0]
    y = oracle.qgemm(q0, torch.tensor(ly['s_a']), ly['w'], ly['s_w'], ly['bias'])
    v = oracle.gelu_rn(y) if ly['kind'] == 'gelu' else y
    return torch.clamp(torch.round(v / ly['s_out']), -128, 127)


def _check(dva, oracle, ly, codes):
    """lean == general fused == separate == oracle for the rows `codes` and every prefix in ROWS"""
    L = dva.engine.lib()
    x = codes.to(torch.int8).contiguous().cuda()
    ref = _oracle(oracle, ly, codes)
    sep, _ = _separate(dva, ly, x)
    assert torch.equal(sep.cpu().float(), ref), int((sep.cpu().float() != ref).sum())
    for M in sorted(set(ROWS + (codes.shape[0],))):
        if M > codes.shape[0]:
            continue
        xm = x[:M].contiguous()
        with lean(L, 0):
            old, _ = _fused(dva, ly, xm)
        new, _ = _fused(dva, ly, xm)
        assert torch.equal(old, sep[:M]), (M, int((old != sep[:M]).sum()))
        assert torch.equal(new, old), (M, int((new != old).sum()))


ROWS = (1, 2, 63, 64, 65, 130)


@pytest.mark.parametrize('w4', (False, True))
@pytest.mark.parametrize('C_', (64, 192, 384))
@pytest.mark.parametrize('N,kind,pm_one', [(128, 'requant', True), (384, 'gelu', False), (384, 'requant', False), (128, 'gelu', True)])
def test_lean_vs_general_separate_and_oracle(dva, oracle, C_, N, kind, pm_one, w4):
    ly = _layer(dva, 17, C_, N, kind, pm_one, w4=w4)
    codes = _codes(dva.synth, 17, 'x%d_%d' % (C_, N), (130, C_), 35.0)
    codes[0] = torch.round(codes[0] * 0.03)
    _check(dva, oracle, ly, codes)


@pytest.mark.parametrize('C_,with_out', [(352, False), (384, True), (192, True)])
def test_other_launches_keep_the_general_kernel(dva, oracle, C_, with_out):
    """C that is no whole number of k-tiles, and a launch with the LayerNorm output: the general form runs whatever the switch says.  The
    launcher reports no selection, so the test sees it through the results only: the lean phase assumes whole k-tiles (at C = 352 its last
    32 channels would be normalised as data) and never writes the LayerNorm codes, which must be the separate path's here."""
    ly = _layer(dva, 19, C_, 128, 'requant', True)
    codes = _codes(dva.synth, 19, 'y%d' % C_, (65, C_), 35.0)
    x = codes.to(torch.int8).contiguous().cuda()
    sep, ln_sep = _separate(dva, ly, x)
    out, ln = _fused(dva, ly, x, want_ln=with_out)
    assert torch.equal(out, sep)
    if with_out:
        assert torch.equal(ln, ln_sep)
    assert torch.equal(out.cpu().float(), _oracle(oracle, ly, codes))


def _fast_predicate(ly, codes):
    """ln_scalars' `fast` per row, in its fp32 operation order"""
    f = np.float32
    pre = ly['lnp'].pre
    mask = torch.round(ly['in_scale'] / ly['s1']).double()
    xq = codes.double() * mask
    S1f, S2f = xq.sum(1).numpy().astype(f), (xq * xq).sum(1).numpy().astype(f)
    s1, Cf = f(float(ly['s1'])), f(ly['C'])
    with np.errstate(all='ignore'):
        stdv = (s1 / Cf) * np.sqrt(Cf * S2f - S1f * S1f)
        rs = s1 / stdv
        mos = ((S1f / Cf) * s1) / stdv
        amin = rs * f(pre.gmin)
        tlim = ((((amin.view(np.uint32) >> 23) & 255) + 15) << 23).astype(np.uint32).view(f)
        return (amin >= f(2.0 ** -24)) & (rs * f(pre.gmax) < f(256)) & ((f(pre.bmax) + np.abs(mos) * f(pre.gmax)) * f(1.01) < tlim)


@pytest.mark.parametrize('kind,pm_one', [('requant', True), ('gelu', False)])
def test_rows_that_leave_the_fast_chain_inside_a_workgroup(dva, oracle, kind, pm_one):
    """rows of very small (never zero) variance make rs * gmax >= 256: the generic chain, next to fast rows of the same pair, wave and
    workgroup"""
    C_ = 384
    ly = _layer(dva, 23, C_, 128, kind, pm_one)
    codes = _codes(dva.synth, 23, 'z', (130, C_), 35.0)
    ch = int(torch.argmin(ly['in_scale']))                       # a channel of mask 1
    for i, r in enumerate((0, 3, 10, 11, 21, 40, 47, 62, 129)):
        codes[r] = 0.0
        codes[r, ch] = (-1.0, 1.0, 2.0, -2.0)[i % 4]               # x_q = 0 but for one value: std = |value| * sqrt(C - 1) / C of a step
    fast = _fast_predicate(ly, codes)
    wg0 = fast[:64]
    assert wg0.any() and not wg0.all()
    assert any(wg0[2 * k] != wg0[2 * k + 1] for k in range(32))            # both outcomes in one row pair
    assert any(not wg0[2 * k] and not wg0[2 * k + 1] for k in range(32))   # ... and a pair that leaves the fast chain with both rows
    assert not fast[129] and fast[64:128].any()
    _check(dva, oracle, ly, codes)


def test_extreme_codes_at_the_largest_mask(dva, oracle):
    """every code +-127 / -128 on PTF mask 8: the largest sums of squares the 32-bit reduction sees at C = 384"""
    C_ = 384
    in_scale = torch.full((C_,), 0.0123 * 8.0); in_scale[5] = 0.0123
    ly = _layer(dva, 29, C_, 128, 'requant', True, in_scale=in_scale)
    u = dva.synth.uniform(29, 'e', (66, C_), 0, 3)
    codes = torch.where(u < 1, torch.tensor(-128.0), torch.where(u < 2, torch.tensor(127.0), torch.tensor(-127.0)))
    codes[1] = 127.0; codes[1, ::2] = -128.0
    assert float(((codes * torch.round(in_scale / in_scale.min())) ** 2).sum(1).max()) > 2.0 ** 28
    _check(dva, oracle, ly, codes)


def test_whole_model_micro(dva, micro):
    L = dva.engine.lib()
    arch = micro['arch']
    plan = dva.FrozenPlan(arch, micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    n = 4 * arch['depth'] + 2
    for bits in ([8] * n, [4] * n):
        on = plan.forward(x, bits).clone()
        with lean(L, 0):
            off = plan.forward(x, bits).clone()
        torch.cuda.synchronize()
        assert torch.equal(on, off), bits[0]


def test_whole_model_deit_small(dva):
    from diff_vit_amd import data as D
    L = dva.engine.lib()
    arch = dva.synth.ARCHS['deit_small']
    mean, std, _ = D.MODEL_STATS['deit']
    m = dva.VisionTransformer(img_size=arch['img_size'], patch_size=arch['patch_size'], embed_dim=arch['embed_dim'], depth=arch['depth'],
                              num_heads=arch['num_heads'], num_classes=arch['num_classes'], mlp_ratio=arch['mlp_ratio'], qkv_bias=True,
                              norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(arch, 11), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, D.normalize_uint8(dva.synth.images_uint8(111, 8, arch['img_size']), mean, std).cuda())
    x = D.normalize_uint8(dva.synth.images_uint8(21, 2, arch['img_size']), mean, std).cuda()
    n = 4 * arch['depth'] + 2
    for bits in ([8] * n, [4] * n):
        with torch.no_grad():
            on = m(x, bits)[0].clone()                      # (the first quantized forward freezes the plan)
            assert getattr(m, '_plan', None) is not None
            with lean(L, 0):
                off = m(x, bits)[0].clone()
        torch.cuda.synchronize()
        assert torch.equal(on, off), bits[0]
