"""GPU: the Swin model diff on the engine - the mid-code output of the RESID epilogue, the P2V_OP_COS / P2V_OP_COS_COMBINE / P2V_OP_GEMM_F32
records of p2v_run_ops, SwinPlan.forward_ddv / forward_linear_taps against oracle values, and the module surface (compute_ddv,
get_activations / compute_cka, hooks on a fused Swin, the command line).

Tolerances: int8 stages with one scale are exact integer sums, compared bit for bit; per-channel stages sum at most
C <= 4096 fp64 terms in another order than the restatement, 2 C 2^-53 < 1e-12 relative; fp32 stages sum up to ~10^6 fp64 products in
another order, 1e-9 relative.  A dot product a.b is measured against sqrt(a.a b.b), the two squares against themselves."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from _arena import Arena, twice
from _tuning import tuning
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _q8(v):
    return torch.clamp(torch.round(v), -128, 127)


def _close(got, want, tol, what):
    """[n, 3] sums: a.a and b.b relative to themselves, a.b relative to sqrt(a.a b.b)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.isfinite(got).all(), what
    root = np.sqrt(want[:, 1] * want[:, 2])
    assert np.all(np.abs(got[:, 1] - want[:, 1]) <= tol * want[:, 1]), (what, 'aa')
    assert np.all(np.abs(got[:, 2] - want[:, 2]) <= tol * want[:, 2]), (what, 'bb')
    assert np.all(np.abs(got[:, 0] - want[:, 0]) <= tol * root), (what, 'ab')


# --------------------------------------------------------------------------------------------------
# 1. RESID mid codes, operator level
# --------------------------------------------------------------------------------------------------
MS = (1, 33, 129, 257)


@functools.lru_cache(maxsize=None)
def _resid_case(N, K):
    """a layer whose first quotient covers the whole code range and its clamp edges: y / s_mid has a spread of ~90 codes (both clamps
    are hit), and in row 0 (no activations) the bias puts columns 0 .. 5 exactly on +-127.5, +-128.5 and +-126.5 codes of a dyadic
    s_mid (ties and the clamp boundaries); everywhere else s_mid, s_res, s_next are non-power-of-two PTF scales (base x 2^k)"""
    import p2vit_oracle as O
    gen = _gen(100 * N + K)
    rows = max(MS)
    x = torch.clamp(torch.round(torch.randn(rows, K, generator=gen) * 40), -128, 127)
    x[0] = 0
    w = torch.clamp(torch.round(torch.randn(N, K, generator=gen) * 30), -128, 127)
    ptf = lambda base: base * 2.0 ** torch.randint(0, 4, (N,), generator=gen).float()
    s_mid, s_res, s_next = ptf(0.0131), ptf(0.0173), ptf(0.0209)
    s_mid[:6] = 2.0 ** -5
    s_x, s_w = 2.0 ** -6, torch.full((N,), 2.0 ** -7)
    # acc ~ 40 * 30 * sqrt(K) -> y = acc * 2^-13 ~ 1.2 ... 2: |y / s_mid| reaches a few hundred codes where s_mid is small
    bias = torch.randn(N, generator=gen) * 0.2
    bias[:6] = torch.tensor([127.5, -128.5, 126.5, -127.5, 128.5, -126.5]) * 2.0 ** -5
    res = torch.clamp(torch.round(torch.randn(rows, N, generator=gen) * 50), -128, 127)
    y = O.qgemm(x, torch.tensor(s_x), w, s_w, bias)
    q3 = _q8(y / s_mid)
    out = _q8((res * s_res + q3 * s_mid) / s_next)
    return dict(x=x, w=w, s_x=s_x, s_w=s_w, bias=bias, s_mid=s_mid, s_res=s_res, s_next=s_next, res=res, q3=q3, out=out)


@pytest.mark.parametrize('N', [96, 128, 272])
@pytest.mark.parametrize('K', [64, 192])
def test_resid_mid_codes_operator(dva, N, K):
    """p2v_gemm_i8(RESID, out_codes): the mid codes equal q8(qgemm(...) / s_mid) of the oracle, `out` equals the launch without the tap byte
    for byte, and in sentinel arenas (ldo = N + 16) the columns [N, ldo) and everything around both outputs stay untouched - for both
    tile heights and with / without the pre-folded table"""
    E = dva.engine
    L = E.lib()
    c = _resid_case(N, K)
    assert float(c['q3'].max()) == 127 and float(c['q3'].min()) == -128 and 0.02 < float((c['q3'].abs() >= 127).float().mean()) < 0.6
    assert c['q3'][0, :6].tolist() == [127, -128, 126, -128, 127, -126]            # ties to even, then the clamp
    n_pad = (N + 127) // 128 * 128
    wp = torch.zeros(n_pad, K, dtype=torch.int8)
    wp[:N] = c['w'].to(torch.int8)
    pad = lambda v: torch.cat([v.float(), torch.zeros(n_pad - N)]).cuda()
    d = dict(w=wp.cuda(), cs=pad(c['s_x'] * c['s_w']), b=pad(c['bias']), s_mid=c['s_mid'].cuda(), s_res=c['s_res'].cuda(), s_next=c['s_next'].cuda())
    lin = E.Linear(E.ptr(d['w']), E.ptr(d['cs']), E.ptr(d['b']), None, 0)
    epi0 = E.Epilogue()
    epi0.s_mid, epi0.s_res, epi0.s_next = E.ptr(d['s_mid']), E.ptr(d['s_res']), E.ptr(d['s_next'])
    nb = L.p2v_resid_prefold_bytes(N)
    tab = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
    usable = C.c_int(-1)
    E.check(L.p2v_resid_prefold(C.byref(lin), C.byref(epi0), N, E.ptr(tab), nb, C.byref(usable), None))
    ldo = N + 16

    def run(sentinel, M, tap, with_tab):
        a = Arena(M, K, K, torch.int8, sentinel, init=c['x'][:M])
        res = Arena(M, N, ldo, torch.int8, sentinel, init=c['res'][:M])
        out = Arena(M, N, ldo, torch.int8, sentinel)
        mid = Arena(M, N, ldo, torch.int8, sentinel) if tap else None
        epi = E.Epilogue()
        epi.s_mid, epi.s_res, epi.s_next, epi.residual = epi0.s_mid, epi0.s_res, epi0.s_next, res.ptr
        if with_tab:
            epi.resid_tab = E.ptr(tab)
        E.check(L.p2v_gemm_i8(E.EPI_RESID, a.ptr, K, M, K, N, C.byref(lin), C.byref(epi), out.ptr, ldo, mid.ptr if tap else None, E.stream_ptr()))
        torch.cuda.synchronize()
        what = (M, N, K, tap, with_tab)
        a.read(('x', what)), res.read(('residual', what))
        r = dict(out=out.read(('out', what)))
        if tap:
            r['mid'] = mid.read(('mid', what))
        return r

    for tile in (128, 256):
        for pre in (0, 1):
            with tuning(L, gemm_tile=tile, resid_pre=pre):
                for M in MS:
                    with_tab = bool(usable.value)
                    plain = twice(lambda s: run(s, M, False, with_tab))
                    tapped = twice(lambda s: run(s, M, True, with_tab))
                    key = (tile, pre, M)
                    assert torch.equal(tapped['mid'].float(), c['q3'][:M]), (key, int((tapped['mid'].float() != c['q3'][:M]).sum()))
                    assert torch.equal(tapped['out'], plain['out']), key
                    assert torch.equal(plain['out'].float(), c['out'][:M]), key
    # the refusals of the tap: misaligned destination, packed int4 weights
    one = C.c_void_p(256)
    epi0.residual = one
    assert L.p2v_gemm_i8(E.EPI_RESID, one, K, 1, K, N, C.byref(lin), C.byref(epi0), one, ldo, C.c_void_p(264), None) == E.E_ARG
    lin4 = E.Linear(one, one, one, None, 1)
    assert L.p2v_gemm_i8(E.EPI_RESID, one, K, 1, K, N, C.byref(lin4), C.byref(epi0), one, ldo, one, None) == E.E_UNSUPPORTED


# --------------------------------------------------------------------------------------------------
# 2. P2V_OP_COS / P2V_OP_COS_COMBINE through p2v_run_ops
# --------------------------------------------------------------------------------------------------
COS_SHAPES = ((5, 96, 128), (1, 64, 64), (49, 1024, 1024))          # rows, cols, row stride (elements)


def _cos_op(E, n, ptr, rows, cols, stride, dtype, scale=None):
    o = E.Op()
    o.kind, o.inp = E.OP_COS, ptr
    o.i0, o.i1, o.M, o.N, o.lda = n, dtype, rows, cols, stride
    o.i2, o.i3 = rows * stride, 0
    o.lin.colscale = scale
    esz = 1 if dtype == E.COS_I8 else 4
    lay = E.CosLayer(ptr, C.c_void_p(ptr.value + n * rows * stride * esz), scale, rows * stride, stride, rows, cols, dtype)
    return o, lay


@pytest.mark.parametrize('n', [1, 3])
def test_cos_records_through_run_ops(dva, n):
    """hand-built records: every shape as int8 without scale (bit-equal to pair_cosine_cpu), with per-channel scales (1e-12) and as fp32
    (1e-9); padding between the rows holds 0x7f and is never read; two stages share one buffer that a P2V_OP_MERGE record overwrites
    between them; in arenas only the partial and sum slots are written"""
    E = dva.engine
    L = E.lib()
    gen = _gen(7 + n)
    host, plans = [], []                      # plans: (arena, a, b, scale) per stage, in record order
    ops, lays = [], []
    for rows, cols, stride in COS_SHAPES:
        for kind in ('i8', 'i8s', 'f32'):
            dt = torch.float32 if kind == 'f32' else torch.int8
            v = torch.randn(2 * n, rows, cols, generator=gen) * 30
            v = v if kind == 'f32' else _q8(v)
            ar = Arena(2 * n * rows, cols, stride, dt, 0x7f, init=v.reshape(-1, cols))
            sc = (torch.rand(cols, generator=gen) + 0.05) * 2.0 ** -4 if kind == 'i8s' else None
            scd = sc.cuda() if sc is not None else None
            o, lay = _cos_op(E, n, ar.ptr, rows, cols, stride, E.COS_F32 if kind == 'f32' else E.COS_I8, E.ptr(scd))
            ops.append(o), lays.append(lay)
            host.append((ar, scd))
            plans.append((v[:n] if kind == 'f32' else v[:n].to(torch.int8), v[n:] if kind == 'f32' else v[n:].to(torch.int8), sc))
    # two stages on one buffer: [2n][4][64] = the output of a patch-merge gather of [2n][4 x 4][16]
    first = _q8(torch.randn(2 * n, 4, 64, generator=gen) * 40)
    src = _q8(torch.randn(2 * n, 16, 16, generator=gen) * 40)
    shared = Arena(2 * n * 4, 64, 64, torch.int8, 0x7f, init=first.reshape(-1, 64))
    srcd = src.to(torch.int8).cuda()
    o1, l1 = _cos_op(E, n, shared.ptr, 4, 64, 64, E.COS_I8)
    om = E.Op()
    om.kind, om.inp, om.out = E.OP_MERGE, E.ptr(srcd), shared.ptr
    om.i0, om.i1, om.i2, om.i3 = 2 * n, 4, 4, 16
    o2, l2 = _cos_op(E, n, shared.ptr, 4, 64, 64, E.COS_I8)
    import swin_oracle as SO
    merged = SO.patch_merge_gather(src, 4, 4)
    ops += [o1, om, o2]
    lays += [l1, l2]
    plans += [(first[:n].to(torch.int8), first[n:].to(torch.int8), None), (merged[:n].to(torch.int8), merged[n:].to(torch.int8), None)]
    stage_ops = [o for o in ops if o.kind == E.OP_COS]
    S = len(stage_ops)
    dbytes = L.p2v_cos_stage_desc_bytes()
    hostd = (C.c_char * (dbytes * S))()
    items = L.p2v_cos_stage_descs((E.CosLayer * S)(*lays), S, n, hostd)
    assert items >= S * n
    descs = torch.frombuffer(bytearray(hostd.raw), dtype=torch.uint8).cuda()
    want = dva.ddv.pair_cosine_cpu([p[0] for p in plans], [p[1] for p in plans], [p[2] for p in plans]).numpy()

    def run(sentinel):
        parts = Arena(1, int(items) * 3, dtype=torch.int64, sentinel=sentinel)
        sums = Arena(S * n, 3, dtype=torch.float64, sentinel=sentinel)
        shared.dev[shared.start:shared.start + 2 * n * 4 * 64] = first.reshape(-1).to(torch.int8).cuda().view(torch.uint8)
        for k, o in enumerate(stage_ops):
            o.out = parts.ptr
            o.lin.w_codes = C.c_void_p(descs.data_ptr() + k * dbytes)
        oc = E.Op()
        oc.kind, oc.inp, oc.out = E.OP_COS_COMBINE, E.ptr(descs), sums.ptr
        oc.i0, oc.i1 = n, S
        oc.lin.w_codes = parts.ptr
        seq = ops + [oc]
        E.check(L.p2v_run_ops((E.Op * len(seq))(*seq), len(seq), E.stream_ptr()))
        torch.cuda.synchronize()
        parts.read('partials')
        for ar, _ in host:
            ar.read('input')
        return dict(sums=sums.read('sums').reshape(S, n, 3))

    got = twice(run)['sums'].numpy()
    assert np.isfinite(got).all()
    for k, (a, b, sc) in enumerate(plans):
        if a.dtype == torch.int8 and sc is None:
            assert np.array_equal(got[k], want[k]), k
        else:
            _close(got[k], want[k], 1e-12 if sc is not None else 1e-9, k)
    assert not np.array_equal(got[-1], got[-2])                 # the shared buffer was read before and after the overwrite


def test_gemm_f32_record_and_refusals(dva):
    """P2V_OP_GEMM_F32 == qgemm of the oracle bit for bit (one fp32 rounding), the public p2v_gemm_i8 refuses kind 7, kind 99 stays unknown"""
    import p2vit_oracle as O
    E = dva.engine
    L = E.lib()
    gen = _gen(3)
    M, K, N = 70, 128, 96
    x, w = _q8(torch.randn(M, K, generator=gen) * 40), _q8(torch.randn(N, K, generator=gen) * 30)
    bias = torch.randn(N, generator=gen)
    wp = torch.zeros(128, K, dtype=torch.int8)
    wp[:N] = w.to(torch.int8)
    pad = lambda v: torch.cat([v.float(), torch.zeros(128 - N)]).cuda()
    d = dict(w=wp.cuda(), cs=pad(torch.full((N,), 2.0 ** -12)), b=pad(bias), x=x.to(torch.int8).cuda())
    out = torch.zeros(M, N, dtype=torch.float32, device='cuda')
    o = E.Op()
    o.kind, o.inp, o.out = E.OP_GEMM_F32, E.ptr(d['x']), E.ptr(out)
    o.M, o.K, o.N, o.lda, o.ldo = M, K, N, K, N
    o.lin = E.Linear(E.ptr(d['w']), E.ptr(d['cs']), E.ptr(d['b']), None, 0)
    E.check(L.p2v_run_ops((E.Op * 1)(o), 1, E.stream_ptr()))
    want = O.qgemm(x, torch.tensor(2.0 ** -6), w, torch.full((N,), 2.0 ** -6), bias)
    assert torch.equal(out.cpu(), want)
    one = C.c_void_p(256)
    assert L.p2v_gemm_i8(7, one, 64, 1, 64, 16, C.byref(o.lin), C.byref(E.Epilogue()), one, 16, None, None) == E.E_ARG
    o.kind = 99
    assert L.p2v_run_ops((E.Op * 1)(o), 1, None) == E.E_ARG and b'unknown op kind' in L.p2v_last_error()


# --------------------------------------------------------------------------------------------------
# 3 - 5. SwinPlan.forward_ddv against oracle values, every stage
# --------------------------------------------------------------------------------------------------
def _calibrated(dva, make, img, seed=5, **kw):
    m = make(cfg=dva.Config(True, True, 'minmax'), num_classes=10, **kw).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), seed))
    x = dva.synth.images(seed, 2, img)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x); m.model_close_calibrate()
        m.model_quant()
    return m


def _pairs(dva, n, img, seed=11):
    x = dva.synth.images(seed, n, img)
    xa = x + 0.25 * dva.synth.images(seed + 1, n, img)
    return x, xa


def oracle_stages(m, x, bits):
    """name -> (values [B, ...] of all B images, per-channel scale or None, is_fp32) for EVERY stage of ddv.swin_stage_names(depths, True).
    The stages OracleSwin.quant_forward taps come from it; attn.qact1 / attn.qact3 from window_attention_quant(taps=) on the tapped qact1
    (window order: a permutation of an image's tokens, which the sums of a stage with one scale do not see); qact3 from int_layernorm on
    the tapped qact2; mlp.qact2 from qgemm and q8; the linear stages from qgemm on the layer's input codes."""
    import p2vit_oracle as O
    import swin_oracle as SO
    a, c = m.arch, m.export_calib()
    W = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    bt = 'int%d' % bits
    taps = {}
    logits = SO.OracleSwin(a, W).quant_forward(x, c, bits, taps)
    B = x.shape[0]
    st = {}

    def lin(xc, s_x, name, bias=True):
        s_w = c[name][bt].reshape(-1)
        return O.qgemm(xc.float(), s_x, O.weight_codes(W[name + '.weight'], None, s_w, bits), s_w, W[name + '.bias'] if bias else None)

    P, g = a['patch_size'], a['img_size'] // a['patch_size']
    s_in = c['qact_input'].reshape(())
    patches = SO.q8(x, s_in).reshape(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, -1)
    st['patch_embed.proj'] = (lin(patches, s_in, 'patch_embed.proj').reshape(B, -1), None, True)
    for nm in ('patch_embed.qact_before_norm', 'patch_embed.qact', 'qact2', 'qact3'):
        st[nm] = (taps[nm].reshape(B, -1), None, False)
    H = g
    for li, depth in enumerate(a['depths']):
        Cc, heads, wsz = a['embed_dim'] * 2 ** li, a['num_heads'][li], min(a['window_size'], H)
        for bi in range(depth):
            p = 'layers.%d.blocks.%d.' % (li, bi)
            shift = 0 if (bi % 2 == 0 or H <= a['window_size']) else a['window_size'] // 2
            q1 = taps[p + 'qact1'].float()
            st[p + 'qact1'] = (q1.reshape(B, -1), None, False)
            s1 = c[p + 'qact1'].reshape(())
            st[p + 'attn.qkv'] = (lin(q1.reshape(-1, Cc), s1, p + 'attn.qkv').reshape(B, -1), None, True)
            idx = SO.window_index(H, H, wsz, shift)
            xw = q1[:, idx.reshape(-1)].reshape(B * idx.shape[0], wsz * wsz, Cc)
            cw = {k: c[p + 'attn.' + k] for k in ('qact1', 'qact_attn1', 'qact_table', 'qact2', 'qact3', 'qact4')}
            cw['qkv'], cw['proj'] = c[p + 'attn.qkv'][bt], c[p + 'attn.proj'][bt]
            Wa = {k: W[p + 'attn.' + k] for k in ('qkv.weight', 'qkv.bias', 'proj.weight', 'proj.bias', 'relative_position_bias_table')}
            wt = {}
            SO.window_attention_quant(xw, float(s1), Wa, cw, heads, wsz, mask=SO.shifted_window_mask(H, H, wsz, shift) if shift else None,
                                      taps=wt, bits=bits)
            st[p + 'attn.qact1'] = (wt['qact1'].reshape(B, -1), None, False)
            st[p + 'attn.qact3'] = (wt['qact3'].reshape(B, -1), None, False)
            s_a3 = c[p + 'attn.qact3'].reshape(())
            yw = lin(wt['qact3'].reshape(-1, Cc), s_a3, p + 'attn.proj')                    # window order -> natural token order
            nat = torch.zeros(B, H * H, Cc)
            nat[:, idx.reshape(-1)] = yw.reshape(B, -1, Cc)
            st[p + 'attn.proj'] = (nat.reshape(B, -1), None, True)
            st[p + 'attn.qact4'] = (taps[p + 'attn.qact4'].reshape(B, -1), None, False)
            s_b2 = c[p + 'qact2'].reshape(-1)
            x2 = taps[p + 'qact2'].float()
            st[p + 'qact2'] = (x2, s_b2, False)
            s3 = c[p + 'qact3'].reshape(())
            ln = O.int_layernorm(x2 * s_b2.reshape(1, 1, -1), s_b2, W[p + 'norm2.weight'], W[p + 'norm2.bias'], s3.reshape(1).expand(Cc))
            q3 = SO.q8(ln * s3, s3)
            st[p + 'qact3'] = (q3.reshape(B, -1), None, False)
            st[p + 'mlp.fc1'] = (lin(q3.reshape(-1, Cc), s3, p + 'mlp.fc1').reshape(B, -1), None, True)
            qm1 = taps[p + 'mlp.qact1'].float()
            st[p + 'mlp.qact1'] = (qm1.reshape(B, -1), None, False)
            s_m1 = c[p + 'mlp.qact1'].reshape(())
            y = lin(qm1.reshape(-1, qm1.shape[-1]), s_m1, p + 'mlp.fc2')
            st[p + 'mlp.fc2'] = (y.reshape(B, -1), None, True)
            st[p + 'mlp.qact2'] = (SO.q8(y, c[p + 'mlp.qact2'].reshape(())).reshape(B, -1), None, False)
            st[p + 'qact4'] = (taps[p + 'qact4'].float(), c[p + 'qact4'].reshape(-1), False)
        if li < len(a['depths']) - 1:
            p = 'layers.%d.downsample.' % li
            qd1 = taps[p + 'qact1'].float()
            st[p + 'qact1'] = (qd1.reshape(B, -1), None, False)
            st[p + 'reduction'] = (lin(qd1.reshape(-1, 4 * Cc), c[p + 'qact1'].reshape(()), p + 'reduction', bias=False).reshape(B, -1), None, True)
            st[p + 'qact2'] = (taps[p + 'qact2'].float(), c[p + 'qact2'].reshape(-1), False)
            H //= 2
    st['head'] = (lin(taps['qact3'].float(), c['qact3'].reshape(()), 'head'), None, True)
    st['act_out'] = (logits, None, True)
    return st, logits


def _check_forward_ddv(dva, m, n, bits):
    D = dva.ddv
    img = m.arch['img_size']
    x, xa = _pairs(dva, n, img)
    x2 = torch.cat((x, xa), 0)
    with torch.no_grad():
        st, ref = oracle_stages(m, x2, bits)
    m.cuda()
    with torch.no_grad():
        fwd = m(x2.cuda(), bits=bits).cpu()
        plan = m._plan
        for with_linear in (True, False):
            logits, names, sums = plan.forward_ddv(x2.cuda(), with_linear)
            torch.cuda.synchronize()
            assert names == D.swin_stage_names(m.arch['depths'], with_linear)
            blocks, merges = sum(m.arch['depths']), len(m.arch['depths']) - 1
            assert len(names) == 9 * blocks + 2 * merges + 5 + (4 * blocks + merges + 2 if with_linear else 0)
            assert torch.equal(logits.cpu(), fwd) and torch.equal(fwd, ref)
            sums = sums.cpu()
            assert tuple(sums.shape) == (len(names), n, 3) and bool(torch.isfinite(sums).all()) and bool((sums[..., 1:] > 0).all())
            for k, nm in enumerate(names):                       # EVERY stage
                v, sc, is_f = st[nm]
                if is_f:
                    want = D.pair_cosine_cpu([v[:n].float()], [v[n:].float()])[0]
                    _close(sums[k], want, 1e-9, (bits, nm))
                elif sc is None:
                    want = D.pair_cosine_cpu([v[:n].to(torch.int32)], [v[n:].to(torch.int32)])[0]
                    assert torch.equal(sums[k], want), (bits, nm)
                else:
                    want = D.pair_cosine_cpu([v[:n].to(torch.int32)], [v[n:].to(torch.int32)], [sc])[0]
                    _close(sums[k], want, 1e-12, (bits, nm))
    m.cpu()
    return len(names)


@functools.lru_cache(maxsize=None)
def _micro7():
    import diff_vit_amd as dva
    return _calibrated(dva, dva.swin.swin_micro_patch4_window7_56, 56)


@pytest.mark.parametrize('bits', [8, 4])
def test_forward_ddv_micro_every_stage(dva, bits):
    """swin_micro_patch4_window7_56 (shifted and unshifted blocks, one merge), n = 3: 43 stages (62 with the linear layers), each against
    pair_cosine_cpu on oracle values; logits byte-equal to forward and to the oracle"""
    m = _micro7()
    _check_forward_ddv(dva, m, 3, bits)
    assert len(dva.ddv.swin_stage_names(m.arch['depths'], False)) == 43


def test_forward_ddv_window12(dva):
    m = _calibrated(dva, dva.swin.swin_micro_patch4_window12_96, 96)
    _check_forward_ddv(dva, m, 2, 8)


def test_forward_ddv_width96(dva):
    """embed_dim 96: K = 96 is no multiple of 64, att and ln have a row stride of 128 whose padding must not be read"""
    make = lambda **kw: dva.SwinTransformer(img_size=56, embed_dim=96, depths=(1, 1), num_heads=(3, 6), **kw)
    m = _calibrated(dva, make, 56)
    _check_forward_ddv(dva, m, 2, 8)


# --------------------------------------------------------------------------------------------------
# 6. linear taps, hooks, CKA
# --------------------------------------------------------------------------------------------------
def test_linear_taps_hooks_and_cka(dva):
    from diff_vit_amd.ptq import QConv2d, QLinear
    m = _micro7()
    x = _pairs(dva, 6, 56)[0]
    with torch.no_grad():
        st, ref = oracle_stages(m, x, 8)
    fp = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    fp.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()}, strict=False)
    m.cuda()
    try:
        acts = dva.get_activations(x, m, 8, 'cuda')
        names = [n_ for n_, mod in m.named_modules() if type(mod) in (QConv2d, QLinear)]
        blocks, merges = sum(m.arch['depths']), len(m.arch['depths']) - 1
        assert len(acts) == 4 * blocks + merges + 2 == len(names)
        for nm, t in zip(names, acts):
            want = st[nm][0]
            got = t.cpu()
            if nm == 'patch_embed.proj':
                got = got.permute(0, 2, 3, 1)                              # the hook of a QConv2d sees [B, D, H/P, W/P]
            assert torch.equal(got.reshape(got.shape[0], -1), want), (nm, float((got.reshape(got.shape[0], -1) - want).abs().max()))
        # hooks: once each, in named_modules order; a replacing hook raises; without hooks the plain forward runs
        seen = []
        hooks = [mod.register_forward_hook(lambda mod_, i, o, nm=nm: seen.append(nm)) for nm, mod in m.named_modules() if type(mod) in (QConv2d, QLinear)]
        with torch.no_grad():
            out = m(x.cuda())
        assert seen == names and torch.equal(out.cpu(), ref)
        for h in hooks:
            h.remove()
        h = m.head.register_forward_hook(lambda mod_, i, o: o * 2)
        with pytest.raises(RuntimeError):
            m(x.cuda())
        h.remove()
        with pytest.raises(NotImplementedError):
            dva.get_activations(x, m, [8] * 10, 'cuda')
        # CKA float vs quantized: finite, and equal to the CPU gram_matrix path on the same taps within the bound of tests/test_cka_gpu.py
        fp.cuda()
        heat = dva.compute_cka(fp, m, [x], None, 8)
        assert heat.is_cuda and tuple(heat.shape) == (len(names), len(names)) and bool(torch.isfinite(heat).all())
        a1 = [t.cpu() for t in dva.get_activations(x, fp, None, 'cuda')]
        a2 = [t.cpu() for t in acts]
        cpu = dva.MinibatchCKA(len(a1), len(a2), across_models=True)
        cpu.update_state_across_models(a1, a2)
        assert float((heat.cpu() - cpu.result()).abs().max()) <= 1e-5
    finally:
        m.cpu()


# --------------------------------------------------------------------------------------------------
# 7. float Swin on the GPU, 8. command line
# --------------------------------------------------------------------------------------------------
def test_float_swin_ddv_on_gpu(dva):
    from test_swin_modeldiff import reference_ddv, hooked_numpy
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    x, xa = _pairs(dva, 3, 56)
    with pytest.raises(NotImplementedError):
        dva.compute_ddv(m, x, xa, [8] * 10)
    m.cuda()
    d = dva.compute_ddv(m, x, xa, None)
    names = dva.ddv.swin_stage_names(m.arch['depths'], True)
    assert list(d) == names and all(v.is_cuda and v.dtype == torch.float64 for v in d.values())
    want = reference_ddv(hooked_numpy(m, x.cuda(), names), hooked_numpy(m, xa.cuda(), names))
    for nm in names:
        assert float(np.abs(d[nm].cpu().numpy() - want[nm]).max()) <= 1e-9, nm


def test_cli_swin_tiny(dva, tmp_path):
    out = str(tmp_path / 'ddv_result')
    sim = dva.ddv.main(['--model', 'swin_tiny', '--n', '2', '--steps', '2', '--result-name', out])
    with open(os.path.join(out, 'ddv.pkl'), 'rb') as f:
        res = pickle.load(f)
    names = dva.ddv.swin_stage_names((2, 2, 6, 2), True)
    assert list(res['float']) == names == list(res['quantized']) == list(sim) and res['bits'] == 8
    assert all(v.shape == (2,) for v in res['quantized'].values())
    with pytest.raises(NotImplementedError):
        dva.ddv.main(['--model', 'swin_tiny', '--bits', 'mixed', '--result-name', out])
