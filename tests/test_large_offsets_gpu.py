"""GPU: operands placed so far from their base pointer that a byte offset reaches 2^31, 2^32 and beyond - the address arithmetic of
every kernel, at strides, pitches and batches no other module uses.

Every operand lives in a device-side sentinel arena (tests/_big_arena.py); the compute is tiny and the memory mostly untouched
padding.  Every operand that reaches 2^31 bytes lies behind a low guard of 2 GiB, so a byte offset that is sign-extended from, or
truncated to, 32 bits lands in memory the test owns and shows as a wrong value or a changed guard byte (not so an ELEMENT offset of
fp32 data truncated to 32 bits: it spans 8 GiB either way, which the 16 GiB a case may hold cannot cover at a 2 GiB sample stride).  A
case holds at most 16 GiB; buffers are dropped between cases and between the two sentinel runs.  Results are compared bit for bit with the
references of the modules that test the same operator at small strides (imported from there, not restated); where the large operand is
a tiling of a few distinct blocks the reference is checked on the blocks at a small launch and the large launch is compared with the
tiled small result on the device.  Both neighbours of every documented bound: the last accepted shape against the reference, the first
refused one by its return code, with nothing written."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from _arena import SENTINELS
from _big_arena import BigArena, twice
from _tuning import tuning
from conftest import gpu_ok
from test_kernel_edges_gpu import Norm, _check, _codes, _gen, _ln_gemm_layer, _random_layer

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

G2 = 1 << 31


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


def _s8(sentinel):
    return int(np.int8(np.uint8(sentinel)))


# --------------------------------------------------------------------------------------------------
# GEMM
# --------------------------------------------------------------------------------------------------
GM, GK, GN = 257, 192, 144            # ragged last tile in M (128 / 256) and N (128); three k-tiles
LDA_LAST = 16711920                   # 257 * lda + 192 = 4 294 963 632 < 2^32: row 128 starts below 2^31, row 129 above
LD_FIRST = 16711936                   # 257 * ld = 4 294 967 552 >= 2^32
assert 128 * LDA_LAST < G2 < 129 * LDA_LAST and GM * LDA_LAST + GK < 1 << 32 <= GM * LD_FIRST


def _gemm(lay, kind, M, lda, ldo, sentinel, a_low=None, o_low=None, a_cover=0, o_cover=0, tapped=False):
    """one launch of p2v_gemm_i8 (tapped: p2v_gemm_resid_tap, the residual in an arena of its own) -> (return code, results on the host).
    RESID through p2v_gemm_i8 runs in place on the residual, as the forward runs it."""
    E, N, K, p = lay.E, lay.N, lay.K, lay.p
    L = E.lib()
    resid = kind.startswith('resid')
    a = BigArena(M, lay.width, lda, torch.int8, sentinel, init=lay.x[:M], low_guard=a_low, cover=a_cover)
    out = BigArena(M, N, ldo, torch.float32 if kind == 'head' else torch.int8, sentinel, init=p['res'][:M] if resid and not tapped else None,
                   low_guard=o_low, cover=o_cover * (4 if kind == 'head' else 1))
    codes = BigArena(M, N, ldo, torch.int8, sentinel, low_guard=o_low, cover=o_cover) if kind == 'head' or tapped else None
    res = BigArena(M, N, ldo, torch.int8, sentinel, init=p['res'][:M], low_guard=o_low, cover=o_cover) if tapped else None
    k, epi = lay.epilogue(kind, (res if tapped else out).ptr)
    if tapped:
        rc = L.p2v_gemm_resid_tap(a.ptr, lda, M, K, N, C.byref(lay.lin), C.byref(epi), out.ptr, ldo, codes.ptr, E.stream_ptr())
    else:
        rc = L.p2v_gemm_i8(k, a.ptr, lda, M, K, N, C.byref(lay.lin), C.byref(epi), out.ptr, ldo, codes.ptr if codes else None, E.stream_ptr())
    _sync()
    what = (kind, M, K, N, lda, ldo, lay.w4, tapped)
    assert a.equals_tiled(lay.x[:M]), ('A changed', what)
    a.read(('A', what), gather=False)
    got = dict(out=out.read(('out', what)).cpu().float())
    if codes:
        got['mid' if tapped else 'codes'] = codes.read(('out_codes', what)).cpu().float()
    if res:
        assert res.equals_tiled(p['res'][:M]), ('residual changed', what)
        res.read(('residual', what), gather=False)
    return rc, got


def _accepted(E, lay, *args, **kw):
    def run(s):
        rc, got = _gemm(lay, *args, sentinel=s, **kw)
        E.check(rc)
        return got
    return twice(run)


def _refused(E, lay, kind, M, lda, ldo, code, needle, **kw):
    """the call returns `code`, its message holds `needle`, and every output row still holds what it held"""
    for s in SENTINELS:
        rc, got = _gemm(lay, kind, M, lda, ldo, sentinel=s, **kw)
        msg = E.lib().p2v_last_error().decode()
        assert rc == code and needle in msg, (rc, msg)
        untouched = lay.p['res'][:M] if kind.startswith('resid') and not kw.get('tapped') else torch.full((M, lay.N), float(_s8(s)))
        assert torch.equal(got['out'], untouched), 'a refused call wrote to out'
        if 'mid' in got:
            assert bool((got['mid'] == _s8(s)).all()), 'a refused call wrote to out_codes'
        torch.cuda.empty_cache()


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('tile', [128, 256])
@pytest.mark.parametrize('kind', ['requant', 'gelu_tab', 'resid', 'resid_pre'])
def test_gemm_a_rows_past_2g(dva, oracle, kind, tile, w4):
    """tiled kernel, M = 257, K = 192, N = 144, lda = 16 711 920: the LDS-DMA lane offsets (unsigned)row * lda + chunk of rows 129 .. 256
    have bit 31 set - saddr + zext(voffset) of global_load_lds_dwordx4 on hardware.  A behind a 2 GiB low guard, the padding between
    its rows poisoned, `out` dense."""
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(3000 + (7 if w4 else 0)), GK, GN, w4, GM)
    with tuning(E.lib(), gemm_tile=tile):
        got = _accepted(E, lay, kind, GM, LDA_LAST, GN, a_low=G2)
    _check(got, lay.reference(oracle, kind, GM), (kind, tile, w4))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
def test_gemm_a_bound(dva, oracle, w4):
    """the other side of M * lda + K < 2^32: lda = 16 711 936 is refused by the tiled kernel with a message that names the bound, and
    nothing is written (A's arena covers what the launch would have read); the few-rows kernel (gemm_rows = 1) addresses with 64 bits
    and takes the same call"""
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(3000 + (7 if w4 else 0)), GK, GN, w4, GM)
    for kind, tile in (('requant', 128), ('gelu_tab', 256), ('resid', 0), ('resid_pre', 128)):
        with tuning(E.lib(), gemm_tile=tile):
            _refused(E, lay, kind, GM, LD_FIRST, GN, E.E_UNSUPPORTED, 'M * lda + K = %d' % (GM * LD_FIRST + GK), a_low=G2)
    for kind in ('requant', 'gelu_tab', 'resid', 'resid_pre'):
        with tuning(E.lib(), gemm_rows=1):
            got = _accepted(E, lay, kind, GM, LD_FIRST, GN)
        _check(got, lay.reference(oracle, kind, GM), (kind, 'rows', w4))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
def test_gemm_64_bit_kernels_past_4g(dva, oracle, w4):
    """M = 65, lda = 2^26 + 64: the last row starts 4096 bytes past 2^32 - few-rows kernel (every epilogue) and the wide kernel (HEAD)"""
    E = dva.engine
    M, lda = 65, (1 << 26) + 64
    assert (M - 1) * lda > 1 << 32
    lay = _random_layer(E, oracle, _gen(3100 + (7 if w4 else 0)), GK, GN, w4, M)
    for kind in ('requant', 'gelu_tab', 'resid', 'resid_pre'):
        with tuning(E.lib(), gemm_rows=1):
            got = _accepted(E, lay, kind, M, lda, GN)
        _check(got, lay.reference(oracle, kind, M), (kind, 'rows', w4))
    got = _accepted(E, lay, 'head', M, lda, GN)
    _check(got, lay.reference(oracle, 'head', M), ('head', w4))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('tile', [128, 256])
def test_gemm_out_rows_past_4g(dva, oracle, tile, w4):
    """the 64-bit stores of the untapped epilogues: REQUANT and GELU at M = 257, ldo = 16 711 936 (the last row starts past 2^32 - 2^24,
    M * ldo >= 2^32), RESID in place (store and residual load at (long long)m * ldo + n) and pre-folded at M = 257, ldo = 16 711 920: rows
    129 .. 256 start past 2^31 (the issue's M = 129 ends at row 128, which starts 8 MB below 2^31); A dense"""
    assert (GM - 1) * LDA_LAST >= G2
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(3200 + (7 if w4 else 0)), GK, GN, w4, GM)
    with tuning(E.lib(), gemm_tile=tile):
        for kind, M, ldo in (('requant', GM, LD_FIRST), ('gelu_tab', GM, LD_FIRST), ('gelu', GM, LD_FIRST), ('resid', GM, LDA_LAST), ('resid_pre', GM, LDA_LAST)):
            got = _accepted(E, lay, kind, M, GK, ldo, o_low=G2)
            _check(got, lay.reference(oracle, kind, M), (kind, tile, w4, M, ldo))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('tile', [128, 256])
def test_gemm_resid_tap_32_bit_stores(dva, oracle, tile, w4):
    """p2v_gemm_resid_tap: out, out_codes and the residual at base + (unsigned)row * ldo + n.  M = 193, ldo = 16 711 920: rows 129 .. 192
    start past 2^31, so their offsets have bit 31 set (the issue's M = 129 ends at row 128, which starts 8 MB below 2^31; 193 rows are what
    three operands behind 2 GiB low guards leave of the 16 GiB a case may hold, and a ragged last tile at either height).  Mid codes =
    q8(qgemm / s_mid) of the oracle, out = the RESID reference."""
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(3300 + (7 if w4 else 0)), GK, GN, w4, GM)
    M = 193
    assert (M - 1) * LDA_LAST >= G2 and 3 * ((M - 1) * LDA_LAST + G2 + (1 << 27)) < 16 << 30
    with tuning(E.lib(), gemm_tile=tile):
        got = _accepted(E, lay, 'resid', M, GK, LDA_LAST, o_low=G2, tapped=True)
    ref = lay.reference(oracle, 'resid', M)
    ref['mid'] = torch.clamp(torch.round(lay.y[:M] / lay.p['s_mid']), -128, 127)
    _check(got, ref, ('resid tap', tile, w4))


def test_gemm_resid_tap_bound(dva, oracle):
    """M * ldo >= 2^32 (M = 257, ldo = 16 711 936): P2V_E_SHAPE from the entry point, nothing written; the three arenas cover the refused
    extent.  The last accepted neighbour at this M: ldo = 16 711 920, rows 129 .. 256 past 2^31.  Three operands of 4.3 GB: 64 MiB low
    guards here (2 GiB each would pass the 16 GiB a case may hold), so a sign-extended offset of the accepted run would land outside the
    test's memory: the run that turns such an address into an assertion is test_gemm_resid_tap_32_bit_stores, rows 129 .. 192 behind 2 GiB
    guards; this test is about the two sides of the bound."""
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(3300), GK, GN, False, GM)
    _refused(E, lay, 'resid', GM, GK, LD_FIRST, E.E_SHAPE, 'M * ldo = %d' % (GM * LD_FIRST), tapped=True, o_low=1 << 26)
    got = _accepted(E, lay, 'resid', GM, GK, LDA_LAST, tapped=True, o_low=1 << 26)
    ref = lay.reference(oracle, 'resid', GM)
    ref['mid'] = torch.clamp(torch.round(lay.y / lay.p['s_mid']), -128, 127)
    _check(got, ref, 'resid tap, last accepted')


# --------------------------------------------------------------------------------------------------
# LayerNorm, alone and fused into the GEMM
# --------------------------------------------------------------------------------------------------
LN_ROWS, LN_STRIDE = 5, (1 << 30) + 16          # row 2 starts past 2^31, row 4 past 2^32


def _layernorm(call, codes, row_stride, out_stride, sentinel):
    rows, C_ = codes.shape
    a = BigArena(rows, C_, row_stride, torch.int8, sentinel, init=codes)
    out = BigArena(rows, C_, out_stride, torch.int8, sentinel)
    call(a.ptr, row_stride, rows, C_, out.ptr, out_stride)
    _sync()
    what = ('layernorm', rows, C_, row_stride, out_stride)
    assert a.equals_tiled(codes), ('x changed', what)
    a.read(('x', what), gather=False)
    return dict(out=out.read(('out', what)).cpu().float())


@pytest.mark.parametrize('C_', [100, 384, 3072])
def test_int_layernorm_rows_a_gib_apart(dva, oracle, C_):
    """p2v_int_layernorm, 5 rows: row_stride = 2^30 + 16 with a dense out, then a dense x with out_stride = 2^30 + 16; the generic chain
    (C = 100), the fast chain (384) and the row-per-workgroup kernel (3072); ln_rows 1 and 4, constants folded ahead or not"""
    E = dva.engine
    L = E.lib()
    gen = _gen(3400 + C_)
    norm = Norm(E, gen, C_)
    codes = _codes(gen, (LN_ROWS, C_), 35.0)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    call = lambda x, rs, rows, c, out, os_: E.check(L.p2v_int_layernorm(x, rs, rows, c, C.byref(norm.ln), out, os_, E.stream_ptr()))
    for (rs, os_), ln_rows, pre in itertools.product(((LN_STRIDE, C_), (C_, LN_STRIDE)), (1, 4), (False, True)):
        norm.prefold(pre)
        with tuning(L, ln_rows=ln_rows):
            got = twice(lambda s: _layernorm(call, codes, rs, os_, s))
        _check(got, dict(out=ref), ('layernorm', C_, rs, os_, ln_rows, pre))
    norm.prefold(False)


def test_float_layernorm_rows_a_gib_apart(dva):
    """p2v_float_layernorm at C = 384, the same two stride patterns, against the helper of test_float_ops_gpu.py"""
    import _float_ops_ref as R
    from test_float_ops_gpu import _ln_rows
    E = dva.engine
    L = E.lib()
    C_ = 384
    gen = _gen(3500)
    x = _ln_rows(LN_ROWS, C_, 3501)
    gamma = torch.rand(C_, generator=gen) + 0.5
    gamma[::7] *= -1.0
    beta = torch.randn(C_, generator=gen) * 0.3
    g = torch.ldexp(torch.ones(C_), (torch.arange(C_) % 9 - 6).to(torch.int32))
    want, _ = R.float_layernorm(x, 0.125, gamma, beta, 1e-6, g)
    dev = [t.cuda() for t in (gamma, beta, g)]
    ln = E.FloatLn(0.125, 1e-6, *[E.ptr(t) for t in dev])
    call = lambda xp, rs, rows, c, out, os_: E.check(L.p2v_float_layernorm(xp, rs, rows, c, C.byref(ln), out, os_, None, E.stream_ptr()))
    for rs, os_ in ((LN_STRIDE, C_), (C_, LN_STRIDE)):
        got = twice(lambda s: _layernorm(call, x.float(), rs, os_, s))
        assert torch.equal(got['out'].long(), want), (rs, os_, int((got['out'].long() != want).sum()))


LG_C, LG_N, LG_M = 384, 1152, 257
LG_STRIDE = 1 << 24                    # the launcher's bound: rows from 128 on start past 2^31, row 256 at 2^32


def _ln_gemm(E, norm, lay, kind, codes, row_stride, with_ln_out, sentinel):
    M, C_ = codes.shape
    N = lay.N
    a = BigArena(M, C_, row_stride, torch.int8, sentinel, init=codes, low_guard=G2)
    out = BigArena(M, N, N, torch.int8, sentinel)
    lno = BigArena(M, C_, C_, torch.int8, sentinel) if with_ln_out else None
    k, epi = lay.epilogue(kind)
    rc = E.lib().p2v_ln_gemm_i8(k, a.ptr, row_stride, M, C_, C.byref(norm.ln), N, C.byref(lay.lin), C.byref(epi), out.ptr, N,
                                lno.ptr if lno else None, E.stream_ptr())
    _sync()
    what = ('ln_gemm', kind, M, C_, N, row_stride, with_ln_out)
    assert a.equals_tiled(codes), ('x changed', what)
    a.read(('x', what), gather=False)
    res = dict(out=out.read(('out', what)).cpu().float())
    if lno:
        res['ln_out'] = lno.read(('ln_out', what)).cpu().float()
    return rc, res


@pytest.mark.parametrize('kind', ['requant', 'gelu_tab'])
def test_ln_gemm_at_the_row_stride_bound(dva, oracle, kind):
    """p2v_ln_gemm_i8, C = 384, N = 1152, M = 257, versions 1 / 2 / 3, with and without ln_out.  row_stride = 2^24, the last the launcher
    takes: k_ln_gemm2 adds lr * (int)row_stride, lr < 64, to the 64-bit address of a workgroup's first row.  row_stride = 2^24 + 4:
    P2V_E_UNSUPPORTED ("not fused"), out and ln_out untouched."""
    E = dva.engine
    L = E.lib()
    gen = _gen(3600)
    norm = Norm(E, gen, LG_C)
    codes = _codes(gen, (LG_M, LG_C), 35.0)
    q0, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    lay = _ln_gemm_layer(E, oracle, gen, norm, q0, LG_N)
    ref = lay.reference(oracle, kind, LG_M)
    for ver, with_ln in itertools.product((1, 2, 3), (False, True)):
        with tuning(L, ln_gemm_version=ver):
            def run(s):
                rc, got = _ln_gemm(E, norm, lay, kind, codes, LG_STRIDE, with_ln, s)
                E.check(rc)
                return got
            got = twice(run)
            _check(got, dict(ref, ln_out=q0) if with_ln else ref, ('ln_gemm', kind, ver, with_ln))
            for s in SENTINELS:
                rc, got = _ln_gemm(E, norm, lay, kind, codes, LG_STRIDE + 4, with_ln, s)
                msg = L.p2v_last_error().decode()
                assert rc == E.E_UNSUPPORTED and 'not fused' in msg, (rc, msg)
                assert all(bool((v == _s8(s)).all()) for v in got.values()), 'a refused call wrote to its outputs'
                torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------
# ViT attention: the batch carries qkv past 2^31 and the planes past 2^32
# --------------------------------------------------------------------------------------------------
def _tiled_launch(launch, block, B, outs, sentinel, what, dtype=torch.int8):
    """an operator over B images that repeat the few images of `block` ([images * rows per image][width], the dense input): outs maps a
    name to (rows per image, width, stride, dtype, expected [images * rows per image][width]) - every output is compared on the device
    with the tiled expectation, every arena is checked, nothing comes back to the host"""
    per = block.shape[0] // 4
    a = BigArena(B * per, block.shape[1], None, dtype, sentinel, init=block)
    arenas = {k: BigArena(B * r, w, st, dt, sentinel) for k, (r, w, st, dt, _) in outs.items()}
    launch(a.ptr, {k: v.ptr for k, v in arenas.items()})
    _sync()
    assert a.equals_tiled(block), ('the input changed', what)
    a.read(('input', what), gather=False)
    for k, ar in arenas.items():
        assert ar.equals_tiled(outs[k][4]), (k, 'differs from the tiled small launch', what)
        ar.read((k, what), gather=False)
    return {}


AT_B, AT_H, AT_N, AT_HD, AT_PITCH = 28400, 4, 197, 32, 208
assert AT_B * AT_N * 3 * AT_H * AT_HD > G2 and AT_B * AT_H * AT_N * AT_PITCH > 1 << 32 and AT_B % 4 == 0


def _lis_attn(E, hd):
    import p2vit_oracle as O
    from test_ddv_attention_gpu import S_A2, S_AT, S_Q1
    x0, bb, cc = O.lis_consts(torch.tensor([S_AT]))
    return E.Attn(S_Q1 * S_Q1, float(np.float32(hd ** -0.5)), 1.0 / S_AT, S_Q1 / S_A2, x0, bb, cc)


@pytest.mark.parametrize('mode', ['plain', 'heads12', 'scores', 'probs', 'scores_stream', 'probs_stream'])
def test_lis_attention_batch_past_2g(dva, oracle, mode):
    """hd = 32, H = 4, N = 197, B = 28 400: qkv is 2.15 GB, the dense probs_k of p2v_lis_attention 4.4 GB, a plane of
    p2v_lis_attention_taps at pitch 208 4.65 GB - one plane per launch (both, each behind its 2 GiB low guard, would pass the 16 GiB a
    case may hold), on the resident kernel and on the streaming kernel through attn_stream = 1.  heads12: H = 12, so that `out` itself
    (B * N * 384 bytes) passes 2^31, without planes.  Four distinct images: a launch at B = 4 against the oracle, the large launch against
    the tiled small result on the device."""
    from test_ddv_attention_gpu import S_A2, S_AT, S_Q1, _run_vit_taps, _vit_case
    from test_kernel_edges_gpu import _run_attention
    E = dva.engine
    L = E.lib()
    H, N, hd = (12 if mode == 'heads12' else AT_H), AT_N, AT_HD
    D = H * hd
    assert mode != 'heads12' or AT_B * N * D > G2
    qkv, sc, k, ref = _vit_case(N, hd, 4, H)
    at = _lis_attn(E, hd)
    i8 = torch.int8
    outs = dict(out=(N, D, D, i8, ref.reshape(4 * N, D)))
    with tuning(L, attn_stream=1 if mode.endswith('_stream') else 0):
        if mode in ('plain', 'heads12'):
            small = _run_attention(E, oracle, qkv, H, hd, S_Q1, S_AT, S_A2, SENTINELS[0])
            assert torch.equal(small['out'], ref) and torch.equal(small['probs_k'], k.long())
            if mode == 'plain':
                outs['probs_k'] = (H * N, N, N, i8, k.reshape(4 * H * N, N))
            launch = lambda x, o: E.check(L.p2v_lis_attention(x, AT_B, N, H, hd, C.byref(at), o['out'], o.get('probs_k'), E.stream_ptr()))
        else:
            scores = mode.startswith('scores')
            small = _run_vit_taps(E, qkv, H, hd, SENTINELS[0], True, AT_PITCH, which=(scores, not scores))
            want = sc if scores else k
            assert torch.equal(small['out'], ref) and torch.equal(small['scores' if scores else 'probs_k'], want.long())
            outs['plane'] = (H * N, N, AT_PITCH, i8, want.reshape(4 * H * N, N))
            launch = lambda x, o: E.check(L.p2v_lis_attention_taps(x, AT_B, N, H, hd, C.byref(at), o['out'], o['plane'] if scores else None,
                                                                   None if scores else o['plane'], AT_PITCH, E.stream_ptr()))
        twice(lambda s: _tiled_launch(launch, qkv.reshape(4 * N, 3 * D), AT_B, outs, s, ('lis attention', mode)))


def test_lis_attention_packed_batch_past_2g(dva, oracle):
    """the packed kernel (609 tokens, hd = 64), H = 1, B = 18 500: B * 609 * 192 > 2^31"""
    from test_ddv_attention_gpu import S_A2, S_AT, S_Q1, _vit_case
    from test_kernel_edges_gpu import _run_attention
    E = dva.engine
    L = E.lib()
    B, H, N, hd = 18500, 1, 609, 64
    assert B * N * 3 * hd > G2 and L.p2v_attention_kernel(hd, N, 0) == 1
    qkv, _, k, ref = _vit_case(N, hd, 4, H)
    small = _run_attention(E, oracle, qkv, H, hd, S_Q1, S_AT, S_A2, SENTINELS[0])
    assert torch.equal(small['out'], ref) and torch.equal(small['probs_k'], k.long())
    at = _lis_attn(E, hd)
    outs = dict(out=(N, hd, hd, torch.int8, ref.reshape(4 * N, hd)))
    launch = lambda x, o: E.check(L.p2v_lis_attention(x, B, N, H, hd, C.byref(at), o['out'], None, E.stream_ptr()))
    twice(lambda s: _tiled_launch(launch, qkv.reshape(4 * N, 3 * hd), B, outs, s, 'packed attention'))


def test_softmax_attention_batch_past_2g(dva, oracle):
    """p2v_softmax_attention in the geometry of test_lis_attention_batch_past_2g, against the helper of test_float_ops_gpu.py"""
    import _float_ops_ref as R
    from _arena import Arena
    from test_float_ops_gpu import _attn_case
    E = dva.engine
    L = E.lib()
    H, N, hd, D = AT_H, AT_N, AT_HD, AT_H * AT_HD
    s_q1, s_a2, s_at = 2.0 ** -3, 2.0 ** -2, 2.0 ** -4
    qkv = _attn_case(N, hd, H, 4, 3700)
    q = qkv.reshape(4, N, 3, H, hd).permute(2, 0, 3, 1, 4).float()
    sc = R.score_codes(oracle, q[0], q[1], torch.tensor(s_q1), torch.tensor(s_at), hd)
    table = R.softmax_table(s_at)
    want = R.softmax_attention(sc, q[2], table, s_q1 / s_a2).transpose(1, 2).reshape(4 * N, D)
    tab = torch.from_numpy(table.astype(np.int32)).cuda()
    at = E.SoftmaxAttn(s_q1 * s_q1, float(np.float32(hd ** -0.5)), 1.0 / s_at, s_q1 / s_a2, E.ptr(tab))
    xin, out = Arena(4 * N, 3 * D, sentinel=SENTINELS[0], init=qkv), Arena(4 * N, D, sentinel=SENTINELS[0])
    E.check(L.p2v_softmax_attention(xin.ptr, 4, N, H, hd, C.byref(at), out.ptr, E.stream_ptr()))
    _sync()
    assert torch.equal(out.read('small out').long(), want)
    outs = dict(out=(N, D, D, torch.int8, want))
    launch = lambda x, o: E.check(L.p2v_softmax_attention(x, AT_B, N, H, hd, C.byref(at), o['out'], E.stream_ptr()))
    twice(lambda s: _tiled_launch(launch, qkv, AT_B, outs, s, 'softmax attention'))


# --------------------------------------------------------------------------------------------------
# Swin window attention: token rows 8 or 16 MiB apart
# --------------------------------------------------------------------------------------------------
WIN_B, WIN_HEADS = 2, 2
# row stride per window side.  2^24 at ws = 7 (392 rows, 6.1 GiB: rows from 128 on start past 2^31, the rows of the second image from
# row 60 on past 2^32); at ws = 12 the 1152 rows of two images would take 18 GiB at 2^24, past the 16 GiB a case may hold, so 2^23
# there (9 GiB): rows from 256 on start past 2^31 and the whole second image past 2^32
WIN_STRIDE = {7: 1 << 24, 12: 1 << 23}


def _win_data(ws):
    from _ddv_attention_ref import window_taps_reference
    from test_ddv_attention_gpu import WIN_SCALES
    Hf, shift, C_ = 2 * ws, ws // 2, WIN_HEADS * 32
    gen = _gen(3800 + ws)
    qkv = _codes(gen, (WIN_B, Hf * Hf, 3 * C_), 25.0)
    qkv[:, 0] = 127
    qkv[:, 1, C_:2 * C_] = -128
    tab = _codes(gen, ((2 * ws - 1) ** 2, WIN_HEADS), 30.0)
    ref = window_taps_reference(qkv, tab, WIN_HEADS, Hf, ws, shift, WIN_SCALES)
    stride = WIN_STRIDE[ws]
    assert (Hf * Hf - 1) * stride >= G2 and (2 * Hf * Hf - 1) * stride >= 1 << 32 and 2 * Hf * Hf * stride + (2 << 30) < 16 << 30
    return qkv, tab, ref, stride


def _win_launch(E, call, qkv, ldq, ldo, sentinel, planes=None):
    """qkv rows ldq apart, out rows ldo apart (0: dense), planes: (rows, N, pitch) of the three tap planes -> out [B T][C] and the planes
    on the host"""
    B, T = qkv.shape[:2]
    C_ = WIN_HEADS * 32
    a = BigArena(B * T, 3 * C_, ldq or 3 * C_, torch.int8, sentinel, init=qkv.reshape(B * T, 3 * C_))
    out = BigArena(B * T, C_, ldo or C_, torch.int8, sentinel)
    taps = [BigArena(planes[0], planes[1], planes[2], torch.int8, sentinel) for _ in range(3)] if planes else []
    call(a.ptr, out.ptr, [t.ptr for t in taps])
    _sync()
    what = ('window attention', T, ldq, ldo)
    assert a.equals_tiled(qkv.reshape(B * T, 3 * C_)), ('qkv changed', what)
    a.read(('qkv', what), gather=False)
    got = dict(out=out.read(('out', what)).cpu().float().reshape(B, T, C_))
    for nm, t in zip(('a1', 'a2', 'k'), taps):
        got[nm] = t.read((nm, what)).cpu().long()
    return got


@pytest.mark.parametrize('ws', [7, 12])
def test_window_attention_rows_mib_apart(dva, oracle, ws):
    """p2v_window_attention (ws = 7) and its wide kernel (ws = 12), feature map 2 ws x 2 ws, shifted, two images, two heads: qkv_stride
    large with a dense out, then a dense qkv with out_stride large; then p2v_window_attention_taps at the large qkv_stride with small
    planes (the stride is the subject, not the planes)"""
    from test_ddv_attention_gpu import WIN_SCALES as c
    E = dva.engine
    L = E.lib()
    qkv, tab, ref, stride = _win_data(ws)
    B, T = qkv.shape[:2]
    N, nW = ws * ws, ref['idx'].shape[0]
    lis = oracle.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(tab=tab.to(torch.int8).contiguous().cuda(), idx=ref['idx'].to(torch.int32).contiguous().cuda(), reg=ref['region'].to(torch.int8).contiguous().cuda())
    wa = lambda ldq, ldo: E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], lis[0], lis[1],
                                    lis[2], E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']), ws, nW, ldq, ldo)
    for ldq, ldo in ((stride, 0), (0, stride)):
        w = wa(ldq, ldo)
        call = lambda x, o, _: E.check(L.p2v_window_attention(x, B, T, WIN_HEADS, 32, C.byref(w), o, None, E.stream_ptr()))
        got = twice(lambda s: _win_launch(E, call, qkv, ldq, ldo, s))
        assert torch.equal(got['out'], ref['want']), (ws, ldq, ldo, int((got['out'] != ref['want']).sum()))
    pitch = (N + 15) // 16 * 16 + 16
    w = wa(stride, 0)
    call = lambda x, o, p: E.check(L.p2v_window_attention_taps(x, B, T, WIN_HEADS, 32, C.byref(w), o, p[0], p[1], p[2], pitch, E.stream_ptr()))

    got = twice(lambda s: _win_launch(E, call, qkv, stride, 0, s, planes=(B * nW * WIN_HEADS * N, N, pitch)))
    assert torch.equal(got['out'], ref['want'])
    for nm in ('a1', 'a2', 'k'):
        assert torch.equal(got[nm].reshape(ref[nm].shape), ref[nm].long()), (ws, nm)


@pytest.mark.parametrize('ws', [7, 12])
def test_window_softmax_attention_rows_mib_apart(dva, ws):
    """p2v_window_softmax_attention in the same two layouts, against the helper of test_swin_float_ops_gpu.py"""
    import _swin_float_ops_ref as R
    from test_swin_float_ops_gpu import SCALES, _dev, _reference, _wa
    E = dva.engine
    qkv, tab, ref, stride = _win_data(ws)
    B, T = qkv.shape[:2]
    cs = dict(ws=ws, heads=WIN_HEADS, B=B, nW=ref['idx'].shape[0], N=ws * ws, T=T, C=WIN_HEADS * 32, qkv=qkv, tab=tab, idx=ref['idx'], region=ref['region'])
    table = R.softmax_table(SCALES['qact2'])
    want, _, _ = _reference(cs, SCALES, table)
    dev = _dev(cs, table)
    for ldq, ldo in ((stride, 0), (0, stride)):
        w = _wa(E, cs, SCALES, dev, ldq, ldo)
        call = lambda x, o, _: E.check(E.lib().p2v_window_softmax_attention(x, B, T, WIN_HEADS, 32, C.byref(w), E.ptr(dev['table']), o, E.stream_ptr()))
        got = twice(lambda s: _win_launch(E, call, qkv, ldq, ldo, s))
        assert torch.equal(got['out'].long(), want), (ws, ldq, ldo, int((got['out'].long() != want).sum()))


# --------------------------------------------------------------------------------------------------
# the model-diff readers: five samples a GiB (int8) / one or two GiB (fp32) apart
# --------------------------------------------------------------------------------------------------
RD_N, RD_ROWS, RD_COLS = 5, 33, 100


def _reader_arena(a, b, row_stride, sample_stride, dtype, sentinel):
    """a, b [n][rows][cols] as two operands of ONE arena (b lies 2^20 elements behind a, inside the padding between a's samples: two
    arenas of 8 GiB each would pass what a case may hold); the padding behind the cols of a row holds the sentinel -> (arena, blocks)"""
    n, rows, cols = a.shape
    width = (rows - 1) * row_stride + cols
    item = 4 if dtype == torch.float32 else 1
    pad = float(np.frombuffer(bytes([sentinel] * 4), np.float32)[0]) if item == 4 else float(sentinel if dtype == torch.uint8 else _s8(sentinel))
    blocks = []
    for v in (a, b):
        t = torch.full((n, rows, row_stride), pad)
        t[:, :, :cols] = v
        blocks.append(t.reshape(n, -1)[:, :width].contiguous())
    ar = BigArena(n, width, sample_stride, dtype, sentinel, init=blocks[0])
    ar.add(1 << 20, blocks[1])
    return ar, blocks


def _readers(E, a, b, row_stride, sample_stride, kind, sentinel, scale=None, shift=None):
    """pair cosine, statistics, stage Grams (and, fp32, the CKA Grams) of one arena -> dict of host results"""
    import _stats_ref as SR
    from _arena import Arena
    from test_stage_grams_gpu import _code_grams, _layer
    from test_stats_gpu import _run as _stats_run
    L = E.lib()
    n, rows, cols = a.shape
    dtype = torch.float32 if kind == 'f32' else (torch.uint8 if kind == 'log2k' else torch.int8)
    ar, blocks = _reader_arena(a, b, row_stride, sample_stride, dtype, sentinel)
    res = {}
    # pair cosine
    sc = scale.cuda() if scale is not None else None
    d = E.CosLayer(ar.ptr_of(0), ar.ptr_of(1), E.ptr(sc) if sc is not None else None, sample_stride, row_stride, rows, cols,
                   dict(i8=E.COS_I8, f32=E.COS_F32, log2k=E.COS_LOG2K)[kind])
    descs = (E.CosLayer * 1)(d)
    nb = L.p2v_pair_cosine_workspace_bytes(descs, 1, n)
    assert nb > 0, L.p2v_last_error()
    ws = Arena(1, nb, None, torch.uint8, sentinel, offset=0)
    sums = Arena(n, 3, None, torch.float64, sentinel)
    E.check(L.p2v_pair_cosine(descs, 1, n, sums.ptr, ws.ptr, nb, E.stream_ptr()))
    _sync()
    ws.read('pair-cosine workspace')
    res['sums'] = sums.read('pair-cosine sums')
    # statistics of a, Grams of a (log2k planes are read as unsigned bytes by the statistics; the Grams take codes and values only)
    sk = dict(i8=E.STAT_I8, f32=E.STAT_F32, log2k=E.STAT_U8)[kind]
    lay = E.StatLayer(ar.ptr_of(0), sample_stride, row_stride, n, rows, cols, sk)
    _, recs = _stats_run(E, [lay], [sk], [cols], sentinel)
    for f in SR.FIELDS:
        res['stats.' + f] = torch.from_numpy(np.atleast_1d(recs[0][f]).copy())
    if kind != 'log2k':
        sh = shift.cuda() if shift is not None else None
        gl = [_layer(E, ar.ptr_of(p).value, rows, cols, sample_stride, row_stride, sh.data_ptr() if sh is not None else None,
                     E.GRAM_F32 if kind == 'f32' else E.GRAM_I8) for p in (0, 1)]
        res['grams'] = _code_grams(E, gl, n, sentinel)
    if kind == 'f32':
        assert row_stride == cols
        descs = (E.CkaLayer * 2)()
        for dd, y in zip(descs, (None, ar.ptr_of(1))):
            dd.x, dd.y, dd.features, dd.ldx, dd.ldy = ar.ptr_of(0), y, rows * cols, sample_stride, sample_stride
        nb = L.p2v_cka_workspace_bytes(descs, 2, n)
        assert nb > 0, L.p2v_last_error()
        ws = Arena(1, nb, None, torch.uint8, sentinel, offset=0)
        out = Arena(2 * n, n, None, torch.float32, sentinel)
        E.check(L.p2v_cka_grams(descs, 2, n, out.ptr, ws.ptr, nb, E.stream_ptr()))
        _sync()
        ws.read('cka workspace')
        res['cka'] = out.read('cka grams').reshape(2, n, n)
    for p in (0, 1):
        assert ar.equals_tiled(blocks[p], p), 'an input of the readers changed'
    ar.read('reader inputs', gather=False)
    return res


def _bits(t):
    return t.contiguous().numpy().view({8: np.int64, 4: np.int32, 1: np.uint8}[t.element_size()])


def _cos_want(a, b, s2=None):
    a, b = a.double().reshape(RD_N, -1, RD_COLS), b.double().reshape(RD_N, -1, RD_COLS)
    s2 = torch.ones(RD_COLS, dtype=torch.float64) if s2 is None else s2
    return torch.stack([(a * b * s2).sum((1, 2)), (a * a * s2).sum((1, 2)), (b * b * s2).sum((1, 2))], 1)


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
def test_int8_readers_samples_a_gib_apart(dva, scaled):
    """p2v_pair_cosine (int8, plain and with per-channel scales), p2v_code_stats and p2v_code_grams (plain and shifted) on n = 5 samples of
    33 x 100 codes, row_stride 112, sample_stride = 2^30 + 16: sample 2 starts past 2^31, sample 4 past 2^32.  The references of
    test_modeldiff_edges_gpu.py (integer sums, exact in fp64 under power-of-two scales), _stats_ref.py and _stage_grams_ref.py."""
    import _stage_grams_ref as G
    import _stats_ref as SR
    from test_modeldiff_edges_gpu import _pow2_scales
    from test_stage_grams_gpu import _shift
    E = dva.engine
    gen = _gen(3900)
    a, b = [torch.randint(-128, 128, (RD_N, RD_ROWS, RD_COLS), generator=gen).float() for _ in range(2)]
    scale = _pow2_scales(RD_COLS) if scaled else None
    shift = _shift(gen, RD_COLS) if scaled else None
    got = twice(lambda s: _readers(E, a, b, 112, (1 << 30) + 16, 'i8', s, scale, shift))
    want = _cos_want(a, b, scale.double() ** 2 if scaled else None)
    assert np.array_equal(_bits(got['sums']), _bits(want)), (got['sums'].tolist(), want.tolist())
    SR.same({f: got['stats.' + f].numpy().reshape(np.shape(w)) for f, w in SR.record(a.numpy().astype(np.int8)).items()},
            SR.record(a.numpy().astype(np.int8)), 'int8 statistics')
    for p, v in enumerate((a, b)):
        G.assert_exact(got['grams'][p], G.int_gram(v.to(torch.int8), shift).double(), ('int8 grams', p, scaled))


def test_log2k_readers_samples_a_gib_apart(dva):
    """P2V_COS_LOG2K and the unsigned-byte statistics on exponent planes in the same layout"""
    import _stats_ref as SR
    from _ddv_attention_ref import log2k_sums
    E = dva.engine
    gen = _gen(3950)
    a, b = [torch.randint(0, 18, (RD_N, RD_ROWS, RD_COLS), generator=gen).float() for _ in range(2)]
    got = twice(lambda s: _readers(E, a, b, 112, (1 << 30) + 16, 'log2k', s))
    want = torch.from_numpy(log2k_sums(a.long(), b.long()))
    assert np.array_equal(_bits(got['sums']), _bits(want)), (got['sums'].tolist(), want.tolist())
    rec = SR.record(a.numpy().astype(np.uint8))
    SR.same({f: got['stats.' + f].numpy().reshape(np.shape(w)) for f, w in rec.items()}, rec, 'uint8 statistics')


@pytest.mark.parametrize('stride', [(1 << 29) + 4, (1 << 28) + 4], ids=['2^29+4', '2^28+4'])
def test_fp32_readers_samples_gib_apart(dva, stride):
    """the fp32 forms - p2v_pair_cosine, p2v_code_stats, p2v_code_grams and p2v_cka_grams (X X^T and X Y^T) - on n = 5 samples of 33 x 100
    dense values, sample_stride = ldx = 2^29 + 4 elements (element offsets pass 2^31, byte offsets 2^33) and 2^28 + 4 (byte offsets pass
    2^31 only).  Small integers: every product and sum is exact in any order, so the comparison is bit equality."""
    import _stage_grams_ref as G
    import _stats_ref as SR
    from _cka_ref import centre_restatement, small_integers
    E = dva.engine
    a, b = small_integers(4000, (RD_N, RD_ROWS, RD_COLS)), small_integers(4001, (RD_N, RD_ROWS, RD_COLS))
    assert float((a.abs().reshape(RD_N, -1) @ b.abs().reshape(RD_N, -1).t()).max()) < 2.0 ** 24
    got = twice(lambda s: _readers(E, a, b, RD_COLS, stride, 'f32', s))
    want = _cos_want(a, b)
    assert np.array_equal(_bits(got['sums']), _bits(want)), (got['sums'].tolist(), want.tolist())
    rec = SR.record(a.numpy())
    SR.same({f: got['stats.' + f].numpy().reshape(np.shape(w)) for f, w in rec.items()}, rec, 'fp32 statistics')
    for p, v in enumerate((a, b)):
        ref, _ = G.f64_gram(v)
        ref.diagonal().fill_(0)
        G.assert_exact(got['grams'][p], ref, ('fp32 grams', p))
    for l, y in enumerate((None, b)):
        r = centre_restatement(a, y)
        assert np.array_equal(_bits(got['cka'][l]), _bits(r)), ('cka grams', l)


# --------------------------------------------------------------------------------------------------
# contiguous operators: the batch alone carries them past 2^31
# --------------------------------------------------------------------------------------------------
def test_avgpool_batch_past_2g(dva):
    """p2v_avgpool_quant, T = 8192, C = 1024, B = 257: the last image starts at 2^31; four distinct images, the formula of
    test_kernel_edges_gpu.py"""
    E = dva.engine
    T, C_, B = 8192, 1024, 257
    assert (B - 1) * T * C_ == G2
    x = _codes(_gen(4100), (4, T, C_), 60.0)
    x[0], x[1] = 127.0, -128.0
    s_in, inv_s_out = 2.0 ** -4, 2.0 ** 4
    ref = torch.clamp(torch.round(((x.sum(1) * s_in) / float(T)) * inv_s_out), -128, 127)
    assert ref[0].max() == 127 and ref[1].min() == -128 and len(torch.unique(ref[3])) > 3

    def run(s):
        a = BigArena(B * T, C_, None, torch.int8, s, init=x.reshape(4 * T, C_))
        out = BigArena(B, C_, None, torch.int8, s)
        E.check(E.lib().p2v_avgpool_quant(a.ptr, B, T, C_, s_in, inv_s_out, out.ptr, E.stream_ptr()))
        _sync()
        assert a.equals_tiled(x.reshape(4 * T, C_))
        a.read('avgpool x', gather=False)
        return dict(out=out.read('avgpool out').cpu().float())
    got = twice(run)['out']
    assert torch.equal(got, ref[torch.arange(B) % 4])


def test_patch_merge_batch_past_2g(dva):
    """p2v_patch_merge_gather, H = W = 64, C = 1024, B = 513: input and output are 2^31 + 2^22 bytes; the reference is the index
    permutation of test_kernel_edges_gpu.py, taken on the device from the input in place"""
    E = dva.engine
    H, W, C_, B = 64, 64, 1024, 513
    assert B * H * W * C_ > G2
    x = _codes(_gen(4200), (4, H * W, C_), 50.0)

    def run(s):
        a = BigArena(B * H * W, C_, None, torch.int8, s, init=x.reshape(4 * H * W, C_))
        out = BigArena(B * (H // 2) * (W // 2), 4 * C_, None, torch.int8, s)
        E.check(E.lib().p2v_patch_merge_gather(a.ptr, B, H, W, C_, out.ptr, E.stream_ptr()))
        _sync()
        xi, oi = a.view().reshape(B, H, W, C_), out.view().reshape(B, (H // 2) * (W // 2), 4 * C_)
        ok = torch.ones((), dtype=torch.bool, device='cuda')
        for b0 in range(0, B, 32):
            v = xi[b0: b0 + 32]
            ref = torch.cat([v[:, 0::2, 0::2], v[:, 1::2, 0::2], v[:, 0::2, 1::2], v[:, 1::2, 1::2]], -1)
            ok &= (ref.reshape(ref.shape[0], -1, 4 * C_) == oi[b0: b0 + 32]).all()
        assert bool(ok), 'merge differs from the index permutation'
        assert a.equals_tiled(x.reshape(4 * H * W, C_))
        a.read('merge x', gather=False)
        out.read('merge out', gather=False)
        return {}
    twice(run)


def test_fake_quant_past_2g_elements(dva):
    """p2v_fake_quant_f32, n = 2^31 + 1027 = 75 * 28 633 129 elements, codes only: a period of 75 values (five scales over runs of 15),
    the reference of test_kernel_edges_gpu.py on one period"""
    from test_kernel_edges_gpu import _fake_quant_ref
    E = dva.engine
    n, per = G2 + 1027, 75
    assert n % per == 0
    gen = _gen(4300)
    x = torch.randn(per, generator=gen) * 9.0
    scale = 2.0 ** torch.randint(-6, -2, (5,), generator=gen).float() * 1.1
    ref = _fake_quant_ref(x, scale, 5, 15, -128, 127)['codes']
    sc = scale.cuda()

    def run(s):
        a = BigArena(n // per, per, None, torch.float32, s, init=x.reshape(1, per))
        cd = BigArena(n // per, per, None, torch.int8, s)
        E.check(E.lib().p2v_fake_quant_f32(a.ptr, n, E.ptr(sc), 5, 15, -128, 127, None, cd.ptr, E.stream_ptr()))
        _sync()
        assert cd.equals_tiled(ref.reshape(1, per)), 'codes differ from the tiled period'
        assert a.equals_tiled(x.reshape(1, per))
        a.read('fake-quant x', gather=False)
        cd.read('fake-quant codes', gather=False)
        return {}
    twice(run)


PF_B, PF_S, PF_P = 14268, 224, 16
assert PF_B * 3 * PF_S * PF_S > G2 and PF_B % 4 == 0


def test_quantize_patchify_batch_past_2g(dva):
    """p2v_quantize_patchify, P = 16, 224 x 224 x 3, B = 14 268: the image passes 2^31 elements (8.6 GB of fp32), the patch matrix 2^31
    bytes; four distinct images, the unfold reference of test_kernel_edges_gpu.py"""
    E = dva.engine
    S, P, rows, kp = PF_S, PF_P, (PF_S // PF_P) ** 2, 3 * PF_P * PF_P
    x = dva.synth.images(6, 4, S) * 3
    q = torch.clamp(torch.round(x * 16.0), -128, 127)
    ref = torch.nn.functional.unfold(q, P, stride=P).transpose(1, 2).reshape(4 * rows, kp)
    assert ref.abs().max() >= 127
    outs = dict(out=(rows, kp, kp, torch.int8, ref))
    launch = lambda xp, o: E.check(E.lib().p2v_quantize_patchify(xp, PF_B, 3, S, S, P, 16.0, o['out'], kp, E.stream_ptr()))
    twice(lambda s: _tiled_launch(launch, x.reshape(4, -1), PF_B, outs, s, 'quantize_patchify', torch.float32))


@pytest.mark.parametrize('layout', ['NHWC', 'NCHW'])
def test_u8_patchify_batch_past_2g(dva, layout):
    """p2v_u8_patchify in the same geometry (the uint8 image passes 2^31 bytes), both layouts, against p2v_quantize_patchify on the
    normalised images at B = 4 as test_kernel_edges_gpu.py does"""
    from diff_vit_amd import data as D
    E = dva.engine
    L = E.lib()
    S, P, rows, kp = PF_S, PF_P, (PF_S // PF_P) ** 2, 3 * PF_P * PF_P
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    u8 = dva.synth.images_uint8(7, 4, S, 3)
    x32 = D.normalize_uint8(u8, mean, std).cuda()
    ref = torch.full((4 * rows, kp), 77, dtype=torch.int8, device='cuda')
    E.check(L.p2v_quantize_patchify(E.ptr(x32), 4, 3, S, S, P, 32.0, E.ptr(ref), kp, E.stream_ptr()))
    _sync()
    li8 = D.uint8_lut_i8(D.uint8_lut(mean, std), 32.0).cuda()
    img = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()
    outs = dict(out=(rows, kp, kp, torch.int8, ref))
    launch = lambda xp, o: E.check(L.p2v_u8_patchify(xp, E.LAYOUTS[layout], E.ptr(li8), PF_B, 3, S, S, P, o['out'], kp, E.stream_ptr()))
    twice(lambda s: _tiled_launch(launch, img.reshape(4, -1), PF_B, outs, s, ('u8_patchify', layout), torch.uint8))
