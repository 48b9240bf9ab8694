"""GPU: the packed attention kernel (k_lis_attention_packed: head_dim 64, 609 .. p2v_packed_tokens tokens, probs_k = NULL) against the
oracle restatement (lis_int -> lis_probs -> requant) and against the streaming kernel ("attn_packed" = 0), bit for bit.  The output lives
in a sentinel arena (tests/_arena.py), every launch runs twice with two fills, and every test first asks the library which kernel runs.

Without the probs_k tap the softmax exponents are seen only through the output: the probe test reads every exponent level 0 .. 16 through
one-hot V columns and two output multipliers, i.e. through both int8 planes of the P.V product."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from _arena import Arena, twice
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

HD = 64
PACKED, STREAM = 1, 2


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


class _packed:
    """the "attn_packed" switch for the duration of a block (tests/_tuning.py does not know it), restored to 1 on the way out"""

    def __init__(self, L, v):
        self.L, self.v = L, v

    def __enter__(self):
        assert self.L.p2v_set_tuning(b'attn_packed', self.v) == 0

    def __exit__(self, *exc):
        assert self.L.p2v_set_tuning(b'attn_packed', 1) == 0


def _q8(v):
    return torch.clamp(torch.round(v), -128, 127)


def _reference(oracle, qkv, H, s_q1, s_at, av_mul, scale):
    """score codes, exponents and output codes: the arithmetic of tests/test_engine_gpu.py::_check_lis_attention, with P.V in fp64 (the
    products 2^-k * v and their sums are exact there) and the one rounding of the output requantisation"""
    B, N = qkv.shape[:2]
    t = qkv.reshape(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    acc = t[0] @ t[1].transpose(-2, -1)
    sc = _q8(((acc * (s_q1 * s_q1)) * scale) / s_at)
    k = oracle.lis_int(sc, torch.tensor([s_at]))
    o = (oracle.lis_probs(k).double() @ t[2].double()).transpose(1, 2).reshape(B, N, H * HD)
    return sc, k, _q8(o * av_mul).float()


def _attn(E, oracle, s_q1, s_at, av_mul, scale):
    x0, bb, cc = oracle.lis_consts(torch.tensor([s_at]))
    return E.Attn(s_q1 * s_q1, scale, 1.0 / s_at, av_mul, x0, bb, cc)


def _run(E, oracle, qkv, H, s_q1, s_at, av_mul, scale, sentinel, rows=None):
    """one launch without the tap, qkv and out in arenas -> out [B][N][D] as int64 (rows: p2v_lis_attention_rows with that many query rows)"""
    B, N = qkv.shape[:2]
    D = H * HD
    at = _attn(E, oracle, s_q1, s_at, av_mul, scale)
    a = Arena(B * N, 3 * D, 3 * D, torch.int8, sentinel, init=qkv.reshape(B * N, 3 * D))
    out = Arena(B * N, D, D, torch.int8, sentinel)
    if rows is None:
        E.check(E.lib().p2v_lis_attention(a.ptr, B, N, H, HD, C.byref(at), out.ptr, None, E.stream_ptr()))
    else:
        E.check(E.lib().p2v_lis_attention_rows(a.ptr, B, N, H, HD, C.byref(at), rows, out.ptr, E.stream_ptr()))
    torch.cuda.synchronize()
    what = ('attention', B, N, H, rows)
    a.read(('qkv', what))
    return dict(out=out.read(('out', what)).long().reshape(B, N, D))


def _both_kernels(E, oracle, qkv, H, s_q1, s_at, av_mul, scale):
    """packed (asserted) twice into arenas, then the streaming kernel through the switch: the two outputs"""
    L = E.lib()
    N = qkv.shape[1]
    assert L.p2v_attention_kernel(HD, N, 0) == PACKED
    got = twice(lambda s: _run(E, oracle, qkv, H, s_q1, s_at, av_mul, scale, s))['out']
    with _packed(L, 0):
        assert L.p2v_attention_kernel(HD, N, 0) == STREAM
        old = _run(E, oracle, qkv, H, s_q1, s_at, av_mul, scale, 0x5B)['out']
    assert L.p2v_attention_kernel(HD, N, 0) == PACKED
    return got, old


def _tokens(L, n):
    limit = L.p2v_packed_tokens(HD)
    return {'limit': limit, 'limit-1': limit - 1}.get(n, n)


F32_SCALE = float(np.float32(HD ** -0.5))


# --------------------------------------------------------------------------------------------------
# 1. against the oracle and the streaming kernel
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N,H,e_at,scale', [
    (1, 609, 2, 4, F32_SCALE),                    # the first launch past the resident range: 10 groups, 31 padded keys
    (2, 640, 1, 5, F32_SCALE),                    # exactly 10 groups, no padding
    (1, 641, 3, 4, F32_SCALE),                    # one key into an 11th group
    (1, 785, 1, 6, F32_SCALE), (1, 1025, 2, 4, F32_SCALE), (1, 'limit-1', 1, 5, F32_SCALE), (1, 'limit', 1, 4, F32_SCALE),
    (1, 641, 1, 4, float(np.float32(80 ** -0.5)))])      # a multiplier that is no power of two: the fp32 requantisation chain
def test_packed_against_oracle_and_streaming(dva, oracle, B, N, H, e_at, scale):
    E, S = dva.engine, dva.synth
    N = _tokens(E.lib(), N)
    D = H * HD
    qkv = torch.clamp(torch.round(S.normal(4, 'aq%d' % N, (B, N, 3 * D), 30.0)), -128, 127)        # the input of _check_lis_attention
    qkv[0, 0, :D] = 127                           # a saturating score row
    qkv[0, 1, :D] = 0                             # an all-equal score row
    s_q1, s_at, s_a2 = 2.0 ** -4, 2.0 ** -e_at, 2.0 ** -3
    _, k, ref = _reference(oracle, qkv, H, s_q1, s_at, s_q1 / s_a2, scale)
    assert (k < 16).any()
    got, old = _both_kernels(E, oracle, qkv, H, s_q1, s_at, s_q1 / s_a2, scale)
    assert torch.equal(got.float(), ref), ('oracle', N, int((got.float() != ref).sum()))
    assert torch.equal(got, old), ('streaming kernel', N, int((got != old).sum()))


# --------------------------------------------------------------------------------------------------
# 2. exponent probe: every level 0 .. 16 through both planes
# --------------------------------------------------------------------------------------------------
def _probe_keys(N, gen):
    """64 distinct keys: the ends of the key range and of the resident range, the places where the lane map of a 64-key group changes
    (byte r, register j, lane group g), both sides of every group boundary, the rest drawn"""
    keys = [0, 15, 16, 63, 64, 607, 608, N - 1, N - 2, 3, 4, 12, 19, 31, 32, 47, 48, 60, 67, 79, 80]
    last = (N - 1) // 64 * 64
    keys += [last - 1, last]
    for m in range(2, (N + 63) // 64):
        keys += [64 * m - 1, 64 * m]
    out = []
    for j in keys:
        if 0 <= j < N and j not in out:
            out.append(j)
    out = out[:64]
    while len(out) < 64:
        j = int(torch.randint(0, N, (1,), generator=gen))
        if j not in out:
            out.append(j)
    return out


def _probe_qk(N, H, keys, gen):
    """q and k with one live channel: score(q, j) = q0[q] * a[j] / 128 (s_attn = 2^-4).  The probed keys carry a falling ladder a = 127 ...
    with a gap behind the top (head 0: an isolated maximum, k = 0) or two keys at the top (head 1: k = 1) and steps of 3 below, every
    other key -128; q0 runs through both signs and sizes, so a row holds the ladder stretched (k up to 16) or compressed, or - q0 < 0 -
    hundreds of keys at the maximum and the probed ones below."""
    q = torch.zeros(N, H, HD)
    k = torch.zeros(N, H, HD)
    cyc = torch.tensor([127., 100., 64., 48., 32., 24., 16., 8., 4., 0., -8., -32., -64., -127., 90., 12.])
    ladders = ([127., 95., 79.] + [71. - 3 * i for i in range(61)], [127., 126., 96., 80.] + [72. - 3 * i for i in range(60)])
    for h in range(H):
        a = torch.full((N,), -128.0)
        a[torch.tensor(keys)] = torch.roll(torch.tensor(ladders[h % 2]), 7 * h)
        k[:, h, 0] = a
        q[:, h, 0] = cyc[(torch.arange(N) + 5 * h) % 16]
        k[:, h, 1] = torch.randint(-20, 21, (N,), generator=gen).float()         # a little noise from a second channel
        q[:, h, 1] = torch.randint(-20, 21, (N,), generator=gen).float()
    return q, k


@pytest.mark.parametrize('N', [609, 'limit'])
def test_packed_exponent_probe(dva, oracle, N):
    """V one-hot per head: channel c is 1 (then 127) at key j_c and 0 elsewhere, so out[q, c] = clamp(rne(v * 2^-k(q, j_c) * av_mul)).  With
    v = 1 and av_mul = 2^7 the exponents 0 .. 7 read 127, 64 ... 1 (plane A), with av_mul = 2^15 the exponents 8 .. 15 do (plane B) and 16
    reads 0: decoded and compared with oracle.lis_int.  That every k in 0 .. 16 occurs at the probed keys is asserted on the oracle first."""
    E = dva.engine
    L = E.lib()
    N = _tokens(L, N)
    H = 2
    gen = torch.Generator().manual_seed(2100 + N)
    keys = _probe_keys(N, gen)
    assert len(set(keys)) == 64 and {0, 15, 16, 63, 64, 607, 608, N - 1} <= set(keys)
    q, kk = _probe_qk(N, H, keys, gen)
    s_q1, s_at = 2.0 ** -4, 2.0 ** -4
    assert L.p2v_attention_kernel(HD, N, 0) == PACKED
    for v_val, muls in ((1.0, (2.0 ** 7, 2.0 ** 15)), (127.0, (1.0, 2.0 ** 8))):
        v = torch.zeros(N, H, HD)
        for h in range(H):
            v[torch.tensor(keys), h, torch.arange(HD)] = v_val
        qkv = torch.stack([q, kk, v], 1).reshape(1, N, 3 * H * HD)
        outs = []
        for av_mul in muls:
            _, k, ref = _reference(oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE)
            kp = k[0][:, :, torch.tensor(keys)]                                   # [H][N][64]: the exponents the output shows
            assert sorted(set(kp.reshape(-1).tolist())) == list(range(17)), sorted(set(kp.reshape(-1).tolist()))
            got = twice(lambda s: _run(E, oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE, s))['out']
            assert torch.equal(got.float(), ref), ('probe', N, v_val, av_mul, int((got.float() != ref).sum()))
            outs.append(got[0].reshape(N, H, HD).permute(1, 0, 2))                # [H][N][channel]
        if v_val == 1.0:
            lo, hi = outs                                                         # av_mul 2^7 / 2^15
            lg = lambda t: torch.log2(torch.clamp(t, min=1).float() + (t == 127).float()).long()       # 127 is the clamped 128
            dec = torch.where(lo > 0, 7 - lg(lo), torch.where(hi > 0, 15 - lg(hi), torch.full_like(lo, 16)))
            assert torch.equal(dec, kp), ('decoded exponents', N, int((dec != kp).sum()))


# --------------------------------------------------------------------------------------------------
# 3. saturation: the constructions of tests/test_kernel_edges_gpu.py::test_lis_attention_saturating_values
# --------------------------------------------------------------------------------------------------
def _attn_heads(gen, N, kind):
    """q and k of one head from {-128, 127}.  'onehot': key 5 is all 127, every other key -128 with up to an eighth flipped to 127; queries
    cycle through all 127, all -128, alternating and random.  'equal': every key is all 127, so every score row is constant."""
    pm = lambda *shape: torch.where(torch.rand(*shape, generator=gen) < 0.5, torch.tensor(-128.0), torch.tensor(127.0))
    q = pm(N, HD)
    q[0::4] = 127.0
    q[1::4] = -128.0
    q[2::4, 0::2], q[2::4, 1::2] = 127.0, -128.0
    if kind == 'equal':
        return q, torch.full((N, HD), 127.0)
    k = torch.full((N, HD), -128.0)
    flips = torch.rand(N, HD, generator=gen) < torch.rand(N, 1, generator=gen) * 0.125
    k[flips] = 127.0
    k[5 % N] = 127.0
    return q, k


@pytest.mark.parametrize('v_kind', ['neg', 'alt'])
@pytest.mark.parametrize('N', [609, 'limit'])
def test_packed_saturating_values(dva, oracle, N, v_kind):
    """a one-hot head and an all-equal head, q and k from {-128, 127}; v = -128 everywhere with av_mul = 1 (-128 x -128 products in the
    planes, the sum of the probabilities above 1 on the clamp bound) / v alternating 127, -128 with av_mul = 2: against the oracle."""
    E = dva.engine
    N = _tokens(E.lib(), N)
    H = 2
    gen = torch.Generator().manual_seed(1300 + N)
    qkv = torch.zeros(1, N, 3, H, HD)
    for h, kind in enumerate(('onehot', 'equal')):
        qkv[0, :, 0, h], qkv[0, :, 1, h] = _attn_heads(gen, N, kind)
    if v_kind == 'neg':
        qkv[:, :, 2] = -128.0
    else:
        par = (torch.arange(N).reshape(N, 1, 1) + torch.arange(HD).reshape(1, 1, HD)) % 2
        qkv[0, :, 2] = torch.where(par == 0, torch.tensor(127.0), torch.tensor(-128.0)).expand(N, H, HD)
    qkv = qkv.reshape(1, N, 3 * H * HD)
    s_q1, s_at, av_mul = 2.0 ** -4, 2.0 ** -4, (1.0 if v_kind == 'neg' else 2.0)
    sc, k, ref = _reference(oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE)
    # the reference alone, before the GPU: the patterns are there
    assert int(((k[0, 0] < 16).sum(-1) == 1).sum()) >= N // 8                      # one key carries the whole probability
    assert int(((sc[0, 0].max(-1)[0] == 127) & (sc[0, 0].min(-1)[0] == -128)).sum()) >= N // 4
    assert bool((sc[0, 1].max(-1)[0] == sc[0, 1].min(-1)[0]).all())
    assert float(oracle.lis_probs(k).sum(-1).max()) > 1.0                          # a sum of probabilities above 1
    assert ref.min() == -128 and (v_kind == 'neg' or ref.max() == 127)
    got, old = _both_kernels(E, oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE)
    assert torch.equal(got.float(), ref), ('oracle', N, v_kind, int((got.float() != ref).sum()))
    assert torch.equal(got, old)


# --------------------------------------------------------------------------------------------------
# 4. query rows
# --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rows_case(dva, oracle):
    B, N, H = 2, 785, 1
    qkv = torch.clamp(torch.round(dva.synth.normal(6, 'rows785', (B, N, 3 * H * HD), 30.0)), -128, 127)
    s_q1, s_at, av_mul = 2.0 ** -4, 2.0 ** -4, 0.5
    assert dva.engine.lib().p2v_attention_kernel(HD, N, 0) == PACKED
    full = twice(lambda s: _run(dva.engine, oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE, s))['out']
    assert torch.equal(full.float(), _reference(oracle, qkv, H, s_q1, s_at, av_mul, F32_SCALE)[2])
    return dict(qkv=qkv, H=H, args=(s_q1, s_at, av_mul, F32_SCALE), full=full)


@pytest.mark.parametrize('rows', [1, 16, 17, 785])
def test_packed_query_rows(dva, oracle, rows_case, rows):
    """p2v_lis_attention_rows on the packed kernel: whole 16-row blocks that cover `rows` are written with the full run's values, every
    row behind them keeps the sentinel, nothing outside `out` is written (Arena.read)."""
    E = dva.engine
    c = rows_case
    N = c['qkv'].shape[1]
    assert E.lib().p2v_attention_kernel(HD, N, 0) == PACKED
    written = min(N, 16 * ((rows + 15) // 16))
    for sentinel in (0x5B, 0xA6):
        got = _run(E, oracle, c['qkv'], c['H'], *c['args'], sentinel, rows=rows)['out']
        assert torch.equal(got[:, :written], c['full'][:, :written]), (rows, int((got[:, :written] != c['full'][:, :written]).sum()))
        s8 = sentinel - 256 if sentinel > 127 else sentinel
        assert bool((got[:, written:] == s8).all()), (rows, 'rows behind the blocks were written')


# --------------------------------------------------------------------------------------------------
# 5. whole model: 677 tokens
# --------------------------------------------------------------------------------------------------
def test_packed_whole_model(dva, oracle):
    """embed_dim 128, 2 heads, depth 2, img_size 416 (677 tokens; built as tests/test_cls_rows_gpu.py::test_logits_equal_at_other_token_counts):
    the plan runs the packed kernel; logits of forward / forward_streams / forward_uint8 for three bit lists, batches 1 and 3, cls_rows 1
    and 0 are the same bytes with "attn_packed" 1 and 0, and for the int8 list they equal the oracle model."""
    from diff_vit_amd import data as Dm
    L = dva.engine.lib()
    img, dim, depth, heads = 416, 128, 2, 2
    arch = dict(img_size=img, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, num_classes=40, mlp_ratio=4.0)
    sd = dva.synth.vit_state_dict(arch, 33)
    m = dva.VisionTransformer(img_size=img, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, num_classes=40, mlp_ratio=4.0,
                              qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(sd, strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(33, 2, img).cuda())
    n = 4 * depth + 2
    x3 = dva.synth.images(33, 3, img, offset=700)
    assert L.p2v_attention_kernel(dim // heads, (img // 16) ** 2 + 1, 0) == PACKED
    out8 = m(x3.cuda(), [8] * n, False)[0]                                            # freezes the plan
    plan = m._plan
    assert plan.tokens == 677 and plan.attention_kernel == 'packed'
    orc = oracle.OracleViT(arch, sd)
    orc.calib = m.export_calib()
    ref = orc.quant_forward(x3, [8] * n)
    assert torch.equal(out8.cpu(), ref), int((out8.cpu() != ref).sum())
    mean, std, _ = Dm.MODEL_STATS['deit']
    lut = plan.input_lut(Dm.uint8_lut(mean, std))
    u3 = dva.synth.images_uint8(34, 3, img)

    def logits(B, bits):
        x, u8 = x3[:B].contiguous().cuda(), u3[:B].contiguous().cuda()
        lg = torch.empty(B, 40, device='cuda')
        plan.forward_streams(x, bits, lg)
        torch.cuda.synchronize()
        res = (plan.forward(x, bits).clone(), lg, plan.forward_uint8(u8, lut, bits).clone())
        torch.cuda.synchronize()
        return res

    try:
        for cls in (1, 0):
            assert L.p2v_set_tuning(b'cls_rows', cls) == 0
            for bits in ([8] * n, [4] * n, [8 if i % 3 else 4 for i in range(n)]):
                for B in (1, 3):
                    assert plan.attention_kernel == 'packed'
                    new = logits(B, bits)
                    with _packed(L, 0):
                        assert plan.attention_kernel == 'stream'
                        old = logits(B, bits)
                    for name, a, b in zip(('forward', 'forward_streams', 'forward_uint8'), new, old):
                        assert torch.equal(a, b), (name, cls, bits[:3], B, int((a != b).sum()))
                        assert torch.isfinite(a).all() and a.abs().max() > 0
                    assert torch.equal(new[0], new[1])
                    if bits == [8] * n and B == 3:
                        assert torch.equal(new[0].cpu(), ref)
    finally:
        L.p2v_set_tuning(b'cls_rows', 1)
