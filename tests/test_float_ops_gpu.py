"""GPU: Config(ptf=False) / Config(lis=False) on the engine - p2v_float_layernorm and p2v_softmax_attention as operators (sentinel arenas,
edge rows, hand-made tables) and the whole model under the three configurations, all bit-equal to tests/_float_ops_ref.py."""
import ctypes as ct

import numpy as np
import pytest
import torch

import _float_ops_ref as R
from _arena import Arena, twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


@pytest.fixture(scope='module')
def E(dva):
    from diff_vit_amd import engine
    engine.lib()
    return engine


def _rand_codes(gen, shape, std):
    return torch.clamp(torch.round(torch.randn(shape, generator=gen) * std), -128, 127).to(torch.int8)


# ---- float LayerNorm ---------------------------------------------------------------------------------------------------------------------
def _ln_rows(rows, C, seed):
    """random rows of several spreads, then (as far as there are rows) a constant row, all -128, all 127, alternating extremes"""
    gen = torch.Generator().manual_seed(seed)
    x = _rand_codes(gen, (rows, C), 40.0)
    x[0] = _rand_codes(gen, (C,), 3.0)
    special = [torch.full((C,), 37), torch.full((C,), -128), torch.full((C,), 127), torch.tensor([-128, 127] * (C // 2))]
    for k, row in enumerate(special):
        if 1 + k < rows:
            x[1 + k] = row.to(torch.int8)
    return x


@pytest.mark.parametrize('C', [16, 64, 192, 384, 768, 2048])
@pytest.mark.parametrize('rows', [1, 3, 64, 65])
def test_float_layernorm_operator(E, rows, C):
    L = E.lib()
    gen = torch.Generator().manual_seed(1000 * rows + C)
    x = _ln_rows(rows, C, rows + C)
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[::7] *= -1.0
    beta = torch.randn(C, generator=gen) * 0.3
    g = torch.ldexp(torch.ones(C), (torch.arange(C) % 9 - 6).to(torch.int32))          # 2^-6 .. 2^2 per channel
    s_in, eps = 0.125, 1e-6
    want, want_y = R.float_layernorm(x, s_in, gamma, beta, eps, g)
    gd, bd, ggd = gamma.cuda(), beta.cuda(), g.cuda()
    ln = E.FloatLn(s_in, eps, E.ptr(gd), E.ptr(bd), E.ptr(ggd))

    def run(sentinel):
        xin = Arena(rows, C, stride=C + 12, sentinel=sentinel, init=x)
        out = Arena(rows, C, stride=C + 8, sentinel=sentinel)
        tap = Arena(rows, C, dtype=torch.float32, sentinel=sentinel)
        out2 = Arena(rows, C, sentinel=sentinel)
        E.check(L.p2v_float_layernorm(xin.ptr, C + 12, rows, C, _ref(ln), out.ptr, C + 8, tap.ptr, E.stream_ptr()))
        E.check(L.p2v_float_layernorm(xin.ptr, C + 12, rows, C, _ref(ln), out2.ptr, C, None, E.stream_ptr()))
        torch.cuda.synchronize()
        return {'codes': out.read('out'), 'tap': tap.read('tap'), 'untapped': out2.read('out2')}

    got = twice(run)
    d = got['codes'].long() - want
    print('rows %d C %d: %d of %d codes differ from the helper' % (rows, C, int((d != 0).sum()), d.numel()))
    assert torch.equal(got['codes'].long(), want)
    assert torch.equal(got['untapped'], got['codes'])
    assert np.array_equal(got['tap'].numpy().view(np.uint32), want_y.numpy().view(np.uint32))
    if rows >= 3:      # the constant row: variance exactly 0, y = beta
        assert torch.equal(got['tap'][1], beta)


def _ref(struct):
    return ct.byref(struct)


def test_float_layernorm_refusals(E):
    L = E.lib()
    z = torch.zeros(64, device='cuda')
    x = torch.zeros(4, 64, dtype=torch.int8, device='cuda')
    ok = E.FloatLn(0.125, 1e-6, E.ptr(z), E.ptr(z), E.ptr(z))
    assert L.p2v_float_layernorm(E.ptr(x), 64, 4, 2052, _ref(ok), E.ptr(x), 2052, None, E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_float_layernorm(E.ptr(x), 64, 4, 12, _ref(ok), E.ptr(x), 64, None, E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_float_layernorm(E.ptr(x), 64, 4, 64, _ref(ok), E.ptr(x), 60, None, E.stream_ptr()) == E.E_SHAPE
    bad = E.FloatLn(0.3, 1e-6, E.ptr(z), E.ptr(z), E.ptr(z))
    assert L.p2v_float_layernorm(E.ptr(x), 64, 4, 64, _ref(bad), E.ptr(x), 64, None, E.stream_ptr()) == E.E_UNSUPPORTED


# ---- table-softmax attention -------------------------------------------------------------------------------------------------------------
def _attn_case(tokens, hd, heads, batch, seed):
    """qkv codes whose score codes fill the int8 range; query row 0 of every image is all zeros (a row of equal scores: every key ties at
    the maximum) and, from two tokens on, the last query / the first two keys of head 0 saturate to 127 and -128 in one row (d = 255)"""
    gen = torch.Generator().manual_seed(seed)
    D = heads * hd
    qkv = _rand_codes(gen, (batch, tokens, 3, heads, hd), 12.0)
    qkv[:, :, 2] = _rand_codes(gen, (batch, tokens, heads, hd), 50.0)
    qkv[:, 0, 0] = 0
    if tokens >= 2:
        qkv[:, tokens - 1, 0, 0] = 127
        qkv[:, 0, 1, 0] = 127
        qkv[:, 1, 1, 0] = -128
    return qkv.reshape(batch * tokens, 3 * D)


def _hand_tables(s):
    full = np.full(256, (1 << 21) - 1, dtype=np.int64)
    only0 = np.zeros(256, dtype=np.int64)
    only0[0] = 12345
    return {'plan': R.softmax_table(s), 'all_max': full, 'only_tab0': only0}


@pytest.mark.parametrize('heads,batch', [(1, 1), (1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize('hd', [32, 64])
@pytest.mark.parametrize('tokens', [1, 5, 17, 64, 65, 197, 608])
def test_softmax_attention_operator(E, oracle, tokens, hd, heads, batch):
    L = E.lib()
    D = heads * hd
    s_q1, s_a2 = 2.0 ** -3, 2.0 ** -2
    s_at = 2.0 ** -4 if (tokens + heads + batch) % 2 else 2.0 ** -5
    qkv = _attn_case(tokens, hd, heads, batch, 7 * tokens + hd + heads + batch)
    q = qkv.reshape(batch, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4).float()
    sc = R.score_codes(oracle, q[0], q[1], torch.tensor(s_q1), torch.tensor(s_at), hd)
    assert float(sc[:, :, 0].min()) == float(sc[:, :, 0].max()) == 0.0                      # the row of equal scores
    if tokens >= 2:
        last = sc[:, 0, tokens - 1]
        assert float(last.max()) == 127 and float(last.min()) == -128                           # d = 255 in one row
    tables = _hand_tables(s_at)
    want = {k: R.softmax_attention(sc, q[2], t, s_q1 / s_a2).transpose(1, 2).reshape(batch * tokens, D) for k, t in tables.items()}
    dev_tabs = {k: torch.from_numpy(t.astype(np.int32)).cuda() for k, t in tables.items()}
    pitch = (tokens + 15) // 16 * 16
    tap_case = heads == 3 and batch == 2

    def run(sentinel):
        xin = Arena(batch * tokens, 3 * D, sentinel=sentinel, init=qkv)
        res = {}
        for k, t in dev_tabs.items():
            at = E.SoftmaxAttn(s_q1 * s_q1, float(np.float32(hd ** -0.5)), 1.0 / s_at, s_q1 / s_a2, E.ptr(t))
            out = Arena(batch * tokens, D, sentinel=sentinel)
            E.check(L.p2v_softmax_attention(xin.ptr, batch, tokens, heads, hd, _ref(at), out.ptr, E.stream_ptr()))
            torch.cuda.synchronize()
            res[k] = out.read(k)
        if tap_case:
            at = E.SoftmaxAttn(s_q1 * s_q1, float(np.float32(hd ** -0.5)), 1.0 / s_at, s_q1 / s_a2, E.ptr(dev_tabs['plan']))
            out = Arena(batch * tokens, D, sentinel=sentinel)
            plane = Arena(batch * heads * tokens, tokens, stride=pitch, sentinel=sentinel)
            E.check(L.p2v_softmax_attention_taps(xin.ptr, batch, tokens, heads, hd, _ref(at), out.ptr, plane.ptr, pitch, E.stream_ptr()))
            torch.cuda.synchronize()
            res['tapped'] = out.read('tapped out')
            res['scores'] = plane.read('score plane')
        return res

    got = twice(run)
    for k in tables:
        d = got[k].long() - want[k]
        print('tokens %d hd %d heads %d batch %d table %s: %d of %d codes differ' % (tokens, hd, heads, batch, k, int((d != 0).sum()), d.numel()))
        assert torch.equal(got[k].long(), want[k]), k
    if tap_case:
        assert torch.equal(got['tapped'], got['plan'])
        assert torch.equal(got['scores'].long(), sc.reshape(batch * heads * tokens, tokens).long())


def test_softmax_attention_refusals(E):
    L = E.lib()
    t = torch.ones(256, dtype=torch.int32, device='cuda')
    x = torch.zeros(609 * 3 * 64, dtype=torch.int8, device='cuda')
    at = E.SoftmaxAttn(2.0 ** -6, 0.125, 16.0, 0.5, E.ptr(t))
    assert L.p2v_softmax_attention(E.ptr(x), 1, 609, 1, 64, _ref(at), E.ptr(x), E.stream_ptr()) == E.E_UNSUPPORTED
    assert L.p2v_softmax_attention(E.ptr(x), 1, 17, 1, 48, _ref(at), E.ptr(x), E.stream_ptr()) == E.E_UNSUPPORTED
    bad = E.SoftmaxAttn(2.0 ** -6, 0.125, 16.0, 0.3, E.ptr(t))
    assert L.p2v_softmax_attention(E.ptr(x), 1, 17, 1, 64, _ref(bad), E.ptr(x), E.stream_ptr()) == E.E_UNSUPPORTED


# ---- whole model -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world(dva, oracle):
    g = R.fixture()
    arch = dva.synth.ARCHS['micro']
    seed = int(g['seed'])
    w = dict(g=g, arch=arch, sd=dva.synth.vit_state_dict(arch, seed), x_cal=dva.synth.images(seed, int(g['n_calib']), arch['img_size']),
             x_ev=dva.synth.images(seed, int(g['n_eval']), arch['img_size'], offset=1000), models={})
    for tag in R.CONFIGS:
        m = R.make_model(dva, arch, w['sd'], tag, 'cuda')
        dva.harness.calibrate_model(m, w['x_cal'].cuda())
        w['models'][tag] = (m, m.export_calib())
    return w


def test_fails_without_the_feature(dva, world, oracle):
    """a quantized forward of a Config(False, False) micro model reports _fused() and equals the helper's logits (before the feature it
    ran the module graph, and freeze raised)"""
    m, c = world['models']['ff']
    assert m._fused()
    with torch.no_grad():
        out = m(world['x_ev'].cuda(), [8] * 10, False)[0].cpu()
    assert m._plan is not None and not m._plan.int_norm and not m._plan.int_softmax
    assert torch.equal(out, R.quant_forward(oracle, world['arch'], world['sd'], c, world['x_ev'], [8] * 10, False, False))


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_micro_logits_equal_the_helper(dva, world, oracle, tag):
    m, c = world['models'][tag]
    g = world['g']
    ptf, lis = R.CONFIGS[tag]
    s_o = float(c['act_out'].reshape(-1)[0])
    for name, bits in R.bit_lists(g, 10).items():
        with torch.no_grad():
            out, flops, gd = m(world['x_ev'].cuda(), bits, False)
        want = R.quant_forward(oracle, world['arch'], world['sd'], c, world['x_ev'], bits, ptf, lis)
        assert torch.equal(out.cpu(), want), (tag, name)
        assert flops == m.flops() and gd == []
        d = np.abs(np.rint((out.cpu().numpy() - g['%s/logits/%s' % (tag, name)]) / s_o))
        print(tag, name, 'engine against the REAL reference: %d of %d logit codes differ (max %d)' % (int((d > 0).sum()), d.size, int(d.max())))
        assert [int((d > 0).sum()), d.size, int(d.max())] == [int(v) for v in g['%s/logit_codes_differ/%s' % (tag, name)]]


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_one_block_at_deit_tiny_width(dva, oracle, tag):
    """192 channels, 3 heads, 224^2 -> 197 tokens, head_dim 64, batch 2.  (Seed 17 is the seed of tests/golden/deit_tiny.npz.  Not every
    seed will do for a one-block model under ptf=True: with 31 a row of block 0 reaches the INTEGER LayerNorm with zero variance, and the
    oracle's own quant_forward - the reference's formula - returns NaN there, whatever the softmax.)"""
    arch = dict(img_size=224, patch_size=16, embed_dim=192, depth=1, num_heads=3, num_classes=16, mlp_ratio=4.0)
    sd = dva.synth.vit_state_dict(arch, 17)
    m = R.make_model(dva, arch, sd, tag, 'cuda')
    dva.harness.calibrate_model(m, dva.synth.images(17, 2, 224).cuda())
    x = dva.synth.images(17, 2, 224, offset=500)
    c = m.export_calib()
    ptf, lis = R.CONFIGS[tag]
    for bits in ([8] * 6, [4, 8, 4, 8, 8, 4]):
        with torch.no_grad():
            out = m(x.cuda(), bits, False)[0].cpu()
        want = R.quant_forward(oracle, arch, sd, c, x, bits, ptf, lis)
        print(tag, bits, 'logit codes that differ:', int((out != want).sum()), 'of', out.numel())
        assert torch.equal(out, want), (tag, bits)


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_uint8_and_sliced_forward(dva, world, tag):
    from diff_vit_amd import data as Dt
    m, _ = world['models'][tag]
    mean, std, _ = Dt.MODEL_STATS['deit']
    u8 = dva.synth.images_uint8(5, 6, 32)
    bits = R.bit_lists(world['g'], 10)['qmix']
    with torch.no_grad():
        assert torch.equal(m.forward_uint8(u8.cuda(), bits, mean, std, 'NHWC')[0], m(Dt.normalize_uint8(u8, mean, std, 'NHWC').cuda(), bits)[0])
        x = dva.synth.images(9, 64, 32).cuda()
        sliced = m(x, bits)[0]                                   # 64 images: forward_streams
        assert torch.equal(sliced, m._plan.forward(x, bits))
        assert torch.equal(sliced[:6], m._plan.forward(x[:6].contiguous(), bits))


@pytest.mark.parametrize('stages', ['engine', 'full'])
@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_ddv_stage_sums(dva, world, oracle, tag, stages):
    """the default and the FULL stage sets of p2v_forward_ddv under the three configurations against sums formed from the helper's stages
    (_float_ops_ref.check_stage: bit-equal integer sums, 1e-12 per-channel, 1e-9 for fp32 values)"""
    m, c = world['models'][tag]
    ptf, lis = R.CONFIGS[tag]
    n = 3
    x = torch.cat((world['x_ev'][:n], world['x_ev'][n:2 * n]), 0)
    bits = [8] * 10
    if m._plan is None:
        m.freeze('cuda')
    out, names, sums = m._plan.forward_ddv(x.cuda(), bits, with_linear=False, stages=stages)
    st = {}
    want = R.quant_forward(oracle, world['arch'], world['sd'], c, x, bits, ptf, lis, stages=st)
    assert torch.equal(out.cpu(), want)
    assert names == dva.ddv.stage_names(2, False, stages == 'full')
    sums = sums.cpu().numpy()
    for k, nm in enumerate(names):
        values, scale, kind = st[nm]
        R.check_stage(nm, sums[k], values, scale, kind, tag=tag + '/' + stages)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(dva, world):
    from diff_vit_amd import swin
    s = swin.swin_micro_patch4_window7_56(cfg=dva.Config(False, True, 'minmax'), num_classes=10).eval()
    with pytest.raises(NotImplementedError):
        s.freeze('cuda')
    for tag in ('ff', 'tf'):
        m, _ = world['models'][tag]
        x = world['x_ev'][:2].cuda()
        with pytest.raises(NotImplementedError):
            dva.ddv.compute_ddv(m, x, x, [8] * 10, attention=True)
        if m._plan is None:
            m.freeze('cuda')
        with pytest.raises(NotImplementedError):
            m._plan.forward_ddv(torch.cat((x, x), 0), [8] * 10, attention=True)
    # more than 608 tokens (img 200 / patch 8: 25 * 25 + 1 = 626; 609 exactly is no square plus one: test_softmax_attention_refusals has it
    # at the operator) and head_dim 48 under lis=False: refused where the plan is created
    from diff_vit_amd import plan as P
    for arch in (dict(img_size=200, patch_size=8, embed_dim=64, depth=1, num_heads=1, num_classes=10, mlp_ratio=4.0),
                 dict(img_size=32, patch_size=8, embed_dim=96, depth=1, num_heads=2, num_classes=10, mlp_ratio=4.0)):
        with pytest.raises(NotImplementedError):
            P.FrozenPlan(arch, {}, {}, device='cuda', int_softmax=False)
