"""GPU: Config(ptf=False) of a Swin model on the engine, bit-equal to tests/_swin_float_ln_ref.py everywhere: p2v_float_layernorm on rows of
up to 4096 channels (k_float_layernorm_xwide beyond 2048) in sentinel arenas, the P2V_OP_FLOAT_LAYERNORM record, and the Swin plans under
(False, True) and (False, False) - fused, uint8, sliced, tapped, linear taps, DDV, statistics, one wide model whose merge norm takes the
new kernel - against the restatement's whole-model forward."""
import ctypes as C

import numpy as np
import pytest
import torch

import _swin_bits_ref as RB
import _swin_float_ln_ref as R
from _arena import Arena, twice
from _float_ops_ref import float_layernorm

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


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------------------
def _edge_rows(C_):
    """all 127, all -128, constant (variance exactly 0: y = beta), alternating 127 / -128, one-hot"""
    e = torch.zeros(5, C_, dtype=torch.int64)
    e[0], e[1], e[2] = 127, -128, 37
    e[3, ::2], e[3, 1::2] = 127, -128
    e[4, (2 * C_) // 3] = 127
    return e


def _constants(C_, seed):
    gen = torch.Generator().manual_seed(seed)
    gamma = torch.rand(C_, generator=gen) + 0.5
    gamma[::7] *= -1.0                                   # negative entries
    gamma[3::11] = 0.0                                   # and zeros: y = beta there
    beta = torch.randn(C_, generator=gen) * 0.3
    g = torch.ldexp(torch.ones(C_), (torch.arange(C_) % 9 - 1).to(torch.int32))          # another power of two per channel: 2^-1 .. 2^7
    return gamma, beta, g


# the smallest width; the old kernel's last; the new kernel's first and second (a last group of 1 and 2 lanes' worth behind two full
# 1024-channel pieces); 3072 (three pieces, Swin-L's merge norm); 4096 (all four)
@pytest.mark.parametrize('rows,C_', [(1, 16), (7, 2048), (5, 2052), (9, 2056), (3, 3072), (2, 4096)])
def test_float_layernorm_operator(E, rows, C_):
    """random rows and the edge rows, row_stride / out_stride > C in sentinel arenas, with and without tap_out: codes and taps equal the
    helper's, no byte outside the result is written, bytes [C, out_stride) of a row are untouched"""
    L = E.lib()
    gen = torch.Generator().manual_seed(100 * rows + C_)
    x = torch.clamp(torch.round(torch.randn(rows, C_, generator=gen) * 40.0), -128, 127).long()
    x = torch.cat((x, _edge_rows(C_)), 0)
    n = x.shape[0]
    gamma, beta, g = _constants(C_, C_ + rows)
    s_in, eps = 0.125, R.SWIN_EPS
    want, want_y = float_layernorm(x, s_in, gamma, beta, eps, g)
    gd, bd, ggd = gamma.cuda(), beta.cuda(), g.cuda()
    ln = E.FloatLn(s_in, eps, E.ptr(gd), E.ptr(bd), E.ptr(ggd))

    def run(sentinel):
        got = {}
        for tag, lo, hi in (('random', 0, rows), ('edge', rows, n)):
            xin = Arena(hi - lo, C_, stride=C_ + 12, sentinel=sentinel, init=x[lo:hi])
            out = Arena(hi - lo, C_, stride=C_ + 8, sentinel=sentinel)
            tap = Arena(hi - lo, C_, dtype=torch.float32, sentinel=sentinel)
            out2 = Arena(hi - lo, C_, stride=C_ + 4, sentinel=sentinel)
            E.check(L.p2v_float_layernorm(xin.ptr, C_ + 12, hi - lo, C_, C.byref(ln), out.ptr, C_ + 8, tap.ptr, E.stream_ptr()))
            E.check(L.p2v_float_layernorm(xin.ptr, C_ + 12, hi - lo, C_, C.byref(ln), out2.ptr, C_ + 4, None, E.stream_ptr()))
            torch.cuda.synchronize()
            xin.read((tag, 'x'))
            got[tag + '/codes'], got[tag + '/tap'], got[tag + '/untapped'] = out.read((tag, 'out')), tap.read((tag, 'tap')), out2.read((tag, 'out2'))
        return got

    got = twice(run)
    codes = torch.cat((got['random/codes'], got['edge/codes']), 0).long()
    tap = torch.cat((got['random/tap'], got['edge/tap']), 0)
    d = codes - want
    print('rows %d C %d: %d of %d codes differ from the helper' % (rows, C_, int((d != 0).sum()), d.numel()))
    assert torch.equal(codes, want)
    assert torch.equal(torch.cat((got['random/untapped'], got['edge/untapped']), 0).long(), want)
    assert np.array_equal(tap.numpy().view(np.uint32), want_y.numpy().view(np.uint32))
    for k in (0, 1, 2):                                   # the constant rows: variance exactly 0, y = beta
        assert torch.equal(got['edge/tap'][k], beta)
    assert C_ == 16 or (int(want.min()) == -128 and int(want.max()) == 127)          # both saturations occur


def test_float_layernorm_refusals(E):
    """C = 2050 (no multiple of 4) and C = 4100 (beyond the kernels), and rows that overlap beyond 2048 channels: refused, nothing launched"""
    L = E.lib()
    z = torch.zeros(4100, device='cuda')
    x = torch.zeros(2, 4100, dtype=torch.int8, device='cuda')
    out = torch.full((2, 4100), 0x5A, dtype=torch.int8, device='cuda')
    ok = E.FloatLn(0.125, 1e-5, E.ptr(z), E.ptr(z), E.ptr(z))
    st = E.stream_ptr()
    assert L.p2v_float_layernorm(E.ptr(x), 4100, 2, 2050, C.byref(ok), E.ptr(out), 4100, None, st) == E.E_UNSUPPORTED
    assert L.p2v_float_layernorm(E.ptr(x), 4100, 2, 4100, C.byref(ok), E.ptr(out), 4100, None, st) == E.E_SHAPE
    assert b'C=4100' in L.p2v_last_error()
    assert L.p2v_float_layernorm(E.ptr(x), 2048, 2, 2052, C.byref(ok), E.ptr(out), 4100, None, st) == E.E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    E.check(L.p2v_float_layernorm(E.ptr(x), 4100, 2, 4096, C.byref(ok), E.ptr(out), 4100, None, st))      # and the call itself is sound
    torch.cuda.synchronize()
    assert bool((out[:, :4096] == 0).all()) and bool((out[:, 4096:] == 0x5A).all())


@pytest.mark.parametrize('rows,C_', [(6, 384), (4, 3072)])
def test_record_kind_equals_the_entry_point(E, rows, C_):
    """P2V_OP_FLOAT_LAYERNORM through p2v_run_ops, with and without the tap: the bytes of the direct call (both kernels)"""
    L = E.lib()
    gen = torch.Generator().manual_seed(C_)
    x = torch.clamp(torch.round(torch.randn(rows, C_ + 16, generator=gen) * 40.0), -128, 127).to(torch.int8).cuda()
    gamma, beta, g = (t.cuda() for t in _constants(C_, 5))
    ln = E.FloatLn(2.0 ** -4, R.SWIN_EPS, E.ptr(gamma), E.ptr(beta), E.ptr(g))
    direct = torch.full((rows, C_ + 32), 0x5A, dtype=torch.int8, device='cuda')
    tap = torch.full((rows, C_), 7.0, device='cuda')
    E.check(L.p2v_float_layernorm(E.ptr(x), C_ + 16, rows, C_, C.byref(ln), E.ptr(direct), C_ + 32, E.ptr(tap), E.stream_ptr()))
    want, want_y = float_layernorm(x[:, :C_].cpu(), 2.0 ** -4, gamma.cpu(), beta.cpu(), R.SWIN_EPS, g.cpu())
    for with_tap in (True, False):
        got = torch.full_like(direct, 0x5A)
        tap2 = torch.full_like(tap, 7.0)
        o = E.Op()
        o.kind, o.inp, o.out = E.OP_FLOAT_LAYERNORM, E.ptr(x), E.ptr(got)
        o.M, o.N, o.lda, o.ldo, o.f0, o.f1 = rows, C_, C_ + 16, C_ + 32, ln.s_in, ln.eps
        o.lin.w_codes, o.lin.colscale, o.lin.bias = ln.gamma, ln.beta, ln.g
        if with_tap:
            o.ep.tap_out = E.ptr(tap2)
        E.check(L.p2v_run_ops(C.byref(o), 1, E.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(got, direct) and bool((got[:, C_:] == 0x5A).all())
        assert torch.equal(got[:, :C_].cpu().long(), want)
        assert torch.equal(tap2, tap if with_tap else torch.full_like(tap, 7.0))
    assert np.array_equal(tap.cpu().numpy().view(np.uint32), want_y.numpy().view(np.uint32))


# ---- 2. the plans -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world(dva, E):
    """per configuration: the micro Swin calibrated under Config(False, lis) with its plan, three images, the widths (8, 4, one mixed
    list of _swin_bits_ref.bit_lists) and the restatement's logits and taps for each, computed once"""
    w = {}
    for tag, cfg in R.CONFIGS.items():
        m, x = R.micro_swin(dva, cfg)
        L = m.bit_config_length()
        lists = [8, 4, RB.bit_lists(L)[3]]
        want, taps = [], []
        for bl in lists:
            t = {}
            want.append(R.quant_forward(m.arch, m.state_dict(), m.export_calib(), x, bl, t, lis=cfg[1]) if isinstance(bl, int) else
                        R.mixed_forward(m, x, bl, t, lis=cfg[1]))
            taps.append(t)
        m.cuda()
        plan = m.freeze('cuda', bits=8)
        assert plan.int_norm is False and plan.int_softmax is cfg[1]
        w[tag] = dict(m=m, x=x.cuda(), plan=plan, L=L, lists=lists, want=want, taps=taps, cfg=cfg)
    return w


def _kinds(plan):
    return [int(r['ops'][i].kind) for r in plan._recorded.values() for i in range(r['n'])]


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_plan_logits_equal_the_restatement(E, world, tag):
    """bits = 8, bits = 4 and one mixed list; every LayerNorm of every recorded sequence is the float one"""
    w = world[tag]
    m, x = w['m'], w['x']
    with torch.no_grad():
        for bl, want in zip(w['lists'], w['want']):
            got = m(x, bits=bl).cpu()
            assert torch.equal(got, want), (tag, bl, float((got - want).abs().max()))
        m(x, bits=8)
    assert m._plan is w['plan']
    assert len({t.numpy().tobytes() for t in w['want']}) == len(w['want'])          # the widths are told apart
    kinds = _kinds(w['plan'])
    norms = 1 + 2 * sum(m.arch['depths']) + (len(m.arch['depths']) - 1) + 1
    assert kinds.count(E.OP_LAYERNORM) == 0 and kinds.count(E.OP_LN_GEMM) == 0 and kinds.count(E.OP_FLOAT_LAYERNORM) == norms * len(w['plan']._recorded)
    assert (kinds.count(E.OP_WINATTN) == 0) is (not w['cfg'][1]) and (kinds.count(E.OP_WINATTN_SOFTMAX) == 0) is w['cfg'][1]
    assert not torch.equal(w['want'][0], world['ff' if tag == 'ft' else 'ft']['want'][0])       # and the two configurations


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_every_tap_equals_the_restatement(world, tag):
    """forward(taps=...) at the plan's default width 8 and 4: every tapped QAct, code for code"""
    w = world[tag]
    m, plan, x = w['m'], w['plan'], w['x']
    with torch.no_grad():
        for k, bits in enumerate((8, 4)):
            m(x, bits=bits)                               # moves the plan's default width
            t = {}
            out = plan.forward(x, taps=t)
            assert torch.equal(out.cpu(), w['want'][k])
            blocks, merges = sum(m.arch['depths']), len(m.arch['depths']) - 1
            assert len(t) == 3 * blocks + merges + 3
            for nm, got in t.items():
                ref = w['taps'][k][nm]
                ref = ref.reshape(-1, ref.shape[-1])
                assert torch.equal(got[:, :ref.shape[1]].cpu().to(torch.int32), ref), (tag, bits, nm)
        m(x, bits=8)


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_uint8_sliced_and_profile(dva, world, tag):
    from diff_vit_amd import data
    w = world[tag]
    m, plan = w['m'], w['plan']
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u8 = dva.synth.images_uint8(7, 2, 56)
    bl = w['lists'][2]
    with torch.no_grad():
        for bits in (8, 4, bl):
            assert torch.equal(m.forward_uint8(u8.cuda(), bits, mean, std, 'NHWC'), m(data.normalize_uint8(u8, mean, std, 'NHWC').cuda(), bits=bits))
        m(w['x'], bits=8)
        xs = dva.synth.images(23, 48, 56).cuda()              # 48 >= 16 * 3: three slices on three streams
        single = plan.forward(xs, n_streams=1)
        assert torch.equal(plan.forward(xs, n_streams=3), single) and torch.equal(plan.forward(xs, n_streams=3), single)
        assert torch.equal(plan.forward(xs, n_streams=3, slices=[20, 15, 13], bit_config=bl), plan.forward(xs, n_streams=1, bit_config=bl))
        assert torch.equal(single[:3].cpu(), plan.forward(xs[:3]).cpu())
        assert torch.equal(plan.forward(w['x']).cpu(), w['want'][0])
        names = [k for k, _, _ in plan.profile(w['x'])]
    assert 'float_layernorm' in names and 'layernorm' not in names and 'ln_gemm' not in names


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_forward_ddv_sums_equal_those_of_the_taps(dva, world, tag):
    """every stage of forward_ddv (with and without the linear layers) against pair_cosine_cpu on the restatement's values, in the manner
    of tests/test_swin_modeldiff_gpu.py; the linear taps, the hooked forward's source, are those values too"""
    from test_swin_modeldiff_gpu import _close, _pairs, oracle_stages
    D = dva.ddv
    w = world[tag]
    m, plan = w['m'], w['plan']
    n = 2
    x, xa = _pairs(dva, n, 56)
    x2 = torch.cat((x, xa), 0)
    mp = R.patched(w['cfg'][1])
    try:
        with torch.no_grad():
            st, ref = oracle_stages(R.model_view(m), x2, 8)
    finally:
        mp.undo()
    with torch.no_grad():
        fwd = m(x2.cuda(), bits=8).cpu()
        assert torch.equal(fwd, ref)
        for with_linear in (True, False):
            logits, names, sums = plan.forward_ddv(x2.cuda(), with_linear)
            assert names == D.swin_stage_names(m.arch['depths'], with_linear) and torch.equal(logits.cpu(), fwd)
            sums = sums.cpu()
            for k, nm in enumerate(names):
                v, sc, is_f = st[nm]
                if is_f:
                    _close(sums[k], D.pair_cosine_cpu([v[:n].float()], [v[n:].float()])[0], 1e-9, (tag, nm))
                elif sc is None:
                    assert torch.equal(sums[k], D.pair_cosine_cpu([v[:n].to(torch.int32)], [v[n:].to(torch.int32)])[0]), (tag, nm)
                else:      # one scale repeated over the channels
                    _close(sums[k], D.pair_cosine_cpu([v[:n].to(torch.int32)], [v[n:].to(torch.int32)], [sc])[0], 1e-12, (tag, nm))
        d = D.compute_ddv(m, x.cuda(), xa.cuda(), 8, with_linear=False)
        assert list(d) == D.swin_stage_names(m.arch['depths'], False)
        out, lin = plan.forward_linear_taps(x2.cuda())
        assert torch.equal(out.cpu(), fwd) and len(lin) == w['L']
        for nm, t in zip(plan.linear_tap_names(), lin):
            assert torch.equal(t.cpu().reshape(t.shape[0], -1), st[nm][0]), (tag, nm)
        seen = []
        hooks = [mod.register_forward_hook(lambda mod_, i, o, nm=nm: seen.append(nm)) for nm, mod in m.linear_modules()]
        assert torch.equal(m(x2.cuda()).cpu(), fwd) and seen == plan.linear_tap_names()
        for h in hooks:
            h.remove()


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_attention_stages_statistics_and_grams(dva, world, tag):
    """attention=True is served under (False, True) and refused under (False, False), as under ptf=True; compute_stats and the stage
    Grams of the CKA run the same recorded sequence and return forward's logits"""
    D = dva.ddv
    w = world[tag]
    m, plan, x = w['m'], w['plan'], w['x']
    x4 = torch.cat([x[:2], x[:2] + 0.01])
    with torch.no_grad():
        m(x, bits=8)
        if w['cfg'][1]:
            lg, names, sums = plan.forward_ddv(x4, with_linear=False, attention=True)
            assert names == D.swin_stage_names(m.arch['depths'], False, attention=True) and torch.equal(lg, plan.forward(x4))
            plain = plan.forward_ddv(x4, with_linear=False)
            keep = [k for k, nm in enumerate(names) if nm in plain[1]]
            assert torch.equal(sums[keep], plain[2]) and bool(torch.isfinite(sums).all())
            assert list(D.compute_ddv(m, x[:2], x[:2] + 0.01, 8, attention=True)) == D.swin_stage_names(m.arch['depths'], True, attention=True)
        else:
            with pytest.raises(NotImplementedError):
                plan.forward_ddv(x4, attention=True)
            with pytest.raises(NotImplementedError):
                D.compute_ddv(m, x[:2], x[:2] + 0.01, 8, attention=True)
        lg, stats = plan.forward_stats(x, with_linear=False)
        assert torch.equal(lg.cpu(), w['want'][0]) and stats.names == D.swin_stage_names(m.arch['depths'], False)
        s2 = dva.stats.compute_stats(m, x, 8, with_linear=False)
        assert s2.names == stats.names
        host = stats.cpu()
        for nm in ('patch_embed.qact', 'layers.0.blocks.1.qact1', 'layers.0.downsample.qact1', 'qact2'):       # float-LayerNorm stages
            rec, ref = host.record(nm), w['taps'][0][nm].long()
            ref = ref.reshape(-1, ref.shape[-1])
            assert int(rec['count']) == ref.numel() and torch.equal(rec['sum'], ref.sum(0)) and torch.equal(rec['sumsq'], (ref * ref).sum(0)), nm
            assert torch.equal(rec['lo'].long(), ref.min(0)[0]) and torch.equal(rec['hi'].long(), ref.max(0)[0]), nm
        # the CKA of a Swin model reads the linear layers through the hooked forward
        xc = dva.synth.images(31, 6, 56)                  # (the Gram kernels take 4 ... 256 images)
        acts = dva.get_activations(xc, m, 8, 'cuda')
        assert len(acts) == w['L']
        heat = dva.compute_cka(m, m, [xc], 8, 8)
        assert tuple(heat.shape) == (w['L'], w['L']) and bool(torch.isfinite(heat).all())
        assert float((torch.diagonal(heat).cpu() - 1).abs().max()) <= 1e-4


def test_plan_refuses_a_scale_that_is_no_power_of_two(dva, world):
    """where the plan is created, naming the module - also for the QActs that are PTF vectors under ptf=True"""
    m = world['ft']['m']
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    for name in ('layers.0.blocks.1.qact2', 'layers.1.blocks.0.qact4', 'layers.0.downsample.qact2', 'layers.0.blocks.0.qact1'):
        calib = dict(m.export_calib())
        calib[name] = calib[name] * 1.5
        with pytest.raises(NotImplementedError, match=name.replace('.', r'\.')):
            dva.SwinPlan(m.arch, sd, calib, device='cuda', int_norm=False)
    assert dva.SwinPlan(m.arch, sd, m.export_calib(), device='cuda', int_norm=False).int_norm is False


@pytest.mark.parametrize('tag', sorted(R.CONFIGS))
def test_wide_model_takes_the_xwide_kernel_in_a_plan(dva, E, tag):
    """stage width 544 (17 heads of 32), depths (1, 1), 56^2 input: the merge norm has 4 * 544 = 2176 channels, beyond the row-per-wave
    kernel; logits and taps equal the restatement's"""
    cfg = R.CONFIGS[tag]
    m, x = R.micro_swin(dva, cfg, n_images=2, embed_dim=544, depths=(1, 1), num_heads=(17, 34))
    assert m.layers[0].downsample.norm.weight.shape == (2176,)
    t = {}
    want = R.quant_forward(m.arch, m.state_dict(), m.export_calib(), x, 8, t, lis=cfg[1])
    m.cuda()
    with torch.no_grad():
        got = m(x.cuda(), bits=8).cpu()
        assert torch.equal(got, want), float((got - want).abs().max())
        gt = {}
        assert torch.equal(m._plan.forward(x.cuda(), taps=gt).cpu(), want)
    for nm, g_ in gt.items():
        ref = t[nm].reshape(-1, t[nm].shape[-1])
        assert torch.equal(g_[:, :ref.shape[1]].cpu().to(torch.int32), ref), nm
    r = m._plan._recorded[(2, 0, True)]
    widths = [int(r['ops'][i].N) for i in range(r['n']) if int(r['ops'][i].kind) == E.OP_FLOAT_LAYERNORM]
    assert widths == [544, 544, 544, 2176, 1088, 1088, 1088]


def test_default_path_did_not_move(dva, E, world):
    """a plan of the (True, True) model built AFTER the ptf=False plans, in the same process: logits byte-identical to the oracle, integer
    LayerNorm records only"""
    assert all(w['plan'].int_norm is False for w in world.values())
    m, x = RB.micro_swin(dva)
    want8, want4 = RB.uniform_oracle(m, x, 8), RB.uniform_oracle(m, x, 4)
    m.cuda()
    with torch.no_grad():
        assert torch.equal(m(x.cuda(), bits=8).cpu(), want8) and torch.equal(m(x.cuda(), bits=4).cpu(), want4)
    assert m._plan.int_norm is True
    kinds = _kinds(m._plan)
    assert kinds.count(E.OP_FLOAT_LAYERNORM) == 0 and kinds.count(E.OP_LAYERNORM) + kinds.count(E.OP_LN_GEMM) > 0
