"""GPU: the FULL DDV stage set on the engine (P2V_DDV_STAGES_FULL, every hook point of the reference's modeldiff_p2.add_hooks).

  operator level    the packed-int4 RESID mid-code tap, the EMBED mid-code taps and the LayerNorm value tap in sentinel arenas
  whole model       FrozenPlan.forward_ddv(stages='full') against oracle values (tests/_ddv_full_ref.py) on the micro-ViT and on the DeiT-S
                    architecture; compute_ddv(fused model, stages='full') against the REAL reference's 30 keys; the call's footprint; refusals

Tolerances (those of test_ddv_gpu.py): one-scale int8 stages are exact integer sums, compared bit for bit; the per-channel stages
(attn.qact3, mlp.qact2) sum the fp32 products code * s_mid[c] in fp64 in another order than the restatement, 1e-12 relative; the fp32
LayerNorm stages 1e-9 of sqrt(aa bb); a DDV entry against the reference 1e-9."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from _arena import SENTINELS, Arena, twice
from _ddv_full_ref import check_stage, full_stage_values, load_reference_calibration
from _tuning import tuning
from conftest import golden_calib, gpu_ok, load_golden
from test_ddv import micro_model
from test_forward_state_gpu import Map, _cfg, _same_bits
from test_kernel_edges_gpu import Layer, Norm, _codes, _embed_case, _gen, _q8

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------
# 1. the packed-int4 RESID mid-code tap
# --------------------------------------------------------------------------------------------------
RESID_MS = (1, 17, 395)


@functools.lru_cache(maxsize=None)
def _resid_case4(N, K):
    """a 4-bit layer whose first quotient covers the whole code range and its clamp edges: in row 0 (no activations) the bias puts columns
    0 .. 5 exactly on +-127.5, +-128.5 and +-126.5 codes of a dyadic s_mid (ties and the clamp boundaries); everywhere else s_mid, s_res,
    s_next are non-power-of-two PTF scales"""
    import p2vit_oracle as O
    gen = _gen(4000 + 100 * N + K)
    rows = max(RESID_MS)
    x = _codes(gen, (rows, K), 40.0)
    x[0] = 0
    w = _codes(gen, (N, K), 3.5, -8, 7)
    ptf = lambda base: base * 2.0 ** torch.randint(0, 4, (N,), generator=gen).float()
    s_mid, s_res, s_next = ptf(0.0131), ptf(0.0173), ptf(0.0209)
    s_mid[:6] = 2.0 ** -5
    s_x, s_w = 2.0 ** -6, torch.full((N,), 2.0 ** -4)
    bias = torch.randn(N, generator=gen) * 0.2
    bias[:6] = torch.tensor([127.5, -128.5, 126.5, -127.5, 128.5, -126.5]) * 2.0 ** -5
    res = _codes(gen, (rows, N), 50.0)
    y = O.qgemm(x, torch.tensor(s_x), w, s_w, bias)
    q3 = _q8(y / s_mid)
    out = _q8((res * s_res + q3 * s_mid) / s_next)
    return dict(x=x, w=w, s_x=s_x, s_w=s_w, bias=bias, s_mid=s_mid, s_res=s_res, s_next=s_next, res=res, q3=q3, out=out)


@pytest.mark.parametrize('N,K', [(96, 64), (272, 192)])
def test_resid_mid_codes_packed_int4(dva, N, K):
    """p2v_gemm_resid_tap on packed int4 weights: the mid codes equal q8(qgemm(...) / s_mid) of the oracle, `out` equals the launch without
    the tap (p2v_gemm_i8) byte for byte, and in sentinel arenas (ldo = N + 16) the columns [N, ldo) and everything around both outputs stay
    untouched - both tile heights, with and without the pre-folded table, M = 1, 17 and 395 (ragged last tile at either height)"""
    E = dva.engine
    L = E.lib()
    c = _resid_case4(N, K)
    assert float(c['q3'].max()) == 127 and float(c['q3'].min()) == -128 and 0.02 < float((c['q3'].abs() >= 127).float().mean()) < 0.6
    assert c['q3'][0, :6].tolist() == [127, -128, 126, -128, 127, -126]            # ties to even, then the clamp
    n_pad = (N + 127) // 128 * 128
    wp = torch.zeros(n_pad, K, dtype=torch.int8)
    wp[:N] = c['w'].to(torch.int8)
    pad = lambda v: torch.cat([v.float(), torch.zeros(n_pad - N)]).cuda()
    d = dict(w=E.pack_int4_tiles(wp).cuda(), cs=pad(c['s_x'] * c['s_w']), b=pad(c['bias']), s_mid=c['s_mid'].cuda(), s_res=c['s_res'].cuda(),
             s_next=c['s_next'].cuda())
    lin = E.Linear(E.ptr(d['w']), E.ptr(d['cs']), E.ptr(d['b']), None, 1)
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
        if tap:
            E.check(L.p2v_gemm_resid_tap(a.ptr, K, M, K, N, C.byref(lin), C.byref(epi), out.ptr, ldo, mid.ptr, E.stream_ptr()))
        else:
            E.check(L.p2v_gemm_i8(E.EPI_RESID, a.ptr, K, M, K, N, C.byref(lin), C.byref(epi), out.ptr, ldo, None, E.stream_ptr()))
        _sync()
        what = (M, N, K, tap, with_tab)
        a.read(('x', what)), res.read(('residual', what))
        r = dict(out=out.read(('out', what)))
        if tap:
            r['mid'] = mid.read(('mid', what))
        return r

    for tile in (128, 256):
        for pre in (0, 1):
            with tuning(L, gemm_tile=tile, resid_pre=pre):
                for M in RESID_MS:
                    with_tab = bool(usable.value)
                    plain = twice(lambda s: run(s, M, False, with_tab))
                    tapped = twice(lambda s: run(s, M, True, with_tab))
                    key = (tile, pre, M)
                    assert torch.equal(tapped['mid'].float(), c['q3'][:M]), (key, int((tapped['mid'].float() != c['q3'][:M]).sum()))
                    assert torch.equal(tapped['out'], plain['out']), key
                    assert torch.equal(plain['out'].float(), c['out'][:M]), key
    one = C.c_void_p(256)
    epi0.residual = one
    assert L.p2v_gemm_resid_tap(one, K, 1, K, N, C.byref(lin), C.byref(epi0), one, ldo, C.c_void_p(264), None) == E.E_ARG
    assert L.p2v_gemm_resid_tap(one, K, 1, K, N, C.byref(lin), C.byref(epi0), one, ldo, None, None) == E.E_ARG


# --------------------------------------------------------------------------------------------------
# 2. the EMBED mid-code taps
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('N', [64, 208])
def test_embed_mid_codes_operator(dva, oracle, N, w4):
    """p2v_gemm_embed_tap, batch 3 x 50 patches (two row tiles, the second ragged), K = 192: pe_codes = clamp(rne(y * inv_s_pe)),
    embed_codes = clamp(rne(pe_codes * pe_to_embed)) at row b * 51 + 1 + p of their planes; `out` byte-identical to p2v_gemm_i8(EMBED); the
    class-token rows of all three, the columns [N, ldo) and everything around them keep the sentinel"""
    E = dva.engine
    L = E.lib()
    B, P, K = 3, 50, 192
    M = B * P
    lay = Layer(E, oracle, *_embed_case(_gen(4800 + N), K, N, w4, B, P))
    p = lay.p
    q1 = _q8(lay.y[:M] * p['inv_s_pe'])
    q2 = _q8(q1 * p['pe_to_embed'])
    ref = lay.reference(oracle, 'embed', M)['out']
    assert q1.max() == 127 and q1.min() == -128 and len(torch.unique(q2)) > 60
    kind, epi = lay.epilogue('embed')

    def run(sentinel, ldo, tap):
        a = Arena(M, K, K, torch.int8, sentinel, init=lay.x[:M])
        planes = [Arena(B * (P + 1), N, ldo, torch.int8, sentinel) for _ in range(3 if tap else 1)]
        if tap:
            E.check(L.p2v_gemm_embed_tap(a.ptr, K, M, K, N, C.byref(lay.lin), C.byref(epi), planes[0].ptr, ldo, planes[1].ptr, planes[2].ptr,
                                         E.stream_ptr()))
        else:
            E.check(L.p2v_gemm_i8(kind, a.ptr, K, M, K, N, C.byref(lay.lin), C.byref(epi), planes[0].ptr, ldo, None, E.stream_ptr()))
        _sync()
        what = ('embed tap', N, w4, ldo, tap)
        assert torch.equal(a.read(('A', what)).float(), lay.x[:M])
        sv = float(np.int8(np.uint8(sentinel)))
        res = {}
        for name, ar in zip(('out', 'pe', 'embed'), planes):
            full = ar.read((name, what)).float().reshape(B, P + 1, N)
            assert bool((full[:, 0] == sv).all()), (name, 'a class-token row was written', what)
            res[name] = full[:, 1:].reshape(M, N).contiguous()
        return res

    for ldo in (N, N + 16):
        plain = twice(lambda s: run(s, ldo, False))
        got = twice(lambda s: run(s, ldo, True))
        assert torch.equal(got['out'], plain['out']) and torch.equal(plain['out'], ref), (N, w4, ldo)
        assert torch.equal(got['pe'], q1), (N, w4, ldo, int((got['pe'] != q1).sum()))
        assert torch.equal(got['embed'], q2), (N, w4, ldo, int((got['embed'] != q2).sum()))


# --------------------------------------------------------------------------------------------------
# 3. the LayerNorm value tap
# --------------------------------------------------------------------------------------------------
def _run_ln_tap(E, norm, codes, tap, sentinel):
    rows, C_ = codes.shape
    a = Arena(rows, C_, C_, torch.int8, sentinel, init=codes)
    out = Arena(rows, C_, C_ + 20, torch.int8, sentinel)
    vals = Arena(rows, C_, C_, torch.float32, sentinel) if tap else None
    L = E.lib()
    if tap:
        E.check(L.p2v_int_layernorm_tap(a.ptr, C_, rows, C_, C.byref(norm.ln), out.ptr, C_ + 20, vals.ptr, E.stream_ptr()))
    else:
        E.check(L.p2v_int_layernorm(a.ptr, C_, rows, C_, C.byref(norm.ln), out.ptr, C_ + 20, E.stream_ptr()))
    _sync()
    what = ('layernorm tap', rows, C_, tap)
    assert torch.equal(a.read(('x', what)).float(), codes)
    r = dict(out=out.read(('out', what)).float())
    if tap:
        r['tap'] = vals.read(('tap', what))
    return r


@pytest.mark.parametrize('chain', ['pot', 'div'])
@pytest.mark.parametrize('C_', [64, 384, 768, 2048])
def test_layernorm_value_tap(dva, oracle, C_, chain):
    """p2v_int_layernorm_tap at C = 64 (one row per half wave), 384, 768 (a row per wave) and 2048, M = 1 and 37: tap = the oracle's UNCLAMPED
    integer times out_scale, bit for bit (an integer below 2^24 times a power of two, or - chain 'div', the generic chain - one fp32
    rounding, the reference's own); the int8 codes byte-identical to p2v_int_layernorm's; with the constants folded ahead and not, and with
    the generic chain forced.  gamma is scaled up on a few channels so that |x_q| goes well beyond 127 (and stays below 2^24)."""
    E = dva.engine
    L = E.lib()
    gen = _gen(5100 + C_)
    norm = Norm(E, gen, C_, chain)
    big = torch.randperm(C_, generator=gen)[:5]
    norm.gamma[big] *= 100.0
    norm.dev[1].copy_(norm.gamma)
    codes = _codes(gen, (37, C_), 35.0)
    s1 = torch.tensor(np.float32(norm.s1))
    xq = codes * norm.mask.reshape(1, -1)
    o = oracle.int_layernorm((xq * s1).unsqueeze(0), torch.full((C_,), float(s1)), norm.gamma, norm.beta, norm.out_scale)[0]
    assert bool(torch.isfinite(o).all()) and float(o.abs().max()) < 2.0 ** 24
    assert float(o[:, big].abs().max()) > 5 * 127 and int((o.abs() > 127).sum()) >= 37, 'the tap must differ from the clamped codes'
    want = o * norm.out_scale.float().reshape(1, -1)
    for rows, pre, generic in itertools.product((1, 37), (False, True), (0, 1)):
        norm.prefold(pre)
        assert L.p2v_set_tuning(b'ln_generic', generic) == 0
        try:
            plain = twice(lambda s: _run_ln_tap(E, norm, codes[:rows], False, s))
            got = twice(lambda s: _run_ln_tap(E, norm, codes[:rows], True, s))
        finally:
            assert L.p2v_set_tuning(b'ln_generic', 0) == 0
        key = (C_, chain, rows, pre, generic)
        assert torch.equal(got['out'], plain['out']), key
        assert np.array_equal(got['tap'].numpy().view(np.uint32), want[:rows].numpy().view(np.uint32)), (key, float((got['tap'] - want[:rows]).abs().max()))
    norm.prefold(False)


# --------------------------------------------------------------------------------------------------
# 4. the whole model
# --------------------------------------------------------------------------------------------------
def _check_full(dva, O, plan, arch, W, c, x, bits, tag):
    depth = arch['depth']
    n = x.shape[0] // 2
    xc = x.cuda()
    logits, names, sums = plan.forward_ddv(xc, bits, with_linear=True, stages='full')
    assert names == dva.ddv.stage_names(depth, True, True) and sums.shape == (13 * depth + 8, n, 3)
    assert torch.equal(logits, plan.forward(xc, bits)), 'the logits are p2v_forward\'s'
    logits0, names0, sums0 = plan.forward_ddv(xc, bits, with_linear=False, stages='full')
    assert names0 == dva.ddv.stage_names(depth, False, True) and sums0.shape == (9 * depth + 7, n, 3) and torch.equal(logits0, logits)
    assert torch.equal(sums, plan.forward_ddv(xc, bits, with_linear=True, stages='full')[2]), 'bitwise repeatable'
    by = dict(zip(names, sums.cpu().numpy()))
    for k, nm in enumerate(names0):                                              # with_linear does not touch the other stages' bits
        assert np.array_equal(sums0[k].cpu().numpy(), by[nm]), nm
    # the stages shared with the engine list: the same bits in both modes
    for lin in (False, True):
        _, en, es = plan.forward_ddv(xc, bits, with_linear=lin)
        assert en == dva.ddv.stage_names(depth, lin)
        for k, nm in enumerate(en):
            assert np.array_equal(es[k].cpu().numpy(), by[nm]), (tag, nm)
    vals, block_norm_ints, _, ref_logits = full_stage_values(O, arch, W, c, x, bits)
    assert torch.equal(logits.cpu(), ref_logits)
    # the precondition that tells a clamped LayerNorm tap from the hooked value
    beyond = sum(int((t.abs() > 127).sum()) for t in block_norm_ints)
    print(tag, 'unclamped block-norm integers beyond int8:', beyond)
    assert beyond > 0
    assert set(vals) == set(names) - set(dva.ddv.stage_names(depth, True))
    for nm, (v, sc) in vals.items():
        check_stage(nm, by[nm], v, sc, tag)


def _fused_micro(dva, synth):
    g = load_golden('micro_vit')
    m = micro_model(dva, synth, g).cuda()
    dva.harness.calibrate_model(m, torch.from_numpy(g['x_cal']).cuda())
    return m, g


def test_forward_ddv_full_micro_vit(dva, oracle, synth):
    m, g = _fused_micro(dva, synth)
    k = load_golden('ddv_micro')
    x = torch.cat((torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])), 0)
    m(x.cuda(), [8] * 10, False)                               # freezes the plan
    sd = {kk[2:]: torch.from_numpy(g[kk]) for kk in g.files if kk.startswith('w/')}
    c = m.export_calib()
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10), ('qmix', [int(b) for b in g['bit_qmix']])):
        _check_full(dva, oracle, m._plan, synth.ARCHS['micro'], sd, c, x, bits, tag)
    with pytest.raises(ValueError):
        m._plan.forward_ddv(x.cuda(), [8] * 10, stages='all')


def test_forward_ddv_full_deit_small(dva, oracle, synth):
    """4 + 4 images of 224 x 224: T = 197, K = 1536 in fc2, the packed-int4 fragment and tile paths"""
    g = load_golden('deit_small')
    arch = synth.ARCHS['deit_small']
    sd = synth.vit_state_dict(arch, int(g['seed']))
    c = golden_calib(g, oracle)
    plan = dva.FrozenPlan(arch, sd, c, device=torch.device('cuda:0'))
    x = synth.images(int(g['seed']), 8, 224, offset=1000)
    L = 4 * arch['depth'] + 2
    for tag, bits in (('q8', [8] * L), ('q4', [4] * L), ('qmix', [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)])):
        _check_full(dva, oracle, plan, arch, sd, c, x, bits, tag)


def test_full_ddv_matches_reference(dva, oracle, synth, monkeypatch):
    """compute_ddv(fused micro model, stages='full') against the REAL reference's DDVs on all 30 keys, within 1e-9 (the engine's codes are
    the reference's bit for bit at micro size; with the reference's calibration in the model - load_reference_calibration says why - only the
    fp64 summation order differs), with ONE engine call and no hooked forward"""
    m, g = _fused_micro(dva, synth)
    print('QAct scales that differed from the reference\'s calibration:', load_reference_calibration(m, golden_calib(g, oracle)))
    k = load_golden('ddv_micro')
    x, xa = torch.from_numpy(k['x']), torch.from_numpy(k['x_adv'])
    calls = {'engine': 0, 'hooks': 0}
    real_ddv, real_hooks = dva.FrozenPlan.forward_ddv, dva.ddv._hooked_outputs

    def spy_ddv(self, *a, **kw):
        calls['engine'] += 1
        return real_ddv(self, *a, **kw)

    def spy_hooks(*a, **kw):
        calls['hooks'] += 1
        return real_hooks(*a, **kw)
    monkeypatch.setattr(dva.FrozenPlan, 'forward_ddv', spy_ddv)
    monkeypatch.setattr(dva.ddv, '_hooked_outputs', spy_hooks)
    RK = dva.ddv.FULL_REFERENCE_KEYS
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10)):
        calls.update(engine=0, hooks=0)
        d = dva.compute_ddv(m, x, xa, bits, stages='full')
        assert calls == {'engine': 1, 'hooks': 0}, calls
        assert all(v.is_cuda and v.dtype == torch.float64 for v in d.values())
        assert list(d) == dva.ddv._with_qact_pos(dva.ddv.stage_names(2, True, True))
        keys = [str(v) for v in k['keys/' + tag]]
        assert len(keys) == 30
        worst = {}
        for r in keys:
            got, want = d[RK[r]].cpu().numpy(), k['ddv64/%s/%s' % (tag, r)]
            assert got.shape == want.shape, r
            worst[r] = float(np.abs(got - want).max())
            print(tag, r, worst[r])
        bad = {r: e for r, e in worst.items() if not e <= 1e-9}
        assert not bad, bad
        # and the printed report over the reference's float DDVs: one line per key
        fp = {r: torch.from_numpy(k['ddv64/fp/' + r]) for r in (str(v) for v in k['keys'])}
        got = dva.ddv.reference_similarity(fp, {r: d[RK[r]] for r in fp})
        assert np.allclose(list(got.values()), k['printed/' + tag], rtol=0, atol=1e-6, equal_nan=True)
    # a -1 entry leaves the fused state: the module graph with hooks, the same keys
    calls.update(engine=0, hooks=0)
    dm = dva.compute_ddv(m, x, xa, [8] * 9 + [-1], stages='full')
    assert list(dm) == list(d) and calls == {'engine': 0, 'hooks': 2} and dm['qact_pos'].tolist() == [1.0]


# --------------------------------------------------------------------------------------------------
# 5. the call's footprint, refusals
# --------------------------------------------------------------------------------------------------
def _ddv_ex(E, pl, x2n, bits, fill, with_linear, stage_set, tap=True, expect=0):
    """p2v_forward_ddv_ex with the workspace (exactly p2v_ddv_workspace_bytes_ex), logits, sums and the tap scratch (exactly
    p2v_ddv_tap_scratch_bytes) in arenas -> (status, logits, sums [stages][n][3], workspace bytes)"""
    L = E.lib()
    n = x2n.shape[0] // 2
    ws = Arena(1, L.p2v_ddv_workspace_bytes(pl._handle, n), None, torch.uint8, fill, offset=0)
    stages = L.p2v_ddv_stage_count_ex(pl._handle, int(with_linear), 1)
    out = Arena(2 * n, pl.arch['num_classes'], None, torch.float32, fill)
    sums = Arena(stages * n, 3, None, torch.float64, fill)
    tb = L.p2v_ddv_tap_scratch_bytes(pl._handle, n)
    tp = Arena(1, tb, None, torch.uint8, fill)
    rc = L.p2v_forward_ddv_ex(pl._handle, E.ptr(x2n), n, _cfg(bits), len(bits), out.ptr, ws.ptr, ws.width, int(with_linear), stage_set,
                              tp.ptr if tap else None, tb if tap else 0, sums.ptr, E.stream_ptr())
    _sync()
    assert rc == expect, (rc, L.p2v_last_error())
    what = ('forward_ddv_ex', n, with_linear, stage_set, hex(fill))
    tp.read(('tap scratch',) + what)
    return rc, out.read(('logits',) + what), sums.read(('sums',) + what).reshape(stages, n, 3), ws.read(('workspace',) + what).numpy().reshape(-1)


@pytest.mark.parametrize('with_linear', [0, 1])
def test_forward_ddv_full_in_arenas(dva, micro, with_linear):
    """one FULL call on three pairs under two fills: nothing outside the workspace, the tap scratch, the sums and the logits is written;
    inside the workspace the alignment gaps between the seven buffers and the trailing 256 bytes (behind the partials) keep the fill; the
    results do not depend on what the buffers held; logits equal to the fixture's, sums equal to a plain-buffer call"""
    E = dva.engine
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    n = x.shape[0] // 2
    mp = Map(E, plan, 2 * n)
    gaps = ~mp.covered()
    assert gaps[-256:].all()
    for tag, bits in (('q8', [8] * plan.n_layers), ('qmix', [int(b) for b in micro['g']['bit_qmix']])):
        _, _, plain = plan.forward_ddv(x, bits, with_linear=bool(with_linear), stages='full')
        _sync()
        for fill in SENTINELS:
            _, out, sums, wsb = _ddv_ex(E, plan, x, bits, fill, with_linear, 1)
            assert _same_bits(out, torch.from_numpy(micro['g']['logits/' + tag])), (tag, hex(fill))
            assert _same_bits(sums, plain.cpu()), (tag, hex(fill), with_linear)
            fwd = wsb[:mp.nbytes]
            assert bool((fwd[gaps] == fill).all()), ('a gap of the workspace was written', tag, hex(fill))


def test_full_refusals_launch_nothing(dva, micro, synth):
    """input_quant = False plan + FULL, FULL without tap_scratch, a bad stage_set: status, message, and every output keeps its sentinel"""
    E = dva.engine
    L = E.lib()
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    bits = [8] * plan.n_layers
    fill = SENTINELS[0]

    def untouched(res):
        _, out, sums, wsb = res
        return bool((out.numpy().view(np.uint8) == fill).all()) and bool((sums.numpy().view(np.uint8) == fill).all()) and bool((wsb == fill).all())
    assert untouched(_ddv_ex(E, plan, x, bits, fill, 1, 2, expect=E.E_ARG)) and b'unknown stage_set 2' in L.p2v_last_error()
    assert untouched(_ddv_ex(E, plan, x, bits, fill, 0, 1, tap=False, expect=E.E_WORKSPACE)) and b'tap_scratch' in L.p2v_last_error()
    with pytest.raises(ValueError):                              # past its own list the entry point runs p2v_forward's checks
        plan.forward_ddv(x, bits[:-1], stages='full')
    fp_plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'], input_quant=False)
    assert fp_plan.inv_s_input == 0.0
    assert untouched(_ddv_ex(E, fp_plan, x, bits, fill, 1, 1, expect=E.E_UNSUPPORTED)) and b'input QAct' in L.p2v_last_error()
    with pytest.raises(NotImplementedError):
        fp_plan.forward_ddv(x, bits, stages='full')
    # the engine list still runs on that plan
    assert fp_plan.forward_ddv(x, bits)[2].shape == (5 * plan.depth + 3, x.shape[0] // 2, 3)
