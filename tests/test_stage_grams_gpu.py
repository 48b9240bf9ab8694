"""GPU: the stage Grams on the MI355X - p2v_code_grams bit for bit against the int64 restatement (tests/_stage_grams_ref.py) with the Grams,
the workspace and the inputs in sentinel arenas, the chunk and overflow edges, the fp32 stages and p2v_cka_centre against the fp64
references of tests/test_cka_gpu.py, then p2v_forward_grams on whole models stage by stage against the staged oracle forwards, and
compute_cka(stages=) end to end.

fp32 stages: the two launches are p2v_cka_grams's, whose Gram rule zeroes the diagonal before anything reads it; the raw fp32 Gram keeps
that zero diagonal (include/p2vit.h), so the bound 4e-6 * max_ij sum |x_i||x_j| is held against the fp64 Gram with a zero diagonal."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _stage_grams_ref as G
from _arena import SENTINELS, Arena, twice
from conftest import golden_calib, load_golden

pytestmark = pytest.mark.gpu

NS = (1, 2, 31, 33, 50, 65)
SHAPES = ((1, 1, 1), (1, 16, 16), (3, 17, 32), (5, 48, 48), (17, 64, 80), (2, 384, 384))      # rows, cols, row_stride


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


def _layer(E, base, rows, cols, ss, rs, shift=None, dtype=0):
    d = E.GramLayer()
    d.base, d.shift, d.sample_stride, d.row_stride, d.rows, d.cols, d.dtype = base, shift, ss, rs, rows, cols, dtype
    return d


def _code_grams(E, layers, n, fill, keep=()):
    """ONE p2v_code_grams call with G and the workspace in arenas -> fp64 [L, n, n] (the guards are checked)"""
    L = E.lib()
    arr = (E.GramLayer * len(layers))(*layers)
    need = L.p2v_code_grams_workspace_bytes(arr, len(layers), n)
    assert need > 0, L.p2v_last_error()
    out = Arena(1, len(layers) * n * n, None, torch.float64, fill)
    ws = Arena(1, need, None, torch.uint8, fill, offset=0)
    rc = L.p2v_code_grams(arr, len(layers), n, out.ptr, ws.ptr, need, E.stream_ptr())
    _sync()
    assert rc == 0, (rc, L.p2v_last_error())
    ws.read(('workspace', hex(fill)))
    return out.read(('grams', hex(fill))).reshape(len(layers), n, n)


def _codes(gen, shape, rails):
    if rails:
        return torch.where(torch.rand(shape, generator=gen) < 0.5, torch.tensor(-128), torch.tensor(127)).to(torch.int8)
    return torch.randint(-128, 128, shape, generator=gen, dtype=torch.int64).to(torch.int8)


def _shift(gen, cols):
    m = torch.randint(0, 4, (cols,), generator=gen).to(torch.uint8)
    m[:min(4, cols)] = torch.arange(4, dtype=torch.uint8)[:min(4, cols)]          # all four values wherever there are four columns
    return m


# --------------------------------------------------------------------------------------------------
# 1. the operator: exact
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', NS)
def test_code_grams_exact(dva, n):
    """every shape x {no shift, shift} x {random codes, rail codes} plus the class-row form in ONE call per fill: inputs, shift bytes,
    Grams and workspace in sentinel arenas under two fills (the row padding is poisoned with two values, nothing outside [L][n][n] is
    written), bit-equal to the int64 restatement, exactly symmetric, and repeated bit for bit"""
    E = dva.engine
    gen = torch.Generator().manual_seed(100 + n)
    cases = []
    for rows, cols, rs in SHAPES:
        for rails in (False, True):
            cases.append((_codes(gen, (n, rows, cols), rails), rs, rows * rs, None))
            cases.append((_codes(gen, (n, rows, cols), rails), rs, rows * rs, _shift(gen, cols)))
    for cols in (16, 17, 384):                             # the class rows of a [tokens][D] plane: rows = 1, samples 5 rows apart
        cases.append((_codes(gen, (n, 1, cols), False), cols, 5 * cols, _shift(gen, cols) if cols != 16 else None))
    want = torch.stack([G.int_gram(c, m).double() for c, _, _, m in cases])

    def run(fill):
        keep, layers = [], []
        for c, rs, ss, m in cases:
            rows, cols = c.shape[1], c.shape[2]
            if ss == rows * rs:
                a = Arena(n * rows, cols, rs, torch.int8, fill, init=c.reshape(n * rows, cols))
            else:
                a = Arena(n, cols, ss, torch.int8, fill, init=c.reshape(n, cols))
            sh = Arena(1, cols, None, torch.uint8, fill, init=m.reshape(1, cols)) if m is not None else None
            keep += [a, sh]
            layers.append(_layer(E, a.ptr.value, rows, cols, ss, rs, sh.ptr.value if sh is not None else None))
        got = _code_grams(E, layers, n, fill)
        for a in keep:
            if a is not None:
                a.read('an input was written')
        return {'grams': got}
    got = twice(run)['grams']
    for k in range(len(cases)):
        G.assert_exact(got[k], want[k], (n, k, tuple(cases[k][0].shape), cases[k][3] is not None))
        assert torch.equal(got[k], got[k].t())


def test_chunk_and_overflow_edges(dva):
    """all codes -128, n = 4, rows = 1: cols = one chunk and one chunk + 16 give exactly cols * 2^14 in every entry (a chunk's int32 sum is
    at most 2^27); shifted by m = 3 across the chunk border cols * 2^14 * 64; a rows x cols walk whose chunk border falls inside a row"""
    E = dva.engine
    C = E.GRAM_CHUNK
    layers, keep, want = [], [], []
    for cols in (C, C + 16):
        x = torch.full((4, cols), -128, dtype=torch.int8, device='cuda')
        keep.append(x)
        layers.append(_layer(E, x.data_ptr(), 1, cols, cols, cols))
        want.append(torch.full((4, 4), float(cols * 2 ** 14), dtype=torch.float64))
    x = torch.full((4, C + 16), -128, dtype=torch.int8, device='cuda')
    m3 = torch.full((C + 16,), 3, dtype=torch.uint8, device='cuda')
    keep += [x, m3]
    layers.append(_layer(E, x.data_ptr(), 1, C + 16, C + 16, C + 16, m3.data_ptr()))
    want.append(torch.full((4, 4), float((C + 16) * 2 ** 14 * 64), dtype=torch.float64))
    gen = torch.Generator().manual_seed(7)
    r = _codes(gen, (4, 27, 1000), False)                  # 63 groups a row: chunk borders inside rows, a scalar tail in every row
    m = _shift(gen, 1000)
    rd, md = r.cuda(), m.cuda()
    keep += [rd, md]
    layers.append(_layer(E, rd.data_ptr(), 27, 1000, 27000, 1000, md.data_ptr()))
    want.append(G.int_gram(r, m).double())
    for fill in SENTINELS:
        got = _code_grams(E, layers, 4, fill)
        for k in range(len(layers)):
            G.assert_exact(got[k], want[k], ('edge', k))


def test_the_op_and_views(dva):
    """torch.ops.p2vit.code_grams: a strided [n, rows, cols] view is read in place, anything else through a copy; fp32 tensors as fp32 stages"""
    gen = torch.Generator().manual_seed(3)
    big = _codes(gen, (9, 7, 40), False).cuda()
    view = big[:, 2:7, :33]                                # cols 33, row stride 40, sample stride 280 on a 16-byte aligned base: scalar loads
    assert view.data_ptr() % 16 == 0
    m = _shift(gen, 33).cuda()
    t4 = _codes(gen, (9, 2, 3, 32), False).cuda()
    xf = torch.randn(9, 5, 12, generator=gen).cuda()
    got = torch.ops.p2vit.code_grams([view, view, t4, xf], [None, m, None, None])
    assert got.shape == (4, 9, 9) and got.dtype == torch.float64
    G.assert_exact(got[0], G.int_gram(view.cpu()), 'view')
    G.assert_exact(got[1], G.int_gram(view.cpu(), m.cpu()), 'shifted view')
    G.assert_exact(got[2], G.int_gram(t4.cpu().reshape(9, -1, 32)), '4-d')
    ref, bound = G.f64_gram(xf)
    ref.diagonal().fill_(0)
    assert float((got[3].cpu() - ref).abs().max()) <= 4e-6 * bound
    with pytest.raises(AssertionError):
        torch.ops.p2vit.code_grams([xf], [m])


@pytest.mark.parametrize('n,F', [(1, 5), (4, 1), (5, 63), (50, 4097), (65, 8200)])
def test_fp32_stages(dva, n, F):
    E = dva.engine
    gen = torch.Generator().manual_seed(n + F)
    x = torch.randn(n, F, generator=gen) * 3
    ref, bound = G.f64_gram(x)
    ref.diagonal().fill_(0)
    xd = x.cuda()
    cols = F // 5 if F % 5 == 0 and F > 5 else F
    lays = [_layer(E, xd.data_ptr(), F // cols, cols, F, cols, None, E.GRAM_F32)]
    a = _code_grams(E, lays, n, SENTINELS[0])
    b = _code_grams(E, lays, n, SENTINELS[1])
    assert torch.equal(a, b) and torch.equal(a[0], a[0].t())
    err = float((a[0] - ref).abs().max())
    print('fp32 stage', n, F, 'error', err, 'bound', 4e-6 * bound)
    assert err <= 4e-6 * bound, (n, F, err, bound)


@pytest.mark.parametrize('n', [4, 5, 50])
def test_cka_centre(dva, n):
    """the centring on raw Grams against test_cka_gpu._gram64 (4e-6 * bound, the bound of the fp32 partial kernels), equal to p2v_cka_grams
    on the same activations; the off-diagonal block of a 2n x 2n Gram against the X Y^T form of cka_grams"""
    from test_cka_gpu import _gram64
    gen = torch.Generator(device='cuda').manual_seed(50 + n)
    for F in (1, 300, 4097):
        x, y = torch.randn(n, F, device='cuda', generator=gen), torch.randn(n, F, device='cuda', generator=gen) + 0.25
        raw = torch.ops.p2vit.code_grams([x], [None])
        got = torch.ops.p2vit.cka_centre(raw)
        assert got.shape == (1, n, n) and got.dtype == torch.float32
        ref, bound = _gram64(x, None)
        assert float((got[0].double() - ref).abs().max()) <= 4e-6 * bound, (n, F)
        assert torch.equal(got, torch.ops.p2vit.cka_grams([x], [])), 'the same partials, the same centring'
        big = torch.ops.p2vit.code_grams([torch.cat((x, y), 0)], [None])                # [1, 2n, 2n]
        blk = torch.ops.p2vit.cka_centre(big[:, :n, n:])
        ref, bound = _gram64(x, y)
        xy = torch.ops.p2vit.cka_grams([x], [y])
        print('cka_centre', n, F, 'block equals cka_grams(x, y):', torch.equal(blk, xy))
        assert float((blk[0].double() - ref).abs().max()) <= 4e-6 * bound, (n, F)
        assert float((blk[0].double() - xy[0].double()).abs().max()) <= 4e-6 * bound, (n, F)
    # integer Grams: against the fp64 centring of the exact Gram, one fp32 step at most (fp64 sums in two orders, one cast)
    c = torch.randint(-128, 128, (n, 3, 48), dtype=torch.int64).to(torch.int8).cuda()
    raw = torch.ops.p2vit.code_grams([c], [None])
    G.assert_exact(raw[0], G.int_gram(c.cpu()), 'int')
    want = G.centre(raw[0]).float().numpy()
    got = torch.ops.p2vit.cka_centre(raw)[0].cpu().numpy()
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


# --------------------------------------------------------------------------------------------------
# 2. whole models
# --------------------------------------------------------------------------------------------------
def _check_stage(nm, gram, unit, values, scale, kind, calib, tag):
    want, want_unit, bound = G.stage_gram(values, scale, kind)
    if kind == 'f32':
        want.diagonal().fill_(0)
        err = float((gram - want).abs().max())
        assert err <= 4e-6 * bound, (tag, nm, err, bound)
        assert unit == 1.0, (tag, nm, unit)
        return
    G.assert_exact(gram, want, (tag, nm))
    if scale is None:
        want_unit = float(calib[nm].reshape(-1)[0])
    assert unit == want_unit, (tag, nm, unit, want_unit)


def _check_model(dva, O, plan, arch, W, c, x, bits_list, int_norm, int_softmax, combos, tag, full_ref=False):
    import _float_ops_ref as R
    xc = x.cuda()
    depth = arch['depth']
    for bits in bits_list:
        plain = plan.forward(xc, bits).clone()
        st = {}
        ref_logits = R.quant_forward(O, arch, W, c, x, bits, int_norm, int_softmax, stages=st)
        lin = None
        for stages, with_linear in combos:
            logits, names, grams, units = plan.forward_grams(xc, bits, with_linear=with_linear, stages=stages)
            _sync()
            assert names == dva.ddv.stage_names(depth, with_linear, stages == 'full')
            assert torch.equal(logits, plain) and torch.equal(logits.cpu(), ref_logits), 'the logits are p2v_forward\'s'
            assert grams.shape == (len(names), x.shape[0], x.shape[0]) and grams.dtype == torch.float64 and units.shape == (len(names),)
            g, u = grams.cpu(), units.cpu()
            if with_linear and lin is None:
                _, bufs = plan.forward_linear_taps(xc, bits)
                lin = {}
                for i in range(depth):
                    for j, leaf in enumerate(('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')):
                        lin['blocks.%d.%s' % (i, leaf)] = bufs[1 + 4 * i + j].cpu()
                lin['head'] = bufs[-1].cpu()
            for k, nm in enumerate(names):
                assert torch.equal(g[k], g[k].t()), (tag, nm)
                if nm in st:
                    values, scale, kind = st[nm]
                    _check_stage(nm, g[k], float(u[k]), values, scale, kind, c, (tag, bits[:3], stages, with_linear))
                else:
                    _check_stage(nm, g[k], float(u[k]), lin[nm], None, 'f32', c, (tag, bits[:3], stages, with_linear))
            again = plan.forward_grams(xc, bits, with_linear=with_linear, stages=stages)
            assert torch.equal(again[2], grams) and torch.equal(again[3], units), 'bitwise repeatable'
            if full_ref and stages == 'full':
                import _ddv_full_ref as F
                for nm, (values, scale) in F.full_stage_values(O, arch, W, c, x, bits)[0].items():
                    kind = 'f32' if values.dtype.is_floating_point else 'codes'
                    _check_stage(nm, g[names.index(nm)], float(u[names.index(nm)]), values, scale, kind, c, (tag, 'full_stage_values'))
        assert torch.equal(plan.forward(xc, bits), plain), 'a plain forward afterwards'


ALL = [('engine', False), ('engine', True), ('full', False), ('full', True)]


def test_forward_grams_micro_vit(dva, oracle, micro):
    """Config(True, True): the micro ViT of the DDV tests, batch 6, three bit lists x {engine, full} x {with_linear}: every integer
    stage's Gram and unit equal the restatement on the staged oracle forward's values, the fp32 stages within the fp32 kernels' bound"""
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'][:6]
    assert x.shape[0] == 6
    bits = [[8] * 10, [4] * 10, [int(b) for b in micro['g']['bit_qmix']]]
    _check_model(dva, oracle, plan, micro['arch'], micro['sd'], micro['calib'], x, bits, True, True, ALL, 'tt', full_ref=True)


def test_forward_grams_micro_vit_float_ops(dva, oracle):
    """Config(False, False): float LayerNorm and softmax between the codes; the per-channel stages repeat one scale (shift 0)"""
    import _float_ops_ref as R
    g = R.fixture()
    arch = dva.synth.ARCHS['micro']
    seed = int(g['seed'])
    sd = dva.synth.vit_state_dict(arch, seed)
    m = R.make_model(dva, arch, sd, 'ff', 'cuda')
    dva.harness.calibrate_model(m, dva.synth.images(seed, int(g['n_calib']), arch['img_size']).cuda())
    c = m.export_calib()
    m.freeze('cuda')
    x = dva.synth.images(seed, 6, arch['img_size'], offset=1000)
    bl = R.bit_lists(g, 10)
    _check_model(dva, oracle, m._plan, arch, sd, c, x, [bl['q8'], bl['q4'], bl['qmix']], False, False, ALL, 'ff')


def test_forward_grams_deit_small(dva, oracle, synth):
    """the DeiT-S architecture at batch 4, engine stages: 197 x 384 ... 197 x 1536 codes a sample, several chunks and a chunk border
    inside a row; exact on every integer stage"""
    g = load_golden('deit_small')
    arch = synth.ARCHS['deit_small']
    sd = synth.vit_state_dict(arch, int(g['seed']))
    c = golden_calib(g, oracle)
    plan = dva.FrozenPlan(arch, sd, c, device=torch.device('cuda:0'))
    x = synth.images(int(g['seed']), 4, 224, offset=1000)
    _check_model(dva, oracle, plan, arch, sd, c, x, [[8] * 50], True, True, [('engine', False)], 'deit_s')


def test_workspace_state_and_refusals(dva, micro):
    """the result does not depend on what the workspace held (a forward_ddv and a forward_stats on the same plan in between); a plan
    without p2v_plan_prepare_grams, the attention flag, and short grams / units / workspace / tap_scratch buffers are refused before any launch"""
    E = dva.engine
    L = E.lib()
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'][:6].cuda().contiguous()
    bits = [int(b) for b in micro['g']['bit_qmix']]
    cfg = (ctypes.c_int8 * 10)(*bits)
    B, K = 6, L.p2v_forward_grams_stage_count(plan._handle, 1, E.DDV_STAGES_FULL)
    assert K == len(dva.ddv.stage_names(2, True, True)) == L.p2v_ddv_stage_count_ex(plan._handle, 1, E.DDV_STAGES_FULL)
    need = L.p2v_forward_grams_bytes(plan._handle, B, 1, E.DDV_STAGES_FULL)
    assert need > L.p2v_workspace_bytes(plan._handle, B)
    tap_need = L.p2v_ddv_tap_scratch_bytes(plan._handle, (B + 1) // 2)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    tap = torch.empty(tap_need, dtype=torch.uint8, device='cuda')
    out = torch.empty(B, micro['arch']['num_classes'], device='cuda')
    grams = torch.full((K, B, B), -7.0, dtype=torch.float64, device='cuda')
    units = torch.full((K,), -7.0, dtype=torch.float64, device='cuda')

    def call(stage_set=E.DDV_STAGES_FULL, lin=1, ws_bytes=need, tap_bytes=tap_need, tap_t=tap, grams_bytes=K * B * B * 8, units_bytes=K * 8, batch=B):
        return L.p2v_forward_grams(plan._handle, E.ptr(x), batch, cfg, 10, E.ptr(out), E.ptr(ws), ws_bytes, lin, stage_set, E.ptr(tap_t), tap_bytes,
                                   E.ptr(grams), grams_bytes, E.ptr(units), units_bytes, E.stream_ptr())
    assert call() == E.E_STATE and b'p2v_plan_prepare_grams' in L.p2v_last_error()
    assert L.p2v_plan_prepare_grams(plan._handle) == 0, L.p2v_last_error()
    for want, rc in ((E.E_UNSUPPORTED, call(stage_set=E.DDV_STAGES_ATTN)), (E.E_UNSUPPORTED, call(stage_set=E.DDV_STAGES_FULL | E.DDV_STAGES_ATTN)),
                     (E.E_ARG, call(stage_set=7)), (E.E_SHAPE, call(batch=0)), (E.E_SHAPE, call(batch=513)),
                     (E.E_WORKSPACE, call(grams_bytes=K * B * B * 8 - 1)), (E.E_WORKSPACE, call(units_bytes=K * 8 - 1)),
                     (E.E_WORKSPACE, call(ws_bytes=need - 1)), (E.E_WORKSPACE, call(ws_bytes=L.p2v_workspace_bytes(plan._handle, B))),
                     (E.E_WORKSPACE, call(tap_bytes=tap_need - 1)), (E.E_WORKSPACE, call(tap_t=None, lin=0)), (E.E_ARG, call(tap_t=None, stage_set=0))):
        assert rc == want, (rc, want, L.p2v_last_error())
    assert L.p2v_forward_grams_stage_count(plan._handle, 0, E.DDV_STAGES_ATTN) == E.E_UNSUPPORTED
    assert L.p2v_forward_grams_bytes(plan._handle, B, 0, E.DDV_STAGES_ATTN) == 0 and L.p2v_forward_grams_bytes(plan._handle, 513, 0, 0) == 0
    _sync()
    assert bool((grams == -7.0).all()) and bool((units == -7.0).all()), 'a refused call writes nothing'
    assert call() == 0, L.p2v_last_error()
    _sync()
    first, first_u, logits = grams.clone(), units.clone(), out.clone()
    rows, cols, kinds = (ctypes.c_int32 * K)(), (ctypes.c_int32 * K)(), (ctypes.c_int32 * K)()
    assert L.p2v_forward_grams_layout(plan._handle, 1, E.DDV_STAGES_FULL, K, rows, cols, kinds, None) == K
    assert (rows[0], kinds[0]) == (16, E.GRAM_I8) and cols[0] >= 192, 'qact_input: the patch matrix'
    assert (rows[K - 1], cols[K - 1], kinds[K - 1]) == (1, micro['arch']['num_classes'], E.GRAM_F32), 'act_out: the logits'
    # the plan's own workspace, dirtied by the other consumers of the stage sites
    a = plan.forward_grams(x, bits, with_linear=True, stages='full')
    assert torch.equal(a[2], first) and torch.equal(a[0], logits)
    plan.forward_ddv(x, bits, with_linear=True, stages='full')
    plan.forward_stats(x, bits, with_linear=True, stages='full')
    ws.fill_(0xA6)
    tap.fill_(0x5B)
    assert call() == 0, L.p2v_last_error()
    b = plan.forward_grams(x, bits, with_linear=True, stages='full')
    _sync()
    assert torch.equal(grams, first) and torch.equal(b[2], first) and torch.equal(out, logits)
    assert torch.equal(units, first_u) and bool((b[3] > 0).all()), 'the Python entry point fills the one-scale units in'


# --------------------------------------------------------------------------------------------------
# 3. end to end
# --------------------------------------------------------------------------------------------------
def test_compute_cka_over_stages(dva, synth):
    from test_cka_gpu import _micro_model
    g = load_golden('micro_vit')
    fp, _ = _micro_model(dva, synth, g)
    q, _ = _micro_model(dva, synth, g)
    fp, q = fp.cuda(), q.cuda()
    dva.harness.calibrate_model(q, torch.from_numpy(g['x_cal']).cuda())
    fp_cpu, q_cpu = copy.deepcopy(fp).cpu(), copy.deepcopy(q).cpu()          # (before the first quantized forward freezes a plan into q)
    x = torch.from_numpy(g['x_ev'])
    bits = [8] * 10
    for stages, lin in (('engine', False), ('full', True)):
        S = len(dva.ddv.stage_names(2, lin, stages == 'full'))
        hm = dva.compute_cka(fp, q, [x], None, bits, stages=stages, with_linear=lin)
        assert hm.shape == (S, S) and bool(torch.isfinite(hm).all())
        n1, g1 = dva.cka.get_stage_grams(x, fp, None, 'cuda', stages=stages, with_linear=lin)
        n2, g2 = dva.cka.get_stage_grams(x, q, bits, 'cuda', stages=stages, with_linear=lin)
        assert n1 == n2 == dva.ddv.stage_names(2, lin, stages == 'full') and g2.is_cuda and g2.dtype == torch.float32
        c = dva.MinibatchCKA(S, S, across_models=True)
        c.update_state_across_models_grams(g1, g2)
        assert torch.equal(c.result(), hm)
        # the fake-quant module graph (hooks on the QAct modules, on the CPU) carries the platform roundings of DESIGN section 2: no
        # fixed distance is asserted, the difference is printed
        graph = dva.compute_cka(fp_cpu, q_cpu, [x], None, bits, stages=stages, with_linear=lin)
        print('compute_cka(stages=%r, with_linear=%r): max |engine - module graph| = %.3g' % (stages, lin, float((hm.cpu() - graph).abs().max())))
