"""GPU: the stage statistics on the MI355X - p2v_code_stats against the numpy restatement of the record (tests/_stats_ref.py) with the records
in sentinel arenas, hand-made planes at the edges of the code range and of the 32-bit counters, accumulation, refusals, the record of a
replayed sequence; then p2v_forward_stats / SwinPlan.forward_stats on whole models, stage by stage.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import _stats_ref as SR
from _arena import SENTINELS, Arena, twice

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


NP = {0: np.int8, 1: np.float32, 2: np.uint8}
VEC = {0: 16, 1: 4, 2: 16}


def _data(rng, kind, shape):
    if kind == 1:
        x = (rng.standard_normal(shape) * np.exp2(rng.randint(-40, 40, shape))).astype(np.float32)
        flat = x.reshape(-1)
        pick = rng.randint(0, flat.size, max(1, flat.size // 50))
        flat[pick] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-42, np.inf, -np.inf, np.nan], np.float32), pick.size)
        return x
    return rng.randint(-128, 128, shape).astype(np.int8) if kind == 0 else rng.randint(0, 256, shape).astype(np.uint8)


def _plane(x, pad_rows, far_samples, poison):
    """x [S, R, cols] on the host -> (device buffer kept alive, [S, R, cols] view of it, sample stride, row stride): rows padded by one
    16-byte group behind whole groups, samples three rows further apart (the class-row layout of a [T][D] plane); padding = ``poison``"""
    S, R, cols = x.shape
    vec = 16 // x.dtype.itemsize
    rs = (cols + vec - 1) // vec * vec + (vec if pad_rows else 0)
    fill = poison if x.dtype != np.float32 else poison * 0x01010101
    buf = np.full((S, R + (3 if far_samples else 0), rs), fill, dtype=np.uint8 if x.dtype != np.float32 else np.uint32).view(x.dtype)
    buf[:, :R, :cols] = x
    dev = torch.from_numpy(buf).cuda()
    return dev, dev[:, :R, :cols], dev.stride(0), dev.stride(1)


def _layer(E, view, kind, rows=None, samples=None):
    d = E.StatLayer()
    d.base, d.sample_stride, d.row_stride = view.data_ptr(), view.stride(0), view.stride(1)
    d.samples, d.rows, d.cols, d.dtype = view.shape[0] if samples is None else samples, view.shape[1] if rows is None else rows, view.shape[2], kind
    return d


def _run(E, layers, kinds, cols, fill, init=True, arena=None):
    """p2v_stats_init on every record of one flat arena, then ONE p2v_code_stats call -> (arena, [parsed records])"""
    L = E.lib()
    sizes = [L.p2v_stats_bytes(c) for c in cols]
    assert sizes == [SR.record_bytes(c) for c in cols]
    offs = np.concatenate(([0], np.cumsum(sizes)))
    if arena is None:
        arena = Arena(1, int(offs[-1]), None, torch.uint8, fill)
    base = arena.dev.data_ptr() + arena.start
    assert base % 16 == 0
    if init:
        for k in range(len(cols)):
            assert L.p2v_stats_init(ctypes.c_void_p(base + int(offs[k])), sizes[k], kinds[k], cols[k], E.stream_ptr()) == 0, L.p2v_last_error()
    recs = (ctypes.c_void_p * len(cols))(*[base + int(o) for o in offs[:-1]])
    arr = (E.StatLayer * len(layers))(*layers)
    rc = L.p2v_code_stats(arr, len(layers), recs, None, 0, E.stream_ptr())
    _sync()
    assert rc == 0, (rc, L.p2v_last_error())
    raw = arena.read(('code_stats', hex(fill))).numpy().reshape(-1)
    return arena, [SR.parse(raw[int(offs[k]):int(offs[k + 1])], cols[k], kinds[k] == 1) for k in range(len(cols))]


# --------------------------------------------------------------------------------------------------
# 1. the operator against the helper
# --------------------------------------------------------------------------------------------------
SAMPLES, ROWS = (1, 2, 6), (1, 2, 17, 63, 64, 65, 257)


@pytest.mark.parametrize('cols', [4, 10, 16, 20, 64, 192, 1000, 3072, 4096])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_code_stats_sweep(dva, kind, cols):
    """every (samples, rows) x {dense, padded rows} x {dense, class-row samples} plane of one width in ONE call, the records back to back
    in a sentinel arena under two fills; the four layouts of one plane hold the same values, so they share one reference record"""
    E = dva.engine
    rng = np.random.RandomState(1000 * kind + cols)
    planes = [_data(rng, kind, (S, R, cols)) for S in SAMPLES for R in ROWS]
    want = [SR.record(x) for x in planes]

    def run(fill):
        keep, layers = [], []
        for x in planes:
            for pad_rows in (False, True):
                for far in (False, True):
                    dev, view, _, _ = _plane(x, pad_rows, far, fill)
                    keep.append(dev)
                    layers.append(_layer(E, view, kind))
        _, got = _run(E, layers, [kind] * len(layers), [cols] * len(layers), fill)
        for k, g in enumerate(got):
            SR.same(g, want[k // 4], (kind, cols, planes[k // 4].shape, 'layout %d' % (k % 4)))
        return {('%d.%s' % (k, f)): torch.from_numpy(np.atleast_1d(g[f]).copy()) for k, g in enumerate(got) for f in SR.FIELDS}
    twice(run)


def test_hand_made_planes(dva):
    E = dva.engine
    lo8, hi8 = np.full((2, 5, 20), -128, np.int8), np.full((2, 5, 20), 127, np.int8)
    out = np.zeros((3, 7, 64), np.int8)
    out[-1, -1, -1] = -77
    u8 = np.random.RandomState(3).randint(128, 256, (2, 9, 48)).astype(np.uint8)
    f = np.random.RandomState(4).standard_normal((3, 6, 12)).astype(np.float32)
    f[0, 0, 0], f[0, 1, 1], f[1, 2, 2], f[2, 3, 3], f[0, 4, 4], f[1, 5, 5] = np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-41
    f[:, :, 6] = -1e-45
    f[:, :, 7] = np.nan                                     # a column without a finite element
    f[:, :, 8] = [[0.0, -0.0] * 3] * 3                      # both zeros: lo = -0, hi = +0
    big = np.full((1, 131073, 4), -128, np.int8)            # sumsq = 131 073 * 2^14 = 2 147 500 032 > 2^31
    wide = np.full((1, 70000, 16), 255, np.uint8)           # sumsq = 70 000 * 65 025 > 2^32: more than one workgroup's 2^16 rows
    planes = [lo8, hi8, out, u8, f, big, wide]
    kinds = [0, 0, 0, 2, 1, 0, 2]
    want = [SR.record(x) for x in planes]
    assert int(want[5]['sumsq'][0]) == 2147500032 and int(want[6]['sumsq'][0]) == 70000 * 65025 > 2 ** 32
    assert want[4]['lo'].view(np.uint32)[7] == 0x7f800000 and want[4]['hi'].view(np.uint32)[7] == 0xff800000
    assert want[4]['lo'].view(np.uint32)[8] == 0x80000000 and want[4]['hi'].view(np.uint32)[8] == 0
    assert want[0]['hist'][0] == lo8.size and want[1]['hist'][255] == hi8.size and want[2]['lo'][-1] == -77 and want[2]['hi'][-1] == 0

    def run(fill):
        keep = [_plane(x, k % 2 == 0, k % 3 == 0, fill) for k, x in enumerate(planes)]
        _, got = _run(E, [_layer(E, v[1], kinds[k]) for k, v in enumerate(keep)], kinds, [x.shape[2] for x in planes], fill)
        for k, g in enumerate(got):
            SR.same(g, want[k], ('hand-made', k))
        return {('%d.%s' % (k, f)): torch.from_numpy(np.atleast_1d(g[f]).copy()) for k, g in enumerate(got) for f in SR.FIELDS}
    twice(run)


def test_accumulation_empty_planes_and_the_op(dva):
    """two accumulating calls equal one call on the concatenation; rows == 0 or samples == 0 succeeds and leaves the empty record;
    torch.ops.p2vit.code_stats and stats.code_stats on views of any stride"""
    E = dva.engine
    rng = np.random.RandomState(11)
    planes = [_data(rng, k, (6, 33, c)) for k, c in ((0, 192), (1, 40), (2, 10))]
    kinds, cols = [0, 1, 2], [192, 40, 10]
    fill = SENTINELS[0]
    once = [_plane(x, True, False, fill) for x in planes]          # (kept alive until the call has run)
    whole = _run(E, [_layer(E, v[1], k) for v, k in zip(once, kinds)], kinds, cols, fill)[1]
    first = [_plane(x[:2], False, True, fill) for x in planes]
    rest = [_plane(x[2:], True, True, fill) for x in planes]
    arena, _ = _run(E, [_layer(E, v[1], k) for v, k in zip(first, kinds)], kinds, cols, fill)
    _, both = _run(E, [_layer(E, v[1], k) for v, k in zip(rest, kinds)], kinds, cols, fill, init=False, arena=arena)
    for k in range(3):
        SR.same(both[k], whole[k], ('accumulated', k))
        SR.same(whole[k], SR.record(planes[k]), ('whole', k))
    # empty planes: nothing is launched, the initialised record stays
    _, empty = _run(E, [_layer(E, first[0][1], 0, rows=0), _layer(E, first[1][1], 1, samples=0), _layer(E, first[2][1], 2, rows=0)], kinds, cols, fill)
    for k in range(3):
        SR.same(empty[k], SR.record(planes[k][:0]), ('empty', k))
    # the op: fresh records; odd widths and strides are served by a padded copy
    t = [torch.from_numpy(x).cuda() for x in planes] + [torch.from_numpy(planes[0]).cuda()[:, ::2, 1:7], torch.from_numpy(planes[1]).cuda().reshape(6, 3, 11, 40)]
    recs = torch.ops.p2vit.code_stats(t)
    refs = [SR.record(x) for x in planes] + [SR.record(planes[0][:, ::2, 1:7]), SR.record(planes[1])]
    for k, r in enumerate(recs):
        SR.same(SR.parse(r.cpu().numpy(), t[k].shape[-1], t[k].dtype == torch.float32), refs[k], ('op', k))
    st = dva.stats.code_stats(t[:3], ['a', 'b', 'c'])
    assert dva.stats.code_stats([x[:0] for x in t[:3]], into=st) is st
    cpu = dva.stats.code_stats_cpu([torch.from_numpy(x) for x in planes], ['a', 'b', 'c'])
    assert torch.equal(st.cpu().arena, cpu.arena)
    two = dva.stats.code_stats([x[:4] for x in t[:3]], ['a', 'b', 'c'])
    dva.stats.code_stats([x[4:] for x in t[:3]], into=two)
    assert torch.equal(two.arena, st.arena) and torch.equal(two.merge(st).cpu().arena, cpu.merge(cpu).arena)


def test_refusals_by_code_and_the_recorded_stage(dva):
    E = dva.engine
    L = E.lib()
    fill = SENTINELS[0]
    x = _data(np.random.RandomState(2), 0, (2, 8, 32))
    dev, view, _, _ = _plane(x, False, False, fill)
    rec = Arena(1, L.p2v_stats_bytes(32), None, torch.uint8, fill)
    st = E.stream_ptr()

    def call(layer=None, record=rec.ptr, n=1, layers=True, recs=True):
        arr = (E.StatLayer * 1)(layer if layer is not None else _layer(E, view, 0))
        rp = (ctypes.c_void_p * 1)(record)
        return L.p2v_code_stats(arr if layers else None, n, rp if recs else None, None, 0, st)

    def bad(**kw):
        d = _layer(E, view, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for rc_want, rc in ((E.E_ARG, call(layers=False)), (E.E_ARG, call(recs=False)), (E.E_ARG, call(n=0)), (E.E_ARG, call(record=None)),
                        (E.E_ARG, call(bad(base=None))), (E.E_ARG, call(bad(dtype=3))), (E.E_SHAPE, call(bad(cols=0))),
                        (E.E_ARG, call(bad(rows=-1))), (E.E_ARG, call(bad(samples=-1))), (E.E_ARG, call(bad(row_stride=31))),
                        (E.E_ARG, call(bad(sample_stride=-16))), (E.E_ARG, call(bad(base=view.data_ptr() + 4))),
                        (E.E_ARG, call(bad(row_stride=40))), (E.E_ARG, call(bad(sample_stride=8 * 32 + 8))),
                        (E.E_ARG, call(record=ctypes.c_void_p(rec.ptr.value + 8))), (E.E_UNSUPPORTED, call(bad(samples=1 << 16, rows=1 << 15)))):
        assert rc == rc_want, (rc, rc_want, L.p2v_last_error())
    assert L.p2v_stats_init(rec.ptr, rec.width - 1, 0, 32, st) == E.E_WORKSPACE
    assert L.p2v_stats_init(rec.ptr, rec.width, 5, 32, st) == E.E_ARG and L.p2v_stats_init(rec.ptr, rec.width, 0, 0, st) == E.E_SHAPE
    assert L.p2v_stats_init(ctypes.c_void_p(rec.ptr.value + 4), rec.width, 0, 32, st) == E.E_ARG
    _sync()
    assert bool((rec.read('refused calls').numpy() == fill).all())
    # P2V_OP_STATS through p2v_run_ops: the stage record of a replayed sequence, a misaligned (scalar-load) plane included
    odd = torch.from_numpy(np.concatenate((np.zeros(4, np.int8), x.reshape(-1)))).cuda()[4:].view(2, 8, 32)
    assert odd.data_ptr() % 16 == 4
    for plane in (view, odd):
        assert L.p2v_stats_init(rec.ptr, rec.width, 0, 32, st) == 0
        op = E.Op()
        op.kind, op.inp, op.out = E.OP_STATS, E.ptr(plane), rec.ptr
        op.i0, op.i1, op.M, op.N, op.lda, op.i2, op.i3 = 2, E.STAT_I8, 8, 32, 32, 8 * 32, 0
        assert L.p2v_run_ops((E.Op * 1)(op), 1, st) == 0, L.p2v_last_error()
        _sync()
        SR.same(SR.parse(rec.read('op').numpy().reshape(-1), 32, False), SR.record(x), 'P2V_OP_STATS')
    op.i1 = 7
    assert L.p2v_run_ops((E.Op * 1)(op), 1, st) == E.E_ARG


# --------------------------------------------------------------------------------------------------
# 2. whole models: ViT / DeiT
# --------------------------------------------------------------------------------------------------
def _np_of(v, kind):
    v = v.detach().cpu()
    if kind == 'f32':
        return v.float().numpy()
    return v.to(torch.int16).numpy().astype(np.int8 if kind == 'i8' else np.uint8)


def _vit_expected(dva, O, R, plan, arch, W, c, x, bits, int_norm, int_softmax, with_linear, attention):
    """stage name -> reference record, from the helper's stages (tests/_float_ops_ref.quant_forward: the oracle's statements), the oracle's
    attention taps and - for the fp32 layer outputs - the tensors forward_linear_taps delivers"""
    st, taps = {}, {}
    logits = R.quant_forward(O, arch, W, c, x, bits, int_norm, int_softmax, taps=taps, stages=st)
    P = arch['patch_size']
    want = {}
    for nm, (v, _, kind) in st.items():
        if nm == 'qact_input':          # the engine's stage is the patch matrix: the real C * P^2 columns of every patch
            v = torch.nn.functional.unfold(v.float(), kernel_size=P, stride=P).transpose(1, 2)
        want[nm] = SR.record(_np_of(v, 'f32' if kind == 'f32' else 'i8'))
    if attention:
        for i in range(arch['depth']):
            p = 'blocks.%d.attn.' % i
            want[p + 'qact_attn1'] = SR.record(_np_of(taps[p + 'qact_attn1'], 'i8'))
            want[p + 'log_int_softmax'] = SR.record(_np_of(O.lis_int(taps[p + 'qact_attn1'].float(), c[p + 'qact_attn1']), 'u8'))
    if with_linear:
        _, bufs = plan.forward_linear_taps(x.cuda(), bits)
        for i in range(arch['depth']):
            for j, leaf in enumerate(('attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')):
                want['blocks.%d.%s' % (i, leaf)] = SR.record(_np_of(bufs[1 + 4 * i + j], 'f32'))
        want['head'] = SR.record(_np_of(bufs[-1].reshape(x.shape[0], 1, -1), 'f32'))
    return want, logits


def _check_vit(dva, O, R, plan, arch, W, c, x, bits, int_norm=True, int_softmax=True, sets=None, tag=''):
    xc = x.cuda()
    plain = plan.forward(xc, bits).clone()
    sets = sets or [('engine', False, False), ('full', False, False), ('engine', False, True), ('engine', True, False), ('full', True, True)]
    for stages, lin, att in sets:
        logits, st = plan.forward_stats(xc, bits, with_linear=lin, stages=stages, attention=att)
        _sync()
        assert st.names == dva.ddv.stage_names(arch['depth'], lin, stages == 'full', att)
        assert torch.equal(logits, plain), 'the logits are p2v_forward\'s'
        want, ref_logits = _vit_expected(dva, O, R, plan, arch, W, c, x, bits, int_norm, int_softmax, lin, att)
        assert torch.equal(logits.cpu(), ref_logits)
        host = st.cpu()
        for nm in st.names:
            SR.same(SR.fields_of(host.record(nm)), want[nm], (tag, stages, lin, att, nm))
        again = plan.forward_stats(xc, bits, with_linear=lin, stages=stages, attention=att)[1]
        assert torch.equal(again.arena, st.arena), 'bitwise repeatable'
        # into= over two batches of different sizes equals one batch of both
        _, two = plan.forward_stats(xc[:2], bits, with_linear=lin, stages=stages, attention=att)
        assert plan.forward_stats(xc[2:], bits, with_linear=lin, stages=stages, attention=att, into=two)[1] is two
        assert torch.equal(two.arena, st.arena), (tag, stages, lin, att, 'into=')
    assert torch.equal(plan.forward(xc, bits), plain), 'a plain forward afterwards'
    return st


def test_forward_stats_micro_vit(dva, oracle, micro):
    """the micro ViT under the three bit lists x {engine, FULL, attention, with_linear}: every stage against the helper; where the REAL
    reference's fixture holds a stage's codes (8-bit and mixed list), the helper's input is checked against them first"""
    import _float_ops_ref as R
    from test_stats import fixture_codes
    g = micro['g']
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    for tag, bits in (('q8', [8] * 10), ('q4', [4] * 10), ('qmix', [int(b) for b in g['bit_qmix']])):
        st = _check_vit(dva, oracle, R, plan, micro['arch'], micro['sd'], micro['calib'], micro['x_ev'], bits, tag=tag)
        host = st.cpu()                                       # the last set: FULL + linear + attention
        codes = fixture_codes(g, tag)
        assert len(codes) == (0 if tag == 'q4' else 23)
        for nm, v in codes.items():
            if nm == 'qact_input':
                v = torch.nn.functional.unfold(torch.from_numpy(v).float(), kernel_size=8, stride=8).transpose(1, 2).numpy().astype(np.int8)
            if nm == 'act_out':                               # the engine's stage holds the logits: codes times the power-of-two scale
                lo, hi = host.channel_ranges(nm)
                s = micro['calib']['act_out'].reshape(-1).numpy().astype(np.float32)
                r = SR.record(v)
                assert np.array_equal(lo.numpy(), r['lo'] * s) and np.array_equal(hi.numpy(), r['hi'] * s)
                continue
            SR.same(SR.fields_of(host.record(nm)), SR.record(v.reshape(6, -1, v.shape[-1])), (tag, 'fixture', nm))
        # derived views on the engine's records: codes times the stage's scale
        lo, hi = host.channel_ranges('blocks.0.qact2')
        r = host.record('blocks.0.qact2')
        s = micro['calib']['blocks.0.qact2'].reshape(-1).float()
        assert torch.equal(lo, r['lo'].float() * s) and torch.equal(hi, r['hi'].float() * s)
        lo, _ = host.channel_ranges('blocks.1.attn.qact1')
        assert torch.equal(lo, host.record('blocks.1.attn.qact1')['lo'].float() * float(micro['calib']['blocks.1.attn.qact1']))


def test_forward_stats_in_arenas_and_refusals(dva, micro):
    """one call per stage set with workspace, logits, scratches and the records in arenas under two fills: nothing outside them is
    written, the records equal a plain-buffer call; refusals leave the records untouched"""
    E = dva.engine
    L = E.lib()
    plan = dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])
    x = micro['x_ev'][:5].cuda().contiguous()
    B = 5
    bits = [int(b) for b in micro['g']['bit_qmix']]
    cfg = (ctypes.c_int8 * 10)(*bits)
    n = (B + 1) // 2

    def call(fill, stage_set, lin, init=True, tap=True, att=True, stats_short=0, expect=0, batch=B):
        total = L.p2v_forward_stats_bytes(plan._handle, lin, stage_set)
        K = L.p2v_ddv_stage_count_ex2(plan._handle, lin, stage_set)
        off, cols, kinds = (ctypes.c_longlong * K)(), (ctypes.c_int32 * K)(), (ctypes.c_int32 * K)()
        assert L.p2v_forward_stats_layout(plan._handle, lin, stage_set, K, off, cols, kinds, None) == K
        assert total == sum(SR.record_bytes(c) for c in cols) and list(off) == list(np.cumsum([0] + [SR.record_bytes(c) for c in cols])[:-1])
        ws = Arena(1, L.p2v_workspace_bytes(plan._handle, B), None, torch.uint8, fill, offset=0)
        out = Arena(B, 10, None, torch.float32, fill)
        tp = Arena(1, L.p2v_ddv_tap_scratch_bytes(plan._handle, n), None, torch.uint8, fill)
        ap = Arena(1, L.p2v_ddv_attn_scratch_bytes(plan._handle, n), None, torch.uint8, fill)
        rec = Arena(1, total, None, torch.uint8, fill)
        if init:
            for k in range(K):
                assert L.p2v_stats_init(ctypes.c_void_p(rec.ptr.value + off[k]), SR.record_bytes(cols[k]), kinds[k], cols[k], E.stream_ptr()) == 0
        rc = L.p2v_forward_stats(plan._handle, E.ptr(x), batch, cfg, 10, out.ptr, ws.ptr, ws.width, lin, stage_set, tp.ptr if tap else None, tp.width,
                                 ap.ptr if att else None, ap.width, rec.ptr, total - stats_short, E.stream_ptr())
        _sync()
        assert rc == expect, (rc, L.p2v_last_error())
        what = ('forward_stats', stage_set, lin, hex(fill))
        ws.read(('workspace',) + what), tp.read(('tap scratch',) + what), ap.read(('attention scratch',) + what)
        return out.read(('logits',) + what), rec.read(('records',) + what).numpy().reshape(-1)

    for stage_set, stages, att in ((0, 'engine', False), (1, 'full', False), (2, 'engine', True), (3, 'full', True)):
        for lin in (0, 1):
            logits, st = plan.forward_stats(x, bits, with_linear=bool(lin), stages=stages, attention=att)
            _sync()
            for fill in SENTINELS:
                out, raw = call(fill, stage_set, lin)
                assert np.array_equal(out.numpy().view(np.uint32), logits.cpu().numpy().view(np.uint32))
                assert np.array_equal(raw, st.arena.cpu().numpy()), (stage_set, lin, hex(fill))
    fill = SENTINELS[0]
    for kw, code in ((dict(stage_set=4), E.E_ARG), (dict(stage_set=1, tap=False), E.E_WORKSPACE), (dict(stage_set=0, lin=1, tap=False), E.E_ARG),
                     (dict(stage_set=2, att=False), E.E_ARG), (dict(stage_set=0, batch=0), E.E_SHAPE)):
        kw.setdefault('lin', 0)
        if kw['stage_set'] == 4:
            assert L.p2v_forward_stats_bytes(plan._handle, 0, 4) == 0 and L.p2v_forward_stats_layout(plan._handle, 0, 4, 0, None, None, None, None) == E.E_ARG
            continue
        out, raw = call(fill, init=False, expect=code, **kw)
        assert bool((raw == fill).all()) and bool((out.numpy().view(np.uint8) == fill).all()), kw
    # a short arena is refused at the record that does not fit: nothing behind the arena's end is written (the guards were read above)
    call(fill, 0, 0, stats_short=16, expect=E.E_WORKSPACE)
    with pytest.raises(AssertionError):
        plan.forward_stats(x, bits, into=plan.forward_stats(x, bits, with_linear=True)[1])
    with pytest.raises(ValueError):
        plan.forward_stats(x, bits, stages='all')


def test_forward_stats_float_configurations(dva, oracle):
    """Config(ptf=False) / Config(lis=False): the arithmetic the engine runs there, stage by stage against the helper"""
    import _float_ops_ref as R
    g = R.fixture()
    arch = dva.synth.ARCHS['micro']
    seed = int(g['seed'])
    sd = dva.synth.vit_state_dict(arch, seed)
    x_cal = dva.synth.images(seed, int(g['n_calib']), arch['img_size'])
    x = dva.synth.images(seed, int(g['n_eval']), arch['img_size'], offset=1000)
    for tag in sorted(R.CONFIGS):
        ptf, lis = R.CONFIGS[tag]
        m = R.make_model(dva, arch, sd, tag, 'cuda')
        dva.harness.calibrate_model(m, x_cal.cuda())
        m.freeze('cuda')
        sets = [('engine', False, False), ('full', True, False)] + ([('full', False, True)] if lis else [])
        _check_vit(dva, oracle, R, m._plan, arch, sd, m.export_calib(), x, R.bit_lists(g, 10)['qmix'], ptf, lis, sets, tag)
        st = dva.compute_stats(m, x.cuda(), [8] * 10, with_linear=False)
        assert st.names == dva.ddv.stage_names(2, False) and st.arena.is_cuda and st.key[0] == 'plan'
        if not lis:
            with pytest.raises(NotImplementedError):
                m._plan.forward_stats(x.cuda(), [8] * 10, attention=True)
            with pytest.raises(NotImplementedError):
                dva.compute_stats(m, x.cuda(), [8] * 10, attention=True)
    # every other state hooks the module graph: a float model on the GPU reduces through the op, as F32
    fp = R.make_model(dva, arch, sd, 'ft', 'cuda')
    sf = dva.compute_stats(fp, x.cuda())
    assert sf.names == dva.ddv.stage_names(2, True) and all(sf.kind(nm) == 'f32' for nm in sf.names)
    cpu = dva.compute_stats(R.make_model(dva, arch, sd, 'ft', 'cpu'), x)
    assert [int(sf.record(nm)['count']) for nm in sf.names] == [int(cpu.record(nm)['count']) for nm in cpu.names]


# --------------------------------------------------------------------------------------------------
# 3. whole models: Swin
# --------------------------------------------------------------------------------------------------
def _check_swin(dva, m, x, bits):
    from _ddv_attention_ref import swin_attention_stages
    from test_swin_modeldiff_gpu import oracle_stages
    D = dva.ddv
    with torch.no_grad():
        st_o, ref = oracle_stages(m, x, bits)
        at_o, _ = swin_attention_stages(m, x, bits)
    m.cuda()
    try:
        with torch.no_grad():
            fwd = m(x.cuda(), bits=bits).cpu()
            plan = m._plan
            for lin, att in ((False, False), (True, True)):
                logits, st = plan.forward_stats(x.cuda(), lin, attention=att)
                _sync()
                assert st.names == D.swin_stage_names(m.arch['depths'], lin, att)
                assert torch.equal(logits.cpu(), fwd) and torch.equal(fwd, ref)
                host = st.cpu()
                for k, nm in enumerate(host.names):
                    cols = host.cols[k]
                    if nm in at_o:
                        v, kind = at_o[nm]
                        want = SR.record(_np_of(v.reshape(-1, cols), 'u8' if kind == 'log2k' else 'i8'))
                    else:
                        v, _, is_f = st_o[nm]
                        want = SR.record(_np_of(v.reshape(-1, cols), 'f32' if is_f else 'i8'))
                    SR.same(SR.fields_of(host.record(nm)), want, (bits, lin, att, nm))
                _, two = plan.forward_stats(x[:1].cuda(), lin, attention=att)
                assert plan.forward_stats(x[1:].cuda(), lin, attention=att, into=two)[1] is two
                assert torch.equal(two.arena, st.arena), (bits, lin, att, 'into=')
            assert torch.equal(m(x.cuda(), bits=bits).cpu(), fwd), 'a plain forward afterwards'
            cs = dva.compute_stats(m, x.cuda(), bits, with_linear=True, attention=True)
            assert torch.equal(cs.arena, st.arena)
            with pytest.raises(NotImplementedError):
                dva.compute_stats(m, x.cuda(), [8] * 10)
    finally:
        m.cpu()


@pytest.mark.parametrize('bits', [8, 4])
def test_forward_stats_micro_swin(dva, bits):
    from test_swin_modeldiff_gpu import _micro7
    _check_swin(dva, _micro7(), dva.synth.images(21, 3, 56), bits)


def test_forward_stats_swin_window12(dva):
    from test_swin_modeldiff_gpu import _calibrated
    _check_swin(dva, _calibrated(dva, dva.swin.swin_micro_patch4_window12_96, 96), dva.synth.images(22, 2, 96), 8)


def test_forward_stats_swin_large_micro(dva):
    """768 -> merge LayerNorm over 3072 channels -> 1536: records of up to 3072 columns (three column tiles)"""
    from test_swin_large import large_micro
    m, x = large_micro()
    _check_swin(dva, m, x[:3], 8)


def test_cli_deit_tiny(dva, tmp_path):
    """the command line on a fused model: two batches accumulated on the device, one line per stage, the pickle"""
    import pickle
    st = dva.stats.main(['--model', 'deit_tiny', '--bits', 'mixed', '--n', '6', '--batch', '4', '--attention', '--result-name', str(tmp_path)])
    assert st.names == dva.ddv.stage_names(12, False, False, True)
    with open(tmp_path / 'stats.pkl', 'rb') as f:
        res = pickle.load(f)
    assert res['stages'] == st.names and res['n'] == 6
    r = res['records']['blocks.3.attn.log_int_softmax']
    assert r['kind'] == 'u8' and int(r['count']) == 6 * 3 * 197 * 197 == int(r['hist'].sum())
    assert int(res['records']['qact1']['count']) == 6 * 197 * 192 and res['records']['qact1']['lo_value'].shape == (192,)
