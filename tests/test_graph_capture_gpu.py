"""GPU: enqueuing the forwards while the caller's stream is being captured into a HIP graph (``torch.cuda.graph``).

A capture records work, it does not run it.  The entry points that only launch on the caller's buffers must therefore replay to the eager
bytes, re-read their input buffers and keep nothing of the first batch; the ones that upload from host memory of their own, synchronise,
allocate or build plan state lazily must refuse while the stream is capturing, enqueue nothing and leave the capture valid.  The two
classes are the table of DESIGN.md, "Graph capture of the forwards"; ``REFUSED`` below is its second class.

Every comparison is ``torch.equal``.  The file sets no environment variable and creates no stream of its own; every capture is a
``with torch.cuda.graph(g):`` block in its default mode, and whatever has to see the capture passes ``E.stream_ptr()`` from inside it."""
import ctypes as C
from functools import partial

import pytest
import torch

import _swin_bits_ref as R

pytestmark = pytest.mark.gpu

BITS = [8] * 10
SLICES = [2, 2, 1]          # two side streams + the caller's: three parallel branches, the third slice wraps onto the caller's stream


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


@pytest.fixture(scope='module')
def E(dva):
    return dva.engine


def _fill(t):
    t.fill_(-7.25 if t.is_floating_point() else 0x5a)


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        assert torch.equal(a, b), (what, k, int((a != b).sum()))


def _clones(ts):
    return [t.clone() for t in ts]


def _static_protocol(call, make, x0, x1, out_shape=None):
    """The protocol of every capturable call.  ``call(target, x, out) -> [result tensors]``; ``make()`` builds a fresh target (plan or
    model).  Warm up eagerly twice on x0, capture into static x / out, replay against the eager result, refill x with x1 and replay
    against an EAGER run of a second, never-captured target, replay three times back to back, drop the graph, run eagerly again."""
    target, ref = make(), make()
    new_out = (lambda: torch.empty(out_shape, dtype=torch.float32, device='cuda')) if out_shape else (lambda: None)
    call(target, x0, new_out())
    eager0 = _clones(call(target, x0, new_out()))
    want1 = _clones(call(ref, x1, new_out()))
    want0 = _clones(call(ref, x0, new_out()))
    _same(eager0, want0, 'eager: two plans of one fixture')
    assert not all(torch.equal(a, b) for a, b in zip(want0, want1)), 'x0 and x1 must give different results'
    x, out = x0.clone(), new_out()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = call(target, x, out)
    for t in res:
        _fill(t)
    g.replay()
    torch.cuda.synchronize()
    _same(res, eager0, 'first replay')
    x.copy_(x1)                               # nothing of the first batch is baked in: the replay re-reads the input buffer
    for t in res:
        _fill(t)
    g.replay()
    torch.cuda.synchronize()
    _same(res, want1, 'replay on refilled input')
    for t in res:
        _fill(t)
    for _ in range(3):                        # workspace reuse across replays that nothing separates
        g.replay()
    torch.cuda.synchronize()
    _same(res, want1, 'three replays back to back')
    del g, res
    _same(call(target, x1, new_out()), want1, 'eager after the graph is gone')
    return target


# ---- 1. warm micro-ViT calls: capture == eager, replays re-read their inputs ------------------------------------------------------------------
@pytest.fixture(scope='module')
def vit(dva, micro):
    from diff_vit_amd import data as D
    mean, std, _ = D.MODEL_STATS['deit']
    lut32 = D.uint8_lut(mean, std)

    def plan():
        return dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])

    def model():
        a = micro['arch']
        m = dva.VisionTransformer(img_size=a['img_size'], patch_size=a['patch_size'], embed_dim=a['embed_dim'], depth=a['depth'],
                                  num_heads=a['num_heads'], num_classes=a['num_classes'], mlp_ratio=a['mlp_ratio'], qkv_bias=True,
                                  norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
        m.load_state_dict(micro['sd'], strict=False)
        m = m.to('cuda').eval()
        dva.harness.calibrate_model(m, micro['x_cal'].cuda())
        return m

    def lut(p):             # the device table goes with the plan; made by the eager warm-up, never inside a capture
        if '_capture_test_lut' not in p.__dict__:
            p.__dict__['_capture_test_lut'] = p.input_lut(lut32)
        return p.__dict__['_capture_test_lut']

    x0, x1 = micro['x_ev'][:5].cuda(), dva.synth.images(91, 5, micro['arch']['img_size']).cuda()
    u0, u1 = dva.synth.images_uint8(3, 5, micro['arch']['img_size']).cuda(), dva.synth.images_uint8(4, 5, micro['arch']['img_size']).cuda()
    return dict(plan=plan, model=model, lut=lut, x0=x0, x1=x1, u0=u0, u1=u1, classes=micro['arch']['num_classes'])


def _nchw(u):
    return u.permute(0, 3, 1, 2).contiguous()


def _stop_after(p, x, out):
    # launch numbering: patchify, embed, class fill, then block 0's fused LayerNorm + qkv (two slots): the qkv codes are complete at 5
    p.forward(x, BITS, stop_after=5)
    return [p.view(x.shape[0], 'qkv', x.shape[0] * p.tokens, 3 * p.D)]


def _taps(p, x, out):
    taps = {}
    o = p.forward(x, BITS, out=out, taps=taps)
    return [o] + taps['qkv_output'] + taps['fc1_output']


def _linear_taps(p, x, out):
    o, bufs = p.forward_linear_taps(x, BITS, out=out)
    return [o] + bufs


def _ddv(p, x, out):
    o, names, sums = p.forward_ddv(x, BITS, with_linear=True, stages='full')
    return [o, sums]


def _stats(p, x, out):
    o, st = p.forward_stats(x, BITS, with_linear=True, stages='full')
    return [o, st.arena]


# name -> (target kind, input kind, images, takes a static `out`, call)
VIT_CASES = {
    'forward_b1': ('plan', 'f32', 1, True, lambda p, x, out: [p.forward(x, BITS, out=out)]),
    'forward_b5_ragged': ('plan', 'f32', 5, True, lambda p, x, out: [p.forward(x, BITS, out=out)]),
    'forward_mixed_bits': ('plan', 'f32', 5, True, lambda p, x, out: [p.forward(x, [4, 8] * 5, out=out)]),
    'forward_stop_after': ('plan', 'f32', 5, False, _stop_after),
    'forward_uint8_nhwc': ('plan', 'u8', 5, True, None),
    'forward_uint8_nchw': ('plan', 'u8_nchw', 5, True, None),
    'forward_streams': ('plan', 'f32', 5, True, lambda p, x, out: [p.forward_streams(x, BITS, out, n_streams=2, slices=SLICES)]),
    'forward_uint8_streams': ('plan', 'u8', 5, True, None),
    'module_forward': ('model', 'f32', 5, False, lambda m, x, out: [m(x, BITS, False)[0]]),
    'forward_taps': ('plan', 'f32', 5, True, _taps),
    'forward_linear_taps': ('plan', 'f32', 5, True, _linear_taps),
    'forward_ddv': ('plan', 'f32', 4, False, _ddv),
    'forward_stats': ('plan', 'f32', 5, False, _stats),
}


@pytest.mark.parametrize('case', sorted(VIT_CASES))
def test_warm_capture_equals_eager_and_rereads_input(vit, case):
    kind, inp, n, has_out, call = VIT_CASES[case]
    lut = vit['lut']
    if case == 'forward_uint8_nhwc':
        call = lambda p, x, out: [p.forward_uint8(x, lut(p), BITS, 'NHWC', out=out)]
    elif case == 'forward_uint8_nchw':
        call = lambda p, x, out: [p.forward_uint8(x, lut(p), BITS, 'NCHW', out=out)]
    elif case == 'forward_uint8_streams':
        call = lambda p, x, out: [p.forward_uint8_streams(x, lut(p), BITS, out, 'NHWC', n_streams=2, slices=SLICES)]
    x0, x1 = {'f32': (vit['x0'], vit['x1']), 'u8': (vit['u0'], vit['u1']), 'u8_nchw': (_nchw(vit['u0']), _nchw(vit['u1']))}[inp]
    _static_protocol(call, vit[kind], x0[:n].contiguous(), x1[:n].contiguous(), (n, vit['classes']) if has_out else None)


# ---- 2. cold capture of the ViT plan ----------------------------------------------------------------------------------------------------------
def test_cold_capture_of_the_vit_plan(vit, E):
    """A plan that has run no forward: the workspace, the slice workspaces and the side streams are first touched inside the capture.
    hipFuncSetAttribute (the dynamic-LDS grant of the launchers) is a host-side function attribute with no stream-capture status among
    its results (hip_runtime_api.h), so a cold capture records like a warm one (DESIGN, "Graph capture of the forwards")."""
    ref = vit['plan']()
    x0, x1 = vit['x0'], vit['x1']
    want0, want1 = ref.forward(x0, BITS).clone(), ref.forward(x1, BITS).clone()
    assert not torch.equal(want0, want1)
    idx = torch.cuda.current_device()
    for sliced in (False, True):
        plan = vit['plan']()
        assert plan._ws is None and plan._ws_multi == []
        saved = E._SIDE_STREAMS.pop(idx, None)      # the pool of this device unchosen, as in a process whose first sliced forward is captured
        try:
            x, out = x0.clone(), torch.empty_like(want0)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if sliced:
                    plan.forward_streams(x, BITS, out, n_streams=2, slices=SLICES)
                else:
                    plan.forward(x, BITS, out=out)
            assert idx not in E._SIDE_STREAMS, 'a capture must leave the side-stream pool unchosen'
            _fill(out)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want0), sliced
            x.copy_(x1)
            _fill(out)
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want1), sliced
            del g
            out2 = torch.empty_like(want0)
            plan.forward_streams(x0, BITS, out2, n_streams=2, slices=SLICES)      # eager: now the pool is probed and chosen
            torch.cuda.synchronize()
            assert idx in E._SIDE_STREAMS
            assert torch.equal(out2, want0), sliced
        finally:
            if saved is not None:
                E._SIDE_STREAMS[idx] = saved        # the process keeps the one probed set it had


# ---- 3. Swin ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def swin(dva):
    from diff_vit_amd import data as D
    m, x = R.micro_swin(dva, n_images=10)
    m.cuda()
    L = m.bit_config_length()
    mean, std, _ = D.MODEL_STATS['deit']
    u = dva.synth.images_uint8(6, 10, 56).cuda()
    return dict(m=m, x0=x[:5].cuda(), x1=x[5:].cuda(), u0=u[:5].contiguous(), u1=u[5:].contiguous(), A=[8] * L,
                B=[8 if i % 2 == 0 else 4 for i in range(L)], make=lambda: m.freeze('cuda', bits=8), lut32=D.uint8_lut(mean, std))


def _swin_lut(swin, p):
    if '_capture_test_lut' not in p.__dict__:
        p.__dict__['_capture_test_lut'] = p.input_lut(swin['lut32'])
    return p.__dict__['_capture_test_lut']


@pytest.mark.parametrize('case', ['single', 'sliced', 'uint8', 'uint8_sliced', 'bit_list', 'bit_list_sliced'])
def test_swin_warm_capture(swin, case):
    sl = dict(n_streams=2, slices=SLICES) if case.endswith('sliced') else {}
    if case.startswith('uint8'):
        call, x0, x1 = (lambda p, x, out: [p.forward_uint8(x, _swin_lut(swin, p), **sl)]), swin['u0'], swin['u1']
    else:
        cfg = swin['B'] if case.startswith('bit_list') else None
        call, x0, x1 = (lambda p, x, out: [p.forward(x, bit_config=cfg, **sl)]), swin['x0'], swin['x1']
    _static_protocol(call, swin['make'], x0, x1)


def test_swin_bit_list_is_baked_at_capture_time(swin):
    """the op table is read when p2v_run_ops is called: a later eager forward under another list moves the recording (``_switch``), the
    graph goes on computing the list it was captured under"""
    plan, ref = swin['make'](), swin['make']()
    A, Bl, x0 = swin['A'], swin['B'], swin['x0']
    want_a, want_b = ref.forward(x0, bit_config=A).clone(), ref.forward(x0, bit_config=Bl).clone()
    assert not torch.equal(want_a, want_b)
    plan.forward(x0, bit_config=Bl)
    plan.forward(x0, bit_config=A)
    x = x0.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan.forward(x, bit_config=A)
    assert torch.equal(plan.forward(x0, bit_config=Bl), want_b)          # eager, triggers _switch on the captured recording
    assert plan._recorded[(5, 0, True)]['cfg'] == tuple(Bl)
    _fill(out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)


def _swin_state(plan):
    """what a refused capture must leave alone: the recordings and their widths, the frozen codes, fragment copies, RESID tables, scales"""
    forms = sorted((d['name'], k, f['wf'] is not None, f['tab'] is not None) for d in plan._layers for k, f in d['forms'].items())
    widths = sorted((d['name'], b) for d in plan._layers for b in d['width'])
    return sorted((repr(k), r['cfg']) for k, r in plan._recorded.items()), forms, widths, len(plan._keep), list(plan.resid_prefolded)


def _refused_capture(fn):
    """``fn()`` inside a capture raises the RuntimeError that names the capture; the capture stays valid (its one recorded launch replays)"""
    marker = torch.zeros(1, device='cuda')
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match='capturing'):
        with torch.cuda.graph(g):
            marker.add_(1)
            fn()
    g.replay()
    torch.cuda.synchronize()
    assert float(marker) == 1.0


def test_swin_cold_capture_is_refused_and_leaves_the_plan_alone(swin):
    ref = swin['make']()
    A, Bl, x0, x1 = swin['A'], swin['B'], swin['x0'], swin['x1']
    want = {(n, tag): ref.forward(x0[:n], bit_config=cfg).clone() for n in (3, 5) for tag, cfg in (('A', A), ('B', Bl))}
    # (a) a fresh plan: nothing frozen, nothing recorded
    plan = swin['make']()
    before = _swin_state(plan)
    assert before[0] == [] and before[1] == []
    x = x0.clone()
    _refused_capture(lambda: plan.forward(x))
    assert _swin_state(plan) == before
    assert torch.equal(plan.forward(x0), want[(5, 'A')])                          # the same call, eagerly, right afterwards
    # (b) a warm plan, a batch size it has not seen
    before = _swin_state(plan)
    x3 = x0[:3].clone()
    _refused_capture(lambda: plan.forward(x3))
    assert _swin_state(plan) == before
    assert torch.equal(plan.forward(x0[:3]), want[(3, 'A')])
    # (b') a slicing it has not seen: refused before the fork, so the capture ends joined
    before = _swin_state(plan)
    _refused_capture(lambda: plan.forward(x, n_streams=2, slices=SLICES))
    assert _swin_state(plan) == before
    assert torch.equal(plan.forward(x0, n_streams=2, slices=SLICES), want[(5, 'A')])
    # (c) a warm plan, a bit list whose 4-bit codes are not frozen (no freeze_all)
    before = _swin_state(plan)
    _refused_capture(lambda: plan.forward(x, bit_config=Bl))
    assert _swin_state(plan) == before and plan._recorded[(5, 0, True)]['cfg'] == tuple(A)
    assert torch.equal(plan.forward(x0, bit_config=A), want[(5, 'A')])
    assert torch.equal(plan.forward(x0, bit_config=Bl), want[(5, 'B')])
    # (d) freeze_all and an eager warm-up of the batch: now the capture goes through
    plan2 = swin['make']().freeze_all()
    x = x0.clone()
    _refused_capture(lambda: plan2.forward(x, bit_config=Bl))                      # frozen, but batch 5 is not recorded yet
    plan2.forward(x0, bit_config=Bl)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = plan2.forward(x, bit_config=Bl)
    _fill(out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want[(5, 'B')])
    x.copy_(x1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref.forward(x1, bit_config=Bl))
    # the event-timed replay and a plan built inside a capture are refused as well
    _refused_capture(lambda: plan2.profile(x))
    _refused_capture(swin['make'])
    assert isinstance(plan2.profile(x0), list)


# ---- 4. refusals: the second class of the DESIGN table ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def op_buffers(dva, E):
    """17-token micro shapes for the per-operator entry points: LayerNorm -> qkv GEMM -> attention, and a p2v_run_ops list"""
    from diff_vit_amd.plan import lis_consts
    g = torch.Generator().manual_seed(17)
    Bn, T, D, H = 3, 17, 64, 2
    rows = Bn * T

    def codes(*shape, lo=-128, hi=128):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int32).to(torch.int8).cuda()

    t = dict(Bn=Bn, T=T, D=D, H=H, rows=rows)
    t['xa'], t['xb'] = codes(rows, D), codes(rows, D)
    t['x'] = t['xa'].clone()
    t['mask'], t['post_mul'] = torch.ones(D).cuda(), torch.ones(D).cuda()
    t['gamma'] = (0.6 + 0.8 * torch.rand(D, generator=g)).cuda()
    t['beta'] = (0.1 * torch.randn(D, generator=g)).cuda()
    t['inv_out'] = torch.full((D,), 8.0).cuda()
    t['w'] = torch.zeros(256, 64, dtype=torch.int8).cuda()
    t['w'][:192] = codes(192, 64, lo=-20, hi=21)
    t['colscale'] = torch.full((256,), 2.0 ** -9).cuda()
    t['bias'] = torch.zeros(256).cuda()
    t['bias'][:192] = (0.1 * torch.randn(192, generator=g)).cuda()
    t['ln_out'] = torch.empty(rows, D, dtype=torch.int8, device='cuda')
    t['qkv'] = torch.empty(rows, 3 * D, dtype=torch.int8, device='cuda')
    t['att'] = torch.empty(rows, D, dtype=torch.int8, device='cuda')
    t['pooled'] = torch.empty(Bn, 3 * D, dtype=torch.int8, device='cuda')
    t['ln'] = E.Ln(2.0 ** -4, E.ptr(t['mask']), E.ptr(t['gamma']), E.ptr(t['beta']), E.ptr(t['inv_out']), E.ptr(t['post_mul']))
    t['lin'] = E.Linear(E.ptr(t['w']), E.ptr(t['colscale']), E.ptr(t['bias']))
    t['epi'] = E.Epilogue()
    t['epi'].inv_s_out = 4.0
    x0_, b_, c_ = lis_consts(torch.tensor(0.125))
    t['attn'] = E.Attn(2.0 ** -4, float(torch.tensor(32.0) ** -0.5), 8.0, 4.0, x0_, b_, c_)
    ops = (E.Op * 3)()
    ops[0].kind, ops[0].inp, ops[0].out = E.OP_LAYERNORM, E.ptr(t['x']), E.ptr(t['ln_out'])
    ops[0].M, ops[0].N, ops[0].lda, ops[0].ldo, ops[0].ln = rows, D, D, D, t['ln']
    ops[1].kind, ops[1].epi, ops[1].inp, ops[1].out = E.OP_GEMM, E.EPI_REQUANT, E.ptr(t['ln_out']), E.ptr(t['qkv'])
    ops[1].M, ops[1].K, ops[1].N, ops[1].lda, ops[1].ldo, ops[1].lin, ops[1].ep = rows, D, 3 * D, D, 3 * D, t['lin'], t['epi']
    ops[2].kind, ops[2].inp, ops[2].out = E.OP_AVGPOOL, E.ptr(t['qkv']), E.ptr(t['pooled'])
    ops[2].i0, ops[2].i1, ops[2].i2, ops[2].f0, ops[2].f1 = Bn, T, 3 * D, 2.0 ** -2, 2.0 ** 3
    t['ops'] = ops
    return t


def _operators(E, t):
    L, st = E.lib(), E.stream_ptr()
    E.check(L.p2v_int_layernorm(E.ptr(t['x']), t['D'], t['rows'], t['D'], C.byref(t['ln']), E.ptr(t['ln_out']), t['D'], st))
    E.check(L.p2v_gemm_i8(E.EPI_REQUANT, E.ptr(t['ln_out']), t['D'], t['rows'], t['D'], 3 * t['D'], C.byref(t['lin']), C.byref(t['epi']),
                          E.ptr(t['qkv']), 3 * t['D'], None, st))
    E.check(L.p2v_lis_attention(E.ptr(t['qkv']), t['Bn'], t['T'], t['H'], t['D'] // t['H'], C.byref(t['attn']), E.ptr(t['att']), None, st))
    return [t['ln_out'], t['qkv'], t['att']]


def _run_ops(E, t):
    E.check(E.lib().p2v_run_ops(t['ops'], 3, E.stream_ptr()))
    return [t['ln_out'], t['qkv'], t['pooled']]


@pytest.fixture(scope='module')
def refusal_ctx(vit, E, op_buffers):
    """a warm plan with everything the refused calls take, allocated and prepared ahead of any capture"""
    L = E.lib()
    plan = vit['plan']()
    x = vit['x0']
    c = dict(plan=plan, x=x, want=plan.forward(x, BITS).clone(), ws=plan.workspace(5), cfg=plan._cfg(BITS),
             logits=torch.empty(5, vit['classes'], device='cuda'))
    plan.forward_grams(x, BITS)                        # (p2v_plan_prepare_grams is a plan-time call: made here)
    c['f32'] = [torch.randn(5, 40, device='cuda'), torch.randn(5, 3, 24, device='cuda')]
    c['i8'] = [torch.randint(-128, 128, (5, 4, 32), dtype=torch.int32).to(torch.int8).cuda()]
    built = [k[1] for k, v in E._GELU_TABLES.items() if v[1] is not None]      # a scale whose table the plan's build has proven
    c['gelu_inv_s'] = built[0] if built else 16.0
    tab = E.GeluTab()
    assert L.p2v_gelu_table_plan(c['gelu_inv_s'], C.byref(tab)) == 0
    c['gelu_table'] = torch.empty(tab.cells * 2, dtype=torch.int32, device='cuda')
    c['gelu_scratch'] = torch.empty(L.p2v_gelu_table_scratch_bytes(tab.cells), dtype=torch.uint8, device='cuda')
    tab.table = E.ptr(c['gelu_table'])
    c['gelu'] = tab
    t = op_buffers
    c['vecs'] = [(0.01 + 0.02 * torch.rand(128)).cuda() for _ in range(3)]
    c['r_epi'] = E.Epilogue()
    c['r_epi'].s_mid, c['r_epi'].s_res, c['r_epi'].s_next = [E.ptr(v) for v in c['vecs']]
    c['r_tab'] = torch.empty(L.p2v_resid_prefold_bytes(64) // 4, device='cuda')
    c['ms'], c['kind'], c['n_max'] = plan._profile_buffers()
    torch.cuda.synchronize()
    return c


def _py(fn):
    """a Python wrapper as (status, message): E.check raises NotImplementedError for P2V_E_UNSUPPORTED, with p2v_last_error() as its text"""
    def run(E, c):
        try:
            fn(E, c)
        except NotImplementedError as e:
            return E.E_UNSUPPORTED, str(e)
        return 0, ''
    return run


def _c(fn):
    """a call at the C boundary as (status, p2v_last_error())"""
    def run(E, c):
        rc = fn(E, c)
        return rc, E.lib().p2v_last_error().decode()
    return run


def _profile_args(E, c):
    p = c['plan']
    return (p._handle, E.ptr(c['x']), 5, c['cfg'], 10, E.ptr(c['logits']), E.ptr(c['ws']), c['ws'].numel(), E.stream_ptr())


def _profile_begin(E, c):
    tok = C.c_void_p()
    rc = E.lib().p2v_forward_profile_begin(*_profile_args(E, c), C.byref(tok))
    if rc == 0:
        assert E.lib().p2v_forward_profile_end(tok, c['ms'], c['kind'], c['n_max']) > 0
    else:
        assert not tok.value
    return rc


# The second class of the table in DESIGN.md, "Graph capture of the forwards": every entry point that takes a stream and cannot be recorded,
# at the C boundary and through the Python wrappers above it (the plan-time calls without a stream are documented there, not checked here)
REFUSED = {
    'p2v_forward_profile': _c(lambda E, c: min(0, E.lib().p2v_forward_profile(*_profile_args(E, c), c['ms'], c['kind'], c['n_max']))),
    'p2v_forward_profile_begin': _c(_profile_begin),
    'p2v_run_ops_profile': _c(lambda E, c: E.lib().p2v_run_ops_profile(c['opb']['ops'], 3, E.stream_ptr(), (C.c_float * 3)())),
    'p2v_gelu_table_build': _c(lambda E, c: E.lib().p2v_gelu_table_build(c['gelu_inv_s'], C.byref(c['gelu']), E.ptr(c['gelu_scratch']),
                                                                      c['gelu_scratch'].numel(), E.stream_ptr())),
    'p2v_resid_prefold': _c(lambda E, c: E.lib().p2v_resid_prefold(C.byref(c['opb']['lin']), C.byref(c['r_epi']), 64, E.ptr(c['r_tab']),
                                                                   c['r_tab'].numel() * 4, C.byref(C.c_int(0)), E.stream_ptr())),
    'p2v_pair_cosine': _py((lambda E, c: torch.ops.p2vit.pair_cosine(c['f32'], [t.flip(0) for t in c['f32']], [None, None]))),
    'p2v_cka_grams': _py((lambda E, c: torch.ops.p2vit.cka_grams(c['f32'], []))),
    'p2v_code_grams': _py((lambda E, c: torch.ops.p2vit.code_grams(c['i8'] + c['f32'][:1], [None, None]))),
    'p2v_forward_grams': _py((lambda E, c: c['plan'].forward_grams(c['x'], BITS, with_linear=True))),
    'FrozenPlan.profile': _py((lambda E, c: c['plan'].profile(c['x'], BITS))),
    'FrozenPlan.profile_streams': _py((lambda E, c: c['plan'].profile_streams(c['x'], BITS, n_streams=2, slices=SLICES))),
}


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_uncapturable_call_refuses_and_keeps_the_capture_valid(refusal_ctx, op_buffers, E, name):
    c = dict(refusal_ctx, opb=op_buffers)
    call = REFUSED[name]
    plan, x = c['plan'], c['x'].clone()
    out = torch.empty_like(c['want'])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc, msg = call(E, c)
        plan.forward(x, BITS, out=out)               # enqueued behind the refusal, in the same capture
    assert rc == E.E_UNSUPPORTED, (name, rc, msg)
    assert 'capturing' in msg, msg
    assert not name.startswith('p2v_') or msg.startswith(name + ':'), msg
    _fill(out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, c['want']), name         # the capture stayed valid and recorded the forward alone
    del g
    assert call(E, c)[0] == 0, (name, E.lib().p2v_last_error())   # outside the capture the call behaves as before
    torch.cuda.synchronize()
    assert torch.equal(plan.forward(c['x'], BITS), c['want'])


def test_profile_end_refuses_while_its_stream_captures(refusal_ctx, E):
    """a pass begun before the capture cannot be ended inside it (the call waits for an event); the token stays valid"""
    c, L = refusal_ctx, E.lib()
    g = torch.cuda.CUDAGraph()
    ctx = torch.cuda.graph(g)
    tok = C.c_void_p()
    with torch.cuda.stream(ctx.capture_stream):      # eagerly, on the stream the capture below records
        assert L.p2v_forward_profile_begin(*_profile_args(E, c), C.byref(tok)) == 0 and tok.value
    marker = torch.zeros(1, device='cuda')
    with ctx:
        marker.add_(1)
        rc = L.p2v_forward_profile_end(tok, c['ms'], c['kind'], c['n_max'])
        msg = L.p2v_last_error().decode()
    assert rc == E.E_UNSUPPORTED and 'capturing' in msg and msg.startswith('p2v_forward_profile_end:'), (rc, msg)
    g.replay()
    torch.cuda.synchronize()
    assert float(marker) == 1.0
    assert L.p2v_forward_profile_end(tok, c['ms'], c['kind'], c['n_max']) > 0


def test_plan_construction_inside_a_capture_is_refused(vit):
    _refused_capture(vit['plan'])
    plan = vit['plan']()
    assert torch.equal(plan.forward(vit['x0'], BITS), vit['plan']().forward(vit['x0'], BITS))


def test_forward_grams_before_prepare_is_refused_without_touching_the_capture(vit):
    """a plan whose Gram scales are not prepared yet: p2v_plan_prepare_grams synchronises the device, so the wrapper refuses ahead of it"""
    plan = vit['plan']()
    plan.forward(vit['x0'], BITS)
    _refused_capture(lambda: plan.forward_grams(vit['x0'], BITS))
    assert not getattr(plan, '_grams_ready', False)
    out, names, grams, units = plan.forward_grams(vit['x0'], BITS)
    ref = vit['plan']().forward_grams(vit['x0'], BITS)
    assert torch.equal(grams, ref[2]) and torch.equal(units, ref[3]) and torch.equal(out, ref[0])


# ---- 5. the operator entry points the plans are built from -----------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['operators', 'run_ops'])
def test_operator_entry_points_capture(op_buffers, E, which):
    """p2v_int_layernorm -> p2v_gemm_i8 -> p2v_lis_attention, and one p2v_run_ops list, recorded straight from the C boundary"""
    t = op_buffers
    run = _operators if which == 'operators' else _run_ops
    want = {}
    for tag in ('xa', 'xb'):
        t['x'].copy_(t[tag])
        want[tag] = _clones(run(E, t))
    for r in want['xa']:
        assert r.min() < r.max()                       # (not saturated into one code)
    assert not all(torch.equal(a, b) for a, b in zip(want['xa'], want['xb']))
    t['x'].copy_(t['xa'])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = run(E, t)
    for tag in ('xa', 'xb', 'xa'):
        t['x'].copy_(t[tag])
        for r in res:
            _fill(r)
        g.replay()
        torch.cuda.synchronize()
        _same(res, want[tag], (which, tag))
