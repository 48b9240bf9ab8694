"""GPU: the weight-freeze kernel (p2v_freeze_weights) byte for byte against the four host functions, its footprint and refusals; the Swin
plan under per-layer bit lists against the MIXED oracle (tests/_swin_bits_ref.py) and against its own single-width forwards."""
import ctypes as C
import random

import pytest
import torch

import _swin_bits_ref as R

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


@pytest.fixture(scope='module')
def micro(dva, E):
    """the calibrated micro Swin on the GPU with its plan (default width 8, everything frozen), its images and the oracle's logits of
    every list of R.bit_lists on the first two images (computed once)"""
    m, x = R.micro_swin(dva)
    L = m.bit_config_length()
    lists = R.bit_lists(L)
    want = [R.mixed_oracle(m, x[:2], bl) for bl in lists]
    m.cuda()
    plan = m.freeze('cuda', bits=8)
    plan.freeze_all()
    return dict(m=m, x=x.cuda(), plan=plan, L=L, lists=lists, want=want)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _host_rows(w, s, bits):
    """the padded row-major codes as SwinPlan._linear made them on the host"""
    N, K = w.shape
    lo, hi = (-128, 127) if bits == 8 else (-8, 7)
    codes = torch.clamp(torch.round(w / s.reshape(-1, 1)), lo, hi)
    wp = torch.zeros((N + 127) // 128 * 128, (K + 63) // 64 * 64, dtype=torch.int8)
    wp[:N, :K] = codes.to(torch.int8)
    return wp


def _weights(N, K, s, seed):
    """fp32 [N, K] around the scales ``s`` (1 or N values): every tie (c + 0.5) * s of both widths, values beyond both clamp edges, the
    edges themselves, zeros of both signs and a seeded spread"""
    g = torch.Generator().manual_seed(seed)
    sv = s.reshape(-1, 1).expand(N, 1) if s.numel() == N else s.reshape(1, 1).expand(N, 1)
    ties = torch.arange(-131, 131, dtype=torch.float32) + 0.5
    special = torch.tensor([0.0, -0.0, 127.0, 128.0, -128.0, -129.0, 7.0, 8.0, -8.0, -9.0, 1000.0, -1000.0, 7.4999, -8.5001, 127.5001, 3e38, -3e38])
    base = torch.cat([ties, special])
    units = (torch.randn(N * K, generator=g) * 6.0)
    units[torch.randperm(N * K, generator=g)[:base.numel()]] = base          # N * K >= 480 > 279: every special value lands somewhere
    assert N * K >= base.numel()
    return (units.reshape(N, K) * sv).contiguous()


def _place(w, ldw):
    """``w`` on the GPU in rows ``ldw`` floats apart, the first one 4 bytes behind a 16-byte boundary when ldw != K"""
    N, K = w.shape
    if ldw == K:
        return w.cuda()
    flat = torch.full((N * ldw + 1,), float('nan'), device='cuda')
    view = flat[1:].view(N, ldw)[:, :K]
    view.copy_(w)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == ldw
    return view


SHAPES = [(10, 128), (64, 48), (192, 64), (128, 256), (130, 200)]


@pytest.mark.parametrize('N,K', SHAPES)
def test_freeze_weights_equals_host_layouts(E, N, K):
    host = {E.W_ROWS_I8: lambda wp: wp, E.W_FRAG_I8: E.fragment_order, E.W_TILES_P4: E.pack_int4_tiles, E.W_FRAG_P4: E.fragment_order_packed4}
    scales = {'tensor_pot': torch.tensor([2.0 ** -6]), 'tensor_odd': torch.tensor([0.0123]),
              'row_pot': 2.0 ** -torch.arange(N).remainder(9).float(), 'row_odd': 0.003 + 0.0007 * torch.arange(N).float()}
    n = 0
    for tag, s in scales.items():
        w = _weights(N, K, s, seed=N * 1000 + K)
        for ldw in (K, K + 3):
            wd, sd = _place(w, ldw), s.cuda()
            for bits, layouts in ((8, (E.W_ROWS_I8, E.W_FRAG_I8)), (4, (E.W_ROWS_I8, E.W_FRAG_I8, E.W_TILES_P4, E.W_FRAG_P4))):
                wp = _host_rows(w, s, bits)
                for lay in layouts:
                    got = E.freeze_weights(wd, sd, bits, lay).cpu()
                    want = host[lay](wp)
                    assert got.dtype == want.dtype and got.shape == want.shape, (tag, ldw, bits, lay)
                    assert torch.equal(got, want), (tag, ldw, bits, lay, int((got != want).sum()))
                    n += 1
    assert n == 4 * 2 * 6
    assert int(_host_rows(w, s, 8).min()) == -128 and int(_host_rows(w, s, 8).max()) == 127        # both clamp edges were reached


def test_freeze_weights_footprint(E):
    L = E.lib()
    for N, K in ((10, 128), (130, 200)):
        w, s = _place(_weights(N, K, torch.tensor([0.02]), 3), K + 3), torch.tensor([0.02]).cuda()
        n_pad, k_pad = (N + 127) // 128 * 128, (K + 63) // 64 * 64
        for lay, bits in ((E.W_ROWS_I8, 8), (E.W_FRAG_I8, 4), (E.W_TILES_P4, 4), (E.W_FRAG_P4, 4)):
            nbytes = L.p2v_freeze_bytes(N, K, lay)
            assert nbytes == n_pad * k_pad // (2 if lay in (E.W_TILES_P4, E.W_FRAG_P4) else 1)
            buf = torch.full((nbytes + 4096,), 0x5A, dtype=torch.uint8, device='cuda')
            E.check(L.p2v_freeze_weights(E.ptr(w), w.stride(0), N, K, E.ptr(s), 1, bits, lay, E.ptr(buf), nbytes, E.stream_ptr()))
            torch.cuda.synchronize()
            assert bool((buf[nbytes:] == 0x5A).all()), (N, K, lay)
            assert torch.equal(buf[:nbytes].cpu(), E.freeze_weights(w, s, bits, lay).cpu().reshape(-1).view(torch.uint8)), (N, K, lay)
    assert L.p2v_freeze_bytes(0, 64, 0) == 0 and L.p2v_freeze_bytes(64, 0, 0) == 0
    assert L.p2v_freeze_bytes(64, 64, 4) == 0 and L.p2v_freeze_bytes(64, 64, -1) == 0


def test_freeze_weights_refusals(E):
    L = E.lib()
    N, K = 10, 48
    w, s1, sn = torch.ones(N, K, device='cuda'), torch.ones(1, device='cuda'), torch.ones(N, device='cuda')
    nbytes = L.p2v_freeze_bytes(N, K, E.W_ROWS_I8)
    out = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device='cuda')
    st = E.stream_ptr()

    def call(w_=w, ldw=K, N_=N, K_=K, s_=s1, ns=1, bits=8, lay=E.W_ROWS_I8, out_=out, nb=nbytes):
        return L.p2v_freeze_weights(E.ptr(w_), ldw, N_, K_, E.ptr(s_), ns, bits, lay, E.ptr(out_), nb, st)
    assert call(w_=None) == E.E_ARG and call(s_=None) == E.E_ARG and call(out_=None) == E.E_ARG
    assert call(N_=0) == E.E_SHAPE and call(K_=0) == E.E_SHAPE and call(K_=-5) == E.E_SHAPE
    assert call(ldw=K - 1) == E.E_SHAPE
    assert call(ns=0) == E.E_SHAPE and call(ns=2) == E.E_SHAPE and call(s_=sn, ns=N + 1) == E.E_SHAPE
    assert call(nb=nbytes - 1) == E.E_WORKSPACE and call(nb=0) == E.E_WORKSPACE
    assert call(bits=8, lay=E.W_TILES_P4, nb=nbytes) == E.E_BITS and call(bits=8, lay=E.W_FRAG_P4) == E.E_BITS
    assert call(bits=6) == E.E_BITS
    assert b'p2v_freeze_weights' in L.p2v_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())                      # nothing was launched
    assert call(s_=sn, ns=N) == 0 and call() == 0
    torch.cuda.synchronize()
    assert not bool((out == 0x5A).all())


# ---- 2. the plan under bit lists ------------------------------------------------------------------------------------------------------------
def test_micro_swin_lists_equal_the_mixed_oracle(micro):
    m, x = micro['m'], micro['x'][:2]
    assert len(micro['lists']) == 5 + micro['L']
    with torch.no_grad():
        for bl, want in zip(micro['lists'], micro['want']):
            got = m(x, bits=bl).cpu()
            assert torch.equal(got, want), (bl, float((got - want).abs().max()))
    # the single-4 lists are told apart: each differs from the all-8 logits
    assert all(not torch.equal(w, micro['want'][0]) for w in micro['want'][5:])


def test_list_equivalences(dva, micro):
    m, x, L = micro['m'], micro['x'], micro['L']
    with torch.no_grad():
        o8, o4 = m(x, bits=8).clone(), m(x, bits=4).clone()
        assert m._plan is micro['plan'] and m._plan.bits == 4                  # no rebuild: the int moved the default width
        assert torch.equal(m(x, bits=[8] * L), o8) and torch.equal(m(x, bits=[4] * L), o4)
        assert torch.equal(m(x, bits=8), o8) and m._plan is micro['plan'] and m._plan.bits == 8
        assert torch.equal(m._plan.forward(x), o8) and torch.equal(m._plan.forward(x, bit_config=[4] * L), o4)
        assert not torch.equal(o8, o4)
        # int8-stored 4-bit codes give what the packed ones give
        m2, _ = R.micro_swin(dva)
        m2.cuda()
        p2 = m2.freeze('cuda', bits=4, pack4=False)
        mixed = micro['lists'][3]
        assert torch.equal(p2.forward(x), o4) and torch.equal(p2.forward(x, bit_config=mixed), m(x, bits=mixed))
        assert all(k[1] is False for d in p2._layers for k in d['forms']) and any(k[1] for d in micro['plan']._layers for k in d['forms'])


def test_forward_uint8_with_a_list(dva, micro):
    from diff_vit_amd import data
    m, L = micro['m'], micro['L']
    bl = micro['lists'][4]
    u8 = dva.synth.images_uint8(7, 3, 56)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    with torch.no_grad():
        got = m.forward_uint8(u8.cuda(), bl, mean, std, 'NHWC')
        want = m(data.normalize_uint8(u8, mean, std, 'NHWC').cuda(), bits=bl)
        assert torch.equal(got, want)
        assert not torch.equal(got, m.forward_uint8(u8.cuda(), 8, mean, std, 'NHWC'))
        with pytest.raises(ValueError):
            m.forward_uint8(u8.cuda(), bl[:-1], mean, std, 'NHWC')


def test_sliced_forward_with_a_list(dva, micro):
    plan, bl = micro['plan'], micro['lists'][2]
    x = dva.synth.images(23, 50, 56).cuda()                 # 50 >= 16 * 3: three slices on three streams
    with torch.no_grad():
        single = plan.forward(x, n_streams=1, bit_config=bl)
        assert torch.equal(plan.forward(x, n_streams=3, bit_config=bl), single)
        assert torch.equal(plan.forward(x, n_streams=3, bit_config=bl), single)          # (the threaded enqueue, once recorded)
        other = micro['lists'][3]
        assert torch.equal(plan.forward(x, n_streams=3, bit_config=other), plan.forward(x, n_streams=1, bit_config=other))
        assert torch.equal(plan.forward(x, n_streams=3, slices=[20, 17, 13], bit_config=bl), single)


def test_window12_geometry_with_a_list(dva):
    m, x = R.micro_swin(dva, 'swin_micro_patch4_window12_96', 96, 2)
    L = m.bit_config_length()
    bl = [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]
    assert 4 in bl and 8 in bl
    want = R.mixed_oracle(m, x, bl)
    m.cuda()
    with torch.no_grad():
        got = m(x.cuda(), bits=bl).cpu()
    assert torch.equal(got, want), float((got - want).abs().max())


def test_lists_in_turn_do_not_grow_memory(micro):
    plan, x, L = micro['plan'], micro['x'], micro['L']
    r = random.Random(9)
    lists = []
    while len(lists) < 40:
        bl = [r.choice((4, 8)) for _ in range(L)]
        if bl not in lists:
            lists.append(bl)
    plan.freeze_all()
    outs, mem = [], None
    with torch.no_grad():
        for i, bl in enumerate(lists):
            outs.append(plan.forward(x, bit_config=bl).cpu())
            torch.cuda.synchronize()
            if i == 2:
                mem = torch.cuda.memory_allocated()
            elif i > 2:
                assert torch.cuda.memory_allocated() == mem, (i, torch.cuda.memory_allocated() - mem)
        assert torch.equal(plan.forward(x, bit_config=lists[0]).cpu(), outs[0])
    assert len({o.numpy().tobytes() for o in outs}) > 30
    assert len([k for k in plan._recorded if isinstance(k[0], int) and k[0] == x.shape[0] and k[2] is True]) == 1         # one recording per (batch, slot), whatever the list


def test_model_diff_after_mixed_forwards(dva, micro):
    """forward_ddv / forward_linear_taps of a plan that has served mixed lists = those of a fresh single-width plan"""
    m, x, plan = micro['m'], micro['x'], micro['plan']
    x4 = torch.cat([x[:2], x[:2] + 0.01])
    with torch.no_grad():
        for bl in micro['lists'][2:5]:
            plan.forward(x, bit_config=bl)
        for bits in (8, 4):
            m(x, bits=bits)                                    # moves the default width of the SAME plan
            assert m._plan is plan and plan.bits == bits
            fresh_m, _ = R.micro_swin(dva)
            fresh = fresh_m.cuda().freeze('cuda', bits=bits)
            lg, names, sums = plan.forward_ddv(x4, with_linear=True)
            lg2, names2, sums2 = fresh.forward_ddv(x4, with_linear=True)
            assert names == names2 and torch.equal(lg, lg2) and torch.equal(sums, sums2)
            assert torch.equal(lg, plan.forward(x4))
            out, taps = plan.forward_linear_taps(x)
            out2, taps2 = fresh.forward_linear_taps(x)
            assert torch.equal(out, out2) and len(taps) == len(taps2) == micro['L']
            assert all(torch.equal(a, b) for a, b in zip(taps, taps2))
            with pytest.raises(NotImplementedError):
                plan.forward(x, taps={}, bit_config=[8] * micro['L'])
        m(x, bits=8)
