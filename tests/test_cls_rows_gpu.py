"""GPU: the last ViT block on the class-token rows only (switch "cls_rows"), the few-rows GEMM kernel (switch "gemm_rows") against the
tiled kernel and the oracle, and p2v_lis_attention_rows against p2v_lis_attention.  Every comparison is bit equality."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

from conftest import golden_calib, golden_weights, gpu_ok, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


# --------------------------------------------------------------------------------------------------
# 1. logits with the class-row path on and off, in one process
# --------------------------------------------------------------------------------------------------
def _on_off(L, fn):
    outs = []
    try:
        for v in (1, 0):
            assert L.p2v_set_tuning(b'cls_rows', v) == 0
            outs.append(fn().clone())
            torch.cuda.synchronize()
    finally:
        L.p2v_set_tuning(b'cls_rows', 1)
    return outs


def _check_plan(dva, plan, size, bit_lists, batches, seed):
    from diff_vit_amd import data as D
    L = dva.engine.lib()
    mean, std, _ = D.MODEL_STATS['deit']
    lut = plan.input_lut(D.uint8_lut(mean, std))
    classes = None
    for B in batches:
        x = dva.synth.images(seed, min(B, 32), size, offset=300)
        x = x.repeat((B + x.shape[0] - 1) // x.shape[0], 1, 1, 1)[:B].contiguous().cuda()
        u8 = dva.synth.images_uint8(seed + 1, min(B, 32), size)
        u8 = u8.repeat((B + u8.shape[0] - 1) // u8.shape[0], 1, 1, 1)[:B].contiguous().cuda()
        for bits in bit_lists:
            on, off = _on_off(L, lambda: plan.forward(x, bits))
            assert torch.equal(on, off), ('forward', B, bits[:6], int((on != off).sum()))
            classes = on.shape[1]

            def sliced():
                lg = torch.empty(B, classes, device='cuda')
                plan.forward_streams(x, bits, lg)
                torch.cuda.synchronize()
                return lg
            s_on, s_off = _on_off(L, sliced)
            assert torch.equal(s_on, s_off), ('forward_streams', B, bits[:6], int((s_on != s_off).sum()))
            assert torch.equal(s_on, on), ('forward_streams vs forward', B, bits[:6])
            u_on, u_off = _on_off(L, lambda: plan.forward_uint8(u8, lut, bits))
            assert torch.equal(u_on, u_off), ('forward_uint8', B, bits[:6], int((u_on != u_off).sum()))
            assert torch.isfinite(on).all() and on.abs().max() > 0


@pytest.mark.parametrize('name,batches', [('micro', (1, 3, 68)), ('deit_tiny', (1, 3, 68)), ('deit_small', (1, 3, 68, 256)), ('vit_base', (1, 3, 68))])
def test_logits_equal_with_class_rows_on_and_off(dva, oracle, name, batches):
    """p2v_forward / p2v_forward_u8, one call and sliced over the streams, with the reference's calibration state of the golden files: the
    logits do not change when the last block computes the class rows only; int8, packed int4 and the mixed list."""
    g = load_golden('micro_vit' if name == 'micro' else name)
    arch = dva.synth.ARCHS[name]
    sd = golden_weights(g) if name == 'micro' else dva.synth.vit_state_dict(arch, int(g['seed']))
    plan = dva.FrozenPlan(arch, sd, golden_calib(g, oracle))
    n = 4 * arch['depth'] + 2
    _check_plan(dva, plan, arch['img_size'], ([8] * n, [4] * n, [int(b) for b in g['bit_qmix']]), batches, 41)


@pytest.mark.parametrize('img,tokens', [(384, 577), (416, 677)])
def test_logits_equal_at_other_token_counts(dva, img, tokens):
    """577 tokens (384^2 / 16: the widest resident attention instantiations) and 677 (the streaming attention kernel, which computes
    every query row and leaves the row limit to the launches behind it)."""
    dim, depth, heads = 128, 2, 2
    m = dva.VisionTransformer(img_size=img, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, num_classes=40, mlp_ratio=4.0,
                              qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    arch = dict(img_size=img, patch_size=16, embed_dim=dim, depth=depth, num_heads=heads, num_classes=40, mlp_ratio=4.0)
    m.load_state_dict(dva.synth.vit_state_dict(arch, 33), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(33, 2, img).cuda())
    n = 4 * depth + 2
    m(dva.synth.images(33, 1, img).cuda(), [8] * n, False)          # freezes the plan
    plan = m._plan
    assert plan.tokens == tokens
    assert (tokens > dva.engine.lib().p2v_resident_tokens(dim // heads)) == (img == 416)
    _check_plan(dva, plan, img, ([8] * n, [4] * n, [8 if i % 3 else 4 for i in range(n)]), (1, 3, 20), 43)


def test_full_buffers_stay_readable_through_stop_after(dva, micro):
    """stop_after >= 0 computes every row of the last block whatever the switch says (the parity tests read them)."""
    arch = micro['arch']
    plan = dva.FrozenPlan(arch, micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    B, depth, D, T = x.shape[0], arch['depth'], arch['embed_dim'], plan.tokens
    bits = [8] * (4 * depth + 2)
    L = dva.engine.lib()
    views = []
    try:
        for v in (1, 0):
            assert L.p2v_set_tuning(b'cls_rows', v) == 0
            plan.forward(x, bits, stop_after=3 + 7 * depth)
            torch.cuda.synchronize()
            views.append(plan.view(B, 'x', B * T, D).clone())
    finally:
        L.p2v_set_tuning(b'cls_rows', 1)
    assert torch.equal(views[0], views[1])
    ref = micro['g']['taps/q8/blocks.%d.qact4' % (depth - 1)].reshape(B * T, D)
    assert np.array_equal(views[0].cpu().numpy().astype(np.int64), ref.astype(np.int64))


# --------------------------------------------------------------------------------------------------
# 3. the few-rows GEMM against the tiled GEMM (p2v_gemm_i8, "gemm_rows" 1 against 2) and against the oracle
# --------------------------------------------------------------------------------------------------
KINDS = ('requant', 'gelu_tab', 'gelu', 'resid', 'resid_pre')
SENT = 99


class _Layer:
    """one random layer (K, N) on the device: int8 or packed int4 weights, per-channel constants, RESID scales and table"""
    tables = usable = 0

    def __init__(self, dva, gen, K, N, w4, m_max, e_out=None):
        E = dva.engine
        self.E, self.K, self.N, self.w4 = E, K, N, w4
        n_pad = (N + 127) // 128 * 128
        w = torch.clamp(torch.round(torch.randn(N, K, generator=gen) * (3.5 if w4 else 30.0)), -8 if w4 else -128, 7 if w4 else 127)
        self.w = w
        wp = torch.zeros(n_pad, K, dtype=torch.int8)
        wp[:N] = w.to(torch.int8)
        self.s_x = 2.0 ** -5
        self.s_w = 2.0 ** -(torch.randint(2, 6, (N,), generator=gen).float() + (0 if w4 else 4))
        self.bias = torch.randn(N, generator=gen) * 0.4
        pad = lambda v: torch.cat([v, torch.zeros(n_pad - N)]).cuda()
        self.d = dict(w=(E.pack_int4_tiles(wp) if w4 else wp).cuda(), cs=pad(self.s_x * self.s_w), b=pad(self.bias))
        self.lin = E.Linear(E.ptr(self.d['w']), E.ptr(self.d['cs']), E.ptr(self.d['b']), None, 1 if w4 else 0)
        ptf = lambda base: base * 2.0 ** torch.randint(0, 4, (N,), generator=gen).float()
        self.s_mid, self.s_res, self.s_next = ptf(0.0131), ptf(0.0173), ptf(0.0209)
        self.d.update(sm=self.s_mid.cuda(), sr=self.s_res.cuda(), sn=self.s_next.cuda())
        self.e_req = e_out if e_out is not None else int(torch.randint(2, 5, (1,), generator=gen))
        self.e_gelu = e_out + 2 if e_out is not None else int(torch.randint(3, 7, (1,), generator=gen))
        self.x = torch.clamp(torch.round(torch.randn(m_max, K, generator=gen) * 40.0), -128, 127)
        self.res = torch.clamp(torch.round(torch.randn(m_max, N, generator=gen) * 50.0), -128, 127)
        self.tab = None

    def epilogue(self, kind, residual):
        E = self.E
        epi = E.Epilogue()
        if kind == 'requant':
            epi.inv_s_out = 2.0 ** self.e_req
            return E.EPI_REQUANT, epi
        if kind in ('gelu', 'gelu_tab'):
            epi.inv_s_out = 2.0 ** self.e_gelu
            if kind == 'gelu_tab':
                epi.gelu = E.gelu_table(2.0 ** self.e_gelu, 'cuda')
                assert epi.gelu.table and epi.gelu.cells > 10
            return E.EPI_GELU, epi
        epi.s_mid, epi.s_res, epi.s_next, epi.residual = E.ptr(self.d['sm']), E.ptr(self.d['sr']), E.ptr(self.d['sn']), E.ptr(residual)
        if kind == 'resid_pre':
            if self.tab is None:
                L = E.lib()
                nb = L.p2v_resid_prefold_bytes(self.N)
                tab = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
                usable = C.c_int(-1)
                E.check(L.p2v_resid_prefold(C.byref(self.lin), C.byref(epi), self.N, E.ptr(tab), nb, C.byref(usable), None))
                # about one random channel in 1e5 fails the exhaustive check of its table: the layer then runs the generic epilogue, as a plan does
                assert usable.value in (0, 1)
                self.tab = tab if usable.value == 1 else False
                _Layer.tables += 1
                _Layer.usable += usable.value
            if self.tab is not False:
                epi.resid_tab = E.ptr(self.tab)
        return E.EPI_RESID, epi

    def run(self, kind, M, rows_switch, strided=False):
        """-> the whole output buffer (for RESID: the residual buffer the call ran in place on)"""
        E, K, N = self.E, self.K, self.N
        L = E.lib()
        resid = kind.startswith('resid')
        lda = K + 64 if strided else K
        ldo = 2 * N + 16 if strided else N
        a = torch.full((M, lda), SENT, dtype=torch.int8)
        a[:, :K] = self.x[:M].to(torch.int8)
        a = a.cuda()
        out = torch.full((M, ldo), SENT, dtype=torch.int8)
        if resid:
            out[:, :N] = self.res[:M].to(torch.int8)
        out = out.cuda()
        k, epi = self.epilogue(kind, out)
        assert L.p2v_set_tuning(b'gemm_rows', rows_switch) == 0
        try:
            E.check(L.p2v_gemm_i8(k, E.ptr(a), lda, M, K, N, C.byref(self.lin), C.byref(epi), E.ptr(out), ldo, None, E.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            L.p2v_set_tuning(b'gemm_rows', 0)
        return out.cpu()

    def reference(self, oracle, kind, M):
        y = oracle.qgemm(self.x[:M], torch.tensor(self.s_x), self.w, self.s_w, self.bias)
        if kind == 'requant':
            return torch.clamp(torch.round(y / 2.0 ** -self.e_req), -128, 127)
        if kind in ('gelu', 'gelu_tab'):
            return torch.clamp(torch.round(oracle.gelu_rn(y) / 2.0 ** -self.e_gelu), -128, 127)
        q3 = torch.clamp(torch.round(y / self.s_mid), -128, 127)
        return torch.clamp(torch.round((self.res[:M] * self.s_res + q3 * self.s_mid) / self.s_next), -128, 127)


MS = (1, 2, 31, 52, 64, 65, 68, 128, 200, 256)


@pytest.mark.parametrize('w4', [False, True])
@pytest.mark.parametrize('K,N', [(384, 384), (384, 1536), (1536, 384), (192, 768), (768, 3072), (3072, 768), (448, 400)])
def test_row_gemm_equals_tiled_gemm(dva, K, N, w4):
    """every epilogue of the layer GEMMs, int8 and packed int4 weights: the output bytes of the row kernel are those of the tiled kernel;
    the RESID forms also in place on a strided residual buffer (lda > K, ldo > N) whose bytes between the rows stay untouched."""
    gen = torch.Generator().manual_seed(1000 + K + N + (7 if w4 else 0))
    lay = _Layer(dva, gen, K, N, w4, max(MS))
    for M in MS:
        for kind in KINDS:
            for strided in ((False, True) if kind.startswith('resid') else (False,)):
                rows = lay.run(kind, M, 1, strided)
                tiled = lay.run(kind, M, 2, strided)
                assert torch.equal(rows, tiled), (M, kind, strided, int((rows != tiled).sum()))
                assert bool((rows[:, N:] == SENT).all()), (M, kind, strided)
                assert int(rows[:, :N].to(torch.int32).abs().max()) > 0
    # an explicit tile height keeps meaning the tiled kernel, whatever "gemm_rows" says: same bytes again
    L = dva.engine.lib()
    assert L.p2v_set_tuning(b'gemm_tile', 128) == 0
    try:
        forced = lay.run('requant', 68, 1)
    finally:
        L.p2v_set_tuning(b'gemm_tile', 0)
    assert torch.equal(forced, lay.run('requant', 68, 1))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('w4', [False, True])
def test_row_gemm_vs_oracle(dva, oracle, kind, w4):
    """the row kernel against expectations built from the oracle's operations (qgemm, gelu_rn, IEEE divisions), as test_gemm_residual_epilogue
    builds them; e_out = 3 / 5 as there (the clamps are exercised)."""
    gen = torch.Generator().manual_seed(77)
    for K, N, M in ((384, 384, 68), (1536, 384, 130), (448, 400, 65)):
        lay = _Layer(dva, gen, K, N, w4, M, e_out=3)
        got = lay.run(kind, M, 1).float()
        ref = lay.reference(oracle, kind, M)
        assert torch.equal(got, ref), (kind, w4, K, N, int((got != ref).sum()))
        assert ref.abs().max() >= 127


def test_row_gemm_random_cases(dva, oracle):
    """240 seeded random cases (M <= 300, K, N, scales, epilogue, weight width): row kernel == tiled kernel on every byte, and every
    eighth case also against the oracle."""
    gen = torch.Generator().manual_seed(20240)
    n_cases = 240
    for case in range(n_cases):
        M = int(torch.randint(1, 301, (1,), generator=gen))
        K = 64 * int(torch.randint(1, 17, (1,), generator=gen))
        N = 16 * int(torch.randint(1, 41, (1,), generator=gen))
        kind = KINDS[int(torch.randint(0, len(KINDS), (1,), generator=gen))]
        w4 = bool(torch.randint(0, 2, (1,), generator=gen))
        strided = bool(torch.randint(0, 2, (1,), generator=gen))
        lay = _Layer(dva, gen, K, N, w4, M)
        rows = lay.run(kind, M, 1, strided)
        tiled = lay.run(kind, M, 2, strided)
        assert torch.equal(rows, tiled), (case, M, K, N, kind, w4, strided, int((rows != tiled).sum()))
        assert bool((rows[:, N:] == SENT).all()), (case, M, K, N, kind)
        if case % 8 == 0:
            assert torch.equal(rows[:, :N].float(), lay.reference(oracle, kind, M)), (case, M, K, N, kind, w4)
    assert _Layer.tables >= 20 and _Layer.usable >= _Layer.tables - 2              # the pre-folded form was what ran


# --------------------------------------------------------------------------------------------------
# 4. attention with a query-row limit
# --------------------------------------------------------------------------------------------------
ATTN_SHAPES = [(2, 17, 2, 32, 4), (3, 49, 4, 32, 5), (2, 197, 3, 64, 4), (1, 197, 6, 64, 6), (2, 50, 2, 64, 3),
               (1, 193, 2, 64, 5), (1, 224, 2, 64, 4), (1, 209, 1, 32, 4), (1, 64, 2, 64, 4), (1, 1, 1, 32, 4),
               (2, 65, 3, 32, 4), (2, 128, 2, 64, 4), (1, 145, 2, 64, 5), (1, 257, 2, 64, 4), (1, 320, 1, 32, 4),
               (1, 577, 2, 64, 5), (1, 577, 1, 32, 4), (1, 608, 1, 64, 4),
               (2, 197, 2, 128, 4), (1, 384, 1, 128, 5), (1, 33, 2, 128, 4), (2, 197, 3, 96, 4), (1, 544, 1, 96, 5),
               (2, 197, 2, 80, 4), (1, 577, 1, 80, 5), (2, 50, 2, 48, 4), (1, 608, 1, 48, 4)]


@pytest.mark.parametrize('B,N,H,hd,e_at', ATTN_SHAPES)
def test_lis_attention_rows(dva, oracle, B, N, H, hd, e_at):
    """the shapes of test_lis_attention: the first query_rows rows equal p2v_lis_attention's, nothing is written behind the last 16-row
    block that holds one of them."""
    E, S = dva.engine, dva.synth
    L = E.lib()
    D = H * hd
    qkv = torch.clamp(torch.round(S.normal(4, 'aq%d' % N, (B, N, 3 * D), 30.0)), -128, 127)
    qkv[0, 0, :D] = 127
    s_q1, s_at, s_a2 = 2.0 ** -4, 2.0 ** -e_at, 2.0 ** -3
    x0, bb, cc = oracle.lis_consts(torch.tensor([s_at]))
    at = E.Attn(s_q1 * s_q1, float(np.float32(hd ** -0.5)), 1.0 / s_at, s_q1 / s_a2, x0, bb, cc)
    dq = qkv.to(torch.int8).cuda()
    full = torch.zeros(B, N, D, dtype=torch.int8, device='cuda')
    E.check(L.p2v_lis_attention(E.ptr(dq), B, N, H, hd, C.byref(at), E.ptr(full), None, E.stream_ptr()))
    assert int(full.to(torch.int32).abs().max()) > 0
    for nq in sorted({min(q, N) for q in (1, 16, 17, N)}):
        out = torch.full((B, N, D), SENT, dtype=torch.int8, device='cuda')
        E.check(L.p2v_lis_attention_rows(E.ptr(dq), B, N, H, hd, C.byref(at), nq, E.ptr(out), E.stream_ptr()))
        torch.cuda.synchronize()
        assert torch.equal(out[:, :nq], full[:, :nq]), (nq, int((out[:, :nq] != full[:, :nq]).sum()))
        last = min(N, 16 * ((nq + 15) // 16))
        assert torch.equal(out[:, :last], full[:, :last]), nq                  # the rows that share a block are correct as well
        assert bool((out[:, last:] == SENT).all()), (nq, last)


def test_lis_attention_rows_refusals(dva, oracle):
    E = dva.engine
    L = E.lib()
    at = E.Attn(2.0 ** -8, 0.125, 16.0, 1.0, *oracle.lis_consts(torch.tensor([2.0 ** -4])))
    z = torch.zeros(4, 3 * 64, dtype=torch.int8, device='cuda')
    out = torch.zeros(4, 64, dtype=torch.int8, device='cuda')
    assert L.p2v_lis_attention_rows(E.ptr(z), 1, 4, 1, 64, C.byref(at), 1, E.ptr(out), E.stream_ptr()) == 0
    assert L.p2v_lis_attention_rows(E.ptr(z), 1, 4, 1, 64, C.byref(at), 0, E.ptr(out), E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_lis_attention_rows(E.ptr(z), 1, 4, 1, 64, C.byref(at), 5, E.ptr(out), E.stream_ptr()) == E.E_SHAPE
    assert L.p2v_lis_attention_rows(E.ptr(z), 1, 4, 1, 40, C.byref(at), 1, E.ptr(out), E.stream_ptr()) != 0
    assert L.p2v_lis_attention_rows(None, 1, 4, 1, 64, C.byref(at), 1, E.ptr(out), E.stream_ptr()) == E.E_ARG
    torch.cuda.synchronize()


def test_lis_attention_rows_custom_op(dva, oracle):
    E = dva.engine
    B, N, H, hd = 2, 197, 3, 64
    qkv = torch.clamp(torch.round(dva.synth.normal(4, 'aqop', (B, N, 3 * H * hd), 30.0)), -128, 127).to(torch.int8).cuda()
    x0, bb, cc = oracle.lis_consts(torch.tensor([2.0 ** -4]))
    args = (H, 2.0 ** -8, 0.125, 16.0, 1.0, x0, bb, cc)
    full = torch.ops.p2vit.lis_attention(qkv, *args)
    one = torch.ops.p2vit.lis_attention_rows(qkv, *args, 1)
    assert one.shape == (B, 1, H * hd) and torch.equal(one, full[:, :1])
