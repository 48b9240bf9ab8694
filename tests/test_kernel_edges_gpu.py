"""GPU: what the operator kernels write outside their result, and the values at which their arithmetic shortcuts are decided.

Footprint: every operand lives in a sentinel arena (tests/_arena.py: guards of >= 64 KB / 256 rows around it, padding between strided
rows, an offset of 80 bytes); after the launch the result equals the oracle's, every other byte of every arena is unchanged, and a second
launch into fresh arenas with another sentinel gives the same bytes (so poisoned input padding is not read into a result, a store of
the sentinel's own value cannot hide, and the launch repeats).

Values: exact rounding ties in every quotient of the GEMM epilogues, accumulators at the top of the oracle's 24-bit domain, LayerNorm
rows at the bounds of its integer sums, saturating attention scores and values, average-pool and fake-quant ties.  The tie shares are
asserted on the reference before the GPU is touched.  Every comparison is bit equality against the oracle's operations."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from _arena import SENTINELS, Arena, twice
from _tuning import tuning
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(gen, shape, std, lo=-128, hi=127):
    return torch.clamp(torch.round(torch.randn(shape, generator=gen) * std), lo, hi)


def _randint(gen, lo, hi, shape):
    """integers in [lo, hi] as floats"""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _q8(v):
    return torch.clamp(torch.round(v), -128, 127)


def _sync():
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------
# p2v_gemm_i8: one layer on the device, every epilogue, operands in arenas
# --------------------------------------------------------------------------------------------------
PATHS = {'tile128': dict(gemm_tile=128), 'tile256': dict(gemm_tile=256), 'rows': dict(gemm_rows=1)}


class Layer:
    """x [rows][width] and w [N][width] integer codes (floats), contraction length K = round_up(width, 64) through zero weight columns;
    colscale = s_x * s_w[n]; p: the epilogue's constants (host tensors / floats)"""

    def __init__(self, E, oracle, x, w, s_x, s_w, bias, w4, p):
        self.E, self.x, self.w, self.s_x, self.s_w, self.bias, self.w4, self.p = E, x, w, s_x, s_w, bias, w4, dict(p)
        self.N, self.width = w.shape
        self.K = (self.width + 63) // 64 * 64
        n_pad = (self.N + 127) // 128 * 128
        wp = torch.zeros(n_pad, self.K, dtype=torch.int8)
        wp[:self.N, :self.width] = w.to(torch.int8)
        pad = lambda v: torch.cat([v.float(), torch.zeros(n_pad - self.N)]).cuda()
        self.d = dict(w=(E.pack_int4_tiles(wp) if w4 else wp).cuda(), cs=pad(s_x * s_w), b=pad(bias))
        self.lin = E.Linear(E.ptr(self.d['w']), E.ptr(self.d['cs']), E.ptr(self.d['b']), None, 1 if w4 else 0)
        for k in ('s_mid', 's_res', 's_next', 'pos_deq'):
            if k in p:
                self.d[k] = p[k].contiguous().cuda()
        self.y = oracle.qgemm(x, torch.tensor(s_x), w, s_w, bias)          # [rows][N], every row: the launches take the first M
        self.tab = None

    def epilogue(self, kind, residual_ptr=None, tap_ptr=None):
        E, p = self.E, self.p
        epi = E.Epilogue()
        if tap_ptr is not None:
            epi.tap_out = tap_ptr
        if kind == 'requant':
            epi.inv_s_out = 2.0 ** p['e_req']
            return E.EPI_REQUANT, epi
        if kind in ('gelu', 'gelu_tab'):
            epi.inv_s_out = 2.0 ** p['e_gelu']
            if kind == 'gelu_tab':
                epi.gelu = E.gelu_table(2.0 ** p['e_gelu'], 'cuda')
                assert epi.gelu.table and epi.gelu.cells > 10
            return E.EPI_GELU, epi
        if kind == 'head':
            epi.inv_s_out, epi.s_out = 2.0 ** p['e_head'], 2.0 ** -p['e_head']
            return E.EPI_HEAD, epi
        if kind == 'embed':
            epi.inv_s_pe, epi.pe_to_embed, epi.s_embed = p['inv_s_pe'], p['pe_to_embed'], p['s_embed']
            epi.s_next, epi.pos_deq, epi.patches = E.ptr(self.d['s_next']), E.ptr(self.d['pos_deq']), p['patches']
            return E.EPI_EMBED, epi
        epi.s_mid, epi.s_res, epi.s_next = E.ptr(self.d['s_mid']), E.ptr(self.d['s_res']), E.ptr(self.d['s_next'])
        epi.residual = residual_ptr
        if kind == 'resid_pre':
            if self.tab is None:
                L = E.lib()
                nb = L.p2v_resid_prefold_bytes(self.N)
                self.tab = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
                usable = C.c_int(-1)
                E.check(L.p2v_resid_prefold(C.byref(self.lin), C.byref(epi), self.N, E.ptr(self.tab), nb, C.byref(usable), None))
                assert usable.value == 1, 'the pre-folded RESID table must be usable for these constants: the case is about that epilogue'
            epi.resid_tab = E.ptr(self.tab)
        return E.EPI_RESID, epi

    def reference(self, oracle, kind, M):
        """-> dict like run()'s"""
        p, y = self.p, self.y[:M]
        if kind == 'requant':
            return dict(out=_q8(y / 2.0 ** -p['e_req']))
        if kind in ('gelu', 'gelu_tab'):
            return dict(out=_q8(oracle.gelu_rn(y) / 2.0 ** -p['e_gelu']))
        if kind == 'head':
            q = _q8(y / 2.0 ** -p['e_head'])
            return dict(out=q * 2.0 ** -p['e_head'], codes=q)
        if kind == 'embed':
            P = p['patches']
            q1 = _q8(y * p['inv_s_pe'])
            q2 = _q8(q1 * p['pe_to_embed'])
            tok = torch.arange(M) % P + 1
            xv = q2 * p['s_embed'] + p['pos_deq'][tok]                     # q2 * s_embed is exact (a power of two): one rounding, the fma's
            return dict(out=_q8(xv / p['s_next']))
        q3 = _q8(y / p['s_mid'])
        return dict(out=_q8((p['res'][:M] * p['s_res'] + q3 * p['s_mid']) / p['s_next']))

    def run(self, kind, M, lda, ldo, sentinel, tap=False):
        """one launch with every operand in an arena of `sentinel` -> dict(out=[M][N] (EMBED: the patch rows), tap=, codes=) on the host"""
        E, N, K, p = self.E, self.N, self.K, self.p
        L = E.lib()
        assert lda >= self.width                                           # columns [width, K) of a row: padding or the next row, poisoned
        a = Arena(M, self.width, lda, torch.int8, sentinel, init=self.x[:M])
        rows_out = M if kind != 'embed' else (M // p['patches']) * (p['patches'] + 1)
        out = Arena(rows_out, N, ldo, torch.float32 if kind == 'head' else torch.int8, sentinel,
                    init=p['res'][:M] if kind.startswith('resid') else None)
        codes = Arena(M, N, ldo, torch.int8, sentinel) if kind == 'head' else None
        tp = Arena(M, N, N, torch.float32, sentinel) if tap else None
        k, epi = self.epilogue(kind, out.ptr, tp.ptr if tap else None)
        E.check(L.p2v_gemm_i8(k, a.ptr, lda, M, K, N, C.byref(self.lin), C.byref(epi), out.ptr, ldo, codes.ptr if codes else None, E.stream_ptr()))
        _sync()
        what = (kind, M, K, N, lda, ldo, self.w4)
        assert torch.equal(a.read(('A', what)).float(), self.x[:M])        # the input arena is untouched as a whole
        res = dict(out=out.read(('out', what)).float())
        if kind == 'embed':
            P = p['patches']
            full = res['out'].reshape(-1, P + 1, N)
            sv = float(np.int8(np.uint8(sentinel)))
            assert bool((full[:, 0] == sv).all()), ('EMBED wrote a class-token row', what)
            res['out'] = full[:, 1:].reshape(M, N).contiguous()
        if codes:
            res['codes'] = codes.read(('out_codes', what)).float()
        if tap:
            res['tap'] = tp.read(('tap_out', what))
        return res


def _check(got, ref, what):
    for k, r in ref.items():
        g = got[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        assert torch.equal(g, r.to(g.dtype)), (what, k, int((g != r).sum()), 'of', r.numel())


def _random_layer(E, oracle, gen, K, N, w4, rows, width=None):
    """the data of the existing operator tests: round(normal * std) codes, random biases, non-dyadic PTF scales"""
    width = K if width is None else width
    x = _codes(gen, (rows, width), 40.0)
    w = _codes(gen, (N, width), 3.5, -8, 7) if w4 else _codes(gen, (N, width), 30.0)
    s_w = 2.0 ** -(torch.randint(2, 6, (N,), generator=gen).float() + (0 if w4 else 4))
    ptf = lambda base: base * 2.0 ** torch.randint(0, 4, (N,), generator=gen).float()
    p = dict(e_req=3, e_gelu=5, e_head=2, s_mid=ptf(0.0131), s_res=ptf(0.0173), s_next=ptf(0.0209), res=_codes(gen, (rows, N), 50.0))
    return Layer(E, oracle, x, w, 2.0 ** -5, s_w, torch.randn(N, generator=gen) * 0.4, w4, p)


FOOT_KINDS = ('requant', 'gelu_tab', 'gelu', 'resid', 'resid_pre')
FOOT_MS = (1, 127, 129, 257)
FOOT_KN = ((64, 16), (128, 144), (192, 400))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('kind', FOOT_KINDS)
def test_gemm_footprint(dva, oracle, kind, w4):
    """tiled kernel, tile heights 128 and 256, M in {1, 127, 129, 257}, (K, N) in {(64, 16), (128, 144), (192, 400)}: the 24 combinations,
    each with ONE of ldo in {N, N + 16, 2N + 16} and ONE of lda in {K, K + 64}, in rotation: every (ldo, lda) pair occurs and every
    tile height, M and (K, N) meets every ldo and lda value, but shapes are not crossed with strides - an (M, K, N) sees two of the three
    ldo values.  RESID in place on the residual, as the forward runs it.  Result == oracle, nothing else written, two sentinels."""
    E = dva.engine
    L = E.lib()
    layers = {kn: _random_layer(E, oracle, _gen(500 + kn[0] + kn[1] + (7 if w4 else 0)), kn[0], kn[1], w4, max(FOOT_MS)) for kn in FOOT_KN}
    for i, (tile, M, (K, N)) in enumerate(itertools.product((128, 256), FOOT_MS, FOOT_KN)):
        lay = layers[(K, N)]
        ldo = (N, N + 16, 2 * N + 16)[(i + i // 3) % 3]
        lda = (K, K + 64)[(i + i // 6) % 2]
        with tuning(L, gemm_tile=tile):
            got = twice(lambda s: lay.run(kind, M, lda, ldo, s))
        _check(got, lay.reference(oracle, kind, M), (kind, w4, tile, M, K, N, lda, ldo))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
def test_gemm_contraction_walks_into_the_next_row(dva, oracle, w4):
    """K = 128 over rows of 96 bytes (lda = 96): k-values [96, 128) of a row are the first bytes of the next one - of the guard behind
    the last - and meet zero weight columns; with lda = 160 they are row padding.  The two runs poison both differently; every epilogue,
    tiled and few-rows kernel."""
    E = dva.engine
    lay = _random_layer(E, oracle, _gen(611), 128, 144, w4, 129, width=96)
    for kind in FOOT_KINDS:
        for path, lda in itertools.product(('tile128', 'tile256', 'rows'), (96, 160)):
            with tuning(E.lib(), **PATHS[path]):
                got = twice(lambda s: lay.run(kind, 129, lda, 160, s))
            _check(got, lay.reference(oracle, kind, 129), (kind, w4, path, lda))


@pytest.mark.parametrize('kind', ['requant', 'gelu_tab', 'gelu'])
def test_gemm_tap_out_footprint(dva, oracle, kind):
    """p2v_epilogue.tap_out: fp32 [M][N] in its own arena holds fmaf(acc, colscale, bias), the codes are unchanged by it"""
    E = dva.engine
    for (K, N), M, tile, w4 in (((64, 16), 1, 128, False), ((128, 144), 129, 256, False), ((192, 400), 257, 128, True), ((128, 144), 127, 256, True)):
        lay = _random_layer(E, oracle, _gen(640 + N), K, N, w4, M)
        with tuning(E.lib(), gemm_tile=tile):
            got = twice(lambda s: lay.run(kind, M, K, N + 16, s, tap=True))
        ref = lay.reference(oracle, kind, M)
        ref['tap'] = lay.y[:M]
        _check(got, ref, (kind, K, N, M, tile, w4))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
def test_gemm_head_footprint(dva, oracle, w4):
    """HEAD: N = 1000 (not a multiple of 16), ldo in {1000, 1008}: fp32 logits on the act_out grid and the int8 out_codes"""
    E = dva.engine
    for K, M, ldo in ((64, 1, 1000), (192, 129, 1008), (64, 129, 1000), (192, 1, 1008)):
        lay = _random_layer(E, oracle, _gen(700 + K + M), K, 1000, w4, M)
        got = twice(lambda s: lay.run('head', M, K + 64, ldo, s))
        _check(got, lay.reference(oracle, 'head', M), ('head', w4, K, M, ldo))


def _embed_case(gen, K, N, w4, batch, patches, ties=False):
    """operands and constants of an EMBED launch -> the arguments of Layer"""
    M = batch * patches
    if ties:                                                     # see test_gemm_exact_ties
        x, w, s_w, bias = _tie_operands(gen, M, K, N, w4, 2.0 ** -5, 2.0 ** -4)
        pos = _randint(gen, -40, 40, (patches + 1, N)) * 2.0 ** -4
        s_next = 2.0 ** -3 * 2.0 ** torch.randint(0, 3, (N,), generator=gen).float()
        # the clamp edges of the last quotient, q2 + pos / s_next at s_next = s_embed, in row 0 (no activations: q1 = bias / s_pe, token 1):
        # q1 = 127 -> q2 = rne(63.5) = 64, pos = 63.5 s_next -> 127.5;  q1 = -128 -> q2 = -64, pos = -64.5 s_next -> -128.5
        bias[2], bias[3] = 127.0 * 2.0 ** -4, -128.0 * 2.0 ** -4
        s_next[2:4] = 2.0 ** -3
        pos[1, 2], pos[1, 3] = 127.0 * 2.0 ** -4, -129.0 * 2.0 ** -4
    else:
        x, w = _codes(gen, (M, K), 40.0), (_codes(gen, (N, K), 3.5, -8, 7) if w4 else _codes(gen, (N, K), 30.0))
        s_w = torch.full((N,), 2.0 ** (-3 if w4 else -7))
        bias = torch.randn(N, generator=gen) * 0.4
        pos = _codes(gen, (patches + 1, N), 20.0) * 2.0 ** -3
        s_next = 0.05 * 2.0 ** torch.randint(0, 4, (N,), generator=gen).float()
    p = dict(inv_s_pe=2.0 ** 4, pe_to_embed=0.5, s_embed=2.0 ** -3, pos_deq=pos, s_next=s_next, patches=patches)
    return x, w, 2.0 ** -5, s_w, bias, w4, p


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('N', [64, 208])
def test_gemm_embed_epilogue(dva, oracle, N, w4):
    """EMBED at the operator level: batch 3, 16 patches, K = 192.  q1 = clamp(rne(y * inv_s_pe)), q2 = clamp(rne(q1 * pe_to_embed)),
    x = fma(q2, s_embed, pos_deq[tok][n]), q = clamp(rne(x / s_next[n])) with the IEEE division, at row b * 17 + 1 + p; the three
    class-token rows keep the sentinel."""
    E = dva.engine
    lay = Layer(E, oracle, *_embed_case(_gen(800 + N), 192, N, w4, 3, 16))
    ref = lay.reference(oracle, 'embed', 48)
    assert ref['out'].abs().max() == 128 and ref['out'].max() == 127 and len(torch.unique(ref['out'])) > 100
    for ldo in (N, N + 16):
        got = twice(lambda s: lay.run('embed', 48, 192, ldo, s))
        _check(got, ref, ('embed', N, w4, ldo))


def test_fill_cls_changes_exactly_the_class_rows(dva, micro):
    """k_fill_cls, the launch behind the EMBED GEMM of p2v_forward (stop_after = 3 against 2) on the micro model: of the whole
    sentinel-filled workspace exactly the class-token rows of "x" change, every image gets the same row, and the patch rows hold the
    reference's qact1 codes."""
    arch = micro['arch']
    plan = dva.FrozenPlan(arch, micro['sd'], micro['calib'])
    x = micro['x_ev'].cuda()
    B, D, T = x.shape[0], arch['embed_dim'], plan.tokens
    bits = [8] * (4 * arch['depth'] + 2)
    plan.forward(x, bits)                                       # allocates the workspace
    _sync()
    snaps = []
    for sent in SENTINELS:
        for stop in (2, 3):
            plan.workspace(B).fill_(sent)
            plan.forward(x, bits, stop_after=stop)
            _sync()
            snaps.append(plan.workspace(B).cpu().numpy().copy())
        before, after = snaps[-2], snaps[-1]
        off = dva.engine.lib().p2v_workspace_view(plan._handle, B, b'x')
        changed = np.nonzero(before != after)[0]
        assert changed.size > 0
        rel = changed - off
        assert rel.min() >= 0 and rel.max() < B * T * D and bool(((rel // D) % T == 0).all()), 'a byte outside the class rows changed'
        xb, xa = before[off: off + B * T * D].view(np.int8).reshape(B, T, D), after[off: off + B * T * D].view(np.int8).reshape(B, T, D)
        assert bool((xb[:, 0] == np.int8(np.uint8(sent))).all())                 # the EMBED epilogue left them alone
        assert bool((xa[:, 0] == xa[0, 0]).all())
        ref = micro['g']['taps/q8/qact1'].reshape(B, T, D)
        assert np.array_equal(xa.astype(np.int64), ref.astype(np.int64))
    assert np.array_equal(snaps[1][off: off + B * T * D], snaps[3][off: off + B * T * D])


# --------------------------------------------------------------------------------------------------
# LayerNorm, alone and fused into the GEMM
# --------------------------------------------------------------------------------------------------
class Norm:
    """constants of one LayerNorm over C channels on the device; chain 'pot': power-of-two output scale and a post multiplier,
    'div': output scale 1.3 x a power of two, divided by exactly (p2v_ln.out_scale)"""

    def __init__(self, E, gen, C_, chain='pot', mask=None):
        self.E, self.C, self.chain = E, C_, chain
        self.mask = (2.0 ** torch.randint(0, 4, (C_,), generator=gen).float()) if mask is None else mask
        if mask is None:
            self.mask[int(torch.randint(0, C_, (1,), generator=gen))] = 1.0
        self.s1 = 0.0123
        self.gamma = torch.rand(C_, generator=gen) * 3.0 - 1.5
        self.beta = torch.randn(C_, generator=gen) * 0.3
        cs = 2.0 ** torch.randint(-2, 3, (C_,), generator=gen).float()
        cs_next = 2.0 ** torch.randint(-2, 3, (C_,), generator=gen).float()
        self.s_a = 2.0 ** -4
        if chain == 'pot':
            self.out_scale = self.s_a * cs
            self.post = self.out_scale / cs_next / self.s_a
            self.cs_next = cs_next
        else:
            self.out_scale = self.s_a * cs * 1.3
            self.post = torch.ones(C_)
        dv = [t.contiguous().cuda() for t in (self.mask, self.gamma, self.beta, 1.0 / self.out_scale, self.post, self.out_scale)]
        self.dev = dv
        self.ln = E.Ln(float(np.float32(self.s1)), *[E.ptr(t) for t in (dv[:5] + ([dv[5]] if chain == 'div' else []))])
        self.pre_buf = None

    def prefold(self, on):
        E = self.E
        L = E.lib()
        if on and self.pre_buf is None:
            nb = L.p2v_ln_prefold_bytes(self.C)
            self.pre_buf = torch.empty(nb // 4, dtype=torch.float32, device='cuda')
            E.check(L.p2v_ln_prefold(C.byref(self.ln), self.C, E.ptr(self.pre_buf), nb))
            self.pre = E.LnPre.from_buffer_copy(self.ln.pre)
            assert self.ln.pre.gm
        self.ln.pre = self.pre if on else E.LnPre()

    def reference(self, oracle, codes):
        """-> (codes [rows][C] of the kernel's output, finite [rows]): the oracle's LayerNorm on x_q = code * mask (in_scale = s1
        everywhere and x = x_q * s1 give exactly that x_q and that s1)"""
        s1 = torch.tensor(np.float32(self.s1))
        xq = codes * self.mask.reshape(1, -1)
        ln = oracle.int_layernorm((xq * s1).unsqueeze(0), torch.full((self.C,), float(s1)), self.gamma, self.beta, self.out_scale)[0]
        finite = torch.isfinite(ln).all(dim=1)
        if self.chain == 'pot':
            q = _q8((ln * self.out_scale.reshape(1, -1)) / self.cs_next.reshape(1, -1) / self.s_a)
        else:
            q = torch.clamp(ln, -128, 127)
        return q, finite


def _run_layernorm(E, norm, codes, row_stride, out_stride, sentinel):
    rows, C_ = codes.shape
    a = Arena(rows, C_, row_stride, torch.int8, sentinel, init=codes)
    out = Arena(rows, C_, out_stride, torch.int8, sentinel)
    E.check(E.lib().p2v_int_layernorm(a.ptr, row_stride, rows, C_, C.byref(norm.ln), out.ptr, out_stride, E.stream_ptr()))
    _sync()
    what = ('layernorm', rows, C_, row_stride, out_stride)
    assert torch.equal(a.read(('x', what)).float(), codes)
    return dict(out=out.read(('out', what)).float())


@pytest.mark.parametrize('C_', [4, 100, 384, 1024, 2048])
def test_layernorm_footprint(dva, oracle, C_):
    """p2v_int_layernorm with row_stride in {C, C + 12, 5 C (the class-row pattern of the final norm)} and out_stride in {C, C + 20,
    round_up(C, 64)} in rotation over rows in {1, 9, 65} x ln_rows in {1, 64} x constants folded ahead or not"""
    E = dva.engine
    L = E.lib()
    gen = _gen(900 + C_)
    norm = Norm(E, gen, C_)
    codes = _codes(gen, (65, C_), 35.0)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    i = 0
    for rows, ln_rows, pre in itertools.product((1, 9, 65), (1, 64), (False, True)):
        rs = (C_, C_ + 12, 5 * C_)[i % 3]
        os_ = (C_, C_ + 20, (C_ + 63) // 64 * 64)[(i + i // 3) % 3]
        i += 1
        norm.prefold(pre)
        with tuning(L, ln_rows=ln_rows):
            got = twice(lambda s: _run_layernorm(E, norm, codes[:rows], rs, os_, s))
        _check(got, dict(out=ref[:rows]), ('layernorm', C_, rows, ln_rows, pre, rs, os_))
    norm.prefold(False)


def _ln_bound_rows(gen, C_):
    """rows at the bounds of ln_sums: codes from {-128, 127} only (four rows), all but one element equal (two), a single non-zero element
    (two), two constant rows (NaN in the reference: present, not compared) and two ordinary rows"""
    pm = lambda: torch.where(torch.rand(C_, generator=gen) < 0.5, torch.tensor(-128.0), torch.tensor(127.0))
    rows = [pm() for _ in range(4)]
    r = torch.full((C_,), -128.0); r[C_ // 3] = 127.0; rows.append(r)
    r = torch.full((C_,), 127.0); r[C_ - 1] = -128.0; rows.append(r)
    r = torch.zeros(C_); r[7] = 127.0; rows.append(r)
    r = torch.zeros(C_); r[C_ - 1] = -128.0; rows.append(r)
    rows += [torch.full((C_,), 127.0), torch.full((C_,), -128.0)]
    rows += [_codes(gen, (C_,), 35.0), _codes(gen, (C_,), 90.0)]
    return torch.stack(rows), [8, 9]


@pytest.mark.parametrize('chain', ['pot', 'div'])
@pytest.mark.parametrize('C_', [384, 1024, 2048])
def test_layernorm_at_its_bounds(dva, oracle, C_, chain):
    """|x_q| = 1016 / 1024 on every channel (PTF mask 8 everywhere: 16-value partial sums of squares reach 2^24, S2 comes within 1 % of
    2^31 at C = 2048 - 0.992 x 2^31 for the +-rows, 2^31 - 16 320 for the row with one 127 among -128s, 2^31 itself for the constant
    row of -128s) and masks mixing 1 and 8; both
    output chains, constants folded ahead and not."""
    E = dva.engine
    gen = _gen(950 + C_)
    codes, constant = _ln_bound_rows(gen, C_)
    for mk in ('all8', 'mix18'):
        mask = torch.full((C_,), 8.0) if mk == 'all8' else torch.where(torch.rand(C_, generator=gen) < 0.5, torch.tensor(1.0), torch.tensor(8.0))
        norm = Norm(E, gen, C_, chain, mask=mask)
        ref, finite = norm.reference(oracle, codes)
        # a constant row is NaN in the reference (zero variance): present, not compared; under the mixed mask no row is constant
        assert [i for i in range(len(codes)) if not bool(finite[i])] == (constant if mk == 'all8' else []), 'only constant rows may drop out'
        if mk == 'all8' and C_ == 2048:
            s2 = ((codes * 8.0).double() ** 2).sum(1)
            assert float(s2[:5].min()) > 0.99 * 2.0 ** 31 and float(s2[5]) > 0.98 * 2.0 ** 31 and float(s2.max()) == 2.0 ** 31
        for pre in (False, True):
            norm.prefold(pre)
            got = twice(lambda s: _run_layernorm(E, norm, codes, C_, C_, s))
            g, r = got['out'][finite], ref[finite]
            assert torch.equal(g, r), (C_, chain, mk, pre, int((g != r).sum()), [int(v) for v in (g != r).sum(1)])
        norm.prefold(False)


def _ln_gemm_layer(E, oracle, gen, norm, q0, N):
    """the GEMM behind a LayerNorm whose output codes are q0 [M][C]"""
    C_ = norm.C
    w = _codes(gen, (N, C_), 30.0)
    s_w = torch.full((N,), 2.0 ** -7); s_w[::3] = 2.0 ** -6
    lay = Layer(E, oracle, q0, w, norm.s_a, s_w, torch.randn(N, generator=gen) * 0.4, False, dict(e_req=3, e_gelu=5))
    n_pad, k_pad = (N + 127) // 128 * 128, (C_ + 63) // 64 * 64
    wp = torch.zeros(n_pad, k_pad, dtype=torch.int8); wp[:N, :C_] = w.to(torch.int8)
    lay.d['wf'] = E.fragment_order(wp).cuda()
    lay.lin.w_frag = E.ptr(lay.d['wf'])
    return lay


def _run_ln_gemm(E, norm, lay, kind, codes, row_stride, with_ln_out, sentinel):
    M, C_ = codes.shape
    N = lay.N
    a = Arena(M, C_, row_stride, torch.int8, sentinel, init=codes)
    out = Arena(M, N, N, torch.int8, sentinel)
    lno = Arena(M, C_, C_, torch.int8, sentinel) if with_ln_out else None
    k, epi = lay.epilogue(kind)
    E.check(E.lib().p2v_ln_gemm_i8(k, a.ptr, row_stride, M, C_, C.byref(norm.ln), N, C.byref(lay.lin), C.byref(epi), out.ptr, N,
                                  lno.ptr if lno else None, E.stream_ptr()))
    _sync()
    what = ('ln_gemm', kind, M, C_, N, row_stride, with_ln_out)
    assert torch.equal(a.read(('x', what)).float(), codes)
    res = dict(out=out.read(('out', what)).float())
    if lno:
        res['ln_out'] = lno.read(('ln_out', what)).float()
    return res


@pytest.mark.parametrize('C_,N,M', [(64, 192, 1), (96, 288, 129), (384, 1152, 65)])
def test_ln_gemm_footprint(dva, oracle, C_, N, M):
    """p2v_ln_gemm_i8, kernel versions 1 / 2 / 3, with and without ln_out, row_stride in {C, C + 32}: out [M][N] and ln_out [M][C]
    against the oracle's LayerNorm + qgemm (+ GELU), nothing else written"""
    E = dva.engine
    L = E.lib()
    gen = _gen(1000 + C_)
    norm = Norm(E, gen, C_)
    codes = _codes(gen, (M, C_), 35.0)
    q0, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    lay = _ln_gemm_layer(E, oracle, gen, norm, q0, N)
    for kind in ('requant', 'gelu_tab'):
        ref = lay.reference(oracle, kind, M)
        for ver, with_ln, rs in itertools.product((1, 2, 3), (False, True), (C_, C_ + 32)):
            with tuning(L, ln_gemm_version=ver):
                got = twice(lambda s: _run_ln_gemm(E, norm, lay, kind, codes, rs, with_ln, s))
            _check(got, dict(ref, ln_out=q0) if with_ln else ref, ('ln_gemm', kind, C_, N, M, ver, with_ln, rs))


@pytest.mark.parametrize('chain', ['pot', 'div'])
def test_ln_gemm_at_the_layernorm_bounds(dva, oracle, chain):
    """the bound rows of test_layernorm_at_its_bounds through the fused kernel at C = 384 (mask 8 everywhere), every kernel version"""
    E = dva.engine
    L = E.lib()
    gen = _gen(1100)
    C_, N = 384, 1152
    codes, constant = _ln_bound_rows(gen, C_)
    norm = Norm(E, gen, C_, chain, mask=torch.full((C_,), 8.0))
    q0, finite = norm.reference(oracle, codes)
    assert [i for i in range(len(codes)) if not bool(finite[i])] == constant
    lay = _ln_gemm_layer(E, oracle, gen, norm, torch.where(finite.reshape(-1, 1), q0, torch.zeros_like(q0)), N)
    ref = lay.reference(oracle, 'requant', len(codes))
    for ver, pre in itertools.product((1, 2, 3), (False, True)):
        norm.prefold(pre)
        with tuning(L, ln_gemm_version=ver):
            got = twice(lambda s: _run_ln_gemm(E, norm, lay, 'requant', codes, C_, True, s))
        for k, r in (('ln_out', q0), ('out', ref['out'])):
            assert torch.equal(got[k][finite], r[finite]), (chain, ver, pre, k, int((got[k][finite] != r[finite]).sum()))
    norm.prefold(False)


# --------------------------------------------------------------------------------------------------
# ViT attention
# --------------------------------------------------------------------------------------------------
def _attn_reference(oracle, qkv, H, hd, s_q1, s_at, s_a2):
    B, N = qkv.shape[:2]
    D = H * hd
    t = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    acc = t[0] @ t[1].transpose(-2, -1)
    scale = float(np.float32(hd ** -0.5))
    sc = _q8(((acc * (s_q1 * s_q1)) * scale) / s_at)
    k = oracle.lis_int(sc, torch.tensor([s_at]))
    o = (oracle.lis_probs(k) @ (t[2] * s_q1)).transpose(1, 2).reshape(B, N, D)
    return sc, k, _q8(o / s_a2)


def _run_attention(E, oracle, qkv, H, hd, s_q1, s_at, s_a2, sentinel):
    B, N = qkv.shape[:2]
    D = H * hd
    x0, bb, cc = oracle.lis_consts(torch.tensor([s_at]))
    at = E.Attn(s_q1 * s_q1, float(np.float32(hd ** -0.5)), 1.0 / s_at, s_q1 / s_a2, x0, bb, cc)
    a = Arena(B * N, 3 * D, 3 * D, torch.int8, sentinel, init=qkv.reshape(B * N, 3 * D))
    out = Arena(B * N, D, D, torch.int8, sentinel)
    pk = Arena(B * H * N, N, N, torch.int8, sentinel)
    E.check(E.lib().p2v_lis_attention(a.ptr, B, N, H, hd, C.byref(at), out.ptr, pk.ptr, E.stream_ptr()))
    _sync()
    what = ('attention', B, N, H, hd)
    a.read(('qkv', what))
    return dict(out=out.read(('out', what)).float().reshape(B, N, D), probs_k=pk.read(('probs_k', what)).long().reshape(B, H, N, N))


@pytest.mark.parametrize('B,N,H,hd,stream', [(2, 1, 1, 32, 0), (2, 17, 2, 64, 0), (1, 197, 3, 64, 0), (1, 33, 1, 128, 0),
                                            (2, 1, 1, 32, 1), (2, 17, 2, 64, 1), (1, 197, 3, 64, 1), (1, 33, 1, 128, 1), (1, 609, 1, 64, 0)])
def test_lis_attention_footprint(dva, oracle, B, N, H, hd, stream):
    """resident kernel, streaming kernel through the switch, and the streaming kernel at 609 tokens where it runs on its own: out
    [B N][D] and probs_k [B][H][N][N] each in an arena"""
    E = dva.engine
    assert stream or (N > E.lib().p2v_resident_tokens(hd)) == (N == 609)
    qkv = _codes(_gen(1200 + N), (B, N, 3 * H * hd), 30.0)
    qkv[0, 0, :H * hd] = 127
    s_q1, s_at, s_a2 = 2.0 ** -4, 2.0 ** -4, 2.0 ** -3
    _, k, ref = _attn_reference(oracle, qkv, H, hd, s_q1, s_at, s_a2)
    with tuning(E.lib(), attn_stream=stream):
        got = twice(lambda s: _run_attention(E, oracle, qkv, H, hd, s_q1, s_at, s_a2, s))
    _check(got, dict(probs_k=k, out=ref), ('attention', B, N, H, hd, stream))


def _attn_heads(gen, N, hd, kind):
    """q and k of one head from {-128, 127}.  'onehot': key 5 is all 127, every other key -128 with a few elements (up to an eighth) flipped to 127;
    queries cycle through all 127 (key 5 scores 127 and every other key -128: one key carries the whole probability, the rest get
    exponent 16 - both ends of the score range in one row), all -128 (the mirror image), alternating and random +-.  'equal': every key
    is all 127, so every score row is constant, at 127, -128 or in between."""
    pm = lambda *shape: torch.where(torch.rand(*shape, generator=gen) < 0.5, torch.tensor(-128.0), torch.tensor(127.0))
    q = pm(N, hd)
    q[0::4] = 127.0
    q[1::4] = -128.0
    q[2::4, 0::2], q[2::4, 1::2] = 127.0, -128.0
    if kind == 'equal':
        return q, torch.full((N, hd), 127.0)
    k = torch.full((N, hd), -128.0)
    flips = torch.rand(N, hd, generator=gen) < torch.rand(N, 1, generator=gen) * 0.125
    k[flips] = 127.0
    k[5 % N] = 127.0
    return q, k


@pytest.mark.parametrize('v_kind', ['neg', 'alt'])
@pytest.mark.parametrize('B,N,H,hd', [(1, 197, 2, 64), (1, 609, 1, 64)])
def test_lis_attention_saturating_values(dva, oracle, B, N, H, hd, v_kind):
    """q, k from {-128, 127}: one-hot rows, rows saturating at both ends of the score range, all-equal rows (a head of its own; at one
    head: a launch of its own).  v = -128 everywhere with av_mul = 1 (the output is -128 times the sum of the probabilities: on the clamp
    bound and beyond it) / alternating 127, -128 over tokens and channels with av_mul = 2: the output requantisation saturates at both ends.
    The reference alone gives (asserted before the launch): 51 of 197 / 153 of 609 rows with a single exponent below 16, every row of
    the one-hot head with scores at 127 and at -128, every row of the other head constant (at 127, at -128 and between).  probs_k and out against the oracle."""
    E = dva.engine
    gen = _gen(1300 + N)
    D = H * hd
    s_q1, s_at, s_a2 = 2.0 ** -4, 2.0 ** -4, (2.0 ** -4 if v_kind == 'neg' else 2.0 ** -5)
    for kinds in ((('onehot', 'equal'),) if H == 2 else (('onehot',), ('equal',))):
        qkv = torch.zeros(B, N, 3, H, hd)
        for h, kind in enumerate(kinds):
            q, k = _attn_heads(gen, N, hd, kind)
            qkv[0, :, 0, h], qkv[0, :, 1, h] = q, k
        if v_kind == 'neg':
            qkv[:, :, 2] = -128.0
        else:
            par = (torch.arange(N).reshape(N, 1, 1) + torch.arange(hd).reshape(1, 1, hd)) % 2
            qkv[0, :, 2] = torch.where(par == 0, torch.tensor(127.0), torch.tensor(-128.0)).expand(N, H, hd)
        qkv = qkv.reshape(B, N, 3 * D)
        sc, k, ref = _attn_reference(oracle, qkv, H, hd, s_q1, s_at, s_a2)
        # the reference alone, before the GPU: the patterns are there
        if 'onehot' in kinds:
            one = ((k[0, 0] < 16).sum(-1) == 1)
            assert int(one.sum()) >= N // 8, int(one.sum())                                  # one key carries the whole probability
            both = (sc[0, 0].max(-1)[0] == 127) & (sc[0, 0].min(-1)[0] == -128)
            assert int(both.sum()) >= N // 4, int(both.sum())                                # both ends of the score range in a row
        if 'equal' in kinds:
            hq = kinds.index('equal')
            assert bool((sc[0, hq].max(-1)[0] == sc[0, hq].min(-1)[0]).all())
            assert bool((sc[0, hq, :, 0] == 127).any()) and bool((sc[0, hq, :, 0] == -128).any())
        assert (ref.min() == -128 and (v_kind == 'neg' or ref.max() == 127)) or kinds == ('equal',)
        got = twice(lambda s: _run_attention(E, oracle, qkv, H, hd, s_q1, s_at, s_a2, s))
        _check(got, dict(probs_k=k, out=ref), ('attention values', N, H, kinds, v_kind))


# --------------------------------------------------------------------------------------------------
# Swin: window attention, patch merge, average pool
# --------------------------------------------------------------------------------------------------
def _window_reference(oracle, qkv, heads, Hf, ws, shift, c, tab):
    import swin_oracle as SO
    B, T = qkv.shape[:2]
    C_, N = heads * 32, ws * ws
    idx = SO.window_index(Hf, Hf, ws, shift)
    nW = idx.shape[0]
    region = mask = None
    if shift:
        mask = SO.shifted_window_mask(Hf, Hf, ws, shift)
        img = torch.zeros(Hf, Hf)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[hs, wsl] = cnt
                cnt += 1
        region = img.reshape(Hf // ws, ws, Hf // ws, ws).permute(0, 2, 1, 3).reshape(nW, N).long()
    xw = qkv[:, idx.reshape(-1)].reshape(B * nW, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
    s1 = torch.tensor(c['qact1'])
    qs = (xw[0] * s1) * torch.tensor(32 ** -0.5, dtype=torch.float32)
    attn = (qs.double() @ (xw[1] * s1).double().transpose(-2, -1)).float()
    a1 = SO.q8(attn, c['qact_attn1'])
    bias = (tab * c['qact_table'])[SO.relative_position_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    xi = SO.q8(a1 * c['qact_attn1'] + bias.unsqueeze(0), c['qact2'])
    if mask is not None:
        xi = (xi.reshape(B, nW, heads, N, N) + torch.round(mask / c['qact2']).unsqueeze(1).unsqueeze(0)).reshape(B * nW, heads, N, N)
    k = oracle.lis_int(xi, torch.tensor([c['qact2']]))
    o = (oracle.lis_probs(k) @ (xw[2] * s1)).transpose(1, 2).reshape(B, nW * N, C_)
    want = torch.zeros(B, T, C_)
    want[:, idx.reshape(-1)] = SO.q8(o, c['qact3'])
    return idx, region, k.long().reshape(B, nW, heads, N, N), want


@pytest.mark.parametrize('Hf,ws,shift', [(14, 7, 0), (14, 7, 3), (8, 4, 0), (8, 4, 2)])
def test_window_attention_footprint(dva, oracle, Hf, ws, shift):
    """p2v_window_attention, three heads (96 channels): qkv_stride / out_stride dense and padded (288 -> 320, 96 -> 128).  The kernel
    writes the heads * 32 codes of a row and never the padding behind them (include/p2vit.h)."""
    E = dva.engine
    heads, B = 3, 2
    C_, T, N = heads * 32, Hf * Hf, ws * ws
    gen = _gen(1400 + Hf + shift)
    qkv = _codes(gen, (B, T, 3 * C_), 25.0)
    qkv[0, 0] = 127
    tab = _codes(gen, ((2 * ws - 1) ** 2, heads), 30.0)
    c = dict(qact1=2.0 ** -4, qact_attn1=2.0 ** -3, qact_table=2.0 ** -5, qact2=2.0 ** -4, qact3=2.0 ** -3)
    idx, region, k, want = _window_reference(oracle, qkv, heads, Hf, ws, shift, c, tab)
    nW = idx.shape[0]
    lis = oracle.lis_consts(torch.tensor([c['qact2']]))
    dev = dict(tab=tab.to(torch.int8).cuda(), idx=idx.to(torch.int32).contiguous().cuda(),
               reg=None if region is None else region.to(torch.int8).contiguous().cuda())

    def run(sentinel, ldq, ldo):
        wa = E.WinAttn(c['qact1'], float(np.float32(32 ** -0.5)), c['qact_attn1'], c['qact_table'], c['qact2'], c['qact3'], lis[0], lis[1], lis[2],
                       E.ptr(dev['tab']), E.ptr(dev['idx']), E.ptr(dev['reg']) if dev['reg'] is not None else None, ws, nW,
                       0 if ldq == 3 * C_ else ldq, 0 if ldo == C_ else ldo)
        a = Arena(B * T, 3 * C_, ldq, torch.int8, sentinel, init=qkv.reshape(B * T, 3 * C_))
        out = Arena(B * T, C_, ldo, torch.int8, sentinel)
        pk = Arena(B * nW * heads * N, N, N, torch.int8, sentinel)
        E.check(E.lib().p2v_window_attention(a.ptr, B, T, heads, 32, C.byref(wa), out.ptr, pk.ptr, E.stream_ptr()))
        _sync()
        what = ('window attention', Hf, ws, shift, ldq, ldo)
        a.read(('qkv', what))
        return dict(out=out.read(('out', what)).float().reshape(B, T, C_), probs_k=pk.read(('probs_k', what)).long().reshape(k.shape))

    for ldq, ldo in ((3 * C_, C_), (320, 128), (3 * C_, 128), (320, C_)):
        got = twice(lambda s: run(s, ldq, ldo))
        _check(got, dict(probs_k=k, out=want), ('window attention', Hf, ws, shift, ldq, ldo))
    assert (k < 16).any() and (k == 16).any()


@pytest.mark.parametrize('H,W,C_', [(2, 2, 16), (14, 6, 96)])
def test_patch_merge_footprint(dva, H, W, C_):
    E = dva.engine
    B = 3
    x = _codes(_gen(1500 + C_), (B, H, W, C_), 50.0)
    ref = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(B * (H // 2) * (W // 2), 4 * C_)

    def run(sentinel):
        a = Arena(B * H * W, C_, C_, torch.int8, sentinel, init=x.reshape(-1, C_))
        out = Arena(ref.shape[0], 4 * C_, 4 * C_, torch.int8, sentinel)
        E.check(E.lib().p2v_patch_merge_gather(a.ptr, B, H, W, C_, out.ptr, E.stream_ptr()))
        _sync()
        a.read('merge x')
        return dict(out=out.read(('merge', H, W, C_)).float())
    _check(twice(run), dict(out=ref), ('merge', H, W, C_))


@pytest.mark.parametrize('T', [1, 49, 50, 64, 8192])
def test_avgpool_values_and_footprint(dva, T):
    """p2v_avgpool_quant: out[b][c] = clamp(rne(((sum * s_in) / T) * inv_s_out)).  Images of all 127 and all -128 (the clamp bounds, and
    beyond them at twice the scale), of codes v and v + 1 in equal parts (at T = 64, and any even T, the mean is v + 1/2: an exact tie in
    every channel, both rounding directions and signs) and a random one; C = 20."""
    E = dva.engine
    gen = _gen(1600 + T)
    C_, B = 20, 4
    x = torch.zeros(B, T, C_)
    x[0], x[1] = 127.0, -128.0
    v = torch.arange(C_).float() * 3 - 30
    x[2] = v.reshape(1, C_) + (torch.arange(T) % 2).reshape(T, 1).float()
    x[3] = _codes(gen, (T, C_), 60.0)
    s_in = 2.0 ** -4
    for inv_s_out in (2.0 ** 4, 2.0 ** 5):
        t = ((x.sum(1) * s_in) / float(T)) * inv_s_out
        ref = _q8(t)
        if T == 64 and inv_s_out == 16.0:
            tie = t[2] - torch.floor(t[2]) == 0.5
            assert int(tie.sum()) == C_ and int((torch.round(t[2]) > t[2]).sum()) >= 5 and int((torch.round(t[2]) < t[2]).sum()) >= 5
            assert bool((t[2] < 0).any()) and bool((t[2] > 0).any())

        def run(sentinel):
            a = Arena(B * T, C_, C_, torch.int8, sentinel, init=x.reshape(-1, C_))
            out = Arena(B, C_, C_, torch.int8, sentinel)
            E.check(E.lib().p2v_avgpool_quant(a.ptr, B, T, C_, s_in, inv_s_out, out.ptr, E.stream_ptr()))
            _sync()
            a.read('avgpool x')
            return dict(out=out.read(('avgpool', T)).float())
        _check(twice(run), dict(out=ref), ('avgpool', T, inv_s_out))
        assert ref[0].max() == 127 and ref[1].min() == -128


# --------------------------------------------------------------------------------------------------
# patchify, fake-quant, GELU quant
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k_pad', [52, 64, 128])
def test_quantize_patchify_padding_columns_are_zero(dva, k_pad):
    """k_pad > C P^2: the columns [C P^2, k_pad) of every row are written, with zeros (include/p2vit.h); the guards are not"""
    E = dva.engine
    B, C_, S, P = 3, 3, 12, 4
    x = dva.synth.images(5, B, S) * 3
    q = _q8(x * 16.0)
    ref = torch.zeros(B * 9, k_pad)
    ref[:, :C_ * P * P] = torch.nn.functional.unfold(q, P, stride=P).transpose(1, 2).reshape(-1, C_ * P * P)

    def run(sentinel):
        a = Arena(1, x.numel(), None, torch.float32, sentinel, init=x.reshape(1, -1))
        out = Arena(B * 9, k_pad, k_pad, torch.int8, sentinel)
        E.check(E.lib().p2v_quantize_patchify(a.ptr, B, C_, S, S, P, 16.0, out.ptr, k_pad, E.stream_ptr()))
        _sync()
        a.read('images')
        return dict(out=out.read(('patchify', k_pad)).float())
    _check(twice(run), dict(out=ref), ('patchify', k_pad))
    assert ref.abs().max() >= 127


@pytest.mark.parametrize('layout', ['NHWC', 'NCHW'])
@pytest.mark.parametrize('P,S,C_', [(32, 352, 3), (16, 256, 8)])
def test_u8_patchify_segmented_band(dva, P, S, C_, layout):
    """a band too wide for the LDS budget of 32 KB - C * 256 is cut into segments: 11 patches of 3072 bytes as 10 + 1, 16 patches of 2048
    bytes (8 channels) as 15 + 1 - nseg = 2 with a short last segment; against p2v_quantize_patchify on the normalised images"""
    from diff_vit_amd import data as D
    E = dva.engine
    L = E.lib()
    gw, patch_bytes = S // P, P * P * C_
    Q = (32768 - C_ * 256) // patch_bytes
    assert 1 <= Q < gw and gw % Q != 0                                        # more than one segment, the last one short
    B = 2
    mean = [0.485, 0.456, 0.406, 0.5, 0.45, 0.4, 0.52, 0.47][:C_]
    std = [0.229, 0.224, 0.225, 0.25, 0.2, 0.23, 0.21, 0.24][:C_]
    u8 = dva.synth.images_uint8(P + S + C_, B, S, C_)
    lut = D.uint8_lut(mean, std)
    x32 = D.normalize_uint8(u8, mean, std).cuda()
    rows = B * gw * gw
    for inv_s, k_pad in ((32.0, (patch_bytes + 63) // 64 * 64), (64.0, patch_bytes + 4)):
        ref = torch.full((rows, k_pad), 77, dtype=torch.int8, device='cuda')
        E.check(L.p2v_quantize_patchify(E.ptr(x32), B, C_, S, S, P, inv_s, E.ptr(ref), k_pad, E.stream_ptr()))
        li8 = D.uint8_lut_i8(lut, inv_s).cuda()
        img = u8 if layout == 'NHWC' else u8.permute(0, 3, 1, 2).contiguous()

        def run(sentinel):
            a = Arena(1, img.numel(), None, torch.uint8, sentinel, init=img.reshape(1, -1))
            out = Arena(rows, k_pad, k_pad, torch.int8, sentinel)
            E.check(L.p2v_u8_patchify(a.ptr, E.LAYOUTS[layout], E.ptr(li8), B, C_, S, S, P, out.ptr, k_pad, E.stream_ptr()))
            _sync()
            a.read('u8 images')
            return dict(out=out.read(('u8 patchify', P, S, C_, k_pad)))
        _check(twice(run), dict(out=ref.cpu()), ('u8 patchify', P, S, C_, layout, k_pad))
    assert int(ref.min()) == -128 or int(ref.max()) == 127


def _run_fake_quant(E, x, scale, n_scale, inner, lo, hi, sentinel, want=('out', 'codes')):
    n = x.numel()
    a = Arena(1, n, None, torch.float32, sentinel, init=x.reshape(1, -1))
    out = Arena(1, n, None, torch.float32, sentinel) if 'out' in want else None
    cd = Arena(1, n, None, torch.int8, sentinel) if 'codes' in want else None
    sc = scale.cuda()
    E.check(E.lib().p2v_fake_quant_f32(a.ptr, n, E.ptr(sc), n_scale, inner, lo, hi, out.ptr if out else None, cd.ptr if cd else None, E.stream_ptr()))
    _sync()
    a.read('fake-quant x')
    res = {}
    if out:
        res['out'] = out.read(('fake-quant out', n)).reshape(-1)
    if cd:
        res['codes'] = cd.read(('fake-quant codes', n)).float().reshape(-1)
    return res


def _fake_quant_ref(x, scale, n_scale, inner, lo, hi):
    s = scale[(torch.arange(x.numel()) // inner) % n_scale]
    q = torch.clamp(torch.round(x / s), lo, hi)
    return dict(out=q * s, codes=q)


@pytest.mark.parametrize('n', [1, 255, 4096 * 256 + 3])
def test_fake_quant_footprint(dva, n):
    """both outputs; n = 4096 * 256 + 3 is past the 4096 x 256 threads of the largest grid: the grid-stride loop runs a second time
    for three elements; per-channel scales with inner > 1; either output alone"""
    E = dva.engine
    gen = _gen(1700)
    x = torch.randn(n, generator=gen) * 9.0
    for n_scale, inner in ((1, 1), (5, 7)):
        scale = 2.0 ** torch.randint(-6, -2, (n_scale,), generator=gen).float() * (1.0 if n_scale == 1 else 1.1)
        ref = _fake_quant_ref(x, scale, n_scale, inner, -128, 127)
        _check(twice(lambda s: _run_fake_quant(E, x, scale, n_scale, inner, -128, 127, s)), ref, ('fake-quant', n, n_scale, inner))
    for want in (('out',), ('codes',)):
        got = twice(lambda s: _run_fake_quant(E, x, scale, n_scale, inner, -128, 127, s, want))
        _check(got, {k: ref[k] for k in want}, ('fake-quant', n, want))


@pytest.mark.parametrize('bt', ['int8', 'int4', 'uint4'])
def test_fake_quant_ties_zeros_and_extremes(dva, oracle, bt):
    """inputs at exactly (k + 1/2) s for every k around the range (power-of-two s: x / s is the tie itself; s = 0.3: whatever the IEEE
    division makes of it), +-0.0, denormals, +-1e30"""
    E = dva.engine
    lo, hi = oracle.BITS[bt]
    k = torch.arange(lo - 3, hi + 3).float() + 0.5
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-45, 1e30, -1e30, 1e-38, 3.4e38])
    for s in (2.0 ** -3, 0.3):
        x = torch.cat([k * np.float32(s), special, -k * np.float32(s)])
        scale = torch.tensor([s], dtype=torch.float32)
        ref = _fake_quant_ref(x, scale, 1, 1, lo, hi)
        if s == 2.0 ** -3:
            t = x[:len(k)] / scale
            assert bool((t - torch.floor(t) == 0.5).all()) and ref['codes'].min() == lo and ref['codes'].max() == hi
        assert torch.equal(ref['out'], oracle.fake_quant(x, scale, lo, hi))
        _check(twice(lambda sn: _run_fake_quant(E, x, scale, 1, 1, lo, hi, sn)), ref, ('fake-quant values', bt, s))


def test_gelu_quant_footprint(dva, oracle):
    E = dva.engine
    gen = _gen(1800)
    y = torch.cat([torch.randn(1001, generator=gen) * 2.5, torch.tensor([0.0, -0.0, -0.7518, 30.0, -30.0, 1e30, -1e30])])
    n = y.numel()
    for inv_s, force in ((8.0, 0), (32.0, 0), (32.0, 1)):
        def run(sentinel):
            a = Arena(1, n, None, torch.float32, sentinel, init=y.reshape(1, -1))
            cd = Arena(1, n, None, torch.int8, sentinel)
            E.check(E.lib().p2v_gelu_quant_f32(a.ptr, n, inv_s, cd.ptr, None, force, E.stream_ptr()))
            _sync()
            a.read('gelu y')
            return dict(codes=cd.read(('gelu codes', inv_s)).float().reshape(-1))
        _check(twice(run), dict(codes=_q8(oracle.gelu_rn(y) * inv_s)), ('gelu quant', inv_s, force))


# --------------------------------------------------------------------------------------------------
# p2v_run_ops: three launches into neighbouring regions of one arena
# --------------------------------------------------------------------------------------------------
def test_run_ops_chain_in_one_arena(dva, oracle):
    """LayerNorm -> REQUANT GEMM -> average pool as ONE recorded list, their outputs side by side in one arena (offsets 0, 1024, 1792
    of 1888 bytes): each launch's neighbours are the guard of the others, the whole region is compared"""
    E = dva.engine
    gen = _gen(1900)
    B, T, C_, N = 2, 8, 64, 48
    M = B * T
    norm = Norm(E, gen, C_)
    codes = _codes(gen, (M, C_), 35.0)
    q0, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    w = _codes(gen, (N, C_), 30.0)
    lay = Layer(E, oracle, q0, w, norm.s_a, torch.full((N,), 2.0 ** -7), torch.randn(N, generator=gen) * 0.4, False, dict(e_req=3))
    q1 = lay.reference(oracle, 'requant', M)['out']
    s_in, inv_s_out = 2.0 ** -3, 2.0 ** 4
    q2 = _q8(((q1.reshape(B, T, N).sum(1) * s_in) / float(T)) * inv_s_out)
    want = torch.cat([q0.reshape(-1), q1.reshape(-1), q2.reshape(-1)])
    o1, o2, total = M * C_, M * C_ + M * N, M * C_ + M * N + B * N
    assert o1 % 16 == 0 and o2 % 16 == 0

    def run(sentinel):
        a = Arena(M, C_, C_, torch.int8, sentinel, init=codes)
        ar = Arena(1, total, None, torch.int8, sentinel)
        base = ar.dev.data_ptr() + ar.start
        ops = (E.Op * 3)()
        ops[0].kind, ops[0].inp, ops[0].out = E.OP_LAYERNORM, a.ptr, C.c_void_p(base)
        ops[0].M, ops[0].N, ops[0].lda, ops[0].ldo, ops[0].ln = M, C_, C_, C_, norm.ln
        k, epi = lay.epilogue('requant')
        ops[1].kind, ops[1].epi, ops[1].inp, ops[1].out = E.OP_GEMM, k, C.c_void_p(base), C.c_void_p(base + o1)
        ops[1].M, ops[1].K, ops[1].N, ops[1].lda, ops[1].ldo, ops[1].lin, ops[1].ep = M, C_, N, C_, N, lay.lin, epi
        ops[2].kind, ops[2].inp, ops[2].out = E.OP_AVGPOOL, C.c_void_p(base + o1), C.c_void_p(base + o2)
        ops[2].i0, ops[2].i1, ops[2].i2, ops[2].f0, ops[2].f1 = B, T, N, s_in, inv_s_out
        E.check(E.lib().p2v_run_ops(ops, 3, E.stream_ptr()))
        _sync()
        a.read('run_ops x')
        return dict(all=ar.read('run_ops arena').float().reshape(-1))
    _check(twice(run), dict(all=want), 'run_ops chain')


# --------------------------------------------------------------------------------------------------
# GEMM values: exact ties, accumulators at 2^24
# --------------------------------------------------------------------------------------------------
def _tie_operands(gen, M, K, N, w4, s_x, s_q):
    """The recipe: codes uniform in [-6, 6], every fifth activation row uniform in the full range, half of the int8 weight rows times
    12 (4-bit weights stay in [-6, 6]), colscale / s_q = 1/2 and the bias an integer multiple of s_q / 2 - so (acc * colscale + bias) / s_q
    is a multiple of 1/2 and about half of the outputs are exact ties.  Row 0 of the activations is zero and the biases of columns 0
    and 1 are 127.5 s_q and -128.5 s_q: one output on each clamp edge whatever the seed gives.  s_q: float or per-channel tensor."""
    x = _randint(gen, -6, 6, (M, K))
    x[4::5] = _randint(gen, -128, 127, (len(x[4::5]), K))
    x[0] = 0.0
    w = _randint(gen, -6, 6, (N, K))
    if not w4:
        w[N // 2:] *= 12.0
    s_q = torch.as_tensor(s_q, dtype=torch.float32).expand(N).clone()
    s_w = s_q / 2.0 / s_x
    hb = _randint(gen, -9, 9, (N,))
    hb[0], hb[1] = 255.0, -257.0
    return x, w, s_w, hb * s_q / 2.0


def _tie_stats(t):
    """t: the exact quotients (fp64)"""
    inr = (t > -128.5) & (t < 127.5)
    tie = ((t - torch.floor(t)) == 0.5) & inr
    r = torch.round(t)
    return dict(in_range=int(inr.sum()), ties=int(tie.sum()), up=int((tie & (r > t)).sum()), down=int((tie & (r < t)).sum()),
                pos=int((tie & (t > 0)).sum()), neg=int((tie & (t < 0)).sum()), hi_edge=int((t == 127.5).sum()), lo_edge=int((t == -128.5).sum()))


TIE_M, TIE_K, TIE_N = 129, 64, 144


def _tie_case(oracle, kind, w4):
    """-> (arguments of Layer, {name of a quotient: its statistics}); needs no GPU"""
    gen = _gen(2000 + (1 if w4 else 0))
    if kind == 'embed':
        args = _embed_case(gen, TIE_K, TIE_N, w4, 3, 43, ties=True)
        x, w, s_x, s_w, bias, _, p = args
        y = oracle.qgemm(x, torch.tensor(s_x), w, s_w, bias)
        t1 = y.double() * p['inv_s_pe']
        q1 = _q8(t1.float())
        t2 = q1.double() * p['pe_to_embed']
        q2 = _q8(t2.float())
        tok = torch.arange(TIE_M) % 43 + 1
        t3 = (q2 * p['s_embed'] + p['pos_deq'][tok]).double() / p['s_next'].double()
        return args, dict(q1=_tie_stats(t1), q2=_tie_stats(t2), q=_tie_stats(t3))
    if kind.startswith('resid'):
        s_mid = 2.0 ** -3 * 2.0 ** torch.randint(0, 4, (TIE_N,), generator=gen).float()          # dyadic PTF base: both quotients tie
        s_next = 2.0 ** -3 * 2.0 ** torch.randint(0, 4, (TIE_N,), generator=gen).float()
        s_next[2:4] = s_mid[2:4]
        x, w, s_w, bias = _tie_operands(gen, TIE_M, TIE_K, TIE_N, w4, 2.0 ** -5, s_mid)
        res = _randint(gen, -128, 127, (TIE_M, TIE_N))
        # the clamp edges of the second quotient, res / 2 + q3 (row 0 has no activations: q3 = bias / s_mid): 63.5 + 64 and -63.5 - 65
        res[0, 2], res[0, 3] = 127.0, -127.0
        bias[2], bias[3] = 64.0 * s_mid[2], -65.0 * s_mid[3]
        p = dict(s_mid=s_mid, s_res=s_next / 2.0, s_next=s_next, res=res)
        y = oracle.qgemm(x, torch.tensor(2.0 ** -5), w, s_w, bias)
        t1 = y.double() / s_mid.double()
        q3 = _q8(t1.float())
        t2 = (res * p['s_res'] + q3 * s_mid).double() / s_next.double()
        return (x, w, 2.0 ** -5, s_w, bias, w4, p), dict(q3=_tie_stats(t1), q=_tie_stats(t2))
    e = 3
    x, w, s_w, bias = _tie_operands(gen, TIE_M, TIE_K, TIE_N, w4, 2.0 ** -5, 2.0 ** -e)
    y = oracle.qgemm(x, torch.tensor(2.0 ** -5), w, s_w, bias)
    return (x, w, 2.0 ** -5, s_w, bias, w4, dict(e_req=e, e_head=e)), dict(q=_tie_stats(y.double() * 2.0 ** e))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
@pytest.mark.parametrize('kind', ['requant', 'head', 'resid', 'resid_pre', 'embed'])
def test_gemm_exact_ties(dva, oracle, kind, w4):
    """M = 129, K = 64, N = 144 with the recipe of _tie_operands: every quotient of the epilogue is a multiple of 1/2 (RESID: dyadic
    s_mid / s_next, s_res = s_next / 2; EMBED: dyadic scales and position codes), so the rounding decides on exact ties on a fixed
    share of the outputs - pack4_pre's add of 1.5 * 2^23, the rintf chains of HEAD and EMBED, the margin tests of div_q8fx4 and of the
    pre-folded RESID epilogue with their IEEE-division fall-backs.  Tiled kernel at both tile heights and the few-rows kernel.
    Asserted on the reference alone, before the first launch, for EVERY quotient: at least 2000 exact ties inside (-128.5, 127.5), at
    least 500 of them rounding up, 500 down, 500 positive, 500 negative, and at least one output on 127.5 and one on -128.5 (planted
    through activation row 0; EMBED's q2 = q1 / 2 cannot reach them).  What the seeds give, ties of outputs in range (up /
    down / positive / negative; on 127.5 / on -128.5):
      REQUANT, HEAD             w8 4378 of 8641 (2238 / 2140 / 2154 / 2224; 5 / 5)      w4 7454 of 14874 (3762 / 3692 / 3767 / 3687; 13 / 9)
      RESID q3                  w8 4229 of 8645 (2077 / 2152 / 2101 / 2128; 6 / 5)      w4 7431 of 14878 (3737 / 3694 / 3751 / 3680; 8 / 3)
      RESID second quotient     w8 4951 of 11481 (2473 / 2478 / 2334 / 2617; 14 / 12)   w4 6465 of 14093 (3140 / 3325 / 3188 / 3277; 10 / 8)
      EMBED q1                  w8 4323 of 8530 (2204 / 2119 / 2129 / 2194; 5 / 6)      w4 7401 of 14770 (3733 / 3668 / 3746 / 3655; 14 / 9)
      EMBED q2                  w8 7144 of 18576 (6119 / 1025 / 6077 / 1067)            w4 5575 of 18576 (3715 / 1860 / 3757 / 1818)
      EMBED q                   w8 5028 of 18571 (2546 / 2482 / 2539 / 2489; 2 / 3)     w4 5008 of 18573 (2471 / 2537 / 2480 / 2528; 1 / 2)"""
    E = dva.engine
    args, stats = _tie_case(oracle, kind, w4)
    for name, st in stats.items():
        assert st['ties'] >= 2000 and min(st['up'], st['down'], st['pos'], st['neg']) >= 500, (kind, name, st)
        assert name == 'q2' or (st['hi_edge'] >= 1 and st['lo_edge'] >= 1), (kind, name, st)       # |q2| <= 64: no edge to reach
    lay = Layer(E, oracle, *args)
    ref = lay.reference(oracle, kind, TIE_M)
    paths = ('tile128', 'tile256', 'rows') if kind in ('requant', 'resid', 'resid_pre') else ('tile128',)
    for path in paths:
        with tuning(E.lib(), **PATHS[path]):
            got = twice(lambda s: lay.run(kind, TIE_M, TIE_K, TIE_N + 16, s))
        _check(got, ref, (kind, w4, path))


@pytest.mark.parametrize('w4', [False, True], ids=['w8', 'w4'])
def test_gemm_accumulators_at_the_top_of_the_domain(dva, oracle, w4):
    """K = 1024 (4-bit weights: 3072): activation rows of all 127, all -128, alternating and uniform in [100, 127] against weight rows of
    +-127 (4-bit: -8 / 7): |acc| reaches 16 646 144 (4-bit: 3 145 728 = 3072 x 128 x 8), just inside the 2^24 that oracle.qgemm asserts
    and the kernels' comments promise.  The bias 0.3 makes the single rounding of fma(acc, colscale, bias) visible in tap_out; REQUANT,
    HEAD, arithmetic GELU; tiled kernel and few-rows kernel."""
    E = dva.engine
    gen = _gen(2100)
    K, N, M = (3072, 32, 8) if w4 else (1024, 32, 8)
    hi_w, lo_w = (7.0, -8.0) if w4 else (127.0, -127.0)
    x = torch.zeros(M, K)
    x[0], x[1] = 127.0, -128.0
    x[2, 0::2], x[2, 1::2] = 127.0, -128.0
    x[3, 0::2], x[3, 1::2] = -128.0, 127.0
    x[4:] = _randint(gen, 100, 127, (M - 4, K))
    w = torch.where(torch.rand(N, K, generator=gen) < 0.5, torch.tensor(lo_w), torch.tensor(hi_w))
    w[0], w[1] = hi_w, lo_w
    w[2, 0::2], w[2, 1::2] = hi_w, lo_w
    w[3, 0::2], w[3, 1::2] = lo_w, hi_w
    amax = float((x.double() @ w.double().t()).abs().max())
    assert amax == (3072 * 128 * 8 if w4 else 1024 * 128 * 127) and amax < 2.0 ** 24
    cs = 2.0 ** (-18 if w4 else -20)
    lay = Layer(E, oracle, x, w, 2.0 ** -5, torch.full((N,), cs * 32.0), torch.full((N,), 0.3), w4, dict(e_req=3, e_head=3, e_gelu=3))
    assert float(lay.y.abs().max()) > 11.9 and len(torch.unique(lay.y)) > 60
    for kind, path in (('requant', 'tile128'), ('requant', 'tile256'), ('requant', 'rows'), ('gelu', 'tile128'), ('gelu', 'rows'), ('head', 'tile128')):
        tap = kind != 'head' and path != 'rows'
        with tuning(E.lib(), **PATHS[path]):
            got = twice(lambda s: lay.run(kind, M, K, N + 16, s, tap=tap))
        ref = lay.reference(oracle, kind, M)
        if tap:
            ref['tap'] = lay.y
        _check(got, ref, ('accumulators', kind, path, w4))
