"""GPU: the model-diff kernels (p2v_cka_grams, p2v_hsic_accumulate, p2v_pair_cosine) on data whose result is exact, every operand in a
sentinel arena (tests/_arena.py).

CKA grams: integer-valued features in [-3, 3] make every product and partial sum exact in fp32 in any order, the centring is restated
one fp64 operation at a time (_cka_ref.centre_restatement, itself pinned to cka.gram_matrix on the CPU), so the comparison is bit
equality - one feature too many, or one padding float read into a product, changes an entry by a whole number.  HSIC: integer grams,
accumulators that start at non-zero integers, one and two calls.  Pair cosine: all -128 and (-128, 127) codes with closed-form sums, more
than 2^16 rows, 2048 samples (one workgroup per sample; two where the rows exceed 2^16) and the longest chain of per-channel int32 sums
the splitting rule allows.
No tolerance anywhere in this module."""
import ctypes as C

import numpy as np
import pytest
import torch

from _arena import Arena, twice
from _cka_ref import centre_restatement, small_integers
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


def _sync():
    torch.cuda.synchronize()


def _bits64(t):
    return t.contiguous().numpy().view(np.int64 if t.element_size() == 8 else np.int32)


# --------------------------------------------------------------------------------------------------
# p2v_cka_grams
# --------------------------------------------------------------------------------------------------
CKA_NS = (4, 5, 31, 32, 33, 64, 65, 256)
CKA_FS = (1, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8193)      # around the 32-feature group, the 1024-feature wave quarter, the 4096-feature chunk
CKA_LD = 8200                                                           # row stride of both operands in floats: > every F, a multiple of 4


@pytest.fixture(scope='module')
def cka_data():
    x, y = small_integers(4242, (max(CKA_NS), max(CKA_FS))), small_integers(4243, (max(CKA_NS), max(CKA_FS)))
    # on the host, before any launch: |x| @ |y|^T < 2^24 (at most 9 F), so the uncentred Gram is an exact integer matrix in fp32
    assert float((x.abs().double() @ y.abs().double().t()).max()) < 2.0 ** 24
    assert float((x.abs().double() @ x.abs().double().t()).max()) < 2.0 ** 24
    return x, y


def _cka_layers(parity):
    """(F, kind) per layer of one call: layers of DIFFERENT F; X Y^T ('other') on every second layer, X X^T given as y == NULL or as
    y == x on the layers between; the two parities together run every F both ways"""
    return [(F, 'other' if (l + parity) % 2 else ('null', 'same')[(l // 2) % 2]) for l, F in enumerate(CKA_FS)]


@pytest.mark.parametrize('n', CKA_NS)
def test_cka_grams_exact(dva, cka_data, n):
    """One call per parity with the eleven F as its layers (so every (n, F) runs as X X^T and as X Y^T), every layer a view [n][F] of the
    one x / y arena with ldx = ldy = 8200: behind the F features of a row lie further integers, behind the 8193rd the sentinel.  Once 16-byte
    aligned (float4 loads) and once at offset 84 (the scalar path): the same bits, equal to the restatement's; the X X^T grams exactly
    symmetric; grams and workspace (exactly p2v_cka_workspace_bytes, 256-byte aligned) in arenas."""
    E = dva.engine
    L = E.lib()
    X, Y = cka_data[0][:n], cka_data[1][:n]
    plans = [_cka_layers(0), _cka_layers(1)]
    ref = [[centre_restatement(X[:, :F], Y[:, :F] if kind == 'other' else None) for F, kind in p] for p in plans]

    def run(sentinel, offset):
        xa = Arena(n, max(CKA_FS), CKA_LD, torch.float32, sentinel, init=X, offset=offset)
        ya = Arena(n, max(CKA_FS), CKA_LD, torch.float32, sentinel, init=Y, offset=offset)
        res = {}
        for pi, p in enumerate(plans):
            descs = (E.CkaLayer * len(p))()
            for d, (F, kind) in zip(descs, p):
                d.x, d.features, d.ldx, d.ldy = xa.ptr, F, CKA_LD, CKA_LD
                d.y = {'null': None, 'same': xa.ptr, 'other': ya.ptr}[kind]
            nb = L.p2v_cka_workspace_bytes(descs, len(p), n)
            assert nb > 0, L.p2v_last_error()
            ws = Arena(1, nb, None, torch.uint8, sentinel, offset=0)
            out = Arena(len(p) * n, n, None, torch.float32, sentinel, offset=offset)
            E.check(L.p2v_cka_grams(descs, len(p), n, out.ptr, ws.ptr, nb, E.stream_ptr()))
            _sync()
            ws.read(('cka workspace', n, pi, offset))
            res['grams%d' % pi] = out.read(('grams', n, pi, offset)).reshape(len(p), n, n)
        assert torch.equal(xa.read(('x', n, offset)), X) and torch.equal(ya.read(('y', n, offset)), Y)
        return res

    for offset in (80, 84):
        got = twice(lambda s: run(s, offset))
        for pi, p in enumerate(plans):
            for l, (F, kind) in enumerate(p):
                g, r = got['grams%d' % pi][l], ref[pi][l]
                bad = _bits64(g) != _bits64(r)
                assert not bad.any(), (n, F, kind, offset, int(bad.sum()), float((g.double() - r.double()).abs().max()))
                if kind != 'other':
                    assert torch.equal(g, g.t()), (n, F, kind, offset)


# --------------------------------------------------------------------------------------------------
# p2v_hsic_accumulate
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('n', [4, 33, 256])
def test_hsic_accumulate_direct(dva, n, dtype):
    """g1 [3][n n], g2 [2][n n] of integers in [-7, 7]; acc [3][2], self1 [3], self2 [2] start at non-zero integers; after k = 1 and 2
    calls every accumulator is start + k * dot exactly (all below 2^24, so also in fp32), with self1 / self2 given, NULL, or one of each"""
    E = dva.engine
    L = E.lib()
    l1, l2, nn = 3, 2, n * n
    g1, g2 = small_integers(900 + n, (l1, nn), 7), small_integers(901 + n, (l2, nn), 7)
    a0 = small_integers(902 + n, (l1, l2), 900) * 2 + 1          # odd: never zero
    s10, s20 = small_integers(903 + n, (1, l1), 900) * 2 + 1, small_integers(904 + n, (1, l2), 900) * 2 + 1
    dot = g1.double() @ g2.double().t()
    d1, d2 = (g1.double() ** 2).sum(1).reshape(1, l1), (g2.double() ** 2).sum(1).reshape(1, l2)
    for start, d in ((a0, dot), (s10, d1), (s20, d2)):
        assert float((start.double().abs() + 2 * d.abs()).max()) < 2.0 ** 24           # exact in fp32 after two calls

    def run(sentinel, with1, with2):
        # flat operands: 1 MB guards (as [l][n n] rows the guards would be 256 rows of 256 KB each)
        a1 = Arena(1, l1 * nn, None, torch.float32, sentinel, init=g1.reshape(1, -1))
        a2 = Arena(1, l2 * nn, None, torch.float32, sentinel, init=g2.reshape(1, -1))
        acc = Arena(l1, l2, None, dtype, sentinel, init=a0)
        s1 = Arena(1, l1, None, dtype, sentinel, init=s10) if with1 else None
        s2 = Arena(1, l2, None, dtype, sentinel, init=s20) if with2 else None
        res = {}
        for k in (1, 2):
            E.check(L.p2v_hsic_accumulate(a1.ptr, l1, a2.ptr, l2, n, acc.ptr, s1.ptr if s1 else None, s2.ptr if s2 else None,
                                          1 if dtype == torch.float64 else 0, E.stream_ptr()))
            _sync()
            res['acc%d' % k] = acc.read(('hsic acc', n, k))
            if s1:
                res['self1_%d' % k] = s1.read(('hsic self1', n, k))
            if s2:
                res['self2_%d' % k] = s2.read(('hsic self2', n, k))
        assert torch.equal(a1.read('g1').reshape(l1, nn), g1) and torch.equal(a2.read('g2').reshape(l2, nn), g2)
        return res

    for with1, with2 in ((True, True), (False, False), (True, False), (False, True)):
        got = twice(lambda s: run(s, with1, with2))
        for k in (1, 2):
            want = {'acc%d' % k: a0.double() + k * dot}
            if with1:
                want['self1_%d' % k] = s10.double() + k * d1
            if with2:
                want['self2_%d' % k] = s20.double() + k * d2
            for name, w in want.items():
                assert got[name].dtype == dtype
                assert torch.equal(got[name].double(), w), (n, name, with1, with2, (got[name].double() - w).abs().max())
        assert set(got) == {'acc1', 'acc2'} | ({'self1_1', 'self1_2'} if with1 else set()) | ({'self2_1', 'self2_2'} if with2 else set())


# --------------------------------------------------------------------------------------------------
# p2v_pair_cosine
# --------------------------------------------------------------------------------------------------
# the bytes around a scale vector are 0xFF whatever the run's sentinel: 0xFFFFFFFF is a NaN, so a scale read behind `cols` poisons the
# sum even where it meets a per-channel sum of zero (the codes behind `cols` are loaded as zeros; a finite stray scale would go unseen)
SCALE_FILL = 0xFF


def _pow2_scales(cols):
    return 2.0 ** -(torch.arange(cols) % 4).float()


def _cos_run(E, stages, n, sentinel):
    """stages: dicts(a, b [n * rows][cols] host tensors or None with `fill` = (va, vb), rows, cols, row_stride, dtype, scale, shared) -> sums
    [stages][n][3] fp64; every operand, the scales, sums and the workspace (exactly p2v_pair_cosine_workspace_bytes) in arenas.
    shared: sample_stride = 0, one sample's buffer for all n."""
    L = E.lib()
    descs = (E.CosLayer * len(stages))()
    keep = []
    for d, st in zip(descs, stages):
        rows, cols, rs = st['rows'], st['cols'], st['row_stride']
        held = 1 if st.get('shared') else n
        a = Arena(held * rows, cols, rs, st['dtype'], sentinel, init=st['a'])
        b = Arena(held * rows, cols, rs, st['dtype'], sentinel, init=st['b'])
        sc = Arena(1, cols, None, torch.float32, SCALE_FILL, init=st['scale'].reshape(1, -1)) if st.get('scale') is not None else None
        keep.append((a, b, sc, st))
        d.a, d.b, d.scale = a.ptr, b.ptr, sc.ptr if sc else None
        d.sample_stride, d.row_stride, d.rows, d.cols = 0 if st.get('shared') else rows * rs, rs, rows, cols
        d.dtype = E.COS_I8 if st['dtype'] == torch.int8 else E.COS_F32
    nb = L.p2v_pair_cosine_workspace_bytes(descs, len(stages), n)
    assert nb > 0, L.p2v_last_error()
    ws = Arena(1, nb, None, torch.uint8, sentinel, offset=0)
    sums = Arena(len(stages) * n, 3, None, torch.float64, sentinel)
    E.check(L.p2v_pair_cosine(descs, len(stages), n, sums.ptr, ws.ptr, nb, E.stream_ptr()))
    _sync()
    ws.read('pair-cosine workspace')
    for a, b, sc, st in keep:
        assert torch.equal(a.read('pair-cosine a'), st['a'].to(st['dtype'])) and torch.equal(b.read('pair-cosine b'), st['b'].to(st['dtype']))
        if sc:
            sc.read('pair-cosine scale')
    return dict(sums=sums.read('pair-cosine sums').reshape(len(stages), n, 3))


def _const_stage(n, rows, cols, va, vb, scaled, shared=False):
    held = 1 if shared else n
    return dict(a=torch.full((held * rows, cols), float(va)), b=torch.full((held * rows, cols), float(vb)), rows=rows, cols=cols,
                row_stride=(cols + 15) // 16 * 16 + 16, dtype=torch.int8, scale=_pow2_scales(cols) if scaled else None, shared=shared)


def _const_sums(st):
    """closed form: every element of a is va and of b is vb; with scales sum_c s_c^2 (powers of two: exact in fp64)"""
    va, vb = float(st['a'][0, 0]), float(st['b'][0, 0])
    w = float(st['rows']) * (st['cols'] if st['scale'] is None else float((st['scale'].double() ** 2).sum()))
    return [va * vb * w, va * va * w, vb * vb * w]


@pytest.mark.parametrize('rows', [1, 65537, 70000])
def test_pair_cosine_extreme_codes_and_many_rows(dva, rows):
    """all -128 against all -128 and against all 127, cols 16 (whole 16-byte groups) and 17 (a group of one code), padded row strides,
    three samples of their own (sample_stride = rows * row_stride).  At n = 3 the splitting rule's cap is 682 splits per sample, so
    65 537 and 70 000 rows are cut by the 16 KB rule into 65 to 73 splits of about 1000 rows, the last one shorter (the at-most-2^16-rows
    floor of the rule is test_pair_cosine_rows_above_2_16_at_one_split_per_sample's).  Plain and with power-of-two per-channel scales:
    the sums are closed-form integers (multiples of 2^-6), asserted bit for bit."""
    E = dva.engine
    n = 3
    stages = [_const_stage(n, rows, cols, va, vb, scaled) for cols in (16, 17) for va, vb in ((-128, -128), (-128, 127), (127, -128))
              for scaled in (False, True)]
    got = twice(lambda s: _cos_run(E, stages, n, s))['sums']
    for k, st in enumerate(stages):
        want = torch.tensor(_const_sums(st), dtype=torch.float64).expand(n, 3)
        assert abs(float(want[0, 1])) < 2.0 ** 53
        assert np.array_equal(_bits64(got[k]), _bits64(want)), (rows, st['cols'], st['scale'] is not None, got[k][0].tolist(), want[0].tolist())


def _ws_bytes(E, n, stages):
    """p2v_pair_cosine_workspace_bytes of stages given as (rows, cols, scaled): it reads the shapes and the alignment only, so the
    operands are a 16-byte aligned address that nothing dereferences"""
    p = 1 << 20
    descs = (E.CosLayer * len(stages))(*[E.CosLayer(p, p, p if scaled else None, 0, (cols + 15) // 16 * 16 + 16, rows, cols, E.COS_I8)
                                         for rows, cols, scaled in stages])
    nb = E.lib().p2v_pair_cosine_workspace_bytes(descs, len(stages), n)
    assert nb > 0, E.lib().p2v_last_error()
    return nb


@pytest.mark.parametrize('rows', [65537, 70000])
def test_pair_cosine_rows_above_2_16_at_one_split_per_sample(dva, rows):
    """n = 2048 with sample_stride = 0: the cap of the splitting rule is ONE split per sample, and more than 2^16 rows raise it to
    ceil(rows / 2^16) = 2 (`min_ns` of p2v_cos_desc: no workgroup of the scaled form may sum more than 2^16 rows into its int32 channels).
    cols 16 and 17, all -128 against all -128 / all 127 and the reverse, plain and scaled.  The workspace is exactly that of two splits
    per sample - one 3 x 8-byte partial per sample and stage more than the same stages need at one row - and the closed-form sums over
    both splits (32 769 + 32 768 rows, 35 000 + 35 000) come out bit for bit."""
    E = dva.engine
    n = 2048
    stages = [_const_stage(n, rows, cols, va, vb, scaled, shared=True) for cols in (16, 17)
              for va, vb in ((-128, -128), (-128, 127), (127, -128)) for scaled in (False, True)]
    shapes = [(st['rows'], st['cols'], st['scale'] is not None) for st in stages]
    one_split = _ws_bytes(E, n, [(1, cols, scaled) for _, cols, scaled in shapes])
    assert _ws_bytes(E, n, shapes) == one_split + len(stages) * n * 3 * 8, 'two splits per sample at more than 2^16 rows'
    assert _ws_bytes(E, n, [(65536, cols, scaled) for _, cols, scaled in shapes]) == one_split, 'one split per sample up to 2^16 rows'
    got = twice(lambda s: _cos_run(E, stages, n, s))['sums']
    for k, st in enumerate(stages):
        want = torch.tensor(_const_sums(st), dtype=torch.float64).expand(n, 3)
        assert abs(float(want[0, 1])) < 2.0 ** 53
        assert np.array_equal(_bits64(got[k]), _bits64(want)), (rows, st['cols'], st['scale'] is not None, got[k][0].tolist(), want[0].tolist())


def test_pair_cosine_2048_samples_share_one_buffer(dva):
    """n = 2048 (cap = 1: one workgroup per sample, however large) with sample_stride = 0: every sample is the same buffer, 2048 equal
    rows of sums; random codes, int8 plain / scaled and fp32, odd widths"""
    E = dva.engine
    n = 2048
    gen = torch.Generator().manual_seed(77)
    stages = []
    for rows, cols, dtype, scaled in ((3, 17, torch.int8, False), (300, 50, torch.int8, True), (1, 16, torch.int8, True), (40, 5, torch.float32, False)):
        per = 16 if dtype == torch.int8 else 4
        stages.append(dict(a=torch.randint(-128, 128, (rows, cols), generator=gen).float(), b=torch.randint(-128, 128, (rows, cols), generator=gen).float(),
                           rows=rows, cols=cols, row_stride=(cols + per - 1) // per * per + per, dtype=dtype,
                           scale=_pow2_scales(cols) if scaled else None, shared=True))
    got = twice(lambda s: _cos_run(E, stages, n, s))['sums']
    for k, st in enumerate(stages):
        a, b = st['a'].double(), st['b'].double()
        s2 = torch.ones(st['cols'], dtype=torch.float64) if st['scale'] is None else st['scale'].double() ** 2
        want = torch.stack([(a * b * s2).sum(), (a * a * s2).sum(), (b * b * s2).sum()]).expand(n, 3)          # integers times 2^-6: exact in any order
        assert np.array_equal(_bits64(got[k]), _bits64(want)), (k, got[k][0].tolist(), want[0].tolist())


@pytest.mark.parametrize('rows,cols', [(1, 4), (197, 5), (65537, 4), (33, 1000)])
def test_pair_cosine_fp32_integers_exact(dva, rows, cols):
    """the fp32 form on integer-valued data: fp64 products and sums of integers below 2^53 are exact in every order, so the sums equal
    the integer sums bit for bit (include/p2vit.h: 'fp64 products (exact) and sums').  65 537 rows at n = 3 are a row count past 2^16 for
    the indexing only: the 16 KB rule cuts them into 64 splits of 1025 rows (the last one shorter), far above the at-most-2^16-rows floor,
    which belongs to the scaled int8 form and to test_pair_cosine_rows_above_2_16_at_one_split_per_sample"""
    E = dva.engine
    n = 3
    gen = torch.Generator().manual_seed(rows + cols)
    a = torch.randint(-128, 128, (n * rows, cols), generator=gen).float() * 256.0
    b = torch.randint(-128, 128, (n * rows, cols), generator=gen).float() * 256.0
    a[0], b[0] = -32768.0, 32512.0
    st = dict(a=a, b=b, rows=rows, cols=cols, row_stride=(cols + 3) // 4 * 4 + 4, dtype=torch.float32, scale=None)
    got = twice(lambda s: _cos_run(E, [st], n, s))['sums'][0]
    ad, bd = a.double().reshape(n, -1), b.double().reshape(n, -1)
    want = torch.stack([(ad * bd).sum(1), (ad * ad).sum(1), (bd * bd).sum(1)], 1)
    assert float(want.abs().max()) < 2.0 ** 53
    assert np.array_equal(_bits64(got), _bits64(want)), (rows, cols)


# the longest chain of per-channel int32 sums: ns = 1 needs n >= 2048 and rows <= 65 536, one row lane per column group needs >= 256 column
# groups (cols >= 4081): a thread then adds 65 536 products of at most 2^14, 2^30 in all.  Operands of 256 MB: built and checked on the device
CHAIN_N, CHAIN_ROWS, CHAIN_COLS = 2048, 65536, 4096


class _DeviceArena:
    """a flat operand of one byte value between two 1 MB guards, built and checked on the device (the host arenas of _arena.py would move
    256 MB each way per operand)"""
    GUARD = 1 << 20

    def __init__(self, nbytes, value, sentinel):
        self.n, self.sentinel = nbytes, sentinel
        self.dev = torch.full((2 * self.GUARD + nbytes,), sentinel, dtype=torch.uint8, device='cuda')
        self.dev[self.GUARD: self.GUARD + nbytes] = value & 0xFF
        self.value = value & 0xFF
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = C.c_void_p(self.dev.data_ptr() + self.GUARD)

    def check(self, what):
        g = self.GUARD
        assert bool((self.dev[:g] == self.sentinel).all()) and bool((self.dev[g + self.n:] == self.sentinel).all()), (what, 'guard written')
        assert bool((self.dev[g: g + self.n] == self.value).all()), (what, 'operand written')


def test_pair_cosine_longest_int32_chain(dva):
    """the scaled form at n = 2048, rows = 65 536, cols = 4096 with sample_stride = 0: one workgroup per sample, one thread per column
    group, each per-channel int32 sum runs over all 65 536 rows of +-2^14 and ends at exactly +-2^30 (all -128 against all -128) or
    -65 536 * 16 256 (against all 127).  Closed-form sums, bit for bit; sums and workspace in host arenas."""
    E = dva.engine
    L = E.lib()
    n, rows, cols = CHAIN_N, CHAIN_ROWS, CHAIN_COLS
    scale = _pow2_scales(cols)

    def run(sentinel):
        a = _DeviceArena(rows * cols, -128, sentinel)
        res = {}
        for tag, vb in (('same', -128), ('other', 127)):
            b = _DeviceArena(rows * cols, vb, sentinel)
            sc = Arena(1, cols, None, torch.float32, SCALE_FILL, init=scale.reshape(1, -1))
            d = E.CosLayer(a.ptr, b.ptr, sc.ptr, 0, cols, rows, cols, E.COS_I8)
            descs = (E.CosLayer * 1)(d)
            nb = L.p2v_pair_cosine_workspace_bytes(descs, 1, n)
            one_row = (E.CosLayer * 1)(E.CosLayer(a.ptr, b.ptr, sc.ptr, 0, cols, 1, cols, E.COS_I8))
            assert nb == L.p2v_pair_cosine_workspace_bytes(one_row, 1, n), 'one split per sample: the chain of a thread covers every row'
            ws = Arena(1, nb, None, torch.uint8, sentinel, offset=0)
            sums = Arena(n, 3, None, torch.float64, sentinel)
            E.check(L.p2v_pair_cosine(descs, 1, n, sums.ptr, ws.ptr, nb, E.stream_ptr()))
            _sync()
            ws.read('chain workspace'); sc.read('chain scale'); b.check('chain b')
            res[tag] = sums.read('chain sums')
            del b
        a.check('chain a')
        return res

    got = twice(run)
    w = float(rows) * float((scale.double() ** 2).sum())
    assert rows * 128 * 128 == 2 ** 30
    for tag, vb in (('same', -128.0), ('other', 127.0)):
        want = torch.tensor([-128.0 * vb * w, 16384.0 * w, vb * vb * w], dtype=torch.float64).expand(n, 3)
        assert np.array_equal(_bits64(got[tag]), _bits64(want)), (tag, got[tag][0].tolist(), want[0].tolist())
