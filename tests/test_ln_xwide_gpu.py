"""GPU: p2v_int_layernorm on rows of 2049 ... 4096 channels (k_int_layernorm_xwide, csrc/p2vit_ln_xwide.hip: a row per workgroup, the
row sums through LDS as integers) - values against oracle.int_layernorm clamped as in tests/test_kernel_edges_gpu.py, rows whose sum
of squares lies between 2^31 and 2^32, the output footprint in sentinel arenas, and the unchanged routing at 2048 channels and below.

The statistics are exact while C * (128 * mask_max)^2 < 2^32 (SwinPlan._ln refuses otherwise): any PTF mask of {1, 2, 4, 8} up to
3072 channels, masks {1, 2, 4} beyond in these tests; _bound() asserts it for every case before the launch."""
import ctypes as C
import itertools

import pytest
import torch

from _arena import Arena, twice
from _tuning import tuning
from conftest import gpu_ok
from test_kernel_edges_gpu import Layer, Norm, _check, _codes, _gen, _run_layernorm, _sync, dva  # noqa: F401  (dva: fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

WIDTHS = (2052, 2304, 3072, 3076, 4092, 4096)       # first width of the kernel, a partly empty last group, both NCH (3: <= 3072, 4)
ROWS = (1, 3, 37)                                   # fewer rows than a workgroup walks (8), several workgroups with a ragged tail


def _masks(gen, C_):
    """PTF masks drawn from {1, 2, 4, 8} ({1, 2, 4} beyond 3072 channels), every value present, one channel pinned to 1"""
    top = 4 if C_ <= 3072 else 3
    m = 2.0 ** torch.randint(0, top, (C_,), generator=gen).float()
    m[:top] = 2.0 ** torch.arange(top).float()
    return m


def _bound(C_, mask):
    assert C_ * (128.0 * float(mask.max())) ** 2 < 2.0 ** 32, (C_, float(mask.max()))


class generic_chain:
    """p2v_set_tuning('ln_generic', 1) for a block: every row takes the generic per-element chain"""

    def __init__(self, L, on):
        self.L, self.on = L, on

    def __enter__(self):
        assert self.L.p2v_set_tuning(b'ln_generic', 1 if self.on else 0) == 0

    def __exit__(self, *exc):
        assert self.L.p2v_set_tuning(b'ln_generic', 0) == 0


@pytest.mark.parametrize('C_', WIDTHS)
def test_xwide_values(dva, oracle, C_):
    """rows in {1, 3, 37} x fast / generic chain x constants folded ahead (p2v_ln_prefold) or per workgroup, power-of-two output
    scales with a post multiplier; and a non-power-of-two out_scale through the out_scale != NULL division, folded and not"""
    E = dva.engine
    L = E.lib()
    gen = _gen(4100 + C_)
    codes = _codes(gen, (max(ROWS), C_), 35.0)
    for chain in ('pot', 'div'):
        mask = _masks(gen, C_)
        _bound(C_, mask)
        norm = Norm(E, gen, C_, chain, mask=mask)
        ref, finite = norm.reference(oracle, codes)
        assert bool(finite.all())
        for rows, generic, pre in itertools.product(ROWS, (False, True) if chain == 'pot' else (False,), (False, True)):
            norm.prefold(pre)
            with generic_chain(L, generic):
                got = _run_layernorm(E, norm, codes[:rows], C_, C_, 0x5B)
            _check(got, dict(out=ref[:rows]), ('xwide', C_, chain, rows, generic, pre))
        norm.prefold(False)
        with tuning(L, ln_pre=0):                   # the switch that ignores p2v_ln.pre reaches the kernel too
            norm.prefold(True)
            got = _run_layernorm(E, norm, codes[:3], C_, C_, 0xA6)
        _check(got, dict(out=ref[:3]), ('xwide ln_pre=0', C_, chain))
        norm.prefold(False)


def _bound_rows(C_):
    """all -128, alternating -128 / 127, one 127 among -128s, a constant row of 127 (zero variance), and their sums of squares"""
    alt = torch.full((C_,), -128.0)
    alt[1::2] = 127.0
    one = torch.full((C_,), -128.0)
    one[C_ // 3] = 127.0
    return torch.stack([torch.full((C_,), -128.0), alt, one, torch.full((C_,), 127.0)])


@pytest.mark.parametrize('chain', ['pot', 'div'])
@pytest.mark.parametrize('C_,m', [(3072, 8.0), (4096, 4.0)])
def test_xwide_at_the_bound_of_the_sums(dva, oracle, C_, m, chain):
    """the largest mask everywhere: sum x_q^2 = C * (128 m)^2 = 0.75 * 2^32 for the row of -128s at C = 3072, mask 8 (2^30 at
    C = 4096, mask 4) - beyond any signed 32-bit value at 3072.  A constant row has zero variance: whatever the oracle yields for it
    (NaN: the row is present, not compared; otherwise compared)."""
    E = dva.engine
    L = E.lib()
    gen = _gen(4200 + C_)
    codes = _bound_rows(C_)
    mask = torch.full((C_,), m)
    _bound(C_, mask)
    s2 = ((codes * m).double() ** 2).sum(1)
    assert float(s2[0]) == C_ * (128.0 * m) ** 2 and float(s2.max()) < 2.0 ** 32
    if C_ == 3072:
        assert float(s2[0]) == 0.75 * 2.0 ** 32 and float(s2[:3].min()) > 2.0 ** 31
    norm = Norm(E, gen, C_, chain, mask=mask)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite[1]) and bool(finite[2]), 'the rows with a variance are compared'
    for generic, pre in itertools.product((False, True) if chain == 'pot' else (False,), (False, True)):
        norm.prefold(pre)
        with generic_chain(L, generic):
            got = twice(lambda s: _run_layernorm(E, norm, codes, C_, C_, s))
        g, r = got['out'][finite], ref[finite]
        assert torch.equal(g, r), (C_, chain, generic, pre, int((g != r).sum()), [int(v) for v in (g != r).sum(1)])
    norm.prefold(False)


@pytest.mark.parametrize('C_', [2052, 3072, 4096])
def test_xwide_footprint(dva, oracle, C_):
    """row_stride in {C, C + 12, 5 C} x out_stride in {C, C + 20}, rows in {3, 37}: nothing outside [0, C) of `rows` rows is written
    (Arena.read), and a second launch into arenas of another sentinel gives the same bytes (twice)"""
    E = dva.engine
    gen = _gen(4300 + C_)
    mask = _masks(gen, C_)
    _bound(C_, mask)
    norm = Norm(E, gen, C_, mask=mask)
    codes = _codes(gen, (37, C_), 35.0)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    for i, (rs, os_) in enumerate(itertools.product((C_, C_ + 12, 5 * C_), (C_, C_ + 20))):
        rows = (37, 3)[i % 2] if rs != 5 * C_ else 3
        norm.prefold(i % 3 == 0)
        got = twice(lambda s: _run_layernorm(E, norm, codes[:rows], rs, os_, s))
        _check(got, dict(out=ref[:rows]), ('xwide footprint', C_, rows, rs, os_))
    norm.prefold(False)


@pytest.mark.parametrize('C_', [384, 1024, 2048])
def test_routing_below_2049_is_unchanged(dva, oracle, C_):
    """widths the new kernel does not take: the same bytes as the oracle, as before (rows per half wave 1 and 4, folded or not)"""
    E = dva.engine
    L = E.lib()
    gen = _gen(4400 + C_)
    norm = Norm(E, gen, C_)
    codes = _codes(gen, (37, C_), 35.0)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    for ln_rows, pre in itertools.product((1, 4), (False, True)):
        norm.prefold(pre)
        with tuning(L, ln_rows=ln_rows):
            got = twice(lambda s: _run_layernorm(E, norm, codes, C_, C_ + 20, s))
        _check(got, dict(out=ref), ('routing', C_, ln_rows, pre))
    norm.prefold(False)


def test_torch_op_follows(dva, oracle):
    """torch.ops.p2vit.int_layernorm at 3072 channels: the same entry point, nothing of its own to widen"""
    E = dva.engine
    gen = _gen(4600)
    C_ = 3072
    norm = Norm(E, gen, C_, mask=_masks(gen, C_))
    codes = _codes(gen, (5, C_), 35.0)
    ref, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    dv = norm.dev
    got = torch.ops.p2vit.int_layernorm(codes.to(torch.int8).cuda(), norm.ln.s1, dv[0], dv[1], dv[2], dv[3], dv[4])
    assert got.dtype == torch.int8 and torch.equal(got.cpu().float(), ref)


def test_run_ops_layernorm_3072_then_reduction(dva, oracle):
    """one recorded list P2V_OP_LAYERNORM (C = 3072) -> P2V_OP_GEMM REQUANT (K = 3072, N = 1536), the PatchMerging pair of Swin-L,
    against the oracle's LayerNorm + qgemm"""
    E = dva.engine
    gen = _gen(4500)
    M, C_, N = 37, 3072, 1536
    mask = _masks(gen, C_)
    _bound(C_, mask)
    norm = Norm(E, gen, C_, mask=mask)
    codes = _codes(gen, (M, C_), 35.0)
    q0, finite = norm.reference(oracle, codes)
    assert bool(finite.all())
    w = _codes(gen, (N, C_), 30.0)
    lay = Layer(E, oracle, q0, w, norm.s_a, torch.full((N,), 2.0 ** -9), torch.zeros(N), False, dict(e_req=1))
    q1 = lay.reference(oracle, 'requant', M)['out']
    assert float(q1.abs().mean()) > 4.0 and float((q1.abs() >= 127).float().mean()) < 0.5, 'the output codes use their range'

    def run(sentinel):
        a = Arena(M, C_, C_, torch.int8, sentinel, init=codes)
        mid = Arena(M, C_, C_, torch.int8, sentinel)
        out = Arena(M, N, N, torch.int8, sentinel)
        ops = (E.Op * 2)()
        ops[0].kind, ops[0].inp, ops[0].out = E.OP_LAYERNORM, a.ptr, mid.ptr
        ops[0].M, ops[0].N, ops[0].lda, ops[0].ldo, ops[0].ln = M, C_, C_, C_, norm.ln
        k, epi = lay.epilogue('requant')
        ops[1].kind, ops[1].epi, ops[1].inp, ops[1].out = E.OP_GEMM, k, mid.ptr, out.ptr
        ops[1].M, ops[1].K, ops[1].N, ops[1].lda, ops[1].ldo, ops[1].lin, ops[1].ep = M, C_, N, C_, N, lay.lin, epi
        E.check(E.lib().p2v_run_ops(ops, 2, E.stream_ptr()))
        _sync()
        a.read('run_ops x')
        return dict(ln=mid.read('run_ops ln').float(), out=out.read('run_ops out').float())
    for pre in (True, False):
        norm.prefold(pre)
        _check(twice(run), dict(ln=q0, out=q1), ('run_ops 3072 -> 1536', pre))
    norm.prefold(False)
