"""No GPU: the argument checks of the LayerNorm entry points around the 4096-channel limit (rows of 2049 ... 4096 channels run the
kernel of csrc/p2vit_ln_xwide.hip).  Every refusal here comes from the entry layer, ahead of its first HIP call: the pointers are
dummies that nothing may follow, and the codes and messages are the entry layer's own (a HIP call without a device, or with these
pointers, would answer P2V_E_LAUNCH / P2V_E_ARG 'not a device pointer' instead)."""
import ctypes as C

import pytest

_DUMMY = C.c_void_p(4096)             # non-null, never dereferenced


@pytest.fixture(scope='module')
def E():
    import diff_vit_amd
    diff_vit_amd.engine.lib()
    return diff_vit_amd.engine


def test_prefold_accepts_3072_channels_up_to_the_constants(E):
    """C = 3072 (the PatchMerging LayerNorm behind a 768-channel stage) passes the shape check: a LayerNorm with null arrays is then
    refused for its missing constants.  (Before the 4096-channel limit the answer was P2V_E_SHAPE, 'up to 2048'.)"""
    L = E.lib()
    for C_ in (2052, 3072, 4096):
        ln = E.Ln()
        rc = L.p2v_ln_prefold(C.byref(ln), C_, _DUMMY, 1 << 20)
        assert rc == E.E_ARG, (C_, rc, L.p2v_last_error())
        assert L.p2v_last_error() == b'p2v_ln_prefold: LayerNorm constants missing'
        assert not ln.pre.gm and not ln.pre.bt


@pytest.mark.parametrize('C_', [4100, 4098, 8192, 0, -4])
def test_prefold_refuses_beyond_4096(E, C_):
    L = E.lib()
    ln = E.Ln()
    rc = L.p2v_ln_prefold(C.byref(ln), C_, _DUMMY, 1 << 20)
    assert rc == E.E_SHAPE, (C_, rc, L.p2v_last_error())
    assert L.p2v_last_error() == b'p2v_ln_prefold: C must be a positive multiple of 4 up to 4096'
    assert not ln.pre.gm


def test_prefold_bytes(E):
    L = E.lib()
    for C_ in (3072, 4096, 2052, 3076, 4092):
        assert L.p2v_ln_prefold_bytes(C_) == 2 * ((C_ + 255) // 256 * 256) * 4, C_
    assert L.p2v_ln_prefold_bytes(3072) == 24576 and L.p2v_ln_prefold_bytes(4096) == 32768


def test_int_layernorm_refuses_beyond_4096_before_the_launch(E):
    """C = 4100 is a shape refusal of the entry point (the launcher, which has no kernel for it, is never reached: it would answer
    P2V_E_LAUNCH); C = 4098 meets the multiple-of-4 refusal first, as at every width."""
    L = E.lib()
    ln = E.Ln()
    rc = L.p2v_int_layernorm(_DUMMY, 4100, 3, 4100, C.byref(ln), _DUMMY, 4100, None)
    assert rc == E.E_SHAPE, (rc, L.p2v_last_error())
    assert b'p2v_int_layernorm: C=4100' in L.p2v_last_error() and b'4096' in L.p2v_last_error()
    rc = L.p2v_int_layernorm(_DUMMY, 4100, 3, 4098, C.byref(ln), _DUMMY, 4100, None)
    assert rc == E.E_UNSUPPORTED and L.p2v_last_error() == b'C and strides must be multiples of 4'
    # beyond 2048 channels a row_stride inside the row (overlapping input rows) is a shape refusal too, at any row count
    for rows in (1, 3):
        rc = L.p2v_int_layernorm(_DUMMY, 64, rows, 3072, C.byref(ln), _DUMMY, 3072, None)
        assert rc == E.E_SHAPE and b'row_stride >= C' in L.p2v_last_error(), (rows, rc, L.p2v_last_error())
    assert L.p2v_int_layernorm(_DUMMY, 64, 1, 4096, C.byref(ln), _DUMMY, 4096, None) == E.E_SHAPE
    # the recorded form goes through the same checks
    ops = (E.Op * 1)()
    ops[0].kind, ops[0].inp, ops[0].out = E.OP_LAYERNORM, _DUMMY, _DUMMY
    ops[0].M, ops[0].N, ops[0].lda, ops[0].ldo = 3, 4100, 4100, 4100
    assert L.p2v_run_ops(ops, 1, None) == E.E_SHAPE and b'4096' in L.p2v_last_error()
