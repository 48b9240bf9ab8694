"""CPU: what the class-row path adds to the C ABI is exported, declared to the binding and refuses bad arguments before any HIP call."""
import ctypes as C

import pytest


def _lib():
    import diff_vit_amd
    if not diff_vit_amd.engine.available():
        pytest.fail('libp2vit_hip.so is not built: run __graft_entry__.build()')
    return diff_vit_amd.engine, diff_vit_amd.engine.lib()


def test_new_entry_point_is_exported_and_bound():
    E, L = _lib()
    raw = C.CDLL(E.LIB_PATH)
    assert hasattr(raw, 'p2v_lis_attention_rows')
    assert len(L.p2v_lis_attention_rows.argtypes) == 9
    assert L.p2v_abi_version() == E.P2V_ABI_VERSION == 6                    # additive: the ABI version did not move


def test_attention_rows_refuses_bad_arguments_without_gpu():
    E, L = _lib()
    one = C.c_void_p(16)
    at = E.Attn(2.0 ** -8, 0.125, 16.0, 1.0, -12, 43, 714)
    call = lambda qkv, tokens, rows, out, a=at: L.p2v_lis_attention_rows(qkv, 1, tokens, 1, 64, C.byref(a) if a is not None else None, rows, out, None)
    assert call(None, 4, 1, one) == E.E_ARG
    assert call(one, 4, 1, None) == E.E_ARG
    assert call(one, 4, 1, one, None) == E.E_ARG
    assert call(one, 0, 1, one) == E.E_SHAPE
    assert call(one, 4, 0, one) == E.E_SHAPE
    assert call(one, 4, -3, one) == E.E_SHAPE
    assert call(one, 4, 5, one) == E.E_SHAPE                                # more query rows than tokens
    assert b'query_rows' in L.p2v_last_error()
    bad = E.Attn(2.0 ** -8, 0.125, 2.0 ** 12, 1.0, -2839, 11089, 46843912)   # qact_attn1 scale 2^-12: outside the exact range, as p2v_lis_attention
    assert call(one, 4, 1, one, bad) != 0


def test_new_tuning_switches():
    E, L = _lib()
    for name, good, bad in ((b'gemm_rows', (0, 1, 2), (-1, 3)), (b'cls_rows', (0, 1), (-1, 2))):
        try:
            for v in good:
                assert L.p2v_set_tuning(name, v) == 0
            for v in bad:
                assert L.p2v_set_tuning(name, v) == E.E_ARG
                assert b'out of range' in L.p2v_last_error()
        finally:
            L.p2v_set_tuning(name, 1 if name == b'cls_rows' else 0)


def test_custom_op_registered():
    import torch
    import diff_vit_amd as dva
    assert 'lis_attention_rows' in dva.ops.OPS and hasattr(torch.ops.p2vit, 'lis_attention_rows')
    with pytest.raises(NotImplementedError):                                # no CPU kernel: no silent fallback
        torch.ops.p2vit.lis_attention_rows(torch.zeros(1, 4, 192, dtype=torch.int8), 1, 2.0 ** -8, 0.125, 16.0, 1.0, -12, 43, 714, 1)
