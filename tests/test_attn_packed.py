"""CPU: what the library says about the packed attention kernel (k_lis_attention_packed: head_dim 64, 609 .. p2v_packed_tokens tokens, no
probs_k tap) - its token limit, the kernel selection p2v_launch_attention itself follows, and the "attn_packed" switch.  No compute calls."""
import pytest


@pytest.fixture(scope='module')
def EL():
    import diff_vit_amd
    E = diff_vit_amd.engine
    if not E.available():
        pytest.fail('libp2vit_hip.so is not built: run __graft_entry__.build()')
    return E, E.lib()


RESIDENT, PACKED, STREAM, REFUSED = 0, 1, 2, -1


def test_packed_token_limit(EL):
    E, L = EL
    limit = L.p2v_packed_tokens(64)
    assert [L.p2v_packed_tokens(h) for h in (32, 48, 64, 80, 96, 128, 16)] == [0, 0, limit, 0, 0, 0, 0]
    assert 1025 < limit <= L.p2v_max_tokens(64)
    assert limit > L.p2v_resident_tokens(64)
    assert limit % 64 == 0                                    # whole 64-key groups: a launch pads by fewer than 64 keys


def test_attention_kernel_selection(EL):
    E, L = EL
    limit = L.p2v_packed_tokens(64)
    k = L.p2v_attention_kernel
    assert k(64, 1, 0) == RESIDENT and k(64, 197, 0) == RESIDENT and k(64, 608, 0) == RESIDENT
    assert k(64, 609, 0) == PACKED and k(64, limit, 0) == PACKED
    assert k(64, limit + 1, 0) == STREAM and k(64, 4096, 0) == STREAM
    assert k(64, 609, 1) == STREAM                            # the probs_k tap stays on the streaming kernel
    assert k(64, 608, 1) == RESIDENT
    assert k(128, 609, 0) == STREAM and k(32, 700, 0) == STREAM and k(96, 545, 0) == STREAM and k(96, 544, 0) == RESIDENT
    try:
        assert L.p2v_set_tuning(b'attn_packed', 0) == 0
        assert k(64, 609, 0) == STREAM and k(64, limit, 0) == STREAM and k(64, 608, 0) == RESIDENT
    finally:
        assert L.p2v_set_tuning(b'attn_packed', 1) == 0
    try:
        assert L.p2v_set_tuning(b'attn_stream', 1) == 0
        assert k(64, 197, 0) == STREAM and k(64, 609, 0) == STREAM
    finally:
        assert L.p2v_set_tuning(b'attn_stream', 0) == 0
    assert k(64, 609, 0) == PACKED
    assert k(64, 4097, 0) == REFUSED and k(16, 197, 0) == REFUSED and k(64, 0, 0) == REFUSED


def test_attn_packed_switch_values(EL):
    E, L = EL
    try:
        for v in (0, 1):
            assert L.p2v_set_tuning(b'attn_packed', v) == 0
        for v in (-1, 2):
            assert L.p2v_set_tuning(b'attn_packed', v) == E.E_ARG
            assert L.p2v_last_error() == b'p2v_set_tuning: unknown switch or value out of range: attn_packed = %d' % v
    finally:
        assert L.p2v_set_tuning(b'attn_packed', 1) == 0
