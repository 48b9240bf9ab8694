"""CPU: the batch slices ``FrozenPlan.slice_sizes`` chooses, and the slice-to-stream rule of ``forward_streams`` / ``profile_streams``."""
import types

import pytest

from diff_vit_amd.plan import FrozenPlan

# (D, tokens, batch, n_streams) -> slices
SLICES = [((384, 197, 256, 3), [68, 68, 68, 52]),
          ((384, 197, 192, 3), [51, 51, 51, 39]),
          ((384, 197, 128, 3), [47, 47, 34]),
          ((384, 197, 64, 3), [37, 27]),
          ((384, 197, 32, 3), [32]),
          ((384, 197, 256, 2), [93, 93, 70]),
          ((384, 197, 256, 1), [256]),
          ((384, 577, 64, 3), [37, 27]),
          ((192, 197, 256, 3), [93, 93, 70]),
          ((768, 197, 512, 3), [256, 256]),
          ((768, 197, 64, 3), [32, 32]),
          ((768, 197, 63, 3), [63]),
          ((384, 197, 1, 3), [1])]


@pytest.mark.parametrize('case,want', SLICES, ids=['-'.join(map(str, c)) for c, _ in SLICES])
def test_slice_sizes(case, want):
    D, tokens, batch, n_streams = case
    got = FrozenPlan.slice_sizes(types.SimpleNamespace(D=D, tokens=tokens), batch, n_streams)
    assert got == want and sum(got) == batch


def test_slice_streams_is_round_robin_with_the_callers_stream_last():
    """slice i runs on stream i % (n_side + 1); index n_side is the caller's stream"""
    for n_side in (1, 2, 3):
        for n_slices in range(1, 7):
            assert FrozenPlan.slice_streams(n_slices, n_side) == [i % (n_side + 1) for i in range(n_slices)]
