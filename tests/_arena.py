"""Sentinel arenas for the GPU footprint tests (tests/test_kernel_edges_gpu.py: the operator kernels; tests/test_forward_state_gpu.py: the
whole-model entry points; tests/test_modeldiff_edges_gpu.py: CKA, HSIC, pair cosine): one device allocation per operand,

    | guard | rows of the operand, `stride` apart, padding between them | guard |

filled with one byte value.  The operand starts 80 bytes behind a 256-byte boundary (a multiple of 16, not of 256: the alignment the
entry points promise, not the allocator's), each guard is at least 64 KB and at least 256 rows (1 MB around a flat operand), so a stray store of one tile still
lands in memory the test owns and is seen.  A plain helper module, not a conftest."""
import ctypes as C

import numpy as np
import torch

SENTINELS = (0x5B, 0xA6)          # 91 / -90 as int8; 0x5B5B5B5B / 0xA6A6A6A6 are finite fp32 of either sign
OFFSET = 80


class Arena:
    def __init__(self, rows, width, stride=None, dtype=torch.int8, sentinel=SENTINELS[0], init=None, offset=OFFSET):
        """rows x width elements of `dtype`, `stride` elements between row starts (default: dense).  init: tensor [rows][width] or None
        (the operand region keeps the sentinel: an output).  offset: bytes between a 256-byte boundary and the operand - 0 for a workspace
        (the entry points that take one ask for 256-byte alignment), 84 for a start that is 4-byte but not 16-byte aligned (the scalar
        load paths)."""
        self.dtype, self.rows, self.width = dtype, int(rows), int(width)
        self.item = torch.empty((), dtype=dtype).element_size()
        self.stride = self.width if stride is None else int(stride)
        assert self.stride >= self.width and self.rows >= 1
        self.sentinel = int(sentinel)
        row_b, stride_b = self.width * self.item, self.stride * self.item
        # a flat operand (one row) has no rows to count: 1 MB, the reach of 4096 threads that each store 256 bytes too far
        guard = (max(65536, 256 * stride_b if self.rows > 1 else 1 << 20) + 255) // 256 * 256
        assert 0 <= int(offset) < 256
        self.start = guard + int(offset)
        self.total = self.start + (self.rows - 1) * stride_b + row_b + guard
        host = np.full(self.total, self.sentinel, dtype=np.uint8)
        self.inside = np.zeros(self.total, dtype=bool)
        if stride_b == row_b:
            self.inside[self.start: self.start + self.rows * row_b] = True
        else:
            idx = self.start + np.arange(self.rows, dtype=np.int64)[:, None] * stride_b + np.arange(row_b, dtype=np.int64)[None, :]
            self.inside[idx.reshape(-1)] = True
        if init is not None:
            t = init.to(dtype).contiguous().reshape(self.rows, self.width)
            host[self.inside] = t.numpy().view(np.uint8).reshape(-1)
        self.dev = torch.from_numpy(host).cuda()
        assert self.dev.data_ptr() % 256 == 0
        self.raw = None

    @property
    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + self.start)

    def read(self, what=''):
        """download once: every guard and padding byte must still hold the sentinel -> the operand region as a [rows][width] tensor"""
        got = self.dev.cpu().numpy()
        self.raw = got
        bad = np.nonzero((got != self.sentinel) & ~self.inside)[0]
        if bad.size:
            rel = bad - self.start
            stride_b = self.stride * self.item
            where = [(int(r // stride_b), int(r % stride_b)) for r in rel[:6]]
            raise AssertionError('%s: %d bytes outside the result were written; first (row, byte in row): %s' % (what, bad.size, where))
        return torch.from_numpy(got[self.inside].copy().view(_NP[self.dtype]).reshape(self.rows, self.width))


_NP = {torch.int8: np.int8, torch.uint8: np.uint8, torch.float32: np.float32, torch.int32: np.int32, torch.float64: np.float64,
       torch.int64: np.int64}


def twice(run):
    """run(sentinel) -> dict of result tensors, once per sentinel, each time into fresh arenas: the guards are checked inside `run`
    (Arena.read), a store of the sentinel's own value cannot hide behind both, the input padding is poisoned with two values, and the
    second launch repeats the first bit for bit."""
    a = run(SENTINELS[0])
    b = run(SENTINELS[1])
    assert a.keys() == b.keys()
    for k in a:
        same = torch.equal(a[k], b[k]) if not a[k].is_floating_point() else \
            np.array_equal(a[k].numpy().view(np.uint32), b[k].numpy().view(np.uint32))
        assert same, ('%s differs between the two runs (poisoned padding read, or not repeatable)' % k, int((a[k] != b[k]).sum()))
    return a
