"""Device-side sentinel arenas for operands of several GiB (tests/test_large_offsets_gpu.py): the layout of tests/_arena.py,

    | low guard | rows of the operand, `stride` apart, padding between them | high guard |

one device allocation filled with one of its two SENTINELS, but nothing of it ever exists on the host: the fill, the initialisation
(a small host block, repeated down the rows on the device), the gather of the result rows and the check of every other byte all run on
the device, the check in chunks of at most 256 MiB.

Guards: the rule of _arena.py - 64 KB, or 256 rows (1 MB around a flat operand) - with the 256 rows capped at max(64 MiB, one row),
since 256 rows of a GiB stride cannot be owned.  low_guard = 1 << 31 is for an operand whose offsets a kernel holds, or may come to
hold, in 32 bits: an offset in [2^31, 2^32) that is sign-extended lands 2^32 - off bytes BELOW the operand, inside that guard, one that is
truncated mod 2^32 lands inside the arena - a wrong address is a wrong value or a changed guard byte, not a fault.  It is the default
(low_guard = None) for every operand that reaches 2^31 bytes, since only such an operand has an offset with bit 31 set; pass a size to
override it.
A plain helper module, not a conftest."""
import ctypes as C

import torch

from _arena import OFFSET, SENTINELS

CHUNK = 1 << 28                   # bytes per reduction: no temporary beyond a chunk's mask


class BigArena:
    def __init__(self, rows, width, stride=None, dtype=torch.int8, sentinel=SENTINELS[0], init=None, low_guard=None, offset=OFFSET,
                 cover=0):
        """rows x width elements of `dtype`, `stride` elements between row starts (default: dense).  init: host tensor [r][width], r <= rows:
        row i of the operand holds init[i % r]; None: the operand region keeps the sentinel (an output).  cover: bytes behind the operand's
        start that the arena owns before its high guard begins, at least (for a call that is to be refused at a longer stride: what it would
        have touched is memory of the test)."""
        self.dtype, self.rows, self.width = dtype, int(rows), int(width)
        self.item = torch.empty((), dtype=dtype).element_size()
        self.stride = self.width if stride is None else int(stride)
        assert self.stride >= self.width and self.rows >= 1
        self.sentinel = int(sentinel)
        row_b, stride_b = self.width * self.item, self.stride * self.item
        guard = max(65536, min(256 * stride_b, max(1 << 26, stride_b)) if self.rows > 1 else 1 << 20)
        up = lambda v: (v + 255) // 256 * 256
        assert 0 <= int(offset) < 256 and int(offset) % self.item == 0
        body = max((self.rows - 1) * stride_b + row_b, int(cover))
        if low_guard is None:
            low_guard = max(guard, 1 << 31) if body >= 1 << 31 else guard
        self.start = up(int(low_guard)) + int(offset)
        self.total = up(self.start + body + up(guard))
        self.dev = torch.full((self.total,), self.sentinel, dtype=torch.uint8, device='cuda')
        assert self.dev.data_ptr() % 256 == 0
        self.parts = [self.start]
        if init is not None:
            self._init(init, 0)

    def _init(self, init, part):
        t = init.to(self.dtype).contiguous().reshape(-1, self.width).cuda()
        r = t.shape[0]
        assert 1 <= r <= self.rows
        full, rem = divmod(self.rows, r)
        self._tiles(r, part).copy_(t.unsqueeze(0).expand(full, r, self.width))
        if rem:
            self._rows(full * r, rem, part).copy_(t[:rem])

    def add(self, shift, init=None):
        """a second operand of the same shape inside the padding of the first, `shift` elements behind it (two operands a GiB stride
        apart in one allocation) -> its part number for view / ptr_of / equals_tiled; read() covers every part"""
        shift = int(shift)
        assert self.rows > 1 and shift * self.item % 16 == 0
        assert all(abs(self.start + shift * self.item - p) >= self.width * self.item for p in self.parts) and shift + self.width <= self.stride
        self.parts.append(self.start + shift * self.item)
        if init is not None:
            self._init(init, len(self.parts) - 1)
        return len(self.parts) - 1

    def _rows(self, first, count, part=0):
        return torch.as_strided(self.dev.view(self.dtype), (count, self.width), (self.stride, 1), self.parts[part] // self.item + first * self.stride)

    def _tiles(self, r, part=0):
        """the first rows // r * r rows as [rows // r][r][width]"""
        return torch.as_strided(self.dev.view(self.dtype), (self.rows // r, r, self.width), (r * self.stride, self.stride, 1), self.parts[part] // self.item)

    def view(self, part=0):
        """the operand in place: [rows][width], strided"""
        return self._rows(0, self.rows, part)

    @property
    def ptr(self):
        return self.ptr_of(0)

    def ptr_of(self, part):
        return C.c_void_p(self.dev.data_ptr() + self.parts[part])

    def equals_tiled(self, block, part=0):
        """row i == block[i % r] for every row, compared on the device a few tiles at a time (block: [r][width], host or device)"""
        t = block.to(self.dtype).reshape(-1, self.width).cuda()
        r = t.shape[0]
        full, rem = divmod(self.rows, r)
        tiles = self._tiles(r, part)
        step = max(1, CHUNK // (r * self.width * self.item))
        ok = torch.ones((), dtype=torch.bool, device='cuda')
        for i in range(0, full, step):
            some = tiles[i: i + step]
            ok &= _same_bits(some, t.unsqueeze(0).expand_as(some))
        if rem:
            ok &= _same_bits(self._rows(full * r, rem, part), t[:rem])
        return bool(ok)

    def read(self, what='', gather=True):
        """-> the operand rows as a dense device tensor [rows][width] (None without `gather`), after the check of the footprint: the rows
        are overwritten with the sentinel on the device, then every byte of the allocation must hold it.  The last use of an arena: its
        buffer is freed."""
        got = self.view().clone(memory_format=torch.contiguous_format) if gather else None
        row_b, stride_b = self.width * self.item, self.stride * self.item
        for p in self.parts:
            torch.as_strided(self.dev, (self.rows, row_b), (stride_b, 1), p).fill_(self.sentinel)
        pattern = int.from_bytes(bytes([self.sentinel]) * 8, 'little', signed=True)
        words = self.dev.view(torch.int64)
        bad = torch.zeros((), dtype=torch.int64, device='cuda')
        for lo in range(0, words.numel(), CHUNK // 8):
            bad += (words[lo: lo + CHUNK // 8] != pattern).sum()
        if int(bad):
            where, count = [], 0
            for lo in range(0, self.total, CHUNK):
                m = self.dev[lo: lo + CHUNK] != self.sentinel
                n = int(m.sum())
                if n and len(where) < 6:
                    first = lo + int(m.to(torch.uint8).argmax())
                    near = torch.nonzero(self.dev[first: first + 4096] != self.sentinel).reshape(-1)[:6 - len(where)].cpu()
                    where += [divmod(first + int(o) - self.start, stride_b) for o in near]
                count += n
            del m, words
            self.free()                       # before the traceback holds this frame: the next case needs the memory
            raise AssertionError('%s: %d bytes outside the result were written; first (row, byte in row): %s' % (what, count, where))
        del words
        self.free()
        return got

    def free(self):
        del self.dev
        torch.cuda.empty_cache()


def _same_bits(a, b):
    """-> 0-d bool tensor on the device; floats are compared as their bits"""
    if a.is_floating_point():
        as_int = {4: torch.int32, 8: torch.int64}[a.element_size()]
        a, b = a.view(as_int), b.contiguous().view(as_int)
    return (a == b).all()


def same_bits(a, b):
    """bit equality of two tensors of one shape and dtype, on whatever device they are"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(_same_bits(a, b.to(a.device)))


def twice(run):
    """run(sentinel) -> dict of result tensors, once per sentinel, one after the other: `run` builds its arenas, checks them
    (BigArena.read) and drops them before it returns, and the allocator's cache is emptied between the runs, so the two never hold
    their buffers at once.  As _arena.twice: a store of the sentinel's own value cannot hide behind both, poisoned padding is read as two
    different values, and the second launch repeats the first bit for bit."""
    torch.cuda.empty_cache()
    a = run(SENTINELS[0])
    torch.cuda.empty_cache()
    b = run(SENTINELS[1])
    torch.cuda.empty_cache()
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), '%s differs between the two runs (poisoned padding read, or not repeatable)' % k
    return a
