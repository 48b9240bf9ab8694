"""The record of the stage statistics (include/p2vit.h, p2v_code_stats) restated in numpy for the tests: int64 arithmetic, the
sign-magnitude key for the fp32 order, exponent-field bins.

    record(x)          x [..., cols] int8 / uint8 / float32 -> dict(hist, count, nonfinite, lo, hi, sum, sumsq), reduced over everything
                       but the last dimension
    merge(a, b)        the record of both data sets
    same(got, want)    field by field, bit for bit (fp32 extrema by their bits: -0 and +0 differ)
"""
import numpy as np

FIELDS = ('hist', 'count', 'nonfinite', 'lo', 'hi', 'sum', 'sumsq')
INT_MAX, INT_MIN = np.int32(2 ** 31 - 1), np.int32(-2 ** 31)


def key(bits):
    """fp32 bits as int32 -> the int32 whose signed order is the total order of the values (-0 < +0); its own inverse"""
    bits = np.asarray(bits, dtype=np.int32)
    return bits ^ ((bits >> 31) & np.int32(0x7fffffff))


def record(x):
    x = np.asarray(x)
    cols = x.shape[-1]
    x = x.reshape(-1, cols)
    out = dict(count=np.int64(x.size), nonfinite=np.zeros(3, np.int64), sum=np.zeros(cols, np.int64), sumsq=np.zeros(cols, np.int64))
    if x.dtype == np.float32:
        bits = np.ascontiguousarray(x).view(np.int32)
        e = (bits >> 23) & 255
        frac = bits & 0x7fffff
        out['hist'] = np.bincount(e.reshape(-1), minlength=256).astype(np.int64)
        out['nonfinite'] = np.array([((e == 255) & (frac != 0)).sum(), ((e == 255) & (frac == 0) & (bits >= 0)).sum(),
                                     ((e == 255) & (frac == 0) & (bits < 0)).sum()], np.int64)
        k, fin = key(bits), e != 255
        lo = np.where(fin, k, INT_MAX).min(0, initial=INT_MAX)
        hi = np.where(fin, k, INT_MIN).max(0, initial=INT_MIN)
        some = fin.any(0) if x.shape[0] else np.zeros(cols, bool)
        out['lo'] = np.where(some, key(lo), np.int32(0x7f800000)).astype(np.int32).view(np.float32)
        out['hi'] = np.where(some, key(hi), np.int32(-0x00800000)).astype(np.int32).view(np.float32)           # 0xff800000 = -Inf
        return out
    assert x.dtype in (np.int8, np.uint8), x.dtype
    v = x.astype(np.int64)
    out['hist'] = np.bincount((v + (128 if x.dtype == np.int8 else 0)).reshape(-1), minlength=256).astype(np.int64)
    out['lo'] = v.min(0, initial=int(INT_MAX)).astype(np.int32)
    out['hi'] = v.max(0, initial=int(INT_MIN)).astype(np.int32)
    out['sum'] = v.sum(0, dtype=np.int64)
    out['sumsq'] = (v * v).sum(0, dtype=np.int64)
    return out


def merge(a, b):
    out = {f: a[f] + b[f] for f in ('hist', 'count', 'nonfinite', 'sum', 'sumsq')}
    if a['lo'].dtype == np.float32:
        out['lo'] = key(np.minimum(key(a['lo'].view(np.int32)), key(b['lo'].view(np.int32)))).view(np.float32)
        out['hi'] = key(np.maximum(key(a['hi'].view(np.int32)), key(b['hi'].view(np.int32)))).view(np.float32)
    else:
        out['lo'], out['hi'] = np.minimum(a['lo'], b['lo']), np.maximum(a['hi'], b['hi'])
    return out


def fields_of(rec):
    """a record of ``StageStats.record`` (torch views) as numpy arrays"""
    return {f: np.asarray(rec[f].detach().cpu().numpy()) for f in FIELDS}


def same(got, want, what=''):
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        if w.dtype == np.float32:
            assert g.dtype == np.float32, (what, f, g.dtype)
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.nonzero(np.atleast_1d(g != w))[0]
        assert bad.size == 0, (what, f, 'first of %d' % bad.size, int(bad[0]), np.atleast_1d(g)[bad[0]], np.atleast_1d(w)[bad[0]])


def parse(raw, cols, f32):
    """the bytes of one record (uint8 numpy, p2v_stats_bytes(cols) of them) -> its fields"""
    raw = np.ascontiguousarray(raw)
    head = raw[:2080].view(np.int64)
    ext = np.float32 if f32 else np.int32
    return dict(hist=head[:256].copy(), count=head[256].copy(), nonfinite=head[257:260].copy(),
                lo=raw[2080:2080 + 4 * cols].view(ext).copy(), hi=raw[2080 + 4 * cols:2080 + 8 * cols].view(ext).copy(),
                sum=raw[2080 + 8 * cols:2080 + 16 * cols].view(np.int64).copy(), sumsq=raw[2080 + 16 * cols:2080 + 24 * cols].view(np.int64).copy())


def record_bytes(cols):
    return (2080 + 24 * cols + 15) // 16 * 16
