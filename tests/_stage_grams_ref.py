"""The stage Grams of ``p2v_code_grams`` / ``p2v_forward_grams`` restated in int64 torch, for the tests (include/p2vit.h, "Stage Grams").

A stage is n samples of rows x cols elements, sample i at + i * sample_stride, row r at + r * row_stride (in elements).
    int8, one scale        v = code                           G[i][j] = sum v_i v_j  (exact integer), unit = the scale
    int8, per-channel s_c  v = code * 2^m_c, m_c = log2(s_c / min s)   G exact integer,  unit = min_c s_c
    fp32                   v = the value                      G in fp64 (the reference of the fp32 kernels), unit = 1
A plain helper module, not a conftest."""
import numpy as np
import torch


def shifts_of(scale):
    """(m_c uint8 [cols], unit) of a per-channel scale vector whose ratios to its minimum are 1, 2, 4 or 8 (PTF)"""
    s = scale.reshape(-1).double()
    unit = float(s.min())
    q = s / unit
    m = torch.log2(q).round()
    assert bool((torch.exp2(m) == q).all()) and float(m.max()) <= 3, 'the scales are not PTF multiples of their minimum'
    return m.to(torch.uint8), unit


def strided(buf, n, rows, cols, sample_stride, row_stride, offset=0):
    """the [n, rows, cols] stage of a flat buffer, walked with the strides"""
    idx = (offset + torch.arange(n, dtype=torch.int64)[:, None, None] * sample_stride
           + torch.arange(rows, dtype=torch.int64)[None, :, None] * row_stride + torch.arange(cols, dtype=torch.int64)[None, None, :])
    return buf.reshape(-1)[idx]


def int_gram(codes, shift=None):
    """int64 [n, n] of integer codes [n, ..., cols]; shift: None or m_c [cols]"""
    n = codes.shape[0]
    v = codes.detach().cpu().to(torch.int64).reshape(n, -1, codes.shape[-1])
    if shift is not None:
        v = v * (torch.ones((), dtype=torch.int64) << shift.cpu().to(torch.int64)).reshape(1, 1, -1)
    v = v.reshape(n, -1)
    return v @ v.t()


def f64_gram(x):
    """(fp64 [n, n] Gram of fp32 values, max_ij sum |x_i| |x_j|: the scale of the fp32 kernels' error bound)"""
    n = x.shape[0]
    v = x.detach().cpu().reshape(n, -1).double()
    return v @ v.t(), float((v.abs() @ v.abs().t()).max())


def dequantised(codes, shift, unit):
    """the values v * unit as fp32, what a hook on the QAct sees up to one rounding per element"""
    n = codes.shape[0]
    v = codes.detach().cpu().double().reshape(n, -1, codes.shape[-1])
    if shift is not None:
        v = v * torch.exp2(shift.cpu().double()).reshape(1, 1, -1)
    return (v * unit).float()


def stage_gram(values, scale, kind):
    """(Gram fp64 [n, n], unit, bound or None) of one stage of ``tests/_float_ops_ref.quant_forward(..., stages=)``: codes under one scale,
    codes under per-channel scales ('per_channel' / 'deq'), or fp32 values"""
    if kind == 'f32':
        g, bound = f64_gram(values)
        return g, 1.0, bound
    if scale is None:
        return int_gram(values).double(), None, None
    m, unit = shifts_of(scale)
    return int_gram(values, m).double(), unit, None


def centre(raw):
    """efficient_CKA._generate_gram_matrix's centring of a raw fp64 Gram [n, n] (the diagonal counts as zero), fp64"""
    g = raw.detach().cpu().double().clone()
    n = g.shape[0]
    g.diagonal().fill_(0)
    means = g.sum(0) / (n - 2)
    means = means - means.sum() / (2 * (n - 1))
    g = g - means.unsqueeze(0)
    g = g - means.unsqueeze(1)
    g.diagonal().fill_(0)
    return g


def assert_exact(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu().double()
    assert got.dtype == torch.float64 and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    assert torch.equal(got, want), (what, 'max |difference| = %g' % float((got - want).abs().max()),
                                    np.argwhere((got != want).numpy())[:4].tolist())
