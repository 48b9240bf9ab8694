"""The fp64 restatement of the patch-similarity entropy ("Data-free calibration images"): the value by the formula, the
gradient by autograd on it.  The truth of tests/test_psaq.py and tests/test_psaq_gpu.py; it shares no code with diff_vit_amd.psaq."""
import math

import torch

H_BW = 0.01
C_KDE = 1.0 / math.sqrt(2.0 * math.pi * H_BW * H_BW)
CASES = [(2, 1, 2, 17, 8), (3, 1, 3, 197, 64), (2, 4, 3, 49, 32), (2, 1, 3, 197, 64), (1, 1, 1, 33, 4), (1, 2, 2, 144, 32), (1, 1, 1, 3, 128)]
CORRELATED = 3            # index of the case whose rows share a direction


def case_input(k):
    """the fp32 input of CASES[k] (seeded; the correlated case: a shared row plus 0.6 * noise)"""
    B, G, H, N, hd = CASES[k]
    gen = torch.Generator().manual_seed(1000 + k)
    av = torch.randn(B * G, H, N, hd, generator=gen)
    if k == CORRELATED:
        av = torch.randn(B * G, H, 1, hd, generator=gen) + 0.6 * av
    return av


def similarities(av, groups):
    """S [images, groups, T, T] in av's dtype: rows = head mean without row 0, each divided by max(|row|, 1e-8)"""
    a = av.mean(dim=1)[:, 1:, :]
    ahat = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    s = ahat @ ahat.transpose(-1, -2)
    return s.reshape(av.shape[0] // groups, groups, s.shape[-1], s.shape[-1])


def value_of(av, groups):
    """the value in fp64 (a 0-dim tensor attached to av's graph)"""
    av = av.double()
    s = similarities(av, groups)
    B = s.shape[0]
    lo, hi = s.detach().min(), s.detach().max()
    x = lo + (hi - lo) * torch.arange(10, dtype=torch.float64) / 9.0
    sm = s.reshape(B, 1, -1)
    n = sm.shape[-1]
    p = (C_KDE / n) * torch.exp(-(x.view(1, 10, 1) - sm) ** 2 / (2.0 * H_BW * H_BW)).sum(-1)
    q = p + 1e-4
    f = -q * torch.log(q)
    w = torch.full((10,), 1.0, dtype=torch.float64) * (hi - lo) / 9.0
    w[0] = w[0] / 2
    w[9] = w[9] / 2
    return (f * w).sum(-1).mean()


def value_and_grad(av, groups):
    """(value fp64 0-dim, gradient fp64 like av); images are processed one by one once the range is known, so that the [10, n] terms of
    a 197-token case stay small"""
    av = av.detach().double()
    with torch.no_grad():
        s = similarities(av, groups)
        lo, hi = s.min(), s.max()
    B = av.shape[0] // groups
    x = lo + (hi - lo) * torch.arange(10, dtype=torch.float64) / 9.0
    w = torch.full((10,), 1.0, dtype=torch.float64) * (hi - lo) / 9.0
    w[0] = w[0] / 2
    w[9] = w[9] / 2
    value = torch.zeros((), dtype=torch.float64)
    grad = torch.zeros_like(av)
    for b in range(B):
        leaf = av[b * groups:(b + 1) * groups].clone().requires_grad_(True)
        sm = similarities(leaf, groups).reshape(1, -1)
        p = (C_KDE / sm.shape[-1]) * torch.exp(-(x.view(10, 1) - sm) ** 2 / (2.0 * H_BW * H_BW)).sum(-1)
        q = p + 1e-4
        e = ((-q * torch.log(q)) * w).sum() / B
        grad[b * groups:(b + 1) * groups], = torch.autograd.grad(e, leaf)
        value += e.detach()
    return value, grad


def grad_error(g, g64, groups):
    """per image |g - g64|_2 / |g64|_2, the maximum over the images (None when some image's |g64|_2 is below 1e-6)"""
    B = g64.shape[0] // groups
    d = (g.double() - g64).reshape(B, -1).norm(dim=1)
    n = g64.reshape(B, -1).norm(dim=1)
    if float(n.min()) < 1e-6:
        return None
    return float((d / n).max())


def value_error(v, v64):
    v, v64 = (float(t.detach()) if torch.is_tensor(t) else float(t) for t in (v, v64))
    return abs(v - v64) / abs(v64)
