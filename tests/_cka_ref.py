"""Host references shared by tests/test_cka.py (which pins them to cka.gram_matrix on the CPU) and tests/test_modeldiff_edges_gpu.py
(which holds the GPU to them bit for bit).  A plain helper module, like _arena.py."""
import numpy as np
import torch


def centre_restatement(x, y=None):
    """k_cka_centre (csrc/p2vit_cka.hip) restated on the host, one fp64 operation at a time and in the kernel's order: the uncentred Gram
    with a zero diagonal, its column sums row by row, / (n - 2), the sum of the means in index order, / (2 (n - 1)), (G - m[j]) - m[i],
    ONE cast to fp32, zero diagonal.  For integer-valued operands whose |x| @ |y|^T stays below 2^24 the Gram and its column sums are
    exact integers in any order, and every later step is a single correctly rounded IEEE operation: the GPU result has to equal this bit
    for bit (tests/test_modeldiff_edges_gpu.py).  -> fp32 [n][n]"""
    X = x.reshape(x.shape[0], -1).double().numpy()
    Y = X if y is None else y.reshape(y.shape[0], -1).double().numpy()
    n = X.shape[0]
    G = X @ Y.T
    np.fill_diagonal(G, 0.0)
    s = np.zeros(n)
    for i in range(n):
        s = s + G[i]
    m = s / float(n - 2)
    c = 0.0
    for k in range(n):
        c = c + float(m[k])
    m = m - c / float(2 * (n - 1))
    out = ((G - m[None, :]) - m[:, None]).astype(np.float32)
    np.fill_diagonal(out, 0.0)
    return torch.from_numpy(out)


def small_integers(seed, shape, bound=3):
    """integer-valued fp32 in [-bound, bound]"""
    return torch.randint(-bound, bound + 1, shape, generator=torch.Generator().manual_seed(seed)).float()
