"""fp64 numpy restatement of the profiling-input search state (include/p2vit.h, p2v_profile_*): what tests/test_profiling_gpu.py compares
the kernels against.  A plain helper module, not a conftest."""
import numpy as np


def cdist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = a[:, None, :] - b[None, :, :]
    return np.sqrt((d * d).sum(-1))


def diversity(o):
    return float(np.mean(cdist(o, o)))


class State:
    """O, O0, D, g per model and the score; ``step`` applies one iteration given the candidates' logits rows [2][classes] per model"""

    def __init__(self, logits1, logits2):
        self.O = [np.array(logits1, dtype=np.float32), np.array(logits2, dtype=np.float32)]
        self.O0 = [o.copy() for o in self.O]
        self.n = self.O[0].shape[0]
        self.refresh()
        self.score = self.value(self.D, self.g)

    def refresh(self):
        self.D = [cdist(o, o) for o in self.O]
        self.g = [np.sqrt(((o.astype(np.float64) - o0.astype(np.float64)) ** 2).sum(1)) for o, o0 in zip(self.O, self.O0)]

    def value(self, D, g):
        n = self.n
        return (g[0].sum() / n) * (g[1].sum() / n) * (D[0].sum() / (n * n)) * (D[1].sum() / (n * n))

    def candidate(self, idx, rows):
        """(D, g, O) of both models with row idx replaced by rows[m]"""
        D, g, O = [], [], []
        for m in range(2):
            o = self.O[m].copy()
            o[idx] = rows[m]
            d = self.D[m].copy()
            r = cdist(o[idx:idx + 1], o)[0]
            r[idx] = 0.0
            d[idx, :] = r
            d[:, idx] = r
            gg = self.g[m].copy()
            gg[idx] = np.sqrt(((o[idx].astype(np.float64) - self.O0[m][idx].astype(np.float64)) ** 2).sum())
            D.append(d); g.append(gg); O.append(o)
        return D, g, O

    def step(self, idx, cand1, cand2):
        """-> (score_right, score_left, decision, score after); commits on acceptance"""
        c = [self.candidate(idx, (cand1[k], cand2[k])) for k in range(2)]
        r, l = self.value(c[0][0], c[0][1]), self.value(c[1][0], c[1][1])
        dec = 0 if (r <= self.score and l <= self.score) else (1 if r > l else 2)
        if dec:
            self.D, self.g, self.O = c[dec - 1]
            self.score = (r, l)[dec - 1]
        return r, l, dec, self.score
