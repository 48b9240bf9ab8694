"""Scoring of the logits with a defined tie rule: Prec@k and the cross-entropy loss of ``harness.validate`` (test_quant.py:430-439,
488-501) without a host synchronisation per batch.

The logits of this engine are 8-bit codes times a power of two: 1000 classes share some 80 - 180 distinct values, and ties at the top-1 or
top-5 boundary are common.  ``torch.topk`` leaves their order undefined, so the reference's Prec@k depends on the
platform.  Here, among equal logits the LOWER CLASS INDEX RANKS FIRST, and every result also carries the bracket [sure, possible] that any
tie order must land in.

Per row (``score_rows_reference``, and ``torch.ops.p2vit.score_logits`` on the GPU), with y the label and x the row:
    gt = #{j : x_j > x_y}    eq_lo = #{j < y : x_j == x_y}    eq_hi = #{j > y : x_j == x_y}    argmax = lowest index of the maximum
    loss = log(sum_j exp((double)x_j - m)) + m - (double)x_y,  m = max_j x_j, in fp64
A label outside [0, classes) (``ignore_index = -100`` included) makes the row invalid: gt = -1, eq_lo = eq_hi = 0, loss = 0.
Per k:  hit = gt + eq_lo < k   sure = gt + eq_lo + eq_hi < k   possible = gt < k.
"""
import numpy as np
import torch


def score_rows_reference(logits, labels):
    """numpy restatement of the record definition above (the CPU path, and what the GPU tests compare against):
    (ranks int32 [rows, 4] = gt, eq_lo, eq_hi, argmax; loss float64 [rows])."""
    x = np.ascontiguousarray(logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else logits, dtype=np.float32)
    y = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels, dtype=np.int64).reshape(-1)
    rows, classes = x.shape
    assert y.shape[0] == rows and classes >= 1
    valid = (y >= 0) & (y < classes)
    yc = np.where(valid, y, 0)
    xy = x[np.arange(rows), yc]
    j = np.arange(classes, dtype=np.int64)[None, :]
    eq = x == xy[:, None]
    ranks = np.zeros((rows, 4), dtype=np.int32)
    ranks[:, 0] = np.where(valid, (x > xy[:, None]).sum(1), -1)
    ranks[:, 1] = np.where(valid, (eq & (j < yc[:, None])).sum(1), 0)
    ranks[:, 2] = np.where(valid, (eq & (j > yc[:, None])).sum(1), 0)
    ranks[:, 3] = x.argmax(1) if rows else 0               # numpy: the first occurrence of the maximum
    xd = x.astype(np.float64)
    m = xd.max(1) if rows else np.zeros(0)
    loss = np.log(np.exp(xd - m[:, None]).sum(1)) + m - xy.astype(np.float64)
    return ranks, np.where(valid, loss, 0.0)


class DeviceMeter:
    """Running totals of a validation pass, ``slots`` independent sets of them (one per configuration of ``harness.validate_many``).

    ``update`` enqueues the two score kernels on the current stream for CUDA tensors and never synchronises; CPU tensors go through
    ``score_rows_reference``.  ``result`` is the one host read.  The totals are one int64 tensor [slots, 3 + 3 * len(ks)] on the device
    of the first update: n, invalid, hit[k], sure[k], possible[k] and, in the last column, the bits of the fp64 loss sum."""

    def __init__(self, ks=(1, 5), slots=1, device=None):
        self.ks = tuple(int(k) for k in ks)
        if not 1 <= len(self.ks) <= 8 or min(self.ks) < 1:
            raise ValueError('DeviceMeter: 1 to 8 values of k, each >= 1 (got %r)' % (ks,))
        if slots < 1:
            raise ValueError('DeviceMeter: at least one slot')
        self.slots = int(slots)
        self.totals = None
        if device is not None:
            self._alloc(torch.device(device))

    def _alloc(self, device):
        self.totals = torch.zeros(self.slots, 3 + 3 * len(self.ks), dtype=torch.int64, device=device)

    def reset(self):
        if self.totals is not None:
            self.totals.zero_()

    def update(self, logits, target, slot=0):
        if not 0 <= slot < self.slots:
            raise IndexError('DeviceMeter: slot %d of %d' % (slot, self.slots))
        if self.totals is None:
            self._alloc(logits.device)
        if logits.device != self.totals.device:
            raise ValueError('DeviceMeter: logits on %s, totals on %s' % (logits.device, self.totals.device))
        if logits.is_cuda:
            ranks, loss = torch.ops.p2vit.score_logits(logits, target.to(logits.device))
            torch.ops.p2vit.score_accumulate(ranks, loss, list(self.ks), self.totals[slot])
            return
        ranks, loss = score_rows_reference(logits, target)
        ok = ranks[:, 0] >= 0
        gt, lo, hi = (ranks[ok, c].astype(np.int64) for c in range(3))
        add = [int(ok.sum()), int((~ok).sum())]
        add += [int((gt + lo < k).sum()) for k in self.ks] + [int((gt + lo + hi < k).sum()) for k in self.ks] + [int((gt < k).sum()) for k in self.ks]
        t = self.totals[slot].numpy()                      # shares memory with the tensor
        t[:-1] += np.asarray(add, dtype=np.int64)
        t[-1:].view(np.float64)[0] += loss[ok].sum()

    def result(self, slot=0):
        """{'n', 'invalid', 'loss', 'prec': {k: %}, 'sure': {k: %}, 'possible': {k: %}}: percentages and the mean loss over the valid
        rows (0.0 when there are none).  Synchronises with the device: the one host read of a pass."""
        nk = len(self.ks)
        if self.totals is None:
            t = np.zeros(3 + 3 * nk, dtype=np.int64)
        else:
            t = self.totals[slot].cpu().numpy()
        n = int(t[0])
        pct = lambda v: 100.0 * int(v) / n if n else 0.0
        return {'n': n, 'invalid': int(t[1]), 'loss': float(t[-1:].view(np.float64)[0]) / n if n else 0.0,
                'prec': {k: pct(t[2 + q]) for q, k in enumerate(self.ks)},
                'sure': {k: pct(t[2 + nk + q]) for q, k in enumerate(self.ks)},
                'possible': {k: pct(t[2 + 2 * nk + q]) for q, k in enumerate(self.ks)}}

    def all_reduce(self, group=None):
        """sum the totals of every slot across the ranks of ``group``: an int64 all-reduce for the counters and an fp64 one for the loss
        sums (gloo for CPU totals, RCCL for GPU totals)."""
        import torch.distributed as dist
        if self.totals is None:
            raise RuntimeError('DeviceMeter.all_reduce: no totals yet (pass device= or update first)')
        counters = self.totals[:, :-1].contiguous()
        loss = self.totals[:, -1:].contiguous().view(torch.float64)
        dist.all_reduce(counters, group=group)
        dist.all_reduce(loss, group=group)
        self.totals[:, :-1] = counters
        self.totals[:, -1:] = loss.view(torch.int64)
