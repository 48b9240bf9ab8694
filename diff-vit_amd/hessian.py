"""Per-layer Hessian traces that weight the mixed-precision search (test_quant.py:147-191, pyhessian/hessian.py:163-211 of the
reference): ``search.omega_rank`` ranks by Omega = sum_i hessian_i * distance_i, and this module supplies hessian_i.

Hutchinson's estimate: tr(H_ll) = E[v_l^T H_ll v_l] over +-1 vectors v_l, averaged probe by probe until the running mean moves by less
than ``tol`` (:func:`stop_scan`).  The Hessian-vector product is torch's double backward through the float module graph (the model's
backward is autograd's everywhere in this package).  What runs on the HIP engine is everything around it: the
probe vectors of all selected tensors in one launch (``p2v_rademacher_fill``), v . Hv of all of them in two
(``p2v_hutchinson_step``) and every layer's stopping state on the device - the host reads a few bytes once per ``check_every`` probes
instead of one ``.item()`` per tensor and probe.  On CPU tensors the same call runs the host restatements (:func:`rademacher_host`,
fp64 torch sums, :func:`stop_scan`).

Two probe modes.  ``'layer'`` is the reference's loop: one Hessian-vector product per layer and probe, v non-zero on that layer only,
value v_l^T H_ll v_l.  ``'joint'`` draws v over all selected tensors at once and takes ONE product per probe; layer l's value is
v_l^T (H v)_l = v_l^T H_ll v_l + sum_{m != l} v_l^T H_lm v_m.  The cross terms have mean zero (E[v_l v_m^T] = 0 for l != m), so the
estimate of tr(H_ll) stays unbiased at 1 / L of the double backwards; its variance is higher, by the squared Frobenius norms of the
off-diagonal blocks H_lm, so a layer needs more probes to settle and a stopped trace is noisier at equal ``tol``.

One quirk of the reference is NOT reproduced: a layer that converges with a trace of exactly 0.0 is appended twice there
(hessian.py:198-207), which shifts every later layer.  Here every layer yields one entry.
"""
import numpy as np
import torch

from . import engine as E
from .synth import _splitmix64

SKIP_NAMES = ('norm', 'bias', 'cls_token', 'pos_embed', 'patch_embed')      # pyhessian/utils.py:79-85
_U64 = (1 << 64) - 1


# ---- parameter selection -----------------------------------------------------------------------------------------------------------
def select_params(model, select='reference'):
    """(names, params) of the tensors whose traces are estimated.  ``'reference'``: the filter of the reference's ``get_params_grad``
    (pyhessian/utils.py:61-101) - parameters that require grad and whose name holds none of ``SKIP_NAMES``; for ViT / DeiT exactly the
    4 * depth + 1 weights behind ``patch_embed``, in the order of ``global_distance`` and ``bit_config[1:]``.  ``'layers'``: the weights of
    the quantised layers behind the first (``bit_config_names()[1:]`` / ``linear_modules()[1:]``) - for Swin, where the name filter
    would also keep ``relative_position_bias_table``, which is no quantised layer."""
    named = list(model.named_parameters())
    if select == 'reference':
        keep = [(n, p) for n, p in named if p.requires_grad and not any(s in n for s in SKIP_NAMES)]
    elif select == 'layers':
        mods = [m[1] if isinstance(m, tuple) else m for m in model.linear_modules()][1:]
        by_id = {id(p): n for n, p in named}
        keep = [(by_id[id(m.weight)], m.weight) for m in mods]
    else:
        raise ValueError("select is 'reference' or 'layers' (got %r)" % (select,))
    return [n for n, _ in keep], [p for _, p in keep]


# ---- the build-owned generator (include/p2vit.h, "The generator") ---------------------------------------------------------------------
def _u64(v):
    return np.asarray([int(v) & _U64], dtype=np.uint64)


def rademacher_key(seed, layer, probe):
    with np.errstate(over='ignore'):
        return _splitmix64(_splitmix64(_splitmix64(_u64(seed)) ^ _u64(int(layer) & 0xFFFFFFFF)) ^ _u64(probe))


def rademacher_host(seed, layer, probe, n):
    """float32 [n] of +-1: element e is +1 when bit e % 64 of splitmix64(key(seed, layer, probe) + e // 64) is set.  Bit-equal to
    ``p2v_rademacher_fill``; a prefix of a longer draw is the shorter draw."""
    n = int(n)
    with np.errstate(over='ignore'):
        words = _splitmix64(np.arange((n + 63) // 64, dtype=np.uint64) + rademacher_key(seed, layer, probe))
    bits = (words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return (bits.reshape(-1)[:n].astype(np.float32) * 2.0 - 1.0).astype(np.float32)


# ---- the stopping rule (hessian.py:177-209), once ------------------------------------------------------------------------------------
def stop_scan(values, tol):
    """(trace, probes, converged) of one layer's per-probe values.  trace starts at 0; at probe i the mean of values[0 .. i] (a
    sequential fp64 sum in index order, divided by i + 1) is compared with it: ``|mean - trace| / (|trace| + 1e-6) < tol`` stops and
    returns the PREVIOUS prefix mean ``trace`` with probes = i + 1; otherwise trace = mean.  A sequence that never stops returns its
    last mean, all its values consumed.  Values behind the stop index are ignored.  The device (``p2v_hutchinson_step``) performs the
    same operations in the same order: the two are bit-equal."""
    trace, total = 0.0, 0.0
    tol = float(tol)
    i = -1
    for i, v in enumerate(values):
        total = total + float(v)
        mean = total / float(i + 1)
        if abs(mean - trace) / (abs(trace) + 1e-6) < tol:
            return trace, i + 1, True
        trace = mean
    return trace, i + 1, False


def read_state(state):
    """decode the device state of ``p2v_hutchinson_step`` (one copy to the host): dict(running, trace [L], probes [L], done [L],
    converged [L])"""
    raw = state.cpu().numpy().view(np.uint8)
    head = raw[:E.HS_HEADER_BYTES].view(np.int32)
    n = int(head[1])
    lay = raw[E.HS_HEADER_BYTES:E.HS_HEADER_BYTES + n * E.HS_LAYER_BYTES].reshape(n, E.HS_LAYER_BYTES)
    f = np.ascontiguousarray(lay[:, :16]).view(np.float64)
    w = np.ascontiguousarray(lay[:, 16:]).view(np.int32)
    return dict(running=int(head[0]), sum=f[:, 0].copy(), trace=f[:, 1].copy(), probes=w[:, 0].copy(), done=w[:, 1].astype(bool),
                converged=w[:, 2].astype(bool))


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def _forward_logits(model, inputs):
    from .vit import VisionTransformer
    out = model(inputs, hessian_statistic=True) if isinstance(model, VisionTransformer) else model(inputs)
    return out[0] if isinstance(out, (tuple, list)) else out


def _draw(rng, seed, layer, probe, p):
    """probe vector of one tensor on the host-restated paths"""
    if rng == 'counter':
        return torch.from_numpy(rademacher_host(seed, layer, probe, p.numel())).to(device=p.device, dtype=p.dtype).view_as(p)
    if rng == 'torch':                       # the reference's draw (hessian.py:184-190), in its order
        v = torch.randint_like(p, high=2)
        v[v == 0] = -1                       # (a boolean-mask write: a host synchronisation on the GPU, as in the reference)
        return v
    return rng(layer, probe, p).to(device=p.device, dtype=p.dtype).view_as(p)


class _ProbeBuffers:
    """the probe vectors of all selected tensors as views of one fp32 buffer, every view starting on a 16-byte boundary"""

    def __init__(self, params):
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.flat = torch.empty(total, dtype=torch.float32, device=params[0].device)
        self.views = [self.flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, params)]


def hutchinson_traces(model, criterion, inputs, targets, max_iter=150, tol=5e-3, probes='layer', rng='counter', seed=0,
                      select='reference', check_every=8):
    """(names, traces, info): the Hutchinson estimate of tr(H_ll) of ``criterion(model(inputs), targets)`` for every selected weight
    tensor l (:func:`select_params`), with the reference's stopping rule per layer (:func:`stop_scan`).

    The model is put in eval mode and must be in its float state (``ValueError`` when ``model.quant`` is on: rounding has zero gradient,
    and the reference computes this before calibration).  The forward is ``model(inputs, hessian_statistic=True)[0]``; the gradients
    come from ``torch.autograd.grad(loss, params, create_graph=True)``.

    ``probes``: ``'layer'`` - per layer and probe one ``autograd.grad(g_l, p_l, v_l)``, as the reference; ``'joint'`` - one
    ``autograd.grad(grads, params, v)`` per probe with v drawn over all tensors, 1 / L of the double backwards, unbiased, higher variance
    (the off-diagonal blocks H_lm enter as zero-mean noise; see the module text).  Each layer keeps its own stopping state; the loop
    ends when every layer has stopped or at ``max_iter``.
    ``rng``: ``'counter'`` - +-1 from (seed, layer, probe, element), :func:`rademacher_host` / ``p2v_rademacher_fill``, bit-reproducible
    on host and device; ``'torch'`` - ``torch.randint_like(p, high=2)`` with 0 -> -1, the reference's draws under the same
    ``torch.manual_seed``; or a callable ``(layer, probe, param) -> tensor``.
    ``probes='layer'`` with ``rng='torch'`` is the replay that pins the loop to the real reference: layer after layer, each layer's
    probes in a row until it stops, and the reference's arithmetic too - the value is ``torch.sum(Hv * v)`` in the parameter's dtype
    (fp32: up to a few 1e-5 relative off the fp64 sum every other mode takes), read back once per probe, on whatever device the model is
    on.  It exists for that comparison, not for speed or accuracy.
    ``check_every``: the host learns about progress once per that many probes (one small read); probes run past a layer's stop index
    are discarded, so the result does not depend on it.

    ``info``: per layer ``probes`` (values consumed), ``values`` (the per-probe record up to there), ``converged``; plus ``hvps`` (double
    backwards run), ``mode`` and ``device_path``."""
    if probes not in ('layer', 'joint'):
        raise ValueError("probes is 'layer' or 'joint' (got %r)" % (probes,))
    if not (callable(rng) or rng in ('counter', 'torch')):
        raise ValueError("rng is 'counter', 'torch' or a callable (got %r)" % (rng,))
    if int(max_iter) < 1 or int(check_every) < 1:
        raise ValueError('max_iter and check_every are positive')
    if getattr(model, 'quant', False):
        raise ValueError('hutchinson_traces needs the float model: model.quant is on (rounding has zero gradient; the reference computes '
                         'the traces before calibration)')
    max_iter, check_every = int(max_iter), int(check_every)
    model.eval()
    names, params = select_params(model, select)
    if not params:
        raise ValueError('no parameter selected')
    loss = criterion(_forward_logits(model, inputs), targets)
    grads = torch.autograd.grad(loss, params, create_graph=True)
    on_device = params[0].is_cuda
    if on_device and any(p.dtype != torch.float32 or not p.is_contiguous() for p in params):
        raise NotImplementedError('hutchinson_traces on the GPU takes contiguous fp32 parameters (the kernels are fp32)')
    replay = probes == 'layer' and rng == 'torch'
    run = _run_device if on_device and not replay else _run_host
    values, counts, traces, converged, hvps = run(params, grads, max_iter, float(tol), probes, rng, seed, check_every)
    info = dict(names=names, probes=[int(c) for c in counts], values=[[float(x) for x in v[:c]] for v, c in zip(values, counts)],
                converged=[bool(c) for c in converged], hvps=hvps, mode=probes, device_path=run is _run_device)
    return names, [float(t) for t in traces], info


def _sequential_torch(params, grads, max_iter, tol):
    """the reference's loop replayed (hessian.py:171-204): layer after layer, each until it stops, its draws and its arithmetic - the
    value is ``torch.sum(Hv * v)`` in the parameter's dtype with one read per probe, as ``group_product(...).cpu().item()``"""
    values, hvps = [], 0
    for g, p in zip(grads, params):
        vals = []
        for i in range(max_iter):
            v = _draw('torch', 0, 0, i, p)
            hv, = torch.autograd.grad(g, p, grad_outputs=v, retain_graph=True)
            hvps += 1
            vals.append(torch.sum(hv * v).cpu().item())
            if stop_scan(vals, tol)[2]:
                break
        values.append(vals)
    return values, hvps


def _finish_host(values, tol, hvps):
    res = [stop_scan(v, tol) for v in values]
    return values, [r[1] for r in res], [r[0] for r in res], [r[2] for r in res], hvps


def _run_host(params, grads, max_iter, tol, probes, rng, seed, check_every):
    L = len(params)
    if probes == 'layer' and rng == 'torch':
        values, hvps = _sequential_torch(params, grads, max_iter, tol)
        return _finish_host(values, tol, hvps)
    values, done, hvps = [[] for _ in range(L)], [False] * L, 0
    for i in range(max_iter):
        vs = [None if (done[l] and probes == 'layer') else _draw(rng, seed, l, i, p) for l, p in enumerate(params)]
        if probes == 'joint':
            hv = torch.autograd.grad(grads, params, grad_outputs=vs, retain_graph=True)
            hvps += 1
        else:
            hv = [None] * L
            for l in range(L):
                if not done[l]:
                    hv[l], = torch.autograd.grad(grads[l], params[l], grad_outputs=vs[l], retain_graph=True)
                    hvps += 1
        for l in range(L):
            values[l].append(0.0 if hv[l] is None else float((hv[l].double() * vs[l].double()).sum()))
        if (i + 1) % check_every == 0 or i + 1 == max_iter:
            done = [stop_scan(v, tol)[2] for v in values]
            if all(done):
                break
    return _finish_host(values, tol, hvps)


def _run_device(params, grads, max_iter, tol, probes, rng, seed, check_every):
    """the loop on the GPU: per probe one fill launch, the double backward(s), one step (two launches); nothing synchronises except
    the read of the state once per ``check_every`` probes"""
    from . import ops
    L, dev = len(params), params[0].device
    buf = _ProbeBuffers(params)
    layers = list(range(L))
    record = torch.zeros(max_iter, L, dtype=torch.float64, device=dev)
    state = ops.hutchinson_state(L, dev)
    done, hvps, used = [False] * L, 0, 0
    for i in range(max_iter):
        live = [l for l in layers if not (done[l] and probes == 'layer')]
        if rng == 'counter':
            torch.ops.p2vit.rademacher_fill([buf.views[l] for l in live], live, seed, i)
        else:
            for l in live:
                buf.views[l].copy_(_draw(rng, seed, l, i, params[l]))
        if probes == 'joint':
            hv = list(torch.autograd.grad(grads, params, grad_outputs=buf.views, retain_graph=True))
            hvps += 1
        else:
            hv = [buf.views[l] for l in layers]               # a finished layer: any finite pair, the state ignores the value
            for l in live:
                hv[l], = torch.autograd.grad(grads[l], params[l], grad_outputs=buf.views[l], retain_graph=True)
                hvps += 1
        torch.ops.p2vit.hutchinson_step([h.contiguous() for h in hv], buf.views, i, tol, record, state)
        used = i + 1
        if used % check_every == 0 or used == max_iter:
            st = read_state(state)                            # the one read: 16 + 32 L bytes
            done = [bool(d) for d in st['done']]
            if st['running'] == 0:
                break
    st = read_state(state)
    rec = record[:used].cpu().numpy()
    counts = [int(c) for c in st['probes']]
    return [rec[:, l].tolist() for l in range(L)], counts, st['trace'].tolist(), st['converged'].tolist(), hvps


# ---- the search's weights (test_quant.py:171-186) -------------------------------------------------------------------------------------
def normalise_traces(trace_list):
    """per batch |trace|, min-max normalised over the layers, then the mean per layer over the batches"""
    rows = []
    for k, traces in enumerate(trace_list):
        t = [abs(float(x)) for x in traces]
        lo, hi = min(t), max(t)
        if hi == lo:
            raise ValueError('batch %d: every layer has the same |trace| %r: the min-max normalisation divides by zero' % (k, hi))
        rows.append([(x - lo) / (hi - lo) for x in t])
    if not rows:
        raise ValueError('no batch')
    return [sum(r[i] for r in rows) / len(rows) for i in range(len(rows[0]))]


def mean_hessian(model, criterion, batches, **kw):
    """the ``mean_hessian`` vector of the reference's driver (test_quant.py:147-186): :func:`hutchinson_traces` on every (inputs, targets)
    of ``batches``, per batch |trace| min-max normalised over the layers, averaged per layer over the batches.  One entry per selected
    layer, in ``global_distance`` order.  ``ValueError`` for a batch whose traces are all equal (the reference divides by zero)."""
    dev = next(model.parameters()).device
    trace_list = [hutchinson_traces(model, criterion, x.to(dev), y.to(dev), **kw)[1] for x, y in batches]
    return normalise_traces(trace_list)


class hessian:
    """drop-in for ``from pyhessian import hessian`` as test_quant.py:156-161 uses it: ``hessian(model, criterion, data=(inputs,
    labels), cuda=...).trace()`` -> (names, traces).  ``cuda`` true moves the batch to the model's device (the reference's
    ``.cuda()``).  ``dataloader=``, ``eigenvalues`` and ``density`` are not provided."""

    def __init__(self, model, criterion, data=None, cuda=True, **kw):
        if data is None:
            raise ValueError('hessian: pass data=(inputs, targets); dataloader= is not supported')
        self.model, self.criterion, self.kw = model.eval(), criterion, kw
        self.inputs, self.targets = data
        if cuda:
            dev = next(model.parameters()).device
            self.inputs, self.targets = self.inputs.to(dev), self.targets.to(dev)

    def trace(self, maxIter=150, tol=5e-3):
        names, traces, self.info = hutchinson_traces(self.model, self.criterion, self.inputs, self.targets, max_iter=maxIter, tol=tol, **self.kw)
        return names, traces
