"""ModelDiff's black-box profiling inputs (Algorithm 1, the search-based generation): the reference's dataset_utility.py:193-302.

    metrics_output_diversity(model, bit_config, inputs, use_torch=False)                         dataset_utility.py:193-207
    gen_profiling_inputs_in_blackbox(model1, model1_bit_config, model2, model2_bit_config,
                                     seed_inputs, use_torch=False, epsilon=0.2,
                                     max_iterations=1000, rng=None, trace=None)                 dataset_utility.py:209-302

With O [n, classes] the logits (fp32, taken in fp64) of a model on the current inputs and O0 those on the seed inputs:

    diversity  = mean over all n^2 ordered pairs (i, j) of sqrt(sum_k (o_ik - o_jk)^2)      np.mean(cdist(O, O)), diagonal included
    divergence = mean_i sqrt(sum_k (o_ik - o0_ik)^2)
    score      = divergence1 * divergence2 * diversity1 * diversity2                          in this order, fp64

Per iteration: ``pos = randint(0, ndims)``, then ``idx = randint(0, n)``; the candidates are the inputs with element ``pos`` of image
``idx`` (C order over [C, H, W]) replaced by ``x + eps`` ("right") and ``x - eps`` ("left"), fp32 additions with ``eps =
np.float32(epsilon)``, no clipping; ``right <= score and left <= score`` keeps the inputs, else ``right > left`` takes right, else left.
The draws do not depend on the results: all (pos, idx) pairs are drawn up front in the reference's interleaved order, from the global
``np.random`` (``rng=None``, as the reference) or from the ``RandomState`` given.

DEVICE LOOP (both models on one GPU): the state of the search lives in one device block (``p2v_profile_*`` in include/p2vit.h).  An
iteration is the candidate builder (one launch), a 2-image forward per model and ``p2v_profile_step`` (two launches) - no ``.item()``,
no copy to the host, no synchronisation between the first and the last iteration.  A fused quant-state model contributes its plan's
forward (``FrozenPlan.forward(..., out=)``, ``SwinPlan.forward``); any other state (float, dequantised, ``-1`` entries) its module graph on
the 2-image batch.  For an engine model a logits row does not depend on the batch it is computed in; for a FLOAT model a row of a
2-image batch can differ from the same row of the full batch in the last ulps (rocBLAS picks its kernels by shape), see DESIGN 8g.

HOST LOOP (everything else, i.e. CPU models): the same algorithm in torch, fp64 scores, full-batch forwards; it prints nothing.

``trace``: a list that receives one row ``[score_right, score_left, decision (0 keep / 1 right / 2 left), score after]`` per iteration.
ViT / DeiT models return the ``(logits, FLOPs, distance)`` triple and take a ``bit_config`` list; Swin models return bare logits and take
``bits`` = 8 | 4 (a list raises ``NotImplementedError``, as everywhere else)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E

__all__ = ['metrics_output_diversity', 'gen_profiling_inputs_in_blackbox', 'draw_mutations', 'diversity', 'divergence']


def _is_swin(model):
    from .swin import SwinTransformer
    return isinstance(model, SwinTransformer)


def _device_of(model):
    p = next(model.parameters(), None)
    return p.device if p is not None else torch.device('cpu')


def _check_swin_bits(model, bit_config):
    if _is_swin(model) and isinstance(bit_config, (list, tuple)):
        raise NotImplementedError('a Swin model has one weight width and no per-layer bit_config list (swin_quant.py:813-817); '
                                  'pass 8, 4 or None')


def _module_logits(model, bit_config, x):
    """the model's own forward: fp32 logits [B, classes]"""
    with torch.no_grad():
        if _is_swin(model):
            out = model(x) if bit_config is None else model(x, int(bit_config))
        else:
            out = model(x, bit_config=bit_config, plot=False)
    out = out[0] if isinstance(out, (tuple, list)) else out
    return out.detach().float().contiguous()


def diversity(logits):
    """mean over all ordered pairs of the Euclidean distance between rows, fp64 (CPU or GPU tensor; the torch restatement)"""
    o = logits.detach().double()
    d = o[:, None, :] - o[None, :, :]
    return torch.sqrt((d * d).sum(-1)).mean()


def divergence(logits, seed_logits):
    d = logits.detach().double() - seed_logits.detach().double()
    return torch.sqrt((d * d).sum(-1)).mean()


def _diversity_gpu(logits):
    """``p2v_profile_diversity`` on fp32 GPU logits [n, classes] -> fp64 device scalar"""
    logits = logits.detach().float().contiguous()
    n, classes = logits.shape
    with torch.cuda.device(logits.device):
        out = torch.empty(1, dtype=torch.float64, device=logits.device)
        ws = torch.empty(n * n, dtype=torch.float64, device=logits.device)
        E.check(E.lib().p2v_profile_diversity(E.ptr(logits), classes, n, classes, E.ptr(out), E.ptr(ws), ws.numel() * 8,
                                              E.stream_ptr(logits.device)))
    return out[0]


def metrics_output_diversity(model, bit_config, inputs, use_torch=False):
    """dataset_utility.py:193-207: the diversity of ``model``'s logits on ``inputs`` as a Python float.  GPU logits go through the HIP
    kernel, CPU logits through the fp64 torch restatement.  (``use_torch`` is accepted and ignored, as in the reference.)"""
    _check_swin_bits(model, bit_config)
    logits = _module_logits(model, bit_config, inputs.to(_device_of(model)))
    return float(_diversity_gpu(logits) if logits.is_cuda else diversity(logits))


def draw_mutations(ndims, n_inputs, max_iterations, rng=None):
    """the (pos, idx) draws of all iterations in the reference's interleaved order (dataset_utility.py:272, 280)"""
    r = np.random if rng is None else rng
    pos, idx = [], []
    for _ in range(max_iterations):
        pos.append(int(r.randint(0, ndims)))
        idx.append(int(r.randint(0, n_inputs)))
    return pos, idx


def _decide(right, left, score):
    if right <= score and left <= score:
        return 0
    return 1 if right > left else 2


def _host_loop(f1, f2, x, eps, pos, idx, trace):
    n = x.shape[0]
    o01, o02 = f1(x), f2(x)

    def evaluate(xs):
        o1, o2 = f1(xs), f2(xs)
        return float(divergence(o1, o01)) * float(divergence(o2, o02)) * float(diversity(o1)) * float(diversity(o2))

    score = evaluate(x)
    eps_t = torch.tensor(eps, dtype=torch.float32, device=x.device)
    for p, i in zip(pos, idx):
        right, left = x.clone(), x.clone()
        right.view(n, -1)[i, p] = x.view(n, -1)[i, p] + eps_t
        left.view(n, -1)[i, p] = x.view(n, -1)[i, p] - eps_t
        sr, sl = evaluate(right), evaluate(left)
        dec = _decide(sr, sl, score)
        if dec == 1:
            x, score = right, sr
        elif dec == 2:
            x, score = left, sl
        if trace is not None:
            trace.append([sr, sl, dec, score])
    return x


def _fused_vit(model, bit_config):
    if bit_config is None or any(int(b) == -1 for b in bit_config):
        return False
    return model._fused() and not model.capture_taps and not any(m._forward_hooks for m in model.linear_modules())


def _fused_swin(model, bit_config):
    return (bit_config is not None and model.quant and all(m.quant and not m.calibrate for m in model._q_modules())
            and not any(m._forward_hooks for _, m in model.linear_modules()))


def _forward_fns(model, bit_config, dev):
    """(full(x) -> logits [B, classes], cand(staging) -> logits [2, classes]) of one model for the device loop"""
    from .vit import VisionTransformer
    if isinstance(model, VisionTransformer) and _fused_vit(model, bit_config):
        bits = [int(b) for b in bit_config]
        if model._plan is None:
            model.freeze(dev)
        plan = model._plan
        buf = torch.empty(2, plan.arch['num_classes'], dtype=torch.float32, device=dev)
        return (lambda x: plan.forward(x, bits)), (lambda s: plan.forward(s, bits, out=buf))
    if _is_swin(model) and _fused_swin(model, bit_config):
        bits = int(bit_config)
        if bits not in (4, 8):
            raise ValueError('%r is not in list' % (bit_config,))
        if model._plan is None or model._plan.bits != bits:
            model.freeze(dev, bits=bits)
        plan = model._plan          # held here: the same module may serve as the other model at the other width
        return (lambda x: plan.forward(x, n_streams=1).contiguous()), (lambda s: plan.forward(s, n_streams=1).contiguous())
    f = lambda x: _module_logits(model, bit_config, x)
    return f, f


def _device_loop(model1, cfg1, model2, cfg2, x, eps, pos, idx, trace, dev):
    L = E.lib()
    if not hasattr(L, 'p2v_profile_step'):
        raise RuntimeError('libp2vit_hip.so has no p2v_profile_* entry points: rebuild it')
    with torch.cuda.device(dev):
        full1, cand1 = _forward_fns(model1, cfg1, dev)
        full2, cand2 = _forward_fns(model2, cfg2, dev)
        n, elems = x.shape[0], x[0].numel()
        o1, o2 = full1(x).float().contiguous(), full2(x).float().contiguous()
        if o1.shape[0] != n or o2.shape[0] != n or o1.shape[1] != o2.shape[1]:
            raise AssertionError('the two models must give [n, classes] logits of one shape, got %s and %s' % (tuple(o1.shape), tuple(o2.shape)))
        classes = o1.shape[1]
        nbytes = L.p2v_profile_state_bytes(n, classes)
        if nbytes == 0:
            raise NotImplementedError('profiling inputs on the device: n = %d, classes = %d are outside the kernels\' limits' % (n, classes))
        state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        staging = torch.empty((2,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
        rows = torch.empty(max(len(pos), 1), 4, dtype=torch.float64, device=dev)
        st = E.stream_ptr(dev)
        E.check(L.p2v_profile_init(E.ptr(state), nbytes, n, classes, E.ptr(o1), E.ptr(o2), st))
        ps, px, pg, pr = E.ptr(state), E.ptr(x), E.ptr(staging), rows.data_ptr()
        for it in range(len(pos)):
            E.check(L.p2v_profile_candidates(px, n, elems, idx[it], pos[it], eps, pg, st))
            c1, c2 = cand1(staging), cand2(staging)
            E.check(L.p2v_profile_step(ps, nbytes, n, classes, E.ptr(c1), E.ptr(c2), pg, px, elems, idx[it], pos[it],
                                       C.c_void_p(pr + 32 * it), st))
        if trace is not None and len(pos):
            trace.extend([r[0], r[1], int(r[2]), r[3]] for r in rows[:len(pos)].cpu().tolist())
    return x


def gen_profiling_inputs_in_blackbox(model1, model1_bit_config, model2, model2_bit_config, seed_inputs, use_torch=False, epsilon=0.2,
                                     max_iterations=1000, rng=None, trace=None):
    """dataset_utility.py:209-302 (module docstring): the final inputs, on the models' device."""
    _check_swin_bits(model1, model1_bit_config)
    _check_swin_bits(model2, model2_bit_config)
    if seed_inputs.dim() < 2 or seed_inputs.shape[0] < 1:
        raise AssertionError('seed_inputs must be a batch [n, ...] of at least one input')
    d1, d2 = _device_of(model1), _device_of(model2)
    n, ndims = seed_inputs.shape[0], int(np.prod(seed_inputs.shape[1:]))
    pos, idx = draw_mutations(ndims, n, int(max_iterations), rng)
    eps = float(np.float32(epsilon))
    x = seed_inputs.detach().to(d1).float().contiguous().clone()
    if d1.type == 'cuda' and d1 == d2:
        return _device_loop(model1, model1_bit_config, model2, model2_bit_config, x, eps, pos, idx, trace, d1)
    f1 = lambda t: _module_logits(model1, model1_bit_config, t.to(d1))
    f2 = lambda t: _module_logits(model2, model2_bit_config, t.to(d2)).to(d1)
    return _host_loop(f1, f2, x, eps, pos, idx, trace)
