"""DDV model diff: ModelDiff's "decision distance vector" per layer (the reference's modeldiff_p2.py), on the fused engine.

    compute_ddv(model, normal_inputs, adv_inputs, bit_config=None, with_linear=True, stages='engine', attention=False)     modeldiff_p2.py:84-116
    similarity(ddv_a, ddv_b)                 per-stage cosine of two DDVs (ModelDiff's metric)
    reference_similarity(ddv_a, ddv_b)       what calculate_and_print_similarities prints    modeldiff_p2.py:118-131
    AttackPGD / gen_adv_inputs(model, inputs, epsilon=0.3, step_size=0.01, num_steps=50)     modeldiff_p2.py:152-194

For every stage (a hooked module) and seed sample the DDV holds the cosine between the stage's activation on the clean input and on
its perturbed twin; the vector over the samples is divided by its L2 norm.  All of it in fp64: cos = dot / (sqrt(aa) sqrt(bb)), 0/0
stays NaN as in numpy.

On a fused model (``model_quant()`` state on a GPU) ``compute_ddv`` makes ONE ``p2v_forward_ddv`` call on the batch [clean; perturbed]:
the int8 codes of qact1, attn.qact1, attn.qact2, Block.qact2, mlp.qact1, Block.qact4 and the final qact2 are reduced in the workspace
between the launches of the forward (exact integer sums; per-channel PTF scales applied in fp64), the logits as fp32, and with
``with_linear`` the outputs of attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 / head through one fp32 tap buffer.  Any other state (a float
model, ``-1`` entries, ``model_dequant()``, a CPU model) runs the module graph with forward hooks on the same-named modules and reduces
through ``torch.ops.p2vit.pair_cosine`` (GPU tensors) or ``pair_cosine_cpu`` (CPU tensors, the plain-torch twin).

Swin models (``swin_stage_names``): ``compute_ddv(swin, x, xa, 8)`` (or 4: Swin's ``bits``, one weight width for the whole model) on a
quant-state GPU model makes ONE ``SwinPlan.forward_ddv`` call - a recorded sequence with a ``P2V_OP_COS`` record behind every launch that
completes a stage and one combine at its end.  Its stages are the QActs of the module graph outside the window kernel - patch_embed's two,
per block qact1 (norm1), attn.qact1, attn.qact3, attn.qact4, qact2, qact3 (norm2), mlp.qact1, mlp.qact2, qact4, per merge qact1 / qact2, the
tail's qact2 / qact3 / act_out - and with ``with_linear`` the fp32 output of every QConv2d / QLinear.  attn.qact4 and mlp.qact2 are the
codes between proj / fc2 and the residual add: the RESID epilogue stores them next to its result.  ``bit_config=None``, a float,
dequantized or CPU Swin hooks the same-named modules (outputs of the window modules, [B * nW, ...], are regrouped per image).  A LIST
``bit_config`` raises ``NotImplementedError`` for a Swin: the reference's Swin has no per-layer widths (swin_quant.py:813-817).

``stages='full'`` (ViT / DeiT; a Swin model's list is already its full one) serves every hook point of the reference's ``add_hooks``
(modeldiff_p2.py:50-82, 10 * depth + 10 keys, ``FULL_REFERENCE_KEYS``): on a fused model still ONE engine call (``p2v_forward_ddv_ex``,
``P2V_DDV_STAGES_FULL``), which adds qact_input (the patch matrix), patch_embed.qact and qact_embed (the mid codes of the EMBED launch),
per block norm1 / norm2 (the LayerNorm's unclamped integer times its out_scale, fp32, from the unfused LayerNorm launch), attn.qact3 /
mlp.qact2 (the mid codes of the RESID launches) and ``norm`` over all rows.  ``qact_pos`` does not depend on the input: its entry is made
here from the plan's calibration - the length-1 vector [1.0], or NaN when every code of the position embedding is zero, as numpy gives in
the reference.  Any other state hooks the same-named modules.

``attention=True`` adds the QActs INSIDE the attention kernels, where P2-ViT quantizes hardest: per ViT / DeiT block
``attn.qact_attn1`` (the int8 score codes) and ``attn.log_int_softmax`` (the output of QIntSoftmax: probabilities 0 and 2^-k, k = 0 ... 15),
in module order between attn.qact1 and attn.qact2; per Swin block ``attn.qact_attn1``, ``attn.qact2`` and ``attn.log_int_softmax`` between
attn.qact1 and attn.qact3.  On a fused model it is still the ONE engine call: the attention launch runs its tapped instantiation, which stores
the score codes and the exponents k of one block into a scratch (``FrozenPlan.ddv_attn_bytes``) that is reduced right behind the launch - the
codes as exact integer sums, the exponents as exact sums of 2^(30 - ka - kb) (``P2V_COS_LOG2K``) - and reused by the next block.  Any other
state hooks the same-named modules (there ``log_int_softmax`` is the module's output, a plain softmax in a float model).  Swin's
``attn.qact_table`` quantizes a parameter, not an activation: it is no stage.

Not covered: DDV
on sliced streams; the FULL stages of an ``input_quant=False`` model on the engine (the reference's own ``add_hooks`` fails there: no
qact_input); and forward hooks of your own on QAct / QIntLayerNorm modules of a fused model - they never fire, because the engine
bypasses the module graph (hooks on QLinear / QConv2d are served, see ``cka``).

``python -m diff_vit_amd.ddv --model deit_small --bits 8 --n 50`` (or ``--model swin_tiny``; ``--bits mixed`` is refused for Swin) prints
the float-vs-quantized similarity per stage on the synthetic data of ``harness`` and writes ``ddv_result/ddv.pkl``; ``--stages full``
prints every hook point of the reference's list, ``--attention`` also the stages inside the attention kernels; ``--no-ptf --no-lis`` diffs the configuration of the reference's modeldiff_p2.py
(``Config(False, False, 'minmax')``: float LayerNorm and float softmax between int8 codes, on the engine; ``attention=True`` is refused
for a quantized ``lis=False`` model).  ``--inputs blackbox
--mut-iters 1000`` takes the perturbed twins from ``profiling.gen_profiling_inputs_in_blackbox`` on (float model, quantized model) instead
of PGD (the default, ``--inputs pgd``)."""
import argparse
import copy
import os
import pickle

import torch
import torch.nn as nn

from . import ops  # noqa: F401  (registers torch.ops.p2vit.*)


def stage_names(depth, with_linear=True, full=False, attention=False):
    """the DDV stages in module order, the one list ``FrozenPlan.forward_ddv`` and the module-graph path share.  ``full``: plus the stages
    behind the reference's remaining hook points (``P2V_DDV_STAGES_FULL``; qact_pos, which no input reaches, is not a stage).
    ``attention``: plus the two QActs inside the attention kernel (``P2V_DDV_STAGES_ATTN``), 2 per block."""
    names = (['qact_input', 'patch_embed.qact', 'qact_embed'] if full else []) + ['qact1']
    for i in range(depth):
        p = 'blocks.%d.' % i
        names += ([p + 'norm1'] if full else []) + ([p + 'attn.qkv'] if with_linear else []) + [p + 'attn.qact1']
        names += ([p + 'attn.qact_attn1', p + 'attn.log_int_softmax'] if attention else []) + [p + 'attn.qact2']
        names += ([p + 'attn.proj'] if with_linear else []) + ([p + 'attn.qact3'] if full else []) + [p + 'qact2']
        names += ([p + 'norm2'] if full else []) + ([p + 'mlp.fc1'] if with_linear else []) + [p + 'mlp.qact1']
        names += ([p + 'mlp.fc2'] if with_linear else []) + ([p + 'mlp.qact2'] if full else []) + [p + 'qact4']
    return names + (['norm'] if full else []) + ['qact2'] + (['head'] if with_linear else []) + ['act_out']


def swin_stage_names(depths, with_linear=True, attention=False):
    """the DDV stages of a Swin model in execution order (a linear layer in front of the QAct that follows it), the one list
    ``SwinPlan.forward_ddv`` and the module-graph path share: 9 per block, 2 per merge, 5 fixed; ``with_linear`` adds 4 per block, 1 per
    merge and 2; ``attention`` the three QActs inside the window kernel, 3 per block."""
    inner = ['attn.qact_attn1', 'attn.qact2', 'attn.log_int_softmax'] if attention else []
    lin = bool(with_linear)
    names = (['patch_embed.proj'] if lin else []) + ['patch_embed.qact_before_norm', 'patch_embed.qact']
    for li, depth in enumerate(depths):
        for bi in range(depth):
            p = 'layers.%d.blocks.%d.' % (li, bi)
            names += [p + 'qact1'] + ([p + 'attn.qkv'] if lin else []) + [p + 'attn.qact1'] + [p + k for k in inner] + [p + 'attn.qact3']
            names += ([p + 'attn.proj'] if lin else []) + [p + 'attn.qact4', p + 'qact2', p + 'qact3']
            names += ([p + 'mlp.fc1'] if lin else []) + [p + 'mlp.qact1'] + ([p + 'mlp.fc2'] if lin else []) + [p + 'mlp.qact2', p + 'qact4']
        if li < len(depths) - 1:
            p = 'layers.%d.downsample.' % li
            names += [p + 'qact1'] + ([p + 'reduction'] if lin else []) + [p + 'qact2']
    return names + ['qact2', 'qact3'] + (['head'] if lin else []) + ['act_out']


def reference_keys(depth, full=False):
    """hook name of modeldiff_p2.add_hooks -> stage name, for the stages both sides have (pos_drop is the identity behind qact1).
    ``full``: all 10 * depth + 10 hook names onto the entries of ``compute_ddv(..., stages='full')`` (the PatchEmbed module returns its
    qact's output: ``patch_embed`` and ``patch_embed_qact`` are one tensor)."""
    keys = {'pos_drop': 'qact1', 'final_qact2': 'qact2', 'head': 'head', 'act_out': 'act_out'}
    per_block = [('attn_qkv', 'attn.qkv'), ('attn_proj', 'attn.proj'), ('qact2', 'qact2'), ('mlp_fc1', 'mlp.fc1'), ('mlp_fc2', 'mlp.fc2'),
                 ('qact4', 'qact4')]
    if full:
        keys.update({'qact_input': 'qact_input', 'patch_embed': 'patch_embed.qact', 'patch_embed_qact': 'patch_embed.qact',
                     'qact_embed': 'qact_embed', 'qact_pos': 'qact_pos', 'final_norm': 'norm'})
        per_block += [('norm1', 'norm1'), ('attn_qact3', 'attn.qact3'), ('norm2', 'norm2'), ('mlp_qact2', 'mlp.qact2')]
    for i in range(depth):
        for ref, ours in per_block:
            keys['block_%d_%s' % (i, ref)] = 'blocks.%d.%s' % (i, ours)
    return keys


REFERENCE_KEYS = reference_keys(24)         # covers every ViT / DeiT depth of the factories; deeper models: reference_keys(depth)
FULL_REFERENCE_KEYS = reference_keys(24, full=True)      # every hook of add_hooks, for compute_ddv(..., stages='full')


def pair_cosine_cpu(a, b, scales=None):
    """the CPU twin of ``torch.ops.p2vit.pair_cosine``: fp64 [stages, n, 3] = (sum a.b, sum a.a, sum b.b) per stage and sample; integer
    codes are summed as int64 (exact), per-channel scales of the last dimension applied as fp64 s_c^2 on per-channel sums."""
    out = []
    scales = scales if scales is not None else [None] * len(a)
    for x, y, sc in zip(a, b, scales):
        n = x.shape[0]
        if not x.dtype.is_floating_point and sc is None:
            x, y = x.reshape(n, -1).to(torch.int64), y.reshape(n, -1).to(torch.int64)
            out.append(torch.stack([(x * y).sum(1), (x * x).sum(1), (y * y).sum(1)], 1).double())
        elif sc is not None:
            C = x.shape[-1]
            x, y = x.reshape(n, -1, C).to(torch.int64), y.reshape(n, -1, C).to(torch.int64)
            s2 = sc.reshape(-1).double() ** 2
            out.append(torch.stack([((x * y).sum(1).double() * s2).sum(1), ((x * x).sum(1).double() * s2).sum(1),
                                    ((y * y).sum(1).double() * s2).sum(1)], 1))
        else:
            x, y = x.reshape(n, -1).double(), y.reshape(n, -1).double()
            out.append(torch.stack([(x * y).sum(1), (x * x).sum(1), (y * y).sum(1)], 1))
    return torch.stack(out)


def cosines(sums):
    """fp64 [..., 3] sums -> cosines dot / (sqrt(aa) sqrt(bb)); an all-zero sample gives 0/0 = NaN, as numpy does in the reference."""
    sums = sums.double()
    return sums[..., 0] / (torch.sqrt(sums[..., 1]) * torch.sqrt(sums[..., 2]))


def ddv_from_sums(sums):
    """[stages, n, 3] -> [stages, n]: the cosines of a stage divided by their L2 norm when it is not zero (modeldiff_p2.py:110-113)."""
    cos = cosines(sums)
    norm = torch.sqrt((cos * cos).sum(-1, keepdim=True))
    return torch.where(norm != 0, cos / norm, cos)


def _device_of(model):
    p = next(model.parameters(), None)
    return p.device if p is not None else torch.device('cpu')


def _graph_forward(model, x, bit_config):
    """the module graph of ``VisionTransformer.forward`` (its branch behind the fused engine), whatever the model's state."""
    FLOPs, gd = [], []
    h = model.forward_features(x, FLOPs, gd, bit_config, False, False)
    return model.act_out(model.head(h, gd, bit_config[-1] if bit_config else None))


def _with_qact_pos(names):
    """the keys of ``compute_ddv(..., stages='full')``: the stages plus qact_pos where the reference's hook fires (behind qact_embed)"""
    k = names.index('qact_embed') + 1
    return names[:k] + ['qact_pos'] + names[k:]


def _qact_pos_ddv(all_zero, device):
    """the reference's DDV of qact_pos: the module runs on the position embedding (batch dimension 1) whatever the input, so the vector has
    one entry, cos(v, v) / |cos(v, v)| = 1 - or 0/0 = NaN when every code is zero"""
    return torch.tensor([float('nan') if all_zero else 1.0], dtype=torch.float64, device=device)


def _hooked_outputs(model, x, bit_config, names, fused_state):
    mods = dict(model.named_modules())
    got, hooks = {}, []
    for nm in names:
        hooks.append(mods[nm].register_forward_hook(lambda m, i, o, nm=nm: got.__setitem__(nm, o.detach())))
    try:
        with torch.no_grad():
            if fused_state:
                _graph_forward(model, x, bit_config)
            else:
                model(x, bit_config=bit_config, plot=False)
    finally:
        for h in hooks:
            h.remove()
    for nm in names:      # a float pass calls F.linear itself for qkv / fc1 (the SmoothQuant branch): their modules' hooks did not fire
        if nm not in got:
            parent, leaf = nm.rsplit('.', 1)
            got[nm] = getattr(mods[parent], leaf + '_output')
    return [got[nm] for nm in names]


def _swin_hooked_outputs(model, x, names):
    """the module graph of a Swin model with forward hooks on the stages' modules; every output as [B, features of the image] (the window
    modules run on [B * nW, ws * ws, C], image-major: a reshape regroups them per image)"""
    mods = dict(model.named_modules())
    got, hooks = {}, []
    for nm in names:
        hooks.append(mods[nm].register_forward_hook(lambda m, i, o, nm=nm: got.__setitem__(nm, o.detach())))
    try:
        with torch.no_grad():
            model.act_out(model.head(model.forward_features(x)))
    finally:
        for h in hooks:
            h.remove()
    return [got[nm].reshape(x.shape[0], -1) for nm in names]


def _compute_ddv_swin(model, x, xa, bit_config, with_linear, attention=False):
    if isinstance(bit_config, (list, tuple)):
        raise NotImplementedError('compute_ddv: a Swin model has one weight width and no per-layer bit_config list '
                                  '(swin_quant.py:813-817); pass 8, 4 or None')
    if attention and bit_config is not None and not model.cfg.INT_SOFTMAX:
        raise NotImplementedError('compute_ddv(attention=True): under Config(lis=False) the quantized softmax is the float one, its '
                                  'probabilities are not codes')
    dev = _device_of(model)
    x, xa = x.to(dev).float(), xa.to(dev).float()
    quant_state = model.quant and all(m.quant and not m.calibrate for m in model._q_modules())
    if bit_config is not None and quant_state and dev.type == 'cuda':
        if int(bit_config) not in (4, 8):
            raise ValueError('%r is not in list' % (bit_config,))
        if model._plan is None or model._plan.bits != int(bit_config):
            model.freeze(dev, bits=int(bit_config))
        _, names, sums = model._plan.forward_ddv(torch.cat((x, xa), 0), with_linear, attention=attention)
        return names, sums
    names = swin_stage_names(model.arch['depths'], with_linear, attention)
    a, b = _swin_hooked_outputs(model, x, names), _swin_hooked_outputs(model, xa, names)
    if dev.type == 'cuda':
        return names, torch.ops.p2vit.pair_cosine(a, b, [None] * len(a))
    return names, pair_cosine_cpu(a, b)


def compute_ddv(model, normal_inputs, adv_inputs, bit_config=None, with_linear=True, stages='engine', attention=False):
    """modeldiff_p2.compute_ddv:84-116 for ``model`` under ``bit_config``: dict stage name -> fp64 tensor [n] (on the model's device).
    ``stages='full'``: every hook point of the reference's list (module docstring); the ``qact_pos`` entry has length 1.
    ``attention``: also the QActs inside the attention kernels (module docstring); False returns exactly the dict without them."""
    attention = bool(attention)
    from .swin import SwinTransformer
    from .vit import VisionTransformer
    if stages not in ('engine', 'full'):
        raise ValueError("compute_ddv: stages must be 'engine' or 'full', not %r" % (stages,))
    full = stages == 'full'
    if not isinstance(model, (SwinTransformer, VisionTransformer)):
        raise NotImplementedError('compute_ddv covers the ViT / DeiT and the Swin models')
    if isinstance(model, SwinTransformer) and isinstance(bit_config, (list, tuple)):
        _compute_ddv_swin(model, normal_inputs, adv_inputs, bit_config, with_linear, attention)       # raises
    if tuple(normal_inputs.shape) != tuple(adv_inputs.shape) or normal_inputs.dim() != 4 or normal_inputs.shape[0] < 1:
        raise AssertionError('compute_ddv: clean and perturbed inputs must be two [n, C, H, W] batches of one shape')
    if isinstance(model, SwinTransformer):
        names, sums = _compute_ddv_swin(model, normal_inputs, adv_inputs, bit_config, with_linear, attention)
        d = ddv_from_sums(sums)
        return {nm: d[k] for k, nm in enumerate(names)}
    if attention and bit_config is not None and not model.cfg.INT_SOFTMAX:
        raise NotImplementedError('compute_ddv(attention=True): under Config(lis=False) the quantized softmax is the float one, its '
                                  'probabilities are not codes')
    dev = _device_of(model)
    x, xa = normal_inputs.to(dev).float(), adv_inputs.to(dev).float()
    has_fp = bit_config is not None and any(int(b) == -1 for b in bit_config)
    fused_state = model._fused()
    if fused_state and not has_fp and dev.type == 'cuda':
        if bit_config is None:
            raise ValueError('None is not in list')              # bit_pool.index(None), vit_fquant.py:282
        if model._plan is None:
            model.freeze(dev)
        _, names, sums = model._plan.forward_ddv(torch.cat((x, xa), 0), [int(b) for b in bit_config], with_linear, stages=stages,
                                                 **({'attention': True} if attention else {}))
        pos = _qact_pos_ddv(model._plan.qact_pos_all_zero, dev) if full else None
    else:
        if full and not getattr(model, 'input_quant', True):
            raise AttributeError("compute_ddv(stages='full'): the model has no qact_input (input_quant=False), as in the reference's add_hooks")
        names = stage_names(model.depth, with_linear, full, attention)
        hooked = _with_qact_pos(names) if full else names
        a = _hooked_outputs(model, x, bit_config, hooked, fused_state)
        b = _hooked_outputs(model, xa, bit_config, hooked, fused_state)
        pos = None
        if full:      # qact_pos ran on the position embedding, batch dimension 1: a pair of its own
            k = hooked.index('qact_pos')
            pa, pb = [a.pop(k)], [b.pop(k)]
            pos = ddv_from_sums(torch.ops.p2vit.pair_cosine(pa, pb, [None]) if dev.type == 'cuda' else pair_cosine_cpu(pa, pb))[0]
        if dev.type == 'cuda':
            sums = torch.ops.p2vit.pair_cosine(a, b, [None] * len(a))
        else:
            sums = pair_cosine_cpu(a, b)
    d = ddv_from_sums(sums)
    out = {nm: d[k] for k, nm in enumerate(names)}
    if full:
        out = {nm: (pos if nm == 'qact_pos' else out[nm]) for nm in _with_qact_pos(names)}
    return out


def similarity(ddv_a, ddv_b):
    """ModelDiff's metric: per stage both DDVs have, the cosine of the two vectors (fp64)."""
    out = {}
    for k in ddv_a:
        if k in ddv_b:
            a, b = ddv_a[k].double().cpu(), ddv_b[k].double().cpu()
            out[k] = float((a * b).sum() / (torch.sqrt((a * a).sum()) * torch.sqrt((b * b).sum())))
    return out


def reference_similarity(ddv_a, ddv_b):
    """what calculate_and_print_similarities:118-131 prints: it walks the two vectors ELEMENT by element, so each "cosine" is the
    product of two signs; the printed number is the mean sign agreement x 100 (a zero entry gives NaN, as there)."""
    out = {}
    for k in ddv_a:
        if k in ddv_b:
            a, b = ddv_a[k].double().cpu(), ddv_b[k].double().cpu()
            out[k] = float(((a / a.abs()) * (b / b.abs()) * 100).mean())
    return out


def _logits(model, x):
    out = model(x)
    return out[0] if isinstance(out, (tuple, list)) else out


def pgd_objective(yhat, y):
    """what the attack maximises: minus the batch mean of the squared error to ``y``, the first logit at full weight and the mean over
    the remaining logits at a tenth (the objective of modeldiff_p2.py:163-164)."""
    sq = (yhat - y).square()
    return -(sq[:, 0] + 0.1 * sq[:, 1:].mean(dim=1)).mean()


class AttackPGD(nn.Module):
    """Projected gradient ascent on ``pgd_objective`` with the semantics of the reference's attack (modeldiff_p2.py:152-178): a uniform
    random start inside the epsilon ball around the inputs, then ``num_steps`` steps of ``step_size`` along the sign of the input
    gradient, each followed by the projection onto the ball and then onto the image range [0, 1].  Kept as a perturbation ``delta``
    around the fixed inputs; torch autograd through the float module graph of ``basic_net``."""

    def __init__(self, basic_net, epsilon, step_size, num_steps):
        super().__init__()
        self.basic_net = basic_net
        self.epsilon, self.step_size, self.num_steps = float(epsilon), float(step_size), int(num_steps)

    def random_start(self, inputs):
        """the starting point: one uniform draw in [-epsilon, epsilon) per element, added to the inputs (not yet clipped to [0, 1])"""
        noise = torch.empty_like(inputs).uniform_(-self.epsilon, self.epsilon)
        return inputs.detach() + noise

    def _project(self, x, inputs):
        delta = (x - inputs).clamp_(-self.epsilon, self.epsilon)
        return (inputs + delta).clamp_(0.0, 1.0)

    def forward(self, inputs, targets):
        inputs = inputs.detach()
        x = self.random_start(inputs)
        for _ in range(self.num_steps):
            probe = x.clone().requires_grad_(True)
            with torch.enable_grad():
                value = pgd_objective(_logits(self.basic_net, probe), targets)
                direction, = torch.autograd.grad(value, probe)
            x = self._project(x.add(direction.sign(), alpha=self.step_size), inputs)
        return x


def pgd_targets(model, inputs):
    """the targets of the attack (modeldiff_p2.py:182-192): every clean output pushed a thousandfold towards the batch mean."""
    model.eval()
    with torch.no_grad():
        clean = _logits(model, inputs)
    return 1000.0 * (clean.mean(dim=0, keepdim=True) - clean)


def gen_adv_inputs(model, inputs, epsilon=0.3, step_size=0.01, num_steps=50):
    """the perturbed twins of ``inputs`` (values in [0, 1]) for a float model: ``AttackPGD`` towards ``pgd_targets``."""
    attack = AttackPGD(model, epsilon, step_size, num_steps)
    return attack(inputs, pgd_targets(model, inputs)).detach()


def main(argv=None):
    from . import harness, synth
    from .config import Config
    p = argparse.ArgumentParser(description='float vs quantized DDV on synthetic data (modeldiff_p2.py)')
    p.add_argument('--model', default='deit_small')
    p.add_argument('--bits', default='8', choices=['8', '4', 'mixed'])
    p.add_argument('--n', default=50, type=int, help='seed samples')
    p.add_argument('--steps', default=50, type=int, help='PGD steps')
    p.add_argument('--stages', default='engine', choices=['engine', 'full'],
                   help='full: every hook point of the reference\'s add_hooks (ViT / DeiT; a Swin list is already its full one)')
    p.add_argument('--attention', action='store_true',
                   help='also the QActs inside the attention kernels: qact_attn1 and the log2 softmax (Swin: and attn.qact2)')
    p.add_argument('--inputs', default='pgd', choices=['pgd', 'blackbox'],
                   help='the perturbed twins: PGD on the float model, or ModelDiff\'s black-box search on (float, quantized)')
    p.add_argument('--mut-iters', default=1000, type=int, help='iterations of the black-box search (--inputs blackbox)')
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--device', default='cuda')
    p.add_argument('--result-name', default='ddv_result')
    p.add_argument('--no-ptf', action='store_true', help='Config(ptf=False): float LayerNorm (ViT / DeiT and Swin)')
    p.add_argument('--no-lis', action='store_true', help='Config(lis=False): float softmax (ViT / DeiT and Swin; not with --attention)')
    p.add_argument('--softmax-bits', default=None, type=int, choices=[3, 4], help='width of the log-int-softmax (Config.BIT_TYPE_S: uint3 / uint4; default 4)')
    args = p.parse_args(argv)
    if args.attention and args.no_lis and args.model.startswith('swin'):      # refused before anything is built
        raise NotImplementedError('--attention --no-lis: under Config(lis=False) the quantized softmax of a Swin model is the float one, '
                                  'its probabilities are not codes')
    device = torch.device(args.device)
    fp = harness.str2model(args.model)(cfg=Config(not args.no_ptf, not args.no_lis, 'minmax').set_softmax_bits(args.softmax_bits))
    is_swin = harness._is_swin(fp)
    if not hasattr(fp, 'arch') or not (is_swin or hasattr(fp, 'depth')):
        raise NotImplementedError('the DDV tool covers the ViT / DeiT and the Swin models')
    if is_swin:
        if args.bits == 'mixed':
            raise NotImplementedError('--bits mixed: a Swin model has one weight width (swin_quant.py:813-817)')
        fp.load_state_dict(synth.swin_state_dict(fp.state_dict(), args.seed))
    else:
        fp.load_state_dict(synth.vit_state_dict(fp.arch, args.seed), strict=False)
    fp = fp.to(device).eval()
    q = copy.deepcopy(fp)
    harness.calibrate_model(q, synth.images(args.seed + 1, 10, fp.arch['img_size']).to(device))
    if is_swin:
        bits = int(args.bits)
    else:
        L = 4 * fp.depth + 2
        bits = {'8': [8] * L, '4': [4] * L, 'mixed': [8 if (i * 7 + 3) % 5 < 3 else 4 for i in range(L)]}[args.bits]
    x = synth.images(args.seed + 2, args.n, fp.arch['img_size']).to(device)
    x = (x - x.amin()) / (x.amax() - x.amin())                      # the attack works on images in [0, 1]
    if args.inputs == 'blackbox':
        import numpy as np
        from . import profiling
        adv = profiling.gen_profiling_inputs_in_blackbox(fp, None, q, bits, x, max_iterations=args.mut_iters,
                                                         rng=np.random.RandomState(args.seed))
    else:
        torch.manual_seed(args.seed)
        adv = gen_adv_inputs(fp, x, num_steps=args.steps)
    d_fp = compute_ddv(fp, x, adv, None, stages=args.stages, attention=args.attention)
    d_q = compute_ddv(q, x, adv, bits, stages=args.stages, attention=args.attention)
    sim, ref = similarity(d_fp, d_q), reference_similarity(d_fp, d_q)
    for k in d_fp:
        print('%-24s cosine %+.6f   sign agreement %.2f%%' % (k, sim[k], ref[k]))
    os.makedirs(args.result_name, exist_ok=True)
    path = os.path.join(args.result_name, 'ddv.pkl')
    with open(path, 'wb') as f:
        pickle.dump({'float': {k: v.cpu().numpy() for k, v in d_fp.items()}, 'quantized': {k: v.cpu().numpy() for k, v in d_q.items()},
                     'similarity': sim, 'reference_similarity': ref, 'bits': bits}, f)
    print('%d stages, %d samples -> %s' % (len(d_fp), args.n, path))
    return sim


if __name__ == '__main__':
    main()
