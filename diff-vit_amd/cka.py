"""CKA model diff: layer-wise similarity heat maps between two models (the reference's own analysis, cka_utility.py, efficient_CKA.py,
DDV_CKA.py), on the fused engine.

    get_activations(images, model, bit_config, device, normalize_act=False, layer_indices=None)     cka_utility.py:26-113
    MinibatchCKA(num_layers, num_layers2=None, across_models=False, dtype=torch.float32)           efficient_CKA.py
    MinibatchAdvCKA(...)                                                                            DDV_CKA.py
    compute_cka(model1, model2, batches, bit_config1, bit_config2, normalize_act=False)           float vs quantized heat map
    get_stage_grams(images, model, bit_config, device, stages='engine', with_linear=False)         centred Grams over the DDV stage list
    compute_cka(..., stages='engine' | 'full', with_linear=False)                                 the heat map over the two stage lists

On a fused model (``model_quant()`` state) ``get_activations`` makes ONE ``p2v_forward_linear_taps`` call: its forward hooks on
QConv2d / QLinear are fed by the engine (``VisionTransformer._forward_hooked``).  A Swin model is called with its own signature
(``bit_config`` None, 8 or 4 = Swin's ``bits``; a list is refused): in quant state one ``SwinPlan.forward_linear_taps`` replay feeds the
hooks (``SwinTransformer._forward_hooked``) with [B, tokens, N] outputs in natural token order - the module graph would give qkv / proj in
window order, a permutation of an image's features that a Gram matrix does not see.  Otherwise (float model, ``-1`` entries, dequant) the
module graph runs with the hooks, as in the reference.  The CKA classes send GPU activations through the HIP kernels
(``torch.ops.p2vit.cka_grams`` / ``hsic_accumulate``: one grouped Gram launch sequence for all layers of an update) and CPU
activations through ``gram_matrix``, a plain-torch restatement of the same formula.

With ``stages`` the heat map runs over ``ddv.stage_names`` instead of the linear layers - the QAct stages (block inputs, attention and
GELU outputs, the residual streams) included, where the quantization happens.  On a fused GPU model ``get_stage_grams`` makes ONE
``p2v_forward_grams`` call: every int8 stage's Gram is an exact integer contraction of its live codes on the int8 MFMA
(``p2v_code_grams``; per-channel stages as code * 2^m_c in units of the smallest scale, which CKA does not see), no fp32 tap is written
for them, and ``torch.ops.p2vit.cka_centre`` applies the centring.  Any other state runs the module graph with hooks on the same names
(``ddv._hooked_outputs``) and the fp32 Gram path above.  A Swin model and the attention stages are refused with ``stages``.

``python -m diff_vit_amd.cka --model deit_small --bits 8 --batch 50 --iters 2`` (``--stages engine|full`` and ``--with-linear`` for the
stage lists; then ``_names.pkl`` holds the two name lists) (or ``--model swin_tiny``; ``--bits mixed`` is refused
for Swin) writes ``<result-name>/_heatmap.pkl`` (float vs
quantized on the synthetic data of ``harness``)."""
import argparse
import copy
import os
import pickle

import torch

from . import ops  # noqa: F401  (registers torch.ops.p2vit.*)
from .ptq import QConv2d, QLinear
from .vit import Attention, Mlp


def normalize_activations(act):
    """cka_utility.py:6-21 (reshape instead of view: the patch-embed tap of the engine is a permuted view)."""
    act = act.reshape(act.size(0), -1)
    return act / (torch.norm(act, p=2, dim=1, keepdim=True) + 1e-8)


def get_activations(images, model, bit_config, device, normalize_act=False, layer_indices=None):
    """cka_utility.py:26-113: the outputs of every QConv2d / QLinear (and, without a bit_config, Attention.qkv_output /
    Mlp.fc1_output) in named_modules order.  Returns the list, or (list, layer_info) when ``layer_indices`` is given."""
    from .swin import SwinTransformer
    is_swin = isinstance(model, SwinTransformer)
    model = model.to(device)
    activations, layer_info, hooks = [], [], []

    def hook_return(index, name):
        def hook(module, input, output):
            if isinstance(module, Attention):
                activations.append(module.qkv_output)
            elif isinstance(module, Mlp):
                activations.append(module.fc1_output)
            elif is_swin and output.dim() == 3 and output.shape[0] != images.shape[0]:
                # the window modules of the module graph run on [B * nW, ws * ws, N], image-major: one row of features per image again
                activations.append(output.reshape(images.shape[0], -1, output.shape[-1]))
            else:
                activations.append(output)
            layer_info.append({'relative_index': len(layer_info), 'absolute_index': index, 'name': name, 'layer_type': type(module),
                               'path': '%s.%s' % (type(module).__module__, type(module).__name__)})
        return hook

    if is_swin and isinstance(bit_config, (list, tuple)):
        raise NotImplementedError('get_activations: a Swin model has one weight width and no per-layer bit_config list; pass 8, 4 or None')
    # (a Swin has no Attention / Mlp taps: its float pass calls every QLinear as a module, so the hooks on them fire)
    kinds = (QConv2d, QLinear, Attention, Mlp) if bit_config is None and not is_swin else (QConv2d, QLinear)
    for index, (name, layer) in enumerate(model.named_modules()):
        if type(layer) in kinds:
            hooks.append(layer.register_forward_hook(hook_return(index, name)))
    try:
        with torch.no_grad():
            if is_swin:                                  # SwinTransformer.forward(x, bits): 8 when no width is named
                model(images.to(device), bits=8 if bit_config is None else int(bit_config))
            else:
                model(images.to(device), bit_config=bit_config, plot=False)
    finally:
        for h in hooks:
            h.remove()
    order = sorted(range(len(layer_info)), key=lambda k: layer_info[k]['absolute_index'])
    layer_info = [layer_info[i] for i in order]
    activations = [activations[i] for i in order]
    for i, info in enumerate(layer_info):
        info['relative_index'] = i
    if layer_indices is not None:
        keep = [i for i, info in enumerate(layer_info) if info['relative_index'] == layer_indices]
        activations = [activations[i] for i in keep]
        layer_info = [layer_info[i] for i in keep]
    if normalize_act:
        activations = [normalize_activations(a) for a in activations]
    if layer_indices is None:
        return activations
    return activations, layer_info


def gram_matrix(x, y=None, dtype=torch.float32):
    """efficient_CKA.py:23-39 / DDV_CKA.py:20-39 in plain torch: the centred Gram matrix of one layer, flattened to n*n."""
    x = x.reshape(x.size(0), -1)
    gram = x @ (x if y is None else y.reshape(y.size(0), -1)).t()
    n = gram.size(0)
    gram.diagonal().fill_(0)
    gram = gram.to(dtype)
    means = gram.sum(0) / (n - 2)
    means -= means.sum() / (2 * (n - 1))
    gram -= means.unsqueeze(0)
    gram -= means.unsqueeze(1)
    gram.diagonal().fill_(0)
    return gram.reshape(-1)


def _grams(xs, ys, dtype):
    """centred grams: [L, n, n] from the HIP kernels for GPU tensors, [L, n*n] from the restatement for CPU tensors."""
    if xs[0].is_cuda:
        return torch.ops.p2vit.cka_grams(list(xs), list(ys) if ys is not None else [])
    return torch.stack([gram_matrix(x, None if ys is None else y, dtype) for x, y in zip(xs, ys if ys is not None else xs)])


class MinibatchCKA:
    """efficient_CKA.MinibatchCKA: unbiased-HSIC CKA accumulated over minibatches.  The accumulators live on the device of the first
    update (the reference hard-codes .cuda())."""

    def __init__(self, num_layers, num_layers2=None, across_models=False, dtype=torch.float32):
        if num_layers2 is None:
            num_layers2 = num_layers
        self.dtype = dtype
        self.across_models = across_models
        self.hsic_accumulator = torch.zeros((num_layers, num_layers2), dtype=dtype)
        self.hsic_accumulator_model1 = torch.zeros((num_layers,), dtype=dtype)
        self.hsic_accumulator_model2 = torch.zeros((num_layers2,), dtype=dtype)
        self._device = None

    def _to(self, device):
        if self._device is None:
            self._device = device
            self.hsic_accumulator = self.hsic_accumulator.to(device)
            self.hsic_accumulator_model1 = self.hsic_accumulator_model1.to(device)
            self.hsic_accumulator_model2 = self.hsic_accumulator_model2.to(device)
        elif device != self._device:
            raise AssertionError('activations on %s, accumulators on %s' % (device, self._device))

    def _accumulate(self, g1, g2, self_terms):
        self._to(g1.device)
        if g1.is_cuda:
            torch.ops.p2vit.hsic_accumulate(g1, g2, self.hsic_accumulator, self.hsic_accumulator_model1 if self_terms else None,
                                            self.hsic_accumulator_model2 if self_terms else None)
            return
        self.hsic_accumulator.add_(g1 @ g2.t())
        if self_terms:
            self.hsic_accumulator_model1.add_(torch.einsum('ij,ij->i', g1, g1))
            self.hsic_accumulator_model2.add_(torch.einsum('ij,ij->i', g2, g2))

    def update_state(self, activations):
        g = _grams(activations, None, self.dtype)
        self._accumulate(g, g, False)

    def update_state_across_models(self, activations1, activations2):
        assert self.hsic_accumulator.size(0) == len(activations1), 'Number of activation vectors does not match num_layers.'
        assert self.hsic_accumulator.size(1) == len(activations2), 'Number of activation vectors does not match num_layers.'
        self._accumulate(_grams(activations1, None, self.dtype), _grams(activations2, None, self.dtype), True)

    def _flat(self, g):
        """centred Grams as ``_accumulate`` takes them: [L, n, n] on the GPU, [L, n*n] on the CPU"""
        g = g.to(torch.float32 if g.is_cuda else self.dtype)
        return g if g.is_cuda else g.reshape(g.shape[0], -1)

    def update_state_grams(self, g):
        """``update_state`` on centred Grams [L, n, n] (``get_stage_grams``) instead of activations"""
        g = self._flat(g)
        self._accumulate(g, g, False)

    def update_state_across_models_grams(self, g1, g2):
        """``update_state_across_models`` on the centred Grams of the two models"""
        assert self.hsic_accumulator.size(0) == g1.shape[0], 'Number of Gram matrices does not match num_layers.'
        assert self.hsic_accumulator.size(1) == g2.shape[0], 'Number of Gram matrices does not match num_layers.'
        self._accumulate(self._flat(g1), self._flat(g2), True)

    def result(self):
        mean_hsic = self.hsic_accumulator
        if self.across_models:
            mean_hsic = mean_hsic / torch.sqrt(self.hsic_accumulator_model1).unsqueeze(1)
            return mean_hsic / torch.sqrt(self.hsic_accumulator_model2).unsqueeze(0)
        norm = torch.sqrt(mean_hsic.diagonal())
        return mean_hsic / norm.unsqueeze(1) / norm.unsqueeze(0)


class MinibatchAdvCKA(MinibatchCKA):
    """DDV_CKA.MinibatchAdvCKA: grams of X (adv X)^T per model; the result is always normalised by the two self terms."""

    def update_state(self, model1_activations, model1_adv_activations, model2_activations, model2_adv_activations):
        g1 = _grams(model1_activations, model1_adv_activations, self.dtype)
        g2 = _grams(model2_activations, model2_adv_activations, self.dtype)
        self._accumulate(g1, g2, True)

    def update_state_grams(self, g1, g2):
        """``update_state`` on centred X X_adv^T Grams [L, n, n] of the two models - e.g. ``torch.ops.p2vit.cka_centre`` of the
        off-diagonal blocks ``raw[:, :n, n:]`` of the raw Grams of a batch [clean; perturbed]"""
        self._accumulate(self._flat(g1), self._flat(g2), True)

    def update_state_across_models_grams(self, g1, g2):
        self.update_state_grams(g1, g2)

    def result(self):
        mean_hsic = self.hsic_accumulator / torch.sqrt(self.hsic_accumulator_model1).unsqueeze(1)
        return mean_hsic / torch.sqrt(self.hsic_accumulator_model2).unsqueeze(0)


def _device_of(model):
    p = next(model.parameters(), None)
    return p.device if p is not None else torch.device('cpu')


def _check_stages(model, stages):
    from .swin import SwinTransformer
    from .vit import VisionTransformer
    if stages not in ('engine', 'full'):
        if stages in ('attention', 'attn'):
            raise NotImplementedError('CKA over the stages inside the attention kernels is not served: the log2 exponent planes are no '
                                      'byte codes the Gram kernel takes')
        raise ValueError("stages must be None, 'engine' or 'full', not %r" % (stages,))
    if isinstance(model, SwinTransformer):
        raise NotImplementedError('CKA over the DDV stage list covers the ViT / DeiT models: the Swin plan has no Gram entry point yet; '
                                  'use stages=None (the linear layers)')
    if not isinstance(model, VisionTransformer):
        raise NotImplementedError('CKA over the DDV stage list covers the ViT / DeiT models')


def get_stage_grams(images, model, bit_config, device, stages='engine', with_linear=False, attention=False, dtype=torch.float32):
    """(names, centred Grams [S, n, n]) of ``model`` under ``bit_config`` over ``ddv.stage_names(depth, with_linear, stages == 'full')``.
    A fused model on a GPU makes ONE ``FrozenPlan.forward_grams`` call plus ``cka_centre`` (fp32 Grams); any other state (float model,
    ``-1`` entries, dequant, CPU) takes the outputs of forward hooks on the same names through ``_grams``."""
    from .ddv import _hooked_outputs, stage_names
    if attention:
        raise NotImplementedError('CKA over the stages inside the attention kernels is not served: the log2 exponent planes are no byte '
                                  'codes the Gram kernel takes')
    _check_stages(model, stages)
    device = torch.device(device)
    model = model.to(device)
    x = images.to(device).float()
    full = stages == 'full'
    has_fp = bit_config is not None and any(int(b) == -1 for b in bit_config)
    fused_state = model._fused()
    if fused_state and bit_config is not None and not has_fp and device.type == 'cuda':
        if model._plan is None:
            model.freeze(device)
        _, names, raw, _ = model._plan.forward_grams(x, [int(b) for b in bit_config], with_linear, stages=stages)
        return names, torch.ops.p2vit.cka_centre(raw)
    if full and not getattr(model, 'input_quant', True):
        raise AttributeError("get_stage_grams(stages='full'): the model has no qact_input (input_quant=False)")
    names = stage_names(model.depth, with_linear, full, False)
    acts = [a.reshape(x.shape[0], -1) for a in _hooked_outputs(model, x, bit_config, names, fused_state)]
    g = _grams(acts, None, dtype)
    return names, g.reshape(len(names), x.shape[0], x.shape[0])


def _compute_cka_stages(model1, model2, batches, bit_config1, bit_config2, stages, with_linear, dtype):
    cka = None
    for images in batches:
        if isinstance(images, (tuple, list)):
            images = images[0]
        _, g1 = get_stage_grams(images, model1, bit_config1, _device_of(model1), stages, with_linear, dtype=dtype)
        _, g2 = get_stage_grams(images, model2, bit_config2, _device_of(model2), stages, with_linear, dtype=dtype)
        if cka is None:
            cka = MinibatchCKA(g1.shape[0], g2.shape[0], across_models=True, dtype=dtype)
        cka.update_state_across_models_grams(g1, g2.to(g1.device))
    if cka is None:
        raise ValueError('compute_cka: no batches')
    return cka.result()


def compute_cka(model1, model2, batches, bit_config1, bit_config2, normalize_act=False, dtype=torch.float32, stages=None, with_linear=False):
    """the CKA heat map [layers of model1, layers of model2] between two models over ``batches`` (image tensors, or (images, labels)
    pairs), one update_state_across_models per batch.  ``stages='engine' | 'full'``: over the DDV stage lists of the two models
    (``get_stage_grams``; ``with_linear`` adds the linear outputs) instead of the linear layers."""
    if stages is not None:
        if normalize_act:
            raise NotImplementedError('compute_cka(stages=...): normalize_act rescales every image by its own norm, which the integer Grams '
                                      'of the codes do not carry')
        _check_stages(model1, stages)
        _check_stages(model2, stages)
        return _compute_cka_stages(model1, model2, batches, bit_config1, bit_config2, stages, with_linear, dtype)
    cka = None
    for images in batches:
        if isinstance(images, (tuple, list)):
            images = images[0]
        a1 = get_activations(images, model1, bit_config1, _device_of(model1), normalize_act)
        a2 = get_activations(images, model2, bit_config2, _device_of(model2), normalize_act)
        if cka is None:
            cka = MinibatchCKA(len(a1), len(a2), across_models=True, dtype=dtype)
        cka.update_state_across_models(a1, [a.to(a1[0].device) for a in a2])
    if cka is None:
        raise ValueError('compute_cka: no batches')
    return cka.result()


def main(argv=None):
    from . import harness, synth
    from .config import Config
    p = argparse.ArgumentParser(description='float vs quantized CKA heat map on synthetic data (cka_utility.py)')
    p.add_argument('--model', default='deit_small')
    p.add_argument('--bits', default='8', choices=['8', '4', 'mixed'])
    p.add_argument('--batch', default=50, type=int)
    p.add_argument('--iters', default=2, type=int)
    p.add_argument('--seed', default=0, type=int)
    p.add_argument('--device', default='cuda')
    p.add_argument('--result-name', default='cka_result')
    p.add_argument('--no-ptf', action='store_true', help='Config(ptf=False): float LayerNorm (ViT / DeiT and Swin)')
    p.add_argument('--no-lis', action='store_true', help='Config(lis=False): float softmax (ViT / DeiT and Swin)')
    p.add_argument('--softmax-bits', default=None, type=int, choices=[3, 4], help='width of the log-int-softmax (Config.BIT_TYPE_S: uint3 / uint4; default 4)')
    p.add_argument('--stages', default='linear', choices=['linear', 'engine', 'full'],
                   help='linear: the QConv2d / QLinear outputs; engine / full: the DDV stage lists (ViT / DeiT), from one engine call per batch')
    p.add_argument('--with-linear', action='store_true', help='with --stages engine / full: the linear outputs as stages too')
    args = p.parse_args(argv)
    if args.stages != 'linear' and args.model.startswith('swin'):      # refused before anything is built
        raise NotImplementedError('--stages %s: CKA over the DDV stage list covers the ViT / DeiT models' % args.stages)
    device = torch.device(args.device)
    fp = harness.str2model(args.model)(cfg=Config(not args.no_ptf, not args.no_lis, 'minmax').set_softmax_bits(args.softmax_bits))
    is_swin = harness._is_swin(fp)
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
    loader = harness.SyntheticLoader(args.batch * args.iters, args.batch, fp.arch['img_size'], fp.arch['num_classes'], args.seed + 2, device)
    stages = None if args.stages == 'linear' else args.stages
    heatmap = compute_cka(fp, q, loader, None, bits, stages=stages, with_linear=args.with_linear).cpu().numpy()
    os.makedirs(args.result_name, exist_ok=True)
    if stages is not None:
        from .ddv import stage_names
        names = stage_names(fp.depth, args.with_linear, stages == 'full')
        with open(os.path.join(args.result_name, '_names.pkl'), 'wb') as f:
            pickle.dump({'model1': names, 'model2': names}, f)
    path = os.path.join(args.result_name, '_heatmap.pkl')
    with open(path, 'wb') as f:
        pickle.dump(heatmap, f)
    print('heat map %s -> %s' % (heatmap.shape, path))
    return heatmap


if __name__ == '__main__':
    main()
