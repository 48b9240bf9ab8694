"""Data-free calibration images (the reference's ``--mode 2``, generate_data.py: PSAQ-ViT): images are optimised from Gaussian noise
through the FLOAT module graph of a model of this package, 2 x ``iterations`` Adam steps on

    total = - sum over blocks of entropy(attn @ v)  +  1.0 * CE(logits, pseudo labels)  +  0.05 * | TV(images) - var_pred |

``entropy`` is the patch-similarity entropy (generate_data.py:102-113, 128-134 with utils/kde.py:87-96).  For ``av`` [images * groups, heads,
tokens, head_dim] (groups = windows per image, 1 for ViT / DeiT):

    a   = mean over heads, row 0 of every group dropped                 T = tokens - 1 rows of head_dim values per group
    S   = cosine similarity of every pair of rows of a group            each row divided by max(|row|, 1e-8); diagonal included
    lo, hi = min, max of S over the whole call                           constants of the differentiation (the reference's .item())
    x_k = linspace(lo, hi, 10)
    p_k = (c / n) sum_m exp(-(x_k - s_m)^2 / (2 h^2))                   per image over its n = groups * T^2 similarities; h = 0.01, c = 1 / sqrt(2 pi h^2)
    q_k = p_k + 1e-4,  f_k = -q_k ln q_k,  E_b = trapezoid rule of f over x,  value = mean_b E_b

On a CUDA tensor :func:`patch_similarity_entropy` is ONE call of ``torch.ops.p2vit.patch_similarity_entropy`` (csrc/p2vit_psaq.hip): value
and closed-form gradient together, S in a workspace of images * groups * T^2 floats instead of the composition's [images, 10, n] tensors,
no host synchronisation.  On a CPU tensor it is :func:`patch_similarity_entropy_cpu`, the torch composition image by image (the twin of the
op, as ``ddv.pair_cosine_cpu`` is of its op).  ``generate_data(..., loss='torch')`` runs the reference's whole-batch composition under
autograd instead (the A/B of tools/bench_psaq.py).

Not reproduced: the reference's images bit for bit (it runs timm's float model and the CUDA generator).  The ``random`` module is consumed
in the reference's order: ``batch_size`` pseudo labels, ``var_pred``, then per step the jitter offset and the flip draw."""
import math
import random

import torch
import torch.nn.functional as F

BANDWIDTH = 0.01          # utils/kde.py:47
POINTS = 10               # generate_data.py:110
PDF_EPS = 1e-4            # generate_data.py:130
EPOCHS = ((500, 15), (500, 30))   # generate_data.py:64-70: (steps, jitter limit in pixels) per epoch; `iterations` replaces the steps
WARMUP = 100              # generate_data.py:72


def _composition(av, groups, rng=None, images=None):
    """the reference's lines on ``av`` [images * groups, heads, tokens, head_dim] under autograd: sum over the images of ``av`` of the
    per-image entropy, divided by ``images`` (default: those of ``av``).  ``rng`` = (lo, hi) overrides the range of this call's own
    similarities (python floats, as ``.item()`` yields them)."""
    BG, H, N, hd = av.shape
    B = BG // groups
    a = av.mean(dim=1)[:, 1:, :]
    sims = torch.cosine_similarity(a.unsqueeze(1), a.unsqueeze(2), dim=3)
    if rng is None:
        rng = (sims.min().item(), sims.max().item())
    train = sims.reshape(B, 1, -1)
    x = torch.linspace(rng[0], rng[1], steps=POINTS, dtype=av.dtype, device=av.device).repeat(B, 1)
    var = BANDWIDTH ** 2
    kern = torch.exp(-torch.pow(x.view(B, POINTS, 1) - train, 2) / (2 * var))
    coef = 1 / torch.sqrt(torch.tensor(2 * math.pi * var))
    pdf = (coef * kern).mean(dim=-1) + PDF_EPS
    f = -1 * pdf * torch.log(pdf)
    return torch.trapz(f, x, dim=-1).sum() / (images or B)


def patch_similarity_entropy_torch(av, groups=1):
    """the whole-batch torch composition (differentiable by autograd; one host synchronisation for the range): what the reference runs"""
    return _composition(av, groups)


def patch_similarity_entropy_cpu(av, groups=1):
    """the twin of ``torch.ops.p2vit.patch_similarity_entropy`` in plain torch, any device: (value fp64 [], grad like ``av``) of the
    composition in ``av``'s dtype, image by image (the range first, over every image), so that memory stays at one image's [10, n]."""
    if av.dim() != 4 or groups < 1 or av.shape[0] % groups:
        raise AssertionError('patch_similarity_entropy: av is [images * groups, heads, tokens, head_dim] (got shape %s, groups %d)'
                             % (tuple(av.shape), groups))
    av = av.detach()
    B = av.shape[0] // groups
    lo, hi = math.inf, -math.inf
    with torch.no_grad():
        for b in range(B):
            a = av[b * groups:(b + 1) * groups].mean(dim=1)[:, 1:, :]
            s = torch.cosine_similarity(a.unsqueeze(1), a.unsqueeze(2), dim=3)
            lo, hi = min(lo, s.min().item()), max(hi, s.max().item())
    value = torch.zeros((), dtype=torch.float64, device=av.device)
    grad = torch.empty_like(av)
    for b in range(B):
        with torch.enable_grad():
            leaf = av[b * groups:(b + 1) * groups].clone().requires_grad_(True)
            part = _composition(leaf, groups, (lo, hi), B)
            grad[b * groups:(b + 1) * groups], = torch.autograd.grad(part, leaf)
        value += part.detach().double()
    return value, grad


class _PatchSimilarityEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, av, groups):
        if av.is_cuda:
            value, grad = torch.ops.p2vit.patch_similarity_entropy(av.detach(), groups)
        else:
            value, grad = patch_similarity_entropy_cpu(av, groups)
        ctx.save_for_backward(grad)
        return value.to(av.dtype)

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return grad.to(g.dtype) * g, None


def patch_similarity_entropy(av, groups=1):
    """value of the patch-similarity entropy of ``av`` [images * groups, heads, tokens, head_dim], differentiable with respect to ``av``:
    value and gradient come from one call (the HIP operator on a CUDA tensor, :func:`patch_similarity_entropy_cpu` on a CPU tensor) and
    backward scales the stored gradient."""
    return _PatchSimilarityEntropy.apply(av, groups)


def image_prior_loss(x):
    """the total-variation prior (generate_data.py:137-145): the sum of the 2-norms of the four neighbour differences (right, down and
    the two diagonals) of a batch [B, C, H, W]"""
    d1 = x[:, :, :, :-1] - x[:, :, :, 1:]
    d2 = x[:, :, :-1, :] - x[:, :, 1:, :]
    d3 = x[:, :, 1:, :-1] - x[:, :, :-1, 1:]
    d4 = x[:, :, :-1, :-1] - x[:, :, 1:, 1:]
    return torch.norm(d1) + torch.norm(d2) + torch.norm(d3) + torch.norm(d4)


def clip_images(x, mean, std):
    """clamp every channel of ``x`` [B, C, H, W] in place to the normalised image range [-m / s, (1 - m) / s] (generate_data.py:148-160)"""
    for c, (m, s) in enumerate(zip(mean, std)):
        x[:, c] = torch.clamp(x[:, c], -m / s, (1 - m) / s)
    return x


def lr_cosine_policy(base_lr, warmup_length, epochs):
    """generate_data.py:163-182: ``policy(optimizer, iteration, epoch)`` sets every group's lr - linear over ``warmup_length`` steps up
    to ``base_lr``, then half a cosine down to 0 at ``epochs``; ``policy.lr(epoch)`` is the value alone"""
    def lr(epoch):
        if epoch < warmup_length:
            return base_lr * (epoch + 1) / warmup_length
        return 0.5 * (1 + math.cos(math.pi * (epoch - warmup_length) / (epochs - warmup_length))) * base_lr

    def policy(optimizer, iteration, epoch):
        for group in optimizer.param_groups:
            group['lr'] = lr(epoch)
    policy.lr = lr
    return policy


def _attention_modules(model):
    from .swin import SwinTransformer
    if isinstance(model, SwinTransformer):
        return [blk.attn for layer in model.layers for blk in layer.blocks]
    return [blk.attn for blk in model.blocks]


def _logits(model, x):
    out = model(x)
    return out[0] if isinstance(out, (tuple, list)) else out


def generate_data(model, batch_size, iterations=500, seed=None, loss='engine', family=None):
    """``batch_size`` calibration images for ``model`` (a float-state VisionTransformer or SwinTransformer of this package), generated
    on the model's device by the reference's loop (generate_data.py:33-125): two epochs of ``iterations`` Adam steps (betas 0.5 / 0.9,
    lr 0.20, Swin 0.25, 100 warm-up steps then cosine), jitter up to 15 / 30 pixels, random flip, pseudo labels drawn from
    ``num_classes``; after every step the images are clamped to the normalised [0, 1] range of ``family`` (a key of
    ``data.MODEL_STATS``; default 'swin' for a Swin model, else 'deit': the reference clamps with the ImageNet statistics).
    ``loss='engine'``: the entropy term through :func:`patch_similarity_entropy`; ``'torch'``: the whole-batch composition.
    ``seed`` seeds ``random`` and torch.  The parameters are frozen for the duration; a quantized or calibrating model raises."""
    from .data import MODEL_STATS
    from .swin import SwinTransformer
    if loss not in ('engine', 'torch'):
        raise ValueError("loss must be 'engine' or 'torch'")
    if getattr(model, 'quant', False) or any(m.quant or m.calibrate for m in model._q_modules()):
        raise ValueError('generate_data needs the float model: call it before calibration (model_dequant() returns a quantized model '
                         'to the float state)')
    is_swin = isinstance(model, SwinTransformer)
    mean, std, _ = MODEL_STATS[family or ('swin' if is_swin else 'deit')]
    entropy = patch_similarity_entropy if loss == 'engine' else patch_similarity_entropy_torch
    device = next(model.parameters()).device
    size = model.arch['img_size']
    if seed is not None:
        random.seed(seed)
        torch.manual_seed(seed)
    img = torch.randn((batch_size, model.in_chans, size, size)).to(device).requires_grad_(True)
    base_lr = 0.25 if is_swin else 0.20
    optimizer = torch.optim.Adam([img], lr=base_lr, betas=(0.5, 0.9), eps=1e-8)
    pred = torch.LongTensor([random.randint(0, model.num_classes - 1) for _ in range(batch_size)]).to(device)
    var_pred = random.uniform(2500, 3000)
    attns = _attention_modules(model)
    products = []
    params = [(p, p.requires_grad) for p in model.parameters()]
    training = model.training
    try:
        model.eval()
        for p, _ in params:
            p.requires_grad_(False)
        for m in attns:
            m.av_hook = products.append
        for _, lim in EPOCHS:
            schedule = lr_cosine_policy(base_lr, WARMUP, iterations)
            for itr in range(iterations):
                schedule(optimizer, itr, itr)
                off = random.randint(-lim, lim)
                jit = torch.roll(img, shifts=(off, off), dims=(2, 3))
                if random.random() > 0.5:
                    jit = torch.flip(jit, dims=(3,))
                optimizer.zero_grad()
                del products[:]
                with torch.enable_grad():
                    output = _logits(model, jit)
                    loss_oh = F.cross_entropy(output, pred)
                    loss_tv = torch.norm(image_prior_loss(jit) - var_pred)
                    loss_entropy = 0
                    for av in products:
                        loss_entropy = loss_entropy - entropy(av, av.shape[0] // batch_size)
                    total = loss_entropy + 1.0 * loss_oh + 0.05 * loss_tv
                total.backward()
                optimizer.step()
                img.data = clip_images(img.data, mean, std)
    finally:
        for m in attns:
            m.av_hook = None
        for p, flag in params:
            p.requires_grad_(flag)
        model.train(training)
        del products[:]
    return img.detach()
