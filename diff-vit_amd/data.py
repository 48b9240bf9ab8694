"""Real-data leg of the evaluation harness: the reference's ``build_transform`` and ImageFolder loaders (test_quant.py:100-144,
504-534) without torchvision (not installed here) -- PIL + torch only.

``build_transform`` = Resize(floor(input/crop_pct), bicubic) -> CenterCrop(input) -> ToTensor -> Normalize with torchvision's
geometry rules (shorter side to ``size``, the other side ``int(size * long / short)``; crop offsets ``int(round((dim - crop) / 2))``).
**Parity unpinned**: nothing in the reference pins the transform's pixels and torchvision cannot be imported here to compare; the
resampling itself is PIL's, which is also what torchvision calls for PIL inputs.  ``ImageFolder`` follows torchvision's convention
(classes = sorted sub-directory names, samples sorted by path, the usual image extensions).

uint8 input: ``build_transform(..., to_uint8=True)`` stops before ToTensor and yields the HWC uint8 crop; ``normalize_uint8`` is the rest of
the chain (ToTensor's ``.float().div(255.0)``, then Normalize), op for op, and ``uint8_lut`` the same values as a [C][256] table - the one
definition that the device kernels (``forward_uint8``) and the unfused fallback read.
"""
import math
import os

import numpy as np
import torch
from PIL import Image

IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')
_INTERP = {'bicubic': Image.BICUBIC, 'lanczos': Image.LANCZOS, 'hamming': Image.HAMMING}

# per model family, test_quant.py:100-113
MODEL_STATS = {'deit': ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.875),
               'vit': ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), 0.9),
               'swin': ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 0.9)}


def _stats(mean, std, chans):
    """fp32 mean / std tensors [C, 1, 1], as build_transform builds them; their length must match the channel count"""
    mean_t = torch.tensor(mean, dtype=torch.float32).reshape(-1)
    std_t = torch.tensor(std, dtype=torch.float32).reshape(-1)
    if mean_t.numel() != chans or std_t.numel() != chans:
        raise ValueError('mean / std have %d / %d entries, the images %d channels' % (mean_t.numel(), std_t.numel(), chans))
    return mean_t.reshape(chans, 1, 1), std_t.reshape(chans, 1, 1)


def normalize_uint8(images, mean, std, layout='NHWC'):
    """uint8 images -> the fp32 tensor ``build_transform`` produces from them: ToTensor's ``.float().div(255.0)``, then
    ``(x - mean) / std`` with fp32 tensors, each an IEEE fp32 operation on the CPU.  ``images``: one image ([H, W, C] or [C, H, W]) or a
    batch ([B, H, W, C] or [B, C, H, W]) in ``layout`` 'NHWC' or 'NCHW'; the result is channels first ([C, H, W] or [B, C, H, W])."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise ValueError('normalize_uint8 takes a uint8 tensor, got %s' % (images.dtype if isinstance(images, torch.Tensor) else type(images).__name__))
    if layout not in ('NHWC', 'NCHW'):
        raise ValueError("layout must be 'NHWC' or 'NCHW', got %r" % (layout,))
    if images.dim() not in (3, 4):
        raise ValueError('normalize_uint8 takes [H, W, C] / [C, H, W] or a batch of them, got shape %s' % (tuple(images.shape),))
    x = images.cpu()
    if layout == 'NHWC':
        x = x.permute(2, 0, 1) if x.dim() == 3 else x.permute(0, 3, 1, 2)
    mean_t, std_t = _stats(mean, std, x.shape[-3])
    x = x.float().div(255.0)                                                                       # ToTensor
    return ((x - mean_t) / std_t).contiguous()                                                     # Normalize (NHWC input: NCHW memory order too)


def uint8_lut(mean, std, chans=None):
    """fp32 [C, 256]: entry [c, v] is what ``normalize_uint8`` makes of byte v in channel c (computed BY it, from an image that holds
    every byte value once per channel).  C = len(mean) unless ``chans`` is given."""
    chans = len(mean) if chans is None else chans
    v = torch.arange(256, dtype=torch.uint8).reshape(1, 256, 1).expand(1, 256, chans).contiguous()    # [1, 256, C]: NHWC, H = 1
    return normalize_uint8(v, mean, std, 'NHWC').reshape(chans, 256).contiguous()


def uint8_lut_i8(lut_f32, inv_s):
    """int8 [C, 256]: the codes ``k_quantize_patchify`` writes for the values of ``lut_f32`` - x * inv_s (the power-of-two inverse of
    the qact_input scale), rounded half to even, saturated to int8."""
    return torch.clamp(torch.round(lut_f32 * float(inv_s)), -128, 127).to(torch.int8)


def expand_uint8(images, lut_f32, layout='NHWC'):
    """uint8 images (a batch in ``layout``) -> fp32 [B, C, H, W] on their own device, every pixel looked up in ``lut_f32`` [C, 256]
    (``uint8_lut``): what ``normalize_uint8`` computes, by gathering.  The unfused states of ``forward_uint8`` and the calibration of a
    uint8 pipeline feed this to ``forward``."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise AssertionError('forward_uint8 takes uint8 images, got %s (fp32 images go to forward)' % getattr(images, 'dtype', type(images)))
    if layout not in ('NHWC', 'NCHW'):
        raise AssertionError("layout must be 'NHWC' or 'NCHW', got %r" % (layout,))
    if images.dim() != 4:
        raise AssertionError('uint8 images must be a 4-D batch ([B, H, W, C] or [B, C, H, W]), got shape %s' % (tuple(images.shape),))
    x = images.permute(0, 3, 1, 2) if layout == 'NHWC' else images
    if x.shape[1] != lut_f32.shape[0]:
        raise AssertionError('uint8 images in layout %s have %d channels, the statistics %d' % (layout, x.shape[1], lut_f32.shape[0]))
    lut = lut_f32.to(images.device)
    out = torch.empty(x.shape, dtype=torch.float32, device=images.device)
    for c in range(x.shape[1]):
        out[:, c] = lut[c][x[:, c].long()]
    return out


def build_transform(input_size=224, interpolation='bicubic', mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), crop_pct=0.875,
                    to_uint8=False):
    """test_quant.py:504-534: PIL image -> normalised fp32 tensor [3, input_size, input_size].  ``to_uint8``: everything before
    ToTensor, i.e. the uint8 crop [input_size, input_size, 3] (HWC) that ``normalize_uint8`` turns into the same fp32 tensor."""
    method = _INTERP.get(interpolation, Image.BILINEAR)
    size = int(math.floor(input_size / crop_pct)) if input_size > 32 else None
    mean_t = torch.tensor(mean, dtype=torch.float32).reshape(3, 1, 1)
    std_t = torch.tensor(std, dtype=torch.float32).reshape(3, 1, 1)

    def transform(img):
        img = img.convert('RGB')
        if size is not None:
            w, h = img.size
            if (w <= h and w != size) or (h <= w and h != size):              # Resize(int): shorter side -> size
                nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
                img = img.resize((nw, nh), method)
            w, h = img.size
            if w < input_size or h < input_size:                                # CenterCrop pads small images with zeros
                pad = Image.new('RGB', (max(w, input_size), max(h, input_size)))
                pad.paste(img, ((pad.size[0] - w) // 2, (pad.size[1] - h) // 2))
                img, (w, h) = pad, pad.size
            top, left = int(round((h - input_size) / 2.0)), int(round((w - input_size) / 2.0))
            img = img.crop((left, top, left + input_size, top + input_size))
        u8 = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())
        if to_uint8:
            return u8
        x = u8.permute(2, 0, 1).float().div(255.0)                                                       # ToTensor
        return (x - mean_t) / std_t                                                                        # Normalize

    return transform


class ImageFolder(torch.utils.data.Dataset):
    """root/<class>/<image>: (transformed image, class index), torchvision.datasets.ImageFolder's ordering (test_quant.py:122,136)."""

    def __init__(self, root, transform=None):
        self.root, self.transform = root, transform
        self.classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
        if not self.classes:
            raise FileNotFoundError("Couldn't find any class folder in %s." % root)
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}
        self.samples = []
        for c in self.classes:
            for dirpath, _, files in sorted(os.walk(os.path.join(root, c), followlinks=True)):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXTENSIONS):
                        self.samples.append((os.path.join(dirpath, f), self.class_to_idx[c]))
        if not self.samples:
            raise FileNotFoundError('Found no valid file for the classes in %s.' % root)

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        path, target = self.samples[i]
        with Image.open(path) as img:
            x = img.convert('RGB')
        return (self.transform(x) if self.transform else x), target


def model_family(model_name):
    """the MODEL_STATS key of a model name"""
    return 'swin' if model_name.startswith('swin') else ('vit' if model_name.startswith('vit') else 'deit')


def build_loaders(data_root, model_name, val_batchsize, calib_batchsize, num_workers=0, uint8=False, input_size=224):
    """the reference's two loaders (test_quant.py:118-144): val (in order) and train (shuffled, drop_last; calibration batches).
    ``uint8``: the batches are the uint8 crops, NHWC [B, H, W, 3] (a quarter of the bytes to copy; ``forward_uint8`` normalises them on
    the device with the family's MODEL_STATS).  ``input_size``: the crop the model takes (384 for the window-12 Swin factories)."""
    mean, std, crop_pct = MODEL_STATS[model_family(model_name)]
    tf = build_transform(input_size=input_size, mean=mean, std=std, crop_pct=crop_pct, to_uint8=uint8)
    val = torch.utils.data.DataLoader(ImageFolder(os.path.join(data_root, 'val'), tf), batch_size=val_batchsize, shuffle=False,
                                      num_workers=num_workers, pin_memory=torch.cuda.is_available())       # (test_quant.py:128: pin_memory=True)
    train_dir = os.path.join(data_root, 'train')
    train = None
    if os.path.isdir(train_dir):
        train = torch.utils.data.DataLoader(ImageFolder(train_dir, tf), batch_size=calib_batchsize, shuffle=True, num_workers=num_workers,
                                            pin_memory=torch.cuda.is_available(), drop_last=True)
    return val, train
