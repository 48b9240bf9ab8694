"""GPU: what the softmax width costs.
  python tools/bench_softmax_bits.py tokens [img] [batch] [dump.npy]
      the DeiT-S architecture of tools/bench_tokens.py at one image size (default 448: 785 tokens, the packed attention kernel) with the
      default 4-bit softmax: images/s of the one-stream and the sliced forward (median of 5 loops of 10 steps) and the md5 of the logits -
      run once per library build (tools/abx.sh swaps the library the same way) to compare two builds
  python tools/bench_softmax_bits.py widths
      launch times (HIP events, median of 20 launches after 5) of the attention operators at 3 and at 4 bits on the same codes:
      k_lis_attention_packed (785 tokens, head_dim 64, 64 images x 6 heads) and the 7 x 7 k_window_attention (56 x 56 tokens, 4 heads,
      64 images: stage 0 of Swin-B), through p2v_lis_attention_bits / p2v_window_attention_bits
"""
import ctypes as C
import hashlib
import os
import statistics
import sys
import time
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import diff_vit_amd as dva          # noqa: E402

E = dva.engine


def tokens(img=448, batch=64, dump=None):
    arch = dict(img_size=img, patch_size=16, embed_dim=384, depth=12, num_heads=6, num_classes=1000, mlp_ratio=4.0)
    m = dva.VisionTransformer(qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config(), **arch)
    m.load_state_dict(dva.synth.vit_state_dict(arch, 5), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(5, 2, img).cuda())
    plan = m.freeze()
    x = dva.synth.images(5, batch, img, offset=100).cuda()
    bc = [8] * 50
    out = torch.empty(batch, 1000, device='cuda')
    for mode in ('one stream', 'sliced'):
        run = (lambda: plan.forward(x, bc, out=out)) if mode == 'one stream' else (lambda: plan.forward_streams(x, bc, out, 3))
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        loops = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(10):
                run()
            torch.cuda.synchronize()
            loops.append((time.perf_counter() - t0) / 10)
        dt = statistics.median(loops)
        print('img %d (%d tokens, %s) batch %d %-10s %8.1f img/s  %7.3f ms  (loops %s)' % (
            img, (img // 16) ** 2 + 1, plan.attention_kernel, batch, mode, batch / dt, dt * 1e3, ' '.join('%.3f' % (v * 1e3) for v in loops)), flush=True)
    logits = plan.forward(x, bc).cpu().numpy()
    print('logits md5 %s' % hashlib.md5(logits.tobytes()).hexdigest(), flush=True)
    if dump:
        np.save(dump, logits)


def _time(launch, n=20, warm=5):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def widths():
    import p2vit_oracle as O
    import swin_oracle as SO
    L = E.lib()
    gen = torch.Generator().manual_seed(3)
    codes = lambda shape, std: torch.clamp(torch.round(torch.randn(shape, generator=gen) * std), -128, 127).to(torch.int8)
    # ViT: 785 tokens, head_dim 64 -> the packed kernel
    B, N, H, hd = 64, 785, 6, 64
    assert L.p2v_attention_kernel(hd, N, 0) == 1
    qkv = codes((B, N, 3 * H * hd), 30.0).cuda()
    out = torch.empty(B, N, H * hd, dtype=torch.int8, device='cuda')
    x0, bb, cc = O.lis_consts(torch.tensor([2.0 ** -4]))
    at = E.Attn(2.0 ** -8, float(np.float32(hd ** -0.5)), 2.0 ** 4, 0.5, x0, bb, cc)
    res = {}
    for rnd in range(3):                     # alternating, three rounds
        for bits in (4, 3):
            res.setdefault(('packed', bits), []).append(_time(lambda: E.check(L.p2v_lis_attention_bits(
                E.ptr(qkv), B, N, H, hd, C.byref(at), bits, E.ptr(out), None, E.stream_ptr())))[0])
    # Swin: 7 x 7 windows over 56 x 56 tokens, 4 heads
    Hf, ws, heads, Bw = 56, 7, 4, 64
    T, Cc = Hf * Hf, heads * 32
    wq = codes((Bw, T, 3 * Cc), 25.0).cuda()
    wo = torch.empty(Bw, T, Cc, dtype=torch.int8, device='cuda')
    tab = codes(((2 * ws - 1) ** 2, heads), 30.0).cuda()
    idx = SO.window_index(Hf, Hf, ws, 3).to(torch.int32).contiguous().cuda()
    img = torch.zeros(Hf, Hf)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -3), slice(-3, None)):
        for wsl in (slice(0, -ws), slice(-ws, -3), slice(-3, None)):
            img[hs, wsl] = cnt
            cnt += 1
    reg = img.reshape(Hf // ws, ws, Hf // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws).to(torch.int8).contiguous().cuda()
    wa = E.WinAttn(2.0 ** -4, float(np.float32(32 ** -0.5)), 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, x0, bb, cc, E.ptr(tab), E.ptr(idx), E.ptr(reg),
                   ws, idx.shape[0])
    for rnd in range(3):
        for bits in (4, 3):
            res.setdefault(('window7', bits), []).append(_time(lambda: E.check(L.p2v_window_attention_bits(
                E.ptr(wq), Bw, T, heads, 32, C.byref(wa), bits, E.ptr(wo), None, E.stream_ptr())))[0])
    for (name, bits), v in sorted(res.items()):
        print('%-8s softmax_bits %d: median launch %.4f ms  (rounds %s)' % (name, bits, statistics.median(v), ' '.join('%.4f' % t for t in v)), flush=True)


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'widths'
    if mode == 'tokens':
        tokens(int(sys.argv[2]) if len(sys.argv) > 2 else 448, int(sys.argv[3]) if len(sys.argv) > 3 else 64, sys.argv[4] if len(sys.argv) > 4 else None)
    else:
        widths()
