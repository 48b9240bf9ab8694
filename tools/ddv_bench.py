"""Times a DDV of the quantized model on the GPU (not bench.py): n clean + n perturbed images, [8] * L, median of --reps, one JSON line
per model.

    python tools/ddv_bench.py [--n 50] [--reps 10] [--models deit_small,vit_base] [--stages full]
    python tools/ddv_bench.py --swin swin_base [--n 50] [--reps 10]        the Swin lines (below), instead of the ViT / DeiT ones

  (a)  forward_ms                 FrozenPlan.forward of the 2n images (one stream; the last block on the class rows only)
       forward_all_rows_ms        the same with the switch cls_rows = 0: every row of the last block, what every tap entry point computes
  (b)  ddv_int8_ms                FrozenPlan.forward_ddv: the 5 * depth + 3 stages reduced from the live int8 buffers
  (c)  ddv_linear_ms              forward_ddv(with_linear=True): + the 4 * depth + 1 linear outputs through ONE fp32 tap buffer
       --stages full adds         ddv_full_int8_ms / ddv_full_linear_ms: forward_ddv(stages='full'), the 9 * depth + 7 / 13 * depth + 8 stages
                                  of P2V_DDV_STAGES_FULL (every hook point of the reference's list), and forward_unfused_all_rows_ms: the
                                  plain forward with cls_rows = 0 and ln_gemm = 0, the launch sequence the FULL call runs its stages between
  (d)  taps_torch_ms              what there was before: forward_linear_taps (all fp32 taps resident) + torch cosine_similarity per tap
       reduction                  bytes the reductions of (b) read (both operands of every stage), the time they add to the all-rows
                                  forward, and the rate; `standalone`: ONE grouped p2v_pair_cosine over buffers of the same shapes,
                                  ~0.9 GB that no launch has just written.  HBM: 8.0 TB/s peak, 6.29 TB/s measured for a float4 copy
                                  (MI355X_MICROARCH.md); the live buffers of (b) mostly sit in the 256 MiB Infinity Cache.

  --swin (synthetic weights, calibrated on two images, 8-bit, one stream):
       forward_ms                 SwinPlan.forward of the 2n images (n_streams = 1)
       ddv_int8_ms                SwinPlan.forward_ddv(with_linear=False): the recorded sequence with a P2V_OP_COS behind every stage
       ddv_linear_ms              forward_ddv(with_linear=True): + every linear output through ONE fp32 scratch buffer
       taps_torch_ms              the alternative it replaces: forward(taps=...) (segmented replay, every tap cloned) +
                                  torch.ops.p2vit.pair_cosine on the cloned taps
       resid_tap                  the last stage's fc2 (RESID) launch alone, without and with the mid-code output, median of 10 x 20 launches

    python tools/ddv_bench.py --attention [--models deit_small] [--swin swin_tiny] [--n 50] [--reps 10]
       the cost of the stages inside attention: forward_ddv(with_linear=False) without and with attention=True, ALTERNATING in one
       process (three rounds of median-of-reps each), the stage counts and the bytes of the attention scratch"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import numpy as np  # noqa: E402

import diff_vit_amd as dva  # noqa: E402
import p2vit_oracle as O  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def run(model, n, reps, full=False):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', model + '.npz'))
    arch = dva.synth.ARCHS[model]
    sd = dva.synth.vit_state_dict(arch, int(g['seed']))
    calib = O.unflatten_calib({k[len('calib/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('calib/')})
    plan = dva.FrozenPlan(arch, sd, calib, device=torch.device('cuda:0'))
    L = 4 * arch['depth'] + 2
    bits = [8] * L
    x = dva.synth.images(1, 2 * n, 224).cuda()
    lib = dva.engine.lib()
    t_fwd = timed(lambda: plan.forward(x, bits), reps)
    cls_rows = int(os.environ.get('P2V_CLS_ROWS', '1') != '0')        # what the process started with (the library reads it once)
    lib.p2v_set_tuning(b'cls_rows', 0)
    t_all = timed(lambda: plan.forward(x, bits), reps)
    lib.p2v_set_tuning(b'cls_rows', cls_rows)
    t_b = timed(lambda: plan.forward_ddv(x, bits, False), reps)
    t_c = timed(lambda: plan.forward_ddv(x, bits, True), reps)

    def taps_torch():
        logits, taps = plan.forward_linear_taps(x, bits, want=set(range(1, L)))
        return [F.cosine_similarity(t[:n].reshape(n, -1), t[n:].reshape(n, -1), dim=1) for t in taps[1:]] + \
               [F.cosine_similarity(logits[:n], logits[n:], dim=1)]
    t_d = timed(taps_torch, reps)
    extra = {}
    if full:
        lib.p2v_set_tuning(b'cls_rows', 0)
        lib.p2v_set_tuning(b'ln_gemm', 0)
        t_unfused = timed(lambda: plan.forward(x, bits), reps)
        lib.p2v_set_tuning(b'ln_gemm', int(os.environ.get('P2V_LN_GEMM', '1') != '0'))
        lib.p2v_set_tuning(b'cls_rows', cls_rows)
        t_fb = timed(lambda: plan.forward_ddv(x, bits, False, stages='full'), reps)
        t_fc = timed(lambda: plan.forward_ddv(x, bits, True, stages='full'), reps)
        extra = {'stages_full_int8': 9 * arch['depth'] + 7, 'stages_full_linear': 13 * arch['depth'] + 8,
                 'forward_unfused_all_rows_ms': round(t_unfused, 3), 'ddv_full_int8_ms': round(t_fb, 3), 'ddv_full_linear_ms': round(t_fc, 3),
                 'ddv_full_int8_over_ddv_int8': round(t_fb / t_b, 3), 'ddv_full_linear_over_ddv_linear': round(t_fc / t_c, 3),
                 'ddv_full_linear_over_taps_torch': round(t_fc / t_d, 3),
                 'us_per_added_stage': {'int8': round((t_fb - t_b) * 1e3 / (4 * arch['depth'] + 4), 2),
                                        'linear': round((t_fc - t_c) * 1e3 / (4 * arch['depth'] + 4), 2)}}
    T, D, Hd = plan.tokens, plan.D, plan.hidden
    per_block = [(T, 3 * D), (T, D), (T, D), (T, Hd), (T, D)]
    shapes = [(T, D)] + per_block * arch['depth'] + [(1, D)]
    nbytes = 2.0 * n * sum(r * c for r, c in shapes) + 2.0 * n * arch['num_classes'] * 4
    a = [torch.randint(-128, 128, (n, r, c), dtype=torch.int8, device='cuda') for r, c in shapes]
    b = [torch.randint(-128, 128, (n, r, c), dtype=torch.int8, device='cuda') for r, c in shapes]
    t_alone = timed(lambda: torch.ops.p2vit.pair_cosine(a, b, [None] * len(a)), reps)
    tap_bytes = sum(int(np.prod(s)) for s in plan.tap_shapes(2 * n)[1:]) * 4
    return {'model': model, 'n': n, 'images': 2 * n, 'stages_int8': 5 * arch['depth'] + 3, 'stages_linear': 9 * arch['depth'] + 4,
            'forward_ms': round(t_fwd, 3), 'forward_all_rows_ms': round(t_all, 3), 'ddv_int8_ms': round(t_b, 3),
            'ddv_linear_ms': round(t_c, 3), 'taps_torch_ms': round(t_d, 3),
            'ddv_int8_over_forward': round(t_b / t_fwd, 3), 'ddv_linear_over_taps_torch': round(t_c / t_d, 3),
            'fp32_activation_MB': {'ddv_linear': round(plan.ddv_tap_bytes(n) / 1e6, 1), 'taps_torch': round(tap_bytes / 1e6, 1)},
            'reduction': {'MB_read': round(nbytes / 1e6, 1), 'added_ms': round(t_b - t_all, 3),
                          'TBps_in_forward': round(nbytes / max(t_b - t_all, 1e-6) / 1e9, 2),
                          'standalone_ms': round(t_alone, 3), 'standalone_TBps': round(2.0 * n * sum(r * c for r, c in shapes) / t_alone / 1e9, 2),
                          'hbm_TBps': {'peak': 8.0, 'measured_copy': 6.29}}, **extra}


def run_swin(name, n, reps):
    import contextlib
    import ctypes as C
    E = dva.engine
    with contextlib.redirect_stdout(sys.stderr):
        model = dva.harness.str2model(name)(cfg=dva.Config(True, True, 'minmax'))
    model.load_state_dict(dva.synth.swin_state_dict(model.state_dict(), 0))
    model = model.cuda().eval()
    img = model.arch['img_size']
    with torch.no_grad():
        dva.harness.calibrate_model(model, dva.synth.images(0, 2, img).cuda())
    plan = model.freeze(torch.device('cuda:0'), bits=8)
    x = dva.synth.images(1, 2 * n, img).cuda()
    t_fwd = timed(lambda: plan.forward(x, n_streams=1), reps)
    t_b = timed(lambda: plan.forward_ddv(x, False), reps)
    t_c = timed(lambda: plan.forward_ddv(x, True), reps)

    def taps_torch():
        taps = {}
        logits = plan.forward(x, taps=taps)
        ts = list(taps.values())
        return torch.ops.p2vit.pair_cosine([t[:t.shape[0] // 2].reshape(n, -1, t.shape[1]) for t in ts],
                                           [t[t.shape[0] // 2:].reshape(n, -1, t.shape[1]) for t in ts], [None] * len(ts)), logits
    t_d = timed(taps_torch, reps)
    # the mid-code tap on one RESID launch: fc2 of the last stage at 2n images
    b = plan.stages[-1]['blocks'][-1]
    rows, Cc = 2 * n * plan.H_last * plan.H_last, plan.C_last
    hid = torch.randint(-128, 128, (rows, 4 * Cc), dtype=torch.int8, device='cuda')
    res = torch.randint(-128, 128, (rows, Cc), dtype=torch.int8, device='cuda')
    out, mid = torch.empty_like(res), torch.empty_like(res)
    epi = E.Epilogue()
    src = b['fc2_epi']
    lin, tab = plan._lin(b['fc2'], plan.bits), plan._resid_tab(b['fc2'], plan.bits)      # int8-stored codes: what the tapped launch takes
    epi.s_mid, epi.s_res, epi.s_next, epi.residual, epi.resid_tab = src.s_mid, src.s_res, src.s_next, E.ptr(res), tab
    L = E.lib()

    def fc2(tap):
        for _ in range(20):
            E.check(L.p2v_gemm_i8(E.EPI_RESID, E.ptr(hid), 4 * Cc, rows, 4 * Cc, Cc, C.byref(lin), C.byref(epi), E.ptr(out), Cc,
                                  E.ptr(mid) if tap else None, E.stream_ptr()))
    t_plain, t_tap = timed(lambda: fc2(False), reps) / 20, timed(lambda: fc2(True), reps) / 20
    return {'model': name, 'n': n, 'images': 2 * n, 'stages_int8': len(dva.ddv.swin_stage_names(model.arch['depths'], False)),
            'stages_linear': len(dva.ddv.swin_stage_names(model.arch['depths'], True)),
            'forward_ms': round(t_fwd, 3), 'ddv_int8_ms': round(t_b, 3), 'ddv_linear_ms': round(t_c, 3), 'taps_torch_ms': round(t_d, 3),
            'ddv_int8_over_forward': round(t_b / t_fwd, 3),
            'resid_tap': {'layer': 'stage %d fc2' % (len(plan.stages) - 1), 'M': rows, 'K': 4 * Cc, 'N': Cc, 'prefolded': bool(tab),
                          'plain_us': round(t_plain * 1e3, 2), 'tapped_us': round(t_tap * 1e3, 2)}}


def run_attention(name, n, reps, swin):
    """forward_ddv without / with the stages inside attention, alternating; ViT / DeiT from the golden calibration, Swin calibrated on two images"""
    if swin:
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):
            model = dva.harness.str2model(name)(cfg=dva.Config(True, True, 'minmax'))
        model.load_state_dict(dva.synth.swin_state_dict(model.state_dict(), 0))
        model = model.cuda().eval()
        img = model.arch['img_size']
        with torch.no_grad():
            dva.harness.calibrate_model(model, dva.synth.images(0, 2, img).cuda())
        plan = model.freeze(torch.device('cuda:0'), bits=8)
        x = dva.synth.images(1, 2 * n, img).cuda()
        fwd = lambda: plan.forward(x, n_streams=1)
        off, on = (lambda: plan.forward_ddv(x, False)), (lambda: plan.forward_ddv(x, False, attention=True))
        depths = model.arch['depths']
        stages = (len(dva.ddv.swin_stage_names(depths, False)), len(dva.ddv.swin_stage_names(depths, False, True)))
        scratch = 0
        for st_ in plan.stages:      # three planes per stage, shared by its blocks
            b = st_['blocks'][0]
            N = b['ws'] * b['ws']
            scratch += 3 * 2 * n * b['wa'].n_windows * b['heads'] * N * ((N + 15) // 16 * 16)
    else:
        g = np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'))
        arch = dva.synth.ARCHS[name]
        calib = O.unflatten_calib({k[len('calib/'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('calib/')})
        plan = dva.FrozenPlan(arch, dva.synth.vit_state_dict(arch, int(g['seed'])), calib, device=torch.device('cuda:0'))
        bits = [8] * (4 * arch['depth'] + 2)
        x = dva.synth.images(1, 2 * n, 224).cuda()
        fwd = lambda: plan.forward(x, bits)
        off, on = (lambda: plan.forward_ddv(x, bits, False)), (lambda: plan.forward_ddv(x, bits, False, attention=True))
        stages = (len(dva.ddv.stage_names(arch['depth'], False)), len(dva.ddv.stage_names(arch['depth'], False, False, True)))
        scratch = plan.ddv_attn_bytes(n)
    t_fwd = timed(fwd, reps)
    rounds = [(timed(off, reps), timed(on, reps)) for _ in range(3)]
    t_off, t_on = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
    return {'model': name, 'n': n, 'images': 2 * n, 'forward_ms': round(t_fwd, 3), 'stages': {'without': stages[0], 'with_attention': stages[1]},
            'rounds_ms': [[round(a_, 3), round(b_, 3)] for a_, b_ in rounds], 'ddv_int8_ms': round(t_off, 3), 'ddv_int8_attention_ms': round(t_on, 3),
            'attention_over_plain': round(t_on / t_off, 3), 'us_per_added_stage': round((t_on - t_off) * 1e3 / (stages[1] - stages[0]), 2),
            'attention_scratch_MB': round(scratch / 1e6, 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=50)
    p.add_argument('--reps', type=int, default=10)
    p.add_argument('--models', default='deit_small,vit_base')
    p.add_argument('--stages', default='engine', choices=['engine', 'full'], help='full: also time forward_ddv(stages="full") (ViT / DeiT)')
    p.add_argument('--swin', default=None, help='a Swin factory name of harness.str2model (swin_base): the Swin lines instead')
    p.add_argument('--attention', action='store_true', help='the cost of the stages inside attention (see the module docstring)')
    a = p.parse_args()
    if a.attention:
        for m in ([] if a.models == 'deit_small,vit_base' and a.swin else a.models.split(',')):
            print(json.dumps(run_attention(m, a.n, a.reps, False)), flush=True)
        if a.swin:
            print(json.dumps(run_attention(a.swin, a.n, a.reps, True)), flush=True)
        return
    if a.swin:
        print(json.dumps(run_swin(a.swin, a.n, a.reps)), flush=True)
        return
    for m in a.models.split(','):
        print(json.dumps(run(m, a.n, a.reps, a.stages == 'full')), flush=True)


if __name__ == '__main__':
    main()
