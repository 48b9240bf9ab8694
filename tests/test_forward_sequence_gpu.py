"""GPU: the launch sequence of the whole-model forward, as p2v_forward_profile / p2v_forward_profile_begin report it (one P2V_K_* kind per
launch, 'event_gap' last), against literal lists built from the depth - under the switch sets that change the sequence, and for one
geometry the fused LayerNorm+GEMM kernel does not cover."""
import ctypes as C
from functools import partial

import pytest
import torch

from _tuning import tuning
from conftest import gpu_ok

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_ok(), reason='needs a GPU')]

HEAD = ['patchify', 'gemm_embed', 'fill_cls']
FUSED = ['ln_gemm_qkv', 'attention', 'gemm_proj', 'ln_gemm_fc1', 'gemm_fc2']
FUSED_CLS = ['ln_gemm_qkv', 'attention', 'gemm_proj', 'layernorm', 'gemm_fc1', 'gemm_fc2']      # the last block on the class rows: norm2 stands alone
SEVEN = ['layernorm', 'gemm_qkv', 'attention', 'gemm_proj', 'layernorm', 'gemm_fc1', 'gemm_fc2']
TAIL = ['layernorm', 'gemm_head', 'event_gap']


def expected(depth, fused, cls_rows):
    if not fused:
        return HEAD + SEVEN * depth + TAIL                    # the class-row branch launches the same seven kinds
    return HEAD + FUSED * (depth - 1) + (FUSED_CLS if cls_rows else FUSED) + TAIL


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    assert torch.cuda.is_available(), 'GPU tests need the MI355X box'
    diff_vit_amd.engine.lib()
    return diff_vit_amd


@pytest.fixture(scope='module')
def plan(dva, micro):
    return dva.FrozenPlan(micro['arch'], micro['sd'], micro['calib'])


def _kinds(pl, x, bits):
    return [k for k, _ in pl.profile(x, bits)]


def _kinds_begin_end(E, pl, x, bits):
    """the same through p2v_forward_profile_begin / _end"""
    L = E.lib()
    B, n_max = x.shape[0], 7 * pl.depth + 10
    ws = pl.workspace(B)
    out = torch.empty(B, pl.arch['num_classes'], dtype=torch.float32, device=x.device)
    cfg = (C.c_int8 * len(bits))(*bits)
    tok, ms, kind = C.c_void_p(), (C.c_float * n_max)(), (C.c_int32 * n_max)()
    E.check(L.p2v_forward_profile_begin(pl._handle, E.ptr(x), B, cfg, len(bits), E.ptr(out), E.ptr(ws), ws.numel(), E.stream_ptr(), C.byref(tok)))
    n = L.p2v_forward_profile_end(tok, ms, kind, n_max)
    assert 0 < n <= n_max
    return [E.KERNEL_KINDS[kind[i]] for i in range(n)]


SWITCH_SETS = [(dict(), True, 1), (dict(cls_rows=0), True, 0), (dict(ln_gemm=0), False, 1), (dict(ln_gemm=0, cls_rows=0), False, 0),
               (dict(gemm_rows=2), True, 1)]


@pytest.mark.parametrize('switch,fused,cls_rows', SWITCH_SETS, ids=['-'.join('%s=%d' % kv for kv in s[0].items()) or 'default' for s in SWITCH_SETS])
def test_micro_launch_sequence(dva, micro, plan, switch, fused, cls_rows):
    E = dva.engine
    L = E.lib()
    D, Hd = plan.D, plan.hidden
    assert L.p2v_ln_gemm_fusable(E.EPI_REQUANT, D, 3 * D, 0) == 1 and L.p2v_ln_gemm_fusable(E.EPI_GELU, D, Hd, 4096) == 1      # micro is a fused geometry
    assert plan.depth >= 2                                     # so that the last block differs from the others
    x = micro['x_ev'][:2].cuda()
    assert x.shape[0] == 2
    with tuning(L, **switch):
        for bits in ([8] * plan.n_layers, [int(b) for b in micro['g']['bit_qmix']]):
            want = expected(plan.depth, fused, cls_rows)
            assert _kinds(plan, x, bits) == want, (switch, bits[:3])
            assert _kinds_begin_end(E, plan, x, bits) == want, (switch, bits[:3])
    assert len(expected(plan.depth, True, 1)) == 3 + 5 * plan.depth + 1 + 3 and len(expected(plan.depth, False, 0)) == 3 + 7 * plan.depth + 3


def test_unfused_geometry_launch_sequence(dva):
    """the smallest embed_dim p2v_plan_create takes (a multiple of 16 with a head_dim the attention kernels have) for which
    p2v_ln_gemm_fusable returns 0 for qkv and for fc1: seven launches per block with every switch at its default, cls_rows = 1 or 0"""
    E = dva.engine
    L = E.lib()
    HEAD_DIMS = (32, 48, 64, 80, 96, 128)
    dim = heads = None
    for d in range(16, 513, 16):
        hs = [d // hd for hd in HEAD_DIMS if d % hd == 0]
        if hs and L.p2v_ln_gemm_fusable(E.EPI_REQUANT, d, 3 * d, 0) == 0 and L.p2v_ln_gemm_fusable(E.EPI_GELU, d, d, 0) == 0:
            dim, heads = d, max(hs)
            break
    assert dim is not None, 'every width up to 512 is fused: pin the seven-launch block through ln_gemm = 0 alone'
    assert L.p2v_ln_gemm_fusable(E.EPI_GELU, dim, dim, 4096) == 0              # a GELU table only adds to the kernel's LDS
    depth, img, patch = 2, 16, 8
    arch = dict(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=10, mlp_ratio=1.0)
    m = dva.VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, num_classes=10, mlp_ratio=1.0,
                              qkv_bias=True, norm_layer=partial(dva.QIntLayerNorm, eps=1e-6), input_quant=True, cfg=dva.Config())
    m.load_state_dict(dva.synth.vit_state_dict(arch, 41), strict=False)
    m = m.cuda().eval()
    dva.harness.calibrate_model(m, dva.synth.images(41, 2, img).cuda())
    x = dva.synth.images(41, 2, img, offset=300).cuda()
    bits = [8] * (4 * depth + 2)
    m(x, bits, False)                                           # freezes the plan
    pl = m._plan
    assert pl.D == dim and pl.hidden == dim
    for cr in (1, 0):
        with tuning(L, cls_rows=cr):
            assert _kinds(pl, x, bits) == expected(depth, False, cr), cr
