"""CPU: the Swin model diff surface without a GPU - the stage list, compute_ddv on the module graph (float and fake-quant) against a numpy
restatement of the reference's compute_ddv, and the refusals of the new p2v_run_ops records before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def dva():
    import diff_vit_amd
    return diff_vit_amd


def hooked_numpy(model, x, names):
    """the outputs of the named modules on the module graph, one row per image (window modules run on [B * nW, ...], image-major)"""
    mods = dict(model.named_modules())
    got = {}
    hooks = [mods[nm].register_forward_hook(lambda m, i, o, nm=nm: got.__setitem__(nm, o.detach())) for nm in names]
    with torch.no_grad():
        model.act_out(model.head(model.forward_features(x)))
    for h in hooks:
        h.remove()
    return {nm: got[nm].reshape(x.shape[0], -1).double().cpu().numpy() for nm in names}


def reference_ddv(normal, adv):
    """modeldiff_p2.py:101-113 in numpy, fp64: per sample the dot product of the two normalised activations, the vector over the samples
    divided by its norm when that is not zero"""
    out = {}
    for key in normal:
        ddv = []
        for ya, yb in zip(normal[key], adv[key]):
            ya, yb = ya.flatten(), yb.flatten()
            ddv.append(np.dot(ya / np.linalg.norm(ya), yb / np.linalg.norm(yb)))
        ddv = np.array(ddv)
        norm = np.linalg.norm(ddv)
        out[key] = ddv / norm if norm != 0 else ddv
    return out


def test_swin_stage_names_counts_and_order(dva):
    D = dva.ddv
    for depths in ((2, 2), (2, 2, 6, 2), (2, 2, 18, 2), (1, 1)):
        blocks, merges = sum(depths), len(depths) - 1
        plain, lin = D.swin_stage_names(depths, False), D.swin_stage_names(depths, True)
        assert len(plain) == 9 * blocks + 2 * merges + 5 and len(set(plain)) == len(plain)
        assert len(lin) == len(plain) + 4 * blocks + merges + 2 and [n for n in lin if n in set(plain)] == plain
    assert len(D.swin_stage_names((2, 2), False)) == 43
    names = D.swin_stage_names((1, 1), True)
    p = 'layers.0.blocks.0.'
    assert names[:3] == ['patch_embed.proj', 'patch_embed.qact_before_norm', 'patch_embed.qact']
    assert names[3:16] == [p + k for k in ('qact1', 'attn.qkv', 'attn.qact1', 'attn.qact3', 'attn.proj', 'attn.qact4', 'qact2', 'qact3', 'mlp.fc1',
                                           'mlp.qact1', 'mlp.fc2', 'mlp.qact2', 'qact4')]
    assert names[16:19] == ['layers.0.downsample.qact1', 'layers.0.downsample.reduction', 'layers.0.downsample.qact2']
    assert names[-4:] == ['qact2', 'qact3', 'head', 'act_out']
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10)
    mods = dict(m.named_modules())
    assert all(n in mods for n in D.swin_stage_names(m.arch['depths'], True))


def test_compute_ddv_cpu_swin_float_and_fake_quant(dva):
    """fp64 sums over F <= 2^18 features in two orders differ by at most 2 F 2^-53 < 1e-10 relative to sqrt(aa bb): 1e-9 on the DDV"""
    S = dva.synth
    m = dva.swin.swin_micro_patch4_window7_56(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m.load_state_dict(S.swin_state_dict(m.state_dict(), 5))
    x = S.images(11, 3, 56)
    xa = x + 0.25 * S.images(12, 3, 56)
    names = dva.ddv.swin_stage_names(m.arch['depths'], True)
    with pytest.raises(NotImplementedError):
        dva.compute_ddv(m, x, xa, [8] * 10)
    for state in ('float', 'quant'):
        if state == 'quant':
            with torch.no_grad():
                m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
                m.model_quant()
        d = dva.compute_ddv(m, x, xa, None if state == 'float' else 8)
        assert list(d) == names and all(v.dtype == torch.float64 and v.shape == (3,) and bool(torch.isfinite(v).all()) for v in d.values())
        want = reference_ddv(hooked_numpy(m, x, names), hooked_numpy(m, xa, names))
        for nm in names:
            assert float(np.abs(d[nm].numpy() - want[nm]).max()) <= 1e-9, (state, nm)
        d0 = dva.compute_ddv(m, x, xa, None if state == 'float' else 8, with_linear=False)
        assert list(d0) == dva.ddv.swin_stage_names(m.arch['depths'], False) and all(torch.equal(v, d[nm]) for nm, v in d0.items())


def test_new_records_refuse_before_any_hip_call(dva):
    """P2V_OP_COS / P2V_OP_COS_COMBINE / P2V_OP_GEMM_F32 and the stage-record builder reject bad records on the host (no GPU here)"""
    E = dva.engine
    L = E.lib()
    one = ctypes.c_void_p(256)

    def run(o):
        return L.p2v_run_ops((E.Op * 1)(o), 1, None)

    def cos(**kw):
        o = E.Op()
        o.kind, o.inp, o.out = E.OP_COS, one, one
        o.i0, o.i1, o.M, o.N, o.lda, o.i2 = 2, E.COS_I8, 4, 64, 64, 256
        o.lin.w_codes = one
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert run(cos(inp=ctypes.c_void_p(264))) == E.E_ARG and b'multiples of 16' in L.p2v_last_error()      # misaligned buffer
    assert run(cos(lda=72, N=64)) == E.E_ARG and b'multiples of 16' in L.p2v_last_error()                    # misaligned row stride
    assert run(cos(i2=264)) == E.E_ARG                                                                      # misaligned sample stride
    assert run(cos(i0=0)) == E.E_SHAPE                                                                      # n < 1
    assert run(cos(M=1 << 20, N=1 << 19, lda=1 << 19, i2=0, i3=1 << 7)) == E.E_UNSUPPORTED                  # rows * cols >= 2^39
    assert run(cos(i1=2)) == E.E_ARG                                                                        # unknown dtype
    assert run(cos(inp=None)) == E.E_ARG
    o = cos()
    o.lin.w_codes = None
    assert run(o) == E.E_ARG                                                                                # no stage record
    o = cos(i1=E.COS_F32)
    o.lin.colscale = one
    assert run(o) == E.E_UNSUPPORTED                                                                        # scales go with int8
    oc = E.Op()
    oc.kind, oc.inp, oc.out, oc.i0, oc.i1 = E.OP_COS_COMBINE, one, one, 2, 0
    oc.lin.w_codes = one
    assert run(oc) == E.E_ARG and b'without stages' in L.p2v_last_error()
    oc.i1, oc.i0 = 3, 0
    assert run(oc) == E.E_SHAPE
    og = E.Op()
    og.kind, og.inp, og.out = E.OP_GEMM_F32, one, one
    og.M, og.K, og.N, og.lda, og.ldo = 4, 96, 32, 96, 32
    og.lin = E.Linear(one, one, one, None, 0)
    assert run(og) == E.E_SHAPE                                                                             # K no multiple of 64
    og.K, og.ldo = 128, 34
    assert run(og) == E.E_SHAPE
    og.ldo, og.out = 32, ctypes.c_void_p(260)
    assert run(og) == E.E_ARG
    o99 = E.Op()
    o99.kind = 99
    assert run(o99) == E.E_ARG and b'unknown op kind' in L.p2v_last_error()
    # the stage-record builder applies p2v_pair_cosine's rules
    assert L.p2v_cos_stage_desc_bytes() > 0
    lay = E.CosLayer(one, one, None, 256, 64, 4, 64, E.COS_I8)
    buf = (ctypes.c_char * (4 * L.p2v_cos_stage_desc_bytes()))()
    assert L.p2v_cos_stage_descs((E.CosLayer * 1)(lay), 1, 2, buf) == 2                                      # one split per sample
    assert L.p2v_cos_stage_descs((E.CosLayer * 1)(lay), 1, 0, buf) == E.E_SHAPE
    lay.row_stride = 60
    assert L.p2v_cos_stage_descs((E.CosLayer * 1)(lay), 1, 2, buf) == E.E_ARG
