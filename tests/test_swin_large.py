"""CPU: the widths only Swin-L has.  A test-only micro architecture reaches the 3072-channel PatchMerging LayerNorm (4 x 768) with
few parameters: embed_dim 768, depths (1, 1), heads (24, 48), 32^2 images, window 4, mlp_ratio 1 - an 8 x 8 map in four windows, the
merge LayerNorm over 16 rows of 3072 channels per image, then 1536 channels in one window.  Built through the keyword overrides of the
public factory; tests/test_swin_large_gpu.py runs the same model on the engine."""
import functools

import torch

LARGE_MICRO = dict(embed_dim=768, depths=(1, 1), num_heads=(24, 48), img_size=32, window_size=4, mlp_ratio=1.0, num_classes=10)


@functools.lru_cache(maxsize=None)
def large_micro(seed=5):
    """-> (calibrated and quantized module on the CPU, 4 images); calibrated on the first two"""
    import diff_vit_amd as dva
    m = dva.swin.swin_large_patch4_window12_384(cfg=dva.Config(True, True, 'minmax'), **LARGE_MICRO).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), seed))
    x = dva.synth.images(seed, 4, 32)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
        m.model_quant()
    return m, x


def test_large_micro_oracle_equals_module_fake_quant_graph():
    """OracleSwin == the module surface executed op by op in torch fake-quant mode, at 768 -> 3072 -> 1536 channels"""
    import swin_oracle as SO
    m, x = large_micro()
    assert m.arch == dict(LARGE_MICRO, patch_size=4)
    assert m.layers[0].downsample.norm.weight.shape == (3072,) and m.layers[0].downsample.reduction.weight.shape == (1536, 3072)
    assert m.norm.weight.shape == (1536,)
    with torch.no_grad():
        y_mod = m.act_out(m.head(m.forward_features(x[:3])))            # the op-by-op fake-quant graph (not the product path)
        taps = {}
        y_or = SO.OracleSwin(m.arch, m.state_dict()).quant_forward(x[:3], m.export_calib(), 8, taps)
    assert torch.equal(y_mod, y_or)
    assert float((y_or[0] - y_or[1]).abs().max()) > 0                  # not degenerate
    q = taps['layers.0.downsample.qact1']
    assert q.reshape(3, -1, 3072).shape[1] == 16 and float(q.float().std()) > 4.0     # the 3072-wide LayerNorm's codes use their range
    # the exact-statistics bound of the engine's LayerNorm holds for this model's PTF scales (SwinPlan._ln checks the same)
    s = m.export_calib()['layers.0.blocks.0.qact4'].reshape(-1)
    assert 3072 * (128.0 * float(torch.round(s / s.min()).max())) ** 2 < 2.0 ** 32
