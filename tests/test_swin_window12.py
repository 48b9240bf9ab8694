"""CPU: the patch 4 / window 12 Swin geometry (9 x 9 ... 12 x 12 windows) on the module surface, the factories and the C entry's bound."""
import ctypes

import pytest
import torch


def test_swin_micro_window12_oracle_equals_module_fake_quant_graph(synth):
    """swin_micro_patch4_window12_96 (24 x 24 tokens in four shifted 12 x 12 windows, then 12 x 12 as one window without shift):
    OracleSwin == the module surface executed op by op in torch fake-quant mode, as for the window-7 micro model."""
    import diff_vit_amd as dva
    from diff_vit_amd import swin
    import swin_oracle as SO
    m = swin.swin_micro_patch4_window12_96(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    assert m.arch['img_size'] == 96 and m.arch['window_size'] == 12 and m.arch['depths'] == (2, 2) and m.arch['num_heads'] == (2, 4)
    m.load_state_dict(synth.swin_state_dict(m.state_dict(), 5))
    x = synth.images(5, 3, 96)
    with torch.no_grad():
        fp = m(x)
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
        m.model_quant()
        y_mod = m.act_out(m.head(m.forward_features(x)))           # the op-by-op fake-quant graph (not the product path)
        y_or = SO.OracleSwin(m.arch, m.state_dict()).quant_forward(x, m.export_calib(), 8)
    assert fp.shape == (3, 10)
    assert torch.equal(y_mod, y_or)
    assert float((y_or[0] - y_or[1]).abs().max()) > 0              # not degenerate
    with pytest.raises(RuntimeError):                              # the product path has no CPU fallback
        m(x)


@pytest.mark.parametrize('name,embed,heads,last', [('swin_base_patch4_window12_384', 128, (4, 8, 16, 32), 1024),
                                                   ('swin_large_patch4_window12_384', 192, (6, 12, 24, 48), 1536)])
def test_window12_384_factories(name, embed, heads, last):
    """the two real factories: architecture, head_dim 32 in every stage, and the package exports them (built on the meta device: no weights)"""
    import diff_vit_amd as dva
    from diff_vit_amd import swin
    assert getattr(dva, name) is getattr(swin, name) and name in dva.__all__
    with torch.device('meta'):
        m = getattr(swin, name)()
    assert m.arch == dict(img_size=384, patch_size=4, embed_dim=embed, depths=(2, 2, 18, 2), num_heads=heads, window_size=12,
                          mlp_ratio=m.arch['mlp_ratio'], num_classes=1000)
    assert all(embed * 2 ** i // h == 32 for i, h in enumerate(heads))
    assert m.norm.weight.shape == (last,) and last <= 2048          # the final LayerNorm stays inside the kernel's channel limit
    assert getattr(swin, name).__name__ == name
    assert getattr(swin, name)(depths=(1, 1, 1, 1), num_classes=3, img_size=96).arch['window_size'] == 12      # kwargs still override


def test_window12_pretrained_has_no_file_and_never_fetches():
    """pretrained=True for the new names: what checkpoint.load_pretrained does for any name it has no file for"""
    from diff_vit_amd import checkpoint, swin
    with pytest.raises(KeyError):
        checkpoint.load_pretrained(None, 'no_such_factory')
    for name in ('swin_base_patch4_window12_384', 'swin_large_patch4_window12_384'):
        assert name not in checkpoint.PRETRAINED_FILES
    with pytest.raises(KeyError):
        swin.swin_micro_patch4_window12_96(pretrained=True, num_classes=3)


def test_str2model_names():
    import diff_vit_amd as dva
    from diff_vit_amd import swin
    assert dva.harness.str2model('swin_base_384') is swin.swin_base_patch4_window12_384
    assert dva.harness.str2model('swin_large_384') is swin.swin_large_patch4_window12_384
    assert dva.harness.str2model('swin_base') is swin.swin_base_patch4_window7_224


def test_window_attention_refuses_windows_beyond_12_without_gpu():
    """p2v_window_attention: ws = 13 is a shape error before any HIP call, and the message names the bound"""
    import diff_vit_amd
    E = diff_vit_amd.engine
    L = E.lib()
    one = ctypes.c_void_p(16)
    for ws in (13, 0):
        wa = E.WinAttn(2.0 ** -4, 0.1767767, 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, -12, 43, 714, one, one, None, ws, 1)
        with pytest.raises(AssertionError):
            E.check(L.p2v_window_attention(one, 1, 4096, 4, 32, ctypes.byref(wa), one, None, None))
        assert b'1..12' in L.p2v_last_error()
    wa = E.WinAttn(2.0 ** -4, 0.1767767, 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -3, -12, 43, 714, one, one, None, 12, 2)
    with pytest.raises(AssertionError):                            # two 12 x 12 windows do not fit 196 tokens
        E.check(L.p2v_window_attention(one, 1, 196, 4, 32, ctypes.byref(wa), one, None, None))
