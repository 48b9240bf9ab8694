"""Shared by tests/test_swin_bits.py and tests/test_swin_bits_gpu.py: the calibrated micro Swin and the MIXED oracle.

OracleSwin.quant_forward takes one width for the model.  A per-layer list is checked against it by substitution: a layer at 4 bits gets
its weight replaced by its own 4-bit fake-quantised value codes4 * s4 and its 'int8' scale replaced by s4; the 8-bit oracle then derives
exactly codes4 again (the scales are powers of two, so codes4 * s4 and the division by s4 are exact, and |codes4| <= 8 is inside the 8-bit
clamp) and multiplies by s4: the layer computes what the 4-bit oracle computes for it."""
import torch


def micro_swin(dva, factory='swin_micro_patch4_window7_56', img=56, n_images=3):
    """(model calibrated on the first two images and switched to quant state, images)"""
    from diff_vit_amd import swin
    m = getattr(swin, factory)(cfg=dva.Config(True, True, 'minmax'), num_classes=10).eval()
    m.load_state_dict(dva.synth.swin_state_dict(m.state_dict(), 5))
    x = dva.synth.images(11, n_images, img)
    with torch.no_grad():
        m.model_open_calibrate(); m.model_open_last_calibrate(); m(x[:2]); m.model_close_calibrate()
    m.model_quant()
    return m, x


def substituted(m, bit_list):
    """(state dict, calib) under which OracleSwin.quant_forward(x, calib, 8) computes the per-layer widths ``bit_list``"""
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    calib = {k: (dict(v) if isinstance(v, dict) else v) for k, v in m.export_calib().items()}
    names = m.bit_config_names()
    assert len(names) == len(bit_list)
    for name, b in zip(names, bit_list):
        assert b in (4, 8)
        if b == 4:
            s4 = calib[name]['int4'].reshape(-1)
            w = sd[name + '.weight']
            codes = torch.clamp(torch.round(w.reshape(w.shape[0], -1) / s4.reshape(-1, 1)), -8, 7)
            sd[name + '.weight'] = (codes * s4.reshape(-1, 1)).reshape(w.shape)
            calib[name]['int8'] = s4
    return sd, calib


def mixed_oracle(m, x, bit_list):
    import swin_oracle as SO
    sd, calib = substituted(m, bit_list)
    with torch.no_grad():
        return SO.OracleSwin(m.arch, sd).quant_forward(x, calib, 8)


def uniform_oracle(m, x, bits):
    import swin_oracle as SO
    with torch.no_grad():
        return SO.OracleSwin(m.arch, {k: v.detach().cpu() for k, v in m.state_dict().items()}).quant_forward(x, m.export_calib(), bits)


def bit_lists(L, seeds=(1, 2)):
    """the lists the engine is checked on: uniform, alternating, seeded random ones, and every single-4 list"""
    import random
    lists = [[8] * L, [4] * L, [8 if i % 2 == 0 else 4 for i in range(L)]]
    for s in seeds:
        r = random.Random(s)
        lists.append([r.choice((4, 8)) for _ in range(L)])
    lists += [[4 if j == i else 8 for j in range(L)] for i in range(L)]
    return lists
