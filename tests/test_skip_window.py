"""`modules.skip_window`: which channels of a decoder concat [h | skip] the skip-ahead branch may normalise and contract
before h exists -- whole GroupNorm groups of the skip half, whole 32-channel plane chunks.  CPU only.
"""
import math

import torch

from octfusion_amd import configs
from octfusion_amd.graph_unet_union import UNet3DModel
from octfusion_amd.modules import GraphResBlockEmbed, skip_window


def _decoder_windows(config, stage):
    """[(c_h, c_skip, groups, window)] of every decoder res block of a config's net, in execution order."""
    with torch.device('meta'):
        net = UNet3DModel(**configs.unet_params(config, stage))
    hr = getattr(net, 'unet_' + stage)
    blocks = [m for m in hr.output_blocks if isinstance(m, GraphResBlockEmbed)]
    plan = list(reversed(hr._cat_plan))
    assert len(blocks) == len(plan)
    out = []
    for m, (c_h, c_skip, _) in zip(blocks, plan):
        assert m.channels == c_h + c_skip
        out.append((c_h, c_skip, m.block1_norm.group, skip_window(c_h, c_skip, m.block1_norm.group)))
    return out


def test_shipped_config_gives_the_five_windows():
    got = {(c_h, c_skip): win for c_h, c_skip, _, win in _decoder_windows('snet_uncond', 'hr') if win is not None}
    assert got == {(256, 256): (256, 512), (512, 256): (576, 768), (256, 128): (288, 384), (128, 128): (128, 256)}
    # five blocks take them: 256 + 128 occurs at two depths
    wins = [w for _, _, _, w in _decoder_windows('snet_uncond', 'hr') if w is not None]
    assert sorted(wins) == sorted([(256, 512), (576, 768), (288, 384), (288, 384), (128, 256)])


def test_none_when_nothing_remains():
    assert skip_window(64, 32, 32) is None            # 3 channels per group: lcm(3, 32) = 96 = the whole concat
    assert skip_window(128, 64, 32) is None           # 6 per group: first boundary at 192
    assert skip_window(96, 16, 28) is None            # 4 per group, 16 channels left: less than one chunk
    assert skip_window(64, 36, 25) is None            # concat not made of whole 32-channel chunks
    assert skip_window(64, 64, 3) is None             # groups do not divide the concat
    assert skip_window(32, 32, 32) == (32, 64)
    assert skip_window(512, 512, 32) == (512, 1024)


def test_windows_are_aligned_for_every_config():
    seen = 0
    for config, stage in (('snet_uncond', 'hr'), ('snet_cond', 'hr'), ('obja_uncond', 'hr'), ('obja_uncond', 'feature')):
        for c_h, c_skip, groups, win in _decoder_windows(config, stage):
            C = c_h + c_skip
            step = math.lcm(C // groups, 32)
            if win is None:
                # nothing aligned remains: the first boundary at or after c_h leaves fewer than 32 channels
                assert C % 32 or C - (c_h + step - 1) // step * step < 32
                continue
            seen += 1
            c_lo, c_hi = win
            assert c_hi == C and c_h <= c_lo < c_hi and c_hi - c_lo >= 32
            assert c_lo % 32 == 0 and c_hi % 32 == 0 and c_lo % (C // groups) == 0 and c_hi % (C // groups) == 0
            assert c_lo - c_h < step                  # the smallest such c_lo
    assert seen >= 10
