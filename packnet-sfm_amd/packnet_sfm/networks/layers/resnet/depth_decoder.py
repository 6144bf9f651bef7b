"""The monodepth2-style depth decoder on the gfx950 kernels.

Stands in for the reference's packnet_sfm/networks/layers/resnet/depth_decoder.py: DepthDecoder(num_ch_enc, scales, num_output_channels,
use_skips), `forward(features)` -> {('disp', i): map}.  State-dict contract: `decoder` is a ModuleList whose entries 0..9 are the
ConvBlocks of levels 4..0 (two per level: `conv.conv.{weight, bias}`) and whose following entries are the disparity heads of `scales`
(`conv.{weight, bias}`).  The layers are built from a table of (kind, level, channels in, channels out); `self.convs` maps
('upconv', level, 0 | 1) and ('dispconv', scale) to them as the reference's dictionary does.
`disp_range = (a, b)` makes the outputs a + b * sigmoid(.) instead of the plain sigmoid: DepthResNet sets it to its depth range, so the
scaling costs no launch.
"""
import torch.nn as nn

from packnet_sfm.hip import ops as _ops
from packnet_sfm.networks.layers.resnet.layers import ConvBlock, Conv3x3

_WIDTHS = (16, 32, 64, 128, 256)          # decoder channels of levels 0..4


def _layer_table(enc, scales, heads, use_skips):
    rows = []
    for level in range(4, -1, -1):
        cin = int(enc[-1]) if level == 4 else _WIDTHS[level + 1]
        skip = int(enc[level - 1]) if (use_skips and level > 0) else 0
        rows.append((('upconv', level, 0), cin, _WIDTHS[level]))
        rows.append((('upconv', level, 1), _WIDTHS[level] + skip, _WIDTHS[level]))
    return rows + [(('dispconv', s), _WIDTHS[s], heads) for s in scales]


class DepthDecoder(nn.Module):
    def __init__(self, num_ch_enc, scales=range(4), num_output_channels=1, use_skips=True):
        super().__init__()
        self.num_ch_enc, self.scales, self.num_output_channels, self.use_skips = num_ch_enc, scales, num_output_channels, use_skips
        self.num_ch_dec = list(_WIDTHS)
        self.disp_range = (0.0, 1.0)
        self.convs = {key: (ConvBlock if key[0] == 'upconv' else Conv3x3)(cin, cout)
                      for key, cin, cout in _layer_table(num_ch_enc, scales, num_output_channels, use_skips)}
        self.decoder = nn.ModuleList(self.convs.values())

    def forward(self, input_features):
        self.outputs = {}
        x = input_features[-1]
        for level in range(4, -1, -1):
            x = self.convs[('upconv', level, 0)](x)
            skip = input_features[level - 1] if (self.use_skips and level > 0) else None
            # up-sampling, concatenation and reflection pad: one pad launch per source, into one tensor
            x = self.convs[('upconv', level, 1)](x if skip is None else (x, skip), up=2 if skip is None else (2, 1))
            if level in self.scales:
                self.outputs[('disp', level)] = self.convs[('dispconv', level)](x, act=_ops.ACT_DISP, disp=self.disp_range)
        return self.outputs


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
