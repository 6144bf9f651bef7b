"""The monodepth2-style decoder layers on the gfx950 kernels.

Stands in for the reference's packnet_sfm/networks/layers/resnet/layers.py: `Conv3x3` (reflection pad 1 + 3x3 convolution; parameters
conv.{weight, bias}), `ConvBlock` (Conv3x3 + ELU; parameters conv.conv.{weight, bias}), `upsample` (nearest x2) and `disp_to_depth`.
A Conv3x3 runs as reflect_pad1 -> the zero-pad "same" MFMA convolution on the padded map -> a crop of the one-pixel frame
(HF.conv3x3_reflect); the crop is fused with whatever activation follows, and the 2x up-sampling and the channel concatenation in front
of the decoder's second convolution are folded into the padding kernel.  On fp16 inputs (evaluation / inference) the whole Conv3x3 --
up-sampling, concatenation, reflection pad, convolution, bias and activation -- is ONE launch of the gathering convolution
(HF.conv2d_h16_fused, csrc/conv2d_h16g.h).
"""
import torch.nn as nn

from packnet_sfm.hip import functional as HF
from packnet_sfm.hip import ops as _ops


def disp_range(min_depth, max_depth):
    """(a, b) with scaled disparity = a + b * sigmoid: a = 1 / max_depth, a + b = 1 / min_depth."""
    return 1.0 / max_depth, 1.0 / min_depth - 1.0 / max_depth


def disp_to_depth(disp, min_depth, max_depth):
    """(scaled disparity, depth) of a sigmoid output."""
    a, b = disp_range(min_depth, max_depth)
    scaled = a + b * disp
    return scaled, 1 / scaled


class Conv3x3(nn.Module):
    def __init__(self, in_channels, out_channels, use_refl=True):
        super().__init__()
        if not use_refl:
            raise NotImplementedError("Conv3x3(use_refl=False) is not implemented on the gfx950 kernels")
        self.pad = nn.ReflectionPad2d(1)            # parameter-free; kept for the module tree
        self.conv = nn.Conv2d(int(in_channels), int(out_channels), 3)
        self._packed = HF.PackedConvWeight()

    def forward(self, x, act=_ops.ACT_NONE, up=1, disp=(0.0, 1.0)):
        """x: a tensor, or a tuple standing for the channel concatenation; act / up / disp: see HF.conv3x3_reflect."""
        return HF.conv3x3_reflect(x, self.conv.weight, self.conv.bias, self._packed, act=act, up=up, disp=disp)


class ConvBlock(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = Conv3x3(in_channels, out_channels)
        self.nonlin = nn.ELU(inplace=True)          # parameter-free; the ELU runs inside act_crop

    def forward(self, x, up=1):
        return self.conv(x, act=_ops.ACT_ELU, up=up)


def upsample(x):
    return HF.upsample_nearest(x, scale_factor=2)


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
