"""DepthResNet (monodepth2-style ResNet18 / 34 encoder + skip decoder -> inverse depth) on the gfx950 kernels.

Stands in for the reference's packnet_sfm/networks/depth/DepthResNet.py: DepthResNet(version='18' | '34', with the 'pt' suffix for
ImageNet weights, which come from torchvision -- imported only then), `forward(rgb)` -> {'inv_depths': four scaled disparities in
training mode, the full-resolution one in eval mode}, parameters and buffers under encoder.encoder.* and decoder.decoder.*, so the
model-zoo checkpoints load.  '50' (Bottleneck blocks) raises NotImplementedError.
The depth range (0.1 .. 100 m) is folded into the decoder's output activation: 0.01 + 9.99 sigmoid(.).
In eval mode the network also runs in fp16 (`.half()`, fp16 input): 35 launches of the gathering convolution of csrc/conv2d_h16g.h and one
max pooling for version '18'; fp16 in training mode raises NotImplementedError (call .eval()).
"""
from functools import partial

import torch.nn as nn

from packnet_sfm.networks.layers.resnet.depth_decoder import DepthDecoder
from packnet_sfm.networks.layers.resnet.layers import disp_range, disp_to_depth
from packnet_sfm.networks.layers.resnet.resnet_encoder import ResnetEncoder
from packnet_sfm.networks.layers.resnet.versions import parse_version

MIN_DEPTH, MAX_DEPTH = 0.1, 100.0


class DepthResNet(nn.Module):
    def __init__(self, version=None, **kwargs):
        super().__init__()
        layers, pretrained = parse_version(version, 'DepthResNet')
        self.encoder = ResnetEncoder(layers, pretrained)
        self.decoder = DepthDecoder(self.encoder.num_ch_enc)
        self.decoder.disp_range = disp_range(MIN_DEPTH, MAX_DEPTH)      # the decoder's outputs ARE the scaled disparities
        self.scale_inv_depth = partial(disp_to_depth, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)

    def forward(self, rgb):
        maps = self.decoder(self.encoder(rgb))
        scaled = [maps[('disp', s)] for s in range(4)]
        return {'inv_depths': scaled if self.training else scaled[0]}


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
