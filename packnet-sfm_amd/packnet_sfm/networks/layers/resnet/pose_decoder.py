"""The monodepth2-style pose decoder on the gfx950 kernels.

Stands in for the reference's packnet_sfm/networks/layers/resnet/pose_decoder.py: PoseDecoder(num_ch_enc, num_input_features,
num_frames_to_predict_for, stride), `forward(list of feature lists)` -> (axisangle, translation), each [B, frames, 1, 3].  State-dict
contract: `net` is a ModuleList of four nn.Conv2d -- a 1x1 squeeze to 256 channels, two 3x3 convolutions, a 1x1 head with 6 outputs
per frame -- `net.{0..3}.{weight, bias}`.  They are parameter containers: the convolutions are the MFMA kernels with their bias, the
ReLUs behind the first three are HF.act_crop without a crop (no normalisation precedes them).
"""
import torch
import torch.nn as nn

from packnet_sfm.hip import functional as HF
from packnet_sfm.hip import ops as _ops


class PoseDecoder(nn.Module):
    def __init__(self, num_ch_enc, num_input_features, num_frames_to_predict_for=None, stride=1):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("PoseDecoder(stride=%d) is not implemented on the gfx950 kernels: stride 1 only" % stride)
        frames = num_input_features - 1 if num_frames_to_predict_for is None else num_frames_to_predict_for
        self.num_ch_enc, self.num_input_features, self.num_frames_to_predict_for = num_ch_enc, num_input_features, frames
        # (key, channels in, channels out, kernel size, followed by a ReLU)
        table = (('squeeze', int(num_ch_enc[-1]), 256, 1, True), (('pose', 0), num_input_features * 256, 256, 3, True),
                 (('pose', 1), 256, 256, 3, True), (('pose', 2), 256, 6 * frames, 1, False))
        self.convs = {key: nn.Conv2d(cin, cout, k, 1, k // 2) for key, cin, cout, k, _ in table}
        self.net = nn.ModuleList(self.convs.values())
        self._relu = [r for *_, r in table]
        self._packed = [HF.PackedConvWeight() for _ in table]

    def _layer(self, k, x):
        y = HF.conv2d(x, self.net[k].weight, self.net[k].bias, self._packed[k])
        return HF.act_crop(y, 0, _ops.ACT_RELU) if self._relu[k] else y

    def forward(self, input_features):
        squeezed = [self._layer(0, feats[-1]) for feats in input_features]
        x = squeezed[0] if len(squeezed) == 1 else torch.cat(squeezed, 1)
        for k in (1, 2, 3):
            x = self._layer(k, x)
        vec = 0.01 * x.mean(3).mean(2).view(-1, self.num_frames_to_predict_for, 1, 6)
        return vec[..., :3], vec[..., 3:]


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
