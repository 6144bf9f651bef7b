"""PoseResNet (monodepth2-style two-frame ResNet18 encoder + pose decoder -> 6-DoF per context frame) on the gfx950 kernels.

Stands in for the reference's packnet_sfm/networks/pose/PoseResNet.py: PoseResNet(version='18', with the 'pt' suffix for ImageNet
weights from torchvision), `forward(target_image, ref_imgs)` -> [B, len(ref_imgs), 6], translation first, then the axis-angle;
parameters and buffers under encoder.encoder.* and decoder.net.*.  The encoder runs once per context frame on the 6-channel pair
(BatchNorm statistics are per call, as in the reference); of the decoder's two predicted frames the first is the pair's pose.
"""
import torch
import torch.nn as nn

from packnet_sfm.networks.layers.resnet.pose_decoder import PoseDecoder
from packnet_sfm.networks.layers.resnet.resnet_encoder import ResnetEncoder
from packnet_sfm.networks.layers.resnet.versions import parse_version


class PoseResNet(nn.Module):
    def __init__(self, version=None, **kwargs):
        super().__init__()
        layers, pretrained = parse_version(version, 'PoseResNet')
        self.encoder = ResnetEncoder(layers, pretrained, num_input_images=2)
        self.decoder = PoseDecoder(self.encoder.num_ch_enc, num_input_features=1, num_frames_to_predict_for=2)

    def _pair(self, target, ref):
        rot, trans = self.decoder([self.encoder(torch.cat((target, ref), 1))])
        return torch.cat((trans[:, 0], rot[:, 0]), 2)                  # [B, 1, 6]

    def forward(self, target_image, ref_imgs):
        if any(t.dtype == torch.float16 for t in [target_image, self.encoder.encoder.conv1.weight] + list(ref_imgs)):
            raise NotImplementedError('PoseResNet has no fp16 path: fp16 covers the evaluation / inference forward of the depth networks '
                                      '(pose is not part of it); run it in float32')
        return torch.cat([self._pair(target_image, ref) for ref in ref_imgs], 1)


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
