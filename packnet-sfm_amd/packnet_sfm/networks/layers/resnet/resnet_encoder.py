"""ResNet encoder (monodepth2-style: torchvision's ResNet18 / 34 body, five feature maps) on the gfx950 kernels.

Drop-in for the reference's packnet_sfm/networks/layers/resnet/resnet_encoder.py: same constructor, same `forward(image)` -> list of
five feature maps, same parameter and buffer names and shapes as the reference has with torchvision underneath
(encoder.{conv1, bn1, layer{1..4}.{i}.{conv1, bn1, conv2, bn2, downsample.{0, 1}}, fc}.*), so its checkpoints load.  torchvision is
NOT imported here: `ResNet` / `BasicBlock` below are parameter containers with torchvision's attribute names (nn.Conv2d / nn.BatchNorm2d /
nn.Linear objects hold the parameters only).  The unused `fc` is part of torchvision's state dict and is kept; it never receives a
gradient.

Execution: the MFMA convolutions (csrc/conv2d.hip; stride 2 for conv1, layer{2,3,4}.0.conv1 and the 1x1 downsample), the fused dense
BatchNorm (+ residual add, + ReLU), the 3x3 stride-2 max pooling and the input normalisation of csrc/resnet.h.  In a stride-1 block the
input feeds conv1 AND the residual: conv1 takes it with a gradient tap (HF.conv2d_tap), so the two gradients are added inside the
backward-data launch.  The stride-2 convolutions inside the blocks (up to 256 -> 512 channels onto a 6x20 map at KITTI's size) take their
weight gradient through the stride-1 kernel on the zero-upsampled gradient (HF.conv2d_stride2(wgrad_s1=True)): the strided
weight-gradient kernel cannot hold such a layer's patch in LDS.

fp16 (evaluation / inference, eval mode only): BatchNorm, residual, ReLU and the input normalisation are folded into the convolutions
(HF.conv2d_h16_fused, csrc/conv2d_h16g.h): the stem is one launch, a BasicBlock two, or three with its stride-2 shortcut.

Initialisation: the distributions of the reference (convolutions kaiming-normal over fan-out, BatchNorm 1 / 0, fc at nn.Linear's
default), created in torchvision's order; parity of the random stream with torchvision itself is not pinned by a test.
"""
import numpy as np
import torch
import torch.nn as nn

from packnet_sfm.hip import functional as HF
from packnet_sfm.hip import ops as _ops


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride
        self._packed = [HF.PackedConvWeight() for _ in range(3)]

    def _forward_h16(self, x):
        """fp16 eval: conv1 + bn1 + ReLU | the 1x1 shortcut + its bn | conv2 + bn2 + residual + ReLU, one launch each."""
        out = HF.conv2d_h16_fused(x, self.conv1.weight, self._packed[0], stride=self.stride, bn=self.bn1, act=_ops.ACT_RELU)
        if self.downsample is not None:
            conv, bn = self.downsample[0], self.downsample[1]
            x = HF.conv2d_h16_fused(x, conv.weight, self._packed[2], stride=conv.stride[0], bn=bn)
        return HF.conv2d_h16_fused(out, self.conv2.weight, self._packed[1], bn=self.bn2, res=x, act=_ops.ACT_RELU)

    def forward(self, x):
        if x.dtype == torch.float16:
            return self._forward_h16(x)
        if self.stride == 1:
            out, x = HF.conv2d_tap(x, self.conv1.weight, None, self._packed[0])
        else:
            out = HF.conv2d_stride2(x, self.conv1.weight, None, self._packed[0], wgrad_s1=True)
        out = HF.batchnorm_act(out, self.bn1, _ops.ACT_RELU)
        out = HF.conv2d(out, self.conv2.weight, None, self._packed[1])
        if self.downsample is not None:
            conv, bn = self.downsample[0], self.downsample[1]
            if conv.stride[0] == 2:
                x = HF.conv2d_stride2(x, conv.weight, None, self._packed[2], wgrad_s1=True)
            else:
                x = HF.conv2d(x, conv.weight, None, self._packed[2])
            x = HF.batchnorm_act(x, bn, _ops.ACT_NONE)
        return HF.batchnorm_act(out, self.bn2, _ops.ACT_RELU, res=x)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("ResNet50 (Bottleneck blocks) is not implemented on the gfx950 kernels: versions '18' and '34' only")


def _init_resnet(model):
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


# (planes, stride) of layer1..layer4
_STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))


class ResNet(nn.Module):
    """torchvision.models.ResNet by attribute names (conv1, bn1, relu, maxpool, layer1..4, avgpool, fc), BasicBlock only, built once:
    conv1 takes 3 * num_input_images channels (the reference's ResNetMultiImageInput keeps everything else, `fc` included)."""

    def __init__(self, block, layers, num_classes=1000, num_input_images=1):
        super().__init__()
        self.conv1 = nn.Conv2d(num_input_images * 3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        width = 64
        for k, ((planes, stride), depth) in enumerate(zip(_STAGES, layers)):
            out = planes * block.expansion
            shortcut = None
            if stride != 1 or width != out:
                shortcut = nn.Sequential(nn.Conv2d(width, out, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(out))
            blocks = [block(width, planes, stride, shortcut)] + [block(out, planes) for _ in range(1, depth)]
            setattr(self, 'layer%d' % (k + 1), nn.Sequential(*blocks))
            width = out
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(width, num_classes)
        self._packed = HF.PackedConvWeight()
        _init_resnet(self)


_BLOCKS = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3]}


def load_imagenet_state_dict(encoder, state_dict, num_input_images=1):
    """Load a torchvision ImageNet ResNet state dict into `encoder` (the ResNet container); with several input images conv1's weight is
    repeated along the input channels and divided by their number (the reference's resnet_multiimage_input)."""
    sd = dict(state_dict)
    if num_input_images > 1:
        sd['conv1.weight'] = torch.cat([sd['conv1.weight']] * num_input_images, 1) / num_input_images
    encoder.load_state_dict(sd)
    return encoder


def _imagenet_state_dict(num_layers):
    try:
        import torchvision.models as models
    except ImportError as e:
        raise ImportError("the 'pt' (ImageNet-pretrained) ResNet versions take their weights from torchvision, which is not installed; "
                          "install torchvision or use the version without the 'pt' suffix and load a checkpoint") from e
    ctor = getattr(models, 'resnet%d' % num_layers)
    try:
        return ctor(weights='IMAGENET1K_V1').state_dict()
    except TypeError:                       # older torchvision
        return ctor(pretrained=True).state_dict()


class ResnetEncoder(nn.Module):
    def __init__(self, num_layers, pretrained, num_input_images=1):
        super().__init__()
        self.num_ch_enc = np.array([64, 64, 128, 256, 512])
        if num_layers in (50, 101, 152):
            raise NotImplementedError("ResNet%d (Bottleneck blocks) is not implemented on the gfx950 kernels: versions '18' and '34' only"
                                      % num_layers)
        if num_layers not in _BLOCKS:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers))
        if num_input_images > 1 and num_layers != 18:
            raise AssertionError("Can only run with 18 or 50 layer resnet")          # the reference's rule for multi-image encoders
        self.encoder = ResNet(BasicBlock, _BLOCKS[num_layers], num_input_images=num_input_images)
        if pretrained:
            load_imagenet_state_dict(self.encoder, _imagenet_state_dict(num_layers), num_input_images)

    def _forward_h16(self, image):
        """fp16 eval: the stem ((x - 0.45) / 0.225 while staging, 7x7 stride 2, bn1, ReLU) in one launch, the max pooling in one, three
        per block with a shortcut convolution and two per block without: 21 launches for ResNet18."""
        e = self.encoder
        stem = HF.conv2d_h16_fused(image, e.conv1.weight, e._packed, stride=2, bn=e.bn1, act=_ops.ACT_RELU,
                                   pre_affine=(1.0 / 0.225, -0.45 / 0.225))
        self.features = [stem, e.layer1(HF.maxpool3x3s2(stem))]
        for layer in (e.layer2, e.layer3, e.layer4):
            self.features.append(layer(self.features[-1]))
        return self.features

    def forward(self, input_image):
        e = self.encoder
        h16_in, h16_net = input_image.dtype == torch.float16, e.conv1.weight.dtype == torch.float16
        if h16_in or h16_net:
            # decided here, before any kernel or library call: pose networks and batch statistics have no fp16 path
            if e.conv1.weight.shape[1] != 3:
                raise NotImplementedError('the multi-image ResnetEncoder (PoseResNet) has no fp16 path: fp16 covers the evaluation / '
                                          'inference forward of the depth networks; run it in float32')
            if not h16_net:
                raise RuntimeError('%s input into a %s network: convert the network with .half() / .to(dtype=torch.float16)'
                                   % (input_image.dtype, e.conv1.weight.dtype))
            if not h16_in:
                raise RuntimeError('%s input into a float16 network: cast the input with .half()' % input_image.dtype)
            if self.training:
                raise NotImplementedError('ResnetEncoder in fp16 runs in eval mode only (BatchNorm with running statistics): call '
                                          '.eval() for evaluation / inference, train in float32')
            return self._forward_h16(input_image)
        self.features = []
        x = HF.affine(input_image, 1.0 / 0.225, -0.45 / 0.225)
        x = HF.conv2d_stride2(x, e.conv1.weight, None, e._packed)
        self.features.append(HF.batchnorm_act(x, e.bn1, _ops.ACT_RELU))
        self.features.append(e.layer1(HF.maxpool3x3s2(self.features[-1])))
        self.features.append(e.layer2(self.features[-1]))
        self.features.append(e.layer3(self.features[-1]))
        self.features.append(e.layer4(self.features[-1]))
        return self.features


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
