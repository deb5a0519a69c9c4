"""The camera image encoder of the lift-splat branch; mirror of ``CamEncode_Resnet101`` (``opencood/models/sub_modules/lss_submodule.py
:140-233``), the one camera encoder the reference's PTQ surface wraps (``QuantCamEncode_Resnet101``).

The reference takes ``conv1 / bn1 / maxpool / layer1 / layer2`` from torchvision's ``resnet101``: the stem and the first two stages, i.e.
3 + 4 bottlenecks of 64 and 128 planes, the stride on ``conv2``.  Here the same modules are built from this plugin's ``resblock.Bottleneck``
under torchvision's attribute names, so the ``state_dict`` keys are the reference's: ``conv1.weight``, ``bn1.*``, ``layer1.N.convK.weight``,
``layer1.N.bnK.*``, ``layer1.0.downsample.0.weight``, ``layer1.0.downsample.1.*``, ``layer2...``, ``depth_head.*``, ``image_head.*``."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...utils.camera_utils import bin_depths
from .resblock import Bottleneck


class TrunkBottleneck(Bottleneck):
    """torchvision's bottleneck: four times ``planes`` out.  Its own attribute, because the Pyramid fusion backbone sets ``Bottleneck.expansion = 1``
    on the shared class (pyramid_fuse.py, as the reference does) and a camera trunk built after it must not shrink."""
    expansion = 4


def _stage(inplanes, planes, blocks, stride):
    """one torchvision ResNet stage of bottlenecks: the first block carries the stride and a 1x1 + BN shortcut"""
    out = planes * TrunkBottleneck.expansion
    shortcut = nn.Sequential(nn.Conv2d(inplanes, out, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(out))
    return nn.Sequential(TrunkBottleneck(inplanes, planes, stride, shortcut), *[TrunkBottleneck(out, planes) for _ in range(1, blocks)])


class CamEncode_Resnet101(nn.Module):
    """images [B*N, 3 | 4, H, W] -> ``(depth items | None, [B*N, C, D, fH, fW])``: the outer product of the depth distribution and the image
    features, as the reference forms it.  ``features_and_depth`` returns the two factors instead; ``LiftSplatShoot`` pools from those."""

    def __init__(self, D, C, downsample, ddiscr, mode, use_gt_depth=False, depth_supervision=True):
        super().__init__()
        self.D, self.C, self.downsample = D, C, downsample
        self.d_min, self.d_max, self.num_bins = ddiscr[0], ddiscr[1], ddiscr[2]
        self.mode, self.use_gt_depth, self.depth_supervision = mode, use_gt_depth, depth_supervision
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU()
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = _stage(64, 64, 3, 1)
        self.layer2 = _stage(256, 128, 4, 2)
        self.layer3 = nn.Identity()
        if not use_gt_depth:
            self.depth_head = nn.Conv2d(512, self.D, kernel_size=1, padding=0)
        self.image_head = nn.Conv2d(512, self.C, kernel_size=1, padding=0)
        for m in self.modules():                                     # torchvision's initialisation, zero_init_residual=True
            if isinstance(m, nn.Conv2d) and m not in (getattr(self, "depth_head", None), self.image_head):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        for m in self.modules():
            if isinstance(m, Bottleneck):
                nn.init.constant_(m.bn3.weight, 0)

    def get_depth_dist(self, x, eps=1e-5):
        return F.softmax(x, dim=1)

    def get_gt_depth_dist(self, x):
        """measured depth [B*N, H, W] -> (one-hot [B*N, D, fH, fW] of the bin of every feature pixel's centre sample, the indices); outside
        training the one-hot of a depth outside the range is cleared"""
        return gt_depth_dist(self, x)

    def resnet101_forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        return self.layer2(self.layer1(x))

    def get_resnet_features(self, x):
        return self.resnet101_forward(x)

    def features_and_depth(self, x):
        return features_and_depth(self, x)

    def forward(self, x):
        return lift(self, x)


def gt_depth_dist(enc, x):
    """``get_gt_depth_dist`` of ``CamEncode_Resnet101`` and of its quantized wrapper (both carry d_min, d_max, num_bins, mode, downsample)"""
    target = enc.training
    x = x.clamp(max=enc.d_max)
    idx, mask = bin_depths(x, enc.mode, enc.d_min, enc.d_max, enc.num_bins, target=target)
    half, step = enc.downsample // 2, enc.downsample
    idx = idx[:, half::step, half::step]
    onehot = F.one_hot(idx.long()).permute(0, 3, 1, 2)
    if not target:
        onehot = onehot * mask[:, half::step, half::step].unsqueeze(1)
    return onehot, idx


def features_and_depth(enc, x):
    """-> (depth items, depth distribution [B*N, D, fH, fW], ``'logits'`` | ``'probs'``, image features [B*N, C, fH, fW]): the two factors of
    the reference's ``new_x`` and how the first is to be read -- the depth head's logits (softmax pending) or the one-hot of the measured depth"""
    trunk = enc.get_resnet_features(x[:, :3, :, :].clone())
    feats = enc.image_head(trunk)
    gt = idx = None
    if enc.depth_supervision or enc.use_gt_depth:                    # the fourth channel must be there
        gt, idx = enc.get_gt_depth_dist(x[:, 3, :, :])
    if enc.use_gt_depth:
        return None, gt.to(feats.dtype), "probs", feats
    logits = enc.depth_head(trunk)
    return ((logits, idx) if enc.depth_supervision else None), logits, "logits", feats


def lift(enc, x):
    items, depth, mode, feats = features_and_depth(enc, x)
    if mode == "logits":
        depth = enc.get_depth_dist(depth)
    return items, depth.unsqueeze(1) * feats.unsqueeze(2)
