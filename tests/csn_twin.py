"""Plain ``torch.nn`` twins of the channel-separated models (resnet.Bottleneck with resnet.Conv3DDepthwise): the same attribute
tree, hence the same ``state_dict`` keys, with every layer a stock torch module that runs on the CPU in any dtype."""
from torch import nn


def _conv_bn(conv, planes, relu):
    return nn.Sequential(*([conv, nn.BatchNorm3d(planes)] + ([nn.ReLU()] if relu else [])))


class TwinBottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv_bn(nn.Conv3d(inplanes, planes, 1, bias=False), planes, True)
        self.conv2 = _conv_bn(nn.Conv3d(planes, planes, 3, stride=stride, padding=1, groups=planes, bias=False), planes, True)
        self.conv3 = _conv_bn(nn.Conv3d(planes, planes * 4, 1, bias=False), planes * 4, False)
        self.relu = nn.ReLU()
        self.downsample = downsample

    def forward(self, x):
        out = self.conv3(self.conv2(self.conv1(x)))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))


def twin_downsample(inplanes, out_planes, stride):
    return _conv_bn(nn.Conv3d(inplanes, out_planes, 1, stride=stride, bias=False), out_planes, False)


class TwinCSN(nn.Module):
    """``resnet.VideoResNet(Bottleneck, [Conv3DDepthwise] * 4, layers, BasicStem)``; ``forward`` returns the pooled features."""

    def __init__(self, layers, num_classes=400):
        super().__init__()
        self.stem = _conv_bn(nn.Conv3d(3, 64, (3, 7, 7), stride=(1, 2, 2), padding=(1, 3, 3), bias=False), 64, True)
        inplanes = 64
        for i, (planes, stride) in enumerate([(64, 1), (128, 2), (256, 2), (512, 2)]):
            down = twin_downsample(inplanes, planes * 4, stride) if (stride != 1 or inplanes != planes * 4) else None
            blocks = [TwinBottleneck(inplanes, planes, stride, down)]
            inplanes = planes * 4
            blocks += [TwinBottleneck(inplanes, planes) for _ in range(1, layers[i])]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool3d(1)
        self.fc = nn.Linear(2048, num_classes)

    def forward(self, x):
        x = self.layer4(self.layer3(self.layer2(self.layer1(self.stem(x)))))
        return self.avgpool(x).flatten(1)
