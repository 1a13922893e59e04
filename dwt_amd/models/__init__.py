from .lenet import LeNet
from .resnet_dwt import Bottleneck, ResNetDWT, resnet50
from .folded import FoldedResNetDWT, fold_norm_into_conv, fold_resnet
from . import checkpoint

__all__ = ["LeNet", "Bottleneck", "ResNetDWT", "resnet50", "checkpoint",
           "FoldedResNetDWT", "fold_norm_into_conv", "fold_resnet"]
