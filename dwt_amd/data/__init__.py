from .transforms import (Compose, Lambda, Normalize, RandomCrop,
                         RandomHorizontalFlip, Resize, ToTensor, ToUint8HWC)
from .usps import USPS
from .mnist import MNIST
from .folder import ImageFolder, DatasetFolder
from .synthetic import SyntheticDigits, SyntheticOfficeHome
from .device_pipeline import (DeviceBatcher, assemble_views,
                              assemble_views_reference, draw_view_params)

__all__ = [
    "Compose", "Lambda", "Normalize", "RandomCrop", "RandomHorizontalFlip",
    "Resize", "ToTensor", "ToUint8HWC", "USPS", "MNIST", "ImageFolder",
    "DatasetFolder", "SyntheticDigits", "SyntheticOfficeHome",
    "DeviceBatcher", "assemble_views", "assemble_views_reference",
    "draw_view_params",
]
