"""ccnet_amd -- MI355X-native criss-cross attention (the hot path of speedinghzl/CCNet).

Only what the path needs lives here: ``csrc/`` (HIP kernels + the C ABI of include/ccnet_cca.h), the
ctypes binding (:mod:`ccnet_amd._lib`) and the host-side mirror of the reference's
``cc_attention/functions.py`` (:mod:`ccnet_amd.functions`).  Importing the package does not load the
device library; the first kernel call does, and fails loudly if it has not been built.
"""
from . import augment, celovasz
from .abn import ABN, InPlaceABN, InPlaceABNSync, convert_abn
from .abncl import ABNChannelsLastFunction
from .augment import (CITYSCAPES_ID_TO_TRAINID, AugmentParams, CSDataSet, DeviceAugment, DevicePrefetcher, VOCDataSet,
                      draw_params)
from .celovasz import UpsampledCELovasz, UpsampledCELovaszFunction
from .conv3 import DeviceConv3x3, conv3x3, convert_conv3x3
from .dsn import UpsampledCrossEntropy2d, UpsampledCrossEntropyFunction
from .functions import (CA_Map, CA_Weight, CrissCrossAttention, CrissCrossFunction, INF, ca_map, ca_softmax,
                        ca_weight, criss_cross_attention, graph_module)
from .evaluate import MultiScaleEvaluator, SegEvaluator, predict_multiscale, predict_sliding, predict_whole, scaled_size
from .lovasz import CriterionOhemDSN2, LovaszSoftmax, LovaszSoftmaxFunction, lovasz_softmax
from .ohem import CriterionOhemDSN, OhemCrossEntropy2d
from .ohemdsn import UpsampledOhemCrossEntropy2d, UpsampledOhemFunction
from .optim import DeviceMixedSGD, DeviceSGD, bf16_parameters, poly_schedule

__all__ = ["CrissCrossAttention", "CrissCrossFunction", "CA_Weight", "CA_Map", "ca_weight", "ca_map",
           "ca_softmax", "criss_cross_attention", "graph_module", "INF", "OhemCrossEntropy2d", "CriterionOhemDSN",
           "SegEvaluator", "predict_sliding", "predict_whole", "MultiScaleEvaluator", "predict_multiscale", "scaled_size",
           "lovasz_softmax", "LovaszSoftmax", "LovaszSoftmaxFunction",
           "CriterionOhemDSN2", "ABN", "InPlaceABN", "InPlaceABNSync", "convert_abn", "UpsampledCrossEntropy2d",
           "UpsampledCrossEntropyFunction", "UpsampledOhemCrossEntropy2d", "UpsampledOhemFunction",
           "celovasz", "UpsampledCELovasz", "UpsampledCELovaszFunction", "augment", "DeviceAugment", "DevicePrefetcher",
           "CSDataSet", "VOCDataSet", "AugmentParams", "draw_params", "CITYSCAPES_ID_TO_TRAINID", "DeviceSGD", "poly_schedule",
           "DeviceMixedSGD", "bf16_parameters", "conv3x3", "DeviceConv3x3", "convert_conv3x3",
           "ABNChannelsLastFunction"]
__version__ = "0.1.0"
