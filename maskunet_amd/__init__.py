"""maskunet_amd -- MI355X-native (gfx950) MaskAttn-UNet forward/backward path.

Drop-in for the model classes of Belis0811/MaskUnet (code/ade20k/ade_semantic.py:152-314,
code/cityscapes/city_instance.py:216-276): same names, signatures and state_dict keys, running on
hand-written HIP kernels through the C ABI in include/maskunet_hip.h.
"""
from .modules import (ConvBlock, DoubleConv, Down, DownSample, InstanceUNet, Mask2FormerAttention, MaskAttention, OutConv,
                      UNet, Up, UpSample, set_default_compute_dtype)
from .dp import DataParallel, shard_batch
from .losses import CrossEntropyLoss, InstanceContrastiveLoss, cross_entropy, mean_iou, pixel_cross_entropy_nhwc
from .instances import (Instances, generate_instance_mask, instances_from_embeddings, instances_from_id_map, instances_from_labels,
                        predict_instances)
from .matching import CocoEval, CocoMatches, InstanceAP, Matches, PanopticQuality, coco_match, match_instances
from .panoptic import Panoptic, panoptic_segments, predict_panoptic
from .metrics import SemanticBatch, SemanticMetrics, SemanticNativeBatch, metrics_from_counts, semantic_eval, semantic_eval_native
from .rle import RLEs, decode_rle, encode_rle, rle_counts_from_string, rle_string_from_counts
from .coco import CocoMasks, coco_masks
from .images import PackedImages, pack_images, resize_pil_to_nhwc
from .ops import resize_labels_u8, resize_u8_to_nhwc
from .targets import (PackedMaps, PanopticTargets, pack_maps, pack_segments, panoptic_targets, resize_cv2_to_nhwc,
                      resize_labels_cv2)
from .optim import FusedAdamW
from .graph import GraphedStep
from ._lib import get_float32_matmul_precision, set_float32_matmul_precision

__all__ = ["ConvBlock", "DownSample", "UpSample", "Mask2FormerAttention", "UNet", "InstanceUNet", "DoubleConv", "Down", "Up",
           "MaskAttention", "OutConv", "set_default_compute_dtype", "DataParallel", "shard_batch", "pixel_cross_entropy_nhwc",
           "mean_iou", "InstanceContrastiveLoss", "FusedAdamW", "CrossEntropyLoss", "cross_entropy", "GraphedStep",
           "resize_u8_to_nhwc", "resize_labels_u8", "set_float32_matmul_precision", "get_float32_matmul_precision", "predict_instances",
           "instances_from_labels", "generate_instance_mask", "Instances", "instances_from_embeddings", "match_instances", "Matches",
           "InstanceAP", "PanopticQuality", "RLEs", "encode_rle", "decode_rle", "rle_counts_from_string", "rle_string_from_counts",
           "coco_masks", "CocoMasks", "instances_from_id_map", "semantic_eval", "SemanticBatch", "SemanticMetrics",
           "metrics_from_counts", "resize_pil_to_nhwc", "pack_images", "PackedImages", "coco_match", "CocoMatches", "CocoEval",
           "semantic_eval_native", "SemanticNativeBatch", "Panoptic", "panoptic_segments", "predict_panoptic",
           "PackedMaps", "PanopticTargets", "pack_maps", "pack_segments", "panoptic_targets", "resize_cv2_to_nhwc", "resize_labels_cv2"]
__version__ = "0.1.0"
