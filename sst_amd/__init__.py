"""sst_amd — MI355X-native (gfx950) hot path of the SST / FSD sparse LiDAR backbones.

The names exported here are the ones the reference exposes from ``mmdet3d.ops`` / its registries for the
path; they are backed by hand-written HIP kernels in ``sst_amd/csrc`` behind the C ABI of
``include/sst_amd.h``.  There is no CPU or eager fallback: without the built library, or on a CPU
tensor, the ops raise.
"""
from . import _lib
from .kernels import WindowPlan, sra_attention, sra_attention_qk_v
from .norm import NaiveSyncBatchNorm1d, NaiveSyncBatchNorm2d, build_conv_layer, build_norm_layer
from .registry import (BACKBONES, MIDDLE_ENCODERS, MODELS, ROI_EXTRACTORS, VOXEL_ENCODERS, build_backbone,
                       build_middle_encoder, build_voxel_encoder)
from .voxel import (DynamicScatter, Voxelization, build_scatter_plan, dynamic_point_to_voxel_forward,
                    dynamic_scatter, dynamic_voxelize, voxelization)
from .sst_ops import (build_mlp, flat2window, flat2window_v2, get_activation, get_activation_layer,
                      get_flat2win_inds, get_flat2win_inds_v2, get_inner_win_inds, get_window_coors,
                      make_continuous_inds, scatter_v2, window2flat, window2flat_v2)
from .voxel_encoder import DynamicScatterVFE, DynamicVFE, DynamicVFELayer, DynamicVFELayerV2, SIRLayer
from .sir_stage import enable_fused_sir, sir_stage, sir_stage_ok, sir_stage_tile_rows
from .sst_input_layer import PseudoMiddleEncoderForSpconvFSD, SSTInputLayer, SSTInputLayerV2
from .sst_basic_block import BasicShiftBlockV2, EncoderLayer, WindowAttention
from .backbones import SIR, SSTv1, SSTv2
from .cluster import (ClusterAssigner, HybridAssigner, SSGAssigner, connected_components_xy, filter_almost_empty,  # noqa: F401
                      find_connected_componets, find_connected_componets_single_batch, modify_cluster_by_class, ssg,
                      ssg_single_sample)
from .cluster import cluster_assign_classes, enable_class_batched  # noqa: F401
from .fps import fps_segmented, furthest_point_sample, furthest_point_sample_with_dist, ssg_assign  # noqa: F401
from .dynamic_point_pool import DynamicPointROIExtractor, dynamic_point_pool, dynamic_point_pool_mixed
from . import spconv  # noqa: F401  (sst_amd.spconv mirrors mmdet3d.ops.spconv)
from .spconv import (SparseConv3d, SparseConvTensor, SparseConvTranspose3d, SparseInverseConv3d,  # noqa: F401
                     SparseMaxPool3d, SparseModule, SparseSequential, SubMConv3d)
from .sparse_unet import (SimpleSparseUNet, SparseBasicBlock, SparseUNet, VirtualVoxelMixer,  # noqa: F401
                          make_sparse_convmodule)

from .virtual_voxel import VirtualVoxelExtractor  # noqa: F401
from . import box_ops  # noqa: F401
from .box_ops import (box3d_multiclass_nms, boxes3d_overlaps_lidar, boxes_iou_bev, boxes_overlap_1to1,  # noqa: F401
                      boxes_overlap_bev, nms_gpu, nms_normal_gpu, points_in_boxes_batch, points_in_boxes_gpu)
from . import seg_loss  # noqa: F401
from .seg_loss import seg_point_targets, seg_vote_loss  # noqa: F401
from . import detectors  # noqa: F401
from .detectors import (DETECTORS, HEADS, NECKS, FSD, FSDV2, DynamicCenterPoint, DynamicVoxelNet, SingleStageFSD, SingleStageFSDV2, VoteSegHead,  # noqa: F401
                        VoteSegmentor, Voxel2PointScatterNeck, build_detector, build_head, build_model, build_neck,
                        install_fused_extract_feat)
from . import center_head  # noqa: F401
from .center_head import (BBOX_CODERS, CenterHead, CenterPointBBoxCoder, build_bbox_coder, center_decode, center_loss,  # noqa: F401
                          center_targets)
from . import cluster_head  # noqa: F401
from .cluster_head import (BasePointBBoxCoder, FSDSeparateHead, FSDV2Head, SparseClusterHeadV2, cluster_decode, cluster_encode,  # noqa: F401
                           cluster_loss, cluster_targets)
from . import roi_head  # noqa: F401
from .roi_head import (DeltaXYZWLHRBBoxCoder, FullySparseBboxHead, GroupCorrectionHead, roi_assign_sample, roi_compact,  # noqa: F401
                       roi_decode, roi_loss)
from . import anchor_head  # noqa: F401
from .anchor_head import (ANCHOR_GENERATORS, SECONDFPN, AlignedAnchor3DRangeGenerator, Anchor3DHead, Anchor3DRangeGenerator,  # noqa: F401
                          anchor_decode, anchor_loss, anchor_targets, build_anchor_generator)
from . import fg_sample  # noqa: F401
from .fg_sample import (fg_gather_cat, fg_sample_launch, roi_input, roi_input_single)  # noqa: F401
from . import fg_group_sample  # noqa: F401
from .fg_group_sample import group_sample, group_sample_launch, group_topk_extra_mask, virtual_rows  # noqa: F401
from . import fsdv2_step  # noqa: F401
from .fsdv2_step import FSDV2Step, SingleStageFSDV2Step, attach_fsdv2_heads  # noqa: F401
from . import deform_conv  # noqa: F401
from .deform_conv import (DeformConv2d, DeformConv2dPack, deform_conv2d, deform_conv_tile_pixels,  # noqa: F401
                          deform_conv_wgrad_blocks)
from . import optim  # noqa: F401
from .optim import (CyclicLr, CyclicMomentum, FusedAdamW, TrainingUpdate, build_optimizer,  # noqa: F401
                    build_training_update)
from . import tracklet  # noqa: F401
from .tracklet import LiDARTracklet, TrackletAssigner, aligned_iou_3d, tracklet_rows, tracklet_targets  # noqa: F401
from . import tracklet_detector  # noqa: F401
from .tracklet_detector import (TimestampEncoder, TrackletDetector, TrackletPointRoIExtractor, TrackletRoIHead,  # noqa: F401
                                TrackletSegmentor, get_bboxes_from_tracklet)
from . import incremental  # noqa: F401
from .incremental import (box_frame_transform_gpu, find_delta_points_by_voxelization,  # noqa: F401
                          find_delta_points_by_voxelization_list_v3, generate_points, incremental_points_mask,
                          points_frame_transform, seed_crop)
from . import fsdpp  # noqa: F401
from .fsdpp import TwoStageFSDPP  # noqa: F401
from . import augment  # noqa: F401
from .augment import AugmentParams, TrainAugment  # noqa: F401
from . import tracklet_augment  # noqa: F401
from .tracklet_augment import TrackletAugment, TrackletParams  # noqa: F401
from . import tracklet_tta  # noqa: F401
from .tracklet_tta import TrackletTTA, TrackletTTADetector, attach_tracklet_tta, tta_finish  # noqa: F401
from . import tracklet_prep  # noqa: F401
from .tracklet_prep import (box_point_counts, box_point_crops, candidate_stats, crop_tracklet_points,  # noqa: F401
                            generate_candidates, remove_empty_boxes, tracklet_affinity)

__version__ = '0.1.0'

__all__ = [
    'tracklet_prep', 'tracklet_affinity', 'generate_candidates', 'candidate_stats', 'box_point_crops', 'box_point_counts',
    'crop_tracklet_points', 'remove_empty_boxes',
    'augment', 'AugmentParams', 'TrainAugment', 'tracklet_augment', 'TrackletAugment', 'TrackletParams',
    'tracklet_tta', 'TrackletTTA', 'TrackletTTADetector', 'attach_tracklet_tta', 'tta_finish',
    'incremental', 'box_frame_transform_gpu', 'find_delta_points_by_voxelization', 'find_delta_points_by_voxelization_list_v3',
    'generate_points', 'incremental_points_mask', 'points_frame_transform', 'seed_crop', 'fsdpp', 'TwoStageFSDPP',
    'tracklet_detector', 'TimestampEncoder', 'TrackletDetector', 'TrackletPointRoIExtractor', 'TrackletRoIHead', 'TrackletSegmentor',
    'get_bboxes_from_tracklet', 'tracklet', 'LiDARTracklet', 'TrackletAssigner', 'aligned_iou_3d', 'tracklet_rows', 'tracklet_targets',
    'VirtualVoxelExtractor', 'detectors', 'DynamicVoxelNet', 'DynamicCenterPoint', 'install_fused_extract_feat', 'DETECTORS', 'HEADS', 'NECKS', 'FSD', 'FSDV2', 'SingleStageFSD', 'SingleStageFSDV2',
    'VoteSegHead', 'VoteSegmentor', 'Voxel2PointScatterNeck', 'build_detector', 'build_head', 'build_model', 'build_neck',
    'Voxelization', 'voxelization', 'DynamicScatter', 'dynamic_scatter', 'dynamic_voxelize',
    'dynamic_point_to_voxel_forward', 'build_scatter_plan', 'flat2window', 'window2flat', 'get_flat2win_inds',
    'get_inner_win_inds', 'make_continuous_inds', 'flat2window_v2', 'window2flat_v2', 'get_flat2win_inds_v2',
    'get_window_coors', 'scatter_v2', 'build_mlp', 'get_activation', 'get_activation_layer',
    'NaiveSyncBatchNorm1d', 'NaiveSyncBatchNorm2d', 'build_norm_layer', 'build_conv_layer', 'DynamicVFE',
    'DynamicScatterVFE', 'SIRLayer', 'DynamicVFELayer', 'DynamicVFELayerV2', 'SSTInputLayer', 'SSTInputLayerV2',
    'PseudoMiddleEncoderForSpconvFSD', 'WindowAttention', 'EncoderLayer', 'BasicShiftBlockV2', 'SSTv1', 'SSTv2', 'SIR',
    'MODELS', 'VOXEL_ENCODERS', 'MIDDLE_ENCODERS', 'BACKBONES', 'build_voxel_encoder', 'build_middle_encoder',
    'build_backbone', 'WindowPlan', 'sra_attention', 'sra_attention_qk_v', 'ClusterAssigner',
    'find_connected_componets', 'find_connected_componets_single_batch', 'filter_almost_empty',
    'modify_cluster_by_class', 'connected_components_xy', 'cluster_assign_classes', 'enable_class_batched', 'ROI_EXTRACTORS', 'DynamicPointROIExtractor',
    'dynamic_point_pool', 'dynamic_point_pool_mixed', 'spconv', 'SparseConvTensor', 'SparseSequential', 'SparseModule',
    'SubMConv3d', 'SparseConv3d', 'SparseConvTranspose3d', 'SparseInverseConv3d', 'SparseMaxPool3d', 'SparseUNet', 'SimpleSparseUNet', 'VirtualVoxelMixer',
    'SparseBasicBlock', 'make_sparse_convmodule',
    'box_ops', 'boxes_iou_bev', 'boxes_overlap_bev', 'boxes_overlap_1to1', 'nms_gpu', 'nms_normal_gpu',
    'points_in_boxes_gpu', 'points_in_boxes_batch', 'boxes3d_overlaps_lidar', 'box3d_multiclass_nms',
    'furthest_point_sample', 'furthest_point_sample_with_dist', 'fps_segmented', 'ssg_assign', 'ssg', 'ssg_single_sample',
    'SSGAssigner', 'HybridAssigner', 'sir_stage', 'sir_stage_ok', 'sir_stage_tile_rows', 'enable_fused_sir',
    'seg_loss', 'seg_point_targets', 'seg_vote_loss',
    'center_head', 'center_targets', 'center_loss', 'center_decode', 'CenterHead', 'CenterPointBBoxCoder', 'BBOX_CODERS',
    'build_bbox_coder',
    'cluster_head', 'cluster_targets', 'cluster_loss', 'cluster_decode', 'cluster_encode', 'BasePointBBoxCoder', 'FSDSeparateHead',
    'SparseClusterHeadV2', 'FSDV2Head',
    'roi_head', 'roi_assign_sample', 'roi_compact', 'roi_loss', 'roi_decode', 'DeltaXYZWLHRBBoxCoder', 'FullySparseBboxHead',
    'GroupCorrectionHead',
    'anchor_head', 'anchor_targets', 'anchor_loss', 'anchor_decode', 'Anchor3DHead', 'SECONDFPN', 'ANCHOR_GENERATORS',
    'Anchor3DRangeGenerator', 'AlignedAnchor3DRangeGenerator', 'build_anchor_generator',
    'fg_sample', 'fg_sample_launch', 'fg_gather_cat', 'roi_input', 'roi_input_single',
    'fg_group_sample', 'group_sample', 'group_sample_launch', 'group_topk_extra_mask', 'virtual_rows',
    'fsdv2_step', 'attach_fsdv2_heads', 'SingleStageFSDV2Step', 'FSDV2Step',
    'deform_conv', 'deform_conv2d', 'DeformConv2d', 'DeformConv2dPack', 'deform_conv_tile_pixels', 'deform_conv_wgrad_blocks',
    'optim', 'FusedAdamW', 'TrainingUpdate', 'CyclicLr', 'CyclicMomentum', 'build_optimizer', 'build_training_update',
]
