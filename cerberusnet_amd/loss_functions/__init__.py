from .depth_losses import (BackprojectDepth, DepthAwareLoss, DepthReconstructionLossV1, InvHuberLoss, InvHuberLossPyr, Project3D,
                           ScaleInvariantError, inv_huber_loss, reproject_warp)
from .detr_loss import DetrLoss, detr_set_loss
from .ohem_losses import (MixSoftmaxCrossEntropyLoss, MixSoftmaxCrossEntropyOHEMLoss, SoftmaxCrossEntropyOHEMLoss,
                          seg_ohem_cross_entropy)
from .panoptic_loss import DeeplabPanopticLoss, deeplab_panoptic_loss
from .rmi import MultiScaleRMILoss, RMILoss, RMILossAux, rmi_loss
from .seg_losses import FocalLoss2D, SegCrossEntropy, class_balance_weights, seg_cross_entropy
from .UnFlowLoss import (TernaryLoss, census_loss, edge_smoothness, flow_warp, get_corresponding_map, get_occu_mask_backward,
                         get_occu_mask_bidirection, mesh_grid, norm_grid, photometric_loss, unFlowLoss)

__all__ = ["flow_warp", "mesh_grid", "norm_grid", "photometric_loss", "edge_smoothness", "TernaryLoss", "census_loss",
           "get_corresponding_map", "get_occu_mask_backward", "get_occu_mask_bidirection", "unFlowLoss",
           "BackprojectDepth", "Project3D", "DepthReconstructionLossV1", "reproject_warp",
           "seg_cross_entropy", "class_balance_weights", "FocalLoss2D", "SegCrossEntropy",
           "seg_ohem_cross_entropy", "MixSoftmaxCrossEntropyLoss", "SoftmaxCrossEntropyOHEMLoss", "MixSoftmaxCrossEntropyOHEMLoss",
           "inv_huber_loss", "InvHuberLoss", "InvHuberLossPyr", "ScaleInvariantError", "DepthAwareLoss",
           "rmi_loss", "RMILoss", "RMILossAux", "MultiScaleRMILoss",
           "deeplab_panoptic_loss", "DeeplabPanopticLoss",
           "DetrLoss", "detr_set_loss"]
