from .UnFlowLoss import (TernaryLoss, census_loss, edge_smoothness, flow_warp, mesh_grid, norm_grid, photometric_loss,
                         unFlowLoss)

__all__ = ["flow_warp", "mesh_grid", "norm_grid", "photometric_loss", "edge_smoothness", "TernaryLoss", "census_loss",
           "unFlowLoss"]
