"""mvster_amd -- MI355X-native implementation of the MVSTER cost-volume hot path.

Public surface = the reference's ``models`` package surface (models/__init__.py:2):
``MVS4net``, ``MVS4net_loss``, ``Blend_loss``; plus the fusion step of its test script (test_mvs4.py:331-421):
``filter_depth`` for a scan on disk, ``fuse_scene`` / ``scene_tables`` for one in memory; and the loop before it
(``save_scene_depth``, :170-268) at the level of a scan: ``infer_scan`` / ``infer_scan_folder`` (FPN once per image, all
depth maps of a scan on the GPU), ``write_scan_outputs``, ``reconstruct_scan`` (inference + fusion without leaving the GPU);
and the validation half of its training script's epoch (train_mvs4.py:140-192, :252-307): ``Validator`` (forward,
loss, depth metrics and the epoch's averages in one captured graph per batch; the loop over an iterable of batches is
``mvster_amd.validate.validate`` -- not re-exported here, where its name would hide the module), ``validation_scalars``,
``depth_metrics`` and the reference's ``Thres_metrics`` / ``AbsDepthError_metrics`` (utils.py:139-159).
"""
from .fusion import filter_depth, fuse_scene, scene_tables
from .loss import Blend_loss, MVS4net_loss
from .net import MVS4net
from .scan import infer_scan, infer_scan_folder, reconstruct_scan, write_scan_outputs
from .validate import (SCALAR_NAMES, AbsDepthError_metrics, Thres_metrics, Validator, depth_metrics,
                       validation_scalars)

__all__ = ["MVS4net", "MVS4net_loss", "Blend_loss", "filter_depth", "fuse_scene", "scene_tables",
           "infer_scan", "infer_scan_folder", "reconstruct_scan", "write_scan_outputs",
           "Validator", "validation_scalars", "depth_metrics", "Thres_metrics", "AbsDepthError_metrics",
           "SCALAR_NAMES"]
