"""mvster_amd -- MI355X-native implementation of the MVSTER cost-volume hot path.

Public surface = the reference's ``models`` package surface (models/__init__.py:2):
``MVS4net``, ``MVS4net_loss``, ``Blend_loss``; plus the fusion step of its test script (test_mvs4.py:331-421):
``filter_depth`` for a scan on disk, ``fuse_scene`` / ``scene_tables`` for one in memory.
"""
from .fusion import filter_depth, fuse_scene, scene_tables
from .loss import Blend_loss, MVS4net_loss
from .net import MVS4net

__all__ = ["MVS4net", "MVS4net_loss", "Blend_loss", "filter_depth", "fuse_scene", "scene_tables"]
