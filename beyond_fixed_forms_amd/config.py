"""configs/config.yaml -> attribute-style config (the reference uses Munch.fromDict(yaml.safe_load(..)),
projection_2d_to_3d.py:339 / refinement.py:138; `munch` is not a dependency here).

The keys, including their spelling (`min_aggragated_masks`, `if_occurance_threshold`,
`refinment_sim_percentile`, `refiment_iou_thres`), are the reference's (configs/config.yaml:9-67).
"""
from __future__ import annotations

import yaml

# Defaults = the values shipped in the reference's configs/config.yaml.
DEFAULTS = dict(
    width_2d=1296, height_2d=968, downsample_ratio=10,
    iou_thres=0.2, similarity_thres=0.75, min_aggragated_masks=2,
    if_occurance_threshold=False, occurance_threshold=0.3,
    if_detected_ratio_threshold=True, detected_ratio_threshold=0.38,
    remove_filtered_masks=0.4, remove_small_masks=5,
    stage1_iou_thres=0.1, refinment_sim_percentile=0.2, refiment_iou_thres=0.45,
    # not a key of the reference: integer stride s >= 1 renders the depth frames from the cloud at (ceil(height_2d / s),
    # ceil(width_2d / s)) instead of reading depth/<frame>.png (scene.rendered_depth_on_device); 0 = off.  8 is a starting
    # value nobody has tuned
    depth_from_cloud=0,
    # likewise not a key of the reference: the same stride, the frames rasterised from the scene's triangle mesh
    # (scene_mesh_dir/<scene_id>.npz: `faces` (T, 3) integers, optionally `vertices` (V, 3); without them the faces index the
    # rows of <scene_id>.npy).  0 = off; setting both keys is an error
    depth_from_mesh=0, scene_mesh_dir=None,
    # not a key of the reference either: metres.  With depth_from_mesh on, a triangle that reaches nearer than this (or
    # behind the camera) is clipped at this depth instead of dropped whole (scene.mesh_near_clip); 0 = off, the frames as
    # they were.  0.05 is a starting value nobody has tuned
    mesh_near_clip=0.0,
    # not a key of the reference either: metres.  With depth_from_cloud on, every point of the cloud covers the texels within
    # a camera-facing square of this half-width instead of one texel (scene.cloud_splat_radius): near surfaces close their
    # own gaps.  0 = off, the frames as they were.  About the cloud's point spacing; no value has been tuned
    cloud_splat_radius=0.0,
    # not keys of the reference either: rendering 3-D instances back into the views (reproject.py,
    # tools/reproject_3d_to_2d.py).  reproject_stride: integer s >= 1, the label frames are rendered at (ceil(height_2d / s),
    # ceil(width_2d / s)) and upsampled by the integer map; reproject_splat_radius: metres >= 0, the footprint of a point
    # (about the cloud's point spacing, untuned; flat surfels bleed a label by about one radius at silhouettes), 0 = one
    # texel per point; reproject_min_pixels: an instance covering fewer pixels of a frame makes no mask there;
    # reprojected_2d_dir: where the tool saves <cls>/<scene>.pth
    reproject_stride=1, reproject_splat_radius=0.0, reproject_min_pixels=1, reprojected_2d_dir=None,
    # not keys of the reference either: 3-D instances split into spatially connected parts (spatial.py,
    # tools/split_instances_3d.py).  split_voxel: metres > 0, the cell of the voxel grid -- a few point spacings, e.g. 0.1;
    # untuned, and required by the tool; split_min_points: a part with fewer points is dropped; split_mode: "split" (every
    # part becomes an instance) or "largest" (only the largest part of each); split_output_dir: where the tool saves
    # <cls>/<scene>.pth
    split_voxel=None, split_min_points=1, split_mode="split", split_output_dir=None,
    # not keys of the reference either: 3-D instances snapped to superpoints (superpoints.py,
    # tools/snap_instances_3d.py).  superpoint_dir: where the dataset's superpoints/<scene>.pth lie (one integer id per
    # point), required by the tool; snap_ratio: in (0, 1], the share of a superpoint's points an instance must hold to
    # take it whole, untuned; snap_mode: "snap" (rows are independent and may overlap) or "exclusive" (a superpoint goes
    # to the one row that holds most of it); snap_min_points: a snapped instance with fewer points is dropped;
    # snap_output_dir: where the tool saves <cls>/<scene>.pth
    superpoint_dir=None, snap_ratio=0.5, snap_mode="snap", snap_min_points=1, snap_output_dir=None,
    # not keys of the reference either: running on a voxel subsample of the cloud and lifting the instances back to the
    # full cloud by nearest neighbour (lift.py, tools/subsample_cloud.py, tools/lift_instances_3d.py).  subsample_voxel:
    # metres > 0, the cell one point is kept of, untuned; subsample_npy_dir: where the first tool saves the small
    # <scene>.npy (and sample/<scene>.npy, the kept indices); lift_max_dist: metres > 0, a point of the full cloud farther
    # than this from every point of the small one joins no instance, absent = 2 x subsample_voxel; lift_target_npy_dir:
    # where the full clouds lie; lift_output_dir: where the second tool saves <cls>/<scene>.pth
    subsample_voxel=None, subsample_npy_dir=None, lift_max_dist=None, lift_target_npy_dir=None, lift_output_dir=None,
    # not keys of the reference either: 3-D instances clustered by density, DBSCAN with a deterministic border rule
    # (density.py, tools/cluster_instances_3d.py).  cluster_eps: metres > 0, the neighbourhood radius -- a few point
    # spacings, e.g. 0.1; cluster_min_samples: integer >= 1, a point with that many of its instance's points within
    # cluster_eps (itself included) is a core point; both untuned, and required by the tool; cluster_min_points: a cluster
    # with fewer points is dropped; cluster_mode: "split" (every cluster becomes an instance) or "largest" (only the
    # largest cluster of each); cluster_output_dir: where the tool saves <cls>/<scene>.pth
    cluster_eps=None, cluster_min_samples=None, cluster_min_points=1, cluster_mode="split", cluster_output_dir=None,
    # not keys of the reference either: a scene's prediction assembled from all of its query classes (assemble.py,
    # tools/assemble_scene_3d.py).  assemble_nms_thres: in (0, 1], an instance that overlaps a better-scored one by at least
    # this much is removed -- untuned, e.g. 0.5; absent or 0 = no NMS; assemble_criterion: "iou" or "containment" (the
    # intersection over the smaller of the two); assemble_scope: "all" or "class" (only instances of one class remove each
    # other); assemble_exclusive: every point goes to the best-scored instance that holds it; assemble_min_points: an
    # instance with fewer points (after the exclusive step) is dropped; assembled_output_dir: where the tool saves
    # <scene>.pth
    assemble_nms_thres=None, assemble_criterion="iou", assemble_scope="all", assemble_exclusive=False,
    assemble_min_points=1, assembled_output_dir=None,
    # not keys of the reference either: the frames that see each 3-D instance best and the boxes to crop it with (views.py,
    # tools/select_views_3d.py).  views_top_k: integer in 1 .. 64, the frames kept per instance, by the points the depth
    # frame confirms; views_min_points: a frame that confirms fewer points is no candidate; views_crop_levels: integer in
    # 1 .. 8, the crops per view, level l widened by l x floor(views_crop_expand x box side) pixels; views_crop_expand: a
    # number >= 0.  5, 1, 3 and 0.1 are OpenMask3D's values, untuned here; views_output_dir: where the tool saves
    # <cls>/<scene>.pth
    views_top_k=5, views_min_points=1, views_crop_levels=3, views_crop_expand=0.1, views_output_dir=None,
)


class Config(dict):
    """dict with attribute access (the subset of Munch behaviour the hot path relies on)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    @classmethod
    def with_defaults(cls, **over):
        c = cls(DEFAULTS)
        c.update(over)
        return c


def load_config(path: str) -> Config:
    with open(path, "r") as f:
        return Config(yaml.safe_load(f.read()))
