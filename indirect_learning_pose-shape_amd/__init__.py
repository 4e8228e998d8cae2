"""MI355X-native SMPL decoder + body-part soft-rasteriser.

Importing the package does not touch the GPU or the HIP library; the first operator call loads
`libsmplraster_hip.so` and raises if it is missing (there is no CPU fallback).
"""
from . import smpl_model  # noqa: F401
from .smpl_model import SMPLModelData, synthetic_smpl_model, load_part_tables, load_mean_params, mean86  # noqa: F401


def __getattr__(name):
    if name in ("SMPLLayer",):
        from .keras_smpl.batch_smpl import SMPLLayer
        return SMPLLayer
    if name == "SMPLDecoder":
        from .decoder import SMPLDecoder
        return SMPLDecoder
    if name in ("orthographic_project", "compute_mask", "projects_to_seg", "projects_to_silhouette",
                "set_cam_params", "load_mean_set_cam_params", "concat_mean_param"):
        import importlib
        mod = {"orthographic_project": "projection", "set_cam_params": "set_cam_params",
               "load_mean_set_cam_params": "set_cam_params"}.get(name, name)
        return getattr(importlib.import_module(__name__ + ".keras_smpl." + mod), name)
    if name in ("ImageDataGenerator", "DeviceBatches", "BatchIndexer", "affine_matrices", "random_draws", "warp_images",
                "warp_labels"):
        from . import augment
        return getattr(augment, name)
    if name in ("RaggedImages", "EvalBatches", "load_images", "load_labels", "pad_geometry"):
        from . import preprocess
        return getattr(preprocess, name)
    if name in ("SyntheticBatches", "BodySampler", "proxy_inputs", "corruption_draws", "frame_cameras"):
        from . import synthetic
        return getattr(synthetic, name)
    if name in ("gaussian_samples", "gaussian_nll", "fuse_gaussians", "fuse_shape", "sample_spread"):
        from . import prob
        return getattr(prob, name)
    raise AttributeError(name)
