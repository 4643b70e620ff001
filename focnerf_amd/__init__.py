"""focnerf_amd — MI355X (gfx950) implementation of FOCNeRF's volume-rendering hot path:
raymarching, gridencoder, freqencoder, ffmlp (+ the multi-object combine), behind the
reference's Python operator API. The compute lives in libfocnerf_hip.so (C ABI in
include/focnerf.h); importing this package fails loudly if that library is missing."""
from . import _lib  # noqa: F401  (raises ImportError when libfocnerf_hip.so is absent)
from .determinism import use_deterministic, is_deterministic, deterministic  # noqa: F401  (FOC_DETERMINISTIC: bit-reproducible training steps)
from .combine import Attribution  # noqa: F401  (per-object mattes, depths and the instance map of a combined render)
from .placement import Placement  # noqa: F401  (rotation, uniform scale and translation of an object in the combined render)
from .mesh import (density_volume, scene_volume, marching_cubes, extract_geometry, extract_scene_geometry,  # noqa: F401  (triangle meshes
                   write_ply, save_mesh, Mesh, extract_mesh, extract_scene_mesh, read_ply_attributes)      # of objects and placed scenes)
from .simplify import simplify_mesh, SimplifiedMesh  # noqa: F401  (vertex clustering on the device: meshes with fewer triangles)
from .components import label_components, filter_components, Components  # noqa: F401  (connected components on the device: meshes and grids without floaters)
from .query import query_scene, SceneSample  # noqa: F401  (a placed scene at arbitrary points: density, winning object, colour, normal)
from .score import score_view, ViewScore  # noqa: F401  (PSNR and SSIM of a combined view for every background, on the device)
from .normals import density_gradient, field_normals, decode_normal_map, render_normals, normal_map_finish  # noqa: F401  (surface normals from the density field)
from . import optim  # noqa: F401
from .optim import FusedAdam, LossScaler  # noqa: F401  (the trainer's optimizer step: overflow check, unscale and Adam in two launches)
from . import ema  # noqa: F401
from .ema import ParameterEMA  # noqa: F401  (torch_ema's ExponentialMovingAverage; its update rides in FusedAdam's update launch)
from . import batch  # noqa: F401
from .batch import DeviceDataset, RaySampler, photo_loss  # noqa: F401  (a training batch in one launch; loss, gradient and error map in one more)

__all__ = ["raymarching", "gridencoder", "freqencoder", "ffmlp", "activation", "encoding", "shencoder",
           "renderer", "network", "combine", "fixedcull", "use_deterministic", "is_deterministic", "deterministic", "Attribution", "placement", "Placement",
           "mesh", "density_volume", "scene_volume", "marching_cubes", "extract_geometry", "extract_scene_geometry", "write_ply", "save_mesh",
           "Mesh", "extract_mesh", "extract_scene_mesh", "read_ply_attributes", "simplify", "simplify_mesh", "SimplifiedMesh", "components", "label_components", "filter_components", "Components", "query", "query_scene", "SceneSample",
           "score", "score_view", "ViewScore",
           "normals", "density_gradient", "field_normals", "decode_normal_map", "render_normals", "normal_map_finish",
           "optim", "FusedAdam", "LossScaler", "ema", "ParameterEMA",
           "batch", "DeviceDataset", "RaySampler", "photo_loss"]
