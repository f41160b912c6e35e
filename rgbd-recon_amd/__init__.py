"""rgbd-recon_amd -- MI355X-native TSDF fusion core behind rgbd-recon's ReconIntegration surface.

  csrc/      hand-written HIP kernels (gfx950) + the C ABI of include/rgbd_recon_hip.h
  host/      C++ adapter with the reference's class/method names (drop-in for the GL operator)
  binding.py ctypes binding + Python mirror of the operator (used by tests/, bench.py)
  scene.py   synthetic calibrated RGB-D scene (harness input)
  multigpu.py  Z-slab partition driver: one process per GPU, torch.distributed (RCCL) exchange

The directory name carries a hyphen (project naming); import it as ``rgbd_recon_amd`` (alias module at
the repository root) or with importlib.
"""
from .binding import (LANES_NO_FILL_THREAD, LANES_NO_INTEGRATE_LANE, LANES_ONE_STREAM, LANES_SHARED_FILL_LANE, ReconIntegrationHip, TsdfConfig, TsdfError, build_library, declared_symbols,  # noqa: F401
                      load_library, LIB_PATH, HEADER_PATH, read_calib_volume, write_calib_volume,
                      read_stream_record, stream_num_frames, frustum_from_volume, view_matrices, inverse_volume_resolution, invert_calibration, COLOR_RGB8, COLOR_DXT1, COLOR_DXT5, DEPTH_F32, DEPTH_U8,
                      PRESENT_RGBA8, PRESENT_DXT1, PRESENT_TOP_DOWN, MESH_NORMALS, MESH_COLOURS, MESH_OVERFLOW_VERTICES, MESH_OVERFLOW_TRIANGLES, MESH_OVERFLOW_TILES,
                      MeshFrame, unpack_mesh_vertices, MESH_INDEX_U32, MESH_INDEX_TILE16, MESH_TILE_ROW_DTYPE, MeshCompact, unpack_mesh_triangles, MeshPart, join_mesh_parts, MESH_COMPONENT_DTYPE, MESH_COMPONENT_MEASURE_DTYPE, MESH_MEASURE_GRID_DTYPE, MESH_MEASURE_RULE_DTYPE, MESH_RULE_POSITIVE_VOLUME, mesh_measures_si, mesh_measure_rule_for, mesh_volume6, RAYS_UNIT_CUBE, RAY_NORMALS, RAY_COLOURS, RAY_HIT, RAY_OUTSIDE, RAY_INVALID, Ray, RayHit, RaySurface,
                      RAY_DTYPE, RAY_HIT_DTYPE, RAY_SURFACE_DTYPE, as_rays, make_rays, merge_ray_parts,
                      TAPS_UNIT_CUBE, TAPS_SENSOR, TextureTap, SensorTap, TEXTURE_TAP_DTYPE, SENSOR_TAP_DTYPE, blend_from_taps,
                      MESH_STREAM_TAPS, PackedTap, MeshTaps, PACKED_TAP_DTYPE, unpack_mesh_taps,
                      MESH_SEAM_VERTEX_DTYPE, MESH_SEAM_ROOT_DTYPE, MESH_COMPONENT_LINK_DTYPE, MeshComponentSeams, component_seams_struct, merge_mesh_component_seams,
                      drop_mesh_components)
from . import scene  # noqa: F401
