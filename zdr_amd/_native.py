"""ctypes binding of include/zdr.h (libzdr_hip.so).

There is NO CPU fallback: if the HIP library is missing or cannot be loaded this module raises,
so a GPU box can never silently run anything but the hand-written gfx950 kernels.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libzdr_hip.so")
BAKE_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_bake.so")     # the texture-space light baker: likewise
PUSHPULL_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_pushpull.so")   # push-pull hole filling: likewise
PROJECT_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_project.so")     # texture-space views: likewise
MIP_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_mip.so")             # the image pyramid and the mip gather: likewise
ANISO_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_aniso.so")         # the footprint ellipse and the anisotropic gather: likewise
PLAN_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_plan.so")           # the gather plan: likewise
VIEWGRAD_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_viewgrad.so")   # camera gradients: likewise
TANGENT_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_tangent.so")     # UV tangents: likewise
BAKEGRAD_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_bakegrad.so")   # the light baker's adjoint: likewise
BOUNCE_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_bounce.so")       # the bounced-light baker: likewise
BOUNCEGRAD_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_bouncegrad.so")   # the bounced-light baker's adjoint: likewise
BOUNCEENV_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_bounceenv.so")     # its adjoint in the environment map: likewise
TEXEL_LIB_PATH = os.path.join(HERE, "csrc", "libzdr_texel.so")   # the texture-space kernels: a dependency of libzdr_hip.so, found beside it

COLLOCATED, DIRECT, PATH, UVGRAD = 0, 1, 2, 3
SAMPLER_CMJ, SAMPLER_PMJ02BN = 0, 1
ACCEL_AUTO, ACCEL_BRUTE, ACCEL_BVH = 0, 1, 2
ABI_VERSION = 4                # ZDR_ABI_VERSION of the include/zdr.h this binding mirrors
MAX_MATERIALS = 16             # ZDR_MAX_MATERIALS
MAX_COORD = 2.0 ** 30          # ZDR_MAX_COORD: the largest magnitude of a world-space coordinate zdr_scene_create accepts
AOV_CHANNELS = 16              # ZDR_AOV_CHANNELS
DENOISE_MAX_LEVELS = 6         # ZDR_DENOISE_MAX_LEVELS
PRB_MODES = {"expectation": 0, "detached": 1, "literal": 2}
INTEGRATORS = {"collocated": COLLOCATED, "direct": DIRECT, "path": PATH}   # render.py:65-69
SAMPLERS = {"cmj": SAMPLER_CMJ, "corrmj": SAMPLER_CMJ, "pmj02bn": SAMPLER_PMJ02BN}
ACCELS = {"auto": ACCEL_AUTO, "brute": ACCEL_BRUTE, "bvh": ACCEL_BVH}
COUNTER_NAMES = ("samples", "closest_rays", "closest_hits", "shadow_rays", "shaded_vertices",
                 "emitter_hits_bsdf", "nan_samples", "shadow_rays_traced")

# every symbol include/zdr.h declares
EXPORTS = ("zdr_version", "zdr_abi_version", "zdr_last_error", "zdr_scene_create", "zdr_scene_destroy", "zdr_scene_info",
           "zdr_scene_set_emissions", "zdr_scene_set_envmap", "zdr_scene_set_pmj02bn_tables", "zdr_render_forward", "zdr_render_backward",
           "zdr_render_stats", "zdr_scene_check", "zdr_trace_closest", "zdr_trace_any", "zdr_sampler_dump", "zdr_vertex_sampler_dump", "zdr_path_dump", "zdr_trace_fused", "zdr_shading_dump", "zdr_light_dump", "zdr_texture_lookup", "zdr_texture_scatter", "zdr_debug_build_accel", "zdr_debug_never_occluders",
           "zdr_scene_set_material_slots", "zdr_render_forward_materials", "zdr_render_backward_materials",
           "zdr_scene_set_envmap_texture", "zdr_scene_update_envmap_sampling", "zdr_scene_get_envmap_sampling", "zdr_render_backward_env", "zdr_render_backward_materials_env",
           "zdr_scene_set_emission_values", "zdr_render_backward_emission", "zdr_render_backward_materials_emission",
           "zdr_render_aovs", "zdr_render_aovs_backward",
           "zdr_denoise_workspace_bytes", "zdr_denoise", "zdr_denoise_backward",
           "zdr_texel_aovs_workspace_bytes", "zdr_scene_texel_aovs",
           "zdr_texel_lighting_workspace_bytes", "zdr_scene_texel_lighting",
           "zdr_push_pull_workspace_bytes", "zdr_push_pull", "zdr_push_pull_backward",
           "zdr_texel_view_workspace_bytes", "zdr_scene_texel_view", "zdr_texel_gather", "zdr_texel_gather_backward",
           "zdr_image_pyramid_bytes", "zdr_image_pyramid", "zdr_image_pyramid_backward", "zdr_texel_gather_mip", "zdr_texel_gather_mip_backward",
           "zdr_texel_footprint", "zdr_texel_gather_aniso", "zdr_texel_gather_aniso_backward",
           "zdr_gather_plan_rows", "zdr_gather_plan_workspace_bytes", "zdr_gather_plan_count", "zdr_gather_plan_build", "zdr_gather_plan_apply",
           "zdr_texel_gather_dview", "zdr_texel_view_backward_workspace_bytes", "zdr_texel_view_backward",
           "zdr_scene_texel_tangents", "zdr_texel_footprint_tangents",
           "zdr_texel_lighting_backward_workspace_bytes", "zdr_scene_texel_lighting_backward",
           "zdr_texel_bounce_workspace_bytes", "zdr_texel_bounce_lanes_shift", "zdr_scene_texel_bounce", "zdr_texel_bounce_dump",
           "zdr_texel_bounce_backward_workspace_bytes", "zdr_scene_texel_bounce_backward",
           "zdr_texel_bounce_backward_env_workspace_bytes", "zdr_scene_texel_bounce_backward_env")


class CameraPOD(C.Structure):
    _fields_ = [("fov", C.c_float), ("origin", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3)]


class RenderParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("integrator", C.c_int32), ("sampler", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("spp", C.c_uint32), ("seed", C.c_uint32), ("use_tent", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32),
        ("sample_begin", C.c_uint32), ("sample_end", C.c_uint32),
        ("max_depth", C.c_int32), ("rr_depth", C.c_int32),
        ("camera", CameraPOD), ("tex_h", C.c_int32), ("tex_w", C.c_int32),
        ("tile_shard_index", C.c_int32), ("tile_shard_count", C.c_int32), ("prb_mode", C.c_int32),
    ]


class DenoiseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float)]


class TexelLightingParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("spp", C.c_uint32), ("sample_begin", C.c_uint32),
                ("sample_end", C.c_uint32), ("seed", C.c_uint32), ("sampler", C.c_int32), ("max_distance", C.c_float)]


class TexelBounceParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("spp", C.c_uint32), ("seed", C.c_uint32),
                ("sampler", C.c_int32), ("sample_begin", C.c_uint32), ("sample_end", C.c_uint32), ("bounces", C.c_int32)]


class PushPullParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32)]


class TexelViewParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("camera", CameraPOD)]


class TexelGatherParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class ImagePyramidParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("levels", C.c_int32)]


class TexelGatherMipParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("levels", C.c_int32), ("footprint", C.c_float)]


class TexelFootprintParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("camera", CameraPOD)]


class TexelGatherAnisoParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("levels", C.c_int32), ("footprint", C.c_float), ("max_aniso", C.c_int32)]


class GatherPlanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("filter", C.c_int32), ("levels", C.c_int32), ("footprint", C.c_float), ("max_aniso", C.c_int32)]


class TexelGatherDviewParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("tex_h", C.c_int32), ("tex_w", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("filter", C.c_int32), ("levels", C.c_int32), ("footprint", C.c_float)]


class SceneInfo(C.Structure):
    _fields_ = [("ntris", C.c_uint32), ("nverts", C.c_uint32), ("ninst", C.c_uint32), ("light_count", C.c_uint32),
                ("accel", C.c_int32), ("bvh_nodes", C.c_uint32), ("bvh_max_depth", C.c_uint32), ("bvh_stack_entries", C.c_uint32), ("device", C.c_int32),
                ("device_bytes", C.c_uint64)]


class ZdrError(RuntimeError):
    pass


_LIB = None


def lib():
    """Loads libzdr_hip.so (building it in-tree first if the sources are newer)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    from . import build as _build
    if _build.stale():
        _build.build()
    for path in (LIB_PATH, TEXEL_LIB_PATH, BAKE_LIB_PATH, PUSHPULL_LIB_PATH, PROJECT_LIB_PATH, MIP_LIB_PATH, ANISO_LIB_PATH, PLAN_LIB_PATH, VIEWGRAD_LIB_PATH, TANGENT_LIB_PATH, BAKEGRAD_LIB_PATH, BOUNCE_LIB_PATH, BOUNCEGRAD_LIB_PATH):
        if not os.path.exists(path):
            raise ZdrError(f"{path} is missing: the zdr HIP back end was not built (python -m zdr_amd.build)")
    L = C.CDLL(LIB_PATH)
    vp, fp, ip = C.c_void_p, C.c_void_p, C.c_void_p   # raw addresses (host numpy or device data_ptr)
    L.zdr_version.restype = C.c_char_p
    L.zdr_last_error.restype = C.c_char_p
    L.zdr_scene_create.argtypes = [fp, C.c_uint32, ip, C.c_uint32, ip, fp, fp, C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]
    L.zdr_scene_destroy.argtypes = [vp]
    L.zdr_scene_info.argtypes = [vp, C.POINTER(SceneInfo)]
    L.zdr_scene_set_emissions.argtypes = [vp, fp, vp]
    L.zdr_scene_set_envmap.argtypes = [vp, fp, C.c_uint32, C.c_uint32, fp, ip, fp, C.c_uint32, C.c_uint32]
    L.zdr_scene_set_pmj02bn_tables.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_uint32]
    L.zdr_render_forward.argtypes = [vp, C.POINTER(RenderParams), fp, fp, vp]
    L.zdr_render_backward.argtypes = [vp, C.POINTER(RenderParams), fp, fp, fp, vp]
    L.zdr_scene_set_material_slots.argtypes = [vp, ip, vp]
    L.zdr_render_forward_materials.argtypes = [vp, C.POINTER(RenderParams), fp, ip, C.c_uint32, fp, vp]
    L.zdr_render_backward_materials.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.c_uint32, fp, vp]
    L.zdr_scene_set_envmap_texture.argtypes = [vp, fp, vp]
    L.zdr_scene_update_envmap_sampling.argtypes = [vp, C.c_int, vp]
    L.zdr_scene_get_envmap_sampling.argtypes = [vp, fp, ip, fp, vp]
    L.zdr_render_backward_env.argtypes = [vp, C.POINTER(RenderParams), fp, fp, fp, fp, vp]
    L.zdr_render_backward_materials_env.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.c_uint32, fp, fp, vp]
    L.zdr_scene_set_emission_values.argtypes = [vp, fp, vp]
    L.zdr_render_backward_emission.argtypes = [vp, C.POINTER(RenderParams), fp, fp, fp, fp, vp]
    L.zdr_render_backward_materials_emission.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.c_uint32, fp, fp, vp]
    L.zdr_render_aovs.argtypes = [vp, C.POINTER(RenderParams), fp, ip, C.c_uint32, fp, vp]
    L.zdr_render_aovs_backward.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.c_uint32, fp, vp]
    L.zdr_denoise_workspace_bytes.argtypes = [C.POINTER(DenoiseParams)]
    L.zdr_denoise_workspace_bytes.restype = C.c_size_t
    L.zdr_denoise.argtypes = [C.POINTER(DenoiseParams), fp, fp, fp, vp, vp]
    L.zdr_denoise_backward.argtypes = [C.POINTER(DenoiseParams), fp, fp, fp, vp, vp]
    L.zdr_texel_aovs_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_aovs_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_aovs.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, vp, vp]
    L.zdr_texel_lighting_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_lighting_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_lighting.argtypes = [vp, C.POINTER(TexelLightingParams), fp, fp, vp, vp]
    L.zdr_texel_lighting_backward_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int32]
    L.zdr_texel_lighting_backward_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_lighting_backward.argtypes = [vp, C.POINTER(TexelLightingParams), fp, fp, fp, fp, vp, vp]
    L.zdr_texel_bounce_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_bounce_workspace_bytes.restype = C.c_size_t
    L.zdr_texel_bounce_lanes_shift.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32]
    L.zdr_scene_texel_bounce.argtypes = [vp, C.POINTER(TexelBounceParams), fp, fp, ip, C.c_uint32, fp, vp, vp]
    L.zdr_texel_bounce_dump.argtypes = [vp, C.POINTER(TexelBounceParams), fp, fp, ip, C.c_uint32, ip, C.c_uint32, fp, vp]
    L.zdr_texel_bounce_backward_workspace_bytes.argtypes = [vp, C.c_int32, C.c_int32, ip, C.c_uint32]
    L.zdr_texel_bounce_backward_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_bounce_backward.argtypes = [vp, C.POINTER(TexelBounceParams), fp, fp, fp, ip, C.c_uint32, fp, fp, vp, vp]
    L.zdr_texel_bounce_backward_env_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_bounce_backward_env_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_bounce_backward_env.argtypes = [vp, C.POINTER(TexelBounceParams), fp, fp, fp, ip, C.c_uint32, fp, vp, vp]
    L.zdr_push_pull_workspace_bytes.argtypes = [C.POINTER(PushPullParams)]
    L.zdr_push_pull_workspace_bytes.restype = C.c_size_t
    L.zdr_push_pull.argtypes = [C.POINTER(PushPullParams), fp, fp, fp, vp, vp]
    L.zdr_push_pull_backward.argtypes = [C.POINTER(PushPullParams), fp, fp, fp, vp, vp]
    L.zdr_texel_view_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_view_workspace_bytes.restype = C.c_size_t
    L.zdr_scene_texel_view.argtypes = [vp, C.POINTER(TexelViewParams), fp, fp, vp, vp]
    L.zdr_texel_gather.argtypes = [C.POINTER(TexelGatherParams), fp, fp, fp, vp]
    L.zdr_texel_gather_backward.argtypes = [C.POINTER(TexelGatherParams), fp, fp, fp, vp]
    L.zdr_image_pyramid_bytes.argtypes = [C.POINTER(ImagePyramidParams)]
    L.zdr_image_pyramid_bytes.restype = C.c_size_t
    L.zdr_image_pyramid.argtypes = [C.POINTER(ImagePyramidParams), fp, fp, vp]
    L.zdr_image_pyramid_backward.argtypes = [C.POINTER(ImagePyramidParams), fp, fp, vp]
    L.zdr_texel_gather_mip.argtypes = [C.POINTER(TexelGatherMipParams), fp, fp, fp, fp, vp]
    L.zdr_texel_gather_mip_backward.argtypes = [C.POINTER(TexelGatherMipParams), fp, fp, fp, fp, vp]
    L.zdr_texel_footprint.argtypes = [C.POINTER(TexelFootprintParams), fp, fp, vp]
    L.zdr_texel_gather_aniso.argtypes = [C.POINTER(TexelGatherAnisoParams), fp, fp, fp, fp, fp, vp]
    L.zdr_texel_gather_aniso_backward.argtypes = [C.POINTER(TexelGatherAnisoParams), fp, fp, fp, fp, fp, vp]
    L.zdr_gather_plan_rows.argtypes = [C.POINTER(GatherPlanParams)]
    L.zdr_gather_plan_rows.restype = C.c_size_t
    L.zdr_gather_plan_workspace_bytes.argtypes = [C.POINTER(GatherPlanParams), C.c_uint64]
    L.zdr_gather_plan_workspace_bytes.restype = C.c_size_t
    L.zdr_gather_plan_count.argtypes = [C.POINTER(GatherPlanParams), fp, fp, vp, vp]
    L.zdr_gather_plan_build.argtypes = [C.POINTER(GatherPlanParams), fp, fp, C.c_uint64, vp, vp, vp, vp]
    L.zdr_gather_plan_apply.argtypes = [C.POINTER(GatherPlanParams), vp, vp, fp, fp, fp, vp]
    L.zdr_texel_gather_dview.argtypes = [C.POINTER(TexelGatherDviewParams), fp, fp, fp, fp, fp, vp]
    L.zdr_texel_view_backward_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.zdr_texel_view_backward_workspace_bytes.restype = C.c_size_t
    L.zdr_texel_view_backward.argtypes = [C.POINTER(TexelViewParams), fp, fp, fp, vp, vp]
    L.zdr_scene_texel_tangents.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, fp, vp, vp]
    L.zdr_texel_footprint_tangents.argtypes = [C.POINTER(TexelFootprintParams), fp, fp, fp, vp]
    L.zdr_render_stats.argtypes = [vp, C.POINTER(RenderParams), fp, C.POINTER(C.c_uint64), vp]
    L.zdr_scene_check.argtypes = [vp, vp]
    L.zdr_trace_closest.argtypes = [vp, fp, C.c_uint32, ip, fp, vp]
    L.zdr_trace_any.argtypes = [vp, fp, C.c_uint32, ip, vp]
    L.zdr_sampler_dump.argtypes = [vp, C.c_int32, C.c_uint32, C.c_uint32, ip, C.c_uint32, C.c_int32, C.c_int32, fp, vp]
    L.zdr_vertex_sampler_dump.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, ip, C.c_uint32, C.c_int32, C.c_int32, fp, C.POINTER(C.c_int32), vp]
    L.zdr_path_dump.argtypes = [vp, C.POINTER(RenderParams), fp, fp, ip, C.c_uint32, C.c_int32, fp, vp]
    L.zdr_trace_fused.argtypes = [vp, fp, fp, ip, C.c_uint32, C.c_int32, ip, ip, fp, vp]
    L.zdr_shading_dump.argtypes = [vp, C.c_int32, fp, C.c_uint32, fp, vp]
    L.zdr_light_dump.argtypes = [vp, C.c_int32, fp, C.c_uint32, fp, vp]
    L.zdr_texture_lookup.argtypes = [vp, fp, ip, C.c_uint32, fp, C.c_uint32, fp, vp]
    L.zdr_texture_scatter.argtypes = [vp, C.c_int32, ip, C.c_uint32, fp, C.c_uint32, C.c_uint32, fp, fp, ip, vp]
    L.zdr_debug_build_accel.argtypes = [fp, C.c_uint32, C.c_int, fp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), ip, fp]
    L.zdr_debug_never_occluders.argtypes = [fp, C.c_uint32, vp, vp]
    for name in EXPORTS:
        getattr(L, name)          # AttributeError here = header and library disagree
    if L.zdr_abi_version() != ABI_VERSION:
        raise ZdrError(f"{LIB_PATH} speaks ABI {L.zdr_abi_version()}, this binding ABI {ABI_VERSION}: rebuild (python -m zdr_amd.build --force)")
    _LIB = L
    return L


def check(rc: int):
    if rc != 0:
        raise ZdrError(f"libzdr_hip error {rc}: {lib().zdr_last_error().decode()}")
