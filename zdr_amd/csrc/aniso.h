// aniso.h — what the host side (zdr_api.cpp) asks of the anisotropic-gather kernels (zdr_aniso.hip): the per-texel footprint ellipse of a
// camera (zdr_texel_footprint), the gather of an image and its pyramid with several trilinear probes along the ellipse's major axis and
// that gather's adjoint (zdr_texel_gather_aniso, zdr_texel_gather_aniso_backward; include/zdr.h).  Like the mip kernels these live in a
// translation unit and a library of their own (libzdr_aniso.so, a dependency of libzdr_hip.so): nothing here is seen by any other
// kernel's object file.  The pyramid is zdr_image_pyramid's (csrc/mip.h, zdr_mip_plan), unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_ANISO_MAX_PROBES 16           // the largest max_aniso

// Wave-uniform arguments of the footprint kernel.  The camera frame is the one zdr_scene_texel_view derives (zdr_api.cpp, camera_frame).
struct AnisoFootprintArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 7 texel size, 8..10 position, 12 reach are read
    float4 *out;                      // (tex_h, tex_w, 4) floats: major axis x, y (pixels), minor, major
    uint32_t ntexels;
    float half_w, half_h;             // width / 2, height / 2 of the image
    float cam_o[3], cam_fwd[3], cam_right[3], cam_upp[3], cam_tan, aspect;
};

// Wave-uniform arguments of the anisotropic gather and of its adjoint.
struct AnisoGatherArgs {
    const float4 *view;               // (tex_h, tex_w, 8) floats: floats 0 (visible), 2 and 3 (X, Y) are read
    const float4 *foot;               // (tex_h, tex_w, 4) floats: the footprint buffer
    const float4 *in;                 // forward: the image (height, width, 4); adjoint: d_color (tex_h, tex_w, 4)
    const float4 *pyramid;            // forward: the levels >= 1 of the image
    float4 *out;                      // forward: color (tex_h, tex_w, 4), overwritten; adjoint: d_image (height, width, 4), added into
    float4 *d_pyramid;                // adjoint: the levels >= 1, added into
    uint32_t ntexels;
    int32_t width, height, L, max_aniso;
    float footprint;
};

// ZDR_ANISO_LAUNCHER_REF: as ZDR_MIP_LAUNCHER_REF of mip.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library linked
// without libzdr_aniso.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_ANISO_LAUNCHER_REF
#define ZDR_ANISO_LAUNCHER_REF
#endif
// one launch on `stream` each.  No allocation, no synchronisation.
ZDR_ANISO_LAUNCHER_REF int zdr_launch_texel_footprint(const AnisoFootprintArgs &A, hipStream_t stream);
ZDR_ANISO_LAUNCHER_REF int zdr_launch_texel_gather_aniso(const AnisoGatherArgs &G, int backward, hipStream_t stream);
