// project.h — what the host side (zdr_api.cpp) asks of the projective-texturing kernels (zdr_project.hip): the per-texel view buffer of a
// camera (zdr_scene_texel_view), the bilinear gather of an image through it and the gather's adjoint (zdr_texel_gather,
// zdr_texel_gather_backward; include/zdr.h).  Like the baker's and the push-pull kernels these live in a translation unit and a library
// of their own (libzdr_project.so, a dependency of libzdr_hip.so): nothing here is seen by any other kernel's object file.
#pragma once
#include "internal.h"

#define ZDR_PROJECT_HEADER_BYTES 16        // the workspace begins with the list's counter, padded to 16 bytes; the list follows

// Wave-uniform arguments of the three launches of the view buffer.  The camera frame is the one make_render_cfg gives a render
// (zdr_api.cpp, camera_frame).
struct ProjViewArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 7 texel size, 8..10 position, 12 reach are read
    float4 *out;                      // (tex_h, tex_w, 8) floats
    uint32_t *count;                  // workspace: number of list entries (zeroed by the first launch)
    uint32_t *list;                   // workspace: the texels with reach == 1 and no NaN in position or normal, in any order
    uint32_t ntexels; int32_t tex_w, tex_h;
    float width, height, half_w, half_h;      // the image's size as floats; width / 2, height / 2
    float cam_o[3], cam_fwd[3], cam_right[3], cam_upp[3], cam_tan, aspect;
};

// Wave-uniform arguments of the gather and of its adjoint.
struct ProjGatherArgs {
    const float4 *view;               // (tex_h, tex_w, 8) floats: floats 0 (visible), 2 and 3 (X, Y) are read
    const float4 *in;                 // forward: the image (height, width, 4); adjoint: d_color (tex_h, tex_w, 4)
    float4 *out;                      // forward: color (tex_h, tex_w, 4), overwritten; adjoint: d_image (height, width, 4), added into
    uint32_t ntexels;
    int32_t width, height;
};

// ZDR_PROJECT_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_project.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_PROJECT_LAUNCHER_REF
#define ZDR_PROJECT_LAUNCHER_REF
#endif
// three launches on `stream`: clear the counter, compact (and zero the texels that are not shaded), walk.  No allocation, no synchronisation.
ZDR_PROJECT_LAUNCHER_REF int zdr_launch_texel_view(const DScene &S, int accel_is_bvh, const ProjViewArgs &V, hipStream_t stream);
// one launch on `stream`: the gather, or with `backward` its adjoint.
ZDR_PROJECT_LAUNCHER_REF int zdr_launch_texel_gather(const ProjGatherArgs &G, int backward, hipStream_t stream);
