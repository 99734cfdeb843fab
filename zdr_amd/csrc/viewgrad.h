// viewgrad.h — what the host side (zdr_api.cpp) asks of the camera-gradient kernels (zdr_viewgrad.hip): the cotangent of a view buffer
// from a gather's colour cotangent (zdr_texel_gather_dview) and the adjoint of the view buffer in the camera (zdr_texel_view_backward;
// include/zdr.h, "Camera gradients").  Like the other texel filters these live in a translation unit and a library of their own
// (libzdr_viewgrad.so, a dependency of libzdr_hip.so): nothing here is seen by any other kernel's object file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_VIEWGRAD_BLOCK 256             // lanes of a workgroup of either stage of the reduction (four waves)
#define ZDR_VIEWGRAD_MAX_ROWS 1024         // stage 1 has at most this many workgroups, each leaves one partial row
#define ZDR_VIEWGRAD_SUMS 13               // o (3), fwd (3), right (3), upp (3), tan
#define ZDR_VIEWGRAD_ROW 16                // doubles of a partial row in the workspace (13 sums, 3 never touched): 128 bytes

// the number of stage-1 workgroups = partial rows: a function of the number of texels alone
static inline uint32_t zdr_viewgrad_rows(uint32_t ntexels) {
    const uint32_t blocks = (ntexels + ZDR_VIEWGRAD_BLOCK - 1u) / ZDR_VIEWGRAD_BLOCK;
    return blocks < ZDR_VIEWGRAD_MAX_ROWS ? blocks : ZDR_VIEWGRAD_MAX_ROWS;
}

// Wave-uniform arguments of zdr_texel_gather_dview.
struct ViewGradDviewArgs {
    const float4 *view;               // (tex_h, tex_w, 8) floats: floats 0 (visible), 2, 3 (X, Y) and, mip, 6 (scale) are read
    const float4 *image;              // (height, width, 4)
    const float4 *pyramid;            // mip: the levels >= 1 of the image; bilinear: not read
    const float4 *d_color;            // (tex_h, tex_w, 4)
    float4 *out;                      // d_view (tex_h, tex_w, 8), overwritten
    uint32_t ntexels;
    int32_t width, height, L, filter; // filter: TF_BILINEAR or TF_MIP (texel_filter.h)
    float footprint;
};

// Wave-uniform arguments of the two stages of zdr_texel_view_backward.  The frame is the host's camera_frame, the very floats the
// forward projected with; target and up are the camera's own, for the chain rule through that frame.
struct ViewGradCameraArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 7 texel size, 8..10 position, 12 reach are read
    const float4 *d_view;             // (tex_h, tex_w, 8) floats: floats 1..6 of the shaded texels are read
    double *rows;                     // workspace: zdr_viewgrad_rows(ntexels) partial rows of ZDR_VIEWGRAD_ROW doubles
    float *d_camera;                  // 10 floats: fov, origin, target, up; overwritten
    uint32_t ntexels, nrows;
    float half_w, half_h, aspect;
    float cam_o[3], cam_fwd[3], cam_right[3], cam_upp[3], cam_tan;
    float target[3], up[3], fov;
};

// ZDR_VIEWGRAD_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_viewgrad.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_VIEWGRAD_LAUNCHER_REF
#define ZDR_VIEWGRAD_LAUNCHER_REF
#endif
// one launch on `stream`.  No allocation, no synchronisation.
ZDR_VIEWGRAD_LAUNCHER_REF int zdr_launch_texel_gather_dview(const ViewGradDviewArgs &G, hipStream_t stream);
// two launches on `stream`: the partial rows, then their sum and the chain rule.  No allocation, no synchronisation.
ZDR_VIEWGRAD_LAUNCHER_REF int zdr_launch_texel_view_backward(const ViewGradCameraArgs &A, hipStream_t stream);
