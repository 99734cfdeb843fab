// mip.h — what the host side (zdr_api.cpp) asks of the prefiltering kernels (zdr_mip.hip): the mip pyramid of an image and its adjoint
// (zdr_image_pyramid, zdr_image_pyramid_backward), the trilinear gather of an image and its pyramid through a view buffer and that
// gather's adjoint (zdr_texel_gather_mip, zdr_texel_gather_mip_backward; include/zdr.h).  Like the push-pull and the view kernels these
// live in a translation unit and a library of their own (libzdr_mip.so, a dependency of libzdr_hip.so): nothing here is seen by any
// other kernel's object file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_MIP_MAX_LEVELS 32           // 2^28 pixels (ZDR_FILTER_MAX_PIXELS, texel_filter.h) in one row end after 28 halvings
#define ZDR_MIP_TAIL_DIM 32             // a level of at most 32 x 32 and everything above it is one workgroup's work, in LDS
#define ZDR_MIP_TAIL_TEXELS 1368        // 32^2 + 16^2 + ... + 1 = 1365, rounded up to a multiple of 8

// The pyramid of one image: sizes of the levels 0 .. L and where the levels >= 1 sit in the packed buffer, one after another, a float4
// per pixel (so every level begins at a multiple of 16 bytes).  Level 0 is the image itself and is never copied.
struct MipPlan {
    int32_t L;                                       // the top level
    int32_t tail;                                    // the first level <= L that fits the fused tail, L + 1 if none does
    int32_t w[ZDR_MIP_MAX_LEVELS], h[ZDR_MIP_MAX_LEVELS];
    size_t off[ZDR_MIP_MAX_LEVELS];                  // in float4; [0] unused
    size_t bytes;                                    // of the packed buffer, never 0
};

static inline MipPlan zdr_mip_plan(int32_t width, int32_t height, int32_t levels) {
    MipPlan P;
    P.L = 0; P.w[0] = width; P.h[0] = height; P.off[0] = 0;
    size_t off = 0;
    while ((P.w[P.L] > 1 || P.h[P.L] > 1) && (levels <= 0 || P.L < levels) && P.L + 1 < ZDR_MIP_MAX_LEVELS) {
        const int l = ++P.L;
        P.w[l] = (P.w[l - 1] + 1) / 2; P.h[l] = (P.h[l - 1] + 1) / 2;
        P.off[l] = off; off += (size_t)P.w[l] * (size_t)P.h[l];
    }
    P.tail = P.L + 1;
    for (int l = 0; l <= P.L; l++)
        if (P.w[l] <= ZDR_MIP_TAIL_DIM && P.h[l] <= ZDR_MIP_TAIL_DIM) { P.tail = l; break; }
    P.bytes = off ? off * sizeof(float4) : 16;       // (an image without a level >= 1: the size is still not 0)
    return P;
}

// Wave-uniform arguments of the pyramid build and of its adjoint.
struct MipPyramidArgs {
    int32_t width, height, levels;
    const float4 *image;             // forward: level 0 (height, width, 4), read only
    float4 *d_image;                 // adjoint: (height, width, 4), added into
    float4 *pyramid;                 // forward: the levels >= 1, written; adjoint: their cotangents, read and used as a workspace
};

// Wave-uniform arguments of the mip gather and of its adjoint.
struct MipGatherArgs {
    const float4 *view;               // (tex_h, tex_w, 8) floats: floats 0 (visible), 2, 3 (X, Y) and 6 (scale) are read
    const float4 *in;                 // forward: the image (height, width, 4); adjoint: d_color (tex_h, tex_w, 4)
    const float4 *pyramid;            // forward: the levels >= 1 of the image
    float4 *out;                      // forward: color (tex_h, tex_w, 4), overwritten; adjoint: d_image (height, width, 4), added into
    float4 *d_pyramid;                // adjoint: the levels >= 1, added into
    uint32_t ntexels;
    int32_t width, height, L;
    float footprint;
};

// ZDR_MIP_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library linked
// without libzdr_mip.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_MIP_LAUNCHER_REF
#define ZDR_MIP_LAUNCHER_REF
#endif
// at most ceil(L / 2) + 1 launches on `stream`: two levels per launch, then (or, for the adjoint, first) the fused tail.  No allocation,
// no synchronisation.
ZDR_MIP_LAUNCHER_REF int zdr_launch_image_pyramid(const MipPyramidArgs &A, int backward, hipStream_t stream);
// one launch on `stream`: the gather, or with `backward` its adjoint.
ZDR_MIP_LAUNCHER_REF int zdr_launch_texel_gather_mip(const MipGatherArgs &G, int backward, hipStream_t stream);
