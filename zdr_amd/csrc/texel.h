// texel.h — what the host side (zdr_api.cpp) asks of the texture-space rasteriser (zdr_texel.hip): the per-texel feature buffers of
// zdr_scene_texel_aovs (include/zdr.h).  Like the denoiser's and the environment-table kernels, these live in a translation unit of
// their own: nothing here is seen by zdr_kernels.hip, whose object file stays what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_TEXEL_EMPTY 0xFFFFFFFFu       // a key no triangle has written (a triangle's key is its global input index g < 2^25)
#define ZDR_TEXEL_MAX_TEXELS (1u << 26)   // texel indices, and 64-byte rows of the output within 4 GiB
#define ZDR_TEXEL_MAX_DIM (1 << 24)       // lattice coordinates are exact in float32

// Wave-uniform arguments of the three launches.  The scene's records are read as they are (csrc/scene.h: the 128-byte shade record);
// nothing of the acceleration structure is.
struct TexelArgs {
    const float4 *shade;              // 8 float4 per slot
    const int32_t *slot_of_tri;       // global input index g -> slot
    const int32_t *inst_tri_begin;    // ninst + 1
    const int32_t *inst_slot;         // ninst material slots, -1 = none; nullptr = the table was never set: every slot is -1
    int32_t ntris, material, tex_h, tex_w;
    uint2 *keys;                      // workspace: per texel {lowest g that covers it, lowest g that reaches it}
    float4 *aovs;                     // (tex_h, tex_w, 16) floats
};

// ZDR_TEXEL_LAUNCHER_REF: as ZDR_DENOISE_LAUNCHER_REF of denoise.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_texel.so (zdr_amd/build.py: the kernels' own library, a dependency of libzdr_hip.so) still loads, finds the address
// null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_TEXEL_LAUNCHER_REF
#define ZDR_TEXEL_LAUNCHER_REF
#endif
// three launches on `stream`: clear, raster, resolve.  No allocation, no synchronisation.
ZDR_TEXEL_LAUNCHER_REF int zdr_launch_texel_aovs(const TexelArgs &A, hipStream_t stream);
