// bake.h — what the host side (zdr_api.cpp) asks of the texture-space light baker (zdr_bake.hip): direct irradiance and openness per texel,
// zdr_scene_texel_lighting (include/zdr.h).  Like the denoiser's, the environment-table and the rasteriser's kernels, these live in a
// translation unit of their own: nothing here is seen by zdr_kernels.hip, whose object file stays what it was.
#pragma once
#include "internal.h"

#define ZDR_BAKE_MAX_TEXELS (1u << 26)    // texel indices x 64-byte rows of the input within 4 GiB (as ZDR_TEXEL_MAX_TEXELS)
#define ZDR_BAKE_HEADER_BYTES 16          // the workspace begins with the list's counter, padded to 16 bytes; the list follows
#define ZDR_BAKE_MAX_LANES 64             // most lanes that share one texel's samples (one wave)

// Wave-uniform arguments of the three launches.
struct BakeArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 8..10 position, 12 reach are read
    float4 *out;                      // (tex_h, tex_w) float4 {irradiance.rgb, openness}
    uint32_t *count;                  // workspace: number of list entries (zeroed by the first launch)
    uint32_t *list;                   // workspace: the texels with reach == 1 and no NaN in position or normal, in any order
    uint32_t ntexels; int32_t tex_w;
    uint32_t sample_begin, sample_end;
    float inv_spp, spp_f;             // 1 / spp as computed by IEEE division; spp as a float
    float max_distance;
};

// ZDR_BAKE_LAUNCHER_REF: as ZDR_TEXEL_LAUNCHER_REF of texel.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_bake.so (zdr_amd/build.py: the kernels' own library, a dependency of libzdr_hip.so) still loads, finds the address
// null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_BAKE_LAUNCHER_REF
#define ZDR_BAKE_LAUNCHER_REF
#endif
// three launches on `stream`: clear the counter, compact (and zero the texels that are not shaded), shade.  No allocation, no synchronisation.
ZDR_BAKE_LAUNCHER_REF int zdr_launch_texel_lighting(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const BakeArgs &B, hipStream_t stream);
