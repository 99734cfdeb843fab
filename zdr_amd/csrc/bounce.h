// bounce.h — what the host side (zdr_api.cpp) asks of the bounced-light baker (zdr_bounce.hip): per texel, the irradiance that arrives after
// at least one Lambertian bounce and the share of the hemisphere that can bounce light at all, zdr_scene_texel_bounce (include/zdr.h).
// A translation unit and a library of its own (libzdr_bounce.so, a dependency of libzdr_hip.so): libzdr_bake.so keeps exactly its kernels.
#pragma once
#include "internal.h"

#define ZDR_BOUNCE_MAX_TEXELS (1u << 26)  // texel indices x 64-byte rows of the input within 4 GiB (as ZDR_BAKE_MAX_TEXELS)
#define ZDR_BOUNCE_HEADER_BYTES 16        // the workspace begins with the list's counter, padded to 16 bytes; the list follows
#define ZDR_BOUNCE_MAX_LANES 64           // most lanes that share one texel's samples (one wave)
#define ZDR_BOUNCE_MAX_BOUNCES 8

// Wave-uniform arguments of the launches.
struct BounceArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 8..10 position, 12 reach are read
    float4 *out;                      // (tex_h, tex_w) float4 {irradiance.rgb, surface}
    uint32_t *count;                  // workspace: number of list entries (zeroed by the first launch)
    uint32_t *list;                   // workspace: the texels with reach == 1 and no NaN in position or normal, in any order
    const float4 *materials;          // the packed materials of the table
    uint32_t ntexels; int32_t tex_w;
    uint32_t sample_begin, sample_end;
    float inv_spp, spp_f;             // 1 / spp as computed by IEEE division; spp as a float
    int32_t bounces;                  // K, 1 .. ZDR_BOUNCE_MAX_BOUNCES
    int32_t wide_offsets;             // the packed materials do not end within 4 GiB (read_bsdf_in, scene.h)
};

// The launcher's rule for the lanes that share a texel's samples — the rule of zdr_launch_texel_lighting (zdr_bake.hip): enough lanes for
// the machine (256 CUs x 4 SIMDs x 4 waves x 64) when the texels alone are too few, never more than samples, a power of two so that a
// texel's lanes never straddle two waves.  From the texture's size and the length of the sample range alone.
static inline int zdr_bounce_lanes_shift(uint32_t ntexels, uint32_t nsamples) {
    const uint32_t want = (262144u + ntexels - 1u) / ntexels, cap = nsamples < ZDR_BOUNCE_MAX_LANES ? nsamples : ZDR_BOUNCE_MAX_LANES;
    int shift = 0;
    while ((2u << shift) <= cap && (1u << shift) < want) shift++;
    return shift;
}

// ZDR_BOUNCE_LAUNCHER_REF: as ZDR_BAKE_LAUNCHER_REF of bake.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without libzdr_bounce.so still loads, finds the address null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_BOUNCE_LAUNCHER_REF
#define ZDR_BOUNCE_LAUNCHER_REF
#endif
// three launches on `stream`: clear the counter, compact (and zero the texels that are not shaded), shade.  No allocation, no synchronisation.
ZDR_BOUNCE_LAUNCHER_REF int zdr_launch_texel_bounce(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt, hipStream_t stream);
// one launch: lane i walks query i = {x, y, s} and writes its row of 4 + 12 K floats (include/zdr.h, zdr_texel_bounce_dump)
ZDR_BOUNCE_LAUNCHER_REF int zdr_launch_texel_bounce_dump(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt,
                                                         const int32_t *queries, uint32_t n, float *out, hipStream_t stream);
