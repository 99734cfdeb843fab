// bounceenv.h — what the host side (zdr_api.cpp) asks of the adjoint of the bounced-light baker in the environment map
// (zdr_bounceenv.hip): the gradient of zdr_scene_texel_bounce's irradiance in the map's texels, zdr_scene_texel_bounce_backward_env
// (include/zdr.h).  A translation unit and a library of its own (libzdr_bounceenv.so, a dependency of libzdr_hip.so): libzdr_bounce.so
// and libzdr_bouncegrad.so keep exactly their kernels, and neither zdr_bounce.hip nor zdr_bouncegrad.hip is touched — this adjoint
// carries its own copy of the walk, and none of the records, sweeps and queues of k_bgrad_shade.
#pragma once
#include "internal.h"
#include "bounce.h"
#include "bakegrad.h"                 // ZDR_LGRAD_MERGE_ROUNDS: the merge is k_lgrad_shade's

// Workspace: the header of ZDR_BOUNCE_HEADER_BYTES — word 0 the list's counter, word 1 the number of accepted environment samples, word 2
// the number of (cell, 12 floats) groups that went to memory after the wave-level merge (tools/texel_bounce_envgrad_cost.py reads both) —
// then the list (ntexels words, padded to 16 bytes).

// Wave-uniform arguments of the launches.
struct BenvArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 8..10 position, 12 reach are read
    const float4 *d_out;              // (tex_h, tex_w) float4 cotangent: .xyz of the shaded texels is read
    const float4 *materials;          // the packed materials of the table
    float *d_env;                     // (env_h, env_w, 4) floats, rgb added into (alpha never)
    uint32_t *count;                  // workspace: the header
    uint32_t *list;                   // workspace: the shaded texels, in any order
    uint32_t ntexels; int32_t tex_w;
    uint32_t sample_begin, sample_end;
    float inv_spp;                    // 1 / spp as computed by IEEE division
    int32_t bounces;                  // K, 1 .. ZDR_BOUNCE_MAX_BOUNCES
    int32_t wide_offsets;             // the packed materials do not end within 4 GiB (read_bsdf_in, scene.h)
};

// ZDR_BOUNCEENV_LAUNCHER_REF: as ZDR_BOUNCE_LAUNCHER_REF of bounce.h.
#ifndef ZDR_BOUNCEENV_LAUNCHER_REF
#define ZDR_BOUNCEENV_LAUNCHER_REF
#endif
// three launches on `stream`: clear the header; compact; the replay of k_bounce_shade that scatters into the map.  The scene has a map
// (the caller checks).  No allocation, no synchronisation.  Returns 0, or 256 x (the launch that failed, 1 .. 3) + its hipError_t; a
// launch that fails ends the call there.
ZDR_BOUNCEENV_LAUNCHER_REF int zdr_launch_texel_bounce_backward_env(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const BenvArgs &G, const MaterialTable &mt, hipStream_t stream);
