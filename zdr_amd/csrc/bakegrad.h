// bakegrad.h — what the host side (zdr_api.cpp) asks of the adjoint of the texture-space light baker (zdr_bakegrad.hip): the gradient of
// zdr_scene_texel_lighting's irradiance in the lights' emissions and in the environment map, zdr_scene_texel_lighting_backward
// (include/zdr.h).  A translation unit and a library of its own (libzdr_bakegrad.so, a dependency of libzdr_hip.so): libzdr_bake.so keeps
// exactly the ten kernels it had, and zdr_bake.hip is not touched.
#pragma once
#include "internal.h"
#include "bake.h"

#define ZDR_LGRAD_COPIES 256          // rows of the emission accumulator: a wave adds its table into row blockIdx % ZDR_LGRAD_COPIES
#define ZDR_LGRAD_LDS_LIGHTS 32       // lights whose three floats a wave sums in LDS; a light beyond them adds into the row directly
#define ZDR_LGRAD_MERGE_ROUNDS 4      // map cells a wave merges per trip before its lanes go to memory one by one

// Workspace: the header of ZDR_BAKE_HEADER_BYTES — word 0 the list's counter, word 1 the number of accepted environment samples, word 2 the
// number of (cell, 12 floats) groups that went to memory after the wave-level merge (tools/texel_lighting_grad_cost.py reads both) —
// then the list (ntexels words, padded to 16 bytes), then the emission accumulator, ZDR_LGRAD_COPIES x light_count x 3 floats.

// Wave-uniform arguments of the four launches.
struct LgradArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 8..10 position, 12 reach are read
    const float4 *d_out;              // (tex_h, tex_w) float4 cotangent: .xyz of the shaded texels is read
    float *d_env;                     // (env_h, env_w, 4) floats, added into (alpha never), or null
    float *d_emission;                // (ninst, 3) floats, added into, or null
    float *acc;                       // workspace: the emission accumulator (zeroed by the first launch); null with d_emission
    uint32_t *count;                  // workspace: the header
    uint32_t *list;                   // workspace: the shaded texels, in any order
    uint32_t ntexels; int32_t tex_w;
    uint32_t sample_begin, sample_end;
    float inv_spp;                    // 1 / spp as computed by IEEE division
};

// ZDR_BAKEGRAD_LAUNCHER_REF: as ZDR_BAKE_LAUNCHER_REF of bake.h.
#ifndef ZDR_BAKEGRAD_LAUNCHER_REF
#define ZDR_BAKEGRAD_LAUNCHER_REF
#endif
// four launches on `stream` (three without d_emission): clear the header and the accumulator, compact, the adjoint of k_bake_shade, the
// gather of the accumulator's rows into d_emission.  No allocation, no synchronisation.  Returns 0, or 256 x (the launch that failed,
// 1 .. 4) + its hipError_t; a launch that fails ends the call there.
ZDR_BAKEGRAD_LAUNCHER_REF int zdr_launch_texel_lighting_backward(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const LgradArgs &G, hipStream_t stream);
