// bouncegrad.h — what the host side (zdr_api.cpp) asks of the adjoint of the bounced-light baker (zdr_bouncegrad.hip): the gradient of
// zdr_scene_texel_bounce's irradiance in the material texels and in the lights' emissions, zdr_scene_texel_bounce_backward
// (include/zdr.h).  A translation unit and a library of its own (libzdr_bouncegrad.so, a dependency of libzdr_hip.so): libzdr_bounce.so
// keeps exactly its kernels, and zdr_bounce.hip is not touched — the adjoint carries its own copy of the walk.
#pragma once
#include "internal.h"
#include "bounce.h"

#define ZDR_BGRAD_COPIES 256          // rows of the emission accumulator: a wave adds its table into row blockIdx % ZDR_BGRAD_COPIES
#define ZDR_BGRAD_LDS_LIGHTS 32       // lights whose three floats a wave sums in LDS; a light beyond them adds into the row directly
// The vertex records of a wave (dynamic LDS behind the traversal stacks), laid out [vertex][field][lane]: a field of a vertex is 64
// consecutive words, one per lane.  Fields: uv.x, uv.y, slot (-1: not shaded), A w .rgb (the reverse sweep leaves Q there), a.rgb.
#define ZDR_BGRAD_FIELDS 9

// Workspace: the header of ZDR_BOUNCE_HEADER_BYTES — word 0 the list's counter, word 1 the number of vertices pushed into the scatter queue
// (tools/texel_bounce_grad_cost.py reads it) —, then the list (ntexels words, padded to 16 bytes), then the emission accumulator,
// ZDR_BGRAD_COPIES x light_count x 3 floats (padded to 16 bytes), then the materials' staging cells with their copies, 64 bytes each, laid
// out by the rule of every material-table backward call (zdr_api.cpp, material_cell_layout).

// Wave-uniform arguments of the launches.
struct BgradArgs {
    const float4 *texels;             // (tex_h, tex_w, 16) floats: floats 4..6 normal, 8..10 position, 12 reach are read
    const float4 *d_out;              // (tex_h, tex_w) float4 cotangent: .xyz of the shaded texels is read
    const float4 *materials;          // the packed materials of the table
    float *d_materials;               // packed like the materials, rgb added into, or null
    float *d_emission;                // (ninst, 3) floats, added into, or null
    float *acc;                       // workspace: the emission accumulator (zeroed by the first launch); null with d_emission
    float *cells;                     // workspace: the staging cells (zeroed by the first launch); null with d_materials
    uint32_t *count;                  // workspace: the header
    uint32_t *list;                   // workspace: the shaded texels, in any order
    uint32_t ntexels; int32_t tex_w;
    uint32_t sample_begin, sample_end;
    float inv_spp;                    // 1 / spp as computed by IEEE division
    int32_t bounces;                  // K, 1 .. ZDR_BOUNCE_MAX_BOUNCES: sizes the records at launch
    int32_t wide_offsets;             // the packed materials do not end within 4 GiB (read_bsdf_in, scene.h)
    int32_t cell_copies;              // RenderCfg::cell_copies of the layout: copies of the whole cell array when it lives in LDS, else 1
    uint32_t ncell_words;             // float4 words of all staging cells, copies included (what the first launch zeroes)
};

// ZDR_BOUNCEGRAD_LAUNCHER_REF: as ZDR_BOUNCE_LAUNCHER_REF of bounce.h.
#ifndef ZDR_BOUNCEGRAD_LAUNCHER_REF
#define ZDR_BOUNCEGRAD_LAUNCHER_REF
#endif
// up to five launches on `stream`: clear the header, the accumulator and the cells; compact; the adjoint of k_bounce_shade; the gather of
// the cells into d_materials; the gather of the accumulator's rows into d_emission.  No allocation, no synchronisation.  Returns 0, or
// 256 x (the launch that failed, 1 .. 5) + its hipError_t; a launch that fails ends the call there.
ZDR_BOUNCEGRAD_LAUNCHER_REF int zdr_launch_texel_bounce_backward(const DScene &S, int accel_is_bvh, const SamplerCfg &C, const BgradArgs &G, const MaterialTable &mt, hipStream_t stream);
