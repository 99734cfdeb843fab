// internal.h — structures shared by the host side (zdr_api.cpp) and the kernels (zdr_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sampler.h"
#include "scene.h"
#include "zdr.h"

#define ZDR_MAX_RECORDED_DEPTH 16     // prb.py:15 max_depth; vertex records kept per path in backward

// primary ring (integrators.h): parked camera-ray vertices per lane, and camera samples generated per refill
#ifndef ZDR_RING_CAP
#define ZDR_RING_CAP 16
#endif
#ifndef ZDR_RING_BATCH
#define ZDR_RING_BATCH 8
#endif

#define ZDR_MAX_PERSISTENT_BLOCKS 8192   // 256 CUs x 4 SIMDs x 8 waves: upper bound of the path kernels' persistent grid

// Material table of the zdr_render_*_materials calls (zdr.h), a kernel argument like the rest of KernelIO so that a captured graph
// carries its own copy.  Material k is texels [texel, texel + h w) of the packed buffer; its staging cells have `copies` copies of
// (h + 1)(w + 1) cells, copy j at [cell + j stride, ...), and a wave adds into copy blockIdx % copies (zdr_api.cpp, material_cell_layout).
// The texture base pointer stays scalar; only the entry is per lane.
struct MaterialSlot { int32_t texel, h, w, cell, copies, stride; };
#define ZDR_ENV_CELL_BUDGET (1u << 22)   // environment gradient: most staging cells the map's copies take (256 MiB; zdr_api.cpp, render_common)
static_assert(ZDR_ENV_ENTRY == ZDR_MAX_MATERIALS - 1, "the environment-gradient calls keep the map in the last entry of the material table");
struct MaterialTable {
    const int32_t *inst_slot;         // ninst entries: material of each instance, -1 = none (zdr_scene_set_material_slots)
    int32_t nmat, ncells;             // materials in use; staging cells of all of them (of one copy when RenderCfg::cell_copies > 1)
    MaterialSlot m[ZDR_MAX_MATERIALS];
};

// Wave-uniform launch configuration (kernel argument, lives in SGPRs).
struct RenderCfg {
    int32_t width, height;
    int32_t x0, y0, x1, y1;
    uint32_t sample_begin, sample_end;
    uint32_t chunk;                   // samples per wave: chunk c covers [begin + c*chunk, ...)
    int32_t nchunks, tiles_x, tiles_y;
    int32_t shard_index, shard_count, ntiles;   // interleaved tile shard: tile numbers index, index + count, ... ; ntiles = how many that is
    int32_t shard_skew;                         // row r of the tile grid is numbered starting at column r * skew (1 when sharded: diagonals; 0 otherwise)
    int32_t use_tent, max_depth, rr_depth;
    int32_t tex_h, tex_w;
    int32_t prb_mode;                 // backward, path: ZDR_PRB_* of zdr.h (expectation / detached: roulette factors and MIS weights held constant / literal: the weight of prb.py:162)
    int32_t cell_copies;              // backward: replicas of the staging-cell array (scene.h: few texels), >= 1
    float two_over_w, two_over_h, aspect;      // integrator.py:22-23
    float inv_spp;                             // 1 / spp as computed by IEEE division
    float alpha;                               // (sample_end - sample_begin) / spp
    float cam_o[3], cam_fwd[3], cam_right[3], cam_upp[3], cam_tan;   // camera.py:12-15
    int32_t debug_no_scatter;         // measurement builds only (-DZDR_MEASURE, env ZDR_DEBUG_NO_SCATTER; always 0 in the product): timing-only ablations — 1 gradients computed, not added; 2 atomics confined to 64 KiB; 3 no sweep; 4 / 5 the sweep loop cut after 2 / 1 iterations (the tail of long paths dropped: what any scheme that defers it could save at most); 6 queue and flush run, no atomic is issued
};

struct KernelIO {
    const float4 *material;           // (tex_h, tex_w) float4
    float4 *image;                    // (H, W) float4
    union {                           // (one pointer: the struct keeps its size and layout, and with them the kernarg offsets of every kernel)
        float4 *partial;              // forward: scratch when nchunks > 1: [chunk][tile of the shard][lane] float4 (one 1 KiB line per wave)
        float *emit_acc;              // emission-gradient backward (zdr_render_backward_emission): ZDR_EMISSION_COPIES rows of light_count x 3 floats, zeroed per call; a wave adds into row blockIdx % ZDR_EMISSION_COPIES
    };
    const float4 *d_image;            // backward: cotangent
    float *d_material;                // backward: += gathered from the staging cells by k_cells_to_grad
    float *cells;                     // backward: (tex_h + 1) x (tex_w + 1) staging cells of 16 floats, zeroed per call
    unsigned long long *counters;     // stats variant: 8 counters
    const unsigned long long *tile_masks;   // brute-force accel: per 8x8 tile, the triangle pairs its camera rays can hit (k_tile_masks); null = all
    int32_t tile_masks_valid;               // the masks in the buffer already belong to this camera and shard: skip k_tile_masks
    int32_t wide_offsets;                   // the material (or the packed materials) or the image does not end within 4 GiB, or ZDR_WIDE_OFFSETS=1: read_bsdf, read_bsdf_in and the cotangent load of a popped path use 64-bit addresses instead of 32-bit byte offsets (scene.h, load_at).  (In the padding behind tile_masks_valid: the kernel arguments keep their offsets, and the kernels their register allocation.)
    unsigned int *work_counters;      // path integrator: 8 item counters, one per XCD, zeroed before the launch (fetch_item)
    float4 *ring;                     // path integrator: one FIFO of parked camera-ray vertices per persistent workgroup (integrators.h)
    MaterialTable mt;                 // material-table calls only (zdr_render_*_materials): `material` is then the packed buffer, `cells` all materials' cells
};

// What zdr_launch_render runs.  The two gradient targets beside d_material are optional and never given together:
struct RenderLaunch {
    int integrator, accel_is_bvh, backward, stats;
    float *d_env;         // environment-gradient backward (zdr_render_backward_env): io.mt is a material table whose entry ZDR_ENV_ENTRY holds
                          // the map's cells, and they are gathered into d_env (+=)
    float *d_emission;    // emission-gradient backward (zdr_render_backward_emission; the scene has at least one light): io.mt is a material
                          // table, io.emit_acc the zeroed accumulator, and its rows are gathered into d_emission (ninst x 3, +=)
    int aov;              // feature buffers (zdr_render_aovs / zdr_render_aovs_backward): k_aov / k_aov_bwd run whatever `integrator` says; io.mt is
                          // a material table, R has one chunk, io.image / io.d_image are (H, W, 16) and the cells are gathered like any table's
};
int zdr_launch_render(const DScene &S, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io, const RenderLaunch &L, hipStream_t stream);
#define ZDR_EMISSION_COPIES 256       // rows of the emission accumulator
int zdr_launch_set_emission_values(const DScene &S, const float *src, float *emission, float4 *emission4, float4 *light_tris, hipStream_t stream);
int zdr_launch_zero(void *p, size_t bytes, hipStream_t stream);   // kernel zero-fill (graph-safe, see zdr_kernels.hip)
int zdr_launch_copy(void *dst, const void *src, size_t bytes, hipStream_t stream);   // kernel copy of 16-byte words (graph-safe, as the zero-fill)
int zdr_launch_trace(const DScene &S, int accel_is_bvh, int any, const float *rays, uint32_t n,
                     int32_t *out_i, float *out_f, hipStream_t stream);
int zdr_launch_trace_fused(const DScene &S, const float *shadow, const float *next, const int32_t *need, uint32_t n, int backward_layout,
                           int32_t *occluded, int32_t *out_i, float *out_f, hipStream_t stream);   // BVH scenes only
int zdr_launch_shading_dump(int mode, const float *in, uint32_t n, float *out, hipStream_t stream);   // rows of 16 floats, include/zdr.h
int zdr_launch_light_dump(const DScene &S, int accel_is_bvh, int mode, const float *in, uint32_t n, float *out, hipStream_t stream);   // rows of 16 floats, include/zdr.h
int zdr_launch_texture_lookup(const DScene &S, const float *materials, const MaterialTable &mt, const float *rows, uint32_t n, float *out, hipStream_t stream);   // include/zdr.h, zdr_texture_lookup
// zdr_texture_scatter: the push kernel over `rows` (R and io laid out as for a backward call: cells zeroed, io.mt.nmat = 0 for the single
// material; table: the material-table instance; d_env: the one with the map as entry ZDR_ENV_ENTRY), then the folds of a backward call
int zdr_launch_texture_scatter(const RenderCfg &R, const KernelIO &io, int table, float *d_env, const float *rows, uint32_t n, uint32_t rounds, hipStream_t stream);
int zdr_launch_sampler_dump(const SamplerCfg &C, const int32_t *queries, uint32_t n, int32_t nvert,
                            int32_t rr_depth, float *out, int as_path_kernels, int *batched, hipStream_t stream);
int zdr_launch_path_dump(const DScene &S, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io, int accel_is_bvh,
                         const int32_t *queries, uint32_t n, int32_t maxv, float *out, hipStream_t stream);
