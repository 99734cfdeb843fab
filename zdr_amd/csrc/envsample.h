// envsample.h — what the host side (zdr_api.cpp) asks of the kernels that rebuild the environment map's importance-sampling tables
// (zdr_envmap.hip).  Like the denoiser's, the kernels live in a translation unit of their own: nothing here is seen by zdr_kernels.hip
// or zdr_denoise.hip, whose object files stay what they were.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZDR_ENVS_W 512                // the sample map (zdr_amd/envmap.py: SAMPLE_MAP_W, SAMPLE_MAP_H); the kernels are written for this size
#define ZDR_ENVS_H 256
#define ZDR_ENVS_TAPS 17              // taps per axis of the weight map's filter, at offsets of 1/8 texel of the sample map
#define ZDR_ENVS_BLOCK 256            // lanes per workgroup of the per-texel kernels: one partial sum of the map's mean per workgroup
#define ZDR_ENVS_PARTIALS (ZDR_ENVS_W * ZDR_ENVS_H / ZDR_ENVS_BLOCK)

// The scene handle's workspace of a rebuild, allocated by its first call and kept.  row_factor and taps are constants that the host
// computes in double and fills once: the kernels only read them.
struct EnvSamplingScratch {
    float scale[ZDR_ENVS_W * ZDR_ENVS_H];   // the weight map; after the row kernel the weights the tables are built from (compensated, clamped)
    double partial[ZDR_ENVS_PARTIALS];      // sums of `scale` per workgroup of the weight kernel: summed again in a fixed order, no float atomics
    double row_total[ZDR_ENVS_H];           // sum of |weight| of each row
    double marginal_total[2];               // [0]: sum of |row average|
    double row_factor[ZDR_ENVS_H];          // MIS compensation: sin(pi (y + 1/2) / H) / mean_y sin(pi (y + 1/2) / H)
    float row_avg[ZDR_ENVS_H];              // mean weight of each row: the marginal table's values
    float taps[ZDR_ENVS_TAPS * ZDR_ENVS_TAPS + 3];   // exp(-4 (ox^2 + oy^2)), rows of dy; [289] = their sum
};

struct EnvSamplingArgs {
    const float4 *tex; int32_t env_h, env_w;         // the scene's texture (scene.h, env_lookup)
    float *alias_prob; int32_t *alias_idx; float *pdf;   // the scene's tables, in the layout of zdr_scene_set_envmap: marginal first, then the rows
    EnvSamplingScratch *scratch;
    int32_t compensate_mis;
};

// ZDR_ENVMAP_LAUNCHER_REF: as ZDR_DENOISE_LAUNCHER_REF of denoise.h — zdr_api.cpp alone defines it, as a weak attribute, so that a library
// linked without zdr_envmap.o (the host-side sanitizer build of tests/test_host_sanitizers.py) still loads, finds the address null and
// refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_ENVMAP_LAUNCHER_REF
#define ZDR_ENVMAP_LAUNCHER_REF
#endif
// four launches on `stream`: weight map, row tables, marginal table, pdf.  No allocation, no synchronisation.
ZDR_ENVMAP_LAUNCHER_REF int zdr_launch_envmap_sampling(const EnvSamplingArgs &A, hipStream_t stream);
