// denoise.h — what the host side (zdr_api.cpp) asks of the à-trous denoiser kernels (zdr_denoise.hip).  The kernels live in a translation
// unit of their own: nothing here is seen by zdr_kernels.hip, whose object file stays what it was.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Wave-uniform arguments of every denoiser launch (include/zdr.h, zdr_denoise: the formulas).  A term whose sigma is <= 0 is off.
struct DenoiseCfg {
    int32_t width, height;
    float inv_sn2;        // 1 / sigma_normal^2, 0 = off
    float half_sz;        // sigma_depth / 2,    0 = off
    float inv_sa2;        // 1 / sigma_albedo^2, 0 = off
};

// What one launch of a level computes for every pixel p, with w = w_l(p, q) over the 25 taps q = p + step (i, j) inside the image:
enum {
    ZDR_DENOISE_FILTER = 0,     // dst(p) = sum_q w src(q) / sum_q w      (one level of the forward)
    ZDR_DENOISE_DIVIDE = 1,     // dst(p) = src(p) / sum_q w              (adjoint, first half: g / D_l)
    ZDR_DENOISE_GATHER = 2,     // dst(p) = sum_q w src(q)                (adjoint, second half: w is symmetric, so the transpose is this gather)
};

// aovs: (H, W, 16) floats as float4; guides: 2 float4 per pixel, {n.xyz, z} and {a.rgb, id}.
// ZDR_DENOISE_LAUNCHER_REF: zdr_api.cpp alone defines it, as a weak attribute, so that ITS references are weak while the definitions in
// zdr_denoise.hip stay strong: a library linked from zdr_api.o and the path kernels alone (the host-side sanitizer build of
// tests/test_host_sanitizers.py) still loads and checks arguments, finds the two addresses null and refuses to launch (ZDR_E_UNSUPPORTED).
#ifndef ZDR_DENOISE_LAUNCHER_REF
#define ZDR_DENOISE_LAUNCHER_REF
#endif
ZDR_DENOISE_LAUNCHER_REF int zdr_launch_denoise_guides(const DenoiseCfg &R, const float4 *aovs, float4 *guides, hipStream_t stream);
ZDR_DENOISE_LAUNCHER_REF int zdr_launch_denoise_level(const DenoiseCfg &R, int mode, int step, const float4 *guides, const float4 *src, float4 *dst,
                                                      hipStream_t stream);
