// zdr_denoise.hip — the feature-guided à-trous denoiser of include/zdr.h (zdr_denoise, zdr_denoise_backward) for gfx950.
//
// Three kernels, all one thread per pixel in 32 x 8 tiles (a wave = two rows of 32 pixels, so each tap of a wave is two 512-byte
// runs of the source and two 1 KiB runs of the guides), every launch covering the image with a bounds check (tiles numbered in grid.x):
//   k_denoise_guides        the prepass: (H, W, 16) feature buffers -> two float4 per pixel, {n.xyz, z} and {a.rgb, id}, divided by
//                           coverage once so that the 25 taps of every level read 32 bytes per neighbour and not 64;
//   k_denoise_level<MODE>   one level at a given step: the 25 weights from the packed guides and, by MODE (denoise.h), the normalised
//                           filter of the forward, the division g / D of the adjoint, or the adjoint's plain gather.
// The weights are symmetric in (p, q), so the transpose of a level is a gather over the same taps of g / D: no atomics, the same
// sum order in every run.  Levels depend on the whole previous level and are separate launches (zdr_api.cpp ping-pongs the buffers).
// Taps are plain cached loads at every step; out-of-image taps read the centre pixel again and get weight 0, which keeps the loop
// free of branches.  No LDS, no scratch (tests/test_denoise_resources.py).
#include "denoise.h"

#define DN_TILE_X 32
#define DN_TILE_Y 8

// tiles numbered row by row in grid.x alone (grid.y ends at 65,535: an image 1 pixel wide and 600,000 high is a valid one); at most
// 2^30 pixels (zdr_api.cpp) are at most 2^27 tiles
__host__ __device__ __forceinline__ int dn_tiles_x(const DenoiseCfg &R) { return (R.width + DN_TILE_X - 1) / DN_TILE_X; }

__global__ __launch_bounds__(DN_TILE_X * DN_TILE_Y) void k_denoise_guides(DenoiseCfg R, const float4 *__restrict__ aovs, float4 *__restrict__ guides) {
    const int tx = dn_tiles_x(R), ty = (int)(blockIdx.x / (unsigned)tx);
    const int x = ((int)blockIdx.x - ty * tx) * DN_TILE_X + (threadIdx.x & (DN_TILE_X - 1)), y = ty * DN_TILE_Y + threadIdx.x / DN_TILE_X;
    if (x >= R.width || y >= R.height) return;
    const uint32_t p = (uint32_t)y * (uint32_t)R.width + (uint32_t)x;
    const float4 a = aovs[4 * (size_t)p], n = aovs[4 * (size_t)p + 1];          // {albedo.rgb, roughness}, {normal.xyz, depth}
    const float c = aovs[4 * (size_t)p + 2].w, id = aovs[4 * (size_t)p + 3].z;  // coverage (11), instance (14)
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), g1 = make_float4(0.f, 0.f, 0.f, id);
    if (c > 0.f) {
        g0 = make_float4(n.x / c, n.y / c, n.z / c, n.w / c);
        g1 = make_float4(a.x / c, a.y / c, a.z / c, id);
    }
    guides[2 * (size_t)p] = g0;
    guides[2 * (size_t)p + 1] = g1;
}

// b = (1/16, 1/4, 3/8, 1/4, 1/16) by |offset|
__device__ __forceinline__ float b3(int k) { return k == 0 ? 0.375f : (k == 1 || k == -1) ? 0.25f : 0.0625f; }

template <int MODE>
__global__ __launch_bounds__(DN_TILE_X * DN_TILE_Y) void k_denoise_level(DenoiseCfg R, int step, const float4 *__restrict__ guides,
                                                                         const float4 *__restrict__ src, float4 *__restrict__ dst) {
    const int tx = dn_tiles_x(R), ty = (int)(blockIdx.x / (unsigned)tx);
    const int x = ((int)blockIdx.x - ty * tx) * DN_TILE_X + (threadIdx.x & (DN_TILE_X - 1)), y = ty * DN_TILE_Y + threadIdx.x / DN_TILE_X;
    if (x >= R.width || y >= R.height) return;
    const uint32_t W = (uint32_t)R.width, p = (uint32_t)y * W + (uint32_t)x;
    const float4 p0 = guides[2 * (size_t)p], p1 = guides[2 * (size_t)p + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float D = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const int yq = y + j * step;
        const bool row_in = (unsigned)yq < (unsigned)R.height;
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int xq = x + i * step;
            const bool in = row_in && (unsigned)xq < (unsigned)R.width;
            const uint32_t q = in ? (uint32_t)yq * W + (uint32_t)xq : p;
            const float4 q0 = guides[2 * (size_t)q], q1 = guides[2 * (size_t)q + 1];
            const float nx = p0.x - q0.x, ny = p0.y - q0.y, nz = p0.z - q0.z, dz = p0.w - q0.w;
            const float ax = p1.x - q1.x, ay = p1.y - q1.y, az = p1.z - q1.z;
            float T = (nx * nx + ny * ny + nz * nz) * R.inv_sn2 + (ax * ax + ay * ay + az * az) * R.inv_sa2;
            if (R.half_sz > 0.f) {                                   // (wave-uniform)
                const float m = R.half_sz * (p0.w + q0.w);
                T += dz * dz * __builtin_amdgcn_rcpf(m * m + 1e-20f);
            }
            const float w = (in && p1.w == q1.w) ? b3(i) * b3(j) * __expf(-T) : 0.f;
            D += w;
            if (MODE != ZDR_DENOISE_DIVIDE) {
                const float4 v = src[q];
                acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
            }
        }
    }
    if (MODE == ZDR_DENOISE_DIVIDE) acc = src[p];
    if (MODE != ZDR_DENOISE_GATHER) {                                // D >= w(p, p) = 9/64
        const float r = 1.f / D;
        acc.x *= r; acc.y *= r; acc.z *= r; acc.w *= r;
    }
    dst[p] = acc;
}

static dim3 dn_grid(const DenoiseCfg &R) {
    return dim3((unsigned)dn_tiles_x(R) * (unsigned)((R.height + DN_TILE_Y - 1) / DN_TILE_Y));
}

int zdr_launch_denoise_guides(const DenoiseCfg &R, const float4 *aovs, float4 *guides, hipStream_t st) {
    hipLaunchKernelGGL(k_denoise_guides, dn_grid(R), dim3(DN_TILE_X * DN_TILE_Y), 0, st, R, aovs, guides);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_denoise_level(const DenoiseCfg &R, int mode, int step, const float4 *guides, const float4 *src, float4 *dst, hipStream_t st) {
    const dim3 grid = dn_grid(R), block(DN_TILE_X * DN_TILE_Y);
    if (mode == ZDR_DENOISE_FILTER) hipLaunchKernelGGL(k_denoise_level<ZDR_DENOISE_FILTER>, grid, block, 0, st, R, step, guides, src, dst);
    else if (mode == ZDR_DENOISE_DIVIDE) hipLaunchKernelGGL(k_denoise_level<ZDR_DENOISE_DIVIDE>, grid, block, 0, st, R, step, guides, src, dst);
    else hipLaunchKernelGGL(k_denoise_level<ZDR_DENOISE_GATHER>, grid, block, 0, st, R, step, guides, src, dst);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
