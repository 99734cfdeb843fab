// zdr_project.hip — projective texturing for gfx950 (include/zdr.h: zdr_scene_texel_view, zdr_texel_gather, zdr_texel_gather_backward):
// what a camera sees of each texel, the image it took gathered into texture space, and the adjoint of that gather.  The view buffer is
// one any-hit ray per texel, from the texel to the camera, through the path kernels' own walks (accel.h), instantiated here once more;
// the gather and its adjoint read no scene.  Linked into libzdr_project.so (zdr_amd/build.py), compiled without contraction: the
// gather's bits are defined by the operation order of include/zdr.h.
//
// The view buffer is three kernels, launched one after the other on the caller's stream, as zdr_bake.hip's:
//   k_proj_clear      the list's counter to 0;
//   k_proj_compact    thread = texel, tile by tile: a texel with reach == 1 and no NaN in its normal or position is appended to the list in
//                     the workspace (one integer atomic per workgroup of 2,048 texels: ballots, ranks); any other texel gets its eight
//                     zeros here.  The order of the list varies from run to run; no result depends on it;
//   k_proj_view       one wave per workgroup, lane = list entry: the projection, then the segment to the camera for the texels in front
//                     of it and inside its image.  The whole wave enters the walk: a lane without a ray — no list entry, behind the
//                     camera, outside the image — hands in an empty interval (tmax 0), which ends its walk at the root.  The walk is
//                     A::any, which meets every primitive: the shortcut of any_shadow is proven for light segments only.  The grid is
//                     sized for "every texel shaded"; workgroups beyond the list's end leave at once.  No float atomic: a texel's bits
//                     depend on its own row and the camera alone.
// The gather (k_proj_gather) is thread = texel, four loads and a store; its adjoint (k_proj_scatter) is thread = (texel, channel), one float atomic
// per tap and channel into d_image (-munsafe-fp-atomics: global_atomic_add_f32, no compare-and-swap loop).  The taps, the lerp and the
// adjoint's walk are texel_filter.h's, which the mip gather, the anisotropic gather and the gather plan share.
#include "accel.h"
#include "project.h"
#include "texel_filter.h"
#include <algorithm>

#define PROJ_WAVE 64

__global__ __launch_bounds__(64) void k_proj_clear(uint32_t *count) {
    if (threadIdx.x < ZDR_PROJECT_HEADER_BYTES / 4) count[threadIdx.x] = 0u;
}

// thread = texel of an 8 x 8 tile, a wave takes PROJ_TILES_PER_WAVE tiles one after the other, and the workgroup's four waves append
// with ONE returning atomic: a single counter answers about 90 such atomics a microsecond, so that one per wave and tile — 16,384 of
// them at 1024^2 — cost ten times what reading the texels does (measured: 140 us of a 160 us call).  Tiles, not strips of a row: the
// 64 list entries a wave of the walk draws then lie together on the surface.  The list's order reaches no result.
#define PROJ_TILES_PER_WAVE 8
struct ProjTexel { uint32_t t; bool inside; };
ZD ProjTexel proj_tile_texel(const ProjViewArgs &V, uint32_t tile, uint32_t lane) {
    const uint32_t tiles_x = ((uint32_t)V.tex_w + 7u) >> 3, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t x = 8u * tx + (lane & 7u), y = 8u * ty + (lane >> 3);
    ProjTexel r;
    r.inside = x < (uint32_t)V.tex_w && y < (uint32_t)V.tex_h;   // (then t < ntexels; a tile past the last one has y >= tex_h)
    r.t = y * (uint32_t)V.tex_w + x;
    return r;
}

__global__ __launch_bounds__(256) void k_proj_compact(ProjViewArgs V) {
    __shared__ uint32_t wave_total[4], block_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tile0 = (blockIdx.x * 4u + wave) * PROJ_TILES_PER_WAVE;
    unsigned long long masks[PROJ_TILES_PER_WAVE];
    uint32_t total = 0u;
#pragma unroll
    for (int k = 0; k < PROJ_TILES_PER_WAVE; k++) {
        const ProjTexel q = proj_tile_texel(V, tile0 + (uint32_t)k, lane);
        bool shade = false;
        if (q.inside) {
            const float4 *r = V.texels + 4 * (size_t)q.t;
            const float4 nrm = r[1], pos = r[2];
            const float reach = r[3].x;
            shade = (reach == 1.0f) && !any_nan(xyz(nrm)) && !any_nan(xyz(pos));
            if (!shade) { V.out[2 * (size_t)q.t] = make_float4(0.f, 0.f, 0.f, 0.f); V.out[2 * (size_t)q.t + 1] = make_float4(0.f, 0.f, 0.f, 0.f); }
        }
        masks[k] = __ballot(shade);
        total += (uint32_t)__popcll(masks[k]);
    }
    if (lane == 0u) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t sum = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        block_base = sum ? atomicAdd(V.count, sum) : 0u;
    }
    __syncthreads();
    uint32_t base = block_base;
    for (uint32_t w = 0; w < wave; w++) base += wave_total[w];
#pragma unroll
    for (int k = 0; k < PROJ_TILES_PER_WAVE; k++) {
        const unsigned long long m = masks[k];
        if ((m >> lane) & 1ull) {
            const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            V.list[at] = proj_tile_texel(V, tile0 + (uint32_t)k, lane).t;   // (at < ntexels: every texel is appended at most once)
        }
        base += (uint32_t)__popcll(m);
    }
}

template <class A>
__global__ __launch_bounds__(PROJ_WAVE) void k_proj_view(DScene S, ProjViewArgs V) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks (sized at launch); unused otherwise
    const uint32_t count = *V.count;
    if (blockIdx.x * PROJ_WAVE >= count) return;             // wave-uniform: the whole workgroup lies behind the list's end
    const uint32_t entry = blockIdx.x * PROJ_WAVE + threadIdx.x;
    const bool live = entry < count;
    const uint32_t t = live ? V.list[entry] : 0u;
    f3 n = mk3(0.0f, 0.0f, 1.0f), p = mk3(0.0f);
    float texel_size = 0.0f;
    if (live) {
        const uint32_t r = 64u * t;                          // (load_at, scene.h: at most 2^26 texels of 64 bytes)
        const float4 nr = load_at<float4>(V.texels, r, 16);
        n = xyz(nr); texel_size = nr.w; p = xyz(load_at<float4>(V.texels, r, 32));
    }
    // the inverse of pixel_ray (integrators.h), in the operation order of include/zdr.h; divisions and the root are IEEE
    const f3 o = ld3(V.cam_o), v = p - o, w = o - p;
    const float z = dot(v, ld3(V.cam_fwd)), dist = __fsqrt_rn(dot(v, v));
    const f3 wi = mk3(__fdiv_rn(w.x, dist), __fdiv_rn(w.y, dist), __fdiv_rn(w.z, dist));
    const float cosine = dot(n, wi);
    const bool front = z > 0.0f;
    float X = 0.0f, Y = 0.0f, scale = 0.0f;
    if (front) {
        X = (__fdiv_rn(__fdiv_rn(dot(v, ld3(V.cam_right)), z), V.cam_tan) + 1.0f) * V.half_w;
        Y = (__fdiv_rn(__fdiv_rn(-dot(v, ld3(V.cam_upp)), z), V.cam_tan * V.aspect) + 1.0f) * V.half_h;
        scale = __fdiv_rn(texel_size * V.half_w, V.cam_tan * z);
    }
    const bool inside = live && front && X >= 0.0f && X < V.width && Y >= 0.0f && Y < V.height;
    const bool occ = A::any(S, lds, p, wi, 1e-4f, inside ? dist : 0.0f);
    if (live) {
        const uint32_t r = 32u * t;
        store_at<float4>(V.out, r, 0, make_float4((inside && !occ) ? 1.0f : 0.0f, cosine, X, Y));
        store_at<float4>(V.out, r, 16, make_float4(z, dist, scale, 0.0f));
    }
}

__global__ __launch_bounds__(256) void k_proj_gather(ProjGatherArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];                 // {visible, cosine, X, Y}
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tf_on(vw.x)) {                                       // an invisible texel reads nothing of the image
        const float4 r = tf_sample(G.in, vw.z, vw.w, 0, tf_place(G.width, G.height, 0));
        c = make_float4(vw.x * r.x, vw.x * r.y, vw.x * r.z, vw.x * r.w);
    }
    G.out[t] = c;
}

// thread = (texel, channel): the four lanes of a texel add the four channels of a tap with ONE wave-instruction, 16 contiguous bytes
// per texel and, for neighbouring texels, neighbouring pixels — float atomics run at the memory side at a rate set by how few 64-byte
// segments a wave-instruction touches, and a lane per texel would spread each instruction over 64 pixels, a channel at a time.
__global__ __launch_bounds__(256) void k_proj_scatter(ProjGatherArgs G) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, t = id >> 2, c = id & 3u;   // (id < 4 ntexels <= 2^28)
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];
    if (!tf_on(vw.x)) return;
    const float g = ((const float *)G.in)[id];
    float *d = (float *)G.out + c;
    tf_enumerate(tf_texel(vw.x, vw.z, vw.w), TF_BILINEAR, 1.0f, G.width, G.height,
                 [&](bool, uint32_t pixel, float weight) { atomicAdd(d + 4 * (size_t)pixel, weight * g); });
}

int zdr_launch_texel_view(const DScene &S_in, int accel_is_bvh, const ProjViewArgs &V, hipStream_t st) {
    DScene S = S_in;
    // dynamic LDS of a wave that traverses the BVH, as zdr_launch_trace sizes it: the first entries of the per-lane stacks (accel.h)
    size_t dyn = 0;
    if (accel_is_bvh) { S.lds_stack = std::min<int>(S.stack_entries, ZDR_BVH_LDS_STACK); dyn = (size_t)S.lds_stack * PROJ_WAVE * sizeof(int); }
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    hipLaunchKernelGGL(k_proj_clear, dim3(1), dim3(64), 0, st, V.count);
    if (hipGetLastError() != hipSuccess) return -1;
    const uint32_t tiles = (((uint32_t)V.tex_w + 7u) >> 3) * (((uint32_t)V.tex_h + 7u) >> 3);   // < 2^26 + 2^24: a tile holds a texel
    hipLaunchKernelGGL(k_proj_compact, dim3((tiles + 4u * PROJ_TILES_PER_WAVE - 1u) / (4u * PROJ_TILES_PER_WAVE)), dim3(256), 0, st, V);
    if (hipGetLastError() != hipSuccess) return -1;
    const dim3 grid((V.ntexels + PROJ_WAVE - 1u) / PROJ_WAVE);
    if (accel_is_bvh) hipLaunchKernelGGL((k_proj_view<BvhAccel>), grid, dim3(PROJ_WAVE), dyn, st, S, V);
    else hipLaunchKernelGGL((k_proj_view<BruteAccel>), grid, dim3(PROJ_WAVE), dyn, st, S, V);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_texel_gather(const ProjGatherArgs &G, int backward, hipStream_t st) {
    const dim3 grid((G.ntexels + 255u) / 256u);
    if (backward) hipLaunchKernelGGL(k_proj_scatter, dim3((G.ntexels + 63u) / 64u), dim3(256), 0, st, G);
    else hipLaunchKernelGGL(k_proj_gather, grid, dim3(256), 0, st, G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
