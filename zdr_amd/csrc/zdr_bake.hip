// zdr_bake.hip — the texture-space light baker of include/zdr.h (zdr_scene_texel_lighting) for gfx950: per texel, direct irradiance on the
// normal's side and the open fraction of the hemisphere.  The walk starts at the texels instead of at the camera; everything it calls —
// sample_light, env_lookup, make_onb, the samplers, the per-lane any-hit walks of both accelerators — is the path kernels' own device
// code (scene.h, accel.h, sampler.h), instantiated here a second time.  Linked into libzdr_bake.so (zdr_amd/build.py).
//
// Three kernels, launched one after the other on the caller's stream:
//   k_bake_clear      the list's counter to 0;
//   k_bake_compact    thread = texel: a texel with reach == 1 and no NaN in its normal or position is appended to the list in the
//                     workspace (one integer atomic per wave: ballot, rank); any other texel gets its four zeros here.  The order of the
//                     list varies from run to run; no result depends on it;
//   k_bake_shade      one wave per workgroup, lane = (list entry, j): 2^lanes_shift neighbouring lanes share a texel, lane j of them takes
//                     the samples begin + j, begin + j + lanes, ... and keeps their sum in sample order; lane 0 then adds the lanes' sums
//                     in lane order and writes the texel.  A texel's bits therefore depend on its own samples and on lanes_shift, which
//                     the launcher derives from the texture's size and the sample range alone — never on the grid, the list's order or the
//                     wave-mates: the walks are per lane (A::any, A::any_shadow), there is no float atomic.  The grid is sized for
//                     "every texel reached"; workgroups beyond the list's end leave at once, so nothing is read back to size it.
// The sample loop is wave-uniform (every lane makes the same number of trips) and the whole wave enters every walk: a lane without a
// ray — no list entry, no sample left, or a light sample that cannot add anything — hands in an empty interval (tmax 0), which ends
// its walk at the root.
#include "accel.h"
#include "bake.h"
#include <algorithm>

#define BAKE_WAVE 64

__global__ __launch_bounds__(64) void k_bake_clear(uint32_t *count) {
    if (threadIdx.x < ZDR_BAKE_HEADER_BYTES / 4) count[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(256) void k_bake_compact(BakeArgs B) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool shade = false;
    if (t < B.ntexels) {
        const float4 *r = B.texels + 4 * (size_t)t;
        const float4 nrm = r[1], pos = r[2];
        const float reach = r[3].x;
        shade = (reach == 1.0f) && !any_nan(xyz(nrm)) && !any_nan(xyz(pos));
        if (!shade) B.out[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const unsigned long long m = __ballot(shade);
    if (m == 0ull) return;                                   // wave-uniform
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0u;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(B.count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (shade) {
        const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        B.list[at] = t;                                      // (at < ntexels: every texel is appended at most once)
    }
}

ZD bool bake_finite(f3 a) { return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff(); }

template <int SK, class A, bool ENV>
__global__ __launch_bounds__(BAKE_WAVE) void k_bake_shade(DScene S, SamplerCfg C, BakeArgs B, int lanes_shift) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks (sized at launch); unused otherwise
    const uint32_t count = *B.count;
    const uint32_t item = blockIdx.x * BAKE_WAVE + threadIdx.x;
    if (((blockIdx.x * BAKE_WAVE) >> lanes_shift) >= count) return;     // wave-uniform: the whole workgroup lies behind the list's end
    const uint32_t lanes = 1u << lanes_shift, entry = item >> lanes_shift, j = item & (lanes - 1u);
    const bool live = entry < count;
    const uint32_t t = live ? B.list[entry] : 0u;
    f3 n = mk3(0.0f, 0.0f, 1.0f), p = mk3(0.0f);
    if (live) {
        const uint32_t r = 64u * t;                          // (load_at, scene.h: at most 2^26 texels of 64 bytes)
        n = xyz(load_at<float4>(B.texels, r, 16)); p = xyz(load_at<float4>(B.texels, r, 32));
    }
    const uint32_t y = t / (uint32_t)B.tex_w, x = t - y * (uint32_t)B.tex_w;
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4(x, y, C.seed, 0u) : 0u;
    const Onb onb = make_onb(n);
    f3 E = mk3(0.0f);
    float open = 0.0f;
    const uint32_t trips = (B.sample_end - B.sample_begin + lanes - 1u) >> lanes_shift;   // wave-uniform
#pragma unroll 1
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t s = B.sample_begin + j + (k << lanes_shift);
        const bool valid = live && s < B.sample_end;
        // a lane without a sample draws all the same (the wave stays together), from the range's first sample: the pmj02bn tables are
        // indexed with the sample index as it is, and one past sample_end may lie past their end
        Sampler smp = sampler_make<SK>(C, x, y, perm_seed, valid ? s : B.sample_begin);
        const f2 u_ao = sampler_next2<SK>(C, smp);
        const float u_pick = sampler_next<SK>(C, smp), u_prim = sampler_next<SK>(C, smp);
        const f2 u_pt = sampler_next2<SK>(C, smp);
        // openness: the cosine lobe of ggx_sample (microfacet.h) about n
        {
            const float r = fsqrt(u_ao.x), phi = 2.0f * ZDR_PI * u_ao.y;
            float sn, cs;
            sincosf(phi, &sn, &cs);
            const f3 dir = to_world(onb, mk3(r * cs, r * sn, fsqrt(1.0f - u_ao.x)));
            const bool ray = valid && !any_nan(dir);         // a ray of NaNs hits nothing (accel.h)
            const bool occ = A::any(S, lds, p, dir, 1e-4f, ray ? B.max_distance : 0.0f);
            if (valid && !(ray && occ)) open += 1.0f;
        }
        // irradiance: one light sample, the ray and the clamp of direct_sample (integrators.h)
        {
            const LightSample L = sample_light<ENV>(S, p, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; });
            const float c = dot(n, L.wi);
            const bool lit = valid && c > 0.0f && (L.eval.x > 0.0f || L.eval.y > 0.0f || L.eval.z > 0.0f);
            const bool occ = A::any_shadow(S, lds, p, L.wi, 1e-4f, lit ? L.dist : 0.0f);
            if (lit && !occ) {
                const f3 add = L.eval * (c * rcp(fmaxf(L.pdf, 1e-4f)));
                if (bake_finite(add)) E = E + add;
            }
        }
    }
    // the lanes of a texel, in lane order (every lane of the wave is here: the exit above is wave-uniform)
    f3 Es = E;
    float os = open;
    const int self = (int)(threadIdx.x & 63u);
    for (uint32_t k = 1; k < lanes; k++) {                   // wave-uniform
        const int src = (self + (int)k) & 63;                // (lane 0 of a texel reads its own lanes; what the others read is not used)
        const float ex = __shfl(E.x, src), ey = __shfl(E.y, src), ez = __shfl(E.z, src), eo = __shfl(open, src);
        Es = Es + mk3(ex, ey, ez); os += eo;
    }
    if (live && j == 0u)
        store_at<float4>(B.out, 16u * t, 0, make_float4(Es.x * B.inv_spp, Es.y * B.inv_spp, Es.z * B.inv_spp, __fdiv_rn(os, B.spp_f)));
}

template <class A, bool ENV>
static void bake_launch(const DScene &S, const SamplerCfg &C, const BakeArgs &B, int lanes_shift, dim3 grid, size_t dyn, hipStream_t st) {
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_bake_shade<0, A, ENV>), grid, dim3(BAKE_WAVE), dyn, st, S, C, B, lanes_shift);
    else hipLaunchKernelGGL((k_bake_shade<1, A, ENV>), grid, dim3(BAKE_WAVE), dyn, st, S, C, B, lanes_shift);
}

int zdr_launch_texel_lighting(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const BakeArgs &B, hipStream_t st) {
    DScene S = S_in;
    // Lanes per texel: enough lanes for the machine (256 CUs x 4 SIMDs x 4 waves x 64) when the texels alone are too few — a 256^2
    // texture gets 4 — but never more than samples, and a power of two so that a texel's lanes never straddle two waves.
    const uint32_t nsamples = B.sample_end - B.sample_begin, want = (262144u + B.ntexels - 1u) / B.ntexels;
    int lanes_shift = 0;
    while ((2u << lanes_shift) <= std::min<uint32_t>(nsamples, ZDR_BAKE_MAX_LANES) && (1u << lanes_shift) < want) lanes_shift++;
    // dynamic LDS of a wave that traverses the BVH, as zdr_launch_trace sizes it: the first entries of the per-lane stacks (accel.h)
    size_t dyn = 0;
    if (accel_is_bvh) { S.lds_stack = std::min<int>(S.stack_entries, ZDR_BVH_LDS_STACK); dyn = (size_t)S.lds_stack * BAKE_WAVE * sizeof(int); }
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    hipLaunchKernelGGL(k_bake_clear, dim3(1), dim3(64), 0, st, B.count);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_bake_compact, dim3((B.ntexels + 255u) / 256u), dim3(256), 0, st, B);
    if (hipGetLastError() != hipSuccess) return -1;
    const dim3 grid((uint32_t)((((uint64_t)B.ntexels << lanes_shift) + BAKE_WAVE - 1u) / BAKE_WAVE));   // ntexels << shift < 2^27
    const bool env = S.env_count > 0;
    if (accel_is_bvh) { if (env) bake_launch<BvhAccel, true>(S, C, B, lanes_shift, grid, dyn, st); else bake_launch<BvhAccel, false>(S, C, B, lanes_shift, grid, dyn, st); }
    else { if (env) bake_launch<BruteAccel, true>(S, C, B, lanes_shift, grid, dyn, st); else bake_launch<BruteAccel, false>(S, C, B, lanes_shift, grid, dyn, st); }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
