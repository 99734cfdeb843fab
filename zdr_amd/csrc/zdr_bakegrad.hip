// zdr_bakegrad.hip — the adjoint of the texture-space light baker (zdr_bake.hip) for gfx950: the gradient of the irradiance of
// zdr_scene_texel_lighting in the lights' emissions and in the environment map, zdr_scene_texel_lighting_backward (include/zdr.h).  With
// the light list, the sampling tables and visibility held fixed the forward is linear in both, and this is the transpose of that sparse
// map: every accepted sample hands (cotangent x weight) to the one light or to the four map texels it read.  The device code it calls —
// sample_light with its env_uv and mesh_light hooks, the samplers, the per-lane any-hit walks — is the path kernels' own (scene.h, accel.h,
// sampler.h).  Linked into libzdr_bakegrad.so (zdr_amd/build.py).
//
// Four kernels, launched one after the other on the caller's stream:
//   k_lgrad_clear     the workspace's header and the emission accumulator to 0;
//   k_lgrad_compact   k_bake_compact without its stores to `out`: an adjoint writes nothing for a texel that is not shaded;
//   k_lgrad_shade     k_bake_shade's lanes, trips and draws (lanes_shift, the same four draws in the same order, the same sample_light),
//                     the shadow walk alone — the openness ray is not traced.  An accepted sample forms term = (d_out x inv_spp) x w.
//                     Mesh light: the wave sums per light in an LDS table of ZDR_LGRAD_LDS_LIGHTS x 3 floats and writes the table out
//                     once, into row blockIdx % ZDR_LGRAD_COPIES of the accumulator (a light beyond the table adds into that row with
//                     global atomics).  Environment map: the lanes of a wave whose samples fell into the same map cell — importance
//                     sampling sends most of them to a handful — are summed in LDS first, ZDR_LGRAD_MERGE_ROUNDS cells per trip, and
//                     sixteen lanes per cell add the four taps x rgb, two 32-byte row segments; lanes left over add their twelve floats
//                     themselves;
//   k_lgrad_gather    the accumulator's rows summed in float64, light l's three floats added into the row of its instance.
// The sums use float atomics and the list's order varies: the result is not bit-stable from run to run.
#include "accel.h"
#include "bakegrad.h"
#include <algorithm>

#define LGRAD_WAVE 64

__global__ __launch_bounds__(256) void k_lgrad_clear(uint32_t *count, float *acc, uint32_t nacc) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < ZDR_BAKE_HEADER_BYTES / 4) count[i] = 0u;
    if (i < nacc) acc[i] = 0.0f;
}

__global__ __launch_bounds__(256) void k_lgrad_compact(LgradArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    bool shade = false;
    if (t < G.ntexels) {
        const float4 *r = G.texels + 4 * (size_t)t;
        const float4 nrm = r[1], pos = r[2];
        const float reach = r[3].x;
        shade = (reach == 1.0f) && !any_nan(xyz(nrm)) && !any_nan(xyz(pos));
    }
    const unsigned long long m = __ballot(shade);
    if (m == 0ull) return;                                   // wave-uniform
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0u;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(G.count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader);
    if (shade) {
        const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        G.list[at] = t;                                      // (at < ntexels: every texel is appended at most once)
    }
}

ZD bool lgrad_finite(f3 a) { return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff(); }

template <int SK, class A, bool ENV>
__global__ __launch_bounds__(LGRAD_WAVE) void k_lgrad_shade(DScene S, SamplerCfg C, LgradArgs G, int lanes_shift) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks (sized at launch); unused otherwise
    __shared__ float emit_tab[3 * ZDR_LGRAD_LDS_LIGHTS];        // this wave's sums per light
    __shared__ float slots[16 * ZDR_LGRAD_MERGE_ROUNDS];        // this trip's merged cells: [round][tap = 2 dy + dx][rgb, unused]
    __shared__ int slot_key[ZDR_LGRAD_MERGE_ROUNDS];            // their cells (-1: round not used)
    static_assert(16 * ZDR_LGRAD_MERGE_ROUNDS == LGRAD_WAVE, "one lane per float of the merged cells");
    const uint32_t count = *G.count;
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x * LGRAD_WAVE + lane;
    if (((blockIdx.x * LGRAD_WAVE) >> lanes_shift) >= count) return;    // wave-uniform: the whole workgroup lies behind the list's end
    const bool want_emit = G.acc != nullptr, want_env = ENV && G.d_env != nullptr;   // wave-uniform
    if (want_emit) {
        for (uint32_t i = lane; i < 3 * ZDR_LGRAD_LDS_LIGHTS; i += LGRAD_WAVE) emit_tab[i] = 0.0f;
        __syncthreads();                                     // (one wave per workgroup)
    }
    float *const row = want_emit ? G.acc + (size_t)(blockIdx.x % (unsigned)ZDR_LGRAD_COPIES) * (size_t)(3 * S.light_count) : nullptr;
    const uint32_t lanes = 1u << lanes_shift, entry = item >> lanes_shift, j = item & (lanes - 1u);
    const bool live = entry < count;
    const uint32_t t = live ? G.list[entry] : 0u;
    f3 n = mk3(0.0f, 0.0f, 1.0f), p = mk3(0.0f), dcot = mk3(0.0f);
    if (live) {
        const uint32_t r = 64u * t;                          // (load_at, scene.h: at most 2^26 texels of 64 bytes)
        n = xyz(load_at<float4>(G.texels, r, 16)); p = xyz(load_at<float4>(G.texels, r, 32));
        dcot = xyz(load_at<float4>(G.d_out, 16u * t, 0)) * G.inv_spp;   // (float 3, the openness' cotangent, is not used)
    }
    const uint32_t y = t / (uint32_t)G.tex_w, x = t - y * (uint32_t)G.tex_w;
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4(x, y, C.seed, 0u) : 0u;
    uint32_t n_env = 0u, n_groups = 0u;                      // (wave-uniform counts; lane 0 adds them to the header)
    const uint32_t trips = (G.sample_end - G.sample_begin + lanes - 1u) >> lanes_shift;   // wave-uniform
#pragma unroll 1
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t s = G.sample_begin + j + (k << lanes_shift);
        const bool valid = live && s < G.sample_end;
        Sampler smp = sampler_make<SK>(C, x, y, perm_seed, valid ? s : G.sample_begin);   // (as k_bake_shade: a lane without a sample draws all the same)
        (void)sampler_next2<SK>(C, smp);                     // u_ao: drawn, as the forward draws it; the openness has no gradient
        const float u_pick = sampler_next<SK>(C, smp), u_prim = sampler_next<SK>(C, smp);
        const f2 u_pt = sampler_next2<SK>(C, smp);
        f2 env_uv; env_uv.x = -1.0f; env_uv.y = 0.0f;
        int mesh_light = -1;
        const LightSample L = sample_light<ENV, true>(S, p, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; }, &env_uv, &mesh_light);
        const float c = dot(n, L.wi);
        const bool lit = valid && c > 0.0f && (L.eval.x > 0.0f || L.eval.y > 0.0f || L.eval.z > 0.0f);
        const bool occ = A::any_shadow(S, lds, p, L.wi, 1e-4f, lit ? L.dist : 0.0f);
        const float w = c * rcp(fmaxf(L.pdf, 1e-4f));
        const bool accepted = lit && !occ && lgrad_finite(L.eval * w);
        const f3 term = dcot * w;
        if (want_emit && accepted && mesh_light >= 0 && mesh_light < S.light_count) {
            if (mesh_light < ZDR_LGRAD_LDS_LIGHTS) {
                float *e = emit_tab + 3 * mesh_light;
                __hip_atomic_fetch_add(e, term.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(e + 1, term.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                __hip_atomic_fetch_add(e + 2, term.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            } else {
                float *e = row + 3 * (size_t)mesh_light;
                unsafeAtomicAdd(e, term.x); unsafeAtomicAdd(e + 1, term.y); unsafeAtomicAdd(e + 2, term.z);
            }
        }
        if constexpr (ENV) {
            const bool has_env = want_env && accepted && env_uv.x >= 0.0f;
            unsigned long long pend = __ballot(has_env);
            if (pend != 0ull) {                              // wave-uniform
                // the footprint of env_lookup (scene.h): base texel in -1 .. W - 1 (uv lies in [0, 1)), the taps clamped to the edge
                const float fxp = env_uv.x * (float)S.env_w - 0.5f, fyp = env_uv.y * (float)S.env_h - 0.5f;
                const float x0f = floorf(fxp), y0f = floorf(fyp), fx = fxp - x0f, fy = fyp - y0f;
                const int cx = clampi((int)x0f, -1, S.env_w - 1), cy = clampi((int)y0f, -1, S.env_h - 1);
                const int key = has_env ? (cy + 1) * (S.env_w + 1) + (cx + 1) : -1;
                slots[lane] = 0.0f;
                if (lane < ZDR_LGRAD_MERGE_ROUNDS) slot_key[lane] = -1;
                __syncthreads();
                n_env += (uint32_t)__popcll(pend);
                int round = -1;
#pragma unroll
                for (int r = 0; r < ZDR_LGRAD_MERGE_ROUNDS; r++) {
                    if (pend == 0ull) break;                 // wave-uniform
                    const int lead = __ffsll((long long)pend) - 1;
                    const int kk = __shfl(key, lead);
                    const bool mine = has_env && round < 0 && key == kk;
                    if (mine) round = r;
                    if ((int)lane == lead) slot_key[r] = kk;
                    pend &= ~__ballot(mine);
                    n_groups++;
                }
                n_groups += (uint32_t)__popcll(pend);
                if (has_env) {
                    const float kw[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
                    const float tc[3] = {term.x, term.y, term.z};
                    if (round >= 0) {
                        float *sl = slots + 16 * round;
#pragma unroll
                        for (int m = 0; m < 4; m++)
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) __hip_atomic_fetch_add(sl + 4 * m + ch, kw[m] * tc[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    } else {                                 // more distinct cells in this trip than rounds: lane by lane
#pragma unroll
                        for (int m = 0; m < 4; m++) {
                            const int tx = clampi(cx + (m & 1), 0, S.env_w - 1), ty = clampi(cy + (m >> 1), 0, S.env_h - 1);
                            float *d = G.d_env + 4 * ((size_t)ty * (size_t)S.env_w + (size_t)tx);
#pragma unroll
                            for (int ch = 0; ch < 3; ch++) unsafeAtomicAdd(d + ch, kw[m] * tc[ch]);
                        }
                    }
                }
                __syncthreads();
                {   // lane = (round, tap, channel): the four taps of a merged cell are two segments of 32 bytes, one per map row
                    const int r = (int)(lane >> 4), m = (int)((lane >> 2) & 3u), ch = (int)(lane & 3u);
                    const int kk = slot_key[r];
                    const float v = slots[lane];
                    if (kk >= 0 && ch < 3 && v != 0.0f) {
                        const int ky = kk / (S.env_w + 1), kx = kk - ky * (S.env_w + 1);
                        const int tx = clampi(kx - 1 + (m & 1), 0, S.env_w - 1), ty = clampi(ky - 1 + (m >> 1), 0, S.env_h - 1);
                        unsafeAtomicAdd(G.d_env + 4 * ((size_t)ty * (size_t)S.env_w + (size_t)tx) + ch, v);
                    }
                }
                __syncthreads();                             // (the next trip clears the slots)
            }
        }
    }
    if (want_emit) {
        __syncthreads();
        const uint32_t nt = 3u * (uint32_t)(S.light_count < ZDR_LGRAD_LDS_LIGHTS ? S.light_count : ZDR_LGRAD_LDS_LIGHTS);
        for (uint32_t i = lane; i < nt; i += LGRAD_WAVE) {
            const float v = emit_tab[i];
            if (v != 0.0f) unsafeAtomicAdd(row + i, v);
        }
    }
    if (lane == 0u && n_env != 0u) { atomicAdd(G.count + 1, n_env); atomicAdd(G.count + 2, n_groups); }
}

// sums the accumulator's rows in float64 and adds light l's three floats into the row of its instance in d_emission (+=)
__global__ __launch_bounds__(64) void k_lgrad_gather(const float *__restrict__ acc, int copies, int light_count, const int32_t *__restrict__ light_insts, float *__restrict__ d_emission) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 3 * light_count) return;
    double sum = 0.0;
    for (int k = 0; k < copies; k++) sum += (double)acc[(size_t)k * (size_t)(3 * light_count) + i];
    d_emission[3 * (size_t)light_insts[i / 3] + (i % 3)] += (float)sum;
}

template <class A, bool ENV>
static void lgrad_launch(const DScene &S, const SamplerCfg &C, const LgradArgs &G, int lanes_shift, dim3 grid, size_t dyn, hipStream_t st) {
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_lgrad_shade<0, A, ENV>), grid, dim3(LGRAD_WAVE), dyn, st, S, C, G, lanes_shift);
    else hipLaunchKernelGGL((k_lgrad_shade<1, A, ENV>), grid, dim3(LGRAD_WAVE), dyn, st, S, C, G, lanes_shift);
}

int zdr_launch_texel_lighting_backward(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const LgradArgs &G, hipStream_t st) {
    DScene S = S_in;
    // lanes per texel and the dynamic LDS: as zdr_launch_texel_lighting (zdr_bake.hip) derives them, from the same arguments
    const uint32_t nsamples = G.sample_end - G.sample_begin, want = (262144u + G.ntexels - 1u) / G.ntexels;
    int lanes_shift = 0;
    while ((2u << lanes_shift) <= std::min<uint32_t>(nsamples, ZDR_BAKE_MAX_LANES) && (1u << lanes_shift) < want) lanes_shift++;
    size_t dyn = 0;
    if (accel_is_bvh) { S.lds_stack = std::min<int>(S.stack_entries, ZDR_BVH_LDS_STACK); dyn = (size_t)S.lds_stack * LGRAD_WAVE * sizeof(int); }
    const uint32_t nacc = G.acc ? (uint32_t)ZDR_LGRAD_COPIES * 3u * (uint32_t)S.light_count : 0u;
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    // (the value returned names the launch and the error: 256 x launch + hipError_t)
    hipError_t e;
    hipLaunchKernelGGL(k_lgrad_clear, dim3((std::max<uint32_t>(nacc, ZDR_BAKE_HEADER_BYTES / 4) + 255u) / 256u), dim3(256), 0, st, G.count, G.acc, nacc);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 1 + (int)e;
    hipLaunchKernelGGL(k_lgrad_compact, dim3((G.ntexels + 255u) / 256u), dim3(256), 0, st, G);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 2 + (int)e;
    const dim3 grid((uint32_t)((((uint64_t)G.ntexels << lanes_shift) + LGRAD_WAVE - 1u) / LGRAD_WAVE));   // ntexels << shift < 2^27
    const bool env = S.env_count > 0;
    if (accel_is_bvh) { if (env) lgrad_launch<BvhAccel, true>(S, C, G, lanes_shift, grid, dyn, st); else lgrad_launch<BvhAccel, false>(S, C, G, lanes_shift, grid, dyn, st); }
    else { if (env) lgrad_launch<BruteAccel, true>(S, C, G, lanes_shift, grid, dyn, st); else lgrad_launch<BruteAccel, false>(S, C, G, lanes_shift, grid, dyn, st); }
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 3 + (int)e;
    if (G.acc) {
        hipLaunchKernelGGL(k_lgrad_gather, dim3((3 * S.light_count + 63) / 64), dim3(64), 0, st, (const float *)G.acc, ZDR_LGRAD_COPIES, S.light_count, S.light_insts, G.d_emission);
        if ((e = hipGetLastError()) != hipSuccess) return 256 * 4 + (int)e;
    }
    return 0;
}
