// zdr_bounceenv.hip — the adjoint of the bounced-light baker (zdr_bounce.hip) in the environment map, for gfx950: the gradient of the
// irradiance of zdr_scene_texel_bounce in the map's texels, zdr_scene_texel_bounce_backward_env (include/zdr.h).  With the walks, the
// light list, the sampling tables, visibility and the acceptance bits held fixed the bake is exactly linear in the map, and this is the
// transpose of that sparse map: every accepted light sample that came from the map hands (cotangent x beta_k x weight) to the four
// texels it read.  The device code it calls — A::closest, A::any_shadow, surface_interact, read_bsdf_in, sample_light with its env_uv
// hook, the samplers — is the path kernels' own (scene.h, accel.h, sampler.h).  Linked into libzdr_bounceenv.so (zdr_amd/build.py).
//
// A lean kernel of its own, not a third target of k_bgrad_shade (zdr_bouncegrad.hip): the gradient of vertex k needs the prefix beta_k
// alone, which the walk carries anyway — no vertex records, so no dynamic LDS beyond the traversal stacks, no reverse sweep, no scatter
// queue.
//
// Three kernels, launched one after the other on the caller's stream:
//   k_benv_clear      the workspace's header to 0 (a kernel, not a memset node);
//   k_benv_compact    k_bgrad_compact: k_bounce_compact without its stores to `out`;
//   k_benv_shade      k_bounce_shade's lanes, trips and draws, the walk of bounce_sample statement for statement (phase 1 of
//                     k_bgrad_shade, the explicit-fma interaction included: the replay must decide the forward's acceptance bits).  An
//                     accepted sample of vertex k that came from the map forms term = (d_out x inv_spp x beta_k) x w.  Per vertex index
//                     (wave-uniform) the wave's samples go through the merge of k_lgrad_shade (zdr_bakegrad.hip): the lanes whose
//                     samples fell into the same map cell are summed in LDS first, ZDR_LGRAD_MERGE_ROUNDS cells per vertex index, and
//                     sixteen lanes per cell add the four taps x rgb, two 32-byte row segments; lanes left over add their twelve floats
//                     themselves.
// The sums use float atomics and the list's order varies: the result is not bit-stable from run to run.
#include "accel.h"
#include "bounceenv.h"

#define BENV_WAVE 64

__global__ __launch_bounds__(64) void k_benv_clear(uint32_t *count) {
    if (threadIdx.x < ZDR_BOUNCE_HEADER_BYTES / 4) count[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(256) void k_benv_compact(BenvArgs G) {
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

ZD bool benv_finite(f3 a) { return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff(); }

// the cosine lobe of the forward (bounce_cosine_lobe, zdr_bounce.hip)
ZD f3 benv_cosine_lobe(f2 u) {
    const float r = fsqrt(u.x), phi = 2.0f * ZDR_PI * u.y;
    float sn, cs;
    sincosf(phi, &sn, &cs);
    return mk3(r * cs, r * sn, fsqrt(1.0f - u.x));
}

// bgrad_interact (zdr_bouncegrad.hip), copied: surface_interact (scene.h) with the rounding of zdr_bounce.hip's kernels spelled out —
// fma(c, w2, fma(a, w0, b w1)).  A light sample whose shadow ray leaves its own surface at a grazing angle is decided by the last bit of
// it.p, and an explicit fma is the same in every kernel it is inlined into (tests/test_gpu_texel_bake_edges.py, cbox_wide).
ZD Interaction benv_interact(const DScene &S, const Hit &h) {
    Interaction it = surface_interact(S, h);
    const uint32_t r = 128u * (uint32_t)h.slot;
    const float4 r0 = load_at<float4>(S.shade, r, 0), r1 = load_at<float4>(S.shade, r, 16), r2 = load_at<float4>(S.shade, r, 32),
                 r3 = load_at<float4>(S.shade, r, 48), r4 = load_at<float4>(S.shade, r, 64), r5 = load_at<float4>(S.shade, r, 80);
    const float w0 = 1.0f - h.u - h.v, w1 = h.u, w2 = h.v;
    auto mix = [&](float a, float b, float c) { return __builtin_fmaf(c, w2, __builtin_fmaf(a, w0, b * w1)); };
    it.p = mk3(mix(r0.x, r1.x, r2.x), mix(r0.y, r1.y, r2.y), mix(r0.z, r1.z, r2.z));
    it.uv.x = mix(r0.w, r2.w, r4.w);
    it.uv.y = mix(r1.w, r3.w, r5.w);
    it.ns = normalize(mk3(mix(r3.x, r4.x, r5.x), mix(r3.y, r4.y, r5.y), mix(r3.z, r4.z, r5.z)));
    return it;
}

// The two ray queries of the walk.  BruteAccel: its own.  BvhAccel: the loop of BvhAccel::walk (accel.h) over the same start() and step(),
// one ray per call, with the WHOLE traversal stack in this wave's LDS: LN = S.lds_stack = S.stack_entries, the host's bound on the
// pending entries of this tree plus the four slots a node stores unconditionally, so step() never leaves the LDS part and the kernel
// holds no per-lane overflow array in scratch.  (`deep` must still be an address: it points into the wave's own LDS region.)  The order
// of the visits does not depend on where an entry lives, so the hits are those of BvhAccel::closest and BvhAccel::any_shadow.
template <class A> struct BenvRays {
    ZD static Hit closest(const DScene &S, int *stack, f3 o, f3 d, float tmin, float tmax) { return A::closest(S, stack, o, d, tmin, tmax); }
    ZD static bool any_shadow(const DScene &S, int *stack, f3 o, f3 d, float tmin, float tmax) { return A::any_shadow(S, stack, o, d, tmin, tmax); }
};
template <> struct BenvRays<BvhAccel> {
    template <bool ANY> ZD static BvhAccel::Walker run(const DScene &S, int *stack, f3 o, f3 d, float tmin, float tmax) {
        const int LN = S.lds_stack;
        int *deep = stack + (threadIdx.x & 63u);             // never reached: sp stays below LN
        BvhAccel::Walker w;
        BvhAccel::start(S, w, o, d, tmin, tmax);
        bool active = true;
        int trips_left = BvhAccel::walk_budget(S);           // wave-uniform
        while (__ballot(active) != 0ull) {
            if (--trips_left < 0) { raise_device_error(S, ZDR_DEVERR_BVH_BUDGET); break; }   // the walks were cut short: whatever they return is not a result
            if (active && !BvhAccel::step(S, stack, LN, deep, w, ANY)) active = false;
        }
        return w;
    }
    ZD static Hit closest(const DScene &S, int *stack, f3 o, f3 d, float tmin, float tmax) {
        const BvhAccel::Walker w = run<false>(S, stack, o, d, tmin, tmax);
        Hit hit = w.h;
        if (hit.slot >= 0) hit.slot = BvhAccel::slot_of(S, hit.slot);
        hit_barycentrics(S, hit, o, d);
        return hit;
    }
    ZD static bool any_shadow(const DScene &S, int *stack, f3 o, f3 d, float tmin, float tmax) { return run<true>(S, stack, o, d, tmin, tmax).h.slot >= 0; }
};

// what read_bsdf_in needs of a table entry; chosen per lane from the wave-uniform table (BounceMat of zdr_bounce.hip)
struct BenvMat { int32_t texel, h, w; };

template <int SK, class A>
__global__ __launch_bounds__(BENV_WAVE) void k_benv_shade(DScene S, SamplerCfg C, BenvArgs G, MaterialTable mt, int lanes_shift) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks, all of S.stack_entries (sized at launch); unused otherwise
    __shared__ float slots[16 * ZDR_LGRAD_MERGE_ROUNDS];        // this vertex index's merged cells: [round][tap = 2 dy + dx][rgb, unused]
    __shared__ int slot_key[ZDR_LGRAD_MERGE_ROUNDS];            // their cells (-1: round not used)
    static_assert(16 * ZDR_LGRAD_MERGE_ROUNDS == BENV_WAVE, "one lane per float of the merged cells");
    const uint32_t count = *G.count;
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x * BENV_WAVE + lane;
    if (((blockIdx.x * BENV_WAVE) >> lanes_shift) >= count) return;    // wave-uniform: the whole workgroup lies behind the list's end
    const uint32_t lanes = 1u << lanes_shift, entry = item >> lanes_shift, j = item & (lanes - 1u);
    const bool live = entry < count;
    const uint32_t t = live ? G.list[entry] : 0u;
    f3 n = mk3(0.0f, 0.0f, 1.0f), p = mk3(0.0f), dcot = mk3(0.0f);
    if (live) {
        const uint32_t r = 64u * t;                          // (load_at, scene.h: at most 2^26 texels of 64 bytes)
        n = xyz(load_at<float4>(G.texels, r, 16)); p = xyz(load_at<float4>(G.texels, r, 32));
        dcot = xyz(load_at<float4>(G.d_out, 16u * t, 0)) * G.inv_spp;   // (float 3, the cotangent of `surface`, is not used)
    }
    const uint32_t y = t / (uint32_t)G.tex_w, x = t - y * (uint32_t)G.tex_w;
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4(x, y, C.seed, 0u) : 0u;
    uint32_t n_env = 0u, n_groups = 0u;                      // (wave-uniform counts; lane 0 adds them to the header)
    const uint32_t trips = (G.sample_end - G.sample_begin + lanes - 1u) >> lanes_shift;   // wave-uniform
#pragma unroll 1
    for (uint32_t trip = 0; trip < trips; trip++) {
        const uint32_t s = G.sample_begin + j + (trip << lanes_shift);
        const bool valid = live && s < G.sample_end;
        // a lane without a sample draws all the same, from the range's first sample (k_bounce_shade)
        Sampler smp = sampler_make<SK>(C, x, y, perm_seed, valid ? s : G.sample_begin);
        // the walk of bounce_sample (zdr_bounce.hip), statement for statement; the accumulator is replaced by the scatter into the map
        const f2 u_ao = sampler_next2<SK>(C, smp);
        f3 dir = to_world(make_onb(n), benv_cosine_lobe(u_ao));
        f3 org = p;
        float tmin = 1e-4f;
        f3 beta = mk3(1.0f);
        bool alive = valid;
#pragma unroll 1
        for (int k = 0; k < G.bounces; k++) {                // wave-uniform
            const float u_pick = sampler_next<SK>(C, smp), u_prim = sampler_next<SK>(C, smp);
            const f2 u_pt = sampler_next2<SK>(C, smp);
            alive = alive && !any_nan(dir);
            const Hit h = BenvRays<A>::closest(S, lds, org, alive ? dir : mk3(0.0f, 0.0f, 1.0f), tmin, alive ? 1e30f : -1.0f);
            alive = alive && h.slot >= 0;
            const bool hit = alive;
            Hit hs = h;
            if (!hit) { hs.slot = 0; hs.u = 0.0f; hs.v = 0.0f; }    // (a lane without a hit reads the first record: any valid address)
            const Interaction it = benv_interact(S, hs);
            const bool front = !(dot(-dir, it.ng) < 1e-4f || dot(-dir, it.ns) < 1e-4f);
            int slot = -1;
            if (hit) slot = load_at<int32_t>(mt.inst_slot, 4u * (uint32_t)it.inst);
            const bool shaded = hit && front && slot >= 0;
            BenvMat ms; ms.texel = mt.m[0].texel; ms.h = mt.m[0].h; ms.w = mt.m[0].w;
            for (int jm = 1; jm < mt.nmat; jm++) {           // jm and the entry are wave-uniform
                const bool mine = slot == jm;
                ms.texel = mine ? mt.m[jm].texel : ms.texel; ms.h = mine ? mt.m[jm].h : ms.h; ms.w = mine ? mt.m[jm].w : ms.w;
            }
            f2 muv; muv.x = shaded ? it.uv.x : 0.0f; muv.y = shaded ? it.uv.y : 0.0f;
            const float4 m = read_bsdf_in(G.materials, ms, muv, G.wide_offsets != 0);
            if (shaded) beta = beta * mk3(m.x, m.y, m.z);
            alive = shaded;
            f2 env_uv; env_uv.x = -1.0f; env_uv.y = 0.0f;
            const LightSample L = sample_light<true, true>(S, it.p, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; }, &env_uv, nullptr);
            const float c = dot(it.ns, L.wi);
            const bool lit = alive && c > 0.0f && (L.eval.x > 0.0f || L.eval.y > 0.0f || L.eval.z > 0.0f);
            const bool occ = BenvRays<A>::any_shadow(S, lds, it.p, L.wi, 1e-4f, lit ? L.dist : 0.0f);
            const float ws = c * rcp(fmaxf(L.pdf, 1e-4f));
            const f3 add = (beta * L.eval) * ws;
            const bool added = lit && !occ && benv_finite(add);   // the forward's acceptance bit A_k
            {   // ---- the scatter of vertex k: the merge of k_lgrad_shade (zdr_bakegrad.hip) over the wave's samples of this vertex index
                const f3 term = (dcot * beta) * ws;
                const bool has_env = added && env_uv.x >= 0.0f && benv_finite(term);
                unsigned long long pend = __ballot(has_env);
                if (pend != 0ull) {                          // wave-uniform
                    // the footprint of env_lookup (scene.h): base texel in -1 .. W - 1 (uv lies in [0, 1)), the taps clamped to the edge
                    const float fxp = env_uv.x * (float)S.env_w - 0.5f, fyp = env_uv.y * (float)S.env_h - 0.5f;
                    const float x0f = floorf(fxp), y0f = floorf(fyp), fx = fxp - x0f, fy = fyp - y0f;
                    const int cx = clampi((int)x0f, -1, S.env_w - 1), cy = clampi((int)y0f, -1, S.env_h - 1);
                    const int key = has_env ? (cy + 1) * (S.env_w + 1) + (cx + 1) : -1;
                    slots[lane] = 0.0f;
                    if (lane < ZDR_LGRAD_MERGE_ROUNDS) slot_key[lane] = -1;
                    __syncthreads();                         // (one wave per workgroup)
                    n_env += (uint32_t)__popcll(pend);
                    int round = -1;
#pragma unroll
                    for (int r = 0; r < ZDR_LGRAD_MERGE_ROUNDS; r++) {
                        if (pend == 0ull) break;             // wave-uniform
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
                            for (int mm = 0; mm < 4; mm++)
#pragma unroll
                                for (int ch = 0; ch < 3; ch++) __hip_atomic_fetch_add(sl + 4 * mm + ch, kw[mm] * tc[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        } else {                             // more distinct cells at this vertex index than rounds: lane by lane
#pragma unroll
                            for (int mm = 0; mm < 4; mm++) {
                                const int tx = clampi(cx + (mm & 1), 0, S.env_w - 1), ty = clampi(cy + (mm >> 1), 0, S.env_h - 1);
                                float *d = G.d_env + 4 * ((size_t)ty * (size_t)S.env_w + (size_t)tx);
#pragma unroll
                                for (int ch = 0; ch < 3; ch++) unsafeAtomicAdd(d + ch, kw[mm] * tc[ch]);
                            }
                        }
                    }
                    __syncthreads();
                    {   // lane = (round, tap, channel): the four taps of a merged cell are two segments of 32 bytes, one per map row
                        const int r = (int)(lane >> 4), mm = (int)((lane >> 2) & 3u), ch = (int)(lane & 3u);
                        const int kk = slot_key[r];
                        const float v = slots[lane];
                        if (kk >= 0 && ch < 3 && v != 0.0f) {
                            const int ky = kk / (S.env_w + 1), kx = kk - ky * (S.env_w + 1);
                            const int tx = clampi(kx - 1 + (mm & 1), 0, S.env_w - 1), ty = clampi(ky - 1 + (mm >> 1), 0, S.env_h - 1);
                            unsafeAtomicAdd(G.d_env + 4 * ((size_t)ty * (size_t)S.env_w + (size_t)tx) + ch, v);
                        }
                    }
                    __syncthreads();                         // (the next vertex index clears the slots)
                }
            }
            // the next segment: a cosine lobe about the shading normal
            bool on = false;
            f3 nd = dir;
            if (k + 1 < G.bounces) {                         // wave-uniform: the last vertex draws neither u_lobe nor u_dir
                (void)sampler_next<SK>(C, smp);              // u_lobe: drawn and ignored
                const f2 u_dir = sampler_next2<SK>(C, smp);
                const f3 wl = benv_cosine_lobe(u_dir);
                nd = to_world(make_onb(it.ns), wl);
                on = alive && !(dot(nd, it.ng) < 1e-4f || wl.z < 1e-4f);
            }
            alive = on;
            dir = nd; org = offset_ray_origin(it.p, it.ng); tmin = 0.0f;
        }
    }
    if (lane == 0u && n_env != 0u) { atomicAdd(G.count + 1, n_env); atomicAdd(G.count + 2, n_groups); }
}

template <class A>
static void benv_launch(const DScene &S, const SamplerCfg &C, const BenvArgs &G, const MaterialTable &mt, int lanes_shift, dim3 grid, size_t dyn, hipStream_t st) {
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_benv_shade<0, A>), grid, dim3(BENV_WAVE), dyn, st, S, C, G, mt, lanes_shift);
    else hipLaunchKernelGGL((k_benv_shade<1, A>), grid, dim3(BENV_WAVE), dyn, st, S, C, G, mt, lanes_shift);
}

int zdr_launch_texel_bounce_backward_env(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const BenvArgs &G, const MaterialTable &mt, hipStream_t st) {
    DScene S = S_in;
    if (S.env_count <= 0 || !G.d_env) return 256 * 3 + (int)hipErrorInvalidValue;   // (a scene without a map never gets here)
    if (G.bounces < 1 || G.bounces > ZDR_BOUNCE_MAX_BOUNCES) return 256 * 3 + (int)hipErrorInvalidValue;
    const int lanes_shift = zdr_bounce_lanes_shift(G.ntexels, G.sample_end - G.sample_begin);   // the forward's rule
    size_t dyn = 0;                                          // the traversal stacks, whole (BenvRays), and nothing else: at most 64 entries x 256 bytes
    if (accel_is_bvh) {
        if (S.stack_entries < 1 || S.stack_entries > ZDR_BVH_STACK) return 256 * 3 + (int)hipErrorInvalidValue;
        S.lds_stack = S.stack_entries; dyn = (size_t)S.lds_stack * BENV_WAVE * sizeof(int);
    }
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    hipError_t e;
    hipLaunchKernelGGL(k_benv_clear, dim3(1), dim3(64), 0, st, G.count);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 1 + (int)e;
    hipLaunchKernelGGL(k_benv_compact, dim3((G.ntexels + 255u) / 256u), dim3(256), 0, st, G);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 2 + (int)e;
    const dim3 grid((uint32_t)((((uint64_t)G.ntexels << lanes_shift) + BENV_WAVE - 1u) / BENV_WAVE));   // (zdr_launch_texel_bounce: within 32 bits)
    if (accel_is_bvh) benv_launch<BvhAccel>(S, C, G, mt, lanes_shift, grid, dyn, st);
    else benv_launch<BruteAccel>(S, C, G, mt, lanes_shift, grid, dyn, st);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 3 + (int)e;
    return 0;
}
