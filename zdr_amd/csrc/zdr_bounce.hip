// zdr_bounce.hip — the bounced-light baker of include/zdr.h (zdr_scene_texel_bounce) for gfx950: per texel, the irradiance that arrives
// after 1 .. K Lambertian bounces and the share of the hemisphere that can bounce light at all.  A random walk that starts at the texels:
// everything it calls — A::closest, A::any_shadow, surface_interact, read_bsdf_in, sample_light, make_onb, offset_ray_origin, the
// samplers — is the path kernels' own device code (scene.h, accel.h, sampler.h), instantiated here once more.  Linked into
// libzdr_bounce.so (zdr_amd/build.py).
//
// Three kernels, launched one after the other on the caller's stream, and a fourth for the tests:
//   k_bounce_clear    the list's counter to 0;
//   k_bounce_compact  thread = texel: a texel with reach == 1 and no NaN in its normal or position is appended to the list in the
//                     workspace — ONE returning integer atomic per workgroup: the waves leave their counts in LDS, thread 0 reserves
//                     the workgroup's range, every wave finds its base from the counts before it —; any other texel gets its four
//                     zeros here.  The order of the list varies from run to run; no result depends on it;
//   k_bounce_shade    k_bake_shade's lanes and trips (zdr_bake.hip): one wave per workgroup, 2^lanes_shift neighbouring lanes share a
//                     texel, lane j takes the samples begin + j, begin + j + lanes, ... and adds every accepted contribution into one
//                     accumulator, samples ascending and vertices ascending within a sample; lane 0 then adds the lanes' sums in lane
//                     order and writes the texel.  No float atomic, and the walks are per lane: a texel's bits depend on its own
//                     samples and on lanes_shift only;
//   k_bounce_dump     lane = one queried (x, y, s): the same walk with a recorder that writes every vertex (zdr_texel_bounce_dump).
// The walk of one sample is ONE device function, bounce_sample, which both kernels call; it takes a recorder, and the production kernel's
// recorder does nothing.  Its loop is wave-uniform — K trips, every lane of the wave enters both walks of every trip — and a lane
// whose walk has ended, or that has no sample, hands in an empty interval (tmax below tmin), which ends its walk at the root: the slab
// test of BvhAccel (tn <= tf with tf <= tmax) and the range test of every triangle fail for it, as they do for A::any.
#include "accel.h"
#include "bounce.h"

#define BOUNCE_WAVE 64
// k_bounce_compact: threads per workgroup, its waves, and the words of dynamic LDS the launcher hands it — one count per wave and the
// workgroup's base.  (Dynamic, not static: no kernel of this library holds static LDS, tests/test_bounce_resources.py.)
#define BOUNCE_COMPACT_THREADS 256
#define BOUNCE_COMPACT_WAVES (BOUNCE_COMPACT_THREADS / BOUNCE_WAVE)
#define BOUNCE_COMPACT_LDS_WORDS (BOUNCE_COMPACT_WAVES + 1)
static_assert(BOUNCE_COMPACT_THREADS % BOUNCE_WAVE == 0, "k_bounce_compact counts whole waves");

__global__ __launch_bounds__(64) void k_bounce_clear(uint32_t *count) {
    if (threadIdx.x < ZDR_BOUNCE_HEADER_BYTES / 4) count[threadIdx.x] = 0u;
}

__global__ __launch_bounds__(BOUNCE_COMPACT_THREADS) void k_bounce_compact(BounceArgs B) {
    extern __shared__ uint32_t wave_count[];                 // [0, WAVES) the waves' counts, [WAVES] the workgroup's base: BOUNCE_COMPACT_LDS_WORDS words
    const uint32_t t = blockIdx.x * BOUNCE_COMPACT_THREADS + threadIdx.x;
    bool shade = false;
    if (t < B.ntexels) {
        const float4 *r = B.texels + 4 * (size_t)t;
        const float4 nrm = r[1], pos = r[2];
        const float reach = r[3].x;
        shade = (reach == 1.0f) && !any_nan(xyz(nrm)) && !any_nan(xyz(pos));
        if (!shade) B.out[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const unsigned long long m = __ballot(shade);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) wave_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (int w = 0; w < BOUNCE_COMPACT_WAVES; w++) total += wave_count[w];
        wave_count[BOUNCE_COMPACT_WAVES] = total ? atomicAdd(B.count, total) : 0u;
    }
    __syncthreads();
    if (shade) {
        uint32_t base = wave_count[BOUNCE_COMPACT_WAVES];
        for (uint32_t w = 0; w < wave; w++) base += wave_count[w];
        const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        B.list[at] = t;                                      // (at < ntexels: every texel is appended at most once)
    }
}

ZD bool bounce_finite(f3 a) { return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff(); }

// the cosine lobe of ggx_sample (microfacet.h), as the openness ray of k_bake_shade forms it
ZD f3 bounce_cosine_lobe(f2 u) {
    const float r = fsqrt(u.x), phi = 2.0f * ZDR_PI * u.y;
    float sn, cs;
    sincosf(phi, &sn, &cs);
    return mk3(r * cs, r * sn, fsqrt(1.0f - u.x));
}

// what read_bsdf_in needs of a table entry; chosen per lane from the wave-uniform table (scalar loads, no indexed copy of the table)
struct BounceMat { int32_t texel, h, w; };

#define BOUNCE_F_SHADED 1u        // the vertex lies on the front of a model with a material
#define BOUNCE_F_LIT 2u           // its light sample faces the surface and carries light
#define BOUNCE_F_FREE 4u          // the shadow segment is free
#define BOUNCE_F_ADDED 8u         // `add` was accepted
#define BOUNCE_F_ON 16u           // the walk goes on to the next vertex

struct BounceNoRecord {
    ZD void vertex(const DScene &, int, bool, const Interaction &, const Hit &, uint32_t, f3, f3) {}
};

// The walk of one sample (include/zdr.h, zdr_scene_texel_bounce).  `valid`: the lane has a sample at all.  E: the lane's accumulator;
// surface: its count of first segments that landed on the front of a model with a material.
template <int SK, class A, bool ENV, class REC>
ZD void bounce_sample(const DScene &S, const SamplerCfg &C, int *lds, const BounceArgs &B, const MaterialTable &mt, const bool valid,
                      const f3 p, const f3 n, Sampler &smp, f3 &E, float &surface, REC &rec) {
    const f2 u_ao = sampler_next2<SK>(C, smp);
    f3 dir = to_world(make_onb(n), bounce_cosine_lobe(u_ao));
    f3 org = p;
    float tmin = 1e-4f;                                      // the first segment is the openness ray; later ones leave an offset origin at 0
    f3 beta = mk3(1.0f);
    bool alive = valid;
#pragma unroll 1
    for (int k = 0; k < B.bounces; k++) {                    // wave-uniform
        const float u_pick = sampler_next<SK>(C, smp), u_prim = sampler_next<SK>(C, smp);
        const f2 u_pt = sampler_next2<SK>(C, smp);
        alive = alive && !any_nan(dir);
        const Hit h = A::closest(S, lds, org, alive ? dir : mk3(0.0f, 0.0f, 1.0f), tmin, alive ? 1e30f : -1.0f);
        alive = alive && h.slot >= 0;
        const bool hit = alive;
        Hit hs = h;
        if (!hit) { hs.slot = 0; hs.u = 0.0f; hs.v = 0.0f; }    // (a lane without a hit reads the first record: any valid address)
        const Interaction it = surface_interact(S, hs);
        const bool front = !(dot(-dir, it.ng) < 1e-4f || dot(-dir, it.ns) < 1e-4f);
        int slot = -1;
        if (hit) slot = load_at<int32_t>(mt.inst_slot, 4u * (uint32_t)it.inst);
        const bool shaded = hit && front && slot >= 0;
        if (k == 0 && shaded) surface += 1.0f;
        BounceMat ms; ms.texel = mt.m[0].texel; ms.h = mt.m[0].h; ms.w = mt.m[0].w;
        for (int j = 1; j < mt.nmat; j++) {                  // j and the entry are wave-uniform
            const bool mine = slot == j;
            ms.texel = mine ? mt.m[j].texel : ms.texel; ms.h = mine ? mt.m[j].h : ms.h; ms.w = mine ? mt.m[j].w : ms.w;
        }
        f2 muv; muv.x = shaded ? it.uv.x : 0.0f; muv.y = shaded ? it.uv.y : 0.0f;
        const float4 m = read_bsdf_in(B.materials, ms, muv, B.wide_offsets != 0);
        if (shaded) beta = beta * mk3(m.x, m.y, m.z);
        alive = shaded;
        // one light sample: the ray and the clamp of direct_sample (integrators.h)
        const LightSample L = sample_light<ENV>(S, it.p, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; });
        const float c = dot(it.ns, L.wi);
        const bool lit = alive && c > 0.0f && (L.eval.x > 0.0f || L.eval.y > 0.0f || L.eval.z > 0.0f);
        const bool occ = A::any_shadow(S, lds, it.p, L.wi, 1e-4f, lit ? L.dist : 0.0f);
        f3 add = (beta * L.eval) * (c * rcp(fmaxf(L.pdf, 1e-4f)));
        const bool added = lit && !occ && bounce_finite(add);
        if (!added) add = mk3(0.0f);
        asm volatile("" : "+v"(add.x), "+v"(add.y), "+v"(add.z));   // rounded as a product: the sum below never contracts with it, whatever this is inlined into
        if (added) E = E + add;
        // the next segment: a cosine lobe about the shading normal
        bool on = false;
        f3 nd = dir;
        if (k + 1 < B.bounces) {                             // wave-uniform: the last vertex draws neither u_lobe nor u_dir
            (void)sampler_next<SK>(C, smp);                  // u_lobe: drawn and ignored
            const f2 u_dir = sampler_next2<SK>(C, smp);
            const f3 wl = bounce_cosine_lobe(u_dir);
            nd = to_world(make_onb(it.ns), wl);
            on = alive && !(dot(nd, it.ng) < 1e-4f || wl.z < 1e-4f);
        }
        rec.vertex(S, k, hit, it, h, (shaded ? BOUNCE_F_SHADED : 0u) | (lit ? BOUNCE_F_LIT : 0u) | ((lit && !occ) ? BOUNCE_F_FREE : 0u) |
                                      (added ? BOUNCE_F_ADDED : 0u) | (on ? BOUNCE_F_ON : 0u), beta, add);
        alive = on;
        dir = nd; org = offset_ray_origin(it.p, it.ng); tmin = 0.0f;
    }
}

template <int SK, class A, bool ENV>
__global__ __launch_bounds__(BOUNCE_WAVE) void k_bounce_shade(DScene S, SamplerCfg C, BounceArgs B, MaterialTable mt, int lanes_shift) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks (sized at launch); unused otherwise
    const uint32_t count = *B.count;
    const uint32_t item = blockIdx.x * BOUNCE_WAVE + threadIdx.x;
    if (((blockIdx.x * BOUNCE_WAVE) >> lanes_shift) >= count) return;   // wave-uniform: the whole workgroup lies behind the list's end
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
    f3 E = mk3(0.0f);
    float surface = 0.0f;
    BounceNoRecord rec;
    const uint32_t trips = (B.sample_end - B.sample_begin + lanes - 1u) >> lanes_shift;   // wave-uniform
#pragma unroll 1
    for (uint32_t k = 0; k < trips; k++) {
        const uint32_t s = B.sample_begin + j + (k << lanes_shift);
        const bool valid = live && s < B.sample_end;
        // a lane without a sample draws all the same, from the range's first sample (k_bake_shade: the pmj02bn tables end at spp)
        Sampler smp = sampler_make<SK>(C, x, y, perm_seed, valid ? s : B.sample_begin);
        bounce_sample<SK, A, ENV>(S, C, lds, B, mt, valid, p, n, smp, E, surface, rec);
    }
    // the lanes of a texel, in lane order (every lane of the wave is here: the exit above is wave-uniform)
    f3 Es = E;
    float ss = surface;
    const int self = (int)(threadIdx.x & 63u);
    for (uint32_t k = 1; k < lanes; k++) {                   // wave-uniform
        const int src = (self + (int)k) & 63;                // (lane 0 of a texel reads its own lanes; what the others read is not used)
        const float ex = __shfl(E.x, src), ey = __shfl(E.y, src), ez = __shfl(E.z, src), es = __shfl(surface, src);
        Es = Es + mk3(ex, ey, ez); ss += es;
    }
    if (live && j == 0u)
        store_at<float4>(B.out, 16u * t, 0, make_float4(Es.x * B.inv_spp, Es.y * B.inv_spp, Es.z * B.inv_spp, __fdiv_rn(ss, B.spp_f)));
}

// The dump's recorder: vertex k of the lane's row, {bits(inst), bits(prim), u, v, bits(flags), beta.rgb, add.rgb, 0} — instance, input
// triangle and the barycentrics of the INPUT corners 1 and 2, as k_trace reports a hit (zdr_kernels.hip).
struct BounceRecord {
    float *row; int nvert;
    ZD void vertex(const DScene &S, int k, bool hit, const Interaction &it, const Hit &h, uint32_t flags, f3 beta, f3 add) {
        if (!hit) return;
        const float4 r7 = S.shade[8 * (size_t)h.slot + 7];
        const int ro = __float_as_int(r7.z);
        const float hw = 1.0f - h.u - h.v;
        float hu = h.u, hv = h.v;
        if (ro == 1) { hu = hw; hv = h.u; } else if (ro == 2) { hu = h.v; hv = hw; }
        float4 *o = (float4 *)(row + 4 + 12 * k);
        o[0] = make_float4(__int_as_float(it.inst), r7.y, hu, hv);
        o[1] = make_float4(__uint_as_float(flags), beta.x, beta.y, beta.z);
        o[2] = make_float4(add.x, add.y, add.z, 0.0f);
        nvert = k + 1;
    }
};

template <int SK, class A, bool ENV>
__global__ __launch_bounds__(BOUNCE_WAVE) void k_bounce_dump(DScene S, SamplerCfg C, BounceArgs B, MaterialTable mt, const int32_t *queries, uint32_t nq, float *out) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    const uint32_t i = blockIdx.x * BOUNCE_WAVE + threadIdx.x;
    const bool have = i < nq;
    const uint32_t tex_h = B.ntexels / (uint32_t)B.tex_w;
    uint32_t x = 0u, y = 0u, s = B.sample_begin;
    bool valid = false;
    if (have) {
        const int32_t qx = queries[3 * (size_t)i], qy = queries[3 * (size_t)i + 1], qs = queries[3 * (size_t)i + 2];
        valid = qx >= 0 && qx < B.tex_w && qy >= 0 && (uint32_t)qy < tex_h && qs >= 0 && (uint32_t)qs >= B.sample_begin && (uint32_t)qs < B.sample_end;
        if (valid) { x = (uint32_t)qx; y = (uint32_t)qy; s = (uint32_t)qs; }
    }
    const uint32_t t = y * (uint32_t)B.tex_w + x;
    f3 n = mk3(0.0f, 0.0f, 1.0f), p = mk3(0.0f);
    if (valid) {
        const float4 *r = B.texels + 4 * (size_t)t;
        const float4 nrm = r[1], pos = r[2];
        valid = (r[3].x == 1.0f) && !any_nan(xyz(nrm)) && !any_nan(xyz(pos));   // the compaction's rule
        if (valid) { n = xyz(nrm); p = xyz(pos); }
    }
    const int stride = 4 + 12 * B.bounces;
    BounceRecord rec; rec.row = out + (size_t)stride * (have ? i : 0u); rec.nvert = 0;
    if (have) for (int k = 0; k < stride; k++) rec.row[k] = 0.0f;
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4(x, y, C.seed, 0u) : 0u;
    Sampler smp = sampler_make<SK>(C, x, y, perm_seed, s);
    f3 E = mk3(0.0f);
    float surface = 0.0f;
    bounce_sample<SK, A, ENV>(S, C, lds, B, mt, valid, p, n, smp, E, surface, rec);
    if (have) { rec.row[0] = __int_as_float(rec.nvert); rec.row[1] = surface; }
}

// dynamic LDS of a wave that traverses the BVH, as zdr_launch_texel_lighting sizes it: the first entries of the per-lane stacks (accel.h)
static size_t bounce_dyn_lds(DScene &S, int accel_is_bvh) {
    if (!accel_is_bvh) return 0;
    S.lds_stack = S.stack_entries < ZDR_BVH_LDS_STACK ? S.stack_entries : ZDR_BVH_LDS_STACK;
    return (size_t)S.lds_stack * BOUNCE_WAVE * sizeof(int);
}

template <class A, bool ENV>
static void bounce_launch(const DScene &S, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt, int lanes_shift, dim3 grid, size_t dyn, hipStream_t st) {
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_bounce_shade<0, A, ENV>), grid, dim3(BOUNCE_WAVE), dyn, st, S, C, B, mt, lanes_shift);
    else hipLaunchKernelGGL((k_bounce_shade<1, A, ENV>), grid, dim3(BOUNCE_WAVE), dyn, st, S, C, B, mt, lanes_shift);
}

int zdr_launch_texel_bounce(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt, hipStream_t st) {
    DScene S = S_in;
    const int lanes_shift = zdr_bounce_lanes_shift(B.ntexels, B.sample_end - B.sample_begin);
    const size_t dyn = bounce_dyn_lds(S, accel_is_bvh);
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    hipLaunchKernelGGL(k_bounce_clear, dim3(1), dim3(64), 0, st, B.count);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_bounce_compact, dim3((B.ntexels + BOUNCE_COMPACT_THREADS - 1u) / BOUNCE_COMPACT_THREADS), dim3(BOUNCE_COMPACT_THREADS),
                       BOUNCE_COMPACT_LDS_WORDS * sizeof(uint32_t), st, B);
    if (hipGetLastError() != hipSuccess) return -1;
    // Items = ntexels << lanes_shift.  The lanes rule bounds them: the shift is 0 once ntexels exceeds 262144 (want = 1), so items = ntexels
    // <= 2^26 (ZDR_BOUNCE_MAX_TEXELS); below that 2^shift < 2 want <= 2 (262144 / ntexels + 1), so items < 2 (262144 + ntexels) <= 2^20.
    // Either way blockIdx.x * BOUNCE_WAVE in k_bounce_shade stays within 32 bits.
    const dim3 grid((uint32_t)((((uint64_t)B.ntexels << lanes_shift) + BOUNCE_WAVE - 1u) / BOUNCE_WAVE));
    const bool env = S.env_count > 0;
    if (accel_is_bvh) { if (env) bounce_launch<BvhAccel, true>(S, C, B, mt, lanes_shift, grid, dyn, st); else bounce_launch<BvhAccel, false>(S, C, B, mt, lanes_shift, grid, dyn, st); }
    else { if (env) bounce_launch<BruteAccel, true>(S, C, B, mt, lanes_shift, grid, dyn, st); else bounce_launch<BruteAccel, false>(S, C, B, mt, lanes_shift, grid, dyn, st); }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <class A, bool ENV>
static void bounce_dump_launch(const DScene &S, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt, const int32_t *q, uint32_t n, float *out, size_t dyn, hipStream_t st) {
    const dim3 grid((n + BOUNCE_WAVE - 1u) / BOUNCE_WAVE);
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_bounce_dump<0, A, ENV>), grid, dim3(BOUNCE_WAVE), dyn, st, S, C, B, mt, q, n, out);
    else hipLaunchKernelGGL((k_bounce_dump<1, A, ENV>), grid, dim3(BOUNCE_WAVE), dyn, st, S, C, B, mt, q, n, out);
}

int zdr_launch_texel_bounce_dump(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const BounceArgs &B, const MaterialTable &mt,
                                 const int32_t *queries, uint32_t n, float *out, hipStream_t st) {
    DScene S = S_in;
    if (n == 0) return 0;
    const size_t dyn = bounce_dyn_lds(S, accel_is_bvh);
    const bool env = S.env_count > 0;
    if (accel_is_bvh) { if (env) bounce_dump_launch<BvhAccel, true>(S, C, B, mt, queries, n, out, dyn, st); else bounce_dump_launch<BvhAccel, false>(S, C, B, mt, queries, n, out, dyn, st); }
    else { if (env) bounce_dump_launch<BruteAccel, true>(S, C, B, mt, queries, n, out, dyn, st); else bounce_dump_launch<BruteAccel, false>(S, C, B, mt, queries, n, out, dyn, st); }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
