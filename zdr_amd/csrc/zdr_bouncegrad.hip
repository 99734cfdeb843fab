// zdr_bouncegrad.hip — the adjoint of the bounced-light baker (zdr_bounce.hip) for gfx950: the gradient of the irradiance of
// zdr_scene_texel_bounce in the material texels and in the lights' emissions, zdr_scene_texel_bounce_backward (include/zdr.h).  The walk's
// directions come from cosine lobes about the normals, so neither the hits nor the draws depend on the materials: with the walks, the
// light list, the sampling tables, visibility and the acceptance bits held fixed the bake is, per seed, a polynomial in the material
// texels (linear for one bounce) and linear in the emissions, and both gradients are exact transposes.  The device code it calls —
// A::closest, A::any_shadow, surface_interact, read_bsdf_in, sample_light with its mesh_light hook, the samplers, the scatter queue — is
// the path kernels' own (scene.h, accel.h, sampler.h).  Linked into libzdr_bouncegrad.so (zdr_amd/build.py).
//
// Five kernels, launched one after the other on the caller's stream:
//   k_bgrad_clear        the workspace's header, the emission accumulator and the staging cells to 0 (a kernel, not a memset node);
//   k_bgrad_compact      k_bounce_compact without its stores to `out`: an adjoint writes nothing for a texel that is not shaded;
//   k_bgrad_shade        k_bounce_shade's lanes, trips and draws.  Per trip three phases.  (1) Forward replay: the control flow of
//                        bounce_sample (zdr_bounce.hip), vertex by vertex; every vertex leaves a record in LDS — uv, slot, A w, a — and an
//                        accepted sample from the front of a mesh light adds (cotangent x beta x weight) to the wave's table of sums per
//                        light.  (2) Reverse sweep: Q_k = A_k w_k + a_{k+1} Q_{k+1}, written over A w.  (3) Forward sweep with the prefix
//                        beta_{k-1}: d a_k = cotangent x beta_{k-1} x Q_k, one scatter_push per vertex index by the whole wave.  Division
//                        free: an albedo of 0 costs nothing.  The queue's cells, copies and the few-texel LDS path are those of every
//                        material-table backward call (scene.h);
//   k_bgrad_gather_mat   k_material_cells_to_grad (zdr_kernels.hip) for rgb alone: the roughness channel is never written, and a texel
//                        whose cells hold nothing keeps its bits;
//   k_bgrad_gather_emit  the accumulator's rows summed in float64, light l's three floats added into the row of its instance.
// The sums use float atomics and the list's order varies: the result is not bit-stable from run to run.
#include "accel.h"
#include "bouncegrad.h"

#define BGRAD_WAVE 64

__global__ __launch_bounds__(256) void k_bgrad_clear(uint32_t *count, float *acc, uint32_t nacc, float4 *cells, uint32_t ncell_words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < ZDR_BOUNCE_HEADER_BYTES / 4) count[i] = 0u;
    if (i < nacc) acc[i] = 0.0f;
    if (i < ncell_words) cells[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void k_bgrad_compact(BgradArgs G) {
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

ZD bool bgrad_finite(f3 a) { return fabsf(a.x) < __builtin_inff() && fabsf(a.y) < __builtin_inff() && fabsf(a.z) < __builtin_inff(); }

// the cosine lobe of the forward (bounce_cosine_lobe, zdr_bounce.hip)
ZD f3 bgrad_cosine_lobe(f2 u) {
    const float r = fsqrt(u.x), phi = 2.0f * ZDR_PI * u.y;
    float sn, cs;
    sincosf(phi, &sn, &cs);
    return mk3(r * cs, r * sn, fsqrt(1.0f - u.x));
}

// surface_interact (scene.h) with the rounding of zdr_bounce.hip's kernels spelled out.  The replay must decide every acceptance bit as
// the forward did, and a light sample whose shadow ray leaves its own surface at a grazing angle is decided by the last bit of it.p.  The
// interpolation a w0 + b w1 + c w2 is left to the compiler's contraction in scene.h: every kernel of zdr_bounce.hip rounds b w1 and fuses
// the other two products, fma(c, w2, fma(a, w0, b w1)), and so do this unit's BvhAccel kernels — its BruteAccel kernels rounded a w0 in
// it.p.x instead, and one sample of 19,520 of a Cornell-box bake lost the light sample of its first vertex (tests/test_gpu_texel_bake_edges.py,
// cbox_wide).  An explicit fma is the same in every kernel it is inlined into.
ZD Interaction bgrad_interact(const DScene &S, const Hit &h) {
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

// what read_bsdf_in needs of a table entry; chosen per lane from the wave-uniform table (BounceMat of zdr_bounce.hip)
struct BgradMat { int32_t texel, h, w; };

template <int SK, class A, bool ENV>
__global__ __launch_bounds__(BGRAD_WAVE) void k_bgrad_shade(DScene S, SamplerCfg C, BgradArgs G, MaterialTable mt, int lanes_shift, int rec_offset) {
    extern __shared__ __attribute__((aligned(16))) int lds[];   // BvhAccel: this wave's traversal stacks, rec_offset words; then the vertex records, bounces x ZDR_BGRAD_FIELDS x 64 words (both sized at launch)
    __shared__ __attribute__((aligned(16))) float lds_q[ZDR_SCATTER_LDS_FLOATS];   // the scatter queue of the backward kernels (scene.h)
    __shared__ float emit_tab[3 * ZDR_BGRAD_LDS_LIGHTS];        // this wave's sums per light
    const uint32_t count = *G.count;
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x * BGRAD_WAVE + lane;
    if (((blockIdx.x * BGRAD_WAVE) >> lanes_shift) >= count) return;    // wave-uniform: the whole workgroup lies behind the list's end
    const bool want_emit = G.acc != nullptr, want_mat = G.cells != nullptr;   // wave-uniform
    if (want_emit) {
        for (uint32_t i = lane; i < 3 * ZDR_BGRAD_LDS_LIGHTS; i += BGRAD_WAVE) emit_tab[i] = 0.0f;
        __syncthreads();                                     // (one wave per workgroup)
    }
    float *const row = want_emit ? G.acc + (size_t)(blockIdx.x % (unsigned)ZDR_BGRAD_COPIES) * (size_t)(3 * S.light_count) : nullptr;
    ScatterQueue q = scatter_queue_init_cells(lds_q, mt.ncells, G.cell_copies);
    float *const rec = (float *)(lds + rec_offset) + lane;   // field f of vertex k: rec[(k * ZDR_BGRAD_FIELDS + f) * 64]
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
    uint32_t n_push = 0u;                                    // (wave-uniform; lane 0 adds it to the header)
    const uint32_t trips = (G.sample_end - G.sample_begin + lanes - 1u) >> lanes_shift;   // wave-uniform
#pragma unroll 1
    for (uint32_t trip = 0; trip < trips; trip++) {
        const uint32_t s = G.sample_begin + j + (trip << lanes_shift);
        const bool valid = live && s < G.sample_end;
        // a lane without a sample draws all the same, from the range's first sample (k_bounce_shade)
        Sampler smp = sampler_make<SK>(C, x, y, perm_seed, valid ? s : G.sample_begin);
        // ---- phase 1: the walk of bounce_sample (zdr_bounce.hip), statement for statement; the accumulator is replaced by the records
        const f2 u_ao = sampler_next2<SK>(C, smp);
        f3 dir = to_world(make_onb(n), bgrad_cosine_lobe(u_ao));
        f3 org = p;
        float tmin = 1e-4f;
        f3 beta = mk3(1.0f);
        bool alive = valid;
#pragma unroll 1
        for (int k = 0; k < G.bounces; k++) {                // wave-uniform
            const float u_pick = sampler_next<SK>(C, smp), u_prim = sampler_next<SK>(C, smp);
            const f2 u_pt = sampler_next2<SK>(C, smp);
            alive = alive && !any_nan(dir);
            const Hit h = A::closest(S, lds, org, alive ? dir : mk3(0.0f, 0.0f, 1.0f), tmin, alive ? 1e30f : -1.0f);
            alive = alive && h.slot >= 0;
            const bool hit = alive;
            Hit hs = h;
            if (!hit) { hs.slot = 0; hs.u = 0.0f; hs.v = 0.0f; }    // (a lane without a hit reads the first record: any valid address)
            const Interaction it = bgrad_interact(S, hs);
            const bool front = !(dot(-dir, it.ng) < 1e-4f || dot(-dir, it.ns) < 1e-4f);
            int slot = -1;
            if (hit) slot = load_at<int32_t>(mt.inst_slot, 4u * (uint32_t)it.inst);
            const bool shaded = hit && front && slot >= 0;
            BgradMat ms; ms.texel = mt.m[0].texel; ms.h = mt.m[0].h; ms.w = mt.m[0].w;
            for (int jm = 1; jm < mt.nmat; jm++) {           // jm and the entry are wave-uniform
                const bool mine = slot == jm;
                ms.texel = mine ? mt.m[jm].texel : ms.texel; ms.h = mine ? mt.m[jm].h : ms.h; ms.w = mine ? mt.m[jm].w : ms.w;
            }
            f2 muv; muv.x = shaded ? it.uv.x : 0.0f; muv.y = shaded ? it.uv.y : 0.0f;
            const float4 m = read_bsdf_in(G.materials, ms, muv, G.wide_offsets != 0);
            if (shaded) beta = beta * mk3(m.x, m.y, m.z);
            alive = shaded;
            int mesh_light = -1;
            const LightSample L = sample_light<ENV, true>(S, it.p, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; }, nullptr, &mesh_light);
            const float c = dot(it.ns, L.wi);
            const bool lit = alive && c > 0.0f && (L.eval.x > 0.0f || L.eval.y > 0.0f || L.eval.z > 0.0f);
            const bool occ = A::any_shadow(S, lds, it.p, L.wi, 1e-4f, lit ? L.dist : 0.0f);
            const float ws = c * rcp(fmaxf(L.pdf, 1e-4f));
            const f3 add = (beta * L.eval) * ws;
            const bool added = lit && !occ && bgrad_finite(add);   // the forward's acceptance bit A_k
            {   // the record of vertex k (every lane writes every vertex of every trip: nothing stale is ever read)
                float *r = rec + (k * ZDR_BGRAD_FIELDS) * 64;
                const f3 aw = added ? L.eval * ws : mk3(0.0f);
                r[0] = muv.x; r[64] = muv.y; r[128] = __int_as_float(shaded ? slot : -1);
                r[192] = aw.x; r[256] = aw.y; r[320] = aw.z;
                r[384] = shaded ? m.x : 0.0f; r[448] = shaded ? m.y : 0.0f; r[512] = shaded ? m.z : 0.0f;
            }
            if (want_emit && added && mesh_light >= 0 && mesh_light < S.light_count) {
                const f3 term = (dcot * beta) * ws;
                if (bgrad_finite(term)) {
                    if (mesh_light < ZDR_BGRAD_LDS_LIGHTS) {
                        float *e = emit_tab + 3 * mesh_light;
                        __hip_atomic_fetch_add(e, term.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __hip_atomic_fetch_add(e + 1, term.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __hip_atomic_fetch_add(e + 2, term.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    } else {
                        float *e = row + 3 * (size_t)mesh_light;
                        unsafeAtomicAdd(e, term.x); unsafeAtomicAdd(e + 1, term.y); unsafeAtomicAdd(e + 2, term.z);
                    }
                }
            }
            // the next segment: a cosine lobe about the shading normal
            bool on = false;
            f3 nd = dir;
            if (k + 1 < G.bounces) {                         // wave-uniform: the last vertex draws neither u_lobe nor u_dir
                (void)sampler_next<SK>(C, smp);              // u_lobe: drawn and ignored
                const f2 u_dir = sampler_next2<SK>(C, smp);
                const f3 wl = bgrad_cosine_lobe(u_dir);
                nd = to_world(make_onb(it.ns), wl);
                on = alive && !(dot(nd, it.ng) < 1e-4f || wl.z < 1e-4f);
            }
            alive = on;
            dir = nd; org = offset_ray_origin(it.p, it.ng); tmin = 0.0f;
        }
        if (want_mat) {                                      // wave-uniform: every lane of the wave is here
            // ---- phase 2: Q_k = A_k w_k + a_{k+1} Q_{k+1}, last vertex first, left where A w was
            f3 Q = mk3(0.0f), a_next = mk3(0.0f);
#pragma unroll 1
            for (int k = G.bounces - 1; k >= 0; k--) {       // wave-uniform
                float *r = rec + (k * ZDR_BGRAD_FIELDS) * 64;
                Q = mk3(r[192], r[256], r[320]) + a_next * Q;
                r[192] = Q.x; r[256] = Q.y; r[320] = Q.z;
                a_next = mk3(r[384], r[448], r[512]);
            }
            // ---- phase 3: d a_k = cotangent x beta_{k-1} x Q_k, first vertex first; one push per vertex index by the whole wave
            f3 bprev = dcot;
#pragma unroll 1
            for (int k = 0; k < G.bounces; k++) {            // wave-uniform
                const float *r = rec + (k * ZDR_BGRAD_FIELDS) * 64;
                const int slot = __float_as_int(r[128]);
                f2 guv; guv.x = r[0]; guv.y = r[64];
                const f3 da = bprev * mk3(r[192], r[256], r[320]);
                const bool push = slot >= 0 && bgrad_finite(da) && (da.x != 0.0f || da.y != 0.0f || da.z != 0.0f);
                n_push += (uint32_t)__popcll(__ballot(push));
                scatter_push<true, false>(q, G.cells, push, guv, make_float4(da.x, da.y, da.z, 0.0f), 0, 0, 0, push ? slot : 0, mt.m);
                bprev = bprev * mk3(r[384], r[448], r[512]);
            }
        }
    }
    if (want_mat) scatter_finish<true, false>(q, G.cells, 0, 0, 0, mt.m);
    if (want_emit) {
        __syncthreads();
        const uint32_t nt = 3u * (uint32_t)(S.light_count < ZDR_BGRAD_LDS_LIGHTS ? S.light_count : ZDR_BGRAD_LDS_LIGHTS);
        for (uint32_t i = lane; i < nt; i += BGRAD_WAVE) {
            const float v = emit_tab[i];
            if (v != 0.0f) unsafeAtomicAdd(row + i, v);
        }
    }
    if (lane == 0u && n_push != 0u) atomicAdd(G.count + 1, n_push);
}

// The staging cells into the packed gradient (+=), rgb alone: texel (x, y) of material blockIdx.z receives corner (dx, dy) of every cell
// (ix, iy) with clamp(ix + dx) == x and clamp(iy + dy) == y, over all copies — the footprint and the sums of k_material_cells_to_grad
// (zdr_kernels.hip).  A channel whose cells sum to 0 is not written.
__global__ __launch_bounds__(64) void k_bgrad_gather_mat(const float4 *__restrict__ cells, float *__restrict__ dmat, MaterialTable mt) {
    const MaterialSlot m = mt.m[blockIdx.z];
    const int copies = m.copies;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    if (x >= m.w || y >= m.h) return;
    const int tex_h = m.h, tex_w = m.w;
    int ixs[3], dxs[3], nx = 0, iys[3], dys[3], ny = 0;
    ixs[nx] = x - 1; dxs[nx++] = 1; ixs[nx] = x; dxs[nx++] = 0;
    if (x == 0) { ixs[nx] = -1; dxs[nx++] = 0; }
    if (x == tex_w - 1) { ixs[nx] = tex_w - 1; dxs[nx++] = 1; }
    iys[ny] = y - 1; dys[ny++] = 1; iys[ny] = y; dys[ny++] = 0;
    if (y == 0) { iys[ny] = -1; dys[ny++] = 0; }
    if (y == tex_h - 1) { iys[ny] = tex_h - 1; dys[ny++] = 1; }
    double sx = 0.0, sy = 0.0, sz = 0.0;                     // (float64 for the copies, float32 order otherwise)
    f3 acc = mk3(0.0f);
    for (int k = 0; k < copies; k++)
        for (int b = 0; b < ny; b++)
            for (int a = 0; a < nx; a++) {
                const size_t cell = (size_t)k * m.stride + (size_t)m.cell + (size_t)(ixs[a] + 1) + (size_t)(tex_w + 1) * (iys[b] + 1);
                const float4 c = cells[4 * cell + 2 * dxs[a] + dys[b]];
                if (copies == 1) { acc.x += c.x; acc.y += c.y; acc.z += c.z; }
                else { sx += c.x; sy += c.y; sz += c.z; }
            }
    if (copies > 1) acc = mk3((float)sx, (float)sy, (float)sz);
    float *t = dmat + 4 * ((size_t)m.texel + (size_t)x + (size_t)m.w * y);
    if (acc.x != 0.0f) t[0] += acc.x;
    if (acc.y != 0.0f) t[1] += acc.y;
    if (acc.z != 0.0f) t[2] += acc.z;
}

// sums the accumulator's rows in float64 and adds light l's three floats into the row of its instance in d_emission (+=)
__global__ __launch_bounds__(64) void k_bgrad_gather_emit(const float *__restrict__ acc, int copies, int light_count, const int32_t *__restrict__ light_insts, float *__restrict__ d_emission) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 3 * light_count) return;
    double sum = 0.0;
    for (int k = 0; k < copies; k++) sum += (double)acc[(size_t)k * (size_t)(3 * light_count) + i];
    d_emission[3 * (size_t)light_insts[i / 3] + (i % 3)] += (float)sum;
}

template <class A, bool ENV>
static void bgrad_launch(const DScene &S, const SamplerCfg &C, const BgradArgs &G, const MaterialTable &mt, int lanes_shift, int rec_offset, dim3 grid, size_t dyn, hipStream_t st) {
    if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL((k_bgrad_shade<0, A, ENV>), grid, dim3(BGRAD_WAVE), dyn, st, S, C, G, mt, lanes_shift, rec_offset);
    else hipLaunchKernelGGL((k_bgrad_shade<1, A, ENV>), grid, dim3(BGRAD_WAVE), dyn, st, S, C, G, mt, lanes_shift, rec_offset);
}

int zdr_launch_texel_bounce_backward(const DScene &S_in, int accel_is_bvh, const SamplerCfg &C, const BgradArgs &G, const MaterialTable &mt, hipStream_t st) {
    DScene S = S_in;
    if (G.bounces < 1 || G.bounces > ZDR_BOUNCE_MAX_BOUNCES) return 256 * 3 + (int)hipErrorInvalidValue;   // (the records are sized by it)
    const int lanes_shift = zdr_bounce_lanes_shift(G.ntexels, G.sample_end - G.sample_begin);   // the forward's rule
    // dynamic LDS: the traversal stacks as zdr_launch_texel_bounce sizes them, then the records, sized by `bounces`
    int rec_offset = 0;
    if (accel_is_bvh) { S.lds_stack = S.stack_entries < ZDR_BVH_LDS_STACK ? S.stack_entries : ZDR_BVH_LDS_STACK; rec_offset = S.lds_stack * BGRAD_WAVE; }
    const size_t dyn = ((size_t)rec_offset + (size_t)G.bounces * ZDR_BGRAD_FIELDS * BGRAD_WAVE) * sizeof(int);
    const uint32_t nacc = G.acc ? (uint32_t)ZDR_BGRAD_COPIES * 3u * (uint32_t)S.light_count : 0u;
    const uint32_t ncw = G.cells ? G.ncell_words : 0u;
    uint32_t nclear = ZDR_BOUNCE_HEADER_BYTES / 4;
    if (nacc > nclear) nclear = nacc;
    if (ncw > nclear) nclear = ncw;
    // a launch that fails ends the call there: the next kernel would read what this one did not write
    hipError_t e;
    hipLaunchKernelGGL(k_bgrad_clear, dim3((nclear + 255u) / 256u), dim3(256), 0, st, G.count, G.acc, nacc, (float4 *)G.cells, ncw);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 1 + (int)e;
    hipLaunchKernelGGL(k_bgrad_compact, dim3((G.ntexels + 255u) / 256u), dim3(256), 0, st, G);
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 2 + (int)e;
    const dim3 grid((uint32_t)((((uint64_t)G.ntexels << lanes_shift) + BGRAD_WAVE - 1u) / BGRAD_WAVE));   // (zdr_launch_texel_bounce: within 32 bits)
    const bool env = S.env_count > 0;
    if (accel_is_bvh) { if (env) bgrad_launch<BvhAccel, true>(S, C, G, mt, lanes_shift, rec_offset, grid, dyn, st); else bgrad_launch<BvhAccel, false>(S, C, G, mt, lanes_shift, rec_offset, grid, dyn, st); }
    else { if (env) bgrad_launch<BruteAccel, true>(S, C, G, mt, lanes_shift, rec_offset, grid, dyn, st); else bgrad_launch<BruteAccel, false>(S, C, G, mt, lanes_shift, rec_offset, grid, dyn, st); }
    if ((e = hipGetLastError()) != hipSuccess) return 256 * 3 + (int)e;
    if (G.cells) {
        int mh = 1, mw = 1;
        for (int k = 0; k < mt.nmat; k++) { mh = mt.m[k].h > mh ? mt.m[k].h : mh; mw = mt.m[k].w > mw ? mt.m[k].w : mw; }
        hipLaunchKernelGGL(k_bgrad_gather_mat, dim3((mw + 63) / 64, mh, mt.nmat), dim3(64), 0, st, (const float4 *)G.cells, G.d_materials, mt);
        if ((e = hipGetLastError()) != hipSuccess) return 256 * 4 + (int)e;
    }
    if (G.acc) {
        hipLaunchKernelGGL(k_bgrad_gather_emit, dim3((3 * S.light_count + 63) / 64), dim3(64), 0, st, (const float *)G.acc, ZDR_BGRAD_COPIES, S.light_count, S.light_insts, G.d_emission);
        if ((e = hipGetLastError()) != hipSuccess) return 256 * 5 + (int)e;
    }
    return 0;
}
