// zdr_kernels.hip — gfx950 kernels of the zdr hot path and their launchers.
//
// Work item = one 8x8 pixel tile x one chunk of the sample range; workgroups are single 64-lane waves, so
// no workgroup barrier exists anywhere.  The direct / collocated / uvgrad kernels run one workgroup per item
// (lane = pixel), the block index remapped so that each XCD (blocks b, b+8, ... share one) receives a contiguous
// run of tiles: primary-hit texel footprints of neighbouring tiles then share that XCD's L2.  The path kernels are
// persistent waves that draw items from per-XCD counters and treat lanes as workers (see k_path).
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include "integrators.h"
#include "zdr.h"

#define WAVE 64
// __launch_bounds__ second argument = minimum waves per SIMD (caps the VGPR budget at 512 / n).
// Measured on cbox 512^2 spp 256 (profiles/r1_ab_flags.txt): 3 (<= 168 VGPRs, no spills) is best for both.

struct WorkItem { int x, y, pix; bool valid; uint32_t s_begin, s_end; int chunk, tile, tile_local; };   // tile: number within the rectangle; tile_local: within this call's shard

// Work item `logical` = (tile, sample chunk); consecutive items are the chunks of one tile, then the next tile.
ZD WorkItem decode_item(const RenderCfg &R, int logical) {
    const int nblocks = R.ntiles * R.nchunks;
    WorkItem w;
    w.valid = logical >= 0 && logical < nblocks;
    const int tl = w.valid ? logical / R.nchunks : 0;
    w.chunk = w.valid ? logical - tl * R.nchunks : 0;
    const int number = tl * R.shard_count + R.shard_index;   // interleaved tile shard (zdr.h): tile numbers index, index + count, ...
    const int ty = number / R.tiles_x;
    int tx = number - ty * R.tiles_x + ty * R.shard_skew;    // row ty is numbered from column ty * skew on: a shard's tiles run along diagonals
    tx -= (tx / R.tiles_x) * R.tiles_x;
    w.tile = ty * R.tiles_x + tx; w.tile_local = tl;         // .tile: position in the tile grid (tile masks), .tile_local: position in the shard's workspace
    const int lane = threadIdx.x;
    w.x = R.x0 + tx * 8 + (lane & 7);
    w.y = R.y0 + ty * 8 + (lane >> 3);
    w.valid = w.valid && (w.x < R.x1) && (w.y < R.y1);
    w.pix = w.x + w.y * R.width;
    w.s_begin = R.sample_begin + (uint32_t)w.chunk * R.chunk;
    uint32_t e = w.s_begin + R.chunk;
    w.s_end = (e < R.sample_end) ? e : R.sample_end;
    return w;   // the sample range is wave-uniform; lanes outside the shard are masked with w.valid
}

// one workgroup per item (direct / collocated / uvgrad kernels): XCD-contiguous tile runs
ZD WorkItem decode_block(const RenderCfg &R) {
    const int nblocks = R.ntiles * R.nchunks;
    const int per_xcd = (nblocks + 7) >> 3;
    const int b = blockIdx.x;
    const int logical = (b & 7) * per_xcd + (b >> 3);
    return decode_item(R, logical < nblocks ? logical : -1);
}

// Persistent waves (path kernels) draw items from eight counters, one per XCD: a wave on XCD x
// (workgroups are dealt round-robin, x = blockIdx.x & 7) walks x's contiguous run of tiles, so the texel
// footprints of neighbouring tiles share that XCD's L2; when its own run is used up it takes from the others.
// Wave-uniform; returns -1 when no item is left.  Counters only grow, by at most 8 per call.
ZD int fetch_item(const RenderCfg &R, unsigned int *counters) {
    const int nblocks = R.ntiles * R.nchunks;
    const int per_xcd = (nblocks + 7) >> 3;
    int got = -1;
    if (threadIdx.x == 0) {
        const int x = blockIdx.x & 7;
        for (int j = 0; j < 8 && got < 0; j++) {
            const int y = (x + j) & 7;
            const unsigned int local = atomicAdd(&counters[y], 1u);
            const long long logical = (long long)y * per_xcd + local;
            if (local < (unsigned int)per_xcd && logical < nblocks) got = (int)logical;
        }
    }
    return __builtin_amdgcn_readfirstlane(got);
}

// candidate triangle pairs of this wave's camera rays (BruteAccel::closest_camera): the tile's mask, or every pair
ZD unsigned long long camera_mask(const DScene &S, const KernelIO &io, const WorkItem &w) {
    const int npairs = (S.nquads + 1) >> 1;
    const unsigned long long all = (npairs >= 64) ? ~0ull : ((1ull << npairs) - 1ull);
    return io.tile_masks ? io.tile_masks[w.tile] : all;
}

ZD void store_pixel(const RenderCfg &R, const SamplerCfg &C, const KernelIO &io, const WorkItem &w, f3 sum) {
    if (!w.valid) return;
    if (R.nchunks == 1) {   // integrator.py:29: (s / spp, 1)
        float fs = (float)C.spp;
        io.image[w.pix] = make_float4(__fdiv_rn(sum.x, fs), __fdiv_rn(sum.y, fs), __fdiv_rn(sum.z, fs), R.alpha);
    } else {
        // chunk partials: [chunk][tile of this shard][lane] — a wave writes one contiguous 1 KiB line
        io.partial[((size_t)w.chunk * R.ntiles + w.tile_local) * WAVE + threadIdx.x] = make_float4(sum.x, sum.y, sum.z, 0.0f);
    }
}

ZD f3 load_le_grad(const SamplerCfg &C, const KernelIO &io, const WorkItem &w) {   // integrator.py:38-40
    f3 g = mk3(0.0f);
    if (w.valid) {
        float4 gi = io.d_image[w.pix];
        float fs = (float)C.spp;
        g = mk3(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs));
        if (any_nan(g)) g = mk3(0.0f);
    }
    return g;
}

template <bool STATS>
ZD void flush_counters(const KernelIO &io, const Counters &cnt) {
    if (!STATS) return;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        unsigned long long v = cnt.c[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
        if (threadIdx.x == 0 && v) atomicAdd(io.counters + i, v);
    }
}

// --------------------------------------------------------------------------- tile masks
// One wave per 8x8 tile, lane = pair of primitives of the brute-force walk: bit k of the tile's mask is set unless ALL triangles
// of pair k lie entirely outside one side plane of the tile's camera frustum (or behind the camera).
// The frustum is padded by one pixel: the tent filter (camera.py:20-31) moves a sample up to half a
// pixel outside its pixel.  Conservative by construction — a set bit only costs a test.
__global__ __launch_bounds__(WAVE) void k_tile_masks(DScene S, RenderCfg R, unsigned long long *masks) {
    const int tile = blockIdx.x, ty = tile / R.tiles_x, tx = tile - ty * R.tiles_x, lane = threadIdx.x;
    const float X0 = (float)(R.x0 + tx * 8) - 1.0f, X1 = (float)(R.x0 + tx * 8 + 8) + 1.0f;
    const float Y0 = (float)(R.y0 + ty * 8) - 1.0f, Y1 = (float)(R.y0 + ty * 8 + 8) + 1.0f;
    const f3 right = ld3(R.cam_right), upp = ld3(R.cam_upp), fwd = ld3(R.cam_fwd), co = ld3(R.cam_o);
    auto dir = [&](float X, float Y) {                      // pixel_ray without the normalisation
        float px = (R.two_over_w * X - 1.0f) * R.cam_tan, py = ((R.two_over_h * Y - 1.0f) * R.aspect) * R.cam_tan;
        return (right * px - upp * py) + fwd;
    };
    const f3 c00 = dir(X0, Y0), c10 = dir(X1, Y0), c01 = dir(X0, Y1), c11 = dir(X1, Y1);
    f3 n[4] = { cross(c00, c01), cross(c11, c10), cross(c10, c00), cross(c01, c11) };   // left, right, top, bottom
    const f3 inside = (c00 + c11) + (c10 + c01);
#pragma unroll
    for (int k = 0; k < 4; k++) if (dot(n[k], inside) < 0.0f) n[k] = n[k] * -1.0f;
    const int npairs = (S.nquads + 1) >> 1;
    bool keep = false;
    if (lane < npairs) {
        // the (up to four) triangles of primitives 2 lane and 2 lane + 1: quads cover slots 2q, 2q + 1, single triangles follow (accel.h)
        const int q0 = 2 * lane, q1 = 2 * lane + 1;
        const int b0 = q0 < S.nquads2 ? 2 * q0 : q0 + S.nquads2, n0 = q0 < S.nquads2 ? 2 : 1;
        const int b1 = q1 < S.nquads2 ? 2 * q1 : q1 + S.nquads2, n1 = q1 >= S.nquads ? 0 : (q1 < S.nquads2 ? 2 : 1);
        for (int i = 0; i < n0 + n1; i++) {
            const int t = i < n0 ? b0 + i : b1 + (i - n0);
            const float4 *r = S.shade + 8 * (size_t)t;
            f3 v0 = xyz(r[0]) - co, v1 = xyz(r[1]) - co, v2 = xyz(r[2]) - co;
            float vm = fmaxf(fmaxf(length(v0), length(v1)), length(v2));
            bool culled = (dot(v0, fwd) <= 0.0f) && (dot(v1, fwd) <= 0.0f) && (dot(v2, fwd) <= 0.0f);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float e = -1e-4f * length(n[k]) * vm;
                culled = culled || ((dot(n[k], v0) < e) && (dot(n[k], v1) < e) && (dot(n[k], v2) < e));
            }
            keep = keep || !culled;
        }
    }
    unsigned long long m = __ballot(keep);
    if (lane == 0) masks[tile] = m;
}

// ------------------------------------------------------------------------------------- path
// Forward (and the counting variant).  PERSISTENT waves: the grid is what the chip holds at once, and each
// wave draws work items (tile x sample chunk) until none is left.  Two alternating phases:
//   refill  lane = pixel: ZDR_RING_BATCH camera samples per pixel of the current item are generated, traced
//           and classified by the whole wave and the vertices to shade are parked in the wave's FIFO;
//   flat loop  a lane is just a worker: it takes the next parked vertex (of ANY pixel) and each trip
//           shades one vertex:  shade (light sample, BSDF sample, the vertex's two rays) -> classify the new hit.
// Items overlap: when the current item has no camera sample left the wave starts the next one while the last
// paths of the old one are still running, so lanes never wait for a tile's longest path.  Per-pixel state
// (radiance sums, CMJ seeds) therefore lives in LDS in two banks, item n in bank n & 1; a path carries its
// bank and pixel.  Radiance is added with ds_add_f32 — one wave, program order: a pixel's sum depends only on the trips and lanes
// its paths finish on.  Those are fixed for the first item a wave draws.  A later item starts among the last paths of the one
// before, and which item that was depends on the order in which the waves reached the work counters: its sums are the same terms,
// added in an order that can differ from run to run, i.e. in the last bit (DESIGN.md section 5 has the measurement).
// Four named scalars, chosen by a wave-uniform bank with a select and never with an index: as two arrays indexed by `bank` the
// struct was demoted to scratch memory in every k_path_bwd (16 bytes of its private segment), and each trip read and wrote these
// four loop counters through the vector-memory path, behind the flush's atomics (profiles/item_banks_isa.txt).  Every writer pins
// its value with readfirstlane, so the members live in SGPRs and the bookkeeping runs on the scalar unit.
struct ItemBanks {
    int logical0, logical1;          // item held by each bank, -1 = free (wave-uniform)
    uint32_t inflight0, inflight1;   // parked + running paths of each bank (wave-uniform)
    ZD void init() { logical0 = logical1 = -1; inflight0 = inflight1 = 0u; }
    ZD int logical(int bank) const { return bank ? logical1 : logical0; }
    ZD uint32_t inflight(int bank) const { return bank ? inflight1 : inflight0; }
    ZD void set_logical(int bank, int item) {
        item = __builtin_amdgcn_readfirstlane(item);
        logical0 = bank ? logical0 : item; logical1 = bank ? item : logical1;
    }
    ZD void parked(int bank, uint32_t n) {              // n more paths of `bank` are in the FIFO
        n = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
        inflight0 += bank ? 0u : n; inflight1 += bank ? n : 0u;
    }
    ZD void finished(bool done, int pix) {              // the paths that ended this trip leave their banks (pix: bank * 64 + pixel)
        inflight0 -= (uint32_t)__popcll(__ballot(done && (pix >> 6) == 0));
        inflight1 -= (uint32_t)__popcll(__ballot(done && (pix >> 6) == 1));
    }
    // every camera sample generated and no path left (cur: the current item's bank, drained: it has no camera sample left)
    ZD bool retirable(int b, int cur, bool drained) const { return logical(b) >= 0 && inflight(b) == 0u && (b != cur || drained); }
};

// The persistent kernels read their launch constants (scene pointers, camera, sampler grid ...) through a pointer to the kernarg
// segment that is laundered once per trip, so a constant is s_load-ed again where a trip uses it instead of being kept for the whole
// kernel in an SGPR that is spilled to a VGPR lane (v_readlane / v_writelane / s_nop on the VALU port: 320 reloads in
// k_path<cmj, brute> before; profiles/r3_bwd_records_and_atomics.txt).  PathKArgs must be the kernels' parameter list, in order:
// every kernel that uses the macros is declared through ZDR_PATH_KERNEL_PARAMS, and the layout rules the kernarg segment follows
// (each by-value struct at its natural alignment, at most 8 here) are asserted below.
struct PathKArgs { DScene S; RenderCfg R; SamplerCfg C; KernelIO io; };
#define ZDR_PATH_KERNEL_PARAMS DScene S_, RenderCfg R_, SamplerCfg C_, KernelIO io_
static constexpr size_t zdr_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static_assert(std::is_trivially_copyable<PathKArgs>::value && std::is_standard_layout<PathKArgs>::value, "kernel arguments are copied bytewise");
static_assert(offsetof(PathKArgs, S) == 0, "first kernel argument at offset 0 of the kernarg segment");
static_assert(offsetof(PathKArgs, R) == zdr_align_up(sizeof(DScene), alignof(RenderCfg)), "PathKArgs does not mirror the kernarg packing");
static_assert(offsetof(PathKArgs, C) == zdr_align_up(offsetof(PathKArgs, R) + sizeof(RenderCfg), alignof(SamplerCfg)), "PathKArgs does not mirror the kernarg packing");
static_assert(offsetof(PathKArgs, io) == zdr_align_up(offsetof(PathKArgs, C) + sizeof(SamplerCfg), alignof(KernelIO)), "PathKArgs does not mirror the kernarg packing");
static_assert(alignof(DScene) <= 8 && alignof(RenderCfg) <= 8 && alignof(SamplerCfg) <= 8 && alignof(KernelIO) <= 8, "an over-aligned member would change the kernarg packing");
typedef __attribute__((address_space(4))) const char karg_byte_t;
ZD const PathKArgs &kargs_fresh() {
    karg_byte_t *p = (karg_byte_t *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const PathKArgs *)p;
}
#define ZDR_KARGS_BEGIN const PathKArgs *ka = &kargs_fresh();
#define ZDR_KARGS_REFRESH ka = &kargs_fresh();
// Timing-only ablations of the backward kernels exist in measurement builds alone (-DZDR_MEASURE, tools/): the product reads no
// ZDR_DEBUG_NO_SCATTER and every `ZDR_ABLATE == n` below folds to false.
#ifdef ZDR_MEASURE
#define ZDR_ABLATE (R.debug_no_scatter)
#else
#define ZDR_ABLATE 0
#endif

// MT: material-table mode (zdr_render_forward_materials): io.material is the packed buffer and io.mt says which material shades what
template <int SK, class A, bool STATS, bool ENV, bool MT>
__global__ __launch_bounds__(WAVE, ENV ? A::kMinWavesFwdEnv : A::kMinWavesFwd) void k_path(ZDR_PATH_KERNEL_PARAMS) {
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    __shared__ uint32_t lds_perm[2 * WAVE];
    __shared__ int lds_origin[4];
    __shared__ float lds_sum[2 * 3 * WAVE];
    const int lane = threadIdx.x;
    Counters cnt;
#pragma unroll
    for (int i = 0; i < 8; i++) cnt.c[i] = 0;
    PathVertex pv; f3 term_Li = mk3(0.0f);
    ItemBanks ib; ib.init();
    int bank = 1;                                           // bank of the current item (the first fetch flips it to 0)
    bool more_items = true;
    WorkItem w = decode_item(R, -1);
    uint32_t next_sample = 0, s_end = 0, perm_seed = 0;
    unsigned long long cam_mask = 0ull;
    f3 sum = mk3(0.0f);                                     // current item, this lane's pixel: paths that ended at the camera ray
    PrimaryQueue q = queue_init(io);
    bool alive = false; int pix = 0;                        // pix: bank * 64 + pixel of the running path
    PathState ps; Interaction it;
    ps.o = mk3(0.0f); ps.d = mk3(0.0f, 0.0f, 1.0f); ps.beta = mk3(1.0f); ps.L = mk3(0.0f); ps.pdf_bsdf = 1e30f; ps.depth = 0;
    ps.smp = sampler_make<SK>(C, 0, 0, 0, 0);
    it.p = mk3(0.0f); it.uv.x = 0.0f; it.uv.y = 0.0f; it.ns = mk3(0.0f, 0.0f, 1.0f); it.ng = it.ns; it.inst = 0; it.prim = 0;
    int stall = 0;
    for (;;) {
        ZDR_KARGS_REFRESH
        bool progress = false;
        if (q.tail - q.head < (uint32_t)__popcll(__ballot(!alive))) {          // the FIFO cannot serve every idle lane
            if (next_sample < s_end) {
                progress = true;
                const uint32_t t0 = q.tail;
                primary_refill<SK, A, false, STATS, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, q, sum, cnt,
                                                             MT ? io.mt.inst_slot : nullptr);
                ib.parked(bank, q.tail - t0);
            } else if (more_items && ib.logical(bank ^ 1) < 0) {                // next item, into the free bank
                if (ib.logical(bank) >= 0) {                                    // park the register part of the old item's sums
                    atomicAdd(&lds_sum[(bank * 3 + 0) * WAVE + lane], sum.x); atomicAdd(&lds_sum[(bank * 3 + 1) * WAVE + lane], sum.y);
                    atomicAdd(&lds_sum[(bank * 3 + 2) * WAVE + lane], sum.z);
                    sum = mk3(0.0f);
                }
                const int nxt = fetch_item(R, io.work_counters);
                if (nxt < 0) more_items = false;
                else {
                    bank ^= 1;
                    ib.set_logical(bank, nxt);
                    w = decode_item(R, nxt);
                    perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
                    cam_mask = camera_mask(S, io, w);
                    lds_perm[bank * WAVE + lane] = perm_seed;
                    if (lane == 0) { lds_origin[bank * 2] = w.x; lds_origin[bank * 2 + 1] = w.y; }
                    lds_sum[(bank * 3 + 0) * WAVE + lane] = 0.0f; lds_sum[(bank * 3 + 1) * WAVE + lane] = 0.0f; lds_sum[(bank * 3 + 2) * WAVE + lane] = 0.0f;
                    __syncthreads();
                    next_sample = w.s_begin; s_end = w.s_end;
                }
                stall = 0;
                continue;
            }
        }
        const int took = primary_pop<SK, MT>(S, C, !alive, lds_perm, lds_origin, q, ps, it, MT ? io.mt.inst_slot : nullptr);
        if (took >= 0) { alive = true; pix = took; }
        {   // (No wave-uniform `if (__ballot(alive) != 0ull)` around this: with it the compiler kept the path state in two register sets, one
            // that lives across the trips and one that the shading works on, and copied all 27 registers in before and back after every trip.)
            if (__ballot(alive) != 0ull) progress = true;
            bool done = false;
            if (alive) {
                Hit h;
                done = path_shade<SK, A, false, STATS, ENV, MT>(S, R, C, io, lds, ps, it, pv, h, cnt);
                if (!done) { path_continue<A, STATS>(S, lds, ps, h, cnt); done = path_arrive<false, STATS, ENV, MT>(S, ps, h, it, term_Li, cnt, nullptr, MT ? io.mt.inst_slot : nullptr); }
                if (done) {
                    alive = false;
                    if (!any_nan(ps.L)) {                   // integrator.py:27-28
                        f3 c = clamp_radiance(ps.L);
                        const int bk = pix >> 6, px = pix & 63;
                        atomicAdd(&lds_sum[(bk * 3 + 0) * WAVE + px], c.x); atomicAdd(&lds_sum[(bk * 3 + 1) * WAVE + px], c.y);
                        atomicAdd(&lds_sum[(bk * 3 + 2) * WAVE + px], c.z);
                    } else COUNT(C_NAN);
                }
            }
            ib.finished(done, pix);
        }
        // retire finished items: every camera sample generated and no path left
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (ib.retirable(b, bank, next_sample >= s_end)) {
                __syncthreads();
                const WorkItem wb = decode_item(R, ib.logical(b));
                f3 tot = mk3(lds_sum[(b * 3 + 0) * WAVE + lane], lds_sum[(b * 3 + 1) * WAVE + lane], lds_sum[(b * 3 + 2) * WAVE + lane]);
                if (b == bank) { tot = tot + sum; sum = mk3(0.0f); }
                if (!STATS) store_pixel(R, C, io, wb, tot);         // the stats variant owns no image
                ib.set_logical(b, -1);
            }
        }
        if (__ballot(alive) == 0ull && q.tail == q.head && next_sample >= s_end && !more_items) break;   // both banks are retired by now
        stall = progress ? 0 : stall + 1;
        if (stall > 4) { raise_device_error(S, ZDR_DEVERR_STALL); break; }   // cannot happen (every branch above makes progress); never spin on the GPU, never end silently
    }
    flush_counters<STATS>(io, cnt);
#undef S
#undef R
#undef C
#undef io
}

// Environment-gradient kernels: the cotangent / spp of pixel (px, py), as a popped path of k_path_bwd computes it
ZD f3 pixel_cotangent(const SamplerCfg &C, const KernelIO &io, int width, uint32_t px, uint32_t py) {
    const float4 gi = io.d_image[px + py * (uint32_t)width];   // (once per camera sample or term, not per trip: left in the 64-bit form)
    f3 g;
    if (C.spp_pow2) g = mk3(gi.x * C.inv_spp, gi.y * C.inv_spp, gi.z * C.inv_spp);
    else { const float fs = (float)C.spp; g = mk3(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs)); }
    if (any_nan(g)) g = mk3(0.0f);
    return g;
}
// queues the gradient g of an environment term at map coordinates uv (whole wave; g = 0: nothing).  A NaN gradient is dropped here, per
// term: a path whose radiance turns NaN later (the forward drops that sample) keeps the terms it queued before.  Alpha receives nothing.
ZD void env_push(ScatterQueue &q, const KernelIO &io, const RenderCfg &R, f3 g, f2 uv) {
    const float4 g4 = make_float4(g.x, g.y, g.z, 0.0f);
    scatter_push<true, true>(q, io.cells, any_nonzero4(g4) && !any_nan4(g4), uv, g4, R.tex_h, R.tex_w, ZDR_ABLATE, ZDR_ENV_ENTRY, io.mt.m);
}

// Emission-gradient kernels (LG; zdr_render_backward_emission).  Every term is (weight x cotangent) -> the three floats of ONE light, and a
// shaded vertex brings one or two of them: sent to memory one by one they would all meet on 3 x light_count addresses.  So a wave sums
// them on chip first, in a table of ZDR_EMIT_LDS_LIGHTS x 3 floats in LDS (ds_add_f32, any lane, no reconvergence needed; the table lives
// as long as the wave, i.e. over all trips and items of a persistent wave) and writes the table out ONCE, when the kernel ends, into
// row blockIdx % ZDR_EMISSION_COPIES of the replicated accumulator io.emit_acc [copy][light][3]; k_emission_gather sums the rows in float64.
// A light beyond the table (index >= ZDR_EMIT_LDS_LIGHTS) adds straight into the wave's row with global atomics: correct, and slow
// when such lights carry most of the terms.  A NaN term is dropped on its own, like an environment term.
#define ZDR_EMIT_LDS_LIGHTS 10       // 120 bytes: what the backward path kernel's eight LDS blocks have left beside the record pool
ZD void emit_table_init(float *lds_emit) {   // whole wave
    if (threadIdx.x < 3 * ZDR_EMIT_LDS_LIGHTS) lds_emit[threadIdx.x] = 0.0f;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
ZD float *emit_row(const KernelIO &io, int light_count) { return io.emit_acc + (size_t)(blockIdx.x % (unsigned)ZDR_EMISSION_COPIES) * (size_t)(3 * light_count); }
ZD void emit_add(float *lds_emit, const KernelIO &io, int light_count, const EmitTerm &t, f3 cotangent) {   // any lane
    const f3 g = t.w * cotangent;
    if (t.light < 0 || t.light >= light_count || any_nan(g) || !((g.x != 0.0f) | (g.y != 0.0f) | (g.z != 0.0f))) return;
    if (t.light < ZDR_EMIT_LDS_LIGHTS) {
        float *c = lds_emit + 3 * t.light;
        __hip_atomic_fetch_add(c, g.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(c + 1, g.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        __hip_atomic_fetch_add(c + 2, g.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    } else {
        float *c = emit_row(io, light_count) + 3 * (size_t)t.light;
        unsafeAtomicAdd(c, g.x); unsafeAtomicAdd(c + 1, g.y); unsafeAtomicAdd(c + 2, g.z);
    }
}
ZD void emit_table_finish(float *lds_emit, const KernelIO &io, int light_count) {   // whole wave, end of the kernel
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n = 3 * (light_count < ZDR_EMIT_LDS_LIGHTS ? light_count : ZDR_EMIT_LDS_LIGHTS);
    if ((int)threadIdx.x < n) {
        const float v = lds_emit[threadIdx.x];
        if (v != 0.0f) unsafeAtomicAdd(emit_row(io, light_count) + threadIdx.x, v);
    }
}
// sums the accumulator's rows in float64 and adds light l's three floats into the row of its instance in d_emission (+=)
__global__ void k_emission_gather(const float *__restrict__ acc, int copies, int light_count, const int32_t *__restrict__ light_insts, float *__restrict__ d_emission) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * light_count) return;
    double sum = 0.0;
    for (int k = 0; k < copies; k++) sum += (double)acc[(size_t)k * (size_t)(3 * light_count) + i];
    d_emission[3 * (size_t)light_insts[i / 3] + (i % 3)] += (float)sum;
}
// zdr_scene_set_emission_values: block l rewrites light l's emission in `emission`, `emission4` (.w keeps the light index) and the light table
__global__ void k_set_emission_values(const float *__restrict__ src, const int32_t *__restrict__ light_insts, const int32_t *__restrict__ light_range,
                                      float *__restrict__ emission, float4 *__restrict__ emission4, float4 *__restrict__ light_tris) {
    const int l = blockIdx.x, inst = light_insts[l];
    const float4 e = make_float4(src[3 * (size_t)inst], src[3 * (size_t)inst + 1], src[3 * (size_t)inst + 2], __int_as_float(l));
    if (threadIdx.x == 0) {
        emission[3 * (size_t)inst] = e.x; emission[3 * (size_t)inst + 1] = e.y; emission[3 * (size_t)inst + 2] = e.z;
        emission4[inst] = e;
    }
    const int base = light_range[2 * l], T = light_range[2 * l + 1];
    for (int t = threadIdx.x; t < T; t += blockDim.x) light_tris[5 * (size_t)(base + t) + 4] = make_float4(e.x, e.y, e.z, 0.0f);
}
int zdr_launch_set_emission_values(const DScene &S, const float *src, float *emission, float4 *emission4, float4 *light_tris, hipStream_t st) {
    if (S.light_count <= 0) return 0;
    hipLaunchKernelGGL(k_set_emission_values, dim3(S.light_count), dim3(64), 0, st, src, S.light_insts, S.light_range, emission, emission4, light_tris);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// PRB backward with ONE traversal.  Each trip a live lane shades one vertex of its path (same trip
// order, primary queue, pixel-free lanes, persistent waves and item banks as k_path) and appends it to its record list.  The
// records (5 float4 + a link to the path's previous one) live in a per-wave LDS POOL, see below; the few that find no slot go to
// per-lane scratch.  When a path ends, a short wave-uniform loop sweeps its records last to first and queues the
// gradients; all queue traffic happens at reconverged points so the whole wave takes part in a flush.
// Keeping the records out of scratch is what matters: 2.3 KB of scratch per lane thrashed L2 (113 GB of
// fabric traffic per launch, 13 of 37 ms, round 1); the last 17 % cost 1.4 ms of 13.6 (profiles/r3_bwd_records_and_atomics.txt).
// Neither the CMJ seeds nor the pixel cotangents of the two item banks are kept in LDS (a popped path hashes its seed again and
// loads its cotangent from the image): that leaves room for the pool in 8 of gfx950's 1,280-byte LDS blocks, 16 waves per CU.
// (The lane-owned record rows, the 12-wave layout with seeds and cotangents in LDS and the LDS padding experiment that preceded
// this are kept as profiles/r4_pruned_experiment_branches.patch.)
// MT (zdr_render_backward_materials): a record's material rides in its link word — the pool's links are 16 bits wide (two slots fewer keep the
// LDS blocks), the scratch links are ints anyway — as `previous location | material << 8`; the 80-byte record itself is unchanged.
// EG (zdr_render_backward_env; implies ENV and MT, the map being entry ZDR_ENV_ENTRY of the material table): the terms that read the
// environment map are queued as they happen, each as (weight x the path's cotangent) at its map coordinates — a camera ray that misses
// (primary_refill), a light sample on the environment once its shadow ray is known to be free, a continuation ray that misses.  They
// need no sweep: nothing that decides a path reads the map.  They share the scatter queue with the material gradients.
// LG (zdr_render_backward_emission; implies MT, never with EG): the terms that read a light's emission — a camera ray or a continuation
// ray that ends on a light, a light sample on a mesh light whose shadow ray is free — go to the wave's emission table (emit_add) as they
// happen; no sweep either.
// All three are appended template flags: with a flag off, the kernel compiles to the very instructions it had before the flag existed
// (tools/isa_diff.py --pair-appended-false; profiles/fold_backward_isa_diff.txt).
typedef unsigned int zdr_u4 __attribute__((ext_vector_type(4)));
template <int SK, class A, bool ENV, bool MT, bool EG = false, bool LG = false>
__global__ __launch_bounds__(WAVE, A::kMinWavesBwd) void k_path_bwd(ZDR_PATH_KERNEL_PARAMS) {
    static_assert(!EG || (ENV && MT), "the environment gradient runs in the material-table environment kernels");
    static_assert(!LG || (MT && !EG), "the emission gradient runs in the material-table kernels, without the environment gradient");
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    __shared__ __attribute__((aligned(16))) float lds_q[ZDR_SCATTER_LDS_FLOATS];   // the queue writes g as one float4
    // The records of all paths of the wave share ONE pool of NS slots (80 bytes + a link each): a lane takes its home slot
    // (slot == lane) when that is free and otherwise the lowest free one, and gives the slot back when the sweep has read it.
    constexpr int NS = MT ? A::kPoolSlots - 2 : A::kPoolSlots;
    static_assert(NS >= 16 && NS <= 128, "the free mask is two 64-bit words");
    static_assert(ZDR_MAX_MATERIALS <= 256, "a material fits the upper byte of a link");
    typedef typename std::conditional<MT, unsigned short, unsigned char>::type link_t;
    __shared__ float4 lds_pool[5 * NS];                     // [float4 f][slot]
    __shared__ link_t lds_link[NS];                  // slot of the path's previous record (255: in scratch; a path's first record links to nothing and its link is never followed).  One byte: three more slots fit
    // bit s set: slot s is free.  The only state lanes share: lane 0 stores the mask after an allocation, the sweep's lanes OR freed
    // slots in, every lane reads it before the next allocation.  All three accesses are volatile or atomic and stand between
    // wavefront-scope fences, so the protocol does not rest on what the optimiser happens to do with plain LDS accesses.
    __shared__ __attribute__((aligned(16))) unsigned int lds_free[4];
    __shared__ int lds_origin[4];                           // first pixel of each item bank's tile
    float *lds_emit = nullptr;                              // LG: the wave's emission table (emit_add)
    if constexpr (LG) { __shared__ float lds_emit_table[3 * ZDR_EMIT_LDS_LIGHTS]; lds_emit = lds_emit_table; }
    const int lane = threadIdx.x;
    constexpr unsigned long long all_lo = (NS >= 64) ? ~0ull : ((1ull << (NS & 63)) - 1ull);
    constexpr unsigned long long all_hi = (NS > 64) ? ((NS >= 128) ? ~0ull : ((1ull << ((NS - 64) & 63)) - 1ull)) : 0ull;
    if (lane < 4) {
        const unsigned long long w = (lane < 2) ? all_lo : all_hi;
        lds_free[lane] = (unsigned int)((lane & 1) ? (w >> 32) : w);
    }
    __syncthreads();
    int last = -1;                                          // where the running path's most recent record lives: slot, 255 = scratch, -1 = none yet
    int deep_link[ZDR_MAX_RECORDED_DEPTH];
    Counters cnt;
    ItemBanks ib; ib.init();
    int bank = 1;
    bool more_items = true;
    WorkItem w = decode_item(R, -1);
    uint32_t next_sample = 0, s_end = 0, perm_seed = 0;
    unsigned long long cam_mask = 0ull;
    f3 le_grad = mk3(0.0f);                                 // cotangent of the running path's pixel
    ScatterQueue q = MT ? scatter_queue_init_cells(lds_q, io.mt.ncells, R.cell_copies) : scatter_queue_init(lds_q, R.tex_h, R.tex_w, R.cell_copies);
    if constexpr (EG) q.lds_cells = nullptr;                // the map's cells are never in LDS (table_cell_env)
    if constexpr (LG) emit_table_init(lds_emit);
    PackedVertex deep[ZDR_MAX_RECORDED_DEPTH];
    int nrec = 0;
    PrimaryQueue pq = queue_init(io);
    f3 unused_sum = mk3(0.0f);
    bool alive = false; int pix = 0;
    PathState ps; Interaction it;
    ps.o = mk3(0.0f); ps.d = mk3(0.0f, 0.0f, 1.0f); ps.beta = mk3(1.0f); ps.L = mk3(0.0f); ps.pdf_bsdf = 1e30f; ps.depth = 0;
    ps.smp = sampler_make<SK>(C, 0, 0, 0, 0);
    it.p = mk3(0.0f); it.uv.x = 0.0f; it.uv.y = 0.0f; it.ns = mk3(0.0f, 0.0f, 1.0f); it.ng = it.ns; it.inst = 0; it.prim = 0;
    int stall = 0;
#ifdef ZDR_MEASURE_STATS
    unsigned long long st_trips = 0, st_shaded = 0, st_fin = 0, st_iters = 0, st_steps = 0;
#endif
    for (;;) {
        ZDR_KARGS_REFRESH
        bool progress = false;
        if (pq.tail - pq.head < (uint32_t)__popcll(__ballot(!alive))) {
            if (next_sample < s_end) {
                const uint32_t t0 = pq.tail;
                if constexpr (EG) {
                    // lane = pixel here: a camera ray that misses is a term of this lane's own pixel (weight 1 x mis of pdf_bsdf = 1e30)
                    auto camera_miss = [&](const EnvTerm &e) {
                        f3 g = mk3(0.0f);
                        if (w.valid && ((e.w.x != 0.0f) | (e.w.y != 0.0f) | (e.w.z != 0.0f))) g = e.w * pixel_cotangent(C, io, R.width, (uint32_t)w.x, (uint32_t)w.y);
                        env_push(q, io, R, g, e.uv);
                    };
                    primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                                io.mt.inst_slot, camera_miss);
                } else if constexpr (LG) {
                    // lane = pixel here: a camera ray that ends on a light is a term of this lane's own pixel
                    auto camera_emit = [&](const EmitTerm &e) {
                        if (e.light >= 0) emit_add(lds_emit, io, S.light_count, e, pixel_cotangent(C, io, R.width, (uint32_t)w.x, (uint32_t)w.y));
                    };
                    primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                                io.mt.inst_slot, NoEnvMiss(), camera_emit);
                } else
                primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                            MT ? io.mt.inst_slot : nullptr);
                ib.parked(bank, pq.tail - t0);
                progress = true;
            } else if (more_items && ib.logical(bank ^ 1) < 0) {
                const int nxt = fetch_item(R, io.work_counters);
                if (nxt < 0) more_items = false;
                else {
                    bank ^= 1;
                    ib.set_logical(bank, nxt);
                    w = decode_item(R, nxt);
                    perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
                    cam_mask = camera_mask(S, io, w);
                    if (lane == 0) { lds_origin[bank * 2] = w.x; lds_origin[bank * 2 + 1] = w.y; }
                    __syncthreads();
                    next_sample = w.s_begin; s_end = w.s_end;
                }
                stall = 0;
                continue;
            }
        }
        const int took = primary_pop<SK, MT>(S, C, !alive, nullptr, lds_origin, pq, ps, it, MT ? io.mt.inst_slot : nullptr);
        if (took >= 0) {
            {   // the pixel's cotangent / spp, straight from the image (load_le_grad; a popped path is inside the shard)
                const uint32_t gp = ps.smp.px + ps.smp.py * (uint32_t)R.width;
                const float4 gi = io.wide_offsets ? io.d_image[gp] : load_at<float4>(io.d_image, 16u * gp);   // (an image within 4 GiB: load_at, scene.h)
                if (C.spp_pow2) le_grad = mk3(gi.x * C.inv_spp, gi.y * C.inv_spp, gi.z * C.inv_spp);   // x / 2^k == x * 2^-k exactly: three IEEE divisions (~30 VALU per trip) less
                else { const float fs = (float)C.spp; le_grad = mk3(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs)); }
                if (any_nan(le_grad)) le_grad = mk3(0.0f);
            }
            nrec = 0;
            last = -1;
            alive = true; pix = took;
        }
        if (__ballot(alive) != 0ull) {
            progress = true;
            bool done = false;
            // sweep state: set when a path ends and used up before the trip is over — local to the trip, so that it
            // holds no registers while the vertex is shaded
            f3 term_Li = mk3(0.0f);
            PackedVertex plast;                             // the vertex shaded this trip, as recorded
            plast.a = plast.b = plast.c = plast.d = plast.e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int pmat = 0;                                   // MT: material of plast
            int sw_k = -1;                                  // next vertex the sweep consumes
            bool want_store = false, mute = false;
            SweepState sw; sw.A = mk3(0.0f); sw.Lv = mk3(0.0f); sw.s = 0.0f; sw.Z = 0.0f; sw.tw = 0.0f;
            EnvTerm env_nee, env_miss;                      // EG: this trip's light sample on the environment, continuation ray that missed
            if constexpr (EG) { env_term_clear(env_nee); env_term_clear(env_miss); }
            if (alive) {
                PathVertex pv; float term_plfrac = 0.0f;
                Hit h;
                if (MT) pmat = it.mat;
                if constexpr (EG) done = path_shade<SK, A, true, false, ENV, MT, true>(S, R, C, io, lds, ps, it, pv, h, cnt, &env_nee);
                else if constexpr (LG) {
                    EmitTerm emit_nee;                      // (final when path_shade returns: added at once, nothing of it lives through the next ray)
                    done = path_shade<SK, A, true, false, ENV, MT, false, true>(S, R, C, io, lds, ps, it, pv, h, cnt, nullptr, &emit_nee);
                    emit_add(lds_emit, io, S.light_count, emit_nee, le_grad);
                } else
                done = path_shade<SK, A, true, false, ENV, MT>(S, R, C, io, lds, ps, it, pv, h, cnt);
                plast = pack_vertex(pv, le_grad, R.prb_mode);
                if constexpr (LG) {
                    if (!done) {
                        EmitTerm emit_hit; emit_term_clear(emit_hit);
                        path_continue<A, false>(S, lds, ps, h, cnt);
                        done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, io.mt.inst_slot, nullptr, &emit_hit);
                        emit_add(lds_emit, io, S.light_count, emit_hit, le_grad);
                    }
                } else
                if constexpr (EG) {
                    if (!done) { path_continue<A, false>(S, lds, ps, h, cnt); done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, io.mt.inst_slot, &env_miss); }
                } else
                if (!done) { path_continue<A, false>(S, lds, ps, h, cnt); done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, MT ? io.mt.inst_slot : nullptr); }
                // Only a vertex whose path goes on is put away: when the path ends here (52 % of the vertices) the sweep below starts
                // from plast and nothing would read the record.  (5 LDS or scratch stores per vertex: 16.4 -> 15.5 ms for skipping
                // the vertices that stop at the shading step alone.)
                want_store = !done && ZDR_ABLATE != 3;      // (ablation 3, no sweep: nothing is kept, so no slot leaks)
                nrec++;
                if (done) {
                    alive = false;
                    // a NaN path (prb.py:100: contributes nothing) is swept all the same, muted: the sweep is what returns its slots
                    if (nrec > 0 && ZDR_ABLATE != 3) {
                        mute = any_nan(ps.L);
                        sw_k = nrec - 1;
                        sw.A = le_grad * term_Li; sw.Lv = sw.A; sw.s = 0.0f; sw.Z = 0.0f;
                        sw.tw = (R.prb_mode != ZDR_PRB_EXPECTATION) ? 0.0f : term_plfrac * dot(ps.beta, sw.A);   // emitter hit: d w_bsdf/dr = w_bsdf pl/(pb+pl) dln(pb)/dr
                    }
                }
            }
            // EG, reconverged: both terms are final (a NaN in one is dropped by its push, whatever the rest of the path does: env_push)
            if constexpr (EG) { env_push(q, io, R, env_nee.w * le_grad, env_nee.uv); env_push(q, io, R, env_miss.w * le_grad, env_miss.uv); }
            // Reconverged: hand out slots, all requests of the trip at once.  Home slot first (slot == lane: conflict-free LDS access);
            // the lanes whose home is taken — a path's second and later records, or a home another lane borrowed — are ranked, the free
            // slots are ranked (a lane speaks for slot `lane`, then for slot 64 + lane), and request r takes free slot r: one
            // ds_permute sends every free slot's number to the lane of its rank, one ds_bpermute lets a request read the number at
            // its own rank.  Slots above 63 go first so that homes stay free; no slot left: the record goes to scratch.
            {
                const unsigned long long req = __ballot(want_store);
                int slot = -1;
                if (req != 0ull) {
                    // acquire: the ds_or of the previous trips' sweeps (any lane) are visible to this read
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const zdr_u4 fw = *(volatile const zdr_u4 *)lds_free;       // same address in every lane: a broadcast read
                    unsigned long long free_lo = ((unsigned long long)__builtin_amdgcn_readfirstlane(fw.y) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane(fw.x);
                    unsigned long long free_hi = ((unsigned long long)__builtin_amdgcn_readfirstlane(fw.w) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane(fw.z);
                    const bool home = want_store && lane < NS && ((free_lo >> lane) & 1ull) != 0ull;
                    const unsigned long long took = __ballot(home);
                    free_lo &= ~took;
                    if (home) slot = lane;
                    const unsigned long long rest = req & ~took;
                    if (rest != 0ull && (free_lo | free_hi) != 0ull) {
                        const int nrest = __popcll(rest);
                        const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(rest >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)rest, 0u));   // rank of this lane's request
                        const bool mine = want_store && !home;
                        const int cnt_hi = __popcll(free_hi), cnt_lo = __popcll(free_lo);
                        // free slots 64 + lane
                        const bool fh = ((free_hi >> lane) & 1ull) != 0ull;
                        const int jh = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(free_hi >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)free_hi, 0u));
                        const int at_hi = __builtin_amdgcn_ds_permute((fh ? jh : cnt_hi + (lane - jh)) << 2, lane);   // lane j < cnt_hi now holds the j-th free slot (minus 64)
                        const int pick_hi = __builtin_amdgcn_ds_bpermute(r << 2, at_hi);
                        if (mine && r < cnt_hi) slot = 64 + pick_hi;
                        free_hi &= ~__ballot(fh && jh < nrest);
                        // free slots `lane`, for the requests the upper slots did not serve
                        const int r2 = r - cnt_hi, nrest2 = nrest - cnt_hi;
                        const bool fl = ((free_lo >> lane) & 1ull) != 0ull;
                        const int jl = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(free_lo >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)free_lo, 0u));
                        const int at_lo = __builtin_amdgcn_ds_permute((fl ? jl : cnt_lo + (lane - jl)) << 2, lane);
                        const int pick_lo = __builtin_amdgcn_ds_bpermute((r2 & 63) << 2, at_lo);
                        if (mine && r2 >= 0 && r2 < cnt_lo) slot = pick_lo;
                        free_lo &= ~__ballot(fl && jl < nrest2);
                    }
                    if (lane == 0) {
                        const zdr_u4 nw = {(unsigned int)free_lo, (unsigned int)(free_lo >> 32), (unsigned int)free_hi, (unsigned int)(free_hi >> 32)};
                        *(volatile zdr_u4 *)lds_free = nw;
                    }
                    // release: the new mask is in LDS before any lane's ds_or of the sweep below (in-order LDS, one wave)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                if (want_store) {
                    if (slot >= 0) {
                        float4 *r = lds_pool + slot;
                        r[0] = plast.a; r[NS] = plast.b; r[2 * NS] = plast.c; r[3 * NS] = plast.d; r[4 * NS] = plast.e;
                        lds_link[slot] = MT ? (link_t)((last & 255) | (pmat << 8)) : (link_t)last;
                        last = slot;
                    } else {
                        deep[nrec - 1] = plast; deep_link[nrec - 1] = MT ? ((last & 255) | (pmat << 8)) : last;
                        last = 255;
                    }
                }
            }
            ib.finished(done, pix);
            // wave-uniform: sweep every finished path to its first vertex.  The sweep starts from the vertex packed this
            // trip (still in registers).
            PackedVertex cur = plast;
            int cur_mat = pmat;                             // MT: material of `cur`
            int loc = last;                                 // where the record of the sweep's next step lives
#ifdef ZDR_MEASURE_STATS   // measurement build (tools/bwd_stats.sh): how full are the trips and the sweep iterations
            st_trips++; st_shaded += (unsigned long long)__popcll(__ballot(alive || done));
            st_fin += (unsigned long long)__popcll(__ballot(sw_k >= 0));
#endif
            int sweep_cap = (ZDR_ABLATE == 4) ? 2 : ((ZDR_ABLATE == 5) ? 1 : 64);   // timing-only ablations 4 / 5: the sweep loop cut after 2 / 1 iterations
            // One step consumes `cur`, then fetches the record of the NEXT step into the same registers and only then queues the
            // gradient: the fetch (LDS, or scratch beyond the LDS records) is under way while the push runs, and no record is copied
            // (the loop runs 5.45 times per trip at 18 % of the lanes, profiles/r3_bwd_sweep_ablation.txt; fetching one step ahead
            // into a second register set cost 24 v_mov per iteration, and unrolling by two
            // with the sets swapping roles was slower still: profiles/r3_bwd_sweep_ablation.txt section 3).
            while (__ballot(sw_k >= 0) != 0ull && sweep_cap-- > 0) {
                const bool swp = sw_k >= 0;
#ifdef ZDR_MEASURE_STATS
                st_iters++; st_steps += (unsigned long long)__popcll(__ballot(swp));
#endif
                float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                f2 guv; guv.x = 0.0f; guv.y = 0.0f;
                const int gmat = cur_mat;
                if (swp) { g = sweep_vertex(cur, sw, guv, R.prb_mode); sw_k--; }
                // everything that reads `cur` is finished here, before the fetch below overwrites it (left alone the compiler sinks
                // part of the step below the fetch, loads into a second register set and copies — with a wait in front of the copies)
                asm volatile("" : "+v"(g.x), "+v"(g.y), "+v"(g.z), "+v"(g.w), "+v"(guv.x), "+v"(guv.y), "+v"(sw.A.x), "+v"(sw.A.y), "+v"(sw.A.z),
                             "+v"(sw.Lv.x), "+v"(sw.Lv.y), "+v"(sw.Lv.z), "+v"(sw.s), "+v"(sw.Z), "+v"(sw.tw) : : "memory");
                const bool fetch = swp && sw_k >= 0;
                const bool pooled = fetch && loc != 255;
                int nloc = -1;
                if (pooled) {
                    const float4 *r = lds_pool + loc;
                    cur.a = r[0]; cur.b = r[NS]; cur.c = r[2 * NS]; cur.d = r[3 * NS]; cur.e = r[4 * NS];
                    nloc = (int)lds_link[loc];
                    if (MT) { cur_mat = nloc >> 8; nloc &= 255; }
                }
                // LDS first: both kinds of fetch write the same registers (for different lanes), and the second kind waits for the
                // first to land — an LDS read is back in ~100 cycles, a scratch read in ~500 and behind the flush's atomics
                asm volatile("" ::: "memory");
                if (fetch && loc == 255) {
                    cur = deep[sw_k]; nloc = deep_link[sw_k];
                    if (MT) { cur_mat = nloc >> 8; nloc &= 255; }
                }
                // the slots just read are free again: a wavefront-scope RELEASE or, so the reads of the record above are ordered before it
                // (and this wave's LDS operations execute in order anyway: a later write cannot overtake the read)
                if (pooled) __hip_atomic_fetch_or(&lds_free[loc >> 5], 1u << (loc & 31), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (fetch) loc = nloc;
                scatter_push<MT, EG>(q, io.cells, swp && !mute && any_nonzero4(g) && !any_nan4(g), guv, g, R.tex_h, R.tex_w, ZDR_ABLATE, gmat, io.mt.m);   // prb.py:178-187
            }
        }
#pragma unroll
        for (int b = 0; b < 2; b++)                         // an item whose samples are all generated and whose paths have ended frees its bank
            if (ib.retirable(b, bank, next_sample >= s_end)) ib.set_logical(b, -1);
        if (__ballot(alive) == 0ull && pq.tail == pq.head && next_sample >= s_end && !more_items) break;
        stall = progress ? 0 : stall + 1;
        if (stall > 4) { raise_device_error(S, ZDR_DEVERR_STALL); break; }   // cannot happen (every branch above makes progress); never spin on the GPU, never end silently
    }
    scatter_finish<MT, EG>(q, io.cells, R.tex_h, R.tex_w, ZDR_ABLATE, io.mt.m);
    if constexpr (LG) emit_table_finish(lds_emit, io, S.light_count);
    {   // every path has been swept, so every slot must be back: a leaked or doubly allocated slot is a protocol error, said aloud
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const zdr_u4 fw = *(volatile const zdr_u4 *)lds_free;
        const bool whole = fw.x == (unsigned int)all_lo && fw.y == (unsigned int)(all_lo >> 32) && fw.z == (unsigned int)all_hi && fw.w == (unsigned int)(all_hi >> 32);
        if (!whole && lane == 0 && stall <= 4 && ZDR_ABLATE == 0) raise_device_error(S, ZDR_DEVERR_POOL);
    }
#ifdef ZDR_MEASURE_STATS
    if (lane == 0) {
        atomicAdd(io.counters + 0, st_trips); atomicAdd(io.counters + 1, st_shaded); atomicAdd(io.counters + 2, st_fin);
        atomicAdd(io.counters + 3, st_iters); atomicAdd(io.counters + 4, st_steps);
        atomicAdd(io.counters + 5, q.st_flushes); atomicAdd(io.counters + 6, q.st_entries); atomicAdd(io.counters + 7, q.st_dups);
    }
#endif
#undef S
#undef R
#undef C
#undef io
}

// ---------------------------------------------------------------------- direct / collocated
// EG (direct backward only; implies ENV and MT): the terms that read the environment map are queued too (direct_sample, EnvTerm)
// LG (direct backward only; implies MT, never with EG): the terms that read a light's emission (direct_sample, EmitTerm) are added to the
// wave's emission table as they happen
template <int INTEG, int SK, class A, bool BWD, bool STATS, bool ENV, bool MT, bool EG = false, bool LG = false>
#ifndef ZDR_MIN_WAVES_DIRECT
#define ZDR_MIN_WAVES_DIRECT 4   // brute-force direct kernels, cbox 512^2 spp 64: 153 VGPRs (3 waves per SIMD) 1.175 / 1.331 ms, 128 VGPRs (6 spilled) 1.110 / 1.267 ms
#endif
// (the environment instantiations take 170 VGPRs: bounded to 3 waves per SIMD, which costs no spill, instead of the 2 the compiler settles for)
__global__ __launch_bounds__(WAVE, (INTEG == ZDR_DIRECT && !A::kNeedsLds) ? (ENV ? 3 : ZDR_MIN_WAVES_DIRECT) : 1) void k_simple(ZDR_PATH_KERNEL_PARAMS) {
    static_assert(!LG || (INTEG == ZDR_DIRECT && BWD && !STATS && MT && !EG), "the emission gradient runs in the direct backward material-table kernels, without the environment gradient");
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    __shared__ __attribute__((aligned(16))) float lds_q[BWD ? ZDR_SCATTER_LDS_FLOATS : 4];
    float *lds_emit = nullptr;                              // LG: the wave's emission table (emit_add)
    if constexpr (LG) { __shared__ float lds_emit_table[3 * ZDR_EMIT_LDS_LIGHTS]; lds_emit = lds_emit_table; }
    const WorkItem w = decode_block(R);
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
    Counters cnt;
#pragma unroll
    for (int i = 0; i < 8; i++) cnt.c[i] = 0;
    f3 le_grad = mk3(0.0f);
    if (BWD) le_grad = load_le_grad(C, io, w);
    ScatterQueue q = MT ? scatter_queue_init_cells(lds_q, io.mt.ncells, R.cell_copies) : scatter_queue_init(lds_q, R.tex_h, R.tex_w, R.cell_copies);
    if constexpr (EG) q.lds_cells = nullptr;                // the map's cells are never in LDS (table_cell_env)
    if constexpr (LG) emit_table_init(lds_emit);
    const unsigned long long cam_mask = camera_mask(S, io, w);
    f3 sum = mk3(0.0f);
    for (uint32_t it = w.s_begin; it < w.s_end; it++) {     // integrator.py:15 (wave-uniform trip count)
        ZDR_KARGS_REFRESH
        float4 grad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        f2 guv; guv.x = 0.0f; guv.y = 0.0f;
        int gmat = 0;
        EnvTerm e_cam, e_bsdf;
        env_term_clear(e_cam); env_term_clear(e_bsdf);
        if (w.valid) {
            Sampler smp = sampler_make<SK>(C, (uint32_t)w.x, (uint32_t)w.y, perm_seed, it);
            f3 o, d;
            pixel_ray<SK, true>(R, C, smp, w.x, w.y, o, d);
            COUNT(C_SAMPLES);
            f3 rad;
            if constexpr (LG) {   // (the terms live inside this branch only: declared beside e_cam they changed the EG kernels' registers)
                EmitTerm l_cam, l_bsdf;
                emit_term_clear(l_cam); emit_term_clear(l_bsdf);
                rad = direct_sample<SK, A, true, false, ENV, true, false, true>(S, R, C, io, lds, smp, o, d, cam_mask, le_grad, cnt, guv, grad, gmat, nullptr, nullptr, &l_cam, &l_bsdf);
                emit_add(lds_emit, io, S.light_count, l_cam, le_grad); emit_add(lds_emit, io, S.light_count, l_bsdf, le_grad);
            } else
            if (INTEG == ZDR_COLLOCATED) rad = collocated_sample<A, BWD, STATS, MT>(S, R, io, lds, o, d, cam_mask, le_grad, cnt, guv, grad, gmat);
            else rad = direct_sample<SK, A, BWD, STATS, ENV, MT, EG>(S, R, C, io, lds, smp, o, d, cam_mask, le_grad, cnt, guv, grad, gmat,
                                                                      EG ? &e_cam : nullptr, EG ? &e_bsdf : nullptr);
            if (!any_nan(rad)) sum = sum + clamp_radiance(rad); else COUNT(C_NAN);
        }
        if (BWD) scatter_push<MT, EG>(q, io.cells, w.valid && any_nonzero4(grad) && !any_nan4(grad), guv, grad, R.tex_h, R.tex_w, ZDR_ABLATE, gmat, io.mt.m);
        if constexpr (EG) { env_push(q, io, R, e_cam.w * le_grad, e_cam.uv); env_push(q, io, R, e_bsdf.w * le_grad, e_bsdf.uv); }
    }
    if (BWD) scatter_finish<MT, EG>(q, io.cells, R.tex_h, R.tex_w, ZDR_ABLATE, io.mt.m);
    if constexpr (LG) emit_table_finish(lds_emit, io, S.light_count);
    if (!BWD && !STATS) store_pixel(R, C, io, w, sum);
    flush_counters<STATS>(io, cnt);
#undef S
#undef R
#undef C
#undef io
}

// Folds the staging cells into the gradient texture: texel (x, y) receives corner (dx, dy) of every
// cell (ix, iy) with clamp(ix + dx) == x and clamp(iy + dy) == y — the adjoint of read_bsdf's CLAMP
// bilinear lookup (interaction.py:47-60, 73-89).  Deterministic summation order.
__global__ void k_cells_to_grad(const float4 *__restrict__ cells, float4 *__restrict__ dmat, int tex_h, int tex_w, int copies) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= tex_w) return;
    int ixs[3], dxs[3], nx = 0, iys[3], dys[3], ny = 0;
    ixs[nx] = x - 1; dxs[nx++] = 1; ixs[nx] = x; dxs[nx++] = 0;
    if (x == 0) { ixs[nx] = -1; dxs[nx++] = 0; }
    if (x == tex_w - 1) { ixs[nx] = tex_w - 1; dxs[nx++] = 1; }
    iys[ny] = y - 1; dys[ny++] = 1; iys[ny] = y; dys[ny++] = 0;
    if (y == 0) { iys[ny] = -1; dys[ny++] = 0; }
    if (y == tex_h - 1) { iys[ny] = tex_h - 1; dys[ny++] = 1; }
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const size_t ncells = (size_t)(tex_h + 1) * (tex_w + 1);
    if (copies == 1) {
        for (int b = 0; b < ny; b++)
            for (int a = 0; a < nx; a++) {
                size_t cell = (size_t)(ixs[a] + 1) + (size_t)(tex_w + 1) * (iys[b] + 1);
                float4 c = cells[4 * cell + 2 * dxs[a] + dys[b]];
                acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += c.w;
            }
    } else {   // few texels: the waves added into `copies` replicas of the cell array (scene.h); sum them in float64
        double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
        for (int k = 0; k < copies; k++)
            for (int b = 0; b < ny; b++)
                for (int a = 0; a < nx; a++) {
                    size_t cell = (size_t)k * ncells + (size_t)(ixs[a] + 1) + (size_t)(tex_w + 1) * (iys[b] + 1);
                    float4 c = cells[4 * cell + 2 * dxs[a] + dys[b]];
                    sx += c.x; sy += c.y; sz += c.z; sw += c.w;
                }
        acc = make_float4((float)sx, (float)sy, (float)sz, (float)sw);
    }
    float4 d = dmat[(size_t)x + (size_t)tex_w * y];
    dmat[(size_t)x + (size_t)tex_w * y] = make_float4(d.x + acc.x, d.y + acc.y, d.z + acc.z, d.w + acc.w);
}
// The same for every material of a material-table call in one launch (blockIdx.z = material): material k's range of the packed
// gradient receives what its copies of the cells hold (+=).
__global__ void k_material_cells_to_grad(const float4 *__restrict__ cells, float4 *__restrict__ dmat, MaterialTable mt) {
    const MaterialSlot m = mt.m[blockIdx.z];
    const int copies = m.copies;
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= m.w || y >= m.h) return;
    const int tex_h = m.h, tex_w = m.w;
    int ixs[3], dxs[3], nx = 0, iys[3], dys[3], ny = 0;         // (the footprint of k_cells_to_grad)
    ixs[nx] = x - 1; dxs[nx++] = 1; ixs[nx] = x; dxs[nx++] = 0;
    if (x == 0) { ixs[nx] = -1; dxs[nx++] = 0; }
    if (x == tex_w - 1) { ixs[nx] = tex_w - 1; dxs[nx++] = 1; }
    iys[ny] = y - 1; dys[ny++] = 1; iys[ny] = y; dys[ny++] = 0;
    if (y == 0) { iys[ny] = -1; dys[ny++] = 0; }
    if (y == tex_h - 1) { iys[ny] = tex_h - 1; dys[ny++] = 1; }
    double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;              // (float64 for the copies, float32 order otherwise, as k_cells_to_grad)
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < copies; k++)
        for (int b = 0; b < ny; b++)
            for (int a = 0; a < nx; a++) {
                const size_t cell = (size_t)k * m.stride + (size_t)m.cell + (size_t)(ixs[a] + 1) + (size_t)(tex_w + 1) * (iys[b] + 1);
                const float4 c = cells[4 * cell + 2 * dxs[a] + dys[b]];
                if (copies == 1) { acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += c.w; }
                else { sx += c.x; sy += c.y; sz += c.z; sw += c.w; }
            }
    if (copies > 1) acc = make_float4((float)sx, (float)sy, (float)sz, (float)sw);
    float4 *t = dmat + (size_t)m.texel + (size_t)x + (size_t)m.w * y;
    const float4 d = *t;
    *t = make_float4(d.x + acc.x, d.y + acc.y, d.z + acc.z, d.w + acc.w);
}

// render_duvdxy (uvgrad.py:76-98): mean over the samples of the screen->texture Jacobian, NaNs dropped
template <int SK, class A>
__global__ __launch_bounds__(WAVE) void k_uvgrad(DScene S, RenderCfg R, SamplerCfg C, KernelIO io) {
    extern __shared__ int lds[];
    const WorkItem w = decode_block(R);
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t it = w.s_begin; it < w.s_end; it++) {
        if (!w.valid) continue;
        Sampler smp = sampler_make<SK>(C, (uint32_t)w.x, (uint32_t)w.y, perm_seed, it);
        f2 off = sampler_next2<SK>(C, smp);
        if (R.use_tent) { off.x = tent_warp1(off.x) + 0.5f; off.y = tent_warp1(off.y) + 0.5f; }
        const float fx = (float)w.x + off.x, fy = (float)w.y + off.y;
        f3 o = ld3(R.cam_o), d[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {          // rays through (x, y), (x + 1, y), (x, y + 1)
            float px = R.two_over_w * (fx + (k == 1 ? 1.0f : 0.0f)) - 1.0f;
            float py = (R.two_over_h * (fy + (k == 2 ? 1.0f : 0.0f)) - 1.0f) * R.aspect;
            d[k] = normalize((ld3(R.cam_right) * (px * R.cam_tan) - ld3(R.cam_upp) * (py * R.cam_tan)) + ld3(R.cam_fwd));
        }
        float4 g = uvgrad_sample<A>(S, lds, o, d[0], o, d[1], o, d[2]);
        if (!any_nan4(g)) { sum.x += g.x; sum.y += g.y; sum.z += g.z; sum.w += g.w; }
    }
    if (w.valid) {
        float fs = (float)C.spp;
        io.image[w.pix] = make_float4(__fdiv_rn(sum.x, fs), __fdiv_rn(sum.y, fs), __fdiv_rn(sum.z, fs), __fdiv_rn(sum.w, fs));
    }
}

// ----------------------------------------------------------------------- feature buffers
// zdr_render_aovs (include/zdr.h has the channel table): one wave per 8x8 tile, lane = pixel, every sample of the pixel in index order
// (the launcher gives these kernels one chunk: the instance channel has no partial form).  A lane keeps its pixel's sixteen sums in
// registers and writes its own 64-byte line once, as four dwordx4 stores.  Material-table form only; the launch constants are read
// through the laundered kernarg pointer like k_simple's, so that the table and the camera stay in the kernarg segment and in SGPRs.
template <int SK, class A>
__global__ __launch_bounds__(WAVE) void k_aov(ZDR_PATH_KERNEL_PARAMS) {
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    const WorkItem w = decode_block(R);
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
    const unsigned long long cam_mask = camera_mask(S, io, w);
    float4 mat = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nrm = mat, pos = mat;   // {albedo, roughness} {normal, depth} {position, hits}
    f2 uv; uv.x = 0.0f; uv.y = 0.0f;
    float first_inst = -1.0f, first_slot = -1.0f;
    bool seen = false;
    for (uint32_t it = w.s_begin; it < w.s_end; it++) {     // wave-uniform trip count
        ZDR_KARGS_REFRESH
        if (!w.valid) continue;
        const AovSample a = aov_sample<SK, A>(S, R, C, io, lds, w.x, w.y, perm_seed, it, cam_mask);
        if (!a.hit) continue;
        float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (a.slot >= 0) m = read_bsdf_in(io.material, io.mt.m[a.slot], a.uv, io.wide_offsets != 0);
        if (aov_geometry_nan(a) || any_nan4(m)) continue;
        mat.x += m.x; mat.y += m.y; mat.z += m.z; mat.w += m.w;
        nrm.x += a.ns.x; nrm.y += a.ns.y; nrm.z += a.ns.z; nrm.w += a.t;
        pos.x += a.p.x; pos.y += a.p.y; pos.z += a.p.z; pos.w += 1.0f;
        uv.x += a.uv.x; uv.y += a.uv.y;
        if (!seen) { seen = true; first_inst = (float)a.inst; first_slot = (float)a.slot; }
    }
    if (w.valid) {
        const float fs = (float)C.spp;
        float4 *o = io.image + 4 * (size_t)w.pix;
        o[0] = make_float4(__fdiv_rn(mat.x, fs), __fdiv_rn(mat.y, fs), __fdiv_rn(mat.z, fs), __fdiv_rn(mat.w, fs));
        o[1] = make_float4(__fdiv_rn(nrm.x, fs), __fdiv_rn(nrm.y, fs), __fdiv_rn(nrm.z, fs), __fdiv_rn(nrm.w, fs));
        o[2] = make_float4(__fdiv_rn(pos.x, fs), __fdiv_rn(pos.y, fs), __fdiv_rn(pos.z, fs), __fdiv_rn(pos.w, fs));
        o[3] = make_float4(__fdiv_rn(uv.x, fs), __fdiv_rn(uv.y, fs), first_inst, first_slot);
    }
#undef S
#undef R
#undef C
#undef io
}

// zdr_render_aovs_backward: the transpose of the albedo / roughness channels.  Same samples, same hits; a sample whose instance has a
// material queues (uv, cotangent of floats 0..3 / spp, slot) into the scatter queue of the backward kernels (scene.h), once per
// sample iteration by the whole wave; cells, copies and the few-texel LDS path are those of every material-table backward call, and
// k_material_cells_to_grad gathers them.  The cotangent is read once per pixel, outside the loop.
template <int SK, class A>
__global__ __launch_bounds__(WAVE) void k_aov_bwd(ZDR_PATH_KERNEL_PARAMS) {
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    __shared__ __attribute__((aligned(16))) float lds_q[ZDR_SCATTER_LDS_FLOATS];
    const WorkItem w = decode_block(R);
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
    const unsigned long long cam_mask = camera_mask(S, io, w);
    float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (w.valid) {
        const float4 gi = io.d_image[4 * (size_t)w.pix];
        const float fs = (float)C.spp;
        g = make_float4(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs), __fdiv_rn(gi.w, fs));
        if (any_nan4(g)) g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const bool carries = any_nonzero4(g);
    ScatterQueue q = scatter_queue_init_cells(lds_q, io.mt.ncells, R.cell_copies);
    for (uint32_t it = w.s_begin; it < w.s_end; it++) {     // wave-uniform trip count
        ZDR_KARGS_REFRESH
        bool push = false;
        f2 guv; guv.x = 0.0f; guv.y = 0.0f;
        int gmat = 0;
        if (w.valid) {
            const AovSample a = aov_sample<SK, A>(S, R, C, io, lds, w.x, w.y, perm_seed, it, cam_mask);
            if (a.hit && a.slot >= 0 && !aov_geometry_nan(a)) { push = carries; guv = a.uv; gmat = a.slot; }
        }
        scatter_push<true, false>(q, io.cells, push, guv, g, R.tex_h, R.tex_w, 0, gmat, io.mt.m);
    }
    scatter_finish<true, false>(q, io.cells, R.tex_h, R.tex_w, 0, io.mt.m);
#undef S
#undef R
#undef C
#undef io
}

// sums the per-chunk partial images in chunk order (deterministic), integrator.py:29
__global__ void k_reduce_chunks(RenderCfg R, uint32_t spp, const float4 *partial, float4 *image) {
    int x = R.x0 + blockIdx.x * blockDim.x + threadIdx.x, y = R.y0 + blockIdx.y;
    if (x >= R.x1 || y >= R.y1) return;
    const size_t pix = (size_t)x + (size_t)y * R.width;
    const int lx = x - R.x0, ly = y - R.y0, ty = ly >> 3;
    int c = (lx >> 3) - (ty * R.shard_skew) % R.tiles_x;     // the tile's number in its row (decode_item)
    if (c < 0) c += R.tiles_x;
    const int tile = ty * R.tiles_x + c;
    if (tile % R.shard_count != R.shard_index) return;      // another shard's pixel: untouched
    const size_t slot = (size_t)(tile / R.shard_count) * 64 + (size_t)((ly & 7) * 8 + (lx & 7));
    f3 s = mk3(0.0f);
    for (int c = 0; c < R.nchunks; c++) { float4 p = partial[(size_t)c * R.ntiles * 64 + slot]; s = s + mk3(p.x, p.y, p.z); }
    float fs = (float)spp;
    image[pix] = make_float4(__fdiv_rn(s.x, fs), __fdiv_rn(s.y, fs), __fdiv_rn(s.z, fs), R.alpha);
}

// Zero-fill of the per-call workspaces (staging cells, work counters) by a KERNEL, not hipMemsetAsync: captured in a HIP graph, the
// runtime's memset node of the 64 MiB cell array was observed to run out of order with the kernels around it from the second replay on
// (the gradient came back zero); a kernel node is ordered like every other launch.  n16 = number of 16-byte words.
__global__ void k_zero(uint4 *__restrict__ p, size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
int zdr_launch_zero(void *p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return 0;
    const size_t n16 = (bytes + 15) / 16;                    // every workspace is allocated in multiples of 16 bytes
    const unsigned blocks = (unsigned)std::min<size_t>((n16 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_zero, dim3(blocks), dim3(256), 0, st, (uint4 *)p, n16);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

__global__ void k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}
int zdr_launch_copy(void *dst, const void *src, size_t bytes, hipStream_t st) {   // bytes: a multiple of 16 (float4 texels)
    if (bytes == 0) return 0;
    const size_t n16 = bytes / 16;
    const unsigned blocks = (unsigned)std::min<size_t>((n16 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_copy16, dim3(blocks), dim3(256), 0, st, (uint4 *)dst, (const uint4 *)src, n16);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ----------------------------------------------------------------------------------- launch
// dynamic LDS of a wave that traverses the BVH: the first entries of the per-lane stacks (accel.h).  Sets S.lds_stack.
// path_kernels: the launch runs BvhAccel::shadow_and_closest (k_path, k_path_bwd, k_path_dump), whose walk_steal keeps 5 x 64 ints behind the stack.
static size_t bvh_dyn_lds(DScene &S, bool backward, bool path_kernels) {
    S.lds_stack = std::min<int>(S.stack_entries, backward ? ZDR_BVH_LDS_STACK_BWD : ZDR_BVH_LDS_STACK);
    return (size_t)S.lds_stack * WAVE * sizeof(int) + ((ZDR_BVH_STEAL && path_kernels) ? 5 * WAVE * sizeof(int) : 0);
}
// Persistent grid of the path kernels: as many single-wave workgroups as the chip holds at once (never more
// than there are items).  A workgroup that is not resident at first simply starts later and draws what is left.
#define ZDR_LDS_BLOCK_BYTES 1280
#define ZDR_LDS_BLOCKS_PER_CU 128
template <class K>
static dim3 persistent_grid(K kernel, size_t dyn, int nitems) {
    int per_cu = 0, dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    {   // the occupancy query costs tens of microseconds: remember it per (kernel, dynamic LDS, device)
        static std::mutex mu;
        static std::map<std::tuple<const void *, size_t, int>, std::pair<int, int>> cache;
        std::lock_guard<std::mutex> lock(mu);
        auto key = std::make_tuple((const void *)kernel, dyn, dev);
        auto it = cache.find(key);
        if (it == cache.end()) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WAVE, dyn) != hipSuccess || per_cu < 1) per_cu = 8;
            // gfx950 hands out its 160 KiB of LDS in 128 blocks of 1,280 bytes and the query above does not round up: with 13,264
            // bytes per wave it answered 12, 11 were resident, and the twelfth wave of every CU started when the launch was over
            // (profiles/r3_bwd_records_and_atomics.txt).  A persistent grid must not be larger than what is resident at once.
            hipFuncAttributes fa;
            if (hipFuncGetAttributes(&fa, (const void *)kernel) == hipSuccess) {
                const size_t blocks = (fa.sharedSizeBytes + dyn + ZDR_LDS_BLOCK_BYTES - 1) / ZDR_LDS_BLOCK_BYTES;
                if (blocks > 0) per_cu = std::max(1, std::min<int>(per_cu, (int)(ZDR_LDS_BLOCKS_PER_CU / blocks)));
            }
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
            it = cache.emplace(key, std::make_pair(per_cu, cus)).first;
        }
        per_cu = it->second.first; cus = it->second.second;
    }
    if (const char *e = getenv("ZDR_PERSISTENT_WAVES_PER_CU")) per_cu = std::max(1, atoi(e));
    long g = std::min<long>((long)per_cu * cus, (long)ZDR_MAX_PERSISTENT_BLOCKS);
    return dim3((unsigned)std::max<long>(1, std::min<long>(g, nitems)));
}

// Run-time values that choose a template instantiation, each choice written once: f receives the value as a type.
template <class A> struct AccelTag { typedef A type; };
template <class F> static void with_bool(bool b, F &&f) { if (b) f(std::true_type()); else f(std::false_type()); }
template <class F> static void with_accel(int accel_is_bvh, F &&f) { if (accel_is_bvh) f(AccelTag<BvhAccel>()); else f(AccelTag<BruteAccel>()); }
// f(sampler as std::integral_constant<int, SK> (0: cmj, 1: pmj02bn), AccelTag<A>)
template <class F> static void with_sampler_accel(int sampler_kind, int accel_is_bvh, F &&f) {
    with_accel(accel_is_bvh, [&](auto acc) {
        if (sampler_kind == ZDR_SAMPLER_CMJ) f(std::integral_constant<int, 0>(), acc); else f(std::integral_constant<int, 1>(), acc);
    });
}

// The form of its integrator's kernel a call runs.  mt: material-table mode (io.mt.nmat > 0); eg / lg: the environment / emission gradient
// of a backward call.  Only the forms the launchers below name are compiled (each costs about a minute of build time): there is no
// statistics kernel in material-table mode (zdr_render_stats takes one material), eg exists with env && mt only, lg with mt && !eg only.
// A launcher that is asked for a gradient form that does not exist launches nothing and returns false: gradient_form_exists states
// the rule for the run-time values, the `if constexpr` guards in the launchers keep the same forms from being instantiated.  A new
// gradient target changes both together.
struct KernelForm { bool backward, stats, env, mt, eg, lg; };
static bool gradient_form_exists(const KernelForm &k) {
    if (!k.eg && !k.lg) return true;
    return k.backward && k.mt && !(k.eg && k.lg) && (!k.eg || k.env);
}

// persistent path kernels
template <int SK, class A>
static bool launch_path(const KernelForm &k, int nitems, size_t dyn, hipStream_t st, const DScene &S, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io) {
    if (!gradient_form_exists(k)) return false;
    auto go = [&](auto K) { hipLaunchKernelGGL(K, persistent_grid(K, dyn, nitems), dim3(WAVE), dyn, st, S, R, C, io); };
    // the environment-light code is a separate instantiation: inside the default kernels it cost 16 % (cbox forward)
    with_bool(k.env, [&](auto env) {
        constexpr bool ENV = decltype(env)::value;
        if (!k.backward) {
            if (k.mt) go(k_path<SK, A, false, ENV, true>);
            else if (k.stats) go(k_path<SK, A, true, ENV, false>);
            else go(k_path<SK, A, false, ENV, false>);
        } else if (k.eg) { if constexpr (ENV) go(k_path_bwd<SK, A, true, true, true>); }
        else if (k.lg) go(k_path_bwd<SK, A, ENV, true, false, true>);
        else if (k.mt) go(k_path_bwd<SK, A, ENV, true>);
        else go(k_path_bwd<SK, A, ENV, false>);
    });
    return true;
}

// one workgroup per item: direct and collocated (which sees no environment and has neither eg nor lg; its env forms are compiled all
// the same, as they always were, and never launched)
template <int INTEG, int SK, class A>
static bool launch_simple(const KernelForm &k, dim3 grid, size_t dyn, hipStream_t st, const DScene &S, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io) {
    if (!gradient_form_exists(k) || ((k.eg || k.lg) && INTEG != ZDR_DIRECT)) return false;
    auto go = [&](auto K) { hipLaunchKernelGGL(K, grid, dim3(WAVE), dyn, st, S, R, C, io); };
    constexpr bool DIRECT = INTEG == ZDR_DIRECT;
    with_bool(DIRECT && k.env, [&](auto env) {
        constexpr bool ENV = decltype(env)::value;
        if (!k.backward) {
            if (k.mt) go(k_simple<INTEG, SK, A, false, false, ENV, true>);
            else if (k.stats) go(k_simple<INTEG, SK, A, false, true, ENV, false>);
            else go(k_simple<INTEG, SK, A, false, false, ENV, false>);
        } else if (k.eg) { if constexpr (DIRECT && ENV) go(k_simple<INTEG, SK, A, true, false, true, true, true>); }
        else if (k.lg) { if constexpr (DIRECT) go(k_simple<INTEG, SK, A, true, false, ENV, true, false, true>); }
        else if (k.mt) go(k_simple<INTEG, SK, A, true, false, ENV, true>);
        else go(k_simple<INTEG, SK, A, true, false, ENV, false>);
    });
    return true;
}

// What a backward call launches behind its kernel: the staging cells into the gradient buffers (+=).  io.mt.nmat > 0: a material-table
// call, d_env its map's gradient or NULL; else the single material of R.tex_h x R.tex_w.  (zdr_launch_render and the test hook
// zdr_launch_texture_scatter.)
static void launch_cells_fold(const RenderCfg &R, const KernelIO &io, float *d_env, hipStream_t st) {
    if (io.mt.nmat > 0) {   // every material's cells into its range of d_material (+=)
        int mh = 1, mw = 1;
        for (int k = 0; k < io.mt.nmat; k++) { mh = std::max(mh, (int)io.mt.m[k].h); mw = std::max(mw, (int)io.mt.m[k].w); }
        dim3 g((mw + 63) / 64, mh, io.mt.nmat);
        hipLaunchKernelGGL(k_material_cells_to_grad, g, dim3(64), 0, st, (const float4 *)io.cells, (float4 *)io.d_material, io.mt);
        if (d_env) {   // the map's cells into d_env (+=): the same gather, a table whose only material is the map, with the map's own copies
            const MaterialSlot e = io.mt.m[ZDR_ENV_ENTRY];    // {copies, h, w, first cell}
            MaterialTable me = io.mt;
            me.m[0] = e; me.m[0].texel = 0;
            me.m[0].copies = e.texel; me.m[0].stride = (e.h + 1) * (e.w + 1);
            dim3 ge((e.w + 63) / 64, e.h, 1);
            hipLaunchKernelGGL(k_material_cells_to_grad, ge, dim3(64), 0, st, (const float4 *)io.cells, (float4 *)d_env, me);
        }
    } else {   // fold the staging cells into d_material (+=)
        dim3 g((R.tex_w + 63) / 64, R.tex_h);
        hipLaunchKernelGGL(k_cells_to_grad, g, dim3(64), 0, st, (const float4 *)io.cells, (float4 *)io.d_material, R.tex_h, R.tex_w, R.cell_copies);
    }
}

int zdr_launch_render(const DScene &S_in, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io, const RenderLaunch &L, hipStream_t st) {
    DScene S = S_in;
    const int integrator = L.integrator, backward = L.backward, stats = L.stats;
    float *const d_env = L.d_env, *const d_emission = L.d_emission;
    int nblocks = R.ntiles * R.nchunks;
    if (nblocks <= 0) return 0;
    dim3 grid(((nblocks + 7) >> 3) << 3);                   // multiple of 8 for the XCD remap
    const size_t dyn = L.accel_is_bvh ? bvh_dyn_lds(S, backward != 0, integrator == ZDR_PATH && !L.aov) : 0;
    if (io.tile_masks && !io.tile_masks_valid)
        hipLaunchKernelGGL(k_tile_masks, dim3(R.tiles_x * R.tiles_y), dim3(WAVE), 0, st, S, R, (unsigned long long *)io.tile_masks);
    const KernelForm k = {backward != 0, stats != 0, S.env_count > 0, io.mt.nmat > 0, d_env != nullptr, d_emission != nullptr};
    bool launched = true;
    with_sampler_accel(C.kind, L.accel_is_bvh, [&](auto sk, auto acc) {
        constexpr int SK = decltype(sk)::value;
        typedef typename decltype(acc)::type A;
        if (L.aov && backward) hipLaunchKernelGGL((k_aov_bwd<SK, A>), grid, dim3(WAVE), dyn, st, S, R, C, io);
        else if (L.aov) hipLaunchKernelGGL((k_aov<SK, A>), grid, dim3(WAVE), dyn, st, S, R, C, io);
        else if (integrator == ZDR_UVGRAD) hipLaunchKernelGGL((k_uvgrad<SK, A>), grid, dim3(WAVE), dyn, st, S, R, C, io);
        else if (integrator == ZDR_PATH) launched = launch_path<SK, A>(k, nblocks, dyn, st, S, R, C, io);
        else if (integrator == ZDR_DIRECT) launched = launch_simple<ZDR_DIRECT, SK, A>(k, grid, dyn, st, S, R, C, io);
        else launched = launch_simple<ZDR_COLLOCATED, SK, A>(k, grid, dyn, st, S, R, C, io);
    });
    if (!launched) return -1;   // no kernel of that form: nothing wrote the cells, so nothing is gathered
    if (backward) {
        launch_cells_fold(R, io, d_env, st);
        if (io.mt.nmat > 0 && d_emission)      // the accumulator's rows into d_emission (+=), each light into its instance's row
            hipLaunchKernelGGL(k_emission_gather, dim3((3 * S.light_count + 63) / 64), dim3(64), 0, st, (const float *)io.emit_acc, ZDR_EMISSION_COPIES, S.light_count, S.light_insts, d_emission);
    }
    if (!backward && !stats && R.nchunks > 1) {
        dim3 g((R.x1 - R.x0 + 63) / 64, R.y1 - R.y0);
        hipLaunchKernelGGL(k_reduce_chunks, g, dim3(64), 0, st, R, C.spp, (const float4 *)io.partial, io.image);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------- ray batch queries
template <class A, bool ANY>
__global__ __launch_bounds__(WAVE) void k_trace(DScene S, const float4 *rays, uint32_t n, int32_t *out_i, float *out_f) {
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    bool valid = i < n;
    float4 a = valid ? rays[2 * (size_t)i] : make_float4(0, 0, 0, 0), b = valid ? rays[2 * (size_t)i + 1] : make_float4(0, 0, 1, 0);
    if (ANY) {
        bool occ = A::any(S, lds, xyz(a), xyz(b), a.w, b.w);
        if (valid) out_i[i] = occ ? 1 : 0;
    } else {
        Hit h = A::closest(S, lds, xyz(a), xyz(b), a.w, b.w);
        if (valid) {
            int inst = -1, prim = -1;
            if (h.slot >= 0) { inst = __float_as_int(S.shade[8 * (size_t)h.slot + 6].w); prim = __float_as_int(S.shade[8 * (size_t)h.slot + 7].y); }
            out_i[2 * (size_t)i] = inst; out_i[2 * (size_t)i + 1] = prim;
            float hu = h.u, hv = h.v;
            if (h.slot >= 0) {   // the slot's corners may be a rotation of the input triangle's (quads, zdr_api.cpp): report the barycentrics of the INPUT corners 1 and 2
                const int ro = __float_as_int(S.shade[8 * (size_t)h.slot + 7].z);
                const float hw = 1.0f - h.u - h.v;
                if (ro == 1) { hu = hw; hv = h.u; } else if (ro == 2) { hu = h.v; hv = hw; }
            }
            out_f[3 * (size_t)i] = hu; out_f[3 * (size_t)i + 1] = hv; out_f[3 * (size_t)i + 2] = (h.slot >= 0) ? h.t : b.w;
        }
    }
}

int zdr_launch_trace(const DScene &S_in, int accel_is_bvh, int any, const float *rays, uint32_t n, int32_t *out_i, float *out_f, hipStream_t st) {
    DScene S = S_in;
    if (n == 0) return 0;
    dim3 grid((n + WAVE - 1) / WAVE);
    const float4 *r = (const float4 *)rays;
    const size_t dyn = accel_is_bvh ? bvh_dyn_lds(S, false, false) : 0;
    with_accel(accel_is_bvh, [&](auto acc) {
        typedef typename decltype(acc)::type A;
        if (any) hipLaunchKernelGGL((k_trace<A, true>), grid, dim3(WAVE), dyn, st, S, r, n, out_i, out_f);
        else hipLaunchKernelGGL((k_trace<A, false>), grid, dim3(WAVE), dyn, st, S, r, n, out_i, out_f);
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------ fused walk
// Test hook (zdr_trace_fused, include/zdr.h): lane i of wave i / 64 is ray pair i and hands BvhAccel::shadow_and_closest its two rays
// exactly as path_shade does, under the LDS layout of the path kernels (bvh_dyn_lds: the stack of either layout + the cells of
// walk_steal).  Every lane of a wave takes part, the ones beyond n with no ray.  This is walk_steal compiled into a kernel of its
// own: it runs the routine's logic, not the instance inlined into k_path / k_path_bwd (the path parity tests run those).
template <class A>
__global__ __launch_bounds__(WAVE) void k_trace_fused(DScene S, const float4 *shadow, const float4 *next, const int32_t *need, uint32_t n,
                                                      int32_t *occluded, int32_t *out_i, float *out_f) {
    extern __shared__ int lds[];
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    const bool valid = i < n;
    const int nd = valid ? need[i] : 0;
    const float4 sa = valid ? shadow[2 * (size_t)i] : make_float4(0, 0, 0, 0), sb = valid ? shadow[2 * (size_t)i + 1] : make_float4(0, 0, 1, 0);
    const float4 na = valid ? next[2 * (size_t)i] : make_float4(0, 0, 0, 0), nb = valid ? next[2 * (size_t)i + 1] : make_float4(0, 0, 1, 0);
    bool occ; Hit h;
    A::shadow_and_closest(S, lds, (nd & 1) != 0, xyz(sa), xyz(sb), sa.w, sb.w, (nd & 2) != 0, xyz(na), xyz(nb), occ, h);
    if (!valid) return;
    occluded[i] = ((nd & 1) && occ) ? 1 : 0;
    const bool hit = (nd & 2) && h.slot >= 0;
    int inst = -1, prim = -1;
    float hu = 0.0f, hv = 0.0f;
    if (hit) {                          // as k_trace reports them: the barycentrics of the INPUT corners 1 and 2
        inst = __float_as_int(S.shade[8 * (size_t)h.slot + 6].w); prim = __float_as_int(S.shade[8 * (size_t)h.slot + 7].y);
        const int ro = __float_as_int(S.shade[8 * (size_t)h.slot + 7].z);
        const float hw = 1.0f - h.u - h.v;
        hu = h.u; hv = h.v;
        if (ro == 1) { hu = hw; hv = h.u; } else if (ro == 2) { hu = h.v; hv = hw; }
    }
    out_i[2 * (size_t)i] = inst; out_i[2 * (size_t)i + 1] = prim;
    out_f[3 * (size_t)i] = hu; out_f[3 * (size_t)i + 1] = hv; out_f[3 * (size_t)i + 2] = hit ? h.t : 1e30f;
}

int zdr_launch_trace_fused(const DScene &S_in, const float *shadow, const float *next, const int32_t *need, uint32_t n, int backward_layout,
                           int32_t *occluded, int32_t *out_i, float *out_f, hipStream_t st) {
    DScene S = S_in;
    if (n == 0) return 0;
    dim3 grid((n + WAVE - 1) / WAVE);
    const size_t dyn = bvh_dyn_lds(S, backward_layout != 0, true);
    hipLaunchKernelGGL((k_trace_fused<BvhAccel>), grid, dim3(WAVE), dyn, st, S, (const float4 *)shadow, (const float4 *)next, need, n, occluded, out_i, out_f);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------- path dump
// Test hook (zdr_path_dump, include/zdr.h): lane = one queried camera sample, walked vertex by vertex with the SAME
// device functions the path kernels run (path_arrive, path_shade, path_continue, pack_vertex, sweep_vertex), records kept
// per lane.  What it writes per path is what k_path adds to the pixel and what k_path_bwd queues for the scatter.
template <int SK, class A, bool ENV>
__global__ __launch_bounds__(WAVE) void k_path_dump(DScene S, RenderCfg R, SamplerCfg C, KernelIO io, const int32_t *queries, uint32_t n, int maxv, float *out) {
    extern __shared__ int lds[];
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= n) return;                                     // no wave-level operation below: lanes are independent
    const int stride = 8 + 24 * maxv;
    float *o = out + (size_t)i * stride;
    for (int k = 0; k < stride; k++) o[k] = 0.0f;
    const int px = queries[3 * i], py = queries[3 * i + 1];
    const uint32_t idx = (uint32_t)queries[3 * i + 2];
    if (px < 0 || py < 0 || px >= R.width || py >= R.height || idx >= C.spp) return;   // a query outside the image / sample range reads as all zeros
    Counters cnt;
    const uint32_t perm_seed = (SK == 0) ? xxhash32_4((uint32_t)px, (uint32_t)py, C.seed, 0u) : 0u;
    PathState ps;
    ps.smp = sampler_make<SK>(C, (uint32_t)px, (uint32_t)py, perm_seed, idx);
    pixel_ray<SK>(R, C, ps.smp, px, py, ps.o, ps.d);
    ps.beta = mk3(1.0f); ps.L = mk3(0.0f); ps.pdf_bsdf = 1e30f; ps.depth = 0;
    f3 le_grad = mk3(R.inv_spp);
    if (io.d_image) {                                       // integrator.py:38-40
        const float4 gi = io.d_image[(size_t)px + (size_t)py * R.width];
        const float fs = (float)C.spp;
        le_grad = mk3(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs));
        if (any_nan(le_grad)) le_grad = mk3(0.0f);
    }
    PackedVertex recs[ZDR_MAX_RECORDED_DEPTH];
    Hit h = A::closest(S, lds, ps.o, ps.d, 0.0f, 1e30f);
    Interaction it; f3 term_Li = mk3(0.0f); float plfrac = 0.0f;
    bool done = path_arrive<true, false, ENV>(S, ps, h, it, term_Li, cnt, &plfrac);
    int nv = 0;
    while (!done && nv < ZDR_MAX_RECORDED_DEPTH) {
        PathVertex pv; Hit h2; h2.slot = -1; h2.u = h2.v = h2.t = 0.0f;
        const f3 L0 = ps.L;
        const int slot = h.slot;
        term_Li = mk3(0.0f); plfrac = 0.0f;
        bool stop = path_shade<SK, A, true, false, ENV>(S, R, C, io, lds, ps, it, pv, h2, cnt);
        recs[nv] = pack_vertex(pv, le_grad, R.prb_mode);
        if (nv < maxv) {
            float *q = o + 8 + 24 * nv;
            const int went_on = pv.c != 0.0f ? 1 : 0;       // the BSDF sample was kept (prb.py:73-87 passed)
            q[0] = __int_as_float(it.inst); q[1] = S.shade[8 * (size_t)slot + 7].y; q[2] = it.uv.x; q[3] = it.uv.y;
            q[4] = __int_as_float((pv.cL != 0.0f ? 1 : 0) | (went_on << 1) | (pv.rr << 2));
            if (went_on) { q[5] = ps.pdf_bsdf; q[6] = ps.d.x; q[7] = ps.d.y; q[8] = ps.d.z; q[9] = ps.beta.x; q[10] = ps.beta.y; q[11] = ps.beta.z; }
            const f3 ln = ps.L - L0;
            q[16] = ln.x; q[17] = ln.y; q[18] = ln.z;
        }
        nv++;
        if (!stop) { path_continue<A, false>(S, lds, ps, h2, cnt); h = h2; stop = path_arrive<true, false, ENV>(S, ps, h, it, term_Li, cnt, &plfrac); }
        done = stop;
    }
    o[0] = __int_as_float(nv); o[1] = ps.L.x; o[2] = ps.L.y; o[3] = ps.L.z; o[5] = term_Li.x; o[6] = term_Li.y; o[7] = term_Li.z;
    if (!any_nan(ps.L) && nv > 0) {                         // prb.py:100; the sweep of k_path_bwd
        SweepState sw; sw.A = le_grad * term_Li; sw.Lv = sw.A; sw.s = 0.0f; sw.Z = 0.0f; sw.tw = (R.prb_mode != ZDR_PRB_EXPECTATION) ? 0.0f : plfrac * dot(ps.beta, sw.A);
        for (int k = nv - 1; k >= 0; k--) {
            f2 guv; const float4 g = sweep_vertex(recs[k], sw, guv, R.prb_mode);
            if (k < maxv) { float *q = o + 8 + 24 * k; q[12] = g.x; q[13] = g.y; q[14] = g.z; q[15] = g.w; }
        }
    }
}

int zdr_launch_path_dump(const DScene &S_in, const RenderCfg &R, const SamplerCfg &C, const KernelIO &io, int accel_is_bvh,
                         const int32_t *queries, uint32_t n, int32_t maxv, float *out, hipStream_t st) {
    DScene S = S_in;
    if (n == 0) return 0;
    dim3 grid((n + WAVE - 1) / WAVE);
    const size_t dyn = accel_is_bvh ? bvh_dyn_lds(S, true, true) : 0;
    with_sampler_accel(C.kind, accel_is_bvh, [&](auto sk, auto acc) {
        with_bool(S.env_count > 0, [&](auto env) {
            hipLaunchKernelGGL((k_path_dump<decltype(sk)::value, typename decltype(acc)::type, decltype(env)::value>), grid, dim3(WAVE), dyn, st, S, R, C, io, queries, n, maxv, out);
        });
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------- shading dump
// Test hook (zdr_shading_dump, include/zdr.h): lane i is row i and calls the device functions of microfacet.h, brdf_grad and the
// shading frame (scene.h) as sample_bsdf / nee_terms / the collocated integrator call them — no formula is written a second time.
// This compiles those functions into a kernel of its own: it runs their arithmetic, not the instances inlined into k_path /
// k_path_bwd, whose registers and contraction the compiler chooses afresh (the path parity tests run those).  16 floats in, 16 out.
__global__ void k_shading_dump(int mode, const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *a = in + 16 * (size_t)i;
    float *o = out + 16 * (size_t)i;
    float r[16];
    for (int k = 0; k < 16; k++) r[k] = 0.0f;
    if (mode == ZDR_SHADING_EVAL) {
        const f3 wo = ld3(a), wi = ld3(a + 3), diffuse = ld3(a + 7), ct = ld3(a + 10);
        const float roughness = a[6];
        const GgxWo gw = ggx_wo(wo, roughness);
        const GgxTerms g = ggx_terms(gw, wo, wi);
        const f3 f = ggx_brdf_from(g, wi, diffuse);
        float dlnp;
        const float dfdr = ggx_dfdr_from(g, gw, wo, wi, dlnp);
        const float4 gr = brdf_grad(wi.z * ZDR_INV_PI, dfdr, ct);
        r[0] = f.x; r[1] = f.y; r[2] = f.z; r[3] = ggx_pdf_from(g, wo, wi); r[4] = dfdr; r[5] = dlnp; r[6] = g.t; r[7] = g.D;
        r[8] = gr.x; r[9] = gr.y; r[10] = gr.z; r[11] = gr.w;
    } else if (mode == ZDR_SHADING_SAMPLE) {                   // the first lines of sample_bsdf (integrators.h)
        const f3 wo = ld3(a), diffuse = ld3(a + 4);
        const float roughness = a[3], u_lobe = a[7];
        f2 u_dir; u_dir.x = a[8]; u_dir.y = a[9];
        const f3 wi_local = ggx_sample(wo, roughness, u_lobe, u_dir);
        const GgxWo gw = ggx_wo(wo, roughness);
        const GgxTerms g = ggx_terms(gw, wo, wi_local);
        const float pdf = ggx_pdf_from(g, wo, wi_local);
        const f3 f = ggx_brdf_from(g, wi_local, diffuse);
        const float inv_p = rcp(pdf);
        const f3 w = f * inv_p;
        float dlnp;
        const float dfdr = ggx_dfdr_from(g, gw, wo, wi_local, dlnp);
        r[0] = wi_local.x; r[1] = wi_local.y; r[2] = wi_local.z; r[3] = pdf; r[4] = w.x; r[5] = w.y; r[6] = w.z;
        r[7] = dfdr; r[8] = dlnp; r[9] = (wi_local.z < 1e-4f) ? 1.0f : 0.0f; r[10] = g.t; r[11] = g.D;
    } else {                                                   // ZDR_SHADING_FRAME
        const f3 nrm = ld3(a), d = ld3(a + 3);
        const Onb onb = make_onb(nrm);
        const f3 l = to_local(onb, d), w = to_world(onb, l);
        r[0] = onb.tangent.x; r[1] = onb.tangent.y; r[2] = onb.tangent.z; r[3] = onb.binormal.x; r[4] = onb.binormal.y; r[5] = onb.binormal.z;
        r[6] = onb.normal.x; r[7] = onb.normal.y; r[8] = onb.normal.z; r[9] = l.x; r[10] = l.y; r[11] = l.z; r[12] = w.x; r[13] = w.y; r[14] = w.z;
    }
    for (int k = 0; k < 16; k++) o[k] = r[k];
}

int zdr_launch_shading_dump(int mode, const float *in, uint32_t n, float *out, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_shading_dump, dim3((n + 63) / 64), dim3(64), 0, st, mode, in, n, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------------------ light dump
// Test hook (zdr_light_dump, include/zdr.h): lane i is row i and calls the light-side device functions of scene.h — sample_light with
// sample_uniform_triangle, light_pdf and sample_alias_table behind it, sample_light_pdf, env_sampled_light_pdf, env_lookup,
// uv_to_direction, direction_to_uv, env_pdf_scale, balanced_heuristic, offset_ray_origin, surface_interact — and tent_warp1
// (integrators.h), on the scene's own light table, environment map and acceleration structure.  Like k_shading_dump this is a kernel of
// its own: it runs the functions as compiled here, not the instances inlined into the render kernels (the parity tests run those).
// Every lane stays to the end (A::closest is called by the whole wave, as in k_trace); lanes beyond n work on row n - 1 and write nothing.
template <class A, bool ENV>
__global__ __launch_bounds__(WAVE) void k_light_dump(DScene S, int mode, const float *in, uint32_t n, float *out) {
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    const uint32_t i = blockIdx.x * WAVE + threadIdx.x;
    const bool valid = i < n;
    const float *a = in + 16 * (size_t)(valid ? i : n - 1);
    float r[16];
    for (int k = 0; k < 16; k++) r[k] = 0.0f;
    if (mode == ZDR_LIGHT_SAMPLE) {
        const f3 origin = ld3(a);
        const float u_pick = a[3], u_prim = a[4];
        f2 u_pt; u_pt.x = a[5]; u_pt.y = a[6];
        f2 env_uv; env_uv.x = -1.0f; env_uv.y = -1.0f;
        int mesh_light = -1;
        const LightSample L = sample_light<ENV, true>(S, origin, u_pick, [&]() { return u_prim; }, [&]() { return u_pt; }, &env_uv, &mesh_light);
        r[0] = L.wi.x; r[1] = L.wi.y; r[2] = L.wi.z; r[3] = L.dist; r[4] = L.pdf; r[5] = L.eval.x; r[6] = L.eval.y; r[7] = L.eval.z;
        r[8] = env_uv.x; r[9] = env_uv.y; r[10] = __int_as_float(mesh_light);
    } else if (mode == ZDR_LIGHT_PDF) {
        const f3 origin = ld3(a), p = ld3(a + 3);
        const int inst = __float_as_int(a[6]), tri = __float_as_int(a[7]);
        r[0] = r[1] = __int_as_float(0x7fc00000); r[2] = __int_as_float(-1);      // a row that names no triangle of the scene reads nothing
        if (inst >= 0 && inst < S.ninst && tri >= 0 && tri < S.ntris) {
            const int slot = S.slot_of_tri[tri];
            r[0] = sample_light_pdf<ENV, true>(S, origin, inst, slot, p);
            r[1] = sample_light_pdf<ENV, false>(S, origin, inst, slot, p);
            r[2] = __int_as_float(slot);
        }
    } else if (mode == ZDR_LIGHT_ENV) {
        if constexpr (ENV) {
            const f3 d = ld3(a);
            f2 uv; uv.x = a[3]; uv.y = a[4];
            const int nl = S.env_count + S.light_count;
            const f2 duv = direction_to_uv(d);
            const f3 e = env_lookup(S, duv), w = uv_to_direction(uv);
            const f2 back = direction_to_uv(w);
            r[0] = duv.x; r[1] = duv.y; r[2] = env_sampled_light_pdf(S, d, nl); r[3] = e.x; r[4] = e.y; r[5] = e.z;
            r[6] = w.x; r[7] = w.y; r[8] = w.z; r[9] = back.x; r[10] = back.y; r[11] = env_pdf_scale(uv.y, nl);
        }
    } else if (mode == ZDR_LIGHT_MISC) {
        const f3 p = ld3(a + 2), nrm = ld3(a + 5);
        f2 u; u.x = a[8]; u.y = a[9];
        const f3 o = offset_ray_origin(p, nrm), abc = sample_uniform_triangle(u);
        r[0] = balanced_heuristic(a[0], a[1]); r[1] = o.x; r[2] = o.y; r[3] = o.z; r[4] = abc.x; r[5] = abc.y; r[6] = abc.z; r[7] = tent_warp1(a[10]);
    } else {                                                   // ZDR_LIGHT_INTERACT, ZDR_LIGHT_INTERACT_WIDE
        const Hit h = A::closest(S, lds, ld3(a), ld3(a + 3), a[6], a[7]);
        r[0] = r[1] = __int_as_float(-1); r[4] = a[7];
        if (h.slot >= 0) {
            const Interaction it = (mode == ZDR_LIGHT_INTERACT) ? surface_interact<true>(S, h) : surface_interact<false>(S, h);
            float hu = h.u, hv = h.v;                          // as k_trace reports a hit: prim from the record, the barycentrics of the INPUT corners 1 and 2
            const int ro = __float_as_int(S.shade[8 * (size_t)h.slot + 7].z);
            const float hw = 1.0f - h.u - h.v;
            if (ro == 1) { hu = hw; hv = h.u; } else if (ro == 2) { hu = h.v; hv = hw; }
            r[0] = __int_as_float(it.inst); r[1] = S.shade[8 * (size_t)h.slot + 7].y; r[2] = hu; r[3] = hv; r[4] = h.t;
            r[5] = it.p.x; r[6] = it.p.y; r[7] = it.p.z; r[8] = it.uv.x; r[9] = it.uv.y;
            r[10] = it.ns.x; r[11] = it.ns.y; r[12] = it.ns.z; r[13] = it.ng.x; r[14] = it.ng.y; r[15] = it.ng.z;
        }
    }
    if (!valid) return;
    float *o = out + 16 * (size_t)i;
    for (int k = 0; k < 16; k++) o[k] = r[k];
}

int zdr_launch_light_dump(const DScene &S_in, int accel_is_bvh, int mode, const float *in, uint32_t n, float *out, hipStream_t st) {
    DScene S = S_in;
    if (n == 0) return 0;
    const dim3 grid((n + WAVE - 1) / WAVE);
    const size_t dyn = accel_is_bvh ? bvh_dyn_lds(S, false, false) : 0;
    with_accel(accel_is_bvh, [&](auto acc) {
        with_bool(S.env_count > 0, [&](auto env) {
            hipLaunchKernelGGL((k_light_dump<typename decltype(acc)::type, decltype(env)::value>), grid, dim3(WAVE), dyn, st, S, mode, in, n, out);
        });
    });
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ------------------------------------------------------------------- texture lookup and scatter
// Test hooks (zdr_texture_lookup, zdr_texture_scatter, include/zdr.h): the bilinear lookup and its adjoint on rows the caller chooses,
// through the device functions of scene.h — read_bsdf, read_bsdf_in, env_lookup; scatter_queue_init[_cells], scatter_push,
// scatter_finish with scatter_cell, env_cell and table_cell_env behind them — and the folds above.  Like k_shading_dump these are
// kernels of their own: they run the functions as compiled here, not the instances inlined into k_path_bwd / k_simple / k_aov_bwd.
//
// Lookup: lane i is row i {u, v, bits(material), -}.  read_bsdf takes its material's size wave-uniform, as every kernel that calls it
// does (RenderCfg), so the wave walks the table and a lane keeps the result of its own material; read_bsdf_in takes the lane's entry.
// 20 floats out: read_bsdf narrow, wide; read_bsdf_in narrow, wide; env_lookup (zeros without a map), 0.
__global__ void k_texture_lookup(DScene S, const float4 *materials, MaterialTable mt, const float4 *rows, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const float4 row = rows[i < n ? i : n - 1];
    f2 uv; uv.x = row.x; uv.y = row.y;
    const int mat = __float_as_int(row.z);
    float4 r[4];
    for (int k = 0; k < 4; k++) r[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int k = 0; k < mt.nmat; k++) {                        // k and the size are wave-uniform
        const MaterialSlot m = mt.m[k];
        const float4 a = read_bsdf(materials + m.texel, uv, m.h, m.w, false), b = read_bsdf(materials + m.texel, uv, m.h, m.w, true);
        if (k == mat) { r[0] = a; r[1] = b; }
    }
    r[2] = read_bsdf_in(materials, mt.m[mat], uv, false);
    r[3] = read_bsdf_in(materials, mt.m[mat], uv, true);
    const f3 e = (S.env_count > 0) ? env_lookup(S, uv) : mk3(0.0f);
    if (i >= n) return;
    float4 *o = (float4 *)(out + 20 * (size_t)i);
    for (int k = 0; k < 4; k++) o[k] = r[k];
    o[4] = make_float4(e.x, e.y, e.z, 0.0f);
}

int zdr_launch_texture_lookup(const DScene &S, const float *materials, const MaterialTable &mt, const float *rows, uint32_t n, float *out, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_texture_lookup, dim3((n + 63) / 64), dim3(64), 0, st, S, (const float4 *)materials, mt, (const float4 *)rows, n, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Scatter: one wave per block; in round r lane l of wave b holds row 64 (b rounds + r) + l {u, v, g[4], bits(material), -} and the
// whole wave calls scatter_push with `active` = the row exists and its material is >= 0: the caller decides every ballot, and with it
// when the queue flushes.  MT, EG: the template instances of the backward kernels (single material / table / table with the map).
template <bool MT, bool EG>
__global__ __launch_bounds__(WAVE) void k_texture_scatter(RenderCfg R, KernelIO io, const float4 *rows, uint32_t n, int rounds) {
    __shared__ __attribute__((aligned(16))) float lds_q[ZDR_SCATTER_LDS_FLOATS];   // the queue writes g as one float4
    ScatterQueue q = MT ? scatter_queue_init_cells(lds_q, io.mt.ncells, R.cell_copies) : scatter_queue_init(lds_q, R.tex_h, R.tex_w, R.cell_copies);
    if constexpr (EG) q.lds_cells = nullptr;                // the map's cells are never in LDS (table_cell_env)
    for (int r = 0; r < rounds; r++) {
        const size_t i = 64 * ((size_t)blockIdx.x * rounds + r) + threadIdx.x;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = make_float4(0.0f, 0.0f, __int_as_float(-1), 0.0f);
        if (i < n) { a = rows[2 * i]; b = rows[2 * i + 1]; }
        f2 uv; uv.x = a.x; uv.y = a.y;
        const int mat = __float_as_int(b.z);
        scatter_push<MT, EG>(q, io.cells, mat >= 0, uv, make_float4(a.z, a.w, b.x, b.y), R.tex_h, R.tex_w, 0, mat >= 0 ? mat : 0, io.mt.m);
    }
    scatter_finish<MT, EG>(q, io.cells, R.tex_h, R.tex_w, 0, io.mt.m);
}

int zdr_launch_texture_scatter(const RenderCfg &R, const KernelIO &io, int table, float *d_env, const float *rows, uint32_t n, uint32_t rounds, hipStream_t st) {
    if (n == 0) return 0;
    const dim3 grid((uint32_t)(((size_t)n + 64 * (size_t)rounds - 1) / (64 * (size_t)rounds)));
    if (d_env) hipLaunchKernelGGL((k_texture_scatter<true, true>), grid, dim3(WAVE), 0, st, R, io, (const float4 *)rows, n, (int)rounds);
    else if (table) hipLaunchKernelGGL((k_texture_scatter<true, false>), grid, dim3(WAVE), 0, st, R, io, (const float4 *)rows, n, (int)rounds);
    else hipLaunchKernelGGL((k_texture_scatter<false, false>), grid, dim3(WAVE), 0, st, R, io, (const float4 *)rows, n, (int)rounds);
    launch_cells_fold(R, io, d_env, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---------------------------------------------------------------------------- sampler dump
template <int SK>
__global__ void k_sampler_dump(SamplerCfg C, const int32_t *q, uint32_t n, int nvert, int rr_depth, float *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t px = (uint32_t)q[3 * i], py = (uint32_t)q[3 * i + 1], idx = (uint32_t)q[3 * i + 2];
    uint32_t perm_seed = (SK == 0) ? xxhash32_4(px, py, C.seed, 0u) : 0u;
    Sampler s = sampler_make<SK>(C, px, py, perm_seed, idx);
    const int stride = 2 + 8 * nvert;
    float *o = out + (size_t)i * stride;
    int k = 0;
    f2 u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
    for (int v = 0; v < nvert; v++) {
        o[k++] = sampler_next<SK>(C, s); o[k++] = sampler_next<SK>(C, s);
        u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
        o[k++] = sampler_next<SK>(C, s);
        u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
        if (v >= rr_depth) o[k++] = sampler_next<SK>(C, s);
    }
    for (; k < stride; k++) o[k] = 0.0f;
}

// The same numbers drawn THE WAY THE PATH KERNELS DRAW THEM (shade_ctx / sample_bsdf, integrators.h): the pixel's next2f, then per
// vertex all seven numbers at once through cmj_vertex_samples (two Kensler permutations per register, four for a small strata grid) and the roulette draw through
// cmj_next_with_index — whenever cmj_can_batch(C), which is every BASELINE configuration — else the calls one by one.
template <int SK>
__global__ void k_vertex_sampler_dump(SamplerCfg C, const int32_t *q, uint32_t n, int nvert, int rr_depth, int direct, float *out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t px = (uint32_t)q[3 * i], py = (uint32_t)q[3 * i + 1], idx = (uint32_t)q[3 * i + 2];
    uint32_t perm_seed = (SK == 0) ? xxhash32_4(px, py, C.seed, 0u) : 0u;
    Sampler s = sampler_make<SK>(C, px, py, perm_seed, idx);
    const int stride = 2 + 8 * nvert;
    float *o = out + (size_t)i * stride;
    int k = 0;
    f2 u = direct ? sampler_pixel_offset<SK>(C, s) : sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;       // pixel_ray's draw: packed in the direct kernels only
    const bool pre = (SK == 0) && cmj_can_batch(C);             // shade_ctx's x.pre (without an environment light)
    for (int v = 0; v < nvert; v++) {
        if (pre && direct) {                                    // direct_sample (integrators.h): after the packed pixel draw, the calls one by one
            o[k++] = sampler_next<SK>(C, s); o[k++] = sampler_next<SK>(C, s);
            u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
            o[k++] = sampler_next<SK>(C, s);
            u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
            if (v >= rr_depth) o[k++] = sampler_next<SK>(C, s);
        } else if (pre) {
            const VertexSamples vs = cmj_vertex_samples(C, s);
            o[k++] = vs.u_pick; o[k++] = vs.u_prim; o[k++] = vs.u_pt.x; o[k++] = vs.u_pt.y; o[k++] = vs.u_lobe; o[k++] = vs.u_dir.x; o[k++] = vs.u_dir.y;
            if (v >= rr_depth) o[k++] = cmj_next_with_index(C, s, vs.i_rr);
        } else {
            o[k++] = sampler_next<SK>(C, s); o[k++] = sampler_next<SK>(C, s);
            u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
            o[k++] = sampler_next<SK>(C, s);
            u = sampler_next2<SK>(C, s); o[k++] = u.x; o[k++] = u.y;
            if (v >= rr_depth) o[k++] = sampler_next<SK>(C, s);
        }
    }
    for (; k < stride; k++) o[k] = 0.0f;
}

// as_kernels: 0 = the calls one by one, 1 = as the path kernels draw, 2 = as the direct kernels draw
int zdr_launch_sampler_dump(const SamplerCfg &C, const int32_t *queries, uint32_t n, int32_t nvert, int32_t rr_depth, float *out, int as_path_kernels, int *batched, hipStream_t st) {
    const int direct = as_path_kernels == 2;
    if (batched) *batched = (as_path_kernels && C.kind == ZDR_SAMPLER_CMJ && cmj_can_batch(C)) ? ((!direct && cmj_can_batch4(C)) ? 2 : 1) : 0;   // 2: a vertex's four strata in one pass.
    // The kernel does not write its route: cmj_can_batch / cmj_can_batch4 here are the very predicates cmj_vertex_samples and shade_ctx branch on (sampler.h),
    // so the report holds as long as they stay the only guards of those branches; whoever adds a condition there adds it to the predicate.
    if (n == 0) return 0;
    dim3 grid((n + 63) / 64);
    if (as_path_kernels) {
        if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL(k_vertex_sampler_dump<0>, grid, dim3(64), 0, st, C, queries, n, nvert, rr_depth, direct, out);
        else hipLaunchKernelGGL(k_vertex_sampler_dump<1>, grid, dim3(64), 0, st, C, queries, n, nvert, rr_depth, direct, out);
    } else if (C.kind == ZDR_SAMPLER_CMJ) hipLaunchKernelGGL(k_sampler_dump<0>, grid, dim3(64), 0, st, C, queries, n, nvert, rr_depth, out);
    else hipLaunchKernelGGL(k_sampler_dump<1>, grid, dim3(64), 0, st, C, queries, n, nvert, rr_depth, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
