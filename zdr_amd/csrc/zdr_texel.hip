// zdr_texel.hip — the texture-space rasteriser of include/zdr.h (zdr_scene_texel_aovs) for gfx950: which texels of a material lie on a
// model (coverage), which a bilinear lookup on it can read (reach), and where each sits in the world.  Compiled WITHOUT contraction
// (-ffp-contract=off) and linked into libzdr_texel.so (zdr_amd/build.py): the edge function of a shared edge must be the same float in both triangles, whatever it is inlined into.
//
// Three kernels, launched one after the other on the caller's stream:
//   k_texel_clear     thread = texel: the two keys of the workspace to ZDR_TEXEL_EMPTY;
//   k_texel_raster    lane = shade slot, one wave per workgroup, grid.y = bands of texel rows.  A lane whose triangle belongs to the
//                     material builds its pixel-space corners and its bounding box, grown by 1 and clipped to the texture and to the
//                     band.  A box of at most 64 texels is swept by the lane; a larger one by the whole wave, triangle by triangle
//                     (ballot, cross-lane reads, 64 lanes striding over the box).  The bands spread a scene of few triangles over the
//                     machine — the Cornell box is ONE wave of triangles and a million texels — and a scene of many triangles gets one
//                     band.  Both routes run tx_visit: the same inside and reach functions, then atomicMin of the key with g;
//   k_texel_resolve   thread = texel: the two keys, the winner's record through slot_of_tri, barycentrics at the sample point (the
//                     lattice point, or the closest point of the triangle for a texel that is only reached), four float4.
// Every loop is bounded by the clipped box.  No LDS, no scratch (tests/test_texel_resources.py), nothing allocated.
#include "texel.h"
#include "texel_setup.h"     // TxTri, TxSetup, tx_setup, tx_eval, tx_in0/1/2, tx_pixel_space: shared with zdr_tangent.hip

// the box [x - 1, x + 1] x [y - 1, y + 1] and the triangle are not separated along this edge's normal
TXD bool tx_edge_meets(const TxEdge &e, const TxSetup &S, float x, float y) {
    const float c = S.sgn * tx_eval(e, x, y), r = fabsf(e.dx) + fabsf(e.dy);
    return !(c + r < 0.f) && !(c - r > S.abs2);
}

// coverage and reach of lattice point (x, y); returns reach (coverage is a subset of it by construction)
TXD bool tx_test(const TxSetup &S, float x, float y, bool &cov) {
    cov = false;
    const bool box = S.minx <= x + 1.f && S.maxx >= x - 1.f && S.miny <= y + 1.f && S.maxy >= y - 1.f;
    if (S.degenerate) return box;
    const float c0 = S.sgn * tx_eval(S.e0, x, y), c1 = S.sgn * tx_eval(S.e1, x, y), c2 = S.sgn * tx_eval(S.e2, x, y);
    cov = c0 >= 0.f && c1 >= 0.f && c2 >= 0.f;
    return cov || (box && tx_edge_meets(S.e0, S, x, y) && tx_edge_meets(S.e1, S, x, y) && tx_edge_meets(S.e2, S, x, y));
}

// Keys only ever fall, so a key read as <= g needs no atomic whatever has happened to it since.  CHECK: read first — the per-lane route,
// where a million small triangles overlap each other's boxes and most atomics would change nothing.  The cooperative route does not: its
// wave is often alone on its SIMD, a read per step would be a round trip to L2 per step, and its atomics go out 64 neighbours at a time.
template <bool CHECK>
TXD void tx_min(uint32_t *k, uint32_t g) {
    if (!CHECK || __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > g) atomicMin(k, g);
}
template <bool CHECK>
TXD void tx_visit(const TxSetup &S, int x, int y, uint32_t g, const TexelArgs &A) {     // 0 <= x < tex_w, 0 <= y < tex_h
    bool cov;
    if (!tx_test(S, (float)x, (float)y, cov)) return;
    uint32_t *k = (uint32_t *)(A.keys + ((uint32_t)y * (uint32_t)A.tex_w + (uint32_t)x));
    if (cov) tx_min<CHECK>(k, g);
    tx_min<CHECK>(k + 1, g);
}

__global__ __launch_bounds__(256) void k_texel_clear(uint2 *keys, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) keys[p] = make_uint2(ZDR_TEXEL_EMPTY, ZDR_TEXEL_EMPTY);
}

TXD float tx_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

__global__ __launch_bounds__(64) void k_texel_raster(TexelArgs A, int band_rows) {
    const uint32_t slot = blockIdx.x * 64u + threadIdx.x;
    TxTri T = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t g = 0;
    bool live = false;
    if (slot < (uint32_t)A.ntris && A.inst_slot) {
        const float4 *r = A.shade + 8 * (size_t)slot;
        const int inst = __float_as_int(r[6].w);
        if (A.inst_slot[inst] == A.material) {
            const float4 r7 = r[7];
            g = (uint32_t)(A.inst_tri_begin[inst] + __float_as_int(r7.y));
            T = tx_pixel_space(A, __float_as_int(r7.z), r[0].w, r[1].w, r[2].w, r[3].w, r[4].w, r[5].w);
            live = !(T.x0 != T.x0 || T.y0 != T.y0 || T.x1 != T.x1 || T.y1 != T.y1 || T.x2 != T.x2 || T.y2 != T.y2);
        }
    }
    // the box, grown by 1, clipped to the texture (in float: a huge coordinate must not reach the conversion) and to this band of rows
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    if (live) {
        const float wm = (float)(A.tex_w - 1), hm = (float)(A.tex_h - 1);
        const float fx0 = fmaxf(ceilf(fminf(fminf(T.x0, T.x1), T.x2) - 1.f), 0.f), fx1 = fminf(floorf(fmaxf(fmaxf(T.x0, T.x1), T.x2) + 1.f), wm);
        const float fy0 = fmaxf(ceilf(fminf(fminf(T.y0, T.y1), T.y2) - 1.f), 0.f), fy1 = fminf(floorf(fmaxf(fmaxf(T.y0, T.y1), T.y2) + 1.f), hm);
        if (fx0 <= fx1 && fy0 <= fy1) {
            bx0 = (int)fx0; bx1 = (int)fx1;
            by0 = max((int)fy0, (int)blockIdx.y * band_rows); by1 = min((int)fy1, (int)(blockIdx.y + 1) * band_rows - 1);
        }
    }
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    const int count = (bw > 0 && bh > 0) ? bw * bh : 0;       // at most tex_h tex_w <= 2^26
    if (count > 0 && count <= 64) {                          // a small box: this lane alone
        const TxSetup S = tx_setup(T);
        int x = bx0, y = by0;
        for (int i = 0; i < count; i++) {
            tx_visit<true>(S, x, y, g, A);
            if (++x > bx1) { x = bx0; y++; }
        }
    }
    // the large boxes, one after the other, each by the whole wave: lane l takes texels l, l + 64, ... of the box in row order
    unsigned long long big = __ballot(count > 64);
    while (big) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)big) - 1);
        big &= big - 1;
        TxTri U;
        U.x0 = tx_lane(T.x0, src); U.y0 = tx_lane(T.y0, src); U.x1 = tx_lane(T.x1, src); U.y1 = tx_lane(T.y1, src);
        U.x2 = tx_lane(T.x2, src); U.y2 = tx_lane(T.y2, src);
        const uint32_t ug = (uint32_t)__builtin_amdgcn_readlane((int)g, src);
        const int ux0 = __builtin_amdgcn_readlane(bx0, src), ux1 = __builtin_amdgcn_readlane(bx1, src);
        const int uy0 = __builtin_amdgcn_readlane(by0, src), uy1 = __builtin_amdgcn_readlane(by1, src);
        const int uw = ux1 - ux0 + 1, qy = 64 / uw, qx = 64 - qy * uw;     // a step of 64 texels = qy rows and qx columns
        const TxSetup S = tx_setup(U);
        const int l = (int)threadIdx.x;
        int y = uy0 + l / uw, x = ux0 + (l - (l / uw) * uw);
        while (y <= uy1) {
            tx_visit<false>(S, x, y, ug, A);
            x += qx; y += qy;
            if (x > ux1) { x -= uw; y++; }
        }
    }
}

__global__ __launch_bounds__(256) void k_texel_resolve(TexelArgs A) {
    const uint32_t n = (uint32_t)A.tex_h * (uint32_t)A.tex_w, p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint2 k = A.keys[p];
    float4 o1 = make_float4(0.f, 0.f, 0.f, 0.f), o2 = o1, o3 = make_float4(0.f, 0.f, -1.f, -1.f);
    if (k.y != ZDR_TEXEL_EMPTY) {
        const bool cov = k.x != ZDR_TEXEL_EMPTY;
        const uint32_t g = cov ? k.x : k.y;
        const float4 *r = A.shade + 8 * (size_t)A.slot_of_tri[g];
        const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5], r6 = r[6], r7 = r[7];
        const int ro = __float_as_int(r7.z);
        const TxTri T = tx_pixel_space(A, ro, r0.w, r1.w, r2.w, r3.w, r4.w, r5.w);
        const TxSetup S = tx_setup(T);
        const int yi = (int)(p / (uint32_t)A.tex_w), xi = (int)(p - (uint32_t)yi * (uint32_t)A.tex_w);
        const float x = (float)xi, y = (float)yi;
        float w0 = 1.f, w1 = 0.f, w2 = 0.f;                  // a degenerate winner: its corner 0
        if (!S.degenerate) {
            if (cov) {                                       // the lattice point: the edge functions over their sum
                const float e0 = tx_eval(S.e0, x, y), e1 = tx_eval(S.e1, x, y), e2 = tx_eval(S.e2, x, y), s = (e0 + e1) + e2;
                if (s > 0.f || s < 0.f) { w0 = e0 / s; w1 = e1 / s; w2 = e2 / s; }
            } else {                                         // the closest point of the closed triangle: the nearest of its three sides'
                float best = __builtin_inff();
#define TX_SIDE(ax, ay, bx, by, WA, WB, WC) { \
                const float dx = (bx) - (ax), dy = (by) - (ay), l2 = dx * dx + dy * dy; \
                float t = l2 > 0.f ? ((x - (ax)) * dx + (y - (ay)) * dy) / l2 : 0.f; \
                t = fminf(fmaxf(t, 0.f), 1.f); \
                const float qx = (ax) + t * dx, qy = (ay) + t * dy, d = (x - qx) * (x - qx) + (y - qy) * (y - qy); \
                if (d < best) { best = d; WA = 1.f - t; WB = t; WC = 0.f; } }
                TX_SIDE(T.x0, T.y0, T.x1, T.y1, w0, w1, w2)
                TX_SIDE(T.x1, T.y1, T.x2, T.y2, w1, w2, w0)
                TX_SIDE(T.x2, T.y2, T.x0, T.y0, w2, w0, w1)
#undef TX_SIDE
            }
        }
        // attributes of the input triangle's corners, interpolated as surface_interact does (csrc/scene.h)
        const float px = (tx_in0(ro, r0.x, r1.x, r2.x) * w0 + tx_in1(ro, r0.x, r1.x, r2.x) * w1) + tx_in2(ro, r0.x, r1.x, r2.x) * w2;
        const float py = (tx_in0(ro, r0.y, r1.y, r2.y) * w0 + tx_in1(ro, r0.y, r1.y, r2.y) * w1) + tx_in2(ro, r0.y, r1.y, r2.y) * w2;
        const float pz = (tx_in0(ro, r0.z, r1.z, r2.z) * w0 + tx_in1(ro, r0.z, r1.z, r2.z) * w1) + tx_in2(ro, r0.z, r1.z, r2.z) * w2;
        const float nx = (tx_in0(ro, r3.x, r4.x, r5.x) * w0 + tx_in1(ro, r3.x, r4.x, r5.x) * w1) + tx_in2(ro, r3.x, r4.x, r5.x) * w2;
        const float ny = (tx_in0(ro, r3.y, r4.y, r5.y) * w0 + tx_in1(ro, r3.y, r4.y, r5.y) * w1) + tx_in2(ro, r3.y, r4.y, r5.y) * w2;
        const float nz = (tx_in0(ro, r3.z, r4.z, r5.z) * w0 + tx_in1(ro, r3.z, r4.z, r5.z) * w1) + tx_in2(ro, r3.z, r4.z, r5.z) * w2;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        const float size = S.degenerate ? 0.f : sqrtf(r7.x / (0.5f * S.abs2));
        o1 = make_float4(nx / len, ny / len, nz / len, size);
        o2 = make_float4(px, py, pz, cov ? 1.f : 0.f);
        o3 = make_float4(1.f, 0.f, (float)__float_as_int(r6.w), (float)A.material);
    }
    float4 *o = A.aovs + 4 * (size_t)p;
    o[0] = make_float4(0.f, 0.f, 0.f, 0.f); o[1] = o1; o[2] = o2; o[3] = o3;
}

int zdr_launch_texel_aovs(const TexelArgs &A, hipStream_t st) {
    const uint32_t n = (uint32_t)A.tex_h * (uint32_t)A.tex_w, blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_texel_clear, dim3(blocks), dim3(256), 0, st, A.keys, n);
    if (A.ntris > 0) {
        // bands of rows: enough workgroups for the machine when the triangles alone are too few waves (256 CUs x 4 SIMDs x 4).  Every
        // workgroup reads its 64 records again, so more and smaller bands stop paying: measured on the Cornell box at 1024^2, 1,024 bands
        // of one row 19 us, the same cut into 8 bands of columns as well 137 us (profiles/texel_aovs_cost.txt)
        const uint32_t waves = ((uint32_t)A.ntris + 63u) / 64u;
        uint32_t bands = (4096u + waves - 1u) / waves;
        bands = bands > 2048u ? 2048u : bands;
        bands = bands > (uint32_t)A.tex_h ? (uint32_t)A.tex_h : bands;
        const int band_rows = (int)(((uint32_t)A.tex_h + bands - 1u) / bands);
        bands = ((uint32_t)A.tex_h + (uint32_t)band_rows - 1u) / (uint32_t)band_rows;
        hipLaunchKernelGGL(k_texel_raster, dim3(waves, bands), dim3(64), 0, st, A, band_rows);
    }
    hipLaunchKernelGGL(k_texel_resolve, dim3(blocks), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
