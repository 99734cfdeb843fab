// zdr_tangent.hip — per-texel UV tangents for gfx950 (include/zdr.h: zdr_scene_texel_tangents, zdr_texel_footprint_tangents): the world
// derivatives Tx, Ty of a texel's position per texture pixel, and the on-screen footprint ellipse of the parallelogram they span — the
// texel's true patch, where the square patch of zdr_texel_footprint ignores the stretch of the UV mapping.  Linked into libzdr_tangent.so
// (zdr_amd/build.py), compiled without contraction: the bits are defined by the operation order of include/zdr.h.
//
//   k_tan_resolve    thread = texel, after the three launches of zdr_texel.hip on the same stream: the two keys they left in the
//                    workspace, the winner's record through slot_of_tri, its pixel-space corners and the degenerate test by
//                    texel_setup.h — the rasteriser's own functions, so a row is zero exactly where texel_size is —, the 2 x 2 inverse,
//                    and the normal that k_texel_resolve wrote for the sign.  The wave's 64 rows are 128 consecutive float4; they are
//                    handed across the wave so that each of the two store instructions writes one contiguous KiB (as k_vg_dview).
//   k_tan_footprint  thread = texel: k_aniso_footprint with M = (gX.Tx gX.Ty; gY.Tx gY.Ty) — footprint.h's gX, gY and ellipse, the very
//                    functions that kernel calls.  One float4 store per lane, contiguous as it is.
// No atomic, no LDS, no scratch (tests/test_tangent_resources.py), nothing allocated.
#include "tangent.h"
#include "texel_setup.h"
#include "footprint.h"

__global__ __launch_bounds__(256) void k_tan_resolve(TexelArgs A, float4 *tangents) {
    const uint32_t n = (uint32_t)A.tex_h * (uint32_t)A.tex_w, p = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;      // {Tx, area}, {Ty, orientation}
    if (p < n) {
        const uint2 k = A.keys[p];
        if (k.y != ZDR_TEXEL_EMPTY) {
            const uint32_t g = k.x != ZDR_TEXEL_EMPTY ? k.x : k.y;
            const float4 *r = A.shade + 8 * (size_t)A.slot_of_tri[g];
            const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4], r5 = r[5];
            const int ro = __float_as_int(r[7].z);
            const TxTri T = tx_pixel_space(A, ro, r0.w, r1.w, r2.w, r3.w, r4.w, r5.w);
            if (!tx_setup(T).degenerate) {                       // zdr_scene_texel_aovs's own rule, on the same float
                const f3 P0 = mk3(tx_in0(ro, r0.x, r1.x, r2.x), tx_in0(ro, r0.y, r1.y, r2.y), tx_in0(ro, r0.z, r1.z, r2.z));
                const f3 P1 = mk3(tx_in1(ro, r0.x, r1.x, r2.x), tx_in1(ro, r0.y, r1.y, r2.y), tx_in1(ro, r0.z, r1.z, r2.z));
                const f3 P2 = mk3(tx_in2(ro, r0.x, r1.x, r2.x), tx_in2(ro, r0.y, r1.y, r2.y), tx_in2(ro, r0.z, r1.z, r2.z));
                const f3 e1 = P1 - P0, e2 = P2 - P0;
                const float a1 = T.x1 - T.x0, a2 = T.x2 - T.x0, b1 = T.y1 - T.y0, b2 = T.y2 - T.y0;
                const float det = a1 * b2 - a2 * b1;
                const f3 tx = mk3(__fdiv_rn(e1.x * b2 - e2.x * b1, det), __fdiv_rn(e1.y * b2 - e2.y * b1, det), __fdiv_rn(e1.z * b2 - e2.z * b1, det));
                const f3 ty = mk3(__fdiv_rn(e2.x * a1 - e1.x * a2, det), __fdiv_rn(e2.y * a1 - e1.y * a2, det), __fdiv_rn(e2.z * a1 - e1.z * a2, det));
                const f3 c = cross(tx, ty);
                const float area = __fsqrt_rn(dot(c, c));
                const float4 nr = A.aovs[4 * (size_t)p + 1];     // {normal, texel_size}: k_texel_resolve's, earlier on this stream
                const float s = dot(c, mk3(nr.x, nr.y, nr.z));
                const float orient = s > 0.0f ? 1.0f : s < 0.0f ? -1.0f : 0.0f;
                const float big = 3.402823466e38f;               // finite: |x| <= FLT_MAX, false for a NaN
                if (fabsf(tx.x) <= big && fabsf(tx.y) <= big && fabsf(tx.z) <= big && fabsf(ty.x) <= big && fabsf(ty.y) <= big && fabsf(ty.z) <= big &&
                    fabsf(area) <= big) {
                    lo = make_float4(tx.x, tx.y, tx.z, area); hi = make_float4(ty.x, ty.y, ty.z, orient);
                }
            }
        }
    }
    // The wave's 64 rows are 128 consecutive float4: lane l stores the l-th and the (64 + l)-th of them, so that each store instruction
    // writes 1 KiB in one piece (a lane storing its own row's two halves writes 16 of every 32 bytes, twice).  The whole wave is here:
    // no lane left before the shuffles.  Half h of the rows lies with the lanes 32 h .. 32 h + 31; an even float4 is a row's {Tx, area}.
    const uint32_t first = 2u * (p - lane), end = 2u * n;        // (float4 indices: at most 2^27)
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int src = 32 * h + (int)(lane >> 1);
        // every shuffle by the WHOLE wave, the choice afterwards: a shuffle inside a conditional runs with the other lanes switched off,
        // and a lane that is off hands over 0.  Chosen float by float: a float4 chosen whole goes through scratch.
        const float ax = __shfl(lo.x, src, 64), ay = __shfl(lo.y, src, 64), az = __shfl(lo.z, src, 64), aw = __shfl(lo.w, src, 64);
        const float bx = __shfl(hi.x, src, 64), by = __shfl(hi.y, src, 64), bz = __shfl(hi.z, src, 64), bw = __shfl(hi.w, src, 64);
        const bool odd = (lane & 1u) != 0u;
        const float4 v = make_float4(odd ? bx : ax, odd ? by : ay, odd ? bz : az, odd ? bw : aw);
        const uint32_t q = first + 64u * (uint32_t)h + lane;
        if (q < end) tangents[q] = v;
    }
}

__global__ __launch_bounds__(256) void k_tan_footprint(AnisoFootprintArgs A, const float4 *tangents) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= A.ntexels) return;
    const float4 *r = A.texels + 4 * (size_t)t;
    const float4 nr = r[1], pr = r[2];
    const float reach = r[3].x;
    const f3 n = mk3(nr.x, nr.y, nr.z), p = mk3(pr.x, pr.y, pr.z);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((reach == 1.0f) && !any_nan(n) && !any_nan(p)) {         // the view's rule (k_proj_compact), as k_aniso_footprint
        const float4 t0 = tangents[2 * (size_t)t], t1 = tangents[2 * (size_t)t + 1];
        const bool none = t0.x == 0.0f && t0.y == 0.0f && t0.z == 0.0f && t0.w == 0.0f && t1.x == 0.0f && t1.y == 0.0f && t1.z == 0.0f && t1.w == 0.0f;
        if (!none) {
            const fp_jacobian_t J = fp_jacobian(A, p);
            if (J.front) {
                const f3 tx = mk3(t0.x, t0.y, t0.z), ty = mk3(t1.x, t1.y, t1.z);
                out = fp_ellipse(dot(J.gX, tx), dot(J.gX, ty), dot(J.gY, tx), dot(J.gY, ty));
            }
        }
    }
    A.out[t] = out;
}

// ------------------------------------------------------------------------------------------------------------------------ launchers
int zdr_launch_texel_tangents(const TexelArgs &A, float4 *tangents, hipStream_t st) {
    const uint32_t n = (uint32_t)A.tex_h * (uint32_t)A.tex_w;
    hipLaunchKernelGGL(k_tan_resolve, dim3((n + 255u) / 256u), dim3(256), 0, st, A, tangents);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_texel_footprint_tangents(const AnisoFootprintArgs &A, const float4 *tangents, hipStream_t st) {
    hipLaunchKernelGGL(k_tan_footprint, dim3((A.ntexels + 255u) / 256u), dim3(256), 0, st, A, tangents);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
