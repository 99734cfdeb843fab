// zdr_aniso.hip — anisotropic prefiltered projective texturing for gfx950 (include/zdr.h: zdr_texel_footprint, zdr_texel_gather_aniso,
// zdr_texel_gather_aniso_backward): the on-screen footprint ellipse of every texel, the gather of an image and its mip pyramid with up to
// max_aniso trilinear probes along the ellipse's major axis — the way a texture unit filters anisotropically — and the exact transpose of
// that gather.  Linked into libzdr_aniso.so (zdr_amd/build.py), compiled without contraction: the bits are defined by the operation order
// of include/zdr.h.
//
//   k_aniso_footprint  thread = texel: the Jacobian of the view buffer's X, Y with respect to the world position, applied to the texel's
//                      square patch (side texel_size in the tangent plane of make_onb(n)), and the singular values and the major axis of
//                      that 2 x 2 matrix in closed form (footprint.h: the Jacobian and the ellipse, shared with k_tan_footprint of
//                      zdr_tangent.hip).  No list, no workspace: a texel that is not shaded writes four zeros itself.
//   k_aniso_gather     thread = texel, a run-time loop over the probes: the level split and the places of the two levels are formed once,
//                      a probe is two bilinear samples and an addition; nothing per probe is kept, so nothing goes to scratch.
//   k_aniso_scatter    thread = (texel, channel), for the reason given above k_proj_scatter (zdr_project.hip): one float atomic per tap,
//                      probe and channel (-munsafe-fp-atomics: global_atomic_add_f32, no compare-and-swap loop).
// The probes, the level split, the places, the taps, the trilinear sample and the adjoint's walk are texel_filter.h's, the very functions
// zdr_mip.hip and zdr_project.hip call.  With one probe (N = 1) the gather IS the mip gather of s = B', and where major x footprint <= 1 the
// bilinear gather, bit for bit.
#include "scene.h"
#include "aniso.h"
#include "footprint.h"
#include "texel_filter.h"

// --------------------------------------------------------------------------------------------------------------------- the footprint
__global__ __launch_bounds__(256) void k_aniso_footprint(AnisoFootprintArgs A) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= A.ntexels) return;
    const float4 *r = A.texels + 4 * (size_t)t;
    const float4 nr = r[1], pr = r[2];
    const float reach = r[3].x, ts = nr.w;
    const f3 n = mk3(nr.x, nr.y, nr.z), p = mk3(pr.x, pr.y, pr.z);
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((reach == 1.0f) && !any_nan(n) && !any_nan(p)) {         // the view's rule (k_proj_compact)
        const fp_jacobian_t J = fp_jacobian(A, p);               // (footprint.h: shared with k_tan_footprint of zdr_tangent.hip)
        if (J.front) {
            const Onb onb = make_onb(n);
            const float m00 = ts * dot(J.gX, onb.tangent), m01 = ts * dot(J.gX, onb.binormal);
            const float m10 = ts * dot(J.gY, onb.tangent), m11 = ts * dot(J.gY, onb.binormal);
            out = fp_ellipse(m00, m01, m10, m11);
        }
    }
    A.out[t] = out;
}

// ------------------------------------------------------------------------------------------------------------------ the gather
__global__ __launch_bounds__(256) void k_aniso_gather(AnisoGatherArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];                 // {visible, cosine, X, Y}
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tf_on(vw.x)) {                                       // an invisible texel reads nothing else: no footprint, no image, no pyramid
        const float4 fp = G.foot[t];                         // {major axis x, y, minor, major}
        const tf_probes_t pr = tf_probes(fp.z, fp.w, G.footprint, G.max_aniso);
        const tf_level_t lv = tf_level(pr.s, G.L);
        const tf_place_t lo = tf_place(G.width, G.height, lv.l0);
        const tf_place_t hi = tf_above(lo, lv.l0);
        const float fN = (float)pr.N, inv_n = __fdiv_rn(1.0f, fN), two_n = 2.0f * fN;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma nounroll                                             // (nor peeled for i == 0: one copy of the body, profiles/texel_filter_cost.txt)
        for (int i = 0; i < pr.N; i++) {
            const tf_xy_t q = tf_probe_xy(vw.z, vw.w, fp.x, fp.y, G.footprint, i, pr.N, two_n);
            const float4 r = tf_trilinear(G.in, G.pyramid, q.X, q.Y, lv, lo, hi);
            acc = i == 0 ? r : make_float4(acc.x + r.x, acc.y + r.y, acc.z + r.z, acc.w + r.w);
        }
        c = make_float4(vw.x * (acc.x * inv_n), vw.x * (acc.y * inv_n), vw.x * (acc.z * inv_n), vw.x * (acc.w * inv_n));
    }
    G.out[t] = c;
}

__global__ __launch_bounds__(256) void k_aniso_scatter(AnisoGatherArgs G) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, t = id >> 2, c = id & 3u;   // (id < 4 ntexels <= 2^28)
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];
    if (!tf_on(vw.x)) return;
    const float4 fp = G.foot[t];
    const tf_probes_t pr = tf_probes(fp.z, fp.w, G.footprint, G.max_aniso);
    tf_texel_t x = tf_texel(vw.x, vw.z, vw.w);
    x.ax = fp.x; x.ay = fp.y; x.N = pr.N;
    x.lv = tf_level(pr.s, G.L);
    const float g = ((const float *)G.in)[id];
    float *d_image = (float *)G.out + c, *d_pyramid = (float *)G.d_pyramid + c;
    tf_enumerate(x, TF_ANISO, G.footprint, G.width, G.height,
                 [&](bool pyramid, uint32_t pixel, float weight) { atomicAdd((pyramid ? d_pyramid : d_image) + 4 * (size_t)pixel, weight * g); });
}


// ------------------------------------------------------------------------------------------------------------------------ launchers
int zdr_launch_texel_footprint(const AnisoFootprintArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_aniso_footprint, dim3((A.ntexels + 255u) / 256u), dim3(256), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_texel_gather_aniso(const AnisoGatherArgs &G, int backward, hipStream_t st) {
    if (backward) hipLaunchKernelGGL(k_aniso_scatter, dim3((G.ntexels + 63u) / 64u), dim3(256), 0, st, G);
    else hipLaunchKernelGGL(k_aniso_gather, dim3((G.ntexels + 255u) / 256u), dim3(256), 0, st, G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
