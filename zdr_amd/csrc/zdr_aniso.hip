// zdr_aniso.hip — anisotropic prefiltered projective texturing for gfx950 (include/zdr.h: zdr_texel_footprint, zdr_texel_gather_aniso,
// zdr_texel_gather_aniso_backward): the on-screen footprint ellipse of every texel, the gather of an image and its mip pyramid with up to
// max_aniso trilinear probes along the ellipse's major axis — the way a texture unit filters anisotropically — and the exact transpose of
// that gather.  Linked into libzdr_aniso.so (zdr_amd/build.py), compiled without contraction: the bits are defined by the operation order
// of include/zdr.h.
//
//   k_aniso_footprint  thread = texel: the Jacobian of the view buffer's X, Y with respect to the world position, applied to the texel's
//                      square patch (side texel_size in the tangent plane of make_onb(n)), and the singular values and the major axis of
//                      that 2 x 2 matrix in closed form.  No list, no workspace: a texel that is not shaded writes four zeros itself.
//   k_aniso_gather     thread = texel, a run-time loop over the probes: the level split and the places of the two levels are formed once,
//                      a probe is two bilinear samples and an addition; nothing per probe is kept, so nothing goes to scratch.
//   k_aniso_scatter    thread = (texel, channel), for the reason given above k_proj_scatter (zdr_project.hip): one float atomic per tap,
//                      probe and channel (-munsafe-fp-atomics: global_atomic_add_f32, no compare-and-swap loop).
// The level split, the places, the taps and the trilinear sample are those of zdr_mip.hip operation for operation, copied (an_*) as
// zdr_mip.hip copied proj_taps: the translation units share no object file.  With one probe (N = 1) the gather IS the mip gather of
// s = B', and where major x footprint <= 1 the bilinear gather, bit for bit.
#include "scene.h"
#include "aniso.h"

ZD int32_t an_clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

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
        const f3 fwd = ld3(A.cam_fwd), right = ld3(A.cam_right), upp = ld3(A.cam_upp);
        const f3 v = p - ld3(A.cam_o);
        const float z = dot(v, fwd), a = dot(v, right), b = dot(v, upp);
        if (z > 0.0f) {
            const float zz = z * z;
            const f3 gX = (right * z - fwd * a) * __fdiv_rn(A.half_w, A.cam_tan * zz);
            const f3 gY = -((upp * z - fwd * b) * __fdiv_rn(A.half_h, (A.cam_tan * A.aspect) * zz));
            const Onb onb = make_onb(n);
            const float m00 = ts * dot(gX, onb.tangent), m01 = ts * dot(gX, onb.binormal);
            const float m10 = ts * dot(gY, onb.tangent), m11 = ts * dot(gY, onb.binormal);
            const float P = m00 * m00 + m01 * m01, Q = m10 * m10 + m11 * m11, R = m00 * m10 + m01 * m11;
            const float hd = 0.5f * (P - Q);
            const float d = __fsqrt_rn(hd * hd + R * R);
            const float major = __fsqrt_rn(0.5f * (P + Q) + d);
            const float minor = major == 0.0f ? 0.0f : __fdiv_rn(fabsf(m00 * m11 - m01 * m10), major);
            float ex, ey;
            if (P >= Q) { ex = hd + d; ey = R; } else { ex = R; ey = 0.5f * (Q - P) + d; }
            const float el = __fsqrt_rn(ex * ex + ey * ey);
            if (el == 0.0f) { ex = 1.0f; ey = 0.0f; } else { ex = __fdiv_rn(ex, el); ey = __fdiv_rn(ey, el); }
            const float ax = major * ex, ay = major * ey;
            const float big = 3.402823466e38f;                   // finite: |x| <= FLT_MAX, false for a NaN
            if (fabsf(ax) <= big && fabsf(ay) <= big && fabsf(minor) <= big && fabsf(major) <= big) out = make_float4(ax, ay, minor, major);
        }
    }
    A.out[t] = out;
}

// ------------------------------------------------------------------------------------------------------------- the level of a texel
// (zdr_mip.hip, mip_level with its footprint factor at 1)  s = max(s, 1), NaN -> 1;  l0 = its binary exponent, f = log2 of its mantissa
struct AnLevel { int l0; float f; };
ZD AnLevel an_level(float s, int L) {
    s = s * 1.0f;
    s = s > 1.0f ? s : 1.0f;
    const uint32_t b = __float_as_uint(s);
    AnLevel r;
    r.l0 = (int)(b >> 23) - 127;
    r.f = 0.0f;
    if (r.l0 >= L) { r.l0 = L; return r; }
    const float m = __uint_as_float((b & 0x007fffffu) | 0x3f800000u);
    if (m != 1.0f) r.f = fminf(log2f(m), 1.0f);
    return r;
}

struct AnPlace { int w, h; size_t off; };
ZD AnPlace an_place(int width, int height, int l) {
    AnPlace p;
    p.w = width; p.h = height; p.off = 0;
    for (int k = 1; k <= l; k++) {
        if (k > 1) p.off += (size_t)p.w * (size_t)p.h;
        p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    }
    return p;
}
ZD AnPlace an_above(AnPlace p, int l) {                              // level l + 1 from level l
    if (l >= 1) p.off += (size_t)p.w * (size_t)p.h;
    p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    return p;
}

// The taps of one probe in a level: the rule of proj_taps (zdr_project.hip) with that level's size.  Whatever X and Y hold — a NaN, an
// infinity, a probe far outside the image — the indices lie inside the level.
struct AnTaps { int32_t i00, i01, i10, i11; float tx, ty; };
ZD AnTaps an_taps(float X, float Y, int32_t width, int32_t height) {
    const float fx = X - 0.5f, fy = Y - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    AnTaps T;
    T.tx = fx - x0f; T.ty = fy - y0f;
    const int32_t x0 = (int32_t)fminf(fmaxf(x0f, -1.0f), (float)width), y0 = (int32_t)fminf(fmaxf(y0f, -1.0f), (float)height);
    const int32_t xa = an_clampi(x0, 0, width - 1), xb = an_clampi(x0 + 1, 0, width - 1);
    const int32_t ya = an_clampi(y0, 0, height - 1), yb = an_clampi(y0 + 1, 0, height - 1);
    T.i00 = ya * width + xa; T.i01 = ya * width + xb; T.i10 = yb * width + xa; T.i11 = yb * width + xb;
    return T;
}

ZD float4 an_lerp(float4 a, float4 b, float t) {
    return make_float4(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t, a.w + (b.w - a.w) * t);
}

ZD float an_exp2_neg(int l) { return __uint_as_float((uint32_t)(127 - l) << 23); }   // 2^-l, l <= 31

ZD float4 an_sample(const float4 *lvl, float X, float Y, int l, AnPlace p) {
    const float inv = an_exp2_neg(l);
    const AnTaps T = an_taps(X * inv, Y * inv, p.w, p.h);
    const float4 top = an_lerp(lvl[T.i00], lvl[T.i01], T.tx), bot = an_lerp(lvl[T.i10], lvl[T.i11], T.tx);
    return an_lerp(top, bot, T.ty);
}

// ------------------------------------------------------------------------------------------------------------- the probes of a texel
// A = major footprint, B = minor footprint.  Not A > 1 (a NaN too): one probe at level 0.  Else B' = max(B, A / max_aniso, 1) (a NaN B is
// passed over), N = clamp(ceil(A / B' - 0.125), 1, max_aniso) (a NaN gives 1), s = B'.
struct AnProbes { int N; float s; };
ZD AnProbes an_probes(float minor, float major, float footprint, int max_aniso) {
    const float A = major * footprint, B = minor * footprint;
    AnProbes r;
    r.N = 1; r.s = 1.0f;
    if (A > 1.0f) {
        const float Bp = fmaxf(fmaxf(B, __fdiv_rn(A, (float)max_aniso)), 1.0f);
        const float q = ceilf(__fdiv_rn(A, Bp) - 0.125f);
        r.N = q >= 1.0f ? (q <= (float)max_aniso ? (int)q : max_aniso) : 1;
        r.s = Bp;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_aniso_gather(AnisoGatherArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];                 // {visible, cosine, X, Y}
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vw.x != 0.0f && vw.x == vw.x) {                      // an invisible texel reads nothing else: no footprint, no image, no pyramid
        const float4 fp = G.foot[t];                         // {major axis x, y, minor, major}
        const AnProbes pr = an_probes(fp.z, fp.w, G.footprint, G.max_aniso);
        const AnLevel lv = an_level(pr.s, G.L);
        const AnPlace lo = an_place(G.width, G.height, lv.l0);
        const AnPlace hi = an_above(lo, lv.l0);              // (read only where f != 0: then l0 < L and the level exists)
        const float4 *plo = lv.l0 ? G.pyramid + lo.off : G.in, *phi = G.pyramid + hi.off;
        const float fN = (float)pr.N, inv_n = __fdiv_rn(1.0f, fN), two_n = 2.0f * fN;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < pr.N; i++) {
            const float ti = __fdiv_rn((float)(2 * i + 1 - pr.N), two_n);
            const float X = vw.z + (ti * G.footprint) * fp.x, Y = vw.w + (ti * G.footprint) * fp.y;
            float4 r = an_sample(plo, X, Y, lv.l0, lo);
            if (lv.f != 0.0f) r = an_lerp(r, an_sample(phi, X, Y, lv.l0 + 1, hi), lv.f);
            acc = i == 0 ? r : make_float4(acc.x + r.x, acc.y + r.y, acc.z + r.z, acc.w + r.w);
        }
        c = make_float4(vw.x * (acc.x * inv_n), vw.x * (acc.y * inv_n), vw.x * (acc.z * inv_n), vw.x * (acc.w * inv_n));
    }
    G.out[t] = c;
}

ZD void an_scatter(float *d, float X, float Y, int l, AnPlace p, float share, float inv_n, float visible, float g) {
    const float inv = an_exp2_neg(l);
    const AnTaps T = an_taps(X * inv, Y * inv, p.w, p.h);
    const float ux = 1.0f - T.tx, uy = 1.0f - T.ty;
    atomicAdd(d + 4 * (size_t)T.i00, ((((ux * uy) * share) * inv_n) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i01, ((((T.tx * uy) * share) * inv_n) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i10, ((((ux * T.ty) * share) * inv_n) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i11, ((((T.tx * T.ty) * share) * inv_n) * visible) * g);
}

__global__ __launch_bounds__(256) void k_aniso_scatter(AnisoGatherArgs G) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, t = id >> 2, c = id & 3u;   // (id < 4 ntexels <= 2^28)
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];
    if (!(vw.x != 0.0f && vw.x == vw.x)) return;
    const float4 fp = G.foot[t];
    const AnProbes pr = an_probes(fp.z, fp.w, G.footprint, G.max_aniso);
    const AnLevel lv = an_level(pr.s, G.L);
    const AnPlace lo = an_place(G.width, G.height, lv.l0);
    const AnPlace hi = an_above(lo, lv.l0);
    float *dlo = (lv.l0 ? (float *)(G.d_pyramid + lo.off) : (float *)G.out) + c, *dhi = (float *)(G.d_pyramid + hi.off) + c;
    const float g = ((const float *)G.in)[id];
    const float fN = (float)pr.N, inv_n = __fdiv_rn(1.0f, fN), two_n = 2.0f * fN, low = 1.0f - lv.f;
    for (int i = 0; i < pr.N; i++) {
        const float ti = __fdiv_rn((float)(2 * i + 1 - pr.N), two_n);
        const float X = vw.z + (ti * G.footprint) * fp.x, Y = vw.w + (ti * G.footprint) * fp.y;
        an_scatter(dlo, X, Y, lv.l0, lo, low, inv_n, vw.x, g);
        if (lv.f != 0.0f) an_scatter(dhi, X, Y, lv.l0 + 1, hi, lv.f, inv_n, vw.x, g);
    }
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
