// texel_filter.h — the arithmetic of the texel filters, stated once: the bilinear gather (zdr_project.hip), the mip gather (zdr_mip.hip), the
// anisotropic gather (zdr_aniso.hip) and the gather plan (zdr_plan.hip) are built from the device functions below, operation for
// operation in the order of include/zdr.h (zdr_texel_gather, zdr_texel_gather_mip, zdr_texel_gather_aniso, zdr_gather_plan_*).  A header
// of forced-inline device functions: it is compiled into each of those translation units and links nothing, so every library keeps its
// own kernels.  Self-contained; every name carries tf_ / TF_, so that it can follow scene.h and accel.h, which define ZD, clampi and their kin.
//
// One formula serves the adjoints of the three filters (tf_enumerate): a tap's weight is (((w share) (1 / N)) visible), w the bilinear
// weight in its level, share the level's part of the trilinear blend, N the probe count.  Where a filter has no such factor it is exactly
// 1 — share = 1 - 0 without a fractional level, 1 / N = 1 / 1 without probes — and a product with 1 is exact, so the bits are those of the
// shorter product.  The atomic scatter kernels add weight * g and the gather plan stores weight: both take it from the one statement
// below, which is what lets the plan stand for the kernels bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TF_D __device__ __forceinline__

#define ZDR_FILTER_MAX_TEXELS (1u << 26)   // texel indices x 64-byte rows of a texel buffer within 4 GiB
#define ZDR_FILTER_MAX_PIXELS (1u << 28)   // pixel indices x 16-byte rows of an image within 4 GiB; the packed levels >= 1 hold less than half
                                           // of it, so a place in them and a row of a plan fit 32 bits

enum { TF_BILINEAR = 0, TF_MIP = 1, TF_ANISO = 2 };   // the values of zdr_gather_plan_params.filter

TF_D int32_t tf_clampi(int32_t v, int32_t lo, int32_t hi) { return min(max(v, lo), hi); }   // (lo <= hi wherever it is called: a level has a pixel)

TF_D bool tf_on(float visible) { return visible != 0.0f && visible == visible; }   // an invisible texel (0, NaN) reads nothing and adds nothing

// ---------------------------------------------------------------------------------------------------------- a position in a level
// The taps of one position in a level of width x height: indices clamped to the level, weights from the unclamped fraction.  The floor is
// clamped as a float before it becomes an integer, so that whatever X and Y hold — a NaN, an infinity, a probe far outside, a caller's
// own view buffer — the indices lie inside the level.
struct tf_taps_t { int32_t i00, i01, i10, i11; float tx, ty; };
TF_D tf_taps_t tf_taps(float X, float Y, int32_t width, int32_t height) {
    const float fx = X - 0.5f, fy = Y - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    tf_taps_t T;
    T.tx = fx - x0f; T.ty = fy - y0f;
    const int32_t x0 = (int32_t)fminf(fmaxf(x0f, -1.0f), (float)width), y0 = (int32_t)fminf(fmaxf(y0f, -1.0f), (float)height);
    const int32_t xa = tf_clampi(x0, 0, width - 1), xb = tf_clampi(x0 + 1, 0, width - 1);
    const int32_t ya = tf_clampi(y0, 0, height - 1), yb = tf_clampi(y0 + 1, 0, height - 1);
    T.i00 = ya * width + xa; T.i01 = ya * width + xb; T.i10 = yb * width + xa; T.i11 = yb * width + xb;
    return T;
}

TF_D float4 tf_lerp(float4 a, float4 b, float t) {
    return make_float4(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t, a.w + (b.w - a.w) * t);
}

TF_D float tf_exp2_neg(int l) { return __uint_as_float((uint32_t)(127 - l) << 23); }   // 2^-l, l <= 31: the scaling of X, Y is exact

// ------------------------------------------------------------------------------------------------------------- the level of a texel
// s = max(s, 1), NaN -> 1;  l0 = its binary exponent, f = log2 of its mantissa in [1, 2); at or beyond the top level: L, 0.  The split is
// integer work on the float's bits: only f carries rounding.  s is the product already formed: scale * footprint (mip), B' (aniso).
struct tf_level_t { int l0; float f; };
TF_D tf_level_t tf_level(float s, int L) {
    s = s > 1.0f ? s : 1.0f;
    const uint32_t b = __float_as_uint(s);
    tf_level_t r;
    r.l0 = (int)(b >> 23) - 127;                                    // (s >= 1: no sign, an exponent field of at least 127; infinity: 128)
    r.f = 0.0f;
    if (r.l0 >= L) { r.l0 = L; return r; }
    const float m = __uint_as_float((b & 0x007fffffu) | 0x3f800000u);
    if (m != 1.0f) r.f = fminf(log2f(m), 1.0f);
    return r;
}

// size of level l and where it begins in the packed levels >= 1, in pixels (level 0 is the image and has no place there: off 0, as
// level 1).  A loop, not a table in the kernel's arguments: l differs from lane to lane, and l0 is small wherever a gather is worth
// calling.  Widen where off becomes part of a pointer.
struct tf_place_t { int w, h; uint32_t off; };
TF_D tf_place_t tf_place(int width, int height, int l) {
    tf_place_t p;
    p.w = width; p.h = height; p.off = 0u;
    for (int k = 1; k <= l; k++) {
        if (k > 1) p.off += (uint32_t)p.w * (uint32_t)p.h;
        p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    }
    return p;
}
TF_D tf_place_t tf_above(tf_place_t p, int l) {                      // level l + 1 from level l
    if (l >= 1) p.off += (uint32_t)p.w * (uint32_t)p.h;
    p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------- the forward samples
TF_D float4 tf_sample(const float4 *lvl, float X, float Y, int l, tf_place_t p) {      // bilinear, in level l, which begins at lvl
    const float inv = tf_exp2_neg(l);
    const tf_taps_t T = tf_taps(X * inv, Y * inv, p.w, p.h);
    const float4 top = tf_lerp(lvl[T.i00], lvl[T.i01], T.tx), bot = tf_lerp(lvl[T.i10], lvl[T.i11], T.tx);
    return tf_lerp(top, bot, T.ty);
}

// trilinear: level l0 (the image where l0 == 0) and, where f != 0, level l0 + 1 (then l0 < L: the level exists; hi is not read otherwise)
TF_D float4 tf_trilinear(const float4 *image, const float4 *pyramid, float X, float Y, tf_level_t lv, tf_place_t lo, tf_place_t hi) {
    float4 r = tf_sample(lv.l0 ? pyramid + (size_t)lo.off : image, X, Y, lv.l0, lo);
    if (lv.f != 0.0f) r = tf_lerp(r, tf_sample(pyramid + (size_t)hi.off, X, Y, lv.l0 + 1, hi), lv.f);
    return r;
}

// ------------------------------------------------------------------------------------------------------------- the probes of a texel
// A = major footprint, B = minor footprint.  Not A > 1 (a NaN too): one probe at level 0.  Else B' = max(B, A / max_aniso, 1) (a NaN B is
// passed over), N = clamp(ceil(A / B' - 0.125), 1, max_aniso) (a NaN gives 1), s = B'.
struct tf_probes_t { int N; float s; };
TF_D tf_probes_t tf_probes(float minor, float major, float footprint, int max_aniso) {
    const float A = major * footprint, B = minor * footprint;
    tf_probes_t r;
    r.N = 1; r.s = 1.0f;
    if (A > 1.0f) {
        const float Bp = fmaxf(fmaxf(B, __fdiv_rn(A, (float)max_aniso)), 1.0f);
        const float q = ceilf(__fdiv_rn(A, Bp) - 0.125f);
        r.N = q >= 1.0f ? (q <= (float)max_aniso ? (int)q : max_aniso) : 1;
        r.s = Bp;
    }
    return r;
}

// probe i of N along the major axis (ax, ay): t_i = (2 i + 1 - N) / (2 N);  two_n = 2 (float)N, formed once by the caller
struct tf_xy_t { float X, Y; };
TF_D tf_xy_t tf_probe_xy(float X, float Y, float ax, float ay, float footprint, int i, int N, float two_n) {
    const float ti = __fdiv_rn((float)(2 * i + 1 - N), two_n);
    tf_xy_t q;
    q.X = X + (ti * footprint) * ax; q.Y = Y + (ti * footprint) * ay;
    return q;
}

// ---------------------------------------------------------------------------------------------------------------------- the adjoint
// What a texel sends back.  tf_texel gives the bilinear filter's state: one probe at level 0; mip sets lv, aniso sets lv, N and the axis.
struct tf_texel_t { float visible, X, Y, ax, ay; int N; tf_level_t lv; };
TF_D tf_texel_t tf_texel(float visible, float X, float Y) {
    tf_texel_t x;
    x.visible = visible; x.X = X; x.Y = Y; x.ax = 0.0f; x.ay = 0.0f; x.N = 1; x.lv.l0 = 0; x.lv.f = 0.0f;
    return x;
}

TF_D float tf_weight(float w, float share, float inv_n, float visible) { return ((w * share) * inv_n) * visible; }

template <class Emit>
TF_D void tf_emit_taps(bool pyramid, float X, float Y, int l, tf_place_t p, float share, float inv_n, float visible, Emit emit) {
    const float inv = tf_exp2_neg(l);
    const tf_taps_t T = tf_taps(X * inv, Y * inv, p.w, p.h);
    const float ux = 1.0f - T.tx, uy = 1.0f - T.ty;
    emit(pyramid, p.off + (uint32_t)T.i00, tf_weight(ux * uy, share, inv_n, visible));
    emit(pyramid, p.off + (uint32_t)T.i01, tf_weight(T.tx * uy, share, inv_n, visible));
    emit(pyramid, p.off + (uint32_t)T.i10, tf_weight(ux * T.ty, share, inv_n, visible));
    emit(pyramid, p.off + (uint32_t)T.i11, tf_weight(T.tx * T.ty, share, inv_n, visible));
}

// emit(pyramid, pixel, weight) for every tap of a visible texel, in the order every adjoint shares: probe by probe, the low level then
// the high one, taps 00, 01, 10, 11.  The destination is pixel `pixel` of the image (pyramid false) or of the packed levels >= 1 (true).
// `filter` decides one thing, whether the probes leave (X, Y): a literal folds that away, and with it — through the constants of
// tf_texel — the loop, the places and the factors that are 1.
template <class Emit>
TF_D void tf_enumerate(const tf_texel_t &x, int filter, float footprint, int width, int height, Emit emit) {
    const tf_place_t lo = tf_place(width, height, x.lv.l0);
    const tf_place_t hi = tf_above(lo, x.lv.l0);
    const float fN = (float)x.N, inv_n = __fdiv_rn(1.0f, fN), two_n = 2.0f * fN, low = 1.0f - x.lv.f;
    for (int i = 0; i < x.N; i++) {
        tf_xy_t q;
        q.X = x.X; q.Y = x.Y;
        if (filter == TF_ANISO) q = tf_probe_xy(x.X, x.Y, x.ax, x.ay, footprint, i, x.N, two_n);
        tf_emit_taps(x.lv.l0 != 0, q.X, q.Y, x.lv.l0, lo, low, inv_n, x.visible, emit);
        if (x.lv.f != 0.0f) tf_emit_taps(true, q.X, q.Y, x.lv.l0 + 1, hi, x.lv.f, inv_n, x.visible, emit);   // (then l0 < L: the level exists)
    }
}

// ------------------------------------------------------------------------------------------------- the derivative in the view buffer
// What a gather's colour does when the view buffer moves (zdr_viewgrad.hip; include/zdr.h, zdr_texel_gather_dview): the derivative of
// tf_sample and tf_trilinear in X, Y and — through the fractional level — in scale, from the taps the forward reads, formed as the
// forward forms them.  The indices are held: the derivative is the one of the piece the position lies in, the right-hand one at an
// integer fx.  Taps that clamp onto one pixel give a difference of 0 by themselves.
struct tf_grad_t { float4 c, gx, gy; };            // the sample itself, and its derivative in the X and Y of level 0
TF_D float4 tf_sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
TF_D float4 tf_mul(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
TF_D float tf_dot4(float4 d, float4 g) { return ((d.x * g.x + d.y * g.y) + d.z * g.z) + d.w * g.w; }   // channels 0 .. 3 in order

// a = c01 - c00, b = c11 - c10;  gx = a + (b - a) ty;  gy = bot - top;  both times 2^-l, which is exact (level 0: times 1)
TF_D tf_grad_t tf_sample_grad(const float4 *lvl, float X, float Y, int l, tf_place_t p) {
    const float inv = tf_exp2_neg(l);
    const tf_taps_t T = tf_taps(X * inv, Y * inv, p.w, p.h);
    const float4 c00 = lvl[T.i00], c01 = lvl[T.i01], c10 = lvl[T.i10], c11 = lvl[T.i11];
    const float4 top = tf_lerp(c00, c01, T.tx), bot = tf_lerp(c10, c11, T.tx);
    tf_grad_t r;
    r.c = tf_lerp(top, bot, T.ty);
    r.gx = tf_mul(tf_lerp(tf_sub(c01, c00), tf_sub(c11, c10), T.ty), inv);
    r.gy = tf_mul(tf_sub(bot, top), inv);
    return r;
}

#define TF_LN2 0.693147180559945309f

// d_X, d_Y, d_scale of one visible texel with the colour's cotangent d.  s = scale * footprint, the product the forward hands to
// tf_level (the bilinear filter: s = 1, L = 0, which folds the levels away).  The levels blend as tf_trilinear blends them, and the
// upper one is not read where f == 0.  d_scale only where the level split moves with s: 0 < f < 1 (then s > 1 and l0 < L; f == 1 is
// the clamp of log2f), f = log2(s) - l0, so df/dscale = footprint / (s ln 2).
struct tf_dview_t { float dX, dY, dS; };
TF_D tf_dview_t tf_dview(const float4 *image, const float4 *pyramid, float visible, float X, float Y, float s, float footprint, int L, int width,
                         int height, float4 d) {
    const tf_level_t lv = tf_level(s, L);
    const tf_place_t lo = tf_place(width, height, lv.l0);
    tf_grad_t g = tf_sample_grad(lv.l0 ? pyramid + (size_t)lo.off : image, X, Y, lv.l0, lo);
    tf_dview_t r;
    r.dS = 0.0f;
    if (lv.f != 0.0f) {
        const tf_place_t hi = tf_above(lo, lv.l0);
        const tf_grad_t h = tf_sample_grad(pyramid + (size_t)hi.off, X, Y, lv.l0 + 1, hi);
        if (lv.f < 1.0f) r.dS = visible * (tf_dot4(d, tf_sub(h.c, g.c)) * __fdiv_rn(footprint, s * TF_LN2));
        g.gx = tf_lerp(g.gx, h.gx, lv.f); g.gy = tf_lerp(g.gy, h.gy, lv.f);
    }
    r.dX = visible * tf_dot4(d, g.gx); r.dY = visible * tf_dot4(d, g.gy);
    return r;
}
