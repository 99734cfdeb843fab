// footprint.h — the two halves of a footprint row that do not depend on what the texel's patch is (include/zdr.h, zdr_texel_footprint and
// zdr_texel_footprint_tangents): the derivatives gX, gY of the view buffer's X, Y with respect to the world position, and the closed-form
// ellipse of the 2 x 2 matrix M that maps the patch's two axes to the screen.  k_aniso_footprint (zdr_aniso.hip: M from texel_size and
// make_onb(n), the square patch) and k_tan_footprint (zdr_tangent.hip: M from the UV tangents) call the very same functions.  Device code
// only, inlined, to be compiled WITHOUT contraction: the bits are the header's operation order.
#pragma once
#include "vecmath.h"
#include "aniso.h"

struct fp_jacobian_t { f3 gX, gY; bool front; };           // front: z > 0; gX, gY are set only then

ZD fp_jacobian_t fp_jacobian(const AnisoFootprintArgs &A, f3 p) {
    fp_jacobian_t J;
    J.gX = mk3(0.f); J.gY = mk3(0.f);
    const f3 fwd = ld3(A.cam_fwd), right = ld3(A.cam_right), upp = ld3(A.cam_upp);
    const f3 v = p - ld3(A.cam_o);
    const float z = dot(v, fwd), a = dot(v, right), b = dot(v, upp);
    J.front = z > 0.0f;
    if (J.front) {
        const float zz = z * z;
        J.gX = (right * z - fwd * a) * __fdiv_rn(A.half_w, A.cam_tan * zz);
        J.gY = -((upp * z - fwd * b) * __fdiv_rn(A.half_h, (A.cam_tan * A.aspect) * zz));
    }
    return J;
}

// {major e.x, major e.y, minor, major} of M = (m00 m01; m10 m11); four zeros where any of them is not finite
ZD float4 fp_ellipse(float m00, float m01, float m10, float m11) {
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
    const float big = 3.402823466e38f;                       // finite: |x| <= FLT_MAX, false for a NaN
    if (fabsf(ax) <= big && fabsf(ay) <= big && fabsf(minor) <= big && fabsf(major) <= big) return make_float4(ax, ay, minor, major);
    return make_float4(0.f, 0.f, 0.f, 0.f);
}
