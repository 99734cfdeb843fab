// texel_setup.h — a triangle of a material in the texture's pixel space, as the texture-space rasteriser (zdr_texel.hip) and the tangent
// resolve (zdr_tangent.hip) both form it: the corners of the INPUT triangle from a shade record, X = u (W - 1), Y = (1 - v) (H - 1), the
// three canonical edges and the degenerate test of include/zdr.h (zdr_scene_texel_aovs).  Device code only, every function inlined, to be
// compiled WITHOUT contraction: the edge function of a shared edge must be the same float in both triangles, and "degenerate" must be
// the same decision in every kernel that asks.
#pragma once
#include "texel.h"

#define TXD __device__ __forceinline__

// One edge of a triangle, P -> Q as the triangle runs, stored with its endpoints in canonical (lexicographic) order: a, d = b - a, and
// sg = -1 when that order is Q, P.  Two triangles that share the edge hold the same a and d, and their values differ in sign only.
struct TxEdge { float ax, ay, dx, dy, sg; };
struct TxTri { float x0, y0, x1, y1, x2, y2; };
struct TxSetup {
    TxEdge e0, e1, e2;               // opposite corner 0, 1, 2: positive on the inside of a counter-clockwise triangle
    float area2, sgn, abs2;          // e0 at corner 0 (twice the signed area), its sign as +-1, its magnitude
    float minx, maxx, miny, maxy;
    bool degenerate;                 // area 0 or NaN: no coverage, reach by the bounding box alone
};

TXD TxEdge tx_edge(float px, float py, float qx, float qy) {
    const bool sw = (qx < px) || (qx == px && qy < py);
    TxEdge e;
    e.ax = sw ? qx : px; e.ay = sw ? qy : py;
    const float bx = sw ? px : qx, by = sw ? py : qy;
    e.dx = bx - e.ax; e.dy = by - e.ay; e.sg = sw ? -1.f : 1.f;
    return e;
}
TXD float tx_eval(const TxEdge &e, float x, float y) { return e.sg * (e.dx * (y - e.ay) - e.dy * (x - e.ax)); }

TXD TxSetup tx_setup(const TxTri &T) {
    TxSetup S;
    S.e0 = tx_edge(T.x1, T.y1, T.x2, T.y2); S.e1 = tx_edge(T.x2, T.y2, T.x0, T.y0); S.e2 = tx_edge(T.x0, T.y0, T.x1, T.y1);
    S.area2 = tx_eval(S.e0, T.x0, T.y0);
    S.degenerate = !(S.area2 > 0.f || S.area2 < 0.f);
    S.sgn = S.area2 < 0.f ? -1.f : 1.f; S.abs2 = fabsf(S.area2);
    S.minx = fminf(fminf(T.x0, T.x1), T.x2); S.maxx = fmaxf(fmaxf(T.x0, T.x1), T.x2);
    S.miny = fminf(fminf(T.y0, T.y1), T.y2); S.maxy = fmaxf(fmaxf(T.y0, T.y1), T.y2);
    return S;
}

// the corners of the INPUT triangle: the brute-force accel stores a slot's corners rotated by `ro` (csrc/scene.h, r7.z)
TXD float tx_in0(int ro, float s0, float s1, float s2) { return ro == 0 ? s0 : ro == 1 ? s2 : s1; }
TXD float tx_in1(int ro, float s0, float s1, float s2) { return ro == 0 ? s1 : ro == 1 ? s0 : s2; }
TXD float tx_in2(int ro, float s0, float s1, float s2) { return ro == 0 ? s2 : ro == 1 ? s1 : s0; }

// X = u (W - 1), Y = (1 - v) (H - 1), as read_bsdf / tex_footprint form them (csrc/scene.h)
TXD TxTri tx_pixel_space(const TexelArgs &A, int ro, float u0, float v0, float u1, float v1, float u2, float v2) {
    const float wm = (float)(A.tex_w - 1), hm = (float)(A.tex_h - 1);
    TxTri T;
    T.x0 = tx_in0(ro, u0, u1, u2) * wm; T.y0 = (1.0f - tx_in0(ro, v0, v1, v2)) * hm;
    T.x1 = tx_in1(ro, u0, u1, u2) * wm; T.y1 = (1.0f - tx_in1(ro, v0, v1, v2)) * hm;
    T.x2 = tx_in2(ro, u0, u1, u2) * wm; T.y2 = (1.0f - tx_in2(ro, v0, v1, v2)) * hm;
    return T;
}
