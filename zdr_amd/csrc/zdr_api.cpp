// zdr_api.cpp — host side of libzdr_hip.so: scene assembly (what LuisaCompute's Accel / heap did
// for render.py:73-128), a binned-SAH BVH2 builder, launch configuration, and the C-ABI of
// include/zdr.h.  Compiled with hipcc -ffp-contract=off: per-triangle constants (edges, geometric
// normal, area, camera frame) are then plain IEEE float32 and reproducible on any host.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#define ZDR_DENOISE_LAUNCHER_REF __attribute__((weak))   // (csrc/denoise.h)
#include "denoise.h"
#define ZDR_ENVMAP_LAUNCHER_REF __attribute__((weak))    // (csrc/envsample.h)
#include "envsample.h"
#define ZDR_TEXEL_LAUNCHER_REF __attribute__((weak))     // (csrc/texel.h)
#include "texel.h"
#define ZDR_BAKE_LAUNCHER_REF __attribute__((weak))      // (csrc/bake.h)
#include "bake.h"
#define ZDR_PUSHPULL_LAUNCHER_REF __attribute__((weak))  // (csrc/pushpull.h)
#include "pushpull.h"
#define ZDR_PROJECT_LAUNCHER_REF __attribute__((weak))   // (csrc/project.h)
#include "project.h"
#define ZDR_MIP_LAUNCHER_REF __attribute__((weak))       // (csrc/mip.h)
#include "mip.h"
#define ZDR_ANISO_LAUNCHER_REF __attribute__((weak))     // (csrc/aniso.h)
#include "aniso.h"
#define ZDR_PLAN_LAUNCHER_REF __attribute__((weak))      // (csrc/plan.h)
#include "plan.h"
#define ZDR_VIEWGRAD_LAUNCHER_REF __attribute__((weak))  // (csrc/viewgrad.h)
#include "viewgrad.h"
#define ZDR_TANGENT_LAUNCHER_REF __attribute__((weak))   // (csrc/tangent.h)
#include "tangent.h"
#define ZDR_BAKEGRAD_LAUNCHER_REF __attribute__((weak))  // (csrc/bakegrad.h)
#include "bakegrad.h"
#define ZDR_BOUNCE_LAUNCHER_REF __attribute__((weak))    // (csrc/bounce.h)
#include "bounce.h"
#define ZDR_BOUNCEGRAD_LAUNCHER_REF __attribute__((weak))   // (csrc/bouncegrad.h)
#include "bouncegrad.h"
#define ZDR_BOUNCEENV_LAUNCHER_REF __attribute__((weak))    // (csrc/bounceenv.h)
#include "bounceenv.h"
#include "internal.h"
#include "zdr.h"

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ZDR_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" const char *zdr_version(void) { return ZDR_VERSION_STRING; }
extern "C" int zdr_abi_version(void) { return ZDR_ABI_VERSION; }
extern "C" const char *zdr_last_error(void) { return g_err.c_str(); }

// ------------------------------------------------------------------------------ host vec3
struct h3 { float x, y, z; };
static inline h3 H3(float x, float y, float z) { return {x, y, z}; }
static inline h3 hsub(h3 a, h3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline h3 hcross(h3 a, h3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static inline float hdot(h3 a, h3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline h3 hscale(h3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static inline h3 hnormalize(h3 a) { return hscale(a, 1.0f / sqrtf(hdot(a, a))); }
static inline h3 xform_point(const float *m, h3 v) {      // (M * float4(v,1)).xyz, interaction.py:19-21
    return {m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3], m[4] * v.x + m[5] * v.y + m[6] * v.z + m[7], m[8] * v.x + m[9] * v.y + m[10] * v.z + m[11]};
}
static void normal_matrix(const float *m, float *n) {      // inverse(transpose(M3x3)), interaction.py:28
    float a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    float c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    float c10 = c * h - b * i, c11 = a * i - c * g, c12 = b * g - a * h;
    float c20 = b * f - c * e, c21 = c * d - a * f, c22 = a * e - b * d;
    float inv = 1.0f / (a * c00 + b * c01 + c * c02);
    n[0] = c00 * inv; n[1] = c01 * inv; n[2] = c02 * inv; n[3] = c10 * inv; n[4] = c11 * inv; n[5] = c12 * inv;
    n[6] = c20 * inv; n[7] = c21 * inv; n[8] = c22 * inv;
}

// ------------------------------------------------------------------------------ BVH builder
// Binned SAH (ZDR_BVH_BINS bins, 3 axes), leaves of <= ZDR_BVH_LEAF triangles, depth bounded by the traversal stack.
#ifndef ZDR_BVH_BINS
#define ZDR_BVH_BINS 32   // 1 M triangles, path fwd / bwd ms at 1024^2 spp 32: 16 bins 33.9 / 44.1, 32 bins 33.5 / 43.7
#endif
// (ZDR_BVH_LEAF lives in scene.h: the walk compiles its generic leaf loop only when leaves can hold more than two triangles)
static_assert(ZDR_BVH_LEAF >= 1 && ZDR_BVH_LEAF <= 6, "the child word holds the leaf size in 3 bits, 7 = unused");
#ifndef ZDR_BVH_BFS_NODES
#define ZDR_BVH_BFS_NODES 341   // root + four levels of a full BVH4: numbered breadth-first, so that "node id < K" is the top of the tree for any K up to here
#endif
struct BNode { float lo[3], hi[3]; int left, right, first, count; };
struct Prim { float lo[3], hi[3], c[3]; int tri; };

struct BvhBuilder {
    std::vector<Prim> prims;
    std::vector<BNode> nodes;
    int max_depth = 0;
    static constexpr int kLeaf = ZDR_BVH_LEAF, kBins = ZDR_BVH_BINS, kDepthLimit = ZDR_BVH_STACK - 2;

    static void grow(float *lo, float *hi, const float *plo, const float *phi) {
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], plo[k]); hi[k] = std::max(hi[k], phi[k]); }
    }
    static int bin_of(float f) {     // float -> bin, clamped; a NaN centroid (garbage input) lands in bin 0 instead of an undefined conversion
        return (f >= 0.0f) ? ((f < (float)kBins) ? (int)f : kBins - 1) : 0;
    }
    static float area(const float *lo, const float *hi) {
        float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return 2.0f * (dx * dy + dy * dz + dz * dx);
    }
    int build(int b, int e, int depth) {
        int id = (int)nodes.size();
        nodes.push_back(BNode());
        max_depth = std::max(max_depth, depth);
        float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
        float clo[3] = {3e38f, 3e38f, 3e38f}, chi[3] = {-3e38f, -3e38f, -3e38f};
        for (int i = b; i < e; i++) { grow(lo, hi, prims[i].lo, prims[i].hi); grow(clo, chi, prims[i].c, prims[i].c); }
        BNode nd; memcpy(nd.lo, lo, 12); memcpy(nd.hi, hi, 12); nd.left = nd.right = -1; nd.first = b; nd.count = e - b;
        int n = e - b;
        if (n <= kLeaf) { nodes[id] = nd; return id; }
        int mid = -1;
        // levels still needed if we split at the median from here on
        int need = 0; for (int m = (n + kLeaf - 1) / kLeaf; m > 1; m = (m + 1) / 2) need++;
        bool force_median = depth + need + 1 >= kDepthLimit;
        if (!force_median) {
            float best = 3e38f; int best_axis = -1, best_bin = -1;
            for (int ax = 0; ax < 3; ax++) {
                float ext = chi[ax] - clo[ax];
                if (!(ext > 0.0f)) continue;
                float blo[kBins][3], bhi[kBins][3]; int bc[kBins];
                for (int k = 0; k < kBins; k++) { bc[k] = 0; for (int j = 0; j < 3; j++) { blo[k][j] = 3e38f; bhi[k][j] = -3e38f; } }
                float scale = (float)kBins / ext;
                for (int i = b; i < e; i++) {
                    int k = bin_of((prims[i].c[ax] - clo[ax]) * scale);
                    bc[k]++; grow(blo[k], bhi[k], prims[i].lo, prims[i].hi);
                }
                float rlo[kBins][3], rhi[kBins][3]; int rc[kBins];
                float alo[3] = {3e38f, 3e38f, 3e38f}, ahi[3] = {-3e38f, -3e38f, -3e38f}; int ac = 0;
                for (int k = kBins - 1; k > 0; k--) { if (bc[k]) grow(alo, ahi, blo[k], bhi[k]); ac += bc[k]; memcpy(rlo[k], alo, 12); memcpy(rhi[k], ahi, 12); rc[k] = ac; }
                float llo[3] = {3e38f, 3e38f, 3e38f}, lhi[3] = {-3e38f, -3e38f, -3e38f}; int lc = 0;
                for (int k = 0; k < kBins - 1; k++) {
                    if (bc[k]) grow(llo, lhi, blo[k], bhi[k]); lc += bc[k];
                    if (lc == 0 || rc[k + 1] == 0) continue;
                    float cost = area(llo, lhi) * (float)lc + area(rlo[k + 1], rhi[k + 1]) * (float)rc[k + 1];
                    if (cost < best) { best = cost; best_axis = ax; best_bin = k; }
                }
            }
            if (best_axis >= 0) {
                float ext = chi[best_axis] - clo[best_axis], scale = (float)kBins / ext;
                auto it = std::partition(prims.begin() + b, prims.begin() + e, [&](const Prim &p) {
                    int k = bin_of((p.c[best_axis] - clo[best_axis]) * scale);
                    return k <= best_bin; });
                mid = (int)(it - prims.begin());
            }
        }
        if (mid <= b || mid >= e) {   // median split along the widest centroid axis
            int ax = 0; float w = chi[0] - clo[0];
            for (int k = 1; k < 3; k++) if (chi[k] - clo[k] > w) { w = chi[k] - clo[k]; ax = k; }
            mid = b + n / 2;
            std::nth_element(prims.begin() + b, prims.begin() + mid, prims.begin() + e, [ax](const Prim &p, const Prim &q) { return p.c[ax] < q.c[ax]; });
        }
        int l = build(b, mid, depth + 1);
        int r = build(mid, e, depth + 1);
        nd.left = l; nd.right = r; nd.count = 0;
        nodes[id] = nd;
        return id;
    }
};

// plane-form intersection record of one triangle, float64 -> float32 (accel.h, tri_test)
static void plane_record(const h3 *p, float4 *out, float4 *w_out = nullptr) {
    double p0[3] = {p[0].x, p[0].y, p[0].z};
    double e1[3] = {(double)p[1].x - p0[0], (double)p[1].y - p0[1], (double)p[1].z - p0[2]};
    double e2[3] = {(double)p[2].x - p0[0], (double)p[2].y - p0[1], (double)p[2].z - p0[2]};
    double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    double nu[3] = {(e2[1] * n[2] - e2[2] * n[1]) / nn, (e2[2] * n[0] - e2[0] * n[2]) / nn, (e2[0] * n[1] - e2[1] * n[0]) / nn};
    double nv[3] = {(n[1] * e1[2] - n[2] * e1[1]) / nn, (n[2] * e1[0] - n[0] * e1[2]) / nn, (n[0] * e1[1] - n[1] * e1[0]) / nn};
    out[0] = make_float4((float)n[0], (float)n[1], (float)n[2], (float)(n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2]));
    out[1] = make_float4((float)nu[0], (float)nu[1], (float)nu[2], (float)-(nu[0] * p0[0] + nu[1] * p0[1] + nu[2] * p0[2]));
    out[2] = make_float4((float)nv[0], (float)nv[1], (float)nv[2], (float)-(nv[0] * p0[0] + nv[1] * p0[1] + nv[2] * p0[2]));
    if (w_out) {    // w = 1 - u - v as an edge function of its own (the third edge of a triangle that found no partner, find_quads)
        const double du = -(nu[0] * p0[0] + nu[1] * p0[1] + nu[2] * p0[2]), dv = -(nv[0] * p0[0] + nv[1] * p0[1] + nv[2] * p0[2]);
        *w_out = make_float4((float)-(nu[0] + nv[0]), (float)-(nu[1] + nv[1]), (float)-(nu[2] + nv[2]), (float)(1.0 - du - dv));
    }
}

// Brute-force scenes: pairs of triangles that form a PLANAR CONVEX QUAD are tested as one primitive (accel.h, quad test):
// one plane, one hit point, the four outer edge functions — 39 VALU for four triangles instead of 62.  Two triangles
// merge when they share an edge (the same two world positions), lie in one plane (the apex of the second at most 5e-7 of
// the quad's size off the plane of the first: a few float32 ulps of the corner coordinates themselves) on opposite sides of
// that edge, and the quad is convex (the apex of each lies strictly inside the other's two outer edges).  For each input
// triangle `rot` says which corner is the apex (= corner 0 of its slot's records: the diagonal is then the w = 0 edge of
// both triangles and the outer edges are their u = 0 and v = 0 edges); `quads` lists the merged pairs (input indices).
struct QuadPair { int a, b; bool par; };   // par: a parallelogram (the second apex = s1 + s2 - first apex)
static void find_quads(const std::vector<h3> &pos, uint32_t ntris, std::vector<int> &rot, std::vector<QuadPair> &quads) {
    rot.assign(ntris, 0); quads.clear();
    struct EdgeKey { float k[6]; bool operator<(const EdgeKey &o) const { return memcmp(k, o.k, sizeof k) < 0; } };
    auto key = [&](h3 a, h3 b) { EdgeKey e; const float A[3] = {a.x, a.y, a.z}, B[3] = {b.x, b.y, b.z};
                                 const bool sw = memcmp(A, B, sizeof A) > 0; memcpy(e.k, sw ? B : A, 12); memcpy(e.k + 3, sw ? A : B, 12);
                                 for (float &f : e.k) if (f == 0.0f) f = 0.0f;   /* -0 -> +0 */ return e; };
    std::map<EdgeKey, std::vector<std::pair<int, int>>> edges;      // edge -> (triangle, corner opposite)
    for (uint32_t t = 0; t < ntris; t++) for (int e = 0; e < 3; e++) edges[key(pos[3 * (size_t)t + (e + 1) % 3], pos[3 * (size_t)t + (e + 2) % 3])].push_back({(int)t, e});
    auto D = [](h3 v, double *o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    // which pairs COULD merge (t with corner e as its apex, t2 with corner e2)
    struct Cand { int t2, e, e2; bool par; };
    std::vector<std::vector<Cand>> adj(ntris);
    for (uint32_t t = 0; t < ntris; t++) {
        for (int e = 0; e < 3; e++) {
            for (const auto &cand : edges[key(pos[3 * (size_t)t + (e + 1) % 3], pos[3 * (size_t)t + (e + 2) % 3])]) {
                const int t2 = cand.first, e2 = cand.second;
                if (t2 == (int)t) continue;
                double a0[3], s1[3], s2[3], b0[3];
                D(pos[3 * (size_t)t + e], a0); D(pos[3 * (size_t)t + (e + 1) % 3], s1); D(pos[3 * (size_t)t + (e + 2) % 3], s2); D(pos[3 * (size_t)t2 + e2], b0);
                double e1[3], e2v[3], r[3], n[3];
                for (int k = 0; k < 3; k++) { e1[k] = s1[k] - a0[k]; e2v[k] = s2[k] - a0[k]; r[k] = b0[k] - a0[k]; }
                n[0] = e1[1] * e2v[2] - e1[2] * e2v[1]; n[1] = e1[2] * e2v[0] - e1[0] * e2v[2]; n[2] = e1[0] * e2v[1] - e1[1] * e2v[0];
                const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
                if (!(nn > 0.0)) continue;
                const double size = sqrt(std::max(std::max(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], e2v[0] * e2v[0] + e2v[1] * e2v[1] + e2v[2] * e2v[2]), r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
                if (fabs(n[0] * r[0] + n[1] * r[1] + n[2] * r[2]) / sqrt(nn) > 5e-7 * size) continue;          // not in one plane
                // barycentrics of b0 in (a0; s1, s2): u = weight of s1, v = weight of s2
                const double u = ((e2v[1] * n[2] - e2v[2] * n[1]) * r[0] + (e2v[2] * n[0] - e2v[0] * n[2]) * r[1] + (e2v[0] * n[1] - e2v[1] * n[0]) * r[2]) / nn;
                const double v = ((n[1] * e1[2] - n[2] * e1[1]) * r[0] + (n[2] * e1[0] - n[0] * e1[2]) * r[1] + (n[0] * e1[1] - n[1] * e1[0]) * r[2]) / nn;
                if (!(u > 1e-6 && v > 1e-6 && 1.0 - u - v < -1e-6)) continue;                                   // not convex, or folded back
                // (the corners at the two apices are corners of a triangle, hence convex: nothing else to check)
                adj[t].push_back({t2, e, e2, fabs(u - 1.0) <= 2e-6 && fabs(v - 1.0) <= 2e-6});
            }
        }
    }
    // greedy matching, the triangles with the fewest possible partners first (each takes its partner with the fewest): a strip
    // of quads pairs up along its own diagonals instead of across its cells
    std::vector<int> by_degree(ntris);
    for (uint32_t t = 0; t < ntris; t++) by_degree[t] = (int)t;
    std::stable_sort(by_degree.begin(), by_degree.end(), [&](int a, int b) { return adj[a].size() < adj[b].size(); });
    std::vector<uint8_t> used(ntris, 0);
    for (int t : by_degree) {
        if (used[t]) continue;
        const Cand *best = nullptr;
        for (const Cand &c : adj[t]) {
            if (used[c.t2]) continue;
            bool mutual = false;                                   // t2 must see t over the same edge (both tolerances hold)
            for (const Cand &d : adj[c.t2]) mutual = mutual || (d.t2 == t && d.e == c.e2 && d.e2 == c.e);
            if (mutual && (!best || adj[c.t2].size() < adj[best->t2].size())) best = &c;
        }
        if (!best) continue;
        used[t] = used[best->t2] = 1; rot[t] = best->e; rot[best->t2] = best->e2;
        quads.push_back({std::min(t, best->t2), std::max(t, best->t2), best->par});
    }
    // parallelograms first (their pairs take the shorter test of accel.h), each group in input order
    std::sort(quads.begin(), quads.end(), [](const QuadPair &x, const QuadPair &y) { return x.par != y.par ? x.par : x.a < y.a; });
}

// Which triangles can NEVER lie between a surface point of the scene and a point of a light — the shadow segments of next-event
// estimation (prb.py:57-59, direct.py:42-44), traced with tmin = 1e-4 and tmax = 0.9999 dist.  A triangle W qualifies when its plane
// SUPPORTS the scene: every vertex of every triangle lies on one side of it (or on it, up to `viol`, the worst violation found)
// and every vertex of every light triangle lies on that side by at least b.  A segment from p (signed distance a >= -viol, as the
// kernel computes it to within r = 4e-7 max|coordinate|) to q on a light (distance >= b) meets the plane at parameter
// t = a dist / (a - b): negative for a > 0, and at most (viol + r) D / b for a < 0, D = the scene's diagonal >= dist.  W is declared
// a non-occluder only if that bound is below HALF of tmin, so the unmasked test could not have accepted it either — the shadow
// walk skips such primitives and returns the same answer, bit for bit (tests/test_gpu_render.py, ZDR_NO_SHADOW_MASK=1).  The walls,
// floor and ceiling of a room lit from inside are the typical case: 3 of the Cornell box's 9 pairs.
static void never_occluders(const std::vector<h3> &pos, uint32_t ntris, const std::vector<uint8_t> &is_light_tri, std::vector<uint8_t> &never) {
    never.assign(ntris, 0);
    bool any_light = false;
    for (uint32_t t = 0; t < ntris; t++) any_light = any_light || is_light_tri[t];
    if (!any_light || ntris > 128) return;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, cmax = 0.0;
    for (size_t i = 0; i < 3 * (size_t)ntris; i++) {
        const double c[3] = {pos[i].x, pos[i].y, pos[i].z};
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], c[k]); hi[k] = std::max(hi[k], c[k]); cmax = std::max(cmax, fabs(c[k])); }
    }
    const double D = sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
    if (!(D > 0.0) || !(D < 1e30)) return;
    for (uint32_t w = 0; w < ntris; w++) {
        const h3 *p = &pos[3 * (size_t)w];
        double e1[3] = {(double)p[1].x - p[0].x, (double)p[1].y - p[0].y, (double)p[1].z - p[0].z}, e2[3] = {(double)p[2].x - p[0].x, (double)p[2].y - p[0].y, (double)p[2].z - p[0].z};
        double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(nn > 0.0)) continue;                                 // degenerate: never hit, but left in (it costs nothing to be careful)
        for (int k = 0; k < 3; k++) n[k] /= nn;
        double dmin = 1e300, dmax = -1e300, lmin = 1e300, lmax = -1e300;
        for (uint32_t t = 0; t < ntris; t++)
            for (int k = 0; k < 3; k++) {
                const h3 &v = pos[3 * (size_t)t + k];
                const double d = n[0] * ((double)v.x - p[0].x) + n[1] * ((double)v.y - p[0].y) + n[2] * ((double)v.z - p[0].z);
                dmin = std::min(dmin, d); dmax = std::max(dmax, d);
                if (is_light_tri[t]) { lmin = std::min(lmin, d); lmax = std::max(lmax, d); }
            }
        const double r = 4e-7 * cmax, tmin = 1e-4;
        const bool above = lmin > 0.0 && (std::max(0.0, -dmin) + r) * D <= 0.5 * tmin * lmin;     // scene on the + side, lights strictly
        const bool below = lmax < 0.0 && (std::max(0.0, dmax) + r) * D <= 0.5 * tmin * -lmax;
        never[w] = (above || below) ? 1 : 0;
    }
}

// Slot order of the brute-force walk: the two triangles of quad q in slots 2q and 2q + 1, the single triangles after them.  Within the
// parallelograms, within the other quads and within the single triangles the primitives that can occlude a shadow segment come first
// (`never`, may be null): the shadow walk then skips whole PAIRS of the others.
static uint32_t brute_slot_order(const std::vector<h3> &pos, uint32_t ntris, std::vector<int> &order, std::vector<int> &rot, uint32_t *npar = nullptr,
                                 const std::vector<uint8_t> *never = nullptr) {
    std::vector<QuadPair> quads;
    rot.assign(ntris, 0);
    if (!getenv("ZDR_NO_QUADS")) find_quads(pos, ntris, rot, quads);
    auto nv = [&](int t) { return never && (*never)[t]; };
    std::stable_sort(quads.begin(), quads.end(), [&](const QuadPair &x, const QuadPair &y) {
        if (x.par != y.par) return (bool)x.par;
        return (nv(x.a) && nv(x.b)) < (nv(y.a) && nv(y.b)); });
    std::vector<uint8_t> in_quad(ntris, 0);
    order.resize(ntris);
    uint32_t slot = 0;
    for (const QuadPair &q : quads) { order[slot++] = q.a; order[slot++] = q.b; in_quad[q.a] = in_quad[q.b] = 1; }
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t t = 0; t < ntris; t++) if (!in_quad[t] && (int)nv((int)t) == pass) order[slot++] = (int)t;
    if (npar) { *npar = 0; for (const QuadPair &q : quads) *npar += q.par ? 1u : 0u; }
    return (uint32_t)quads.size();
}

// Builds the acceleration structure over world-space triangles (pos: ntris x 3 corners).
// order[slot] = input triangle; nodes = BVH4 nodes (empty for the brute-force accel or a single leaf).
static int build_accel(const std::vector<h3> &pos, uint32_t ntris, bool use_bvh, std::vector<int> &order,
                       std::vector<float4> &nodes, uint32_t &bvh_nodes, uint32_t &bvh_depth, uint32_t &stack_entries) {
    order.resize(ntris);
    for (uint32_t t = 0; t < ntris; t++) order[t] = (int)t;
    nodes.clear(); bvh_nodes = 0; bvh_depth = 0; stack_entries = 8;
    if (!use_bvh) return ZDR_OK;
    float slo[3] = {3e38f, 3e38f, 3e38f}, shi[3] = {-3e38f, -3e38f, -3e38f};
    BvhBuilder bb;
    bb.prims.resize(ntris);
    for (uint32_t t = 0; t < ntris; t++) {
        Prim &p = bb.prims[t]; p.tri = (int)t;
        for (int k = 0; k < 3; k++) {
            float a = (&pos[3 * (size_t)t].x)[k], b = (&pos[3 * (size_t)t + 1].x)[k], c = (&pos[3 * (size_t)t + 2].x)[k];
            p.lo[k] = std::min(a, std::min(b, c)); p.hi[k] = std::max(a, std::max(b, c));
            p.c[k] = 0.5f * (p.lo[k] + p.hi[k]);
        }
        BvhBuilder::grow(slo, shi, p.lo, p.hi);
    }
    bb.nodes.reserve((size_t)ntris + 16);
    bb.build(0, (int)ntris, 0);
    for (uint32_t t = 0; t < ntris; t++) order[t] = bb.prims[t].tri;
    // conservative padding so that box culling never rejects what the triangle test accepts
    float diag = sqrtf((shi[0] - slo[0]) * (shi[0] - slo[0]) + (shi[1] - slo[1]) * (shi[1] - slo[1]) + (shi[2] - slo[2]) * (shi[2] - slo[2]));
    float pad = 4e-6f * diag + 1e-30f;
    // Collapse to a 4-wide BVH (which binary nodes survive: `collapse` below).  One node = 64 bytes (four dwordx4 loads per visit — the BVH kernels are
    // bound by the number of per-lane vector loads, so bytes per visit is what counts): the child boxes are
    // quantised to 8 bits per plane on the node's own grid,
    //   {origin.xyz, scale.x} {scale.y, scale.z, qlo.x[4], qlo.y[4]} {qlo.z[4], qhi.x[4], qhi.y[4], qhi.z[4]} {child[4]}
    // plane = origin + scale * q, rounded outwards (a quantised box always contains the padded float box);
    // child = index << 3 | count: count 0 = node index, 1..4 = first slot of a leaf, 7 = unused child.
    // Node 0 is the root; a scene that is one leaf has no nodes.
    // Which binary nodes survive as 4-wide nodes: the choice that minimises the summed surface area of the surviving nodes
    // (= the expected number of node visits of a random ray, the SAH with leaves fixed), by dynamic programming over the
    // binary tree (Ylitie, Karras, Laine 2017, section 3.1 specialised to fixed leaves): cost[n][k] = least area below n when n
    // may occupy up to k child slots of its parent.  The greedy "adopt the grandchildren of the largest child" it replaces
    // filled 3.0 of 4 slots on the 1 M triangle scene; this fills 3.4 (251 k -> 212 k nodes, 2.5 MB less to keep in L2) — at
    // the same speed: the path kernels are bound by the VALU work of the visits, and the visits saved are few.
    struct Collapse {
        const std::vector<BNode> &bn;
        std::vector<float> cost;            // 4 per binary node
        std::vector<uint8_t> split;         // 4 per binary node: 0 = as with one slot fewer, j = left gets j slots
        explicit Collapse(const std::vector<BNode> &b) : bn(b), cost(4 * b.size(), 0.0f), split(4 * b.size(), 0) {
            for (int n = (int)bn.size() - 1; n >= 0; n--) {     // children carry larger indices than their parent
                if (bn[n].count) continue;                      // leaf: constant cost, left out
                const int l = bn[n].left, r = bn[n].right;
                float best4 = 3e38f;
                for (int j = 1; j <= 3; j++) best4 = std::min(best4, cost[4 * l + j - 1] + cost[4 * r + 3 - j]);
                cost[4 * n] = BvhBuilder::area(bn[n].lo, bn[n].hi) + best4;
                for (int k = 2; k <= 4; k++) {
                    float c = cost[4 * n + k - 2]; uint8_t sp = 0;
                    for (int j = 1; j < k; j++) { float v = cost[4 * l + j - 1] + cost[4 * r + k - j - 1]; if (v < c) { c = v; sp = (uint8_t)j; } }
                    cost[4 * n + k - 1] = c; split[4 * n + k - 1] = sp;
                }
            }
        }
        void collect(int n, int k, int *kids, int &nk) const {
            while (k > 1 && !bn[n].count && split[4 * n + k - 1] == 0) k--;
            if (bn[n].count || k == 1) { kids[nk++] = n; return; }
            const int j = split[4 * n + k - 1];
            collect(bn[n].left, j, kids, nk); collect(bn[n].right, k - j, kids, nk);
        }
        void children(int n, int *kids, int &nk) const {       // the children of the wide node made from binary node n
            const int l = bn[n].left, r = bn[n].right;
            int bj = 1; float best = 3e38f;
            for (int j = 1; j <= 3; j++) { float v = cost[4 * l + j - 1] + cost[4 * r + 3 - j]; if (v < best) { best = v; bj = j; } }
            nk = 0; collect(l, bj, kids, nk); collect(r, 4 - bj, kids, nk);
        }
    } collapse(bb.nodes);
    int ninner = 0, worst_stack = 0;
    if (bb.nodes[0].count == 0) {
        // Node numbering: the top of the tree breadth-first (nodes 0 .. ZDR_BVH_BFS_NODES - 1 are the root, its children, their children ...:
        // the kernels keep the first few in LDS, accel.h), everything below depth-first (a subtree stays together in memory).
        struct Item { int bnode, id4, stack; };
        std::vector<Item> todo; todo.push_back({0, 0, 0});
        size_t head = 0;                                        // todo[head ..): pending; taken from the front while numbering breadth-first
        ninner = 1;
        nodes.assign(4, make_float4(0, 0, 0, 0));
        while (head < todo.size()) {
            Item it;
            if (ninner < ZDR_BVH_BFS_NODES) it = todo[head++];
            else { it = todo.back(); todo.pop_back(); }
            int kids[4], nk = 0;
            collapse.children(it.bnode, kids, nk);
            float lo[3][4], hi[3][4]; int child[4], cnt[4];
            for (int k = 0; k < 4; k++) {
                if (k < nk) {
                    const BNode &n = bb.nodes[kids[k]];
                    for (int ax = 0; ax < 3; ax++) { lo[ax][k] = n.lo[ax] - pad; hi[ax][k] = n.hi[ax] + pad; }
                    if (n.count) { child[k] = n.first; cnt[k] = n.count; }
                    else {
                        child[k] = ninner++; cnt[k] = 0;
                        nodes.resize(4 * (size_t)ninner, make_float4(0, 0, 0, 0));
                        todo.push_back({kids[k], child[k], it.stack + nk - 1});
                    }
                } else {
                    for (int ax = 0; ax < 3; ax++) { lo[ax][k] = 3e38f; hi[ax][k] = 3e38f; }
                    child[k] = 0; cnt[k] = -1;     // unused slot: an inverted box (below) that no finite ray enters; count 7 ends a walk that gets there anyway
                }
            }
            worst_stack = std::max(worst_stack, it.stack + nk - 1);
            // quantise on the node's grid
            float org[3], scl[3]; uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
            for (int ax = 0; ax < 3; ax++) {
                float nlo = 3e38f, nhi = -3e38f;
                for (int k = 0; k < nk; k++) { nlo = std::min(nlo, lo[ax][k]); nhi = std::max(nhi, hi[ax][k]); }
                org[ax] = nlo;
                scl[ax] = std::max(nextafterf((nhi - nlo) / 255.0f, 3e38f), 1e-30f);
                for (int k = 0; k < nk; k++) {
                    // outward rounding with a margin, then checked against the float32 plane the device reconstructs
                    double margin = 1e-3 + 8.0 * (double)(nextafterf(std::max(fabsf(nlo), fabsf(nhi)), 3e38f) - std::max(fabsf(nlo), fabsf(nhi))) / scl[ax];
                    int a = (int)std::floor(((double)lo[ax][k] - org[ax]) / scl[ax] - margin);
                    int b = (int)std::ceil(((double)hi[ax][k] - org[ax]) / scl[ax] + margin);
                    a = std::min(std::max(a, 0), 255); b = std::min(std::max(b, 0), 255);
                    while (a > 0 && fmaf((float)a, scl[ax], org[ax]) > lo[ax][k]) a--;
                    while (b < 255 && fmaf((float)b, scl[ax], org[ax]) < hi[ax][k]) b++;
                    if (fmaf((float)a, scl[ax], org[ax]) > lo[ax][k] || fmaf((float)b, scl[ax], org[ax]) < hi[ax][k])
                        return fail(ZDR_E_INVALID, "internal error: BVH box quantisation is not conservative");
                    qlo[ax] |= (uint32_t)a << (8 * k); qhi[ax] |= (uint32_t)b << (8 * k);
                }
                // unused child slots: low plane 255, high plane 0 — whatever the sign of the direction the ray would have to enter
                // after it has left (q_near A + B > q_far A + B for every finite A != 0), so the walk needs no test for them
                for (int k = nk; k < 4; k++) qlo[ax] |= 255u << (8 * k);
            }
            uint32_t cw[4];
            for (int k = 0; k < 4; k++) cw[k] = (cnt[k] < 0) ? 7u : (((uint32_t)child[k] << 3) | (uint32_t)cnt[k]);
            auto bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
            float4 *o = &nodes[4 * (size_t)it.id4];
            o[0] = make_float4(org[0], org[1], org[2], scl[0]);
            o[1] = make_float4(scl[1], scl[2], bits(qlo[0]), bits(qlo[1]));
            o[2] = make_float4(bits(qlo[2]), bits(qhi[0]), bits(qhi[1]), bits(qhi[2]));
            o[3] = make_float4(bits(cw[0]), bits(cw[1]), bits(cw[2]), bits(cw[3]));
        }
    }
    if (worst_stack + 5 > ZDR_BVH_STACK) { return fail(ZDR_E_UNSUPPORTED, "BVH needs a deeper traversal stack than ZDR_BVH_STACK"); }   // + 4 slots of slack for the unconditional stores
    {   // structural self-check before anything reaches the GPU: the nodes form a tree rooted at 0,
        // every node is referenced once, the leaves tile [0, ntris) exactly, counts fit the 3-bit field
        std::vector<uint8_t> seen_node(ninner, 0), seen_tri(ntris, 0);
        bool ok = true;
        if (ninner) seen_node[0] = 1;
        for (int i = 0; i < ninner && ok; i++) {
            uint32_t cw[4]; memcpy(cw, &nodes[4 * (size_t)i + 3], 16);
            int ch[4], ct[4];
            for (int k = 0; k < 4; k++) { ch[k] = (int)(cw[k] >> 3); ct[k] = (int)(cw[k] & 7u); if (ct[k] == 7) ct[k] = -1; }
            for (int k = 0; k < 4 && ok; k++) {
                if (ct[k] < 0) continue;
                if (ct[k] == 0) { ok = ch[k] > i && ch[k] < ninner && !seen_node[ch[k]]; if (ok) seen_node[ch[k]] = 1; }
                else {
                    ok = ct[k] <= ZDR_BVH_LEAF && ch[k] >= 0 && (uint32_t)(ch[k] + ct[k]) <= ntris;
                    for (int q = 0; q < ct[k] && ok; q++) { ok = !seen_tri[ch[k] + q]; seen_tri[ch[k] + q] = 1; }
                }
            }
        }
        for (int i = 0; i < ninner && ok; i++) ok = seen_node[i] != 0;
        if (ninner) for (uint32_t t = 0; t < ntris && ok; t++) ok = seen_tri[t] != 0;
        if (!ok) { return fail(ZDR_E_INVALID, "internal error: BVH failed its structural self-check"); }
    }
    // Child words as the device reads them (accel.h, fetch): the BYTE OFFSET of what the child names inside the one allocation that
    // holds the nodes (64 bytes each, first) and the plane records (48 bytes per slot, behind them), | the count in the low bits
    // (offsets are multiples of 16).  The structural check above read the index form.
    if ((size_t)ninner * 64 + (size_t)ntris * 48 >= (1ull << 32)) return fail(ZDR_E_UNSUPPORTED, "BVH nodes and triangle records exceed 4 GiB");
    for (int i = 0; i < ninner; i++) {
        uint32_t cw[4]; memcpy(cw, &nodes[4 * (size_t)i + 3], 16);
        for (int k = 0; k < 4; k++) {
            const uint32_t idx = cw[k] >> 3, ct = cw[k] & 7u;
            cw[k] = (ct == 7u) ? 7u : ((ct == 0u ? idx * 64u : (uint32_t)ninner * 64u + idx * 48u) | ct);
        }
        memcpy(&nodes[4 * (size_t)i + 3], cw, 16);
    }
    bvh_nodes = (uint32_t)ninner; bvh_depth = (uint32_t)bb.max_depth;
    stack_entries = (uint32_t)((worst_stack + 5 + 3) & ~3);   // deepest pending set + the four unconditionally stored slots
    return ZDR_OK;
}

// --------------------------------------------------------------------------- device memory
static bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

// A workspace that has to grow: not while the stream is capturing (an allocation cannot be recorded, and the capture would name a
// buffer that does not exist yet) — one eager call of the same kind and size beforehand sizes everything.
static int may_allocate(bool capturing, const char *what) {
    if (!capturing) return ZDR_OK;
    return fail(ZDR_E_UNSUPPORTED, std::string("the ") + what + " workspace would have to be allocated while the stream is capturing: make one eager call of this kind, resolution and spp on the handle first");
}

// The device memory of a scene handle (zdr_scene derives from it): every buffer is a DevBuf member of the handle, which registers
// itself here, so that a buffer's life is written once — alloc / reserve / release below, free_all at zdr_scene_destroy.
// A render call recorded while its stream was CAPTURING (hipStreamBeginCapture; torch.cuda.graph) bakes the handle's workspace
// pointers into a graph that may be replayed at any later time.  From then on the handle never frees a buffer a kernel can read or
// write — one that has to grow is retired (kept until zdr_scene_destroy) and replaced — and never trusts the tile masks in the
// buffer, which a replay rebuilds for ITS view behind the host's back (render_common).
struct DevMem { bool captured = false; std::vector<struct DevBuf *> owned; std::vector<void *> retired; };
struct DevBuf {
    DevMem &mem; void *p = nullptr; size_t bytes = 0;      // bytes: as allocated
    explicit DevBuf(DevMem &m) : mem(m) { m.owned.push_back(this); }
    DevBuf(const DevBuf &) = delete;
    hipError_t alloc(size_t n) { const hipError_t e = hipMalloc(&p, n); if (e != hipSuccess) p = nullptr; bytes = p ? n : 0; return e; }   // (of an empty buffer)
    void release() {                        // of a buffer that no kernel in flight reads: freed — unless a captured graph may still name it
        if (p) { if (mem.captured) mem.retired.push_back(p); else (void)hipFree(p); }
        p = nullptr; bytes = 0;
    }
    int reserve(size_t need, bool capturing, const char *what) {   // grow-only; the contents do not survive growing
        if (need <= bytes) return ZDR_OK;
        if (int rc = may_allocate(capturing, what)) return rc;
        release();
        const hipError_t e = alloc(need);
        return e == hipSuccess ? ZDR_OK : fail(ZDR_E_HIP, std::string("hipMalloc of the ") + what + " workspace, " + std::to_string(need) + " bytes: " + hipGetErrorString(e));
    }
    static void free_all(DevMem &m) {       // zdr_scene_destroy
        for (DevBuf *b : m.owned) (void)hipFree(b->p);
        for (void *q : m.retired) (void)hipFree(q);
    }
};
template <class T> struct Dev : DevBuf { using DevBuf::DevBuf; operator T *() const { return (T *)p; } };   // reads as the T * it holds

// ----------------------------------------------------------------------------------- scene
struct zdr_scene : DevMem {
    int device = 0;
    int accel_is_bvh = 0;
    uint32_t ntris = 0, nverts = 0, ninst = 0;
    uint32_t bvh_nodes = 0, bvh_depth = 0, stack_entries = 8;
    std::vector<int32_t> inst_tri_begin;
    std::vector<float> emission;
    Dev<float4> d_isect{*this}, d_pairs{*this}, d_shade{*this}, d_nodes{*this};   // (BVH: the plane records lie in d_nodes, d_isect stays empty)
    std::vector<int> slot_tri;              // brute force: slot -> input triangle
    unsigned long long shadow_pairs = ~0ull;   // brute force: the pairs of the pair walk a shadow segment can meet (never_occluders; rebuilt when the lights change)
    uint32_t nquads = 0, nquads2 = 0, npar = 0;   // brute force: primitives of the pair walk, how many of them are merged quads (find_quads), how many of those parallelograms
    Dev<float4> d_ppairs{*this};
    Dev<float> d_emission{*this};
    // flat light table (scene.h): one 80-byte entry per triangle of every emitting instance + {first entry, count} per light
    std::vector<float4> tri_geo;            // host copy, 4 float4 per INPUT triangle: p0, p1, p2, {ng, area} (lights may change)
    Dev<float4> d_light_tris{*this};
    Dev<int32_t> d_light_range{*this};      // 2 ints per instance slot
    Dev<float4> d_emission4{*this};         // ninst x {e.rgb, bits(light index | -1)}
    Dev<int32_t> d_light_insts{*this}, d_inst_tri_begin{*this}, d_slot_of_tri{*this};
    Dev<uint32_t> d_pmj{*this}; Dev<uint16_t> d_bn{*this}; SamplerTables tab{};
    Dev<float4> d_env_tex{*this}; Dev<float> d_alias_prob{*this}, d_env_pdf{*this}; Dev<int32_t> d_alias_idx{*this};
    Dev<EnvSamplingScratch> d_env_scratch{*this};           // workspace of zdr_scene_update_envmap_sampling: allocated by its first call, kept until zdr_scene_destroy
    Dev<float4> d_partial{*this};
    Dev<unsigned long long> d_tile_masks{*this};                              // camera-ray candidate pairs per tile (k_tile_masks)
    float tile_mask_key[24]; bool tile_mask_key_set = false;                  // camera + tile grid the masks in the buffer were built for (all tiles of the rectangle, whatever the shard)
    Dev<unsigned int> d_work_counters{*this};
    Dev<float4> d_ring{*this};                              // primary rings of the path kernels (integrators.h)
    Dev<float> d_cells{*this};                              // backward staging cells, (tex_h+1) x (tex_w+1) x 16 floats
    Dev<unsigned long long> d_counters{*this};
    std::vector<int32_t> inst_slot;                         // material slot of each instance (zdr_scene_set_material_slots), -1 = none; empty = never set
    Dev<int32_t> d_inst_slot{*this};                        // its device copy, allocated by the first call that needs it
    Dev<int32_t> d_inst_slot0{*this};                       // {0, -1, -1, ...}: the slot table of a single-material environment-gradient call (render_common)
    Dev<float> d_emit_acc{*this};                           // emission-gradient accumulator: ZDR_EMISSION_COPIES rows of light_count x 3 floats (render_common)
    Dev<unsigned int> d_error{*this};                       // device error word (scene.h, ZDR_DEVERR_*), sticky until read
    uint64_t device_bytes = 0;                              // uploads, the slot table and the environment scratch; not the per-call workspaces
    DScene ds{};
};

// a new buffer with a copy of `bytes` host bytes; counted in *acc (zdr_scene_info_t::device_bytes)
static hipError_t upload(DevBuf &dst, const void *src, size_t bytes, uint64_t *acc) {
    hipError_t e = dst.alloc(std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    if (acc) *acc += bytes;
    return bytes ? hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
}

static void light_list(const std::vector<float> &em, uint32_t ninst, std::vector<int32_t> &out, int &count) {
    out.assign(ninst, 0); count = 0;     // render.py:89-90,118-121,146-148
    for (uint32_t i = 0; i < ninst; i++)
        if (em[3 * i] > 0.0f || em[3 * i + 1] > 0.0f || em[3 * i + 2] > 0.0f) out[count++] = (int32_t)i;
}

// The corners of `ntris` triangles as the builders take them: three floats each, `corner` floats from one corner to the next and
// `tri` floats from one triangle to the next — (3, 9) for packed positions, (4, 16) for zdr_scene::tri_geo.
static std::vector<h3> triangle_corners(const float *xyz, uint32_t ntris, size_t corner, size_t tri) {
    std::vector<h3> pos(3 * (size_t)ntris);
    for (uint32_t t = 0; t < ntris; t++) for (int k = 0; k < 3; k++) { const float *c = xyz + tri * t + corner * k; pos[3 * (size_t)t + k] = H3(c[0], c[1], c[2]); }
    return pos;
}
static bool wants_bvh(int accel, uint32_t ntris) { return accel == ZDR_ACCEL_BVH || (accel == ZDR_ACCEL_AUTO && ntris > 64); }

// Light table for sample_light (scene.h): the reference walks light -> instance -> triangle range -> triangle ->
// emission through four dependent lookups (light.py:33-48); on the GPU that is four memory round trips and eleven
// per-lane loads per path vertex.  Flattened here to {first entry, T} per light and one 80-byte entry per light
// triangle {p0} {p1} {p2} {ng, area} {emission, 0}, the same floats the shade records hold.
// the pairs of the brute-force walk that hold at least one primitive a shadow segment can meet, for the current lights
static unsigned long long shadow_pair_mask(const zdr_scene *s, const std::vector<int32_t> &lights, int count) {
    if (s->accel_is_bvh || s->slot_tri.empty() || s->ntris > 128 || getenv("ZDR_NO_SHADOW_MASK")) return ~0ull;
    const std::vector<h3> pos = triangle_corners((const float *)s->tri_geo.data(), s->ntris, 4, 16);
    std::vector<uint8_t> is_light(s->ntris, 0), never;
    for (int l = 0; l < count; l++) for (int t = s->inst_tri_begin[lights[l]]; t < s->inst_tri_begin[lights[l] + 1]; t++) is_light[t] = 1;
    never_occluders(pos, s->ntris, is_light, never);
    unsigned long long m = 0ull;
    for (uint32_t q = 0; q < s->nquads; q++) {                  // primitive q: slots 2q, 2q + 1 (a quad) or slot q + nquads2 (a single triangle)
        const bool quad = q < s->nquads2;
        const uint32_t a = quad ? 2 * q : q + s->nquads2;
        const bool skip = never[s->slot_tri[a]] && (!quad || never[s->slot_tri[a + 1]]);
        if (!skip) m |= 1ull << (q / 2);
    }
    return m;
}

static int upload_light_table(zdr_scene *s, const std::vector<int32_t> &lights, int count, hipStream_t st) {
    s->shadow_pairs = shadow_pair_mask(s, lights, count);
    std::vector<float4> tab; std::vector<int32_t> range(2 * (size_t)s->ninst, 0);
    for (int l = 0; l < count; l++) {
        const int inst = lights[l], b = s->inst_tri_begin[inst], T = s->inst_tri_begin[inst + 1] - b;
        range[2 * l] = (int32_t)(tab.size() / 5); range[2 * l + 1] = T;
        for (int t = b; t < b + T; t++) {
            for (int k = 0; k < 4; k++) tab.push_back(s->tri_geo[4 * (size_t)t + k]);
            tab.push_back(make_float4(s->emission[3 * (size_t)inst], s->emission[3 * (size_t)inst + 1], s->emission[3 * (size_t)inst + 2], 0.0f));
        }
    }
    if (tab.empty()) tab.push_back(make_float4(0, 0, 0, 0));
    if (tab.size() * sizeof(float4) > (1ull << 32)) return fail(ZDR_E_UNSUPPORTED, "light table above 4 GiB: the kernels address its entries with 32-bit byte offsets");
    // (no capture check, hence `false`: this call synchronises the stream, which a capturing stream refuses by itself)
    if (tab.size() * sizeof(float4) > s->d_light_tris.bytes) HIPCHK(hipStreamSynchronize(st));   // nothing in flight may still read the table that goes
    if (int rc = s->d_light_tris.reserve(tab.size() * sizeof(float4), false, "light-table")) return rc;
    if (int rc = s->d_light_range.reserve(range.size() * sizeof(int32_t), false, "light-table")) return rc;
    if (int rc = s->d_emission4.reserve((size_t)s->ninst * sizeof(float4), false, "light-table")) return rc;
    std::vector<float4> e4(s->ninst);
    // .w: bits of the instance's index in the light list, -1 = not a light (read by the emission-gradient kernels only, as an int)
    std::vector<int32_t> light_of(s->ninst, -1);
    for (int l = 0; l < count; l++) light_of[lights[l]] = l;
    for (uint32_t i = 0; i < s->ninst; i++) {
        e4[i] = make_float4(s->emission[3 * (size_t)i], s->emission[3 * (size_t)i + 1], s->emission[3 * (size_t)i + 2], 0.0f);
        memcpy(&e4[i].w, &light_of[i], sizeof(int32_t));
    }
    HIPCHK(hipMemcpyAsync(s->d_light_tris, tab.data(), tab.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_light_range, range.data(), range.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_emission4, e4.data(), e4.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));       // the host vectors go out of scope
    s->ds.light_tris = s->d_light_tris; s->ds.light_range = s->d_light_range; s->ds.emission4 = s->d_emission4;
    s->ds.light0_T = count > 0 ? range[1] : 0;
    return ZDR_OK;
}

// ---- zdr_scene_create, step by step: what the steps hand on, on the host
struct TriRec { h3 p[3], n[3]; float uv[3][2]; h3 ng; float area; int inst, prim; };
struct SceneBuild {
    std::vector<TriRec> rec;                // world-space records, input order
    bool use_bvh = false;
    std::vector<int> order, rot;            // slot -> input triangle; input triangle -> the input corner that is its slot's corner 0 (find_quads)
    std::vector<float4> nodes, isect, shade, wedge;   // wedge: third edge function of every slot (single triangles of the brute-force walk)
    std::vector<int32_t> slot_of_tri;
    std::vector<float> pairs, ppairs;       // brute force: the records of the pair walk
};

// 1. world-space per-triangle records in input order (and the handle's copy of their geometry, zdr_scene::tri_geo)
static void world_records(zdr_scene *s, const float *verts8, const int32_t *tris, const float *inst_xform, SceneBuild &B) {
    B.rec.resize(s->ntris);
    static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (uint32_t i = 0; i < s->ninst; i++) {
        const float *m = inst_xform ? inst_xform + 16 * (size_t)i : ident;
        float nm[9]; normal_matrix(m, nm);
        for (int t = s->inst_tri_begin[i]; t < s->inst_tri_begin[i + 1]; t++) {
            TriRec &r = B.rec[t];
            for (int k = 0; k < 3; k++) {
                const float *v = verts8 + 8 * (size_t)tris[3 * (size_t)t + k];
                r.p[k] = xform_point(m, H3(v[0], v[1], v[2]));
                r.uv[k][0] = v[3]; r.uv[k][1] = v[4];
                r.n[k] = H3(nm[0] * v[5] + nm[1] * v[6] + nm[2] * v[7], nm[3] * v[5] + nm[4] * v[6] + nm[5] * v[7], nm[6] * v[5] + nm[7] * v[6] + nm[8] * v[7]);
            }
            h3 c = hcross(hsub(r.p[1], r.p[0]), hsub(r.p[2], r.p[0]));
            r.ng = hnormalize(c);                       // interaction.py:29, light.py:68
            r.area = sqrtf(hdot(c, c)) / 2.0f;          // light.py:72
            r.inst = (int)i; r.prim = t - s->inst_tri_begin[i];
        }
    }
    s->tri_geo.resize(4 * (size_t)s->ntris);
    for (uint32_t t = 0; t < s->ntris; t++) {
        const TriRec &r = B.rec[t];
        for (int k = 0; k < 3; k++) s->tri_geo[4 * (size_t)t + k] = make_float4(r.p[k].x, r.p[k].y, r.p[k].z, 0.0f);
        s->tri_geo[4 * (size_t)t + 3] = make_float4(r.ng.x, r.ng.y, r.ng.z, r.area);
    }
}

// 2. acceleration structure: slot order + nodes
static int accel_and_slot_order(zdr_scene *s, int accel, SceneBuild &B) {
    const uint32_t ntris = s->ntris;
    const std::vector<h3> pos = triangle_corners((const float *)s->tri_geo.data(), ntris, 4, 16);
    B.use_bvh = wants_bvh(accel, ntris);
    if (int rc = build_accel(pos, ntris, B.use_bvh, B.order, B.nodes, s->bvh_nodes, s->bvh_depth, s->stack_entries)) return rc;
    s->accel_is_bvh = B.use_bvh ? 1 : 0;
    // brute force: merge coplanar triangle pairs into quads; slots 2q, 2q + 1 = quad q, the single triangles follow
    B.rot.assign(ntris, 0);
    if (!B.use_bvh) {
        std::vector<uint8_t> is_light(ntris, 0), never;       // (the lights of the moment only ORDER the primitives; the mask itself follows update_lights)
        for (uint32_t t = 0; t < ntris; t++) { const float *e = &s->emission[3 * (size_t)B.rec[t].inst]; is_light[t] = (e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f) ? 1 : 0; }
        never_occluders(pos, ntris, is_light, never);
        s->nquads2 = brute_slot_order(pos, ntris, B.order, B.rot, &s->npar, &never); s->nquads = ntris - s->nquads2;
        s->slot_tri = B.order;
    }
    return ZDR_OK;
}

// 3. per-slot records: plane records, shade records, third edge functions; brute force: the pair records made of them
static void slot_records(zdr_scene *s, SceneBuild &B) {
    const uint32_t ntris = s->ntris;
    B.isect.assign(3 * (size_t)ntris + 3, make_float4(0, 0, 0, 0)); B.shade.resize(8 * (size_t)ntris);   // + one record: the BVH walk fetches four float4 behind a leaf's first triangle
    B.slot_of_tri.resize(ntris); B.wedge.resize(ntris);
    for (uint32_t slot = 0; slot < ntris; slot++) {
        TriRec r = B.rec[B.order[slot]];
        B.slot_of_tri[B.order[slot]] = (int32_t)slot;
        const int ro = B.rot[B.order[slot]];     // the slot's corner 0 is input corner `ro` (cyclic: same triangle, same orientation)
        if (ro) {
            const TriRec in = r;
            for (int k = 0; k < 3; k++) { r.p[k] = in.p[(k + ro) % 3]; r.n[k] = in.n[(k + ro) % 3]; r.uv[k][0] = in.uv[(k + ro) % 3][0]; r.uv[k][1] = in.uv[(k + ro) % 3][1]; }
        }
        plane_record(r.p, &B.isect[3 * (size_t)slot], &B.wedge[slot]);
        float4 *q = &B.shade[8 * (size_t)slot];
        q[0] = make_float4(r.p[0].x, r.p[0].y, r.p[0].z, r.uv[0][0]);
        q[1] = make_float4(r.p[1].x, r.p[1].y, r.p[1].z, r.uv[0][1]);
        q[2] = make_float4(r.p[2].x, r.p[2].y, r.p[2].z, r.uv[1][0]);
        q[3] = make_float4(r.n[0].x, r.n[0].y, r.n[0].z, r.uv[1][1]);
        q[4] = make_float4(r.n[1].x, r.n[1].y, r.n[1].z, r.uv[2][0]);
        q[5] = make_float4(r.n[2].x, r.n[2].y, r.n[2].z, r.uv[2][1]);
        float fi, fp; memcpy(&fi, &r.inst, 4); memcpy(&fp, &r.prim, 4);
        q[6] = make_float4(r.ng.x, r.ng.y, r.ng.z, fi);
        float fr; memcpy(&fr, &ro, 4);
        q[7] = make_float4(r.area, fp, fr, 0.0f);          // .z: rotation of the slot's corners against the input triangle's
    }
    if (B.use_bvh) return;
    // brute-force loops test two PRIMITIVES per trip with packed fp32 math, a primitive being a quad (slots 2q, 2q + 1)
    // or a single triangle: plane N of the (first) triangle and four edge functions — u and v of both triangles of a quad,
    // or u, v, w, w of a single triangle — five float4, interleaved for the two halves of a float2
    B.pairs.assign(40 * (((size_t)s->nquads + 1) / 2), 0.0f);
    for (uint32_t q = 0; q < s->nquads; q++) {
        const uint32_t a = q < s->nquads2 ? 2 * q : q + s->nquads2;
        float4 src[5] = {B.isect[3 * (size_t)a], B.isect[3 * (size_t)a + 1], B.isect[3 * (size_t)a + 2], B.wedge[a], B.wedge[a]};
        if (q < s->nquads2) { src[3] = B.isect[3 * (size_t)(a + 1) + 1]; src[4] = B.isect[3 * (size_t)(a + 1) + 2]; }
        float *dst = &B.pairs[40 * (size_t)(q / 2) + (q & 1)];
        for (int k = 0; k < 20; k++) dst[2 * k] = ((const float *)src)[k];
    }
    // pairs of two PARALLELOGRAMS (they come first): the outer edges of the second triangle are 1 - u and 1 - v of the first,
    // so the record is the plane and two edge functions — six float4
    const size_t nppairs = s->npar / 2;
    B.ppairs.assign(24 * std::max<size_t>(nppairs, 1), 0.0f);
    for (uint32_t q = 0; q < 2 * nppairs; q++) {
        const float *src = (const float *)&B.isect[3 * (size_t)(2 * q)];
        float *dst = &B.ppairs[24 * (size_t)(q / 2) + (q & 1)];
        for (int k = 0; k < 12; k++) dst[2 * k] = src[k];
    }
    s->ds.nppairs = getenv("ZDR_NO_PARALLELOGRAMS") ? 0 : (int32_t)nppairs;
}

// 4. upload, and the device's view of the scene (DScene)
static int upload_scene(zdr_scene *s, const SceneBuild &B) {
    std::vector<int32_t> lights; int light_count = 0;
    light_list(s->emission, s->ninst, lights, light_count);
    hipError_t e = hipSuccess;
    auto up = [&](DevBuf &dst, const void *src, size_t bytes) { if (e == hipSuccess) e = upload(dst, src, bytes, &s->device_bytes); };
    // BVH: nodes and plane records share ONE allocation, nodes first — the walk then addresses whatever a lane stands on as
    // base + a 32-bit byte offset (accel.h, fetch): no 64-bit address arithmetic, no branch between "node" and "triangle" pointers.
    const bool one_block = B.use_bvh;
    if (one_block) {
        if ((B.nodes.size() + B.isect.size()) * sizeof(float4) >= (1ull << 32)) return fail(ZDR_E_UNSUPPORTED, "BVH nodes and triangle records exceed 4 GiB");
        std::vector<float4> both(B.nodes); both.insert(both.end(), B.isect.begin(), B.isect.end());
        up(s->d_nodes, both.data(), both.size() * sizeof(float4));
    } else {
        up(s->d_isect, B.isect.data(), B.isect.size() * sizeof(float4));
        up(s->d_pairs, B.pairs.data(), B.pairs.size() * sizeof(float));
        up(s->d_ppairs, B.ppairs.data(), B.ppairs.size() * sizeof(float));
    }
    up(s->d_shade, B.shade.data(), B.shade.size() * sizeof(float4));
    if (!one_block) up(s->d_nodes, B.nodes.data(), B.nodes.size() * sizeof(float4));
    up(s->d_emission, s->emission.data(), s->emission.size() * sizeof(float));
    up(s->d_light_insts, lights.data(), lights.size() * sizeof(int32_t));
    up(s->d_inst_tri_begin, s->inst_tri_begin.data(), s->inst_tri_begin.size() * sizeof(int32_t));
    up(s->d_slot_of_tri, B.slot_of_tri.data(), B.slot_of_tri.size() * sizeof(int32_t));
    if (e == hipSuccess) e = s->d_counters.alloc(8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = s->d_error.alloc(sizeof(unsigned int));
    if (e == hipSuccess) e = hipMemset(s->d_error, 0, sizeof(unsigned int));
    if (e != hipSuccess) return fail(ZDR_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    s->ds.isect = one_block ? s->d_nodes + B.nodes.size() : s->d_isect;
    s->ds.pairs = s->d_pairs; s->ds.ppairs = s->d_ppairs; s->ds.shade = s->d_shade; s->ds.nodes = s->d_nodes; s->ds.emission = s->d_emission;
    s->ds.light_insts = s->d_light_insts; s->ds.inst_tri_begin = s->d_inst_tri_begin; s->ds.slot_of_tri = s->d_slot_of_tri;
    s->ds.error_word = s->d_error;
    if (const char *e = getenv("ZDR_DEBUG_BVH_BUDGET")) s->ds.debug_bvh_budget = atoi(e);
    s->ds.nquads = (int32_t)s->nquads; s->ds.nquads2 = (int32_t)s->nquads2;
    s->ds.ntris = (int32_t)s->ntris; s->ds.ninst = (int32_t)s->ninst; s->ds.light_count = light_count; s->ds.nnodes = (int32_t)s->bvh_nodes; s->ds.stack_entries = (int32_t)s->stack_entries;
    const float4 *walk_base = one_block ? s->d_nodes : s->d_isect;
    s->ds.walk_base = (const char *)walk_base; s->ds.isect_off = one_block ? (uint32_t)(B.nodes.size() * sizeof(float4)) : 0u;   // accel.h, fetch
    return upload_light_table(s, lights, light_count, nullptr);
}

// ---- the caller's mesh: every world-space position finite and no larger than ZDR_MAX_COORD (include/zdr.h) = 2^30.
// Why 2^30: the largest power of two L for which nothing the host derives from positions |x|, |y|, |z| <= L can overflow float32
// (FLT_MAX = 2^128 (1 - 2^-24)); an edge component is at most 2 L.
//   plane_record     n = e1 x e2: |n_k| <= 2 (2 L)^2 = 8 L^2;  |N.w| = |n . p0| = |det(p0, p1, p2)| <= (sqrt(3) L)^3 = 5.2 L^3 (Hadamard):
//                    finite up to L = 2^41.  |U| = 1 / (the triangle's height) and U.w = -U . p0 follow the triangle's shape, not L:
//                    a triangle without area has them infinite or NaN at any L, and is never hit (N = 0).
//   build_accel      diag^2 <= 3 (2 L)^2 = 12 L^2: up to 2^62.  SAH cost = area x count <= 24 L^2 x 2^25: up to 2^49.
//   world_records    the FLOAT32 cross product c of two edges, |c_k| <= 8 L^2, and c . c <= 192 L^4 for the area and the geometric
//                    normal: 192 x 2^120 = 1.5 x 2^127 is finite, 192 x 2^124 is not.  This is the one that binds: L = 2^30.
// (A soup scaled by 1e15 built, and then lost every ray to N.w = inf; a coordinate of 1e30 ended in "BVH box quantisation is not
// conservative"; a NaN went through unnoticed.)
static bool position_ok(h3 p) {
    return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && fabsf(p.x) <= ZDR_MAX_COORD && fabsf(p.y) <= ZDR_MAX_COORD && fabsf(p.z) <= ZDR_MAX_COORD;
}
static int bad_position(h3 p, const std::string &who) {       // ZDR_E_INVALID, the message names whose position it is
    char buf[160];
    snprintf(buf, sizeof buf, ": world-space position (%g, %g, %g) %s", (double)p.x, (double)p.y, (double)p.z,
             std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) ? "exceeds ZDR_MAX_COORD = 2^30 in magnitude" : "is not finite");
    return fail(ZDR_E_INVALID, who + buf);
}

extern "C" int zdr_scene_create(const float *verts8, uint32_t nverts, const int32_t *tris, uint32_t ntris,
                                const int32_t *inst_tri_begin, const float *inst_xform, const float *inst_emission,
                                uint32_t ninst, int device, int accel, zdr_scene **out) {
    if (!verts8 || !tris || !inst_tri_begin || !inst_emission || !out) return fail(ZDR_E_INVALID, "null argument");
    if (ntris == 0 || nverts == 0 || ninst == 0) return fail(ZDR_E_INVALID, "empty scene");
    if (ninst > 10000) return fail(ZDR_E_INVALID, "exceeding maximum number of mesh instances");   // render.py:114-115
    if (ntris >= ZDR_MAX_TRIS) return fail(ZDR_E_UNSUPPORTED, "too many triangles: the kernels address the per-triangle records with 32-bit byte offsets (2^25 triangles)");
    if (inst_tri_begin[0] != 0 || (uint32_t)inst_tri_begin[ninst] != ntris) return fail(ZDR_E_INVALID, "inst_tri_begin must span [0, ntris]");
    for (uint32_t i = 0; i < ninst; i++) if (inst_tri_begin[i + 1] < inst_tri_begin[i]) return fail(ZDR_E_INVALID, "inst_tri_begin must be non-decreasing");
    for (size_t i = 0; i < (size_t)ntris * 3; i++) if (tris[i] < 0 || (uint32_t)tris[i] >= nverts) return fail(ZDR_E_INVALID, "triangle index out of range");
    for (uint32_t i = 0; i < ninst; i++) {          // the positions as world_records will make them, before any device is touched
        static const float ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const float *m = inst_xform ? inst_xform + 16 * (size_t)i : ident;
        for (size_t c = 3 * (size_t)inst_tri_begin[i]; c < 3 * (size_t)inst_tri_begin[i + 1]; c++) {
            const float *v = verts8 + 8 * (size_t)tris[c];
            const h3 p = xform_point(m, H3(v[0], v[1], v[2]));
            if (position_ok(p)) continue;
            return bad_position(p, "instance " + std::to_string(i) + ", vertex " + std::to_string(tris[c]) + " (triangle " + std::to_string(c / 3 - (size_t)inst_tri_begin[i]) + " of the instance)");
        }
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ZDR_E_INVALID, "no such HIP device");
    HIPCHK(hipSetDevice(device));

    zdr_scene *s = new zdr_scene();
    s->device = device; s->ntris = ntris; s->nverts = nverts; s->ninst = ninst;
    s->inst_tri_begin.assign(inst_tri_begin, inst_tri_begin + ninst + 1);
    s->emission.assign(inst_emission, inst_emission + 3 * (size_t)ninst);
    SceneBuild B;
    world_records(s, verts8, tris, inst_xform, B);
    int rc = accel_and_slot_order(s, accel, B);
    if (!rc) { slot_records(s, B); rc = upload_scene(s, B); }
    if (rc) { zdr_scene_destroy(s); return rc; }
    *out = s;
    return ZDR_OK;
}

// Host-only view of the acceleration structure (no GPU needed): lets the CPU test-suite run an
// emulation of the device traversal on exactly the data the kernels would see.
extern "C" int zdr_debug_build_accel(const float *tri_xyz, uint32_t ntris, int accel, float *nodes_out, uint32_t nodes_cap,
                                     uint32_t *nnodes, uint32_t *stack_entries, int32_t *order_out, float *isect_out) {
    if (!tri_xyz || !ntris || !nnodes || !order_out || !isect_out) return fail(ZDR_E_INVALID, "null argument");
    const std::vector<h3> pos = triangle_corners(tri_xyz, ntris, 3, 9);
    for (size_t c = 0; c < pos.size(); c++)          // as zdr_scene_create refuses them (no instances here: the triangle and its corner)
        if (!position_ok(pos[c])) return bad_position(pos[c], "triangle " + std::to_string(c / 3) + ", vertex " + std::to_string(c % 3));
    std::vector<int> order; std::vector<float4> nodes; uint32_t nn = 0, depth = 0, se = 8;
    const bool use_bvh = wants_bvh(accel, ntris);
    int rc = build_accel(pos, ntris, use_bvh, order, nodes, nn, depth, se); if (rc) return rc;
    std::vector<int> rot(ntris, 0);
    uint32_t npar = 0;
    if (!use_bvh) { nn = brute_slot_order(pos, ntris, order, rot, &npar); se = npar; }   // brute force: *nnodes = merged quads (slots 2q, 2q + 1), *stack_entries = how many of them are parallelograms (they come first); no nodes
    *nnodes = nn;
    if (stack_entries) *stack_entries = se;
    if (use_bvh) {
        if (nn > nodes_cap) return fail(ZDR_E_NOMEM, "nodes_out too small");
        if (nn) memcpy(nodes_out, nodes.data(), (size_t)nn * 4 * sizeof(float4));
    }
    for (uint32_t slot = 0; slot < ntris; slot++) {
        order_out[slot] = order[slot];
        const int ro = rot[order[slot]];
        h3 c[3]; for (int k = 0; k < 3; k++) c[k] = pos[3 * (size_t)order[slot] + (k + ro) % 3];
        float4 q[3]; plane_record(c, q);
        memcpy(isect_out + 12 * (size_t)slot, q, sizeof q);
    }
    return ZDR_OK;
}

// Host-only: the classification behind the shadow walk's pair mask (never_occluders above), for the CPU test-suite.
extern "C" int zdr_debug_never_occluders(const float *tri_xyz, uint32_t ntris, const uint8_t *is_light_tri, uint8_t *never_out) {
    if (!tri_xyz || !ntris || !is_light_tri || !never_out) return fail(ZDR_E_INVALID, "null argument");
    const std::vector<h3> pos = triangle_corners(tri_xyz, ntris, 3, 9);
    std::vector<uint8_t> light(is_light_tri, is_light_tri + ntris), never;
    never_occluders(pos, ntris, light, never);
    memcpy(never_out, never.data(), ntris);
    return ZDR_OK;
}

extern "C" int zdr_scene_destroy(zdr_scene *s) {
    if (!s) return ZDR_OK;
    (void)hipSetDevice(s->device);
    DevBuf::free_all(*s);
    delete s;
    return ZDR_OK;
}

extern "C" int zdr_scene_info(const zdr_scene *s, zdr_scene_info_t *info) {
    if (!s || !info) return fail(ZDR_E_INVALID, "null argument");
    info->ntris = s->ntris; info->nverts = s->nverts; info->ninst = s->ninst; info->light_count = (uint32_t)s->ds.light_count;
    info->accel = s->accel_is_bvh ? ZDR_ACCEL_BVH : ZDR_ACCEL_BRUTE;
    info->bvh_nodes = s->bvh_nodes; info->bvh_max_depth = s->bvh_depth; info->bvh_stack_entries = s->stack_entries; info->device = s->device; info->device_bytes = s->device_bytes;
    return ZDR_OK;
}

extern "C" int zdr_scene_set_emissions(zdr_scene *s, const float *inst_emission, void *stream) {
    if (!s || !inst_emission) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    s->emission.assign(inst_emission, inst_emission + 3 * (size_t)s->ninst);
    std::vector<int32_t> lights; int count = 0;
    light_list(s->emission, s->ninst, lights, count);
    hipStream_t st = (hipStream_t)stream;
    // pageable sources: these copies return once the data is staged, so the vectors may go out of scope
    HIPCHK(hipMemcpyAsync(s->d_emission, s->emission.data(), s->emission.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_light_insts, lights.data(), lights.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    s->ds.light_count = count;
    return upload_light_table(s, lights, count, st);
}

extern "C" int zdr_scene_set_emission_values(zdr_scene *s, const float *emission, void *stream) {
    if (!s || !emission) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    // in place, stream-ordered, by a kernel: the light list, the table's layout and every pointer stay as they are (the host copy of the
    // emissions, which only zdr_scene_set_emissions reads back, is not touched: that call replaces all of it)
    if (zdr_launch_set_emission_values(s->ds, emission, s->d_emission, s->d_emission4, s->d_light_tris, (hipStream_t)stream))
        return fail(ZDR_E_HIP, "emission kernel launch failed");
    return ZDR_OK;
}

extern "C" int zdr_scene_set_material_slots(zdr_scene *s, const int32_t *inst_slot, void *stream) {
    if (!s || !inst_slot) return fail(ZDR_E_INVALID, "null argument");
    for (uint32_t i = 0; i < s->ninst; i++)
        if (inst_slot[i] < -1 || inst_slot[i] >= ZDR_MAX_MATERIALS)
            return fail(ZDR_E_INVALID, "instance " + std::to_string(i) + ": material slot " + std::to_string(inst_slot[i]) + " outside [-1, " + std::to_string(ZDR_MAX_MATERIALS) + ")");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (!s->d_inst_slot) {
        if (stream_is_capturing(st)) return fail(ZDR_E_UNSUPPORTED, "the material-slot table would have to be allocated while the stream is capturing");
        if (int rc = s->d_inst_slot.reserve(std::max<size_t>(16, (size_t)s->ninst * sizeof(int32_t)), false, "material-slot")) return rc;   // (`false`: refused above, in this call's own words)
        s->device_bytes += (size_t)s->ninst * sizeof(int32_t);
    }
    s->inst_slot.assign(inst_slot, inst_slot + s->ninst);
    HIPCHK(hipMemcpyAsync(s->d_inst_slot, s->inst_slot.data(), (size_t)s->ninst * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZDR_OK;
}

extern "C" int zdr_scene_set_envmap(zdr_scene *s, const float *tex, uint32_t tex_h, uint32_t tex_w, const float *alias_prob,
                                    const int32_t *alias_idx, const float *pdf, uint32_t map_w, uint32_t map_h) {
    if (!s) return fail(ZDR_E_INVALID, "null scene");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());     // nothing in flight may still read the old tables
    s->d_env_tex.release(); s->d_alias_prob.release(); s->d_alias_idx.release(); s->d_env_pdf.release();
    s->ds.env_count = 0; s->ds.env_tex = nullptr; s->ds.alias_prob = nullptr; s->ds.alias_idx = nullptr; s->ds.env_pdf = nullptr;
    if (!tex) return ZDR_OK;
    if (!alias_prob || !alias_idx || !pdf || !tex_h || !tex_w || !map_w || !map_h) return fail(ZDR_E_INVALID, "bad envmap arguments");
    size_t n_alias = (size_t)map_h + (size_t)map_h * map_w;
    for (size_t i = 0; i < n_alias; i++) {
        size_t lim = i < map_h ? map_h : map_w;
        if (alias_idx[i] < 0 || (size_t)alias_idx[i] >= lim) return fail(ZDR_E_INVALID, "alias index out of range");
    }
    HIPCHK(upload(s->d_env_tex, tex, (size_t)tex_h * tex_w * sizeof(float4), &s->device_bytes));
    HIPCHK(upload(s->d_alias_prob, alias_prob, n_alias * sizeof(float), &s->device_bytes));
    HIPCHK(upload(s->d_alias_idx, alias_idx, n_alias * sizeof(int32_t), &s->device_bytes));
    HIPCHK(upload(s->d_env_pdf, pdf, (size_t)map_w * map_h * sizeof(float), &s->device_bytes));
    s->ds.env_tex = s->d_env_tex; s->ds.alias_prob = s->d_alias_prob; s->ds.alias_idx = s->d_alias_idx; s->ds.env_pdf = s->d_env_pdf;
    s->ds.env_h = (int32_t)tex_h; s->ds.env_w = (int32_t)tex_w; s->ds.map_w = (int32_t)map_w; s->ds.map_h = (int32_t)map_h;
    s->ds.env_count = 1;
    return ZDR_OK;
}

extern "C" int zdr_scene_set_envmap_texture(zdr_scene *s, const float *tex, void *stream) {
    if (!s || !tex) return fail(ZDR_E_INVALID, "null argument");
    if (s->ds.env_count == 0 || !s->d_env_tex) return fail(ZDR_E_INVALID, "the scene has no environment map: zdr_scene_set_envmap first");
    if ((uintptr_t)tex % 16 != 0) return fail(ZDR_E_INVALID, "tex must be 16-byte aligned (one float4 texel per load)");
    HIPCHK(hipSetDevice(s->device));
    // in place, stream-ordered, by a kernel (graph-safe like the zero-fills): the pointer the kernels and any captured graph hold stays valid
    if (zdr_launch_copy(s->d_env_tex, tex, (size_t)s->ds.env_h * (size_t)s->ds.env_w * sizeof(float4), (hipStream_t)stream))
        return fail(ZDR_E_HIP, "copy launch failed");
    return ZDR_OK;
}

// The constants of the table kernels (csrc/envsample.h), in double: the 289 tap weights of the weight map's filter and their sum
// (zdr_amd/envmap.py, weight_map) and the row factors of the MIS compensation (build_tables).
static void envmap_sampling_constants(std::vector<double> &row_factor, std::vector<float> &taps) {
    const int n = ZDR_ENVS_TAPS / 2;
    taps.assign(sizeof(EnvSamplingScratch::taps) / sizeof(float), 0.0f);
    double sum = 0.0;
    for (int dy = -n; dy <= n; dy++)
        for (int dx = -n; dx <= n; dx++) {
            const double ox = dx * 0.125, oy = dy * 0.125;
            const float w = (float)exp(-4.0 * (ox * ox + oy * oy));
            taps[(size_t)(dy + n) * ZDR_ENVS_TAPS + (size_t)(dx + n)] = w;
            sum += (double)w;
        }
    taps[ZDR_ENVS_TAPS * ZDR_ENVS_TAPS] = (float)sum;
    const double pi = 3.14159265358979323846;
    row_factor.assign(ZDR_ENVS_H, 0.0);
    double mean = 0.0;
    for (int y = 0; y < ZDR_ENVS_H; y++) { row_factor[y] = sin((y + 0.5) / ZDR_ENVS_H * pi); mean += row_factor[y]; }
    mean /= ZDR_ENVS_H;
    for (int y = 0; y < ZDR_ENVS_H; y++) row_factor[y] /= mean;
}

extern "C" int zdr_scene_update_envmap_sampling(zdr_scene *s, int compensate_mis, void *stream) {
    if (!s) return fail(ZDR_E_INVALID, "null scene");
    if (s->ds.env_count == 0 || !s->d_env_tex) return fail(ZDR_E_INVALID, "the scene has no environment map: zdr_scene_set_envmap first");
    if (s->ds.map_w != ZDR_ENVS_W || s->ds.map_h != ZDR_ENVS_H)
        return fail(ZDR_E_UNSUPPORTED, "the sampling tables are rebuilt on the device for a " + std::to_string(ZDR_ENVS_W) + " x " + std::to_string(ZDR_ENVS_H) + " sample map only");
    if (!zdr_launch_envmap_sampling)                                 // (weak: csrc/envsample.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the environment-table kernels (zdr_envmap.hip)");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const bool capturing = stream_is_capturing(st);
    if (!s->d_env_scratch) {
        if (capturing) return fail(ZDR_E_INVALID, "the workspace of zdr_scene_update_envmap_sampling would have to be allocated while the stream is capturing: call it once on the handle before capturing");
        std::vector<double> row_factor; std::vector<float> taps;
        envmap_sampling_constants(row_factor, taps);
        HIPCHK(s->d_env_scratch.alloc(sizeof(EnvSamplingScratch)));
        EnvSamplingScratch *d = s->d_env_scratch;
        hipError_t e = hipMemcpy(d->row_factor, row_factor.data(), sizeof d->row_factor, hipMemcpyHostToDevice);   // (device addresses only: d is not read here)
        if (e == hipSuccess) e = hipMemcpy(d->taps, taps.data(), sizeof d->taps, hipMemcpyHostToDevice);
        if (e != hipSuccess) { s->d_env_scratch.release(); return fail(ZDR_E_HIP, std::string("envmap sampling constants: ") + hipGetErrorString(e)); }
        s->device_bytes += sizeof(EnvSamplingScratch);
    }
    if (capturing) s->captured = true;                              // a graph names the tables and the workspace from now on (zdr_scene)
    EnvSamplingArgs A;
    A.tex = s->d_env_tex; A.env_h = s->ds.env_h; A.env_w = s->ds.env_w;
    A.alias_prob = s->d_alias_prob; A.alias_idx = s->d_alias_idx; A.pdf = s->d_env_pdf;
    A.scratch = s->d_env_scratch; A.compensate_mis = compensate_mis ? 1 : 0;
    if (zdr_launch_envmap_sampling(A, st)) return fail(ZDR_E_HIP, "environment-table kernel launch failed");
    return ZDR_OK;
}

extern "C" int zdr_scene_get_envmap_sampling(zdr_scene *s, float *alias_prob, int32_t *alias_idx, float *pdf, void *stream) {
    if (!s || !alias_prob || !alias_idx || !pdf) return fail(ZDR_E_INVALID, "null argument");
    if (s->ds.env_count == 0 || !s->d_alias_prob) return fail(ZDR_E_INVALID, "the scene has no environment map: zdr_scene_set_envmap first");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n_alias = (size_t)s->ds.map_h + (size_t)s->ds.map_h * (size_t)s->ds.map_w;
    HIPCHK(hipMemcpyAsync(alias_prob, s->d_alias_prob, n_alias * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(alias_idx, s->d_alias_idx, n_alias * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pdf, s->d_env_pdf, (size_t)s->ds.map_h * (size_t)s->ds.map_w * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZDR_OK;
}

extern "C" int zdr_scene_set_pmj02bn_tables(zdr_scene *s, const uint32_t *pmj, uint32_t nsets, uint32_t nsamples,
                                            const uint16_t *bn, uint32_t ntex, uint32_t bnres) {
    if (!s || !pmj || !bn || !nsets || !nsamples || !ntex || !bnres) return fail(ZDR_E_INVALID, "bad table arguments");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());     // nothing in flight may still read the old tables
    // only the sampler tables belong to this setter (the environment buffers are zdr_scene_set_envmap's)
    s->d_pmj.release(); s->d_bn.release();
    memset(&s->tab, 0, sizeof s->tab);
    HIPCHK(upload(s->d_pmj, pmj, (size_t)nsets * nsamples * 2 * sizeof(uint32_t), &s->device_bytes));
    HIPCHK(upload(s->d_bn, bn, (size_t)ntex * bnres * bnres * sizeof(uint16_t), &s->device_bytes));
    s->tab.pmj = s->d_pmj; s->tab.bn = s->d_bn; s->tab.nsets = nsets; s->tab.nsamples = nsamples; s->tab.ntex = ntex; s->tab.bnres = bnres;
    return ZDR_OK;
}

// ------------------------------------------------------------------------- launch set-up
static uint32_t smear(uint32_t w) { w |= w >> 1; w |= w >> 2; w |= w >> 4; w |= w >> 8; w |= w >> 16; return w; }
static bool is_pow2(uint32_t x) { return x && !(x & (x - 1)); }

static int make_sampler_cfg(const zdr_scene *s, int32_t sampler, uint32_t seed, uint32_t spp, SamplerCfg &C) {
    if (spp == 0) return fail(ZDR_E_INVALID, "spp must be positive");
    memset(&C, 0, sizeof C);
    C.kind = sampler; C.seed = seed; C.spp = spp; C.w = smear(spp - 1);
    // CMJ strata grid: res x res for perfect squares (corrmj.py:67), else res_x * res_y >= spp
    uint32_t res = (uint32_t)(int)sqrtf((float)spp + 0.4f);
    if (res < 1) res = 1;
    if (res * res == spp) { C.res_x = C.res_y = res; }
    else if (is_pow2(spp)) { uint32_t lg = 0; while ((1u << lg) < spp) lg++; C.res_x = 1u << ((lg + 1) / 2); C.res_y = spp / C.res_x; }
    else { uint32_t m = res; while (m * m < spp) m++; C.res_x = m; C.res_y = (spp + m - 1) / m; }
    C.resw_x = smear(C.res_x - 1); C.resw_y = smear(C.res_y - 1);
    C.spp_pow2 = is_pow2(spp); C.res_pow2 = is_pow2(C.res_x) && is_pow2(C.res_y);
    C.inv_spp = 1.0f / (float)spp; C.inv_res_x = 1.0f / (float)C.res_x; C.inv_res_y = 1.0f / (float)C.res_y;
    C.res_x_shift = 0; while ((1u << C.res_x_shift) < C.res_x) C.res_x_shift++;
    if (sampler == ZDR_SAMPLER_PMJ02BN) {
        if (!s->d_pmj || !s->d_bn) return fail(ZDR_E_UNSUPPORTED, "PMJ02bn sampler needs tables: call zdr_scene_set_pmj02bn_tables (the reference's own tables are absent)");
        if (spp > s->tab.nsamples) return fail(ZDR_E_INVALID, "spp exceeds the PMJ02bn table length");
        C.tab = s->tab;
    } else if (sampler != ZDR_SAMPLER_CMJ) return fail(ZDR_E_INVALID, "unknown sampler");
    return ZDR_OK;
}

// The struct grows with the library: a caller built against another header says so in struct_size instead of having the
// library read past (or short of) what it passed.  Checked before anything else looks at the parameters.
static int check_params_abi(const zdr_render_params *p) {
    if (p->struct_size != sizeof(zdr_render_params))
        return fail(ZDR_E_INVALID, "zdr_render_params.struct_size is " + std::to_string(p->struct_size) + ", this library (ABI " + std::to_string(ZDR_ABI_VERSION) +
                                   ") expects " + std::to_string(sizeof(zdr_render_params)) + ": caller and library were built from different include/zdr.h");
    return ZDR_OK;
}

// few texels: replicate the staging cells so that the launch's atomics do not pile up on a handful of addresses (scene.h)
static int32_t cell_copies_for(size_t ncells) {
    return (ncells < (1u << 16)) ? (int32_t)std::min<size_t>(ZDR_MAX_CELL_COPIES, (1u << 20) / ncells) : 1;
}

// KernelIO::wide_offsets: 32-bit byte offsets reach every texel of `texels` float4 and every pixel of the image.  ZDR_WIDE_OFFSETS=1
// (read per launch) forces the 64-bit form, ZDR_LOG_OFFSETS=1 reports the choice on stderr: for the tests of the two forms.
static int32_t wide_offsets_for(size_t texels, size_t pixels) {
    const char *force = getenv("ZDR_WIDE_OFFSETS"), *log = getenv("ZDR_LOG_OFFSETS");
    const int32_t wide = (force && atoi(force) != 0) || texels * sizeof(float4) > (1ull << 32) || pixels * sizeof(float4) > (1ull << 32);
    if (log && atoi(log) != 0) fprintf(stderr, "[zdr offsets] wide=%d texels=%zu pixels=%zu\n", (int)wide, texels, pixels);
    return wide;
}

// The camera's frame as every kernel takes it: a render (RenderCfg) and the view buffer of zdr_scene_texel_view (ProjViewArgs), which
// inverts pixel_ray and must do so with the very floats the ray was made from.
static void camera_frame(const zdr_camera &cam, float o[3], float f[3], float r[3], float u[3], float &tan_half) {
    h3 origin = H3(cam.origin[0], cam.origin[1], cam.origin[2]);
    h3 target = H3(cam.target[0], cam.target[1], cam.target[2]);
    h3 up = H3(cam.up[0], cam.up[1], cam.up[2]);
    h3 fwd = hnormalize(hsub(target, origin));                    // camera.py:12-14
    h3 right = hnormalize(hcross(fwd, up));
    h3 upp = hcross(right, fwd);
    o[0] = origin.x; o[1] = origin.y; o[2] = origin.z;
    f[0] = fwd.x; f[1] = fwd.y; f[2] = fwd.z;
    r[0] = right.x; r[1] = right.y; r[2] = right.z;
    u[0] = upp.x; u[1] = upp.y; u[2] = upp.z;
    tan_half = tanf(0.5f * cam.fov);                              // camera.py:15
}

static int make_render_cfg(const zdr_render_params *p, bool backward, RenderCfg &R) {
    { int rc = check_params_abi(p); if (rc) return rc; }
    if (p->integrator < 0 || p->integrator > ZDR_UVGRAD) return fail(ZDR_E_INVALID, "unknown integrator");
    if (p->integrator == ZDR_UVGRAD && backward) return fail(ZDR_E_UNSUPPORTED, "render_duvdxy has no backward pass");
    if (p->width <= 0 || p->height <= 0) return fail(ZDR_E_INVALID, "bad resolution");
    if (p->x0 < 0 || p->y0 < 0 || p->x1 > p->width || p->y1 > p->height || p->x0 > p->x1 || p->y0 > p->y1) return fail(ZDR_E_INVALID, "bad pixel rectangle");
    if (p->sample_begin > p->sample_end || p->sample_end > p->spp) return fail(ZDR_E_INVALID, "bad sample range");
    if (p->tex_h <= 0 || p->tex_w <= 0) return fail(ZDR_E_INVALID, "bad texture size");
    if (p->max_depth < 1) return fail(ZDR_E_INVALID, "max_depth must be >= 1");
    if (p->tile_shard_count > 1 && (p->tile_shard_index < 0 || p->tile_shard_index >= p->tile_shard_count)) return fail(ZDR_E_INVALID, "tile_shard_index must lie in [0, tile_shard_count)");
    if (backward && p->integrator == ZDR_PATH && p->max_depth > ZDR_MAX_RECORDED_DEPTH) return fail(ZDR_E_UNSUPPORTED, "path backward records at most 16 vertices (prb.py:15)");
    memset(&R, 0, sizeof R);
    R.width = p->width; R.height = p->height; R.x0 = p->x0; R.y0 = p->y0; R.x1 = p->x1; R.y1 = p->y1;
    R.sample_begin = p->sample_begin; R.sample_end = p->sample_end;
    R.use_tent = p->use_tent; R.max_depth = p->max_depth; R.rr_depth = p->rr_depth; R.tex_h = p->tex_h; R.tex_w = p->tex_w;
    R.cell_copies = cell_copies_for((size_t)(p->tex_h + 1) * (size_t)(p->tex_w + 1));
    if ((size_t)p->tex_h * (size_t)p->tex_w >= (1ull << 31)) return fail(ZDR_E_UNSUPPORTED, "material of 2^31 texels or more");   // texel indices are ints (tex_footprint)
    R.two_over_w = 2.0f / (float)p->width; R.two_over_h = 2.0f / (float)p->height;
    R.aspect = (float)p->height / (float)p->width;
    R.inv_spp = 1.0f / (float)p->spp;
    R.alpha = (float)(p->sample_end - p->sample_begin) / (float)p->spp;
    camera_frame(p->camera, R.cam_o, R.cam_fwd, R.cam_right, R.cam_upp, R.cam_tan);
    // work decomposition: 8x8 pixel tiles x sample chunks, enough single-wave workgroups to keep
    // 256 CUs x 4 SIMDs busy with several waves each and to let the dispatcher balance uneven tiles
    R.tiles_x = (p->x1 - p->x0 + 7) / 8; R.tiles_y = (p->y1 - p->y0 + 7) / 8;
    uint32_t ns = p->sample_end - p->sample_begin;
    if (p->prb_mode != ZDR_PRB_EXPECTATION && p->prb_mode != ZDR_PRB_DETACHED && p->prb_mode != ZDR_PRB_LITERAL) return fail(ZDR_E_INVALID, "unknown prb_mode");
    R.prb_mode = p->prb_mode;
    R.shard_count = p->tile_shard_count > 1 ? p->tile_shard_count : 1;
    R.shard_index = p->tile_shard_count > 1 ? p->tile_shard_index : 0;
    R.shard_skew = R.shard_count > 1 ? 1 : 0;
    const long all_tiles = (long)R.tiles_x * R.tiles_y;
    R.ntiles = (int32_t)(all_tiles > R.shard_index ? (all_tiles - R.shard_index + R.shard_count - 1) / R.shard_count : 0);
    long tiles = R.ntiles;
    long target_waves = (backward && p->integrator == ZDR_PATH) ? 131072 : 65536;   // (path backward, 4,096 resident waves since the kernel holds 16 per CU: 131072 11.22 ms, 65536 11.40; forward: the finer split is no faster) work items (tile x sample chunk) the persistent waves draw; cbox 512^2 spp 256: 16384 11.3/18.5 ms, 32768 10.7/17.7, 65536 10.25/17.2, 131072 10.2/17.1
    if (const char *e = getenv("ZDR_TARGET_WAVES")) target_waves = std::max(1L, atol(e));
    uint32_t min_chunk = 8;               // = one refill batch; cbox 512^2 forward / backward ms with 16 / 8 / 4: spp 16 1.10 / 0.99 / 1.06, 1.63 / 1.41 / 1.41; spp 64 2.90 / 2.86 / 2.92, 4.35 / 4.12 / 4.16; spp 256 unchanged
    if (const char *e = getenv("ZDR_MIN_CHUNK")) min_chunk = (uint32_t)std::max(1L, atol(e));
    long want = tiles > 0 ? (target_waves + tiles - 1) / tiles : 1;
    long maxc = std::max<long>(1, ns / min_chunk);
    long nchunks = std::max<long>(1, std::min(want, maxc));
    if (p->integrator == ZDR_UVGRAD) nchunks = 1;        // four-channel output, written directly
#ifdef ZDR_MEASURE   // timing-only ablations exist in measurement builds alone (zdr_kernels.hip, ZDR_ABLATE)
    if (const char *e = getenv("ZDR_DEBUG_NO_SCATTER")) R.debug_no_scatter = atoi(e);
#endif
    R.chunk = ns ? (uint32_t)((ns + nchunks - 1) / nchunks) : 1;
    R.nchunks = ns ? (int32_t)((ns + R.chunk - 1) / R.chunk) : 0;
    return ZDR_OK;
}

static int zero_fill(void *p, size_t bytes, hipStream_t st) { return zdr_launch_zero(p, bytes, st) ? fail(ZDR_E_HIP, "zero-fill launch failed") : ZDR_OK; }

// Workspace of the path kernels: one FIFO of ZDR_RING_CAP x 64 parked camera-ray vertices (two float4 each,
// 32 KiB) per persistent workgroup, and the eight item counters the workgroups draw from (zeroed per launch).
static int ensure_ring(zdr_scene *s, hipStream_t st, bool capturing) {
    if (int rc = s->d_ring.reserve((size_t)ZDR_MAX_PERSISTENT_BLOCKS * ZDR_RING_CAP * 2 * 64 * sizeof(float4), capturing, "parked-vertex FIFO")) return rc;
    if (int rc = s->d_work_counters.reserve(8 * sizeof(unsigned int), capturing, "work-counter")) return rc;
    return zero_fill(s->d_work_counters, 8 * sizeof(unsigned int), st);
}

// ncells: cells of one copy ((tex_h + 1) x (tex_w + 1), or MaterialTable::ncells)
// extra_cells: cells behind all copies (the environment map's, zdr_render_backward_env)
static int ensure_cells(zdr_scene *s, const RenderCfg &R, size_t ncells, hipStream_t st, bool capturing, size_t extra_cells = 0) {
    size_t need = ((size_t)R.cell_copies * ncells + extra_cells) * 16 * sizeof(float);
    if (int rc = s->d_cells.reserve(need, capturing, "staging-cell")) return rc;
    return zero_fill(s->d_cells, need, st);
}

// Reads (and clears) the device error word; the stream is synchronised first.  A set bit means a watchdog ended
// work early (zdr_kernels.hip: stall; accel.h: BVH budget): the image / gradient of the calls since the last
// check is incomplete.
static int check_device_error(zdr_scene *s, hipStream_t st) {
    unsigned int h = 0;
    HIPCHK(hipMemcpyAsync(&h, s->d_error, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!h) return ZDR_OK;
    HIPCHK(hipMemsetAsync(s->d_error, 0, sizeof h, st));
    std::string m = "device watchdog tripped:";
    if (h & ZDR_DEVERR_STALL) m += " a persistent path wave stopped without draining its work items;";
    if (h & ZDR_DEVERR_BVH_BUDGET) m += " a BVH walk exceeded its iteration budget;";
    if (h & ZDR_DEVERR_POOL) m += " a backward wave ended with record-pool slots leaked or handed out twice;";
    return fail(ZDR_E_HIP, m + " results since the last check are incomplete");
}

extern "C" int zdr_scene_check(zdr_scene *s, void *stream) {
    if (!s) return fail(ZDR_E_INVALID, "null scene");
    HIPCHK(hipSetDevice(s->device));
    return check_device_error(s, (hipStream_t)stream);
}

// What every zdr_render_*_materials entry point checks first: its buffers and `dims` are there, nmat is in range
static int check_table_args(bool buffers, const int32_t *dims, uint32_t nmat) {
    if (!buffers || !dims) return fail(ZDR_E_INVALID, "null argument");
    if (nmat < 1 || nmat > ZDR_MAX_MATERIALS) return fail(ZDR_E_INVALID, "nmat is " + std::to_string(nmat) + ", must lie in [1, " + std::to_string(ZDR_MAX_MATERIALS) + "]");
    return ZDR_OK;
}

// The material table of a zdr_render_*_materials call (internal.h): materials packed in order, their cells likewise.
// (dims and nmat have passed check_table_args.)
static int pack_material_table(const int32_t *dims, uint32_t nmat, MaterialTable &mt) {
    memset(&mt, 0, sizeof mt);
    size_t texel = 0, cells = 0;
    for (uint32_t k = 0; k < nmat; k++) {
        const int32_t h = dims[2 * k], w = dims[2 * k + 1];
        if (h < 1 || w < 1) return fail(ZDR_E_INVALID, "material " + std::to_string(k) + " is " + std::to_string(h) + " x " + std::to_string(w) + ": every dimension must be >= 1");
        mt.m[k].texel = (int32_t)texel; mt.m[k].h = h; mt.m[k].w = w; mt.m[k].cell = (int32_t)cells;
        texel += (size_t)h * (size_t)w; cells += (size_t)(h + 1) * (size_t)(w + 1);
        if (texel >= (1ull << 31) || cells >= (1ull << 26)) return fail(ZDR_E_UNSUPPORTED, "materials too large for one material-table call (2^31 texels, 2^26 staging cells)");
    }
    mt.nmat = (int32_t)nmat; mt.ncells = (int32_t)cells;
    return ZDR_OK;
}
// ... and the scene's slot table with it: what a render call hands its kernels.
static int make_material_table(zdr_scene *s, const int32_t *dims, uint32_t nmat, bool capturing, hipStream_t st, MaterialTable &mt) {
    if (int rc = pack_material_table(dims, nmat, mt)) return rc;
    for (size_t i = 0; i < s->inst_slot.size(); i++)
        if (s->inst_slot[i] >= (int32_t)nmat)
            return fail(ZDR_E_INVALID, "instance " + std::to_string(i) + " has material slot " + std::to_string(s->inst_slot[i]) + ", but only " + std::to_string(nmat) + " materials were passed");
    if (!s->d_inst_slot) {                                  // never set: every slot is -1
        if (int rc = may_allocate(capturing, "material-slot")) return rc;
        std::vector<int32_t> none(s->ninst, -1);
        if (int rc = zdr_scene_set_material_slots(s, none.data(), st)) return rc;
    }
    mt.inst_slot = s->d_inst_slot;
    return ZDR_OK;
}

// The slot table of a single-material call that runs in the material-table kernels (an environment gradient): instance 0 has material 0,
// every other instance none — what zdr_render_backward does with instances > 0 (path: light or blocker; direct: its emission).
static int single_material_slots(zdr_scene *s, bool capturing, const int32_t *&out) {
    if (!s->d_inst_slot0) {
        if (int rc = may_allocate(capturing, "material-slot")) return rc;
        std::vector<int32_t> t(s->ninst, -1);
        t[0] = 0;
        HIPCHK(upload(s->d_inst_slot0, t.data(), (size_t)s->ninst * sizeof(int32_t), &s->device_bytes));
    }
    out = s->d_inst_slot0;
    return ZDR_OK;
}

// Staging cells of a material table (scene.h, few texels).  At most ZDR_LDS_CELLS cells in all: the kernels keep the whole array in LDS and
// add it into copy blockIdx % R.cell_copies of it, every material copied alike.  Otherwise each material has copies of its own, sized by
// its own cells (a share of the budget of cell_copies_for), laid out one after the other; R.cell_copies = 1 and mt.ncells = all cells.
// (Copies sized by the total left a 1 x 1 material beside a 1024 x 1024 texture with one copy of its 4 cells: 3.4 % off at 512^2 spp 256.)
static void material_cell_layout(MaterialTable &mt, RenderCfg &R) {
    if (mt.ncells <= ZDR_LDS_CELLS) {
        R.cell_copies = cell_copies_for((size_t)mt.ncells);
        for (int k = 0; k < mt.nmat; k++) { mt.m[k].copies = R.cell_copies; mt.m[k].stride = mt.ncells; }
        return;
    }
    size_t cell = 0;
    for (int pass = 0; pass < 2; pass++) {                  // pass 1: one copy each, if the copies would pass 2^26 cells
        cell = 0;
        for (int k = 0; k < mt.nmat; k++) {
            const size_t one = (size_t)(mt.m[k].h + 1) * (size_t)(mt.m[k].w + 1);
            const size_t copies = (pass == 0 && one < (1u << 16)) ? std::min<size_t>(ZDR_MAX_CELL_COPIES, std::max<size_t>(1, ((1u << 20) / (size_t)mt.nmat) / one)) : 1;
            mt.m[k].cell = (int32_t)cell; mt.m[k].copies = (int32_t)copies; mt.m[k].stride = (int32_t)one;
            cell += copies * one;
        }
        if (cell < (1ull << 26)) break;
    }
    R.cell_copies = 1;
    mt.ncells = (int32_t)cell;
}

// Environment gradient: the map as entry ZDR_ENV_ENTRY of a material table whose materials material_cell_layout has laid out.
// The map's cells follow every copy of the materials' cells, with copies of their own (scene.h, table_cell_env): most light
// samples go to the map's few brightest texels, whatever the map's size, so even a large map gets copies — up to
// ZDR_ENV_CELL_BUDGET cells in all (16 MiB per copy for a 512 x 512 map: 15 copies).  Entry ZDR_ENV_ENTRY = {copies, h, w, first cell};
// env_cells_total = the map's cells, all their copies.
static int env_cell_layout(const zdr_scene *s, MaterialTable &mt, const RenderCfg &R, size_t &env_cells_total) {
    const size_t mat_cells = (size_t)R.cell_copies * (size_t)mt.ncells;
    const size_t one = (size_t)(s->ds.env_h + 1) * (size_t)(s->ds.env_w + 1);
    size_t copies = std::min<size_t>(ZDR_MAX_CELL_COPIES, std::max<size_t>(1, ZDR_ENV_CELL_BUDGET / one));
    if (mat_cells + one >= (1ull << 26)) return fail(ZDR_E_UNSUPPORTED, "materials and environment map too large for one call (2^26 staging cells)");
    copies = std::min<size_t>(copies, ((1ull << 26) - 1 - mat_cells) / one);
    mt.m[ZDR_ENV_ENTRY].texel = (int32_t)copies; mt.m[ZDR_ENV_ENTRY].h = s->ds.env_h; mt.m[ZDR_ENV_ENTRY].w = s->ds.env_w;
    mt.m[ZDR_ENV_ENTRY].cell = (int32_t)mat_cells;
    env_cells_total = copies * one;
    return ZDR_OK;
}

// One render call as the entry points describe it to render_common.
struct RenderCall {
    const float *material = nullptr;                    // the material, or the packed materials of a material-table call
    const int32_t *dims = nullptr; uint32_t nmat = 0;   // material-table call (zdr_render_*_materials; both have passed check_table_args), else nullptr / 0
    float *image = nullptr;                             // forward
    bool backward = false, stats = false;
    const float *d_image = nullptr; float *d_material = nullptr;   // backward
    // backward, path / direct, optional and never both: also the gradient of the environment map, through the material-table kernels with the
    // map as entry ZDR_ENV_ENTRY / of the lights' emissions, through the material-table kernels' emission forms.  A single material becomes
    // a table of one.
    float *d_env = nullptr, *d_emission = nullptr;
    // feature buffers (zdr_render_aovs / zdr_render_aovs_backward): a material-table call whose image / d_image are (H, W, ZDR_AOV_CHANNELS)
    // and whose kernels are k_aov / k_aov_bwd, whatever integrator the parameters name
    bool aov = false;
    void *stream = nullptr;
};

static int render_common(zdr_scene *s, const zdr_render_params *p, const RenderCall &call) {
    const bool backward = call.backward, stats = call.stats;
    const hipStream_t st = (hipStream_t)call.stream;
    if (!s || !p || !call.material) return fail(ZDR_E_INVALID, "null argument");
    if (call.d_env && call.d_emission) return fail(ZDR_E_UNSUPPORTED, "the environment gradient and the emission gradient cannot be taken in one call");
    int rc = check_params_abi(p); if (rc) return rc;
    HIPCHK(hipSetDevice(s->device));
    const bool use_mt = call.dims != nullptr;
    const bool env_grad = backward && call.d_env;            // (the scene has a map: render_backward_call)
    const bool emit_grad = backward && call.d_emission && s->ds.light_count > 0;   // a scene without lights has no such term: the plain call
    const bool table_form = use_mt || env_grad || emit_grad;   // the call runs in the material-table kernels
    if (emit_grad && p->integrator != ZDR_PATH && p->integrator != ZDR_DIRECT) return fail(ZDR_E_UNSUPPORTED, "an emission gradient needs the path or the direct integrator");
    if (env_grad) {
        if (p->integrator != ZDR_PATH && p->integrator != ZDR_DIRECT) return fail(ZDR_E_UNSUPPORTED, "an environment gradient needs the path or the direct integrator");
        if (use_mt && call.nmat > ZDR_ENV_ENTRY) return fail(ZDR_E_UNSUPPORTED, "an environment gradient takes at most " + std::to_string(ZDR_ENV_ENTRY) + " materials (the map is the last entry of the material table)");
    }
    zdr_render_params pm = *p;
    if (use_mt) {                                       // the materials' sizes come from the table
        if (p->integrator == ZDR_UVGRAD) return fail(ZDR_E_UNSUPPORTED, "render_duvdxy has no material-table form");
        pm.tex_h = pm.tex_w = 1;
    }
    RenderCfg R; SamplerCfg C;
    rc = make_render_cfg(&pm, backward != 0, R); if (rc) return rc;
    rc = make_sampler_cfg(s, p->sampler, p->seed, p->spp, C); if (rc) return rc;
    if (call.aov) { R.chunk = p->spp; R.nchunks = 1; }  // a lane owns its pixel's whole sum (and its first hit)
    const bool capturing = stream_is_capturing(st);
    MaterialTable mt; memset(&mt, 0, sizeof mt);
    if (use_mt) {
        rc = make_material_table(s, call.dims, call.nmat, capturing, st, mt); if (rc) return rc;
    } else if (table_form) {                            // the one material as a table of one
        mt.m[0].texel = 0; mt.m[0].h = R.tex_h; mt.m[0].w = R.tex_w; mt.m[0].cell = 0;
        mt.nmat = 1; mt.ncells = (R.tex_h + 1) * (R.tex_w + 1);
        rc = single_material_slots(s, capturing, mt.inst_slot); if (rc) return rc;
    }
    size_t env_cells_total = 0;                         // environment gradient: the map's cells, all their copies
    if (table_form) {
        R.tex_h = R.tex_w = 0;                          // (unused in material-table mode)
        material_cell_layout(mt, R);                    // the materials' copies: as in the call without the map
    }
    if (env_grad) { rc = env_cell_layout(s, mt, R, env_cells_total); if (rc) return rc; }
    if (capturing) s->captured = true;                  // sticky: a graph may name this handle's buffers from now on (zdr_scene)
    if (backward) { rc = ensure_cells(s, R, table_form ? (size_t)mt.ncells : (size_t)(R.tex_h + 1) * (R.tex_w + 1), st, capturing,
                                      env_cells_total); if (rc) return rc; }
    else if (!stats && R.nchunks > 1) {                 // [chunk][tile of the shard][lane]
        rc = s->d_partial.reserve((size_t)R.nchunks * (size_t)R.ntiles * 64 * sizeof(float4), capturing, "chunk-partial"); if (rc) return rc;
    }
    if (p->integrator == ZDR_PATH) {
        if (p->spp > (1u << 25)) return fail(ZDR_E_UNSUPPORTED, "path integrator: spp above 2^25");   // queue entries pack pixel << 26 | bank << 25 | sample
        rc = ensure_ring(s, st, capturing); if (rc) return rc;
    }
    KernelIO io; memset(&io, 0, sizeof io);
    if (emit_grad) {    // the emission-gradient accumulator (internal.h, KernelIO::emit_acc): sized once for every light list the scene can have, zeroed per call
        rc = s->d_emit_acc.reserve((size_t)ZDR_EMISSION_COPIES * 3 * (size_t)s->ninst * sizeof(float), capturing, "emission-accumulator"); if (rc) return rc;
        rc = zero_fill(s->d_emit_acc, (size_t)ZDR_EMISSION_COPIES * 3 * (size_t)s->ds.light_count * sizeof(float), st); if (rc) return rc;
    }
    io.ring = s->d_ring; io.work_counters = s->d_work_counters;
    // brute-force scenes of at most 64 triangle pairs: camera rays test only the pairs their tile can see
    const bool masks = !s->accel_is_bvh && s->ds.ntris <= 128 && p->integrator != ZDR_UVGRAD && !getenv("ZDR_NO_TILE_MASKS");
    if (masks) {
        const size_t need = (size_t)R.tiles_x * R.tiles_y * sizeof(unsigned long long);
        const bool replaced = need > s->d_tile_masks.bytes;
        rc = s->d_tile_masks.reserve(need, capturing, "tile-mask"); if (rc) return rc;
        if (replaced) s->tile_mask_key_set = false;
        io.tile_masks = s->d_tile_masks;
        // the masks depend on the camera and the tile grid only (the geometry of a scene handle never changes):
        // an optimisation loop that renders the same view again does not rebuild them
        float key[24] = {(float)R.x0, (float)R.y0, (float)R.x1, (float)R.y1, (float)R.width, (float)R.height, R.two_over_w, R.two_over_h, R.aspect, R.cam_tan,
                         R.cam_o[0], R.cam_o[1], R.cam_o[2], R.cam_fwd[0], R.cam_fwd[1], R.cam_fwd[2], R.cam_right[0], R.cam_right[1], R.cam_right[2],
                         R.cam_upp[0], R.cam_upp[1], R.cam_upp[2], (float)R.tiles_x, (float)R.tiles_y};
        io.tile_masks_valid = (s->tile_mask_key_set && memcmp(key, s->tile_mask_key, sizeof key) == 0) ? 1 : 0;
        // A captured call must carry its own k_tile_masks (a replay may follow an eager render of another view on this handle), and
        // once a graph exists its replays rewrite the buffer unseen by the host: the key is never trusted again.
        if (s->captured) io.tile_masks_valid = 0;
        // the key is recorded only when k_tile_masks is really going to run: a shard that owns no tile (more shards than
        // tiles) launches nothing, and must not leave the key of masks nobody built behind for the next call
        if ((long)R.ntiles * R.nchunks > 0) { memcpy(s->tile_mask_key, key, sizeof key); s->tile_mask_key_set = true; }
    }
    io.material = (const float4 *)call.material; io.image = (float4 *)call.image; io.partial = s->d_partial;
    if (emit_grad) io.emit_acc = s->d_emit_acc;         // (shares the forward's `partial` pointer: KernelIO keeps its size)
    io.d_image = (const float4 *)call.d_image; io.d_material = call.d_material; io.cells = s->d_cells; io.counters = s->d_counters;
    io.mt = mt;
    {
        size_t texels = (size_t)p->tex_h * (size_t)p->tex_w;    // the material, or every material of the table
        if (use_mt) { texels = 0; for (int k = 0; k < mt.nmat; k++) texels += (size_t)mt.m[k].h * (size_t)mt.m[k].w; }
        io.wide_offsets = wide_offsets_for(texels, (size_t)R.width * (size_t)R.height * (call.aov ? ZDR_AOV_CHANNELS / 4 : 1));
    }
    // every pointer a kernel variant dereferences must be live before anything is launched
    if (backward && (!io.d_image || !io.d_material || !io.cells)) return fail(ZDR_E_INVALID, "backward needs d_image, d_material and the staging cells");
    if (!backward && !stats && !io.image) return fail(ZDR_E_INVALID, "forward needs an image");
    if (!backward && !stats && R.nchunks > 1 && !io.partial) return fail(ZDR_E_NOMEM, "chunk workspace missing");
    if (stats && !io.counters) return fail(ZDR_E_NOMEM, "counter buffer missing");
    if (p->integrator == ZDR_PATH && (!io.ring || !io.work_counters)) return fail(ZDR_E_NOMEM, "path workspace missing");
    if (stats && p->integrator == ZDR_UVGRAD) return fail(ZDR_E_UNSUPPORTED, "no statistics for render_duvdxy");
    DScene S = s->ds;
    // shadow segments end on a light's surface; an environment light sends them to infinity, where nothing can be ruled out
    S.shadow_pairs = (S.env_count > 0) ? ~0ull : s->shadow_pairs;
    const RenderLaunch L = {p->integrator, s->accel_is_bvh, backward, stats, env_grad ? call.d_env : nullptr, emit_grad ? call.d_emission : nullptr, call.aov ? 1 : 0};
    if (zdr_launch_render(S, R, C, io, L, st))
        return fail(ZDR_E_HIP, std::string("kernel launch: ") + hipGetErrorString(hipGetLastError()));
    static const bool check_every_call = getenv("ZDR_CHECK") && atoi(getenv("ZDR_CHECK")) != 0;   // opt-in: costs a synchronise per call
    if (check_every_call && !stats && !capturing) return check_device_error(s, st);   // (a synchronise cannot be captured: zdr_scene_check after the replay instead)
    return ZDR_OK;
}

extern "C" int zdr_render_forward(zdr_scene *s, const zdr_render_params *p, const float *material, float *image, void *stream) {
    if (!image) return fail(ZDR_E_INVALID, "null image");
    RenderCall c; c.material = material; c.image = image; c.stream = stream;
    return render_common(s, p, c);
}

extern "C" int zdr_render_forward_materials(zdr_scene *s, const zdr_render_params *p, const float *materials, const int32_t *dims, uint32_t nmat,
                                            float *image, void *stream) {
    if (int rc = check_table_args(image != nullptr, dims, nmat)) return rc;
    RenderCall c; c.material = materials; c.dims = dims; c.nmat = nmat; c.image = image; c.stream = stream;
    return render_common(s, p, c);
}

// Every zdr_render_backward* entry point.  table: a zdr_render_backward_materials* call (dims, nmat), else one material.  d_env, d_emission:
// the optional target of the *_env / *_emission calls; NULL, or the collocated integrator (which has no environment term and reads no
// emission), makes the call its plain sibling.
static int render_backward_call(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *materials, bool table, const int32_t *dims,
                                uint32_t nmat, float *d_materials, float *d_env, float *d_emission, void *stream) {
    if (d_env && s && s->ds.env_count == 0) return fail(ZDR_E_INVALID, "d_env given, but the scene has no environment map");
    if (p && p->integrator == ZDR_COLLOCATED) d_env = d_emission = nullptr;
    if (table) { if (int rc = check_table_args(d_image && d_materials, dims, nmat)) return rc; }
    else if (!d_image || !d_materials) return fail(ZDR_E_INVALID, "null gradient buffer");
    RenderCall c; c.material = materials; c.backward = true; c.d_image = d_image; c.d_material = d_materials; c.d_env = d_env; c.d_emission = d_emission; c.stream = stream;
    if (table) { c.dims = dims; c.nmat = nmat; }
#ifdef ZDR_MEASURE_STATS   // measurement build (tools/bwd_stats.sh): the path backward kernel counts its trips, sweep iterations and flushes
    if (!table && !d_env && !d_emission) {   // zdr_render_backward, and the *_env / *_emission calls that behave exactly like it
        if (s) { (void)hipSetDevice(s->device); (void)hipMemsetAsync(s->d_counters, 0, 8 * sizeof(unsigned long long), (hipStream_t)stream); }
        int rc = render_common(s, p, c);
        if (!rc) {
            unsigned long long h[8];
            (void)hipMemcpyAsync(h, s->d_counters, sizeof h, hipMemcpyDeviceToHost, (hipStream_t)stream); (void)hipStreamSynchronize((hipStream_t)stream);
            fprintf(stderr, "[bwd stats] trips %llu shaded %llu finished %llu sweep_iterations %llu sweep_steps %llu flushes %llu entries %llu duplicate_cells %llu\n",
                    h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
        }
        return rc;
    }
#endif
    return render_common(s, p, c);
}

extern "C" int zdr_render_backward(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *material,
                                   float *d_material, void *stream) {
    return render_backward_call(s, p, d_image, material, false, nullptr, 0, d_material, nullptr, nullptr, stream);
}

extern "C" int zdr_render_backward_materials(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *materials,
                                             const int32_t *dims, uint32_t nmat, float *d_materials, void *stream) {
    return render_backward_call(s, p, d_image, materials, true, dims, nmat, d_materials, nullptr, nullptr, stream);
}

extern "C" int zdr_render_backward_env(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *material,
                                       float *d_material, float *d_env, void *stream) {
    return render_backward_call(s, p, d_image, material, false, nullptr, 0, d_material, d_env, nullptr, stream);
}

extern "C" int zdr_render_backward_materials_env(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *materials,
                                                 const int32_t *dims, uint32_t nmat, float *d_materials, float *d_env, void *stream) {
    return render_backward_call(s, p, d_image, materials, true, dims, nmat, d_materials, d_env, nullptr, stream);
}

extern "C" int zdr_render_backward_emission(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *material,
                                            float *d_material, float *d_emission, void *stream) {
    return render_backward_call(s, p, d_image, material, false, nullptr, 0, d_material, nullptr, d_emission, stream);
}

extern "C" int zdr_render_backward_materials_emission(zdr_scene *s, const zdr_render_params *p, const float *d_image, const float *materials,
                                                      const int32_t *dims, uint32_t nmat, float *d_materials, float *d_emission, void *stream) {
    return render_backward_call(s, p, d_image, materials, true, dims, nmat, d_materials, nullptr, d_emission, stream);
}

// The parameters of a feature-buffer call as render_common takes them: the integrator and its settings are ignored (include/zdr.h), so
// valid ones stand in — the collocated integrator's, which needs no path workspace.  The whole sample range only.
static int aov_params(const zdr_render_params *p, zdr_render_params &out) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = check_params_abi(p)) return rc;
    if (p->sample_begin != 0 || p->sample_end != p->spp)
        return fail(ZDR_E_UNSUPPORTED, "feature buffers take the whole sample range [0, spp): the instance channel has no partial form");
    out = *p;
    out.integrator = ZDR_COLLOCATED; out.max_depth = 1; out.rr_depth = 0; out.prb_mode = ZDR_PRB_EXPECTATION;
    return ZDR_OK;
}

extern "C" int zdr_render_aovs(zdr_scene *s, const zdr_render_params *p, const float *materials, const int32_t *dims, uint32_t nmat, float *aovs, void *stream) {
    if (int rc = check_table_args(aovs != nullptr, dims, nmat)) return rc;
    zdr_render_params pa;
    if (int rc = aov_params(p, pa)) return rc;
    RenderCall c; c.material = materials; c.dims = dims; c.nmat = nmat; c.image = aovs; c.aov = true; c.stream = stream;
    return render_common(s, &pa, c);
}

extern "C" int zdr_render_aovs_backward(zdr_scene *s, const zdr_render_params *p, const float *d_aovs, const float *materials, const int32_t *dims,
                                        uint32_t nmat, float *d_materials, void *stream) {
    if (int rc = check_table_args(d_aovs && d_materials, dims, nmat)) return rc;
    zdr_render_params pa;
    if (int rc = aov_params(p, pa)) return rc;
    RenderCall c; c.material = materials; c.dims = dims; c.nmat = nmat; c.backward = true; c.d_image = d_aovs; c.d_material = d_materials; c.aov = true;
    c.stream = stream;
    return render_common(s, &pa, c);
}

// ------------------------------------------------------------------------------- denoiser
// zdr_denoise / zdr_denoise_backward (include/zdr.h): no scene handle, no allocation, no synchronisation — argument checks, then
// launches of zdr_denoise.hip on the caller's stream.  Workspace: [guides: 2 float4 per pixel][A: 1 float4 per pixel][B: the same,
// from two levels on].  Neither call leaves anything in it that the other reads: both pack the guides themselves, and the adjoint
// recomputes the normalisers D_l.
static int denoise_check(const zdr_denoise_params *p) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_denoise_params))
        return fail(ZDR_E_INVALID, "zdr_denoise_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " +
                                   std::to_string(sizeof(zdr_denoise_params)) + ": caller and library were built from different include/zdr.h");
    if (p->width <= 0 || p->height <= 0) return fail(ZDR_E_INVALID, "zdr_denoise_params: width and height must be positive");
    if (p->levels < 1 || p->levels > ZDR_DENOISE_MAX_LEVELS)
        return fail(ZDR_E_INVALID, "zdr_denoise_params.levels is " + std::to_string(p->levels) + ": between 1 and " + std::to_string(ZDR_DENOISE_MAX_LEVELS));
    if ((uint64_t)p->width * (uint64_t)p->height > (1ull << 30)) return fail(ZDR_E_UNSUPPORTED, "zdr_denoise: more than 2^30 pixels");
    return ZDR_OK;
}

static int denoise_check_pointers(std::initializer_list<const void *> ptrs) {
    for (const void *q : ptrs) {
        if (!q) return fail(ZDR_E_INVALID, "null argument");
        if ((uintptr_t)q % 16) return fail(ZDR_E_INVALID, "zdr_denoise: every pointer must be 16-byte aligned");
    }
    if (!zdr_launch_denoise_guides || !zdr_launch_denoise_level)     // (weak: csrc/denoise.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the denoiser's kernels (zdr_denoise.hip)");
    return ZDR_OK;
}

// [a, a + na) meets one of the other byte ranges (the sizes follow from the parameters, so the header's "must not overlap" is checked)
struct DenoiseRange { const void *p; size_t bytes; };
static bool denoise_overlap(const void *a, size_t na, std::initializer_list<DenoiseRange> others) {
    const uintptr_t a0 = (uintptr_t)a;
    for (const DenoiseRange &r : others) {
        const uintptr_t b0 = (uintptr_t)r.p;
        if (a0 < b0 + r.bytes && b0 < a0 + na) return true;
    }
    return false;
}

static DenoiseCfg denoise_cfg(const zdr_denoise_params *p) {
    DenoiseCfg R;
    R.width = p->width; R.height = p->height;
    R.inv_sn2 = p->sigma_normal > 0.f ? 1.f / (p->sigma_normal * p->sigma_normal) : 0.f;
    R.half_sz = p->sigma_depth > 0.f ? 0.5f * p->sigma_depth : 0.f;
    R.inv_sa2 = p->sigma_albedo > 0.f ? 1.f / (p->sigma_albedo * p->sigma_albedo) : 0.f;
    return R;
}

extern "C" size_t zdr_denoise_workspace_bytes(const zdr_denoise_params *p) {
    if (denoise_check(p)) return 0;
    const size_t n = (size_t)p->width * (size_t)p->height;
    return n * sizeof(float4) * (p->levels > 1 ? 4 : 3);
}

extern "C" int zdr_denoise(const zdr_denoise_params *p, const float *aovs, const float *image, float *out, void *workspace, void *stream) {
    if (int rc = denoise_check(p)) return rc;
    if (int rc = denoise_check_pointers({aovs, image, out, workspace})) return rc;
    const size_t n = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(out, 16 * n, {{image, 16 * n}, {aovs, 64 * n}, {workspace, zdr_denoise_workspace_bytes(p)}}))
        return fail(ZDR_E_INVALID, "zdr_denoise: out must not alias or overlap an input or the workspace");
    if (denoise_overlap(workspace, zdr_denoise_workspace_bytes(p), {{image, 16 * n}, {aovs, 64 * n}}))
        return fail(ZDR_E_INVALID, "zdr_denoise: the workspace must not overlap an input");
    const DenoiseCfg R = denoise_cfg(p);
    hipStream_t st = (hipStream_t)stream;
    float4 *guides = (float4 *)workspace, *buf[2] = {guides + 2 * n, guides + 3 * n};
    if (zdr_launch_denoise_guides(R, (const float4 *)aovs, guides, st)) return fail(ZDR_E_HIP, "denoise guide launch failed");
    const float4 *src = (const float4 *)image;
    for (int l = 0; l < p->levels; l++) {
        float4 *dst = l == p->levels - 1 ? (float4 *)out : buf[l & 1];
        if (zdr_launch_denoise_level(R, ZDR_DENOISE_FILTER, 1 << l, guides, src, dst, st)) return fail(ZDR_E_HIP, "denoise level launch failed");
        src = dst;
    }
    return ZDR_OK;
}

extern "C" int zdr_denoise_backward(const zdr_denoise_params *p, const float *aovs, const float *d_out, float *d_image, void *workspace, void *stream) {
    if (int rc = denoise_check(p)) return rc;
    if (int rc = denoise_check_pointers({aovs, d_out, d_image, workspace})) return rc;
    const size_t n = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(d_image, 16 * n, {{d_out, 16 * n}, {aovs, 64 * n}, {workspace, zdr_denoise_workspace_bytes(p)}}))
        return fail(ZDR_E_INVALID, "zdr_denoise_backward: d_image must not alias or overlap an input or the workspace");
    if (denoise_overlap(workspace, zdr_denoise_workspace_bytes(p), {{d_out, 16 * n}, {aovs, 64 * n}}))
        return fail(ZDR_E_INVALID, "zdr_denoise_backward: the workspace must not overlap an input");
    const DenoiseCfg R = denoise_cfg(p);
    hipStream_t st = (hipStream_t)stream;
    float4 *guides = (float4 *)workspace, *A = guides + 2 * n, *B = guides + 3 * n;
    if (zdr_launch_denoise_guides(R, (const float4 *)aovs, guides, st)) return fail(ZDR_E_HIP, "denoise guide launch failed");
    const float4 *g = (const float4 *)d_out;
    for (int l = p->levels - 1; l >= 0; l--) {                       // K_l^T g = gather of g / D_l
        float4 *dst = l == 0 ? (float4 *)d_image : B;
        if (zdr_launch_denoise_level(R, ZDR_DENOISE_DIVIDE, 1 << l, guides, g, A, st) ||
            zdr_launch_denoise_level(R, ZDR_DENOISE_GATHER, 1 << l, guides, A, dst, st)) return fail(ZDR_E_HIP, "denoise level launch failed");
        g = dst;
    }
    return ZDR_OK;
}

// ------------------------------------------------------------------- texture-space buffers
// zdr_scene_texel_aovs (include/zdr.h): argument checks, then the three launches of zdr_texel.hip on the caller's stream.  The handle is
// only read — the shade records, slot_of_tri, inst_tri_begin and the material-slot table as they are — so nothing is allocated and the
// call can be captured without a call before.  A table that was never set (every slot -1) travels as a null pointer.
static int texel_check_size(int32_t tex_h, int32_t tex_w) {
    if (tex_h <= 0 || tex_w <= 0) return fail(ZDR_E_INVALID, "zdr_scene_texel_aovs: the texture size must be positive");
    if ((uint64_t)tex_h * (uint64_t)tex_w > ZDR_TEXEL_MAX_TEXELS) return fail(ZDR_E_UNSUPPORTED, "zdr_scene_texel_aovs: more than 2^26 texels");
    if (tex_h > ZDR_TEXEL_MAX_DIM || tex_w > ZDR_TEXEL_MAX_DIM) return fail(ZDR_E_UNSUPPORTED, "zdr_scene_texel_aovs: a dimension above 2^24 (lattice points must be exact in float32)");
    return ZDR_OK;
}

extern "C" size_t zdr_texel_aovs_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (texel_check_size(tex_h, tex_w)) return 0;
    return (size_t)tex_h * (size_t)tex_w * sizeof(uint2);
}

extern "C" int zdr_scene_texel_aovs(zdr_scene *s, int32_t material, int32_t tex_h, int32_t tex_w, float *aovs, void *workspace, void *stream) {
    if (!s || !aovs || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if ((uintptr_t)aovs % 16 || (uintptr_t)workspace % 16) return fail(ZDR_E_INVALID, "zdr_scene_texel_aovs: aovs and workspace must be 16-byte aligned");
    if (material < 0 || material >= ZDR_MAX_MATERIALS)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_aovs: material " + std::to_string(material) + " outside [0, " + std::to_string(ZDR_MAX_MATERIALS) + ")");
    if (int rc = texel_check_size(tex_h, tex_w)) return rc;
    const size_t n = (size_t)tex_h * (size_t)tex_w;
    if (denoise_overlap(aovs, 64 * n, {{workspace, 8 * n}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_aovs: aovs must not overlap the workspace");
    if (!zdr_launch_texel_aovs)                                      // (weak: csrc/texel.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space kernels (zdr_texel.hip)");
    HIPCHK(hipSetDevice(s->device));
    TexelArgs A;
    A.shade = s->ds.shade; A.slot_of_tri = s->ds.slot_of_tri; A.inst_tri_begin = s->ds.inst_tri_begin; A.inst_slot = s->d_inst_slot;
    A.ntris = (int32_t)s->ntris; A.material = material; A.tex_h = tex_h; A.tex_w = tex_w;
    A.keys = (uint2 *)workspace; A.aovs = (float4 *)aovs;
    if (zdr_launch_texel_aovs(A, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel feature-buffer launch failed");
    return ZDR_OK;
}

// zdr_scene_texel_tangents (include/zdr.h): zdr_scene_texel_aovs's checks and three launches, then the tangent resolve of zdr_tangent.hip on
// the keys they left in the workspace.  Nothing is allocated; capturable without a call before.
extern "C" int zdr_scene_texel_tangents(zdr_scene *s, int32_t material, int32_t tex_h, int32_t tex_w, float *aovs, float *tangents, void *workspace, void *stream) {
    const char *name = "zdr_scene_texel_tangents";
    if (!s || !aovs || !tangents || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if ((uintptr_t)aovs % 16 || (uintptr_t)tangents % 16 || (uintptr_t)workspace % 16)
        return fail(ZDR_E_INVALID, std::string(name) + ": aovs, tangents and workspace must be 16-byte aligned");
    if (material < 0 || material >= ZDR_MAX_MATERIALS)
        return fail(ZDR_E_INVALID, std::string(name) + ": material " + std::to_string(material) + " outside [0, " + std::to_string(ZDR_MAX_MATERIALS) + ")");
    if (int rc = texel_check_size(tex_h, tex_w)) return rc;
    const size_t n = (size_t)tex_h * (size_t)tex_w;
    if (denoise_overlap(aovs, 64 * n, {{workspace, 8 * n}, {tangents, 32 * n}}) || denoise_overlap(tangents, 32 * n, {{workspace, 8 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": aovs, tangents and the workspace must not overlap one another");
    if (!zdr_launch_texel_aovs)                                      // (weak: csrc/texel.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space kernels (zdr_texel.hip)");
    if (!zdr_launch_texel_tangents)                                  // (weak: csrc/tangent.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the UV-tangent kernels (zdr_tangent.hip)");
    HIPCHK(hipSetDevice(s->device));
    TexelArgs A;
    A.shade = s->ds.shade; A.slot_of_tri = s->ds.slot_of_tri; A.inst_tri_begin = s->ds.inst_tri_begin; A.inst_slot = s->d_inst_slot;
    A.ntris = (int32_t)s->ntris; A.material = material; A.tex_h = tex_h; A.tex_w = tex_w;
    A.keys = (uint2 *)workspace; A.aovs = (float4 *)aovs;
    if (zdr_launch_texel_aovs(A, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel feature-buffer launch failed");
    if (zdr_launch_texel_tangents(A, (float4 *)tangents, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the tangent launch failed");
    return ZDR_OK;
}

// ------------------------------------------------------------------- texture-space lighting
// zdr_scene_texel_lighting (include/zdr.h): argument checks, then the three launches of zdr_bake.hip on the caller's stream.  The handle
// is only read — the records, the acceleration structure, the light table and the environment tables as they are — so nothing is
// allocated and the call can be captured without a call before.
static int bake_check_size(int32_t tex_h, int32_t tex_w) {
    if (tex_h <= 0 || tex_w <= 0) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: the texture size must be positive");
    if ((uint64_t)tex_h * (uint64_t)tex_w > ZDR_BAKE_MAX_TEXELS) return fail(ZDR_E_UNSUPPORTED, "zdr_scene_texel_lighting: more than 2^26 texels");
    return ZDR_OK;
}

extern "C" size_t zdr_texel_lighting_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (bake_check_size(tex_h, tex_w)) return 0;
    return ZDR_BAKE_HEADER_BYTES + (((size_t)tex_h * (size_t)tex_w * sizeof(uint32_t) + 15) & ~(size_t)15);
}

extern "C" int zdr_scene_texel_lighting(zdr_scene *s, const zdr_texel_lighting_params *p, const float *texel_aovs, float *out, void *workspace, void *stream) {
    if (!s || !p || !texel_aovs || !out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_texel_lighting_params))
        return fail(ZDR_E_INVALID, "zdr_texel_lighting_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " + std::to_string(sizeof(zdr_texel_lighting_params)));
    if ((uintptr_t)texel_aovs % 16 || (uintptr_t)out % 16 || (uintptr_t)workspace % 16)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: texel_aovs, out and workspace must be 16-byte aligned");
    if (int rc = bake_check_size(p->tex_h, p->tex_w)) return rc;
    if (p->spp == 0) return fail(ZDR_E_INVALID, "spp must be positive");
    if (p->sample_begin >= p->sample_end || p->sample_end > p->spp)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: the sample range [" + std::to_string(p->sample_begin) + ", " + std::to_string(p->sample_end) + ") is empty or not within [0, spp)");
    if (!(p->max_distance > 0.0f)) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: max_distance must be positive");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, wbytes = zdr_texel_lighting_workspace_bytes(p->tex_h, p->tex_w);
    if (denoise_overlap(out, 16 * n, {{workspace, wbytes}, {texel_aovs, 64 * n}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: out must not overlap the workspace or texel_aovs");
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting: the workspace must not overlap texel_aovs");
    SamplerCfg C;
    if (int rc = make_sampler_cfg(s, p->sampler, p->seed, p->spp, C)) return rc;
    if (!zdr_launch_texel_lighting)                                  // (weak: csrc/bake.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space lighting kernels (zdr_bake.hip)");
    HIPCHK(hipSetDevice(s->device));
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;      // every pair: the host proves its mask of never-occluders for origins on the scene's own surfaces only, and these points are the caller's
    BakeArgs B;
    B.texels = (const float4 *)texel_aovs; B.out = (float4 *)out;
    B.count = (uint32_t *)workspace; B.list = (uint32_t *)((char *)workspace + ZDR_BAKE_HEADER_BYTES);
    B.ntexels = (uint32_t)n; B.tex_w = p->tex_w; B.sample_begin = p->sample_begin; B.sample_end = p->sample_end;
    B.inv_spp = 1.0f / (float)p->spp; B.spp_f = (float)p->spp; B.max_distance = p->max_distance;
    if (zdr_launch_texel_lighting(S, s->accel_is_bvh, C, B, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel lighting launch failed");
    return ZDR_OK;
}

// zdr_scene_texel_lighting_backward (include/zdr.h): the forward's checks, then the launches of zdr_bakegrad.hip on the caller's stream.
// The handle is only read here too; the emission accumulator lives in the caller's workspace, so nothing is allocated.
static size_t lgrad_list_bytes(int32_t tex_h, int32_t tex_w) { return ((size_t)tex_h * (size_t)tex_w * sizeof(uint32_t) + 15) & ~(size_t)15; }

extern "C" size_t zdr_texel_lighting_backward_workspace_bytes(zdr_scene *s, int32_t tex_h, int32_t tex_w) {
    if (!s) { fail(ZDR_E_INVALID, "null argument"); return 0; }
    if (bake_check_size(tex_h, tex_w)) return 0;
    const size_t acc = ((size_t)ZDR_LGRAD_COPIES * 3 * (size_t)std::max(s->ds.light_count, 0) * sizeof(float) + 15) & ~(size_t)15;
    return ZDR_BAKE_HEADER_BYTES + lgrad_list_bytes(tex_h, tex_w) + acc;
}

extern "C" int zdr_scene_texel_lighting_backward(zdr_scene *s, const zdr_texel_lighting_params *p, const float *texel_aovs, const float *d_out,
                                                 float *d_emission, float *d_env, void *workspace, void *stream) {
    if (!s || !p || !texel_aovs || !d_out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_texel_lighting_params))
        return fail(ZDR_E_INVALID, "zdr_texel_lighting_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " + std::to_string(sizeof(zdr_texel_lighting_params)));
    if (!d_emission && !d_env) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: neither d_emission nor d_env is given");
    if (d_env && s->ds.env_count <= 0) return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: d_env is given, but the scene has no environment map");
    if ((uintptr_t)texel_aovs % 16 || (uintptr_t)d_out % 16 || (uintptr_t)workspace % 16 || (uintptr_t)d_env % 16 || (uintptr_t)d_emission % 4)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: texel_aovs, d_out, d_env and workspace must be 16-byte aligned, d_emission 4-byte aligned");
    if (int rc = bake_check_size(p->tex_h, p->tex_w)) return rc;
    if (p->spp == 0) return fail(ZDR_E_INVALID, "spp must be positive");
    if (p->sample_begin >= p->sample_end || p->sample_end > p->spp)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: the sample range [" + std::to_string(p->sample_begin) + ", " + std::to_string(p->sample_end) + ") is empty or not within [0, spp)");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, wbytes = zdr_texel_lighting_backward_workspace_bytes(s, p->tex_h, p->tex_w);
    const size_t ebytes = d_emission ? 3 * (size_t)s->ninst * sizeof(float) : 0;
    const size_t mbytes = d_env ? 16 * (size_t)s->ds.env_h * (size_t)s->ds.env_w : 0;
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {d_emission, ebytes}, {d_env, mbytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: the workspace must not overlap texel_aovs, d_out, d_emission or d_env");
    if (d_emission && denoise_overlap(d_emission, ebytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {d_env, mbytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: d_emission must not overlap texel_aovs, d_out or d_env");
    if (d_env && denoise_overlap(d_env, mbytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_lighting_backward: d_env must not overlap texel_aovs or d_out");
    SamplerCfg C;
    if (int rc = make_sampler_cfg(s, p->sampler, p->seed, p->spp, C)) return rc;
    if (!zdr_launch_texel_lighting_backward)                         // (weak: csrc/bakegrad.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space lighting gradient kernels (zdr_bakegrad.hip)");
    const bool emit = d_emission && s->ds.light_count > 0;           // a scene without lights: accepted, nothing to add
    if (!emit && !d_env) return ZDR_OK;
    HIPCHK(hipSetDevice(s->device));
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;      // every pair, as the forward
    LgradArgs G;
    G.texels = (const float4 *)texel_aovs; G.d_out = (const float4 *)d_out; G.d_env = d_env; G.d_emission = emit ? d_emission : nullptr;
    G.count = (uint32_t *)workspace; G.list = (uint32_t *)((char *)workspace + ZDR_BAKE_HEADER_BYTES);
    G.acc = emit ? (float *)((char *)workspace + ZDR_BAKE_HEADER_BYTES + lgrad_list_bytes(p->tex_h, p->tex_w)) : nullptr;
    G.ntexels = (uint32_t)n; G.tex_w = p->tex_w; G.sample_begin = p->sample_begin; G.sample_end = p->sample_end;
    G.inv_spp = 1.0f / (float)p->spp;
    if (int rc = zdr_launch_texel_lighting_backward(S, s->accel_is_bvh, C, G, (hipStream_t)stream))
        return fail(ZDR_E_HIP, "texel lighting backward: launch " + std::to_string(rc / 256) + " of 4 failed: " + hipGetErrorString((hipError_t)(rc % 256)));
    return ZDR_OK;
}

// ------------------------------------------------------------------- bounced light
// zdr_scene_texel_bounce (include/zdr.h): argument checks, then the three launches of zdr_bounce.hip on the caller's stream.  The handle
// is only read — the records, the acceleration structure, the light table, the environment tables and the slot table as they are — and
// the material table travels as a kernel argument, so nothing is allocated and the call can be captured without a call before.  A scene
// whose slot table was never set has no material anywhere: every walk ends at its first vertex, and only then would the table have to
// be created — refused while capturing, as everywhere.
static int bounce_check_size(int32_t tex_h, int32_t tex_w) {
    if (tex_h <= 0 || tex_w <= 0) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: the texture size must be positive");
    if ((uint64_t)tex_h * (uint64_t)tex_w > ZDR_BOUNCE_MAX_TEXELS) return fail(ZDR_E_UNSUPPORTED, "zdr_scene_texel_bounce: more than 2^26 texels");
    return ZDR_OK;
}

extern "C" size_t zdr_texel_bounce_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (bounce_check_size(tex_h, tex_w)) return 0;
    return ZDR_BOUNCE_HEADER_BYTES + (((size_t)tex_h * (size_t)tex_w * sizeof(uint32_t) + 15) & ~(size_t)15);
}

extern "C" int zdr_texel_bounce_lanes_shift(int32_t tex_h, int32_t tex_w, uint32_t sample_begin, uint32_t sample_end) {
    if (bounce_check_size(tex_h, tex_w)) return -1;
    if (sample_begin >= sample_end) { fail(ZDR_E_INVALID, "zdr_texel_bounce_lanes_shift: the sample range is empty"); return -1; }
    return zdr_bounce_lanes_shift((uint32_t)tex_h * (uint32_t)tex_w, sample_end - sample_begin);
}

// the checks and the arguments both entry points share
static int bounce_prepare(zdr_scene *s, const zdr_texel_bounce_params *p, const float *texel_aovs, const float *materials, const int32_t *dims, uint32_t nmat,
                          hipStream_t st, SamplerCfg &C, BounceArgs &B, MaterialTable &mt) {
    if (!s || !p || !texel_aovs) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_texel_bounce_params))
        return fail(ZDR_E_INVALID, "zdr_texel_bounce_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " + std::to_string(sizeof(zdr_texel_bounce_params)));
    if (int rc = check_table_args(materials != nullptr, dims, nmat)) return rc;
    if ((uintptr_t)texel_aovs % 16 || (uintptr_t)materials % 16) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: texel_aovs and materials must be 16-byte aligned");
    if (int rc = bounce_check_size(p->tex_h, p->tex_w)) return rc;
    if (p->spp == 0) return fail(ZDR_E_INVALID, "spp must be positive");
    if (p->sample_begin >= p->sample_end || p->sample_end > p->spp)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: the sample range [" + std::to_string(p->sample_begin) + ", " + std::to_string(p->sample_end) + ") is empty or not within [0, spp)");
    if (p->bounces < 1 || p->bounces > ZDR_BOUNCE_MAX_BOUNCES)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: bounces is " + std::to_string(p->bounces) + ", must lie in [1, " + std::to_string(ZDR_BOUNCE_MAX_BOUNCES) + "]");
    if (int rc = make_sampler_cfg(s, p->sampler, p->seed, p->spp, C)) return rc;
    HIPCHK(hipSetDevice(s->device));
    if (int rc = make_material_table(s, dims, nmat, stream_is_capturing(st), st, mt)) return rc;
    memset(&B, 0, sizeof B);
    B.texels = (const float4 *)texel_aovs; B.materials = (const float4 *)materials;
    B.ntexels = (uint32_t)((size_t)p->tex_h * (size_t)p->tex_w); B.tex_w = p->tex_w; B.sample_begin = p->sample_begin; B.sample_end = p->sample_end;
    B.inv_spp = 1.0f / (float)p->spp; B.spp_f = (float)p->spp; B.bounces = p->bounces;
    size_t texels = 0;
    for (uint32_t k = 0; k < nmat; k++) texels += (size_t)dims[2 * k] * (size_t)dims[2 * k + 1];
    B.wide_offsets = wide_offsets_for(texels, 0);
    return ZDR_OK;
}

extern "C" int zdr_scene_texel_bounce(zdr_scene *s, const zdr_texel_bounce_params *p, const float *texel_aovs, const float *materials, const int32_t *dims,
                                      uint32_t nmat, float *out, void *workspace, void *stream) {
    if (!out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if ((uintptr_t)out % 16 || (uintptr_t)workspace % 16) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: out and workspace must be 16-byte aligned");
    if (!zdr_launch_texel_bounce)                                    // (weak: csrc/bounce.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the bounced-light kernels (zdr_bounce.hip)");
    SamplerCfg C; BounceArgs B; MaterialTable mt;
    if (int rc = bounce_prepare(s, p, texel_aovs, materials, dims, nmat, (hipStream_t)stream, C, B, mt)) return rc;
    const size_t n = B.ntexels, wbytes = zdr_texel_bounce_workspace_bytes(p->tex_h, p->tex_w);
    size_t mbytes = 0;
    for (uint32_t k = 0; k < nmat; k++) mbytes += 16 * (size_t)dims[2 * k] * (size_t)dims[2 * k + 1];
    if (denoise_overlap(out, 16 * n, {{workspace, wbytes}, {texel_aovs, 64 * n}, {materials, mbytes}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: out must not overlap the workspace, texel_aovs or the materials");
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}, {materials, mbytes}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce: the workspace must not overlap texel_aovs or the materials");
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;      // every pair (BruteAccel::any_shadow then gives any()'s answer, which the mask of never-occluders equals bit for bit)
    B.out = (float4 *)out;
    B.count = (uint32_t *)workspace; B.list = (uint32_t *)((char *)workspace + ZDR_BOUNCE_HEADER_BYTES);
    if (zdr_launch_texel_bounce(S, s->accel_is_bvh, C, B, mt, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel bounce launch failed");
    return ZDR_OK;
}

extern "C" int zdr_texel_bounce_dump(zdr_scene *s, const zdr_texel_bounce_params *p, const float *texel_aovs, const float *materials, const int32_t *dims,
                                     uint32_t nmat, const int32_t *queries, uint32_t n, float *out, void *stream) {
    if (n == 0) return ZDR_OK;
    if (!queries || !out) return fail(ZDR_E_INVALID, "null argument");
    if ((uintptr_t)out % 16) return fail(ZDR_E_INVALID, "zdr_texel_bounce_dump: out must be 16-byte aligned");
    if (!zdr_launch_texel_bounce_dump)                               // (weak: csrc/bounce.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the bounced-light kernels (zdr_bounce.hip)");
    SamplerCfg C; BounceArgs B; MaterialTable mt;
    if (int rc = bounce_prepare(s, p, texel_aovs, materials, dims, nmat, (hipStream_t)stream, C, B, mt)) return rc;
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;
    if (zdr_launch_texel_bounce_dump(S, s->accel_is_bvh, C, B, mt, queries, n, out, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel bounce dump launch failed");
    return ZDR_OK;
}

// zdr_scene_texel_bounce_backward (include/zdr.h): the forward's checks, then the launches of zdr_bouncegrad.hip on the caller's stream.  The
// handle is only read here too.  The materials' staging cells, their copies and strides follow material_cell_layout — the rule of every
// material-table backward call, so a 1 x 1 material keeps its copies and the few-texel LDS path —, but they live in the caller's
// workspace behind the list and the emission accumulator: nothing is allocated, and the call can be captured without a call before.
static int bgrad_cell_layout(const int32_t *dims, uint32_t nmat, MaterialTable &mt, int32_t &cell_copies, size_t &cells) {
    if (int rc = pack_material_table(dims, nmat, mt)) return rc;
    RenderCfg R; memset(&R, 0, sizeof R);
    material_cell_layout(mt, R);
    cell_copies = R.cell_copies;
    cells = (size_t)R.cell_copies * (size_t)mt.ncells;
    return ZDR_OK;
}
static size_t bgrad_list_bytes(int32_t tex_h, int32_t tex_w) { return ((size_t)tex_h * (size_t)tex_w * sizeof(uint32_t) + 15) & ~(size_t)15; }
static size_t bgrad_acc_bytes(const zdr_scene *s) { return ((size_t)ZDR_BGRAD_COPIES * 3 * (size_t)std::max(s->ds.light_count, 0) * sizeof(float) + 15) & ~(size_t)15; }

extern "C" size_t zdr_texel_bounce_backward_workspace_bytes(zdr_scene *s, int32_t tex_h, int32_t tex_w, const int32_t *dims, uint32_t nmat) {
    if (!s) { fail(ZDR_E_INVALID, "null argument"); return 0; }
    if (check_table_args(true, dims, nmat)) return 0;
    if (bounce_check_size(tex_h, tex_w)) return 0;
    MaterialTable mt; int32_t copies = 1; size_t cells = 0;
    if (bgrad_cell_layout(dims, nmat, mt, copies, cells)) return 0;
    return ZDR_BOUNCE_HEADER_BYTES + bgrad_list_bytes(tex_h, tex_w) + bgrad_acc_bytes(s) + 64 * cells;
}

extern "C" int zdr_scene_texel_bounce_backward(zdr_scene *s, const zdr_texel_bounce_params *p, const float *texel_aovs, const float *d_out, const float *materials,
                                               const int32_t *dims, uint32_t nmat, float *d_materials, float *d_emission, void *workspace, void *stream) {
    if (!d_out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (!d_materials && !d_emission) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward: neither d_materials nor d_emission is given");
    if ((uintptr_t)d_out % 16 || (uintptr_t)workspace % 16 || (uintptr_t)d_materials % 16 || (uintptr_t)d_emission % 4)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward: d_out, d_materials and workspace must be 16-byte aligned, d_emission 4-byte aligned");
    if (!zdr_launch_texel_bounce_backward)                           // (weak: csrc/bouncegrad.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the bounced-light gradient kernels (zdr_bouncegrad.hip)");
    SamplerCfg C; BounceArgs B; MaterialTable mt;
    if (int rc = bounce_prepare(s, p, texel_aovs, materials, dims, nmat, (hipStream_t)stream, C, B, mt)) return rc;
    int32_t cell_copies = 1; size_t cells = 0;
    {   // the cells of the table bounce_prepare made: the same entries, laid out for a backward call
        RenderCfg R; memset(&R, 0, sizeof R);
        material_cell_layout(mt, R);
        cell_copies = R.cell_copies; cells = (size_t)R.cell_copies * (size_t)mt.ncells;
    }
    const size_t n = B.ntexels, lbytes = bgrad_list_bytes(p->tex_h, p->tex_w), abytes = bgrad_acc_bytes(s);
    const size_t wbytes = ZDR_BOUNCE_HEADER_BYTES + lbytes + abytes + 64 * cells;
    size_t mbytes = 0;
    for (uint32_t k = 0; k < nmat; k++) mbytes += 16 * (size_t)dims[2 * k] * (size_t)dims[2 * k + 1];
    const size_t ebytes = d_emission ? 3 * (size_t)s->ninst * sizeof(float) : 0, dmbytes = d_materials ? mbytes : 0;
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {materials, mbytes}, {d_materials, dmbytes}, {d_emission, ebytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward: the workspace must not overlap texel_aovs, d_out, the materials, d_materials or d_emission");
    if (d_materials && denoise_overlap(d_materials, dmbytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {materials, mbytes}, {d_emission, ebytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward: d_materials must not overlap texel_aovs, d_out, the materials or d_emission");
    if (d_emission && denoise_overlap(d_emission, ebytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {materials, mbytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward: d_emission must not overlap texel_aovs, d_out or the materials");
    const bool emit = d_emission && s->ds.light_count > 0;           // a scene without lights: accepted, nothing to add
    if (!emit && !d_materials) return ZDR_OK;
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;      // every pair, as the forward
    BgradArgs G; memset(&G, 0, sizeof G);
    G.texels = B.texels; G.d_out = (const float4 *)d_out; G.materials = B.materials;
    G.d_materials = d_materials; G.d_emission = emit ? d_emission : nullptr;
    G.count = (uint32_t *)workspace; G.list = (uint32_t *)((char *)workspace + ZDR_BOUNCE_HEADER_BYTES);
    G.acc = emit ? (float *)((char *)workspace + ZDR_BOUNCE_HEADER_BYTES + lbytes) : nullptr;
    G.cells = d_materials ? (float *)((char *)workspace + ZDR_BOUNCE_HEADER_BYTES + lbytes + abytes) : nullptr;
    G.ntexels = B.ntexels; G.tex_w = B.tex_w; G.sample_begin = B.sample_begin; G.sample_end = B.sample_end;
    G.inv_spp = B.inv_spp; G.bounces = B.bounces; G.wide_offsets = B.wide_offsets;
    G.cell_copies = cell_copies; G.ncell_words = (uint32_t)(4 * cells);
    if (int rc = zdr_launch_texel_bounce_backward(S, s->accel_is_bvh, C, G, mt, (hipStream_t)stream))
        return fail(ZDR_E_HIP, "texel bounce backward: launch " + std::to_string(rc / 256) + " of 5 failed: " + hipGetErrorString((hipError_t)(rc % 256)));
    return ZDR_OK;
}

// zdr_scene_texel_bounce_backward_env (include/zdr.h): the forward's checks, then the three launches of zdr_bounceenv.hip on the caller's
// stream.  The handle is only read; the workspace is the forward's (a header and the list), so nothing is allocated and the call can be
// captured without a call before.
extern "C" size_t zdr_texel_bounce_backward_env_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (bounce_check_size(tex_h, tex_w)) return 0;
    return ZDR_BOUNCE_HEADER_BYTES + bgrad_list_bytes(tex_h, tex_w);
}

extern "C" int zdr_scene_texel_bounce_backward_env(zdr_scene *s, const zdr_texel_bounce_params *p, const float *texel_aovs, const float *d_out, const float *materials,
                                                   const int32_t *dims, uint32_t nmat, float *d_env, void *workspace, void *stream) {
    if (!d_out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (!d_env) return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward_env: d_env is NULL");
    if ((uintptr_t)d_out % 16 || (uintptr_t)workspace % 16 || (uintptr_t)d_env % 16)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward_env: d_out, d_env and workspace must be 16-byte aligned");
    if (s && s->ds.env_count <= 0) return fail(ZDR_E_INVALID, "d_env given, but the scene has no environment map");
    if (!zdr_launch_texel_bounce_backward_env)                       // (weak: csrc/bounceenv.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the bounced-light environment gradient kernels (zdr_bounceenv.hip)");
    SamplerCfg C; BounceArgs B; MaterialTable mt;
    if (int rc = bounce_prepare(s, p, texel_aovs, materials, dims, nmat, (hipStream_t)stream, C, B, mt)) return rc;
    const size_t n = B.ntexels, wbytes = ZDR_BOUNCE_HEADER_BYTES + bgrad_list_bytes(p->tex_h, p->tex_w);
    size_t mbytes = 0;
    for (uint32_t k = 0; k < nmat; k++) mbytes += 16 * (size_t)dims[2 * k] * (size_t)dims[2 * k + 1];
    const size_t ebytes = 16 * (size_t)s->ds.env_h * (size_t)s->ds.env_w;
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {materials, mbytes}, {d_env, ebytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward_env: the workspace must not overlap texel_aovs, d_out, the materials or d_env");
    if (denoise_overlap(d_env, ebytes, {{texel_aovs, 64 * n}, {d_out, 16 * n}, {materials, mbytes}}))
        return fail(ZDR_E_INVALID, "zdr_scene_texel_bounce_backward_env: d_env must not overlap texel_aovs, d_out or the materials");
    DScene S = s->ds;
    S.shadow_pairs = ~0ull;      // every pair, as the forward
    BenvArgs G; memset(&G, 0, sizeof G);
    G.texels = B.texels; G.d_out = (const float4 *)d_out; G.materials = B.materials; G.d_env = d_env;
    G.count = (uint32_t *)workspace; G.list = (uint32_t *)((char *)workspace + ZDR_BOUNCE_HEADER_BYTES);
    G.ntexels = B.ntexels; G.tex_w = B.tex_w; G.sample_begin = B.sample_begin; G.sample_end = B.sample_end;
    G.inv_spp = B.inv_spp; G.bounces = B.bounces; G.wide_offsets = B.wide_offsets;
    if (int rc = zdr_launch_texel_bounce_backward_env(S, s->accel_is_bvh, C, G, mt, (hipStream_t)stream))
        return fail(ZDR_E_HIP, "texel bounce backward (environment): launch " + std::to_string(rc / 256) + " of 3 failed: " + hipGetErrorString((hipError_t)(rc % 256)));
    return ZDR_OK;
}

// ------------------------------------------------------------------------------- push-pull
// zdr_push_pull / zdr_push_pull_backward (include/zdr.h): no scene handle, no allocation, no synchronisation — argument checks, then the
// launches of zdr_pushpull.hip on the caller's stream.  The workspace holds the pyramid's levels >= 1 (csrc/pushpull.h); neither call
// reads what another left in it.
static int push_pull_check(const zdr_push_pull_params *p) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_push_pull_params))
        return fail(ZDR_E_INVALID, "zdr_push_pull_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " +
                                   std::to_string(sizeof(zdr_push_pull_params)) + ": caller and library were built from different include/zdr.h");
    if (p->width <= 0 || p->height <= 0) return fail(ZDR_E_INVALID, "zdr_push_pull_params: width and height must be positive");
    if (p->levels < 0) return fail(ZDR_E_INVALID, "zdr_push_pull_params.levels is " + std::to_string(p->levels) + ": 0 (down to 1 x 1) or a positive count");
    if ((uint64_t)p->width * (uint64_t)p->height > ZDR_PUSHPULL_MAX_TEXELS) return fail(ZDR_E_UNSUPPORTED, "zdr_push_pull: more than 2^26 texels");
    return ZDR_OK;
}

extern "C" size_t zdr_push_pull_workspace_bytes(const zdr_push_pull_params *p) {
    if (push_pull_check(p)) return 0;
    return zdr_push_pull_plan(p->width, p->height, p->levels).bytes;
}

static int push_pull_call(const char *name, const zdr_push_pull_params *p, const float *weight, const float *in, float *out, void *workspace, void *stream, int backward) {
    if (int rc = push_pull_check(p)) return rc;
    for (const void *q : {(const void *)weight, (const void *)in, (const void *)out, (const void *)workspace}) {
        if (!q) return fail(ZDR_E_INVALID, "null argument");
        if ((uintptr_t)q % 16) return fail(ZDR_E_INVALID, std::string(name) + ": every pointer must be 16-byte aligned");
    }
    const size_t n = (size_t)p->width * (size_t)p->height, wbytes = zdr_push_pull_plan(p->width, p->height, p->levels).bytes;
    if (denoise_overlap(out, 16 * n, {{in, 16 * n}, {weight, 4 * n}, {workspace, wbytes}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the output must not alias or overlap an input or the workspace");
    if (denoise_overlap(workspace, wbytes, {{in, 16 * n}, {weight, 4 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the workspace must not overlap an input");
    if (!zdr_launch_push_pull)                                       // (weak: csrc/pushpull.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the push-pull kernels (zdr_pushpull.hip)");
    PushPullArgs A;
    A.width = p->width; A.height = p->height; A.levels = p->levels;
    A.weight = weight; A.in = (const float4 *)in; A.out = (float4 *)out; A.workspace = workspace;
    if (zdr_launch_push_pull(A, backward, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

extern "C" int zdr_push_pull(const zdr_push_pull_params *p, const float *weight, const float *x, float *out, void *workspace, void *stream) {
    return push_pull_call("zdr_push_pull", p, weight, x, out, workspace, stream, 0);
}

extern "C" int zdr_push_pull_backward(const zdr_push_pull_params *p, const float *weight, const float *d_out, float *d_x, void *workspace, void *stream) {
    return push_pull_call("zdr_push_pull_backward", p, weight, d_out, d_x, workspace, stream, 1);
}

// ------------------------------------------------------------------- texture-space views
// zdr_scene_texel_view (include/zdr.h): argument checks, then the three launches of zdr_project.hip on the caller's stream.  The handle is
// only read — the acceleration structure as it is — so nothing is allocated and the call can be captured without a call before.
// The argument checks the texel-filter entry points share (views, gathers, pyramids, footprints, plans), one condition each; an entry
// point calls them in the order in which its checks fire.
static int filter_check_struct(const std::string &what, uint32_t struct_size, size_t expect) {      // what: "<struct>." or "<entry point>: "
    if (struct_size != expect) return fail(ZDR_E_INVALID, what + "struct_size is " + std::to_string(struct_size) + ", this library expects " + std::to_string(expect));
    return ZDR_OK;
}

static int filter_check_positive(const char *name, const char *what, int32_t a, int32_t b) {         // what: "texture" or "image"
    if (a <= 0 || b <= 0) return fail(ZDR_E_INVALID, std::string(name) + ": the " + what + " size must be positive");
    return ZDR_OK;
}

static int filter_check_texels(const char *name, int32_t tex_h, int32_t tex_w) {
    if ((uint64_t)tex_h * (uint64_t)tex_w > ZDR_FILTER_MAX_TEXELS) return fail(ZDR_E_UNSUPPORTED, std::string(name) + ": more than 2^26 texels");
    return ZDR_OK;
}

static int filter_check_pixels(const char *name, int32_t width, int32_t height) {
    if ((uint64_t)width * (uint64_t)height > ZDR_FILTER_MAX_PIXELS) return fail(ZDR_E_UNSUPPORTED, std::string(name) + ": more than 2^28 pixels");
    return ZDR_OK;
}

static int filter_check_pointers(const char *name, std::initializer_list<const void *> ptrs) {
    for (const void *q : ptrs) {
        if (!q) return fail(ZDR_E_INVALID, "null argument");
        if ((uintptr_t)q % 16) return fail(ZDR_E_INVALID, std::string(name) + ": every pointer must be 16-byte aligned");
    }
    return ZDR_OK;
}

static int project_check_size(int32_t tex_h, int32_t tex_w) {
    if (int rc = filter_check_positive("zdr_scene_texel_view", "texture", tex_h, tex_w)) return rc;
    return filter_check_texels("zdr_scene_texel_view", tex_h, tex_w);
}

static int project_check_image(const char *name, int32_t width, int32_t height) {
    if (int rc = filter_check_positive(name, "image", width, height)) return rc;
    return filter_check_pixels(name, width, height);
}

extern "C" size_t zdr_texel_view_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (project_check_size(tex_h, tex_w)) return 0;
    return ZDR_PROJECT_HEADER_BYTES + (((size_t)tex_h * (size_t)tex_w * sizeof(uint32_t) + 15) & ~(size_t)15);
}

extern "C" int zdr_scene_texel_view(zdr_scene *s, const zdr_texel_view_params *p, const float *texel_aovs, float *out, void *workspace, void *stream) {
    if (!s || !p || !texel_aovs || !out || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (p->struct_size != sizeof(zdr_texel_view_params))
        return fail(ZDR_E_INVALID, "zdr_texel_view_params.struct_size is " + std::to_string(p->struct_size) + ", this library expects " + std::to_string(sizeof(zdr_texel_view_params)));
    if ((uintptr_t)texel_aovs % 16 || (uintptr_t)out % 16 || (uintptr_t)workspace % 16)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_view: texel_aovs, out and workspace must be 16-byte aligned");
    if (int rc = project_check_size(p->tex_h, p->tex_w)) return rc;
    if (int rc = project_check_image("zdr_scene_texel_view", p->width, p->height)) return rc;
    if (!(p->camera.fov > 0.0f && p->camera.fov < 3.14159265358979323846f))       // (false for a NaN)
        return fail(ZDR_E_INVALID, "zdr_scene_texel_view: camera.fov must be finite and lie in (0, pi)");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, wbytes = zdr_texel_view_workspace_bytes(p->tex_h, p->tex_w);
    if (denoise_overlap(out, 32 * n, {{workspace, wbytes}, {texel_aovs, 64 * n}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_view: out must not overlap the workspace or texel_aovs");
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}})) return fail(ZDR_E_INVALID, "zdr_scene_texel_view: the workspace must not overlap texel_aovs");
    if (!zdr_launch_texel_view)                                      // (weak: csrc/project.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space view kernels (zdr_project.hip)");
    HIPCHK(hipSetDevice(s->device));
    ProjViewArgs V;
    V.texels = (const float4 *)texel_aovs; V.out = (float4 *)out;
    V.count = (uint32_t *)workspace; V.list = (uint32_t *)((char *)workspace + ZDR_PROJECT_HEADER_BYTES);
    V.ntexels = (uint32_t)n; V.tex_w = p->tex_w; V.tex_h = p->tex_h;
    V.width =(float)p->width; V.height = (float)p->height; V.half_w = 0.5f * (float)p->width; V.half_h = 0.5f * (float)p->height;
    V.aspect = (float)p->height / (float)p->width;                   // (as make_render_cfg)
    camera_frame(p->camera, V.cam_o, V.cam_fwd, V.cam_right, V.cam_upp, V.cam_tan);
    if (zdr_launch_texel_view(s->ds, s->accel_is_bvh, V, (hipStream_t)stream)) return fail(ZDR_E_HIP, "texel view launch failed");
    return ZDR_OK;
}

// zdr_texel_gather / zdr_texel_gather_backward (include/zdr.h): no scene handle, no workspace, no allocation, no synchronisation —
// argument checks, then one launch of zdr_project.hip on the caller's stream.
static int texel_gather_call(const char *name, const zdr_texel_gather_params *p, const float *view, const float *in, float *out, void *stream, int backward) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = filter_check_struct("zdr_texel_gather_params.", p->struct_size, sizeof(zdr_texel_gather_params))) return rc;
    if (int rc = filter_check_positive(name, "texture", p->tex_h, p->tex_w)) return rc;
    if (int rc = filter_check_texels(name, p->tex_h, p->tex_w)) return rc;
    if (int rc = project_check_image(name, p->width, p->height)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)in, (const void *)out})) return rc;
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(out, 16 * (backward ? npix : n), {{view, 32 * n}, {in, 16 * (backward ? n : npix)}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the output must not alias or overlap an input");
    if (!zdr_launch_texel_gather)                                    // (weak: csrc/project.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the texture-space view kernels (zdr_project.hip)");
    ProjGatherArgs G;
    G.view = (const float4 *)view; G.in = (const float4 *)in; G.out = (float4 *)out;
    G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height;
    if (zdr_launch_texel_gather(G, backward, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

extern "C" int zdr_texel_gather(const zdr_texel_gather_params *p, const float *view, const float *image, float *color, void *stream) {
    return texel_gather_call("zdr_texel_gather", p, view, image, color, stream, 0);
}

extern "C" int zdr_texel_gather_backward(const zdr_texel_gather_params *p, const float *view, const float *d_color, float *d_image, void *stream) {
    return texel_gather_call("zdr_texel_gather_backward", p, view, d_color, d_image, stream, 1);
}

// ------------------------------------------------------------------- prefiltered gather
// zdr_image_pyramid, zdr_image_pyramid_backward, zdr_texel_gather_mip, zdr_texel_gather_mip_backward (include/zdr.h): no scene handle, no
// allocation, no synchronisation — argument checks, then the launches of zdr_mip.hip on the caller's stream.
static int mip_check_image(const char *name, uint32_t struct_size, size_t expect, int32_t width, int32_t height, int32_t levels) {
    if (int rc = filter_check_struct(std::string(name) + ": ", struct_size, expect)) return rc;
    if (int rc = filter_check_positive(name, "image", width, height)) return rc;
    if (levels < 0) return fail(ZDR_E_INVALID, std::string(name) + ": levels is " + std::to_string(levels) + ": 0 (down to 1 x 1) or a positive count");
    return filter_check_pixels(name, width, height);
}

// What zdr_texel_gather_mip*, zdr_texel_gather_aniso* and zdr_gather_plan_* ask of their params: the image and its pyramid, the texture,
// the filter (ZDR_PLAN_*; a plan's is the caller's) and what that filter reads of footprint and max_aniso.
static int filter_check_gather(const char *name, uint32_t struct_size, size_t expect, int32_t tex_h, int32_t tex_w, int32_t width, int32_t height, int32_t levels,
                               int32_t filter, float footprint, int32_t max_aniso) {
    if (int rc = mip_check_image(name, struct_size, expect, width, height, levels)) return rc;
    if (int rc = filter_check_positive(name, "texture", tex_h, tex_w)) return rc;
    if (filter < ZDR_PLAN_BILINEAR || filter > ZDR_PLAN_ANISO)
        return fail(ZDR_E_INVALID, std::string(name) + ": filter is " + std::to_string(filter) + ": 0 (bilinear), 1 (mip) or 2 (aniso)");
    if (filter != ZDR_PLAN_BILINEAR && !(footprint > 0.0f && footprint <= 3.402823466e38f))    // (false for a NaN)
        return fail(ZDR_E_INVALID, std::string(name) + ": footprint must be finite and > 0");
    if (filter == ZDR_PLAN_ANISO && (max_aniso < 1 || max_aniso > ZDR_ANISO_MAX_PROBES))
        return fail(ZDR_E_INVALID, std::string(name) + ": max_aniso is " + std::to_string(max_aniso) + ": it must lie in 1 .. " + std::to_string(ZDR_ANISO_MAX_PROBES));
    return filter_check_texels(name, tex_h, tex_w);
}

extern "C" size_t zdr_image_pyramid_bytes(const zdr_image_pyramid_params *p) {
    if (!p) { fail(ZDR_E_INVALID, "null argument"); return 0; }
    if (mip_check_image("zdr_image_pyramid_params", p->struct_size, sizeof(zdr_image_pyramid_params), p->width, p->height, p->levels)) return 0;
    return zdr_mip_plan(p->width, p->height, p->levels).bytes;
}

static int image_pyramid_call(const char *name, const zdr_image_pyramid_params *p, const float *image, float *d_image, float *pyramid, void *stream, int backward) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = mip_check_image(name, p->struct_size, sizeof(zdr_image_pyramid_params), p->width, p->height, p->levels)) return rc;
    const void *level0 = backward ? (const void *)d_image : (const void *)image;
    if (int rc = filter_check_pointers(name, {level0, (const void *)pyramid})) return rc;
    const size_t npix = (size_t)p->width * (size_t)p->height, pbytes = zdr_mip_plan(p->width, p->height, p->levels).bytes;
    if (denoise_overlap(pyramid, pbytes, {{level0, 16 * npix}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the pyramid must not alias or overlap the image");
    if (!zdr_launch_image_pyramid)                                   // (weak: csrc/mip.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the prefiltering kernels (zdr_mip.hip)");
    MipPyramidArgs A;
    A.width = p->width; A.height = p->height; A.levels = p->levels;
    A.image = (const float4 *)image; A.d_image = (float4 *)d_image; A.pyramid = (float4 *)pyramid;
    if (zdr_launch_image_pyramid(A, backward, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

extern "C" int zdr_image_pyramid(const zdr_image_pyramid_params *p, const float *image, float *pyramid, void *stream) {
    return image_pyramid_call("zdr_image_pyramid", p, image, nullptr, pyramid, stream, 0);
}

extern "C" int zdr_image_pyramid_backward(const zdr_image_pyramid_params *p, float *d_pyramid, float *d_image, void *stream) {
    return image_pyramid_call("zdr_image_pyramid_backward", p, nullptr, d_image, d_pyramid, stream, 1);
}

static int texel_gather_mip_check(const char *name, const zdr_texel_gather_mip_params *p) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    return filter_check_gather(name, p->struct_size, sizeof(*p), p->tex_h, p->tex_w, p->width, p->height, p->levels, ZDR_PLAN_MIP, p->footprint, 1);
}

extern "C" int zdr_texel_gather_mip(const zdr_texel_gather_mip_params *p, const float *view, const float *image, const float *pyramid, float *color, void *stream) {
    const char *name = "zdr_texel_gather_mip";
    if (int rc = texel_gather_mip_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)image, (const void *)pyramid, (const void *)color})) return rc;
    const MipPlan P = zdr_mip_plan(p->width, p->height, p->levels);
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(color, 16 * n, {{view, 32 * n}, {image, 16 * npix}, {pyramid, P.bytes}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the output must not alias or overlap an input");
    if (!zdr_launch_texel_gather_mip)                                // (weak: csrc/mip.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the prefiltering kernels (zdr_mip.hip)");
    MipGatherArgs G;
    G.view = (const float4 *)view; G.in = (const float4 *)image; G.pyramid = (const float4 *)pyramid; G.out = (float4 *)color; G.d_pyramid = nullptr;
    G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height; G.L = P.L; G.footprint = p->footprint;
    if (zdr_launch_texel_gather_mip(G, 0, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

extern "C" int zdr_texel_gather_mip_backward(const zdr_texel_gather_mip_params *p, const float *view, const float *d_color, float *d_image, float *d_pyramid, void *stream) {
    const char *name = "zdr_texel_gather_mip_backward";
    if (int rc = texel_gather_mip_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)d_color, (const void *)d_image, (const void *)d_pyramid})) return rc;
    const MipPlan P = zdr_mip_plan(p->width, p->height, p->levels);
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(d_image, 16 * npix, {{view, 32 * n}, {d_color, 16 * n}, {d_pyramid, P.bytes}}) || denoise_overlap(d_pyramid, P.bytes, {{view, 32 * n}, {d_color, 16 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": an output must not alias or overlap an input or the other output");
    if (!zdr_launch_texel_gather_mip)                                // (weak: csrc/mip.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the prefiltering kernels (zdr_mip.hip)");
    MipGatherArgs G;
    G.view = (const float4 *)view; G.in = (const float4 *)d_color; G.pyramid = nullptr; G.out = (float4 *)d_image; G.d_pyramid = (float4 *)d_pyramid;
    G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height; G.L = P.L; G.footprint = p->footprint;
    if (zdr_launch_texel_gather_mip(G, 1, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

// ------------------------------------------------------------------- anisotropic gather
// zdr_texel_footprint, zdr_texel_gather_aniso, zdr_texel_gather_aniso_backward (include/zdr.h): no scene handle, no workspace, no
// allocation, no synchronisation — argument checks, then one launch of zdr_aniso.hip on the caller's stream.
extern "C" int zdr_texel_footprint(const zdr_texel_footprint_params *p, const float *texel_aovs, float *out, void *stream) {
    const char *name = "zdr_texel_footprint";
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = filter_check_struct("zdr_texel_footprint_params.", p->struct_size, sizeof(zdr_texel_footprint_params))) return rc;
    if (int rc = filter_check_positive(name, "texture", p->tex_h, p->tex_w)) return rc;
    if (int rc = filter_check_positive(name, "image", p->width, p->height)) return rc;
    if (!(p->camera.fov > 0.0f && p->camera.fov < 3.14159265358979323846f))       // (false for a NaN)
        return fail(ZDR_E_INVALID, std::string(name) + ": camera.fov must be finite and lie in (0, pi)");
    if (int rc = filter_check_texels(name, p->tex_h, p->tex_w)) return rc;
    if (int rc = filter_check_pixels(name, p->width, p->height)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)texel_aovs, (const void *)out})) return rc;
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w;
    if (denoise_overlap(out, 16 * n, {{texel_aovs, 64 * n}})) return fail(ZDR_E_INVALID, std::string(name) + ": out must not alias or overlap texel_aovs");
    if (!zdr_launch_texel_footprint)                                 // (weak: csrc/aniso.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the anisotropic-gather kernels (zdr_aniso.hip)");
    AnisoFootprintArgs A;
    A.texels = (const float4 *)texel_aovs; A.out = (float4 *)out; A.ntexels = (uint32_t)n;
    A.half_w = 0.5f * (float)p->width; A.half_h = 0.5f * (float)p->height;
    A.aspect = (float)p->height / (float)p->width;                   // (as zdr_scene_texel_view)
    camera_frame(p->camera, A.cam_o, A.cam_fwd, A.cam_right, A.cam_upp, A.cam_tan);
    if (zdr_launch_texel_footprint(A, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

// zdr_texel_footprint_tangents (include/zdr.h): zdr_texel_footprint's checks, the tangent buffer in addition, one launch of zdr_tangent.hip.
extern "C" int zdr_texel_footprint_tangents(const zdr_texel_footprint_params *p, const float *texel_aovs, const float *tangents, float *out, void *stream) {
    const char *name = "zdr_texel_footprint_tangents";
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = filter_check_struct("zdr_texel_footprint_params.", p->struct_size, sizeof(zdr_texel_footprint_params))) return rc;
    if (int rc = filter_check_positive(name, "texture", p->tex_h, p->tex_w)) return rc;
    if (int rc = filter_check_positive(name, "image", p->width, p->height)) return rc;
    if (!(p->camera.fov > 0.0f && p->camera.fov < 3.14159265358979323846f))       // (false for a NaN)
        return fail(ZDR_E_INVALID, std::string(name) + ": camera.fov must be finite and lie in (0, pi)");
    if (int rc = filter_check_texels(name, p->tex_h, p->tex_w)) return rc;
    if (int rc = filter_check_pixels(name, p->width, p->height)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)texel_aovs, (const void *)tangents, (const void *)out})) return rc;
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w;
    if (denoise_overlap(out, 16 * n, {{texel_aovs, 64 * n}, {tangents, 32 * n}})) return fail(ZDR_E_INVALID, std::string(name) + ": out must not alias or overlap an input");
    if (!zdr_launch_texel_footprint_tangents)                        // (weak: csrc/tangent.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the UV-tangent kernels (zdr_tangent.hip)");
    AnisoFootprintArgs A;
    A.texels = (const float4 *)texel_aovs; A.out = (float4 *)out; A.ntexels = (uint32_t)n;
    A.half_w = 0.5f * (float)p->width; A.half_h = 0.5f * (float)p->height;
    A.aspect = (float)p->height / (float)p->width;                   // (as zdr_texel_footprint)
    camera_frame(p->camera, A.cam_o, A.cam_fwd, A.cam_right, A.cam_upp, A.cam_tan);
    if (zdr_launch_texel_footprint_tangents(A, (const float4 *)tangents, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

static int texel_gather_aniso_check(const char *name, const zdr_texel_gather_aniso_params *p) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    return filter_check_gather(name, p->struct_size, sizeof(*p), p->tex_h, p->tex_w, p->width, p->height, p->levels, ZDR_PLAN_ANISO, p->footprint, p->max_aniso);
}

extern "C" int zdr_texel_gather_aniso(const zdr_texel_gather_aniso_params *p, const float *view, const float *footprint, const float *image, const float *pyramid,
                                      float *color, void *stream) {
    const char *name = "zdr_texel_gather_aniso";
    if (int rc = texel_gather_aniso_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)footprint, (const void *)image, (const void *)pyramid, (const void *)color})) return rc;
    const MipPlan P = zdr_mip_plan(p->width, p->height, p->levels);
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(color, 16 * n, {{view, 32 * n}, {footprint, 16 * n}, {image, 16 * npix}, {pyramid, P.bytes}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the output must not alias or overlap an input");
    if (!zdr_launch_texel_gather_aniso)                              // (weak: csrc/aniso.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the anisotropic-gather kernels (zdr_aniso.hip)");
    AnisoGatherArgs G;
    G.view = (const float4 *)view; G.foot = (const float4 *)footprint; G.in = (const float4 *)image; G.pyramid = (const float4 *)pyramid;
    G.out = (float4 *)color; G.d_pyramid = nullptr;
    G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height; G.L = P.L; G.max_aniso = p->max_aniso; G.footprint = p->footprint;
    if (zdr_launch_texel_gather_aniso(G, 0, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

extern "C" int zdr_texel_gather_aniso_backward(const zdr_texel_gather_aniso_params *p, const float *view, const float *footprint, const float *d_color, float *d_image,
                                               float *d_pyramid, void *stream) {
    const char *name = "zdr_texel_gather_aniso_backward";
    if (int rc = texel_gather_aniso_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)footprint, (const void *)d_color, (const void *)d_image, (const void *)d_pyramid})) return rc;
    const MipPlan P = zdr_mip_plan(p->width, p->height, p->levels);
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(d_image, 16 * npix, {{view, 32 * n}, {footprint, 16 * n}, {d_color, 16 * n}, {d_pyramid, P.bytes}}) ||
        denoise_overlap(d_pyramid, P.bytes, {{view, 32 * n}, {footprint, 16 * n}, {d_color, 16 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": an output must not alias or overlap an input or the other output");
    if (!zdr_launch_texel_gather_aniso)                              // (weak: csrc/aniso.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the anisotropic-gather kernels (zdr_aniso.hip)");
    AnisoGatherArgs G;
    G.view = (const float4 *)view; G.foot = (const float4 *)footprint; G.in = (const float4 *)d_color; G.pyramid = nullptr;
    G.out = (float4 *)d_image; G.d_pyramid = (float4 *)d_pyramid;
    G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height; G.L = P.L; G.max_aniso = p->max_aniso; G.footprint = p->footprint;
    if (zdr_launch_texel_gather_aniso(G, 1, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

// ------------------------------------------------------------------- gather plan
// zdr_gather_plan_* (include/zdr.h): no scene handle, no allocation — argument checks, then the launches of zdr_plan.hip on the caller's
// stream.  None of them synchronises: the ONE synchronisation of a plan's build is the caller's, between zdr_gather_plan_count and the
// read of nnz from the workspace's header.
static int plan_check(const char *name, const zdr_gather_plan_params *p) {
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    return filter_check_gather(name, p->struct_size, sizeof(*p), p->tex_h, p->tex_w, p->width, p->height, p->levels, p->filter, p->footprint, p->max_aniso);
}

// the rows of a plan: the pixels of level 0, then — mip and aniso — the packed levels >= 1 (one pixel where there is none, as the
// pyramid's buffer has it)
static uint32_t plan_rows(const zdr_gather_plan_params *p) {
    const size_t p0 = (size_t)p->width * (size_t)p->height;
    return (uint32_t)(p->filter == ZDR_PLAN_BILINEAR ? p0 : p0 + zdr_mip_plan(p->width, p->height, p->levels).bytes / sizeof(float4));
}

static size_t plan_round(size_t n) { return (n + 255) & ~(size_t)255; }

static bool plan_workspace(const zdr_gather_plan_params *p, uint64_t nnz, void *base, PlanWorkspace &W) {
    const size_t nblocks = ((size_t)p->tex_h * (size_t)p->tex_w + ZDR_PLAN_BLOCK - 1) / ZDR_PLAN_BLOCK;
    int ok = 1;
    W.sort_temp_bytes = zdr_plan_sort_temp_bytes(nnz, plan_rows(p), &ok);
    if (!ok) return false;
    char *at = (char *)base;
    W.nnz = (uint64_t *)at; at += ZDR_PLAN_HEADER_BYTES;
    W.block_off = (uint32_t *)at; at += plan_round(nblocks * sizeof(uint32_t));
    W.keys = (uint32_t *)at; at += plan_round((size_t)nnz * sizeof(uint32_t));
    W.keys_sorted = (uint32_t *)at; at += plan_round((size_t)nnz * sizeof(uint32_t));
    W.vals = (uint64_t *)at; at += plan_round((size_t)nnz * sizeof(uint64_t));
    W.sort_temp = (void *)at; at += plan_round(W.sort_temp_bytes);
    W.bytes = (size_t)(at - (char *)base);
    return true;
}

static PlanEnumArgs plan_enum_args(const zdr_gather_plan_params *p, const float *view, const float *footprint) {
    PlanEnumArgs E;
    E.view = (const float4 *)view; E.foot = (const float4 *)footprint;
    E.ntexels = (uint32_t)((size_t)p->tex_h * (size_t)p->tex_w); E.nblocks = (E.ntexels + ZDR_PLAN_BLOCK - 1u) / ZDR_PLAN_BLOCK;
    E.filter = p->filter; E.width = p->width; E.height = p->height;
    E.L = p->filter == ZDR_PLAN_BILINEAR ? 0 : zdr_mip_plan(p->width, p->height, p->levels).L;
    E.max_aniso = p->filter == ZDR_PLAN_ANISO ? p->max_aniso : 1;
    E.footprint = p->filter == ZDR_PLAN_BILINEAR ? 1.0f : p->footprint;
    E.p0 = (uint32_t)((size_t)p->width * (size_t)p->height);
    return E;
}

extern "C" size_t zdr_gather_plan_rows(const zdr_gather_plan_params *p) {
    if (plan_check("zdr_gather_plan_params", p)) return 0;
    return plan_rows(p);
}

extern "C" size_t zdr_gather_plan_workspace_bytes(const zdr_gather_plan_params *p, uint64_t nnz) {
    if (plan_check("zdr_gather_plan_params", p)) return 0;
    if (nnz > ZDR_PLAN_MAX_NNZ) { fail(ZDR_E_UNSUPPORTED, "zdr_gather_plan_workspace_bytes: more than 2^31 - 1 entries"); return 0; }
    if (!zdr_plan_sort_temp_bytes) { fail(ZDR_E_UNSUPPORTED, "this library was linked without the gather-plan kernels (zdr_plan.hip)"); return 0; }
    PlanWorkspace W;
    if (!plan_workspace(p, nnz, nullptr, W)) { fail(ZDR_E_HIP, "zdr_gather_plan_workspace_bytes: the sort's size query failed (no device?)"); return 0; }
    return W.bytes;
}

static int plan_check_inputs(const char *name, const zdr_gather_plan_params *p, const float *view, const float *footprint, const void *workspace) {
    if (int rc = plan_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)view, workspace})) return rc;
    if (p->filter == ZDR_PLAN_ANISO)
        if (int rc = filter_check_pointers(name, {(const void *)footprint})) return rc;
    if (!zdr_launch_plan_build)                                      // (weak: csrc/plan.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the gather-plan kernels (zdr_plan.hip)");
    return ZDR_OK;
}

extern "C" int zdr_gather_plan_count(const zdr_gather_plan_params *p, const float *view, const float *footprint, void *workspace, void *stream) {
    const char *name = "zdr_gather_plan_count";
    if (int rc = plan_check_inputs(name, p, view, footprint, workspace)) return rc;
    PlanWorkspace W;
    if (!plan_workspace(p, 0, workspace, W)) return fail(ZDR_E_HIP, std::string(name) + ": the sort's size query failed");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w;
    if (denoise_overlap(workspace, W.bytes, {{view, 32 * n}, {footprint, p->filter == ZDR_PLAN_ANISO ? 16 * n : 0}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the workspace must not alias or overlap an input");
    if (zdr_launch_plan_count(plan_enum_args(p, view, footprint), W, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

extern "C" int zdr_gather_plan_build(const zdr_gather_plan_params *p, const float *view, const float *footprint, uint64_t nnz, void *workspace, uint32_t *row_start,
                                     void *entries, void *stream) {
    const char *name = "zdr_gather_plan_build";
    if (int rc = plan_check_inputs(name, p, view, footprint, workspace)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)row_start, (const void *)entries})) return rc;
    if (nnz > ZDR_PLAN_MAX_NNZ) return fail(ZDR_E_UNSUPPORTED, std::string(name) + ": more than 2^31 - 1 entries");
    PlanWorkspace W;
    if (!plan_workspace(p, nnz, workspace, W)) return fail(ZDR_E_HIP, std::string(name) + ": the sort's size query failed");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, rows = plan_rows(p);
    const size_t fbytes = p->filter == ZDR_PLAN_ANISO ? 16 * n : 0;
    if (denoise_overlap(workspace, W.bytes, {{view, 32 * n}, {footprint, fbytes}, {row_start, 4 * (rows + 1)}, {entries, 8 * (size_t)nnz}}) ||
        denoise_overlap(row_start, 4 * (rows + 1), {{view, 32 * n}, {footprint, fbytes}, {entries, 8 * (size_t)nnz}}) ||
        denoise_overlap(entries, 8 * (size_t)nnz, {{view, 32 * n}, {footprint, fbytes}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the workspace and the outputs must not alias or overlap an input or one another");
    if (zdr_launch_plan_build(plan_enum_args(p, view, footprint), W, (uint32_t)nnz, (uint32_t)rows, row_start, (uint64_t *)entries, (hipStream_t)stream))
        return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

extern "C" int zdr_gather_plan_apply(const zdr_gather_plan_params *p, const uint32_t *row_start, const void *entries, const float *d_color, float *d_image,
                                     float *d_pyramid, void *stream) {
    const char *name = "zdr_gather_plan_apply";
    if (int rc = plan_check(name, p)) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)row_start, entries, (const void *)d_color, (const void *)d_image})) return rc;
    if (p->filter != ZDR_PLAN_BILINEAR)
        if (int rc = filter_check_pointers(name, {(const void *)d_pyramid})) return rc;
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height, rows = plan_rows(p);
    const size_t pbytes = p->filter == ZDR_PLAN_BILINEAR ? 0 : 16 * (rows - npix);
    if (denoise_overlap(d_image, 16 * npix, {{row_start, 4 * (rows + 1)}, {d_color, 16 * n}, {d_pyramid, pbytes}}) ||
        denoise_overlap(d_pyramid, pbytes, {{row_start, 4 * (rows + 1)}, {d_color, 16 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": an output must not alias or overlap an input or the other output");
    if (!zdr_launch_plan_apply)                                      // (weak: csrc/plan.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the gather-plan kernels (zdr_plan.hip)");
    PlanApplyArgs A;
    A.row_start = row_start; A.entries = (const uint2 *)entries; A.d_color = d_color; A.d_image = d_image; A.d_pyramid = d_pyramid;
    A.p0 = (uint32_t)npix; A.rows = (uint32_t)rows;
    if (zdr_launch_plan_apply(A, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

// ------------------------------------------------------------------- camera gradients
// zdr_texel_gather_dview, zdr_texel_view_backward (include/zdr.h): no scene handle, no allocation, no synchronisation — argument checks,
// then the launches of zdr_viewgrad.hip on the caller's stream.
extern "C" int zdr_texel_gather_dview(const zdr_texel_gather_dview_params *p, const float *view, const float *image, const float *pyramid,
                                      const float *d_color, float *d_view, void *stream) {
    const char *name = "zdr_texel_gather_dview";
    if (!p) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = filter_check_gather(name, p->struct_size, sizeof(*p), p->tex_h, p->tex_w, p->width, p->height, p->levels, p->filter, p->footprint, 1)) return rc;
    if (p->filter == ZDR_PLAN_ANISO)
        return fail(ZDR_E_UNSUPPORTED, std::string(name) + ": the anisotropic gather has no derivative in the view buffer (its axis and probe count come from the footprint buffer)");
    if (int rc = filter_check_pointers(name, {(const void *)view, (const void *)image, (const void *)d_color, (const void *)d_view})) return rc;
    if (p->filter == ZDR_PLAN_MIP)
        if (int rc = filter_check_pointers(name, {(const void *)pyramid})) return rc;
    const MipPlan P = zdr_mip_plan(p->width, p->height, p->levels);
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, npix = (size_t)p->width * (size_t)p->height;
    if (denoise_overlap(d_view, 32 * n, {{view, 32 * n}, {image, 16 * npix}, {d_color, 16 * n}, {pyramid, p->filter == ZDR_PLAN_MIP ? P.bytes : 0}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the output must not alias or overlap an input");
    if (!zdr_launch_texel_gather_dview)                              // (weak: csrc/viewgrad.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the camera-gradient kernels (zdr_viewgrad.hip)");
    ViewGradDviewArgs G;
    G.view = (const float4 *)view; G.image = (const float4 *)image; G.pyramid = (const float4 *)pyramid; G.d_color = (const float4 *)d_color;
    G.out = (float4 *)d_view; G.ntexels = (uint32_t)n; G.width = p->width; G.height = p->height; G.L = P.L; G.filter = p->filter;
    G.footprint = p->footprint;
    if (zdr_launch_texel_gather_dview(G, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": the launch failed");
    return ZDR_OK;
}

extern "C" size_t zdr_texel_view_backward_workspace_bytes(int32_t tex_h, int32_t tex_w) {
    if (project_check_size(tex_h, tex_w)) return 0;
    return (size_t)zdr_viewgrad_rows((uint32_t)((size_t)tex_h * (size_t)tex_w)) * ZDR_VIEWGRAD_ROW * sizeof(double);
}

extern "C" int zdr_texel_view_backward(const zdr_texel_view_params *p, const float *texel_aovs, const float *d_view, float *d_camera, void *workspace,
                                       void *stream) {
    const char *name = "zdr_texel_view_backward";
    if (!p || !texel_aovs || !d_view || !d_camera || !workspace) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = filter_check_struct("zdr_texel_view_params.", p->struct_size, sizeof(zdr_texel_view_params))) return rc;
    if (int rc = filter_check_pointers(name, {(const void *)texel_aovs, (const void *)d_view, (const void *)d_camera, (const void *)workspace})) return rc;
    if (int rc = project_check_size(p->tex_h, p->tex_w)) return rc;
    if (int rc = project_check_image(name, p->width, p->height)) return rc;
    if (!(p->camera.fov > 0.0f && p->camera.fov < 3.14159265358979323846f))       // (false for a NaN)
        return fail(ZDR_E_INVALID, std::string(name) + ": camera.fov must be finite and lie in (0, pi)");
    const size_t n = (size_t)p->tex_h * (size_t)p->tex_w, wbytes = zdr_texel_view_backward_workspace_bytes(p->tex_h, p->tex_w);
    if (denoise_overlap(d_camera, 10 * sizeof(float), {{workspace, wbytes}, {texel_aovs, 64 * n}, {d_view, 32 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": d_camera must not overlap the workspace or an input");
    if (denoise_overlap(workspace, wbytes, {{texel_aovs, 64 * n}, {d_view, 32 * n}}))
        return fail(ZDR_E_INVALID, std::string(name) + ": the workspace must not overlap an input");
    if (!zdr_launch_texel_view_backward)                             // (weak: csrc/viewgrad.h)
        return fail(ZDR_E_UNSUPPORTED, "this library was linked without the camera-gradient kernels (zdr_viewgrad.hip)");
    ViewGradCameraArgs A;
    A.texels = (const float4 *)texel_aovs; A.d_view = (const float4 *)d_view; A.rows = (double *)workspace; A.d_camera = d_camera;
    A.ntexels = (uint32_t)n; A.nrows = zdr_viewgrad_rows((uint32_t)n);
    A.half_w = 0.5f * (float)p->width; A.half_h = 0.5f * (float)p->height;
    A.aspect = (float)p->height / (float)p->width;                   // (as zdr_scene_texel_view)
    camera_frame(p->camera, A.cam_o, A.cam_fwd, A.cam_right, A.cam_upp, A.cam_tan);
    for (int k = 0; k < 3; k++) { A.target[k] = p->camera.target[k]; A.up[k] = p->camera.up[k]; }
    A.fov = p->camera.fov;
    if (zdr_launch_texel_view_backward(A, (hipStream_t)stream)) return fail(ZDR_E_HIP, std::string(name) + ": a launch failed");
    return ZDR_OK;
}

extern "C" int zdr_render_stats(zdr_scene *s, const zdr_render_params *p, const float *material, uint64_t counters[8], void *stream) {
    if (!s || !counters) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemsetAsync(s->d_counters, 0, 8 * sizeof(unsigned long long), st));
    RenderCall c; c.material = material; c.stats = true; c.stream = stream;
    int rc = render_common(s, p, c); if (rc) return rc;
    unsigned long long h[8];
    HIPCHK(hipMemcpyAsync(h, s->d_counters, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 8; i++) counters[i] = h[i];
    return check_device_error(s, st);
}

extern "C" int zdr_trace_closest(zdr_scene *s, const float *rays, uint32_t n, int32_t *inst_prim, float *bary_t, void *stream) {
    if (!s || !rays || !inst_prim || !bary_t) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (zdr_launch_trace(s->ds, s->accel_is_bvh, 0, rays, n, inst_prim, bary_t, (hipStream_t)stream)) return fail(ZDR_E_HIP, "trace launch failed");
    return ZDR_OK;
}

extern "C" int zdr_trace_any(zdr_scene *s, const float *rays, uint32_t n, int32_t *occluded, void *stream) {
    if (!s || !rays || !occluded) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (zdr_launch_trace(s->ds, s->accel_is_bvh, 1, rays, n, occluded, nullptr, (hipStream_t)stream)) return fail(ZDR_E_HIP, "trace launch failed");
    return ZDR_OK;
}

extern "C" int zdr_trace_fused(zdr_scene *s, const float *shadow_rays, const float *next_rays, const int32_t *need, uint32_t n, int32_t backward_layout,
                               int32_t *occluded, int32_t *inst_prim, float *bary_t, void *stream) {
    if (!s) return fail(ZDR_E_INVALID, "null argument");
    if (!s->accel_is_bvh) return fail(ZDR_E_UNSUPPORTED, "the fused walk exists for BVH scenes only (a brute-force scene walks its two rays one after the other)");
    if (n == 0) return ZDR_OK;
    if (!shadow_rays || !next_rays || !need || !occluded || !inst_prim || !bary_t) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (zdr_launch_trace_fused(s->ds, shadow_rays, next_rays, need, n, backward_layout, occluded, inst_prim, bary_t, (hipStream_t)stream)) return fail(ZDR_E_HIP, "fused trace launch failed");
    return ZDR_OK;
}

extern "C" int zdr_path_dump(zdr_scene *s, const zdr_render_params *p, const float *material, const float *d_image,
                             const int32_t *queries, uint32_t n, int32_t maxv, float *out, void *stream) {
    if (!s || !p || !material || !queries || !out) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = check_params_abi(p)) return rc;
    if (p->integrator != ZDR_PATH) return fail(ZDR_E_UNSUPPORTED, "path traces exist for the path integrator only");
    if (maxv < 1 || maxv > ZDR_MAX_RECORDED_DEPTH) return fail(ZDR_E_INVALID, "maxv must lie in [1, 16]");
    HIPCHK(hipSetDevice(s->device));
    RenderCfg R; SamplerCfg C;
    int rc = make_render_cfg(p, true, R); if (rc) return rc;
    rc = make_sampler_cfg(s, p->sampler, p->seed, p->spp, C); if (rc) return rc;
    KernelIO io; memset(&io, 0, sizeof io);
    io.material = (const float4 *)material; io.d_image = (const float4 *)d_image;
    io.wide_offsets = wide_offsets_for((size_t)p->tex_h * (size_t)p->tex_w, (size_t)p->width * (size_t)p->height);
    DScene S = s->ds;
    S.shadow_pairs = (S.env_count > 0) ? ~0ull : s->shadow_pairs;
    if (zdr_launch_path_dump(S, R, C, io, s->accel_is_bvh, queries, n, maxv, out, (hipStream_t)stream)) return fail(ZDR_E_HIP, "path dump launch failed");
    return ZDR_OK;
}

extern "C" int zdr_shading_dump(zdr_scene *s, int32_t mode, const float *in, uint32_t n, float *out, void *stream) {
    if (!s) return fail(ZDR_E_INVALID, "null argument");
    if (mode != ZDR_SHADING_EVAL && mode != ZDR_SHADING_SAMPLE && mode != ZDR_SHADING_FRAME) return fail(ZDR_E_INVALID, "unknown shading dump mode");
    if (n == 0) return ZDR_OK;
    if (!in || !out) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (zdr_launch_shading_dump(mode, in, n, out, (hipStream_t)stream)) return fail(ZDR_E_HIP, "shading dump launch failed");
    return ZDR_OK;
}

extern "C" int zdr_light_dump(zdr_scene *s, int32_t mode, const float *in, uint32_t n, float *out, void *stream) {
    if (!s) return fail(ZDR_E_INVALID, "null argument");
    if (mode < ZDR_LIGHT_SAMPLE || mode > ZDR_LIGHT_INTERACT_WIDE) return fail(ZDR_E_INVALID, "unknown light dump mode");
    if (mode == ZDR_LIGHT_ENV && s->ds.env_count == 0) return fail(ZDR_E_INVALID, "the environment mode was asked for, but the scene has no environment map");
    if (n == 0) return ZDR_OK;
    if (!in || !out) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (zdr_launch_light_dump(s->ds, s->accel_is_bvh, mode, in, n, out, (hipStream_t)stream)) return fail(ZDR_E_HIP, "light dump launch failed");
    return ZDR_OK;
}

// The rows of a texture hook, read back and checked on the host before anything is launched: every material index names a material
// of the table (or, env_entry, the map's entry; negative = an inactive row, where the hook has such rows).  stride: floats per row.
static int check_texture_rows(const float *rows, uint32_t n, int stride, int mat_at, uint32_t nmat, bool inactive_ok, bool env_entry, hipStream_t st) {
    std::vector<float> h((size_t)n * stride);
    HIPCHK(hipMemcpyAsync(h.data(), rows, h.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++) {
        int32_t k; memcpy(&k, &h[(size_t)i * stride + mat_at], sizeof k);
        if (k < 0 && inactive_ok) continue;
        if (env_entry && k == ZDR_ENV_ENTRY) continue;
        if (k < 0 || (uint32_t)k >= nmat) return fail(ZDR_E_INVALID, "row " + std::to_string(i) + " names material " + std::to_string(k) + ", but " + std::to_string(nmat) + " materials were passed");
    }
    return ZDR_OK;
}

extern "C" int zdr_texture_lookup(zdr_scene *s, const float *materials, const int32_t *dims, uint32_t nmat, const float *rows, uint32_t n,
                                  float *out, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (!s) return fail(ZDR_E_INVALID, "null argument");
    if (int rc = check_table_args(true, dims, nmat)) return rc;
    MaterialTable mt;
    if (int rc = pack_material_table(dims, nmat, mt)) return rc;
    if (n == 0) return ZDR_OK;
    if (!materials || !rows || !out) return fail(ZDR_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(s->device));
    if (stream_is_capturing(st)) return fail(ZDR_E_UNSUPPORTED, "the texture hooks read their rows back to check them: they cannot be captured");
    if (int rc = check_texture_rows(rows, n, 4, 2, nmat, false, false, st)) return rc;
    if (zdr_launch_texture_lookup(s->ds, materials, mt, rows, n, out, st)) return fail(ZDR_E_HIP, "texture lookup launch failed");
    return ZDR_OK;
}

extern "C" int zdr_texture_scatter(zdr_scene *s, int32_t form, const int32_t *dims, uint32_t nmat, const float *rows, uint32_t n, uint32_t rounds,
                                   float *d_materials, float *d_env, int32_t *copies, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (!s) return fail(ZDR_E_INVALID, "null argument");
    if (form != ZDR_SCATTER_SINGLE && form != ZDR_SCATTER_TABLE && form != ZDR_SCATTER_TABLE_ENV) return fail(ZDR_E_INVALID, "unknown texture scatter form");
    if (int rc = check_table_args(true, dims, nmat)) return rc;
    if (form == ZDR_SCATTER_SINGLE && nmat != 1) return fail(ZDR_E_INVALID, "the single-material form takes one material");
    if (form == ZDR_SCATTER_TABLE_ENV) {                // what render_common and render_backward_call ask of an environment-gradient call
        if (nmat > ZDR_ENV_ENTRY) return fail(ZDR_E_INVALID, "the form with the environment map takes at most " + std::to_string(ZDR_ENV_ENTRY) + " materials (the map is the last entry of the material table)");
        if (s->ds.env_count == 0) return fail(ZDR_E_INVALID, "the form with the environment map was asked for, but the scene has no environment map");
    }
    if (rounds < 1 || rounds > 65536) return fail(ZDR_E_INVALID, "rounds must lie in [1, 65536]");
    HIPCHK(hipSetDevice(s->device));
    RenderCfg R; memset(&R, 0, sizeof R);
    KernelIO io; memset(&io, 0, sizeof io);
    MaterialTable mt;
    if (int rc = pack_material_table(dims, nmat, mt)) return rc;
    size_t ncells = (size_t)mt.ncells, env_cells_total = 0;
    if (form == ZDR_SCATTER_SINGLE) {                   // zdr_render_backward: make_render_cfg, no table
        R.tex_h = dims[0]; R.tex_w = dims[1];
        R.cell_copies = cell_copies_for(ncells);
        memset(&mt, 0, sizeof mt);
    } else {                                            // zdr_render_backward_materials[_env]: render_common
        material_cell_layout(mt, R);
        ncells = (size_t)mt.ncells;
        if (form == ZDR_SCATTER_TABLE_ENV) { if (int rc = env_cell_layout(s, mt, R, env_cells_total)) return rc; }
    }
    if (copies) {
        for (int k = 0; k < ZDR_MAX_MATERIALS; k++) copies[k] = (k < (int)nmat) ? (form == ZDR_SCATTER_SINGLE ? R.cell_copies : mt.m[k].copies) : 0;
        if (form == ZDR_SCATTER_TABLE_ENV) copies[ZDR_ENV_ENTRY] = mt.m[ZDR_ENV_ENTRY].texel;
    }
    if (n == 0) return ZDR_OK;
    if (!rows || !d_materials || (form == ZDR_SCATTER_TABLE_ENV && !d_env)) return fail(ZDR_E_INVALID, "null argument");
    const bool capturing = stream_is_capturing(st);
    if (capturing) return fail(ZDR_E_UNSUPPORTED, "the texture hooks read their rows back to check them: they cannot be captured");
    if (int rc = check_texture_rows(rows, n, 8, 6, nmat, true, form == ZDR_SCATTER_TABLE_ENV, st)) return rc;
    if (int rc = ensure_cells(s, R, ncells, st, capturing, env_cells_total)) return rc;
    io.cells = s->d_cells; io.d_material = d_materials; io.mt = mt;
    if (zdr_launch_texture_scatter(R, io, form != ZDR_SCATTER_SINGLE, form == ZDR_SCATTER_TABLE_ENV ? d_env : nullptr, rows, n, rounds, st))
        return fail(ZDR_E_HIP, "texture scatter launch failed");
    return ZDR_OK;
}

extern "C" int zdr_sampler_dump(zdr_scene *s, int32_t sampler, uint32_t seed, uint32_t spp, const int32_t *queries, uint32_t n,
                                int32_t nvert, int32_t rr_depth, float *out, void *stream) {
    if (!s || !queries || !out || nvert < 0) return fail(ZDR_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(s->device));
    SamplerCfg C;
    int rc = make_sampler_cfg(s, sampler, seed, spp, C); if (rc) return rc;
    if (zdr_launch_sampler_dump(C, queries, n, nvert, rr_depth, out, 0, nullptr, (hipStream_t)stream)) return fail(ZDR_E_HIP, "sampler dump launch failed");
    return ZDR_OK;
}

extern "C" int zdr_vertex_sampler_dump(zdr_scene *s, int32_t integrator, int32_t sampler, uint32_t seed, uint32_t spp, const int32_t *queries, uint32_t n,
                                       int32_t nvert, int32_t rr_depth, float *out, int32_t *batched, void *stream) {
    if (!s || !queries || !out || nvert < 0) return fail(ZDR_E_INVALID, "bad argument");
    if (integrator != ZDR_PATH && integrator != ZDR_DIRECT) return fail(ZDR_E_INVALID, "the path and the direct integrator have draw routes of their own");
    HIPCHK(hipSetDevice(s->device));
    SamplerCfg C;
    int rc = make_sampler_cfg(s, sampler, seed, spp, C); if (rc) return rc;
    int b = 0;
    if (zdr_launch_sampler_dump(C, queries, n, nvert, rr_depth, out, integrator == ZDR_DIRECT ? 2 : 1, &b, (hipStream_t)stream)) return fail(ZDR_E_HIP, "sampler dump launch failed");
    if (batched) *batched = b;
    return ZDR_OK;
}
