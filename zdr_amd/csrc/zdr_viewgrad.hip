// zdr_viewgrad.hip — camera gradients of the texture-space views for gfx950 (include/zdr.h, "Camera gradients": zdr_texel_gather_dview,
// zdr_texel_view_backward): what a gather's colour cotangent says about the view buffer, and what a view buffer's cotangent says about
// the camera.  Visibility is held fixed; everything else in the view buffer is a closed form of the camera.  Linked into
// libzdr_viewgrad.so (zdr_amd/build.py), compiled without contraction and without the atomics option: there is no atomic here, and
// the bits are defined by the operation order of include/zdr.h.
//
//   k_vg_dview<filter>  thread = texel, like k_proj_gather and k_mip_gather: the view row, then — only where the texel is visible — the
//                       colour cotangent and the taps the forward reads; two float4 stores.  The arithmetic is texel_filter.h's tf_dview.
//   k_vg_partial        stage 1 of the camera sums.  Lane g of the grid's G = 256 nrows lanes takes the texels g, g + G, g + 2G ..
//                       ascending, so a wave reads 64 consecutive rows at a time; per shaded texel the 13 partial derivatives
//                       (o, fwd, right, upp, tan) in float32, added into 13 float64 sums.  Then the wave's tree (lane i takes lane
//                       i + 32, then 16, 8, 4, 2, 1), then the four waves in wave order through LDS: one row per workgroup.
//   k_vg_camera         stage 2, ONE workgroup: lane (slot, j) adds sum j of the rows slot, slot + 16, slot + 32 .. ascending, then lane j
//                       adds the 16 slots in slot order, then lane 0 takes the 13 totals through the chain rule of camera_frame in
//                       float64 and stores the 10 floats.
// The sums are float64 because the terms cancel (a texel left of the axis against one right of it) and the 13 totals are differenced
// once more by the chain rule (d_fwd lies mostly along fwd, which the normalisation projects out): with float64 sums the result's error
// is that of the float32 terms.  No scratch, 480 + 1,664 bytes of LDS, nothing read that the same call did not write.
#include "viewgrad.h"
#include "texel_filter.h"

#define VG_BLOCK ZDR_VIEWGRAD_BLOCK
#define VG_SUMS ZDR_VIEWGRAD_SUMS
#define VG_ROW ZDR_VIEWGRAD_ROW
#define VG_SLOTS (VG_BLOCK / VG_ROW)
#define ZD __device__ __forceinline__

template <int FILTER>
__global__ __launch_bounds__(256) void k_vg_dview(ViewGradDviewArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    float dX = 0.0f, dY = 0.0f, dS = 0.0f;
    if (t < G.ntexels) {
        const float4 vw = G.view[2 * (size_t)t];             // {visible, cosine, X, Y}
        if (tf_on(vw.x)) {                                   // an invisible texel reads nothing of the image, the pyramid or d_color
            const float4 d = G.d_color[t];
            float s = 1.0f;
            if (FILTER == TF_MIP) s = G.view[2 * (size_t)t + 1].z * G.footprint;
            const tf_dview_t r = tf_dview(G.image, G.pyramid, vw.x, vw.z, vw.w, s, G.footprint, FILTER == TF_MIP ? G.L : 0, G.width, G.height, d);
            dX = r.dX; dY = r.dY; dS = r.dS;
        }
    }
    // The wave's 64 rows are 128 consecutive float4: lane l stores the l-th and the (64 + l)-th of them, so that each store instruction
    // writes 1 KiB in one piece (a lane storing its own row's two halves writes 16 of every 32 bytes, twice).  The whole wave is here:
    // no lane left before the shuffles.  Half h of the rows lies with the lanes 32 h .. 32 h + 31; an even float4 is {0, 0, d_X, d_Y}.
    const uint32_t first = 2u * (t - lane), end = 2u * G.ntexels;     // (float4 indices: at most 2^27)
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int src = 32 * h + (int)(lane >> 1);
        const float x = __shfl(dX, src, 64), y = __shfl(dY, src, 64), s = __shfl(dS, src, 64);
        const uint32_t q = first + 64u * (uint32_t)h + lane;
        if (q < end) G.out[q] = (lane & 1u) ? make_float4(0.f, 0.f, s, 0.f) : make_float4(0.f, 0.f, x, y);
    }
}

struct vg3 { float x, y, z; };
ZD vg3 vg_ld(const float *p) { vg3 r; r.x = p[0]; r.y = p[1]; r.z = p[2]; return r; }
ZD float vg_dot(vg3 a, vg3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ZD bool vg_nan(float4 a) { return a.x != a.x || a.y != a.y || a.z != a.z; }

// the 13 partial derivatives of one shaded texel, in float32, added into S: gv is the cotangent of v = p - o, so d_o = -gv
ZD void vg_texel(const ViewGradCameraArgs &A, float4 nr, float4 ps, float4 g0, float4 g1, double (&S)[VG_SUMS]) {
    const vg3 o = vg_ld(A.cam_o), fwd = vg_ld(A.cam_fwd), right = vg_ld(A.cam_right), upp = vg_ld(A.cam_upp);
    vg3 v; v.x = ps.x - o.x; v.y = ps.y - o.y; v.z = ps.z - o.z;
    const float z = vg_dot(v, fwd), dist = __fsqrt_rn(vg_dot(v, v));
    vg3 wi; wi.x = __fdiv_rn(-v.x, dist); wi.y = __fdiv_rn(-v.y, dist); wi.z = __fdiv_rn(-v.z, dist);
    const float cosine = nr.x * wi.x + nr.y * wi.y + nr.z * wi.z;
    const float g_cos = g0.y, g_X = g0.z, g_Y = g0.w, g_depth = g1.x, g_dist = g1.y, g_scale = g1.z;
    // cosine: -(n - cosine wi) / dist;  distance: v / dist = -wi
    const float kc = __fdiv_rn(g_cos, dist);
    float gz = g_depth, ga = 0.0f, gb = 0.0f, gt = 0.0f;
    if (z > 0.0f) {                                          // elsewhere X, Y and scale are the constant 0
        const float a = vg_dot(v, right), b = vg_dot(v, upp);
        const float kx = __fdiv_rn(A.half_w, z * A.cam_tan), ky = __fdiv_rn(A.half_h, z * (A.cam_tan * A.aspect));
        const float qx = __fdiv_rn(a, z), qy = __fdiv_rn(b, z);
        const float scale = __fdiv_rn(nr.w * A.half_w, A.cam_tan * z);
        ga = g_X * kx; gb = -(g_Y * ky);
        const float gxy = g_Y * (ky * qy) - g_X * (kx * qx);  // d/dz of X and Y together; times z / tan it is their d/dtan
        const float gs = g_scale * scale;
        gz = (g_depth + gxy) - __fdiv_rn(gs, z);
        gt = __fdiv_rn(gxy * z - gs, A.cam_tan);
    }
    const float gvx = ((gz * fwd.x + ga * right.x) + gb * upp.x) - (kc * (nr.x - cosine * wi.x) + g_dist * wi.x);
    const float gvy = ((gz * fwd.y + ga * right.y) + gb * upp.y) - (kc * (nr.y - cosine * wi.y) + g_dist * wi.y);
    const float gvz = ((gz * fwd.z + ga * right.z) + gb * upp.z) - (kc * (nr.z - cosine * wi.z) + g_dist * wi.z);
    S[0] += (double)(-gvx); S[1] += (double)(-gvy); S[2] += (double)(-gvz);
    S[3] += (double)(gz * v.x); S[4] += (double)(gz * v.y); S[5] += (double)(gz * v.z);
    S[6] += (double)(ga * v.x); S[7] += (double)(ga * v.y); S[8] += (double)(ga * v.z);
    S[9] += (double)(gb * v.x); S[10] += (double)(gb * v.y); S[11] += (double)(gb * v.z);
    S[12] += (double)gt;
}

__global__ __launch_bounds__(VG_BLOCK) void k_vg_partial(ViewGradCameraArgs A) {
    __shared__ double part[VG_BLOCK / 64][VG_SUMS + 2];     // (15 doubles a wave)
    double S[VG_SUMS];
#pragma unroll
    for (int j = 0; j < VG_SUMS; j++) S[j] = 0.0;
    const uint32_t stride = A.nrows * VG_BLOCK;              // (<= 2^18)
    for (uint32_t t = blockIdx.x * VG_BLOCK + threadIdx.x; t < A.ntexels; t += stride) {   // (ntexels <= 2^26: t + stride does not wrap)
        const float4 *r = A.texels + 4 * (size_t)t;
        const float4 nr = r[1], ps = r[2];
        const float reach = r[3].x;
        if (reach == 1.0f && !vg_nan(nr) && !vg_nan(ps))     // the forward's rule; a texel that is not shaded: its d_view row is not read
            vg_texel(A, nr, ps, A.d_view[2 * (size_t)t], A.d_view[2 * (size_t)t + 1], S);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int j = 0; j < VG_SUMS; j++) S[j] += __shfl_down(S[j], off, 64);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
#pragma unroll
        for (int j = 0; j < VG_SUMS; j++) part[wave][j] = S[j];
    }
    __syncthreads();
    if (threadIdx.x < VG_SUMS) {
        double s = part[0][threadIdx.x];
        for (int w = 1; w < VG_BLOCK / 64; w++) s += part[w][threadIdx.x];
        A.rows[(size_t)blockIdx.x * VG_ROW + threadIdx.x] = s;
    }
}

struct vgd3 { double x, y, z; };
ZD vgd3 vgd(double x, double y, double z) { vgd3 r; r.x = x; r.y = y; r.z = z; return r; }
ZD vgd3 vgd_ld(const float *p) { return vgd((double)p[0], (double)p[1], (double)p[2]); }
ZD vgd3 vgd_add(vgd3 a, vgd3 b) { return vgd(a.x + b.x, a.y + b.y, a.z + b.z); }
ZD vgd3 vgd_sub(vgd3 a, vgd3 b) { return vgd(a.x - b.x, a.y - b.y, a.z - b.z); }
ZD vgd3 vgd_mul(vgd3 a, double s) { return vgd(a.x * s, a.y * s, a.z * s); }
ZD double vgd_dot(vgd3 a, vgd3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
ZD vgd3 vgd_cross(vgd3 a, vgd3 b) { return vgd(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

__global__ __launch_bounds__(VG_BLOCK) void k_vg_camera(ViewGradCameraArgs A) {
    __shared__ double slot[VG_SLOTS][VG_SUMS];
    const uint32_t j = threadIdx.x & (VG_ROW - 1u), sl = threadIdx.x / VG_ROW;
    if (j < VG_SUMS) {
        double s = 0.0;
        for (uint32_t r = sl; r < A.nrows; r += VG_SLOTS) s += A.rows[(size_t)r * VG_ROW + j];
        slot[sl][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < VG_SUMS) {
        double s = slot[0][threadIdx.x];
        for (int k = 1; k < VG_SLOTS; k++) s += slot[k][threadIdx.x];
        slot[0][threadIdx.x] = s;                            // (lane j alone reads and writes column j)
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    // the chain rule through camera_frame: d = target - o, fwd = d / |d|, c = fwd x up, right = c / |c|, upp = right x fwd, tan(fov / 2)
    const double *T = slot[0];
    const vgd3 g_o = vgd(T[0], T[1], T[2]), g_upp = vgd(T[9], T[10], T[11]);
    vgd3 g_fwd = vgd(T[3], T[4], T[5]), g_right = vgd(T[6], T[7], T[8]);
    // The frame once more, in float64 from the camera's own floats: the Jacobian of the exact map.  (With the float32 frame as values
    // right is not exactly c / |c|, and what the projections remove — d_up along up is 0 — would leak at 1e-7 of the totals.)
    const vgd3 up = vgd_ld(A.up), d = vgd_sub(vgd_ld(A.target), vgd_ld(A.cam_o));
    const double len = sqrt(vgd_dot(d, d));
    const vgd3 fwd = vgd_mul(d, 1.0 / len), c = vgd_cross(fwd, up);
    const double lc = sqrt(vgd_dot(c, c)), tn = tan(0.5 * (double)A.fov);
    const vgd3 right = vgd_mul(c, 1.0 / lc);
    g_right = vgd_add(g_right, vgd_cross(fwd, g_upp));                       // upp = right x fwd
    g_fwd = vgd_add(g_fwd, vgd_cross(g_upp, right));
    const vgd3 g_c = vgd_mul(vgd_sub(g_right, vgd_mul(right, vgd_dot(right, g_right))), 1.0 / lc);
    g_fwd = vgd_add(g_fwd, vgd_cross(up, g_c));                              // c = fwd x up
    const vgd3 g_up = vgd_cross(g_c, fwd);
    const vgd3 g_d = vgd_mul(vgd_sub(g_fwd, vgd_mul(fwd, vgd_dot(fwd, g_fwd))), 1.0 / len);
    const vgd3 g_origin = vgd_sub(g_o, g_d);
    float *out = A.d_camera;
    out[0] = (float)(T[12] * (0.5 * (1.0 + tn * tn)));
    out[1] = (float)g_origin.x; out[2] = (float)g_origin.y; out[3] = (float)g_origin.z;
    out[4] = (float)g_d.x; out[5] = (float)g_d.y; out[6] = (float)g_d.z;
    out[7] = (float)g_up.x; out[8] = (float)g_up.y; out[9] = (float)g_up.z;
}

int zdr_launch_texel_gather_dview(const ViewGradDviewArgs &G, hipStream_t st) {
    const dim3 grid((G.ntexels + 255u) / 256u);
    if (G.filter == TF_MIP) hipLaunchKernelGGL((k_vg_dview<TF_MIP>), grid, dim3(256), 0, st, G);
    else hipLaunchKernelGGL((k_vg_dview<TF_BILINEAR>), grid, dim3(256), 0, st, G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int zdr_launch_texel_view_backward(const ViewGradCameraArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(k_vg_partial, dim3(A.nrows), dim3(VG_BLOCK), 0, st, A);
    if (hipGetLastError() != hipSuccess) return -1;          // the next launch would read what this one did not write
    hipLaunchKernelGGL(k_vg_camera, dim3(1), dim3(VG_BLOCK), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
