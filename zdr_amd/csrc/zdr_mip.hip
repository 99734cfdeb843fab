// zdr_mip.hip — prefiltered projective texturing for gfx950 (include/zdr.h: zdr_image_pyramid, zdr_image_pyramid_backward,
// zdr_texel_gather_mip, zdr_texel_gather_mip_backward): the mip pyramid of a camera's image, the trilinear gather of image and pyramid
// into texture space with the level taken from each texel's on-screen footprint, and the exact transposes of both.  Linked into
// libzdr_mip.so (zdr_amd/build.py), compiled without contraction: the bits are defined by the operation order of include/zdr.h.
//
// The pyramid (csrc/mip.h has the layout): level 0 is the caller's image, the levels >= 1 sit packed in one buffer.
//   k_mip_down2        one thread per pixel of level l + 2: the up to 2 x 2 pixels of level l + 1 below it from 4 x 4 pixels of level l, then
//                      itself from those — TWO levels per launch, the first never read back from memory
//   k_mip_down1        one thread per pixel of level l + 1, where a single level is left before the tail
//   k_mip_tail_fwd     ONE workgroup: from the first level of at most 32 x 32 pixels every remaining level, in LDS (22 KB)
// and its adjoint T_l = G_l + (0.25 m_l) T_{l+1}[parent], a gather (every fine pixel has one parent), top-down:
//   k_mip_tail_bwd     ONE workgroup: the levels from the top down to the first of at most 32 x 32 pixels, in LDS; where that is level 0
//                      it adds into d_image and the whole call is this launch
//   k_mip_up2          one thread per pixel of level l: its parent's T_{l+1} from G_{l+1} and T_{l+2}, recomputed by each of the up to four
//                      children and not stored (the cotangent buffer is a workspace), then T_l in place — level 0 is d_image, added into
//   k_mip_up1          one thread per pixel of level l from T_{l+1}, where a single level is left
// A call is at most ceil(L / 2) + 1 launches: at these sizes a chain of dependent launches costs more than the data
// (profiles/push_pull_cost.txt).  Pixels are numbered row by row in grid.x, 256 to a block; every load and store is a float4 of a pixel,
// every store of a pixel that this thread alone owns: no atomics, no scratch, the same bits whatever the grid.  The level launches and
// the tails go through the SAME device functions (mip_box, mip_down, mip_coef, mip_up), so a level has the same bits in LDS, in a fused
// pair and in a launch of its own.
//
// The gather (k_mip_gather) is thread = texel, like k_proj_gather; it reads both float4 of the view row (scale is float 6).  Its adjoint
// (k_mip_scatter) is thread = (texel, channel), for the reason given above k_proj_scatter (zdr_project.hip): one float atomic per tap
// and channel (-munsafe-fp-atomics: global_atomic_add_f32, no compare-and-swap loop).  The level split, the places, the taps, the
// trilinear sample and the adjoint's walk are texel_filter.h's, shared with the other texel filters.
#include "mip.h"
#include "texel_filter.h"

#define MIP_BLOCK 256
#define ZD __device__ __forceinline__

ZD float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
ZD float4 f4scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
ZD int32_t mini(int32_t a, int32_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------- the pyramid, value by value
ZD float4 mip_box(float4 a00, float4 a01, float4 a10, float4 a11) { return f4scale(f4add(f4add(a00, a01), f4add(a10, a11)), 0.25f); }

// pixel (i, j) (row, column) of the coarser level;  fine(y, x) = the finer level (hf x wf), continued by its border pixels
template <class F>
ZD float4 mip_down(int i, int j, int hf, int wf, F fine) {
    const int y0 = 2 * i, y1 = mini(2 * i + 1, hf - 1), x0 = 2 * j, x1 = mini(2 * j + 1, wf - 1);
    return mip_box(fine(y0, x0), fine(y0, x1), fine(y1, x0), fine(y1, x1));
}

// 0.25 m(y, x) of a level (h x w): how often the parent counted this pixel, times the box weight (0.25, 0.5 or 1: exact)
ZD float mip_coef(int y, int x, int h, int w) {
    const float mx = ((w & 1) && x == w - 1) ? 2.0f : 1.0f, my = ((h & 1) && y == h - 1) ? 2.0f : 1.0f;
    return 0.25f * (mx * my);
}

ZD float4 mip_up(float4 g, float coef, float4 parent) { return f4add(g, f4scale(parent, coef)); }

// ---------------------------------------------------------------------------------------------------------------- level launches
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_down1(int wf, int hf, int wc, int hc, const float4 *__restrict__ src, float4 *__restrict__ dst) {
    const uint32_t idx = blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)wc * (uint32_t)hc) return;
    const int i = (int)(idx / (uint32_t)wc), j = (int)(idx - (uint32_t)i * (uint32_t)wc);
    dst[idx] = mip_down(i, j, hf, wf, [&](int y, int x) -> float4 { return src[(uint32_t)y * (uint32_t)wf + (uint32_t)x]; });
}

// src: level l (hf x wf);  mid: level l + 1 (h1 x w1);  top: level l + 2 (h2 x w2).  A thread owns pixel (I, J) of the top level and the
// pixels (2I + {0, 1}, 2J + {0, 1}) of the middle one that exist; a clamped index names a pixel it owns as well.
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_down2(int wf, int hf, int w1, int h1, int w2, int h2, const float4 *__restrict__ src,
                                                         float4 *__restrict__ mid, float4 *__restrict__ top) {
    const uint32_t idx = blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)w2 * (uint32_t)h2) return;
    const int I = (int)(idx / (uint32_t)w2), J = (int)(idx - (uint32_t)I * (uint32_t)w2);
    auto fine = [&](int y, int x) -> float4 { return src[(uint32_t)y * (uint32_t)wf + (uint32_t)x]; };
    const int i0 = 2 * I, j0 = 2 * J;                                 // (i0 < h1, j0 < w1)
    const bool row = i0 + 1 < h1, col = j0 + 1 < w1;
    const float4 m00 = mip_down(i0, j0, hf, wf, fine);
    const float4 m01 = col ? mip_down(i0, j0 + 1, hf, wf, fine) : m00;
    const float4 m10 = row ? mip_down(i0 + 1, j0, hf, wf, fine) : m00;
    const float4 m11 = row ? (col ? mip_down(i0 + 1, j0 + 1, hf, wf, fine) : m10) : m01;
    const uint32_t at = (uint32_t)i0 * (uint32_t)w1 + (uint32_t)j0;
    mid[at] = m00;
    if (col) mid[at + 1u] = m01;
    if (row) mid[at + (uint32_t)w1] = m10;
    if (row && col) mid[at + (uint32_t)w1 + 1u] = m11;
    top[idx] = mip_box(m00, m01, m10, m11);
}

// cur: level l (h x w), G_l in, T_l out (level 0: d_image, added into);  par: T_{l+1} (wc wide)
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_up1(int w, int h, int wc, float4 *cur, const float4 *__restrict__ par) {
    const uint32_t idx = blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)w * (uint32_t)h) return;
    const int y = (int)(idx / (uint32_t)w), x = (int)(idx - (uint32_t)y * (uint32_t)w);
    cur[idx] = mip_up(cur[idx], mip_coef(y, x, h, w), par[(uint32_t)(y >> 1) * (uint32_t)wc + (uint32_t)(x >> 1)]);
}

// cur: level l (h x w) as above;  mid: G_{l+1} (h1 x w1), only read;  top: T_{l+2} (w2 wide)
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_up2(int w, int h, int w1, int h1, int w2, float4 *cur, const float4 *__restrict__ mid,
                                                       const float4 *__restrict__ top) {
    const uint32_t idx = blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)w * (uint32_t)h) return;
    const int y = (int)(idx / (uint32_t)w), x = (int)(idx - (uint32_t)y * (uint32_t)w);
    const int py = y >> 1, px = x >> 1;
    const float4 t1 = mip_up(mid[(uint32_t)py * (uint32_t)w1 + (uint32_t)px], mip_coef(py, px, h1, w1),
                             top[(uint32_t)(py >> 1) * (uint32_t)w2 + (uint32_t)(px >> 1)]);
    cur[idx] = mip_up(cur[idx], mip_coef(y, x, h, w), t1);
}

// ------------------------------------------------------------------------------------------------------------------ the fused tails
// src: the base level (h0 x w0 <= 32 x 32);  dst: where the next level begins in the packed buffer — the nlev levels above the base
// follow one another there as they do in LDS
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_tail_fwd(int w0, int h0, int nlev, const float4 *__restrict__ src, float4 *__restrict__ dst) {
    __shared__ float4 V[ZDR_MIP_TAIL_TEXELS];
    const int tid = (int)threadIdx.x, n0 = w0 * h0;
    for (int t = tid; t < n0; t += MIP_BLOCK) V[t] = src[t];
    int wf = w0, hf = h0, off = 0;
    for (int l = 0; l < nlev; l++) {
        __syncthreads();
        const int wc = (wf + 1) >> 1, hc = (hf + 1) >> 1, offc = off + wf * hf;
        for (int t = tid; t < wc * hc; t += MIP_BLOCK) {
            const int i = t / wc, j = t - i * wc;
            const float4 v = mip_down(i, j, hf, wf, [&](int y, int x) -> float4 { return V[off + y * wf + x]; });
            V[offc + t] = v;
            dst[offc - n0 + t] = v;
        }
        off = offc; wf = wc; hf = hc;
    }
}

// g: the cotangents of the nlev + 1 levels from the base (h0 x w0) to the top, packed; T of the base level is left in its place.  With
// `image` the base is level 1 of an image (hi x wi <= 32 x 32) and d_image receives (0.25 m_0) T_1[parent] on top of what it holds.
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_tail_bwd(int w0, int h0, int nlev, float4 *g, int wi, int hi, float4 *image) {
    __shared__ float4 V[ZDR_MIP_TAIL_TEXELS];
    const int tid = (int)threadIdx.x;
    int total = 0;
    for (int l = 0; l <= nlev; l++) total += ((w0 + (1 << l) - 1) >> l) * ((h0 + (1 << l) - 1) >> l);
    for (int t = tid; t < total; t += MIP_BLOCK) V[t] = g[t];
    for (int l = nlev - 1; l >= 0; l--) {                            // T of level l (above the base) from its parents
        __syncthreads();
        int off = 0;
        for (int k = 0; k < l; k++) off += ((w0 + (1 << k) - 1) >> k) * ((h0 + (1 << k) - 1) >> k);
        const int w = (w0 + (1 << l) - 1) >> l, h = (h0 + (1 << l) - 1) >> l, wc = (w + 1) >> 1, offc = off + w * h;
        for (int t = tid; t < w * h; t += MIP_BLOCK) {
            const int y = t / w, x = t - y * w;
            V[off + t] = mip_up(V[off + t], mip_coef(y, x, h, w), V[offc + (y >> 1) * wc + (x >> 1)]);
        }
    }
    __syncthreads();
    if (image) {
        for (int t = tid; t < wi * hi; t += MIP_BLOCK) {
            const int y = t / wi, x = t - y * wi;
            image[t] = mip_up(image[t], mip_coef(y, x, hi, wi), V[(y >> 1) * w0 + (x >> 1)]);
        }
    } else {
        for (int t = tid; t < w0 * h0; t += MIP_BLOCK) g[t] = V[t];
    }
}

// ------------------------------------------------------------------------------------------------------------------ the gather
__global__ __launch_bounds__(256) void k_mip_gather(MipGatherArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t], vs = G.view[2 * (size_t)t + 1];   // {visible, cosine, X, Y}, {depth, distance, scale, 0}
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tf_on(vw.x)) {                                       // an invisible texel reads nothing of the image or the pyramid
        const tf_level_t lv = tf_level(vs.z * G.footprint, G.L);
        const tf_place_t lo = tf_place(G.width, G.height, lv.l0);
        const float4 r = tf_trilinear(G.in, G.pyramid, vw.z, vw.w, lv, lo, tf_above(lo, lv.l0));
        c = make_float4(vw.x * r.x, vw.x * r.y, vw.x * r.z, vw.x * r.w);
    }
    G.out[t] = c;
}

__global__ __launch_bounds__(256) void k_mip_scatter(MipGatherArgs G) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, t = id >> 2, c = id & 3u;   // (id < 4 ntexels <= 2^28)
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];
    if (!tf_on(vw.x)) return;
    const float scale = ((const float *)G.view)[8 * (size_t)t + 6];
    tf_texel_t x = tf_texel(vw.x, vw.z, vw.w);
    x.lv = tf_level(scale * G.footprint, G.L);
    const float g = ((const float *)G.in)[id];
    float *d_image = (float *)G.out + c, *d_pyramid = (float *)G.d_pyramid + c;
    tf_enumerate(x, TF_MIP, G.footprint, G.width, G.height,
                 [&](bool pyramid, uint32_t pixel, float weight) { atomicAdd((pyramid ? d_pyramid : d_image) + 4 * (size_t)pixel, weight * g); });
}


// ------------------------------------------------------------------------------------------------------------------------ launchers
static dim3 mip_grid(int w, int h) { return dim3((unsigned)(((size_t)w * (size_t)h + MIP_BLOCK - 1) / MIP_BLOCK)); }

int zdr_launch_image_pyramid(const MipPyramidArgs &A, int backward, hipStream_t st) {
    const MipPlan P = zdr_mip_plan(A.width, A.height, A.levels);
    const dim3 block(MIP_BLOCK);
    const bool fused = P.tail <= P.L;
    const int upto = fused ? P.tail : P.L;                           // the level launches make (or, backward, start from) this level
    auto lev = [&](int l) { return A.pyramid + P.off[l]; };          // l >= 1
    if (!backward) {
        for (int l = 0; l < upto;) {
            const float4 *src = l == 0 ? A.image : (const float4 *)lev(l);
            if (l + 2 <= upto) {
                hipLaunchKernelGGL(k_mip_down2, mip_grid(P.w[l + 2], P.h[l + 2]), block, 0, st, P.w[l], P.h[l], P.w[l + 1], P.h[l + 1], P.w[l + 2], P.h[l + 2],
                                   src, lev(l + 1), lev(l + 2));
                l += 2;
            } else {
                hipLaunchKernelGGL(k_mip_down1, mip_grid(P.w[l + 1], P.h[l + 1]), block, 0, st, P.w[l], P.h[l], P.w[l + 1], P.h[l + 1], src, lev(l + 1));
                l += 1;
            }
            if (hipGetLastError() != hipSuccess) return -1;          // the next launch would read what this one did not write
        }
        if (fused && P.tail < P.L) {
            const int T = P.tail;
            hipLaunchKernelGGL(k_mip_tail_fwd, dim3(1), block, 0, st, P.w[T], P.h[T], P.L - T, T == 0 ? A.image : (const float4 *)lev(T), lev(T + 1));
        }
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    if (P.L == 0) return 0;                                          // no level >= 1: nothing reaches the image
    if (fused) {
        const int T = P.tail, base = T == 0 ? 1 : T;
        if (T == 0) hipLaunchKernelGGL(k_mip_tail_bwd, dim3(1), block, 0, st, P.w[1], P.h[1], P.L - 1, lev(1), P.w[0], P.h[0], A.d_image);
        else if (base < P.L) hipLaunchKernelGGL(k_mip_tail_bwd, dim3(1), block, 0, st, P.w[T], P.h[T], P.L - T, lev(T), 0, 0, (float4 *)nullptr);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    for (int t = upto; t > 0;) {                                     // T_t is in place; the levels below it, two at a time
        if (t >= 2) {
            const int l = t - 2;
            hipLaunchKernelGGL(k_mip_up2, mip_grid(P.w[l], P.h[l]), block, 0, st, P.w[l], P.h[l], P.w[l + 1], P.h[l + 1], P.w[l + 2],
                               l == 0 ? A.d_image : lev(l), (const float4 *)lev(l + 1), (const float4 *)lev(l + 2));
            t -= 2;
        } else {
            hipLaunchKernelGGL(k_mip_up1, mip_grid(P.w[0], P.h[0]), block, 0, st, P.w[0], P.h[0], P.w[1], A.d_image, (const float4 *)lev(1));
            t -= 1;
        }
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

int zdr_launch_texel_gather_mip(const MipGatherArgs &G, int backward, hipStream_t st) {
    if (backward) hipLaunchKernelGGL(k_mip_scatter, dim3((G.ntexels + 63u) / 64u), dim3(256), 0, st, G);
    else hipLaunchKernelGGL(k_mip_gather, dim3((G.ntexels + 255u) / 256u), dim3(256), 0, st, G);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
