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
// and channel (-munsafe-fp-atomics: global_atomic_add_f32, no compare-and-swap loop).
#include "mip.h"

#define MIP_BLOCK 256
#define ZD __device__ __forceinline__

ZD float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
ZD float4 f4scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
ZD int32_t mini(int32_t a, int32_t b) { return a < b ? a : b; }
ZD int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

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

// ------------------------------------------------------------------------------------------------------------- the level of a texel
// s = max(scale footprint, 1), NaN -> 1;  l0 = its binary exponent, f = log2 of its mantissa in [1, 2); at or beyond the top level: L, 0.
// The split is integer work on the float's bits: only f carries rounding.
struct MipLevel { int l0; float f; };
ZD MipLevel mip_level(float scale, float footprint, int L) {
    float s = scale * footprint;
    s = s > 1.0f ? s : 1.0f;
    const uint32_t b = __float_as_uint(s);
    MipLevel r;
    r.l0 = (int)(b >> 23) - 127;                                    // (s >= 1: no sign, an exponent field of at least 127; infinity: 128)
    r.f = 0.0f;
    if (r.l0 >= L) { r.l0 = L; return r; }
    const float m = __uint_as_float((b & 0x007fffffu) | 0x3f800000u);
    if (m != 1.0f) r.f = fminf(log2f(m), 1.0f);
    return r;
}

// size of level l and where it begins in the packed buffer (float4; level 0 is the image and has no place there).  A loop, not a table
// in the kernel's arguments: l differs from lane to lane, and l0 is small wherever the gather is worth calling.
struct MipPlace { int w, h; size_t off; };
ZD MipPlace mip_place(int width, int height, int l) {
    MipPlace p;
    p.w = width; p.h = height; p.off = 0;
    for (int k = 1; k <= l; k++) {
        if (k > 1) p.off += (size_t)p.w * (size_t)p.h;
        p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    }
    return p;
}
ZD MipPlace mip_above(MipPlace p, int l) {                           // level l + 1 from level l
    if (l >= 1) p.off += (size_t)p.w * (size_t)p.h;
    p.w = (p.w + 1) >> 1; p.h = (p.h + 1) >> 1;
    return p;
}

// The taps of one texel in a level: the rule of proj_taps (zdr_project.hip; include/zdr.h, zdr_texel_gather) with that level's size.
struct MipTaps { int32_t i00, i01, i10, i11; float tx, ty; };
ZD MipTaps mip_taps(float X, float Y, int32_t width, int32_t height) {
    const float fx = X - 0.5f, fy = Y - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    MipTaps T;
    T.tx = fx - x0f; T.ty = fy - y0f;
    const int32_t x0 = (int32_t)fminf(fmaxf(x0f, -1.0f), (float)width), y0 = (int32_t)fminf(fmaxf(y0f, -1.0f), (float)height);
    const int32_t xa = clampi(x0, 0, width - 1), xb = clampi(x0 + 1, 0, width - 1);
    const int32_t ya = clampi(y0, 0, height - 1), yb = clampi(y0 + 1, 0, height - 1);
    T.i00 = ya * width + xa; T.i01 = ya * width + xb; T.i10 = yb * width + xa; T.i11 = yb * width + xb;
    return T;
}

ZD float4 mip_lerp(float4 a, float4 b, float t) {
    return make_float4(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t, a.w + (b.w - a.w) * t);
}

ZD float mip_exp2_neg(int l) { return __uint_as_float((uint32_t)(127 - l) << 23); }   // 2^-l, l <= 31: the scaling of X, Y is exact

ZD float4 mip_sample(const float4 *lvl, float X, float Y, int l, MipPlace p) {
    const float inv = mip_exp2_neg(l);
    const MipTaps T = mip_taps(X * inv, Y * inv, p.w, p.h);
    const float4 top = mip_lerp(lvl[T.i00], lvl[T.i01], T.tx), bot = mip_lerp(lvl[T.i10], lvl[T.i11], T.tx);
    return mip_lerp(top, bot, T.ty);
}

__global__ __launch_bounds__(256) void k_mip_gather(MipGatherArgs G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t], vs = G.view[2 * (size_t)t + 1];   // {visible, cosine, X, Y}, {depth, distance, scale, 0}
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vw.x != 0.0f && vw.x == vw.x) {                      // an invisible texel reads nothing of the image or the pyramid
        const MipLevel lv = mip_level(vs.z, G.footprint, G.L);
        const MipPlace lo = mip_place(G.width, G.height, lv.l0);
        float4 r = mip_sample(lv.l0 ? G.pyramid + lo.off : G.in, vw.z, vw.w, lv.l0, lo);
        if (lv.f != 0.0f) {                                  // (then l0 < L: the level above exists)
            const MipPlace hi = mip_above(lo, lv.l0);
            r = mip_lerp(r, mip_sample(G.pyramid + hi.off, vw.z, vw.w, lv.l0 + 1, hi), lv.f);
        }
        c = make_float4(vw.x * r.x, vw.x * r.y, vw.x * r.z, vw.x * r.w);
    }
    G.out[t] = c;
}

ZD void mip_scatter(float *d, float X, float Y, int l, MipPlace p, float share, float visible, float g) {
    const float inv = mip_exp2_neg(l);
    const MipTaps T = mip_taps(X * inv, Y * inv, p.w, p.h);
    const float ux = 1.0f - T.tx, uy = 1.0f - T.ty;
    atomicAdd(d + 4 * (size_t)T.i00, (((ux * uy) * share) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i01, (((T.tx * uy) * share) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i10, (((ux * T.ty) * share) * visible) * g);
    atomicAdd(d + 4 * (size_t)T.i11, (((T.tx * T.ty) * share) * visible) * g);
}

__global__ __launch_bounds__(256) void k_mip_scatter(MipGatherArgs G) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x, t = id >> 2, c = id & 3u;   // (id < 4 ntexels <= 2^28)
    if (t >= G.ntexels) return;
    const float4 vw = G.view[2 * (size_t)t];
    if (!(vw.x != 0.0f && vw.x == vw.x)) return;
    const float scale = ((const float *)G.view)[8 * (size_t)t + 6];
    const MipLevel lv = mip_level(scale, G.footprint, G.L);
    const MipPlace lo = mip_place(G.width, G.height, lv.l0);
    const float g = ((const float *)G.in)[id];
    // with f == 0 the share is 1 and (w 1) visible g is the very product k_proj_scatter adds
    mip_scatter((lv.l0 ? (float *)(G.d_pyramid + lo.off) : (float *)G.out) + c, vw.z, vw.w, lv.l0, lo, 1.0f - lv.f, vw.x, g);
    if (lv.f != 0.0f) {
        const MipPlace hi = mip_above(lo, lv.l0);
        mip_scatter((float *)(G.d_pyramid + hi.off) + c, vw.z, vw.w, lv.l0 + 1, hi, lv.f, vw.x, g);
    }
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
