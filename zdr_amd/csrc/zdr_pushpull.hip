// zdr_pushpull.hip — push-pull hole filling of an (H, W, 4) texture under an (H, W) weight, and its adjoint (include/zdr.h, zdr_push_pull,
// zdr_push_pull_backward) for gfx950.
//
// Both passes are an up-sweep and a down-sweep over the pyramid of csrc/pushpull.h.  Level 0 is the caller's (w, x, out); the levels >= 1
// sit in the workspace, one float4 per texel (p, overwritten by y; for the adjoint G, overwritten by q) and two floats (a, r).
//   k_pp_push<L0>      forward up-sweep, one thread per COARSE texel: a, p of level l + 1 from the 2 x 2 children
//   k_pp_pull<L0>      forward down-sweep, one thread per FINE texel: y_l = p_l + (1 - a_l) U(y_{l+1}), in place (level 0: into out)
//   k_pp_gather<L0>    adjoint up-sweep, one thread per coarse texel: a, r of level l + 1 and G_{l+1} = U^T((1 - a_l) G_l), a gather over
//                      the 4 x 4 fine texels that U can send to this one
//   k_pp_spread<L0>    adjoint down-sweep, one thread per fine texel: q_l = G_l + r[parent] q[parent], in place (level 0: a_0 q_0 into d_x)
//   k_pp_tail_fwd<L0>, k_pp_tail_bwd<L0>
//                      ONE workgroup: from the first level of at most 32 x 32 texels the rest of the up-sweep, the top and the down-sweep
//                      back to that level, all in LDS (33 KB); L0 = that level is level 0 itself, the whole call is this launch
//   k_pp_top           the top of a pyramid that `levels` cut off below the tail's size: y_L = p_L / a_L
// Texels are numbered row by row in grid.x, 256 to a block: a wave reads 64 consecutive float4 (1 KiB) of a row, or, in the up-sweeps,
// 128 consecutive ones as two 16-byte loads per lane, and 64 or 128 consecutive floats of the 1-channel arrays.  Every store is a plain
// 16-byte or 4-byte store of a texel that this thread alone owns: no atomics, no scratch, the same sum order whatever the grid.
// The level launches and the tail go through the SAME device functions (pp_push, pp_upsample, pp_gather, ...) and the file is compiled
// without contraction, so a level computes the same bits in LDS as in memory.
#include "pushpull.h"

#define PP_BLOCK 256

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// ---------------------------------------------------------------------------------------------------- the operator, value by value
// level 0: a_0 = w clamped to [0, 1], NaN -> 0;  p_0 = a_0 x where a_0 > 0, else 0 (a select: what sits behind weight 0 is never multiplied)
__device__ __forceinline__ float pp_a0(float w) { return w > 0.f ? fminf(w, 1.f) : 0.f; }
__device__ __forceinline__ float4 pp_p0(float a, float4 x) { return a > 0.f ? f4scale(x, a) : f4zero(); }

// a and r of coarse texel (I, J);  fa(i, j) = a of the finer level, 0 outside it
template <class FA>
__device__ __forceinline__ void pp_push_weights(int I, int J, FA fa, float &a, float &r) {
    const int i = 2 * I, j = 2 * J;
    const float a00 = fa(i, j), a01 = fa(i, j + 1), a10 = fa(i + 1, j), a11 = fa(i + 1, j + 1);
    const float S = (a00 + a01) + (a10 + a11);
    a = fminf(S, 1.f);
    r = S > 0.f ? a / S : 0.f;
}

// a, r and p of coarse texel (I, J);  fp(i, j) = p of the finer level, 0 outside it
template <class FA, class FP>
__device__ __forceinline__ void pp_push(int I, int J, FA fa, FP fp, float &a, float &r, float4 &p) {
    pp_push_weights(I, J, fa, a, r);
    const int i = 2 * I, j = 2 * J;
    const float4 P = f4add(f4add(fp(i, j), fp(i, j + 1)), f4add(fp(i + 1, j), fp(i + 1, j + 1)));
    p = f4scale(P, r);
}

__device__ __forceinline__ float4 pp_top(float4 v, float a) {
    return a > 0.f ? make_float4(v.x / a, v.y / a, v.z / a, v.w / a) : f4zero();
}

// the second tap of U for fine index i of an axis whose coarser level has nc entries (the first is i >> 1)
__device__ __forceinline__ int pp_nb(int i, int nc) {
    const int c = i >> 1, nb = (i & 1) ? c + 1 : c - 1;
    return nb < 0 ? 0 : nb > nc - 1 ? nc - 1 : nb;
}

// U(v) at fine texel (i, j): along the row first, then across the two rows;  v(y, x) = the coarser level (hc x wc)
template <class F>
__device__ __forceinline__ float4 pp_upsample(int i, int j, int hc, int wc, F v) {
    const int cy = i >> 1, ny = pp_nb(i, hc), cx = j >> 1, nx = pp_nb(j, wc);
    const float4 rc = f4add(f4scale(v(cy, cx), 0.75f), f4scale(v(cy, nx), 0.25f));
    const float4 rn = f4add(f4scale(v(ny, cx), 0.75f), f4scale(v(ny, nx), 0.25f));
    return f4add(f4scale(rc, 0.75f), f4scale(rn, 0.25f));
}

__device__ __forceinline__ float4 pp_pull(float4 p, float a, float4 u) { return f4add(p, f4scale(u, 1.f - a)); }

// what fine index i sends to coarse index c along one axis: 0.75 if c is its first tap, 0.25 if c is its second, both (1) at a clamped border
__device__ __forceinline__ float pp_ut_weight(int i, int c, int nc) {
    return ((i >> 1) == c ? 0.75f : 0.f) + (pp_nb(i, nc) == c ? 0.25f : 0.f);
}

// U^T(h) at coarse texel (I, J): the fine texels 2I - 1 .. 2I + 2 by 2J - 1 .. 2J + 2 that lie inside the finer level (hf x wf), row sums
// first, rows in order;  h(i, j) = (1 - a) G of the finer level
template <class F>
__device__ __forceinline__ float4 pp_gather(int I, int J, int hf, int wf, int hc, int wc, F h) {
    float4 acc = f4zero();
#pragma unroll
    for (int di = 0; di < 4; di++) {
        const int i = 2 * I - 1 + di;
        if (i < 0 || i >= hf) continue;
        float4 row = f4zero();
#pragma unroll
        for (int dj = 0; dj < 4; dj++) {
            const int j = 2 * J - 1 + dj;
            if (j < 0 || j >= wf) continue;
            row = f4add(row, f4scale(h(i, j), pp_ut_weight(j, J, wc)));
        }
        acc = f4add(acc, f4scale(row, pp_ut_weight(i, I, hc)));
    }
    return acc;
}

__device__ __forceinline__ float4 pp_spread(float4 G, float r, float4 q) { return f4add(G, f4scale(q, r)); }
__device__ __forceinline__ float4 pp_dx(float a, float4 q) { return a > 0.f ? f4scale(q, a) : f4zero(); }

// ---------------------------------------------------------------------------------------------------------------- level launches
// wa: w (L0) or a of the finer level;  pf: x (L0) or p of the finer level
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_push(int wf, int hf, int wc, int hc, const float *__restrict__ wa, const float4 *__restrict__ pf,
                                                      float *__restrict__ ac, float4 *__restrict__ pc) {
    const uint32_t idx = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)wc * (uint32_t)hc) return;
    const int I = (int)(idx / (uint32_t)wc), J = (int)(idx - (uint32_t)I * (uint32_t)wc);
    auto fa = [&](int i, int j) -> float {
        if (i >= hf || j >= wf) return 0.f;
        const float v = wa[(uint32_t)i * (uint32_t)wf + (uint32_t)j];
        return L0 ? pp_a0(v) : v;
    };
    auto fp = [&](int i, int j) -> float4 {
        if (i >= hf || j >= wf) return f4zero();
        const uint32_t t = (uint32_t)i * (uint32_t)wf + (uint32_t)j;
        const float4 v = pf[t];
        return L0 ? pp_p0(pp_a0(wa[t]), v) : v;
    };
    float a, r;
    float4 p;
    pp_push(I, J, fa, fp, a, r, p);
    ac[idx] = a;
    pc[idx] = p;
}

// wa: w (L0) or a of this level;  pf: x (L0) or p of this level, which is dst itself then (each thread reads its texel before it writes it)
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_pull(int wf, int hf, int wc, int hc, const float *__restrict__ wa, const float4 *pf,
                                                      const float4 *__restrict__ yc, float4 *dst) {
    const uint32_t idx = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)wf * (uint32_t)hf) return;
    const int i = (int)(idx / (uint32_t)wf), j = (int)(idx - (uint32_t)i * (uint32_t)wf);
    const float a = L0 ? pp_a0(wa[idx]) : wa[idx];
    const float4 v = pf[idx];
    const float4 u = pp_upsample(i, j, hc, wc, [&](int y, int x) -> float4 { return yc[(uint32_t)y * (uint32_t)wc + (uint32_t)x]; });
    float4 y = pp_pull(L0 ? pp_p0(a, v) : v, a, u);
    if (L0 && a == 1.f) y = v;                                       // the same bits, by selection
    dst[idx] = y;
}

__global__ __launch_bounds__(PP_BLOCK) void k_pp_top(uint32_t n, const float *__restrict__ a, float4 *v) {
    const uint32_t idx = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (idx >= n) return;
    v[idx] = pp_top(v[idx], a[idx]);
}

// wa: w (L0) or a of the finer level;  gf: d_out (L0) or G of the finer level
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_gather(int wf, int hf, int wc, int hc, const float *__restrict__ wa, const float4 *__restrict__ gf,
                                                        float *__restrict__ ac, float *__restrict__ rc, float4 *__restrict__ gc) {
    const uint32_t idx = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)wc * (uint32_t)hc) return;
    const int I = (int)(idx / (uint32_t)wc), J = (int)(idx - (uint32_t)I * (uint32_t)wc);
    auto fa = [&](int i, int j) -> float {
        if (i >= hf || j >= wf) return 0.f;
        const float v = wa[(uint32_t)i * (uint32_t)wf + (uint32_t)j];
        return L0 ? pp_a0(v) : v;
    };
    float a, r;
    pp_push_weights(I, J, fa, a, r);
    ac[idx] = a;
    rc[idx] = r;
    gc[idx] = pp_gather(I, J, hf, wf, hc, wc, [&](int i, int j) -> float4 {
        return f4scale(gf[(uint32_t)i * (uint32_t)wf + (uint32_t)j], 1.f - fa(i, j));
    });
}

// w: level 0 only;  gf: d_out (L0) or G of this level, which is dst itself then
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_spread(int wf, int hf, int wc, const float *__restrict__ w, const float4 *gf,
                                                        const float *__restrict__ rc, const float4 *__restrict__ qc, float4 *dst) {
    const uint32_t idx = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (idx >= (uint32_t)wf * (uint32_t)hf) return;
    const int i = (int)(idx / (uint32_t)wf), j = (int)(idx - (uint32_t)i * (uint32_t)wf);
    const uint32_t par = (uint32_t)(i >> 1) * (uint32_t)wc + (uint32_t)(j >> 1);
    float4 q = pp_spread(gf[idx], rc[par], qc[par]);
    if (L0) q = pp_dx(pp_a0(w[idx]), q);
    dst[idx] = q;
}

// ------------------------------------------------------------------------------------------------------------------ the fused tail
// size and LDS offset of level l above a base level of w0 x h0 (halving and rounding up l times is dividing by 2^l and rounding up)
__device__ __forceinline__ void pp_tail_level(int w0, int h0, int l, int &w, int &h, int &off) {
    off = 0;
    for (int k = 0; k < l; k++) off += ((w0 + (1 << k) - 1) >> k) * ((h0 + (1 << k) - 1) >> k);
    w = (w0 + (1 << l) - 1) >> l;
    h = (h0 + (1 << l) - 1) >> l;
}

// The base level (w0 x h0 <= 32 x 32) and the nlev levels above it.  wa: w (L0) or a of the base level;  pin: x (L0) or p of the base level,
// which is dst itself then;  dst: out (L0) or y of the base level.
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_tail_fwd(int w0, int h0, int nlev, const float *__restrict__ wa, const float4 *pin, float4 *dst) {
    __shared__ float4 V[ZDR_PUSHPULL_TAIL_TEXELS];
    __shared__ float A[ZDR_PUSHPULL_TAIL_TEXELS];
    const int tid = (int)threadIdx.x, n0 = w0 * h0;
    for (int t = tid; t < n0; t += PP_BLOCK) {
        const float a = L0 ? pp_a0(wa[t]) : wa[t];
        const float4 v = pin[t];
        A[t] = a;
        V[t] = L0 ? pp_p0(a, v) : v;
    }
    int wf = w0, hf = h0, off = 0;
    for (int l = 0; l < nlev; l++) {                                 // push: level l -> l + 1
        __syncthreads();
        const int wc = (wf + 1) >> 1, hc = (hf + 1) >> 1, offc = off + wf * hf;
        for (int t = tid; t < wc * hc; t += PP_BLOCK) {
            const int I = t / wc, J = t - I * wc;
            float a, r;
            float4 p;
            pp_push(I, J, [&](int i, int j) -> float { return (i < hf && j < wf) ? A[off + i * wf + j] : 0.f; },
                    [&](int i, int j) -> float4 { return (i < hf && j < wf) ? V[off + i * wf + j] : f4zero(); }, a, r, p);
            A[offc + t] = a;
            V[offc + t] = p;
        }
        off = offc; wf = wc; hf = hc;
    }
    __syncthreads();
    for (int t = tid; t < wf * hf; t += PP_BLOCK) V[off + t] = pp_top(V[off + t], A[off + t]);
    for (int l = nlev - 1; l >= 0; l--) {                            // pull: level l from l + 1
        __syncthreads();
        int wc, hc, offc;
        pp_tail_level(w0, h0, l, wf, hf, off);
        pp_tail_level(w0, h0, l + 1, wc, hc, offc);
        for (int t = tid; t < wf * hf; t += PP_BLOCK) {
            const int i = t / wf, j = t - i * wf;
            const float4 u = pp_upsample(i, j, hc, wc, [&](int y, int x) -> float4 { return V[offc + y * wc + x]; });
            V[off + t] = pp_pull(V[off + t], A[off + t], u);
        }
    }
    __syncthreads();
    for (int t = tid; t < n0; t += PP_BLOCK) {
        float4 y = V[t];
        if (L0 && A[t] == 1.f) y = pin[t];                           // the same bits, by selection
        dst[t] = y;
    }
}

// wa: w (L0) or a of the base level;  gin: d_out (L0) or G of the base level, which is dst itself then;  dst: d_x (L0) or q of the base level
template <bool L0>
__global__ __launch_bounds__(PP_BLOCK) void k_pp_tail_bwd(int w0, int h0, int nlev, const float *__restrict__ wa, const float4 *gin, float4 *dst) {
    __shared__ float4 V[ZDR_PUSHPULL_TAIL_TEXELS];
    __shared__ float A[ZDR_PUSHPULL_TAIL_TEXELS];
    __shared__ float R[ZDR_PUSHPULL_TAIL_TEXELS];
    const int tid = (int)threadIdx.x, n0 = w0 * h0;
    for (int t = tid; t < n0; t += PP_BLOCK) {
        A[t] = L0 ? pp_a0(wa[t]) : wa[t];
        V[t] = gin[t];
    }
    int wf = w0, hf = h0, off = 0;
    for (int l = 0; l < nlev; l++) {                                 // a, r and G of level l + 1
        __syncthreads();
        const int wc = (wf + 1) >> 1, hc = (hf + 1) >> 1, offc = off + wf * hf;
        for (int t = tid; t < wc * hc; t += PP_BLOCK) {
            const int I = t / wc, J = t - I * wc;
            float a, r;
            pp_push_weights(I, J, [&](int i, int j) -> float { return (i < hf && j < wf) ? A[off + i * wf + j] : 0.f; }, a, r);
            A[offc + t] = a;
            R[offc + t] = r;
            V[offc + t] = pp_gather(I, J, hf, wf, hc, wc, [&](int i, int j) -> float4 {
                return f4scale(V[off + i * wf + j], 1.f - A[off + i * wf + j]);
            });
        }
        off = offc; wf = wc; hf = hc;
    }
    __syncthreads();
    for (int t = tid; t < wf * hf; t += PP_BLOCK) V[off + t] = pp_top(V[off + t], A[off + t]);
    for (int l = nlev - 1; l >= 0; l--) {                            // q of level l from its parents
        __syncthreads();
        int wc, hc, offc;
        pp_tail_level(w0, h0, l, wf, hf, off);
        pp_tail_level(w0, h0, l + 1, wc, hc, offc);
        for (int t = tid; t < wf * hf; t += PP_BLOCK) {
            const int i = t / wf, j = t - i * wf, par = offc + (i >> 1) * wc + (j >> 1);
            V[off + t] = pp_spread(V[off + t], R[par], V[par]);
        }
    }
    __syncthreads();
    for (int t = tid; t < n0; t += PP_BLOCK) dst[t] = L0 ? pp_dx(A[t], V[t]) : V[t];
}

// ------------------------------------------------------------------------------------------------------------------------ launcher
static dim3 pp_grid(int w, int h) { return dim3((unsigned)(((size_t)w * (size_t)h + PP_BLOCK - 1) / PP_BLOCK)); }

int zdr_launch_push_pull(const PushPullArgs &A, int backward, hipStream_t st) {
    const PushPullPlan P = zdr_push_pull_plan(A.width, A.height, A.levels);
    char *ws = (char *)A.workspace;
    auto V = [&](int l) { return (float4 *)(ws + P.v_off[l]); };
    auto a_ = [&](int l) { return (float *)(ws + P.a_off[l]); };
    auto r_ = [&](int l) { return (float *)(ws + P.r_off[l]); };
    const dim3 block(PP_BLOCK);
    const bool fused = P.tail <= P.L;
    const int upto = fused ? P.tail : P.L;                           // the level launches go up to this level and come back from it
    for (int l = 0; l < upto; l++) {
        const int wf = P.w[l], hf = P.h[l], wc = P.w[l + 1], hc = P.h[l + 1];
        const dim3 grid = pp_grid(wc, hc);
        if (!backward) {
            if (l == 0) hipLaunchKernelGGL(k_pp_push<true>, grid, block, 0, st, wf, hf, wc, hc, A.weight, A.in, a_(1), V(1));
            else hipLaunchKernelGGL(k_pp_push<false>, grid, block, 0, st, wf, hf, wc, hc, (const float *)a_(l), (const float4 *)V(l), a_(l + 1), V(l + 1));
        } else {
            if (l == 0) hipLaunchKernelGGL(k_pp_gather<true>, grid, block, 0, st, wf, hf, wc, hc, A.weight, A.in, a_(1), r_(1), V(1));
            else hipLaunchKernelGGL(k_pp_gather<false>, grid, block, 0, st, wf, hf, wc, hc, (const float *)a_(l), (const float4 *)V(l), a_(l + 1), r_(l + 1), V(l + 1));
        }
    }
    if (fused) {
        const int T = P.tail, nlev = P.L - T;
        const float *wa = T == 0 ? A.weight : a_(T);
        const float4 *src = T == 0 ? A.in : V(T);
        float4 *dst = T == 0 ? A.out : V(T);
        if (!backward) {
            if (T == 0) hipLaunchKernelGGL(k_pp_tail_fwd<true>, dim3(1), block, 0, st, P.w[T], P.h[T], nlev, wa, src, dst);
            else hipLaunchKernelGGL(k_pp_tail_fwd<false>, dim3(1), block, 0, st, P.w[T], P.h[T], nlev, wa, src, dst);
        } else {
            if (T == 0) hipLaunchKernelGGL(k_pp_tail_bwd<true>, dim3(1), block, 0, st, P.w[T], P.h[T], nlev, wa, src, dst);
            else hipLaunchKernelGGL(k_pp_tail_bwd<false>, dim3(1), block, 0, st, P.w[T], P.h[T], nlev, wa, src, dst);
        }
    } else {
        hipLaunchKernelGGL(k_pp_top, pp_grid(P.w[P.L], P.h[P.L]), block, 0, st, (uint32_t)P.w[P.L] * (uint32_t)P.h[P.L], (const float *)a_(P.L), V(P.L));
    }
    for (int l = upto - 1; l >= 0; l--) {
        const int wf = P.w[l], hf = P.h[l], wc = P.w[l + 1], hc = P.h[l + 1];
        const dim3 grid = pp_grid(wf, hf);
        if (!backward) {
            if (l == 0) hipLaunchKernelGGL(k_pp_pull<true>, grid, block, 0, st, wf, hf, wc, hc, A.weight, A.in, (const float4 *)V(1), A.out);
            else hipLaunchKernelGGL(k_pp_pull<false>, grid, block, 0, st, wf, hf, wc, hc, (const float *)a_(l), (const float4 *)V(l), (const float4 *)V(l + 1), V(l));
        } else {
            if (l == 0) hipLaunchKernelGGL(k_pp_spread<true>, grid, block, 0, st, wf, hf, wc, A.weight, A.in, (const float *)r_(1), (const float4 *)V(1), A.out);
            else hipLaunchKernelGGL(k_pp_spread<false>, grid, block, 0, st, wf, hf, wc, (const float *)nullptr, (const float4 *)V(l), (const float *)r_(l + 1), (const float4 *)V(l + 1), V(l));
        }
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
