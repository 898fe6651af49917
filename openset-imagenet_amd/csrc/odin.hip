// Gradient-based open-set scores on the GPU: the head of ODIN (Liang, Li, Srikant, ICLR 2018) and the closed form of GradNorm for the
// last linear layer (Huang, Geng, Li, NeurIPS 2021). include/osi.h (ABI 29) is the definition; openset_imagenet/odin.py is the user's
// face of it, tests/odin_oracle.py the numpy restatement.
//
//   osi_odin_head         one wave per row, fp64: arg-max (a NaN the largest, the lowest index among equals, across lanes as within
//                         one), maximum, the temperature-scaled exponentials and their two sums - s over the whole row in the order
//                         of osi_logit_scores, r in the same order with the predicted column left out -, then the score and the
//                         seed of the input-only backward. A row of at most 1024 columns (a multiple of 4) stays in registers with
//                         its exponentials between the passes; any other row is read three times.
//   osi_gradnorm_scores   one wave per row, fp64: the L1 norm of the feature row, and sum |C p - 1| over the temperature softmax.
// Which form runs is a function of C alone, and so is the order of every sum; no atomics, no workspace.
#include "osi_common.h"

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_BLOCKS = 1 << 20;

// a before b in the arg-max order of torch.argmax: a NaN is the largest value, the lowest index wins among equals (and among NaNs).
// A lane without a column holds (-Inf, INT_MAX) and loses against every column.
__device__ __forceinline__ bool am_before(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}
__device__ __forceinline__ void am_take(float& bv, int& bi, float v, int i) {
    if (am_before(v, i, bv, bi)) { bv = v; bi = i; }
}
__device__ __forceinline__ int wave_argmax(float bv, int bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        am_take(bv, bi, ov, oi);
    }
    return bi;                                              // a total order over distinct indices: every lane ends with the same pair
}

// QUADS: lane l owns the quads l, l + 64, ... of the row (k_logit_scores of shaping.hip: 16-byte loads where the row is aligned, the
// same elements in the same order either way)
__device__ __forceinline__ void load_quads(const float* __restrict__ lr, int nq, int lane, float4 (&q)[4]) {
    const bool vec = ((uintptr_t)lr & 15) == 0;             // uniform in the wave
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        q[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);     // neutral for the maximum; never summed
        if (i < nq) q[k] = vec ? reinterpret_cast<const float4*>(lr)[i] : make_float4(lr[4 * i], lr[4 * i + 1], lr[4 * i + 2], lr[4 * i + 3]);
    }
}

// e = exp((l - shift) / T): the one expression of both kernels and of every pass
__device__ __forceinline__ double tex(float l, double shift, double T) { return exp(((double)l - shift) / T); }

template <bool QUADS>
__global__ __launch_bounds__(NT) void k_odin_head(const float* __restrict__ logits, int M, int C, double T, float* __restrict__ dlogits,
                                                  long long* __restrict__ pred, float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * NW;
    for (long long row = (long long)blockIdx.x * NW + (threadIdx.x >> 6); row < M; row += waves) {
        const float* __restrict__ lr = logits + (size_t)row * C;
        float* __restrict__ dr = dlogits ? dlogits + (size_t)row * C : nullptr;
        double m = -INFINITY, s = 0.0, r = 0.0;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (QUADS) {
            const int nq = C >> 2;
            float4 q[4];
            double e[4][4];
            load_quads(lr, nq, lane, q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * (lane + 64 * k);
                m = fmax(fmax(fmax(m, (double)q[k].x), fmax((double)q[k].y, (double)q[k].z)), (double)q[k].w);
                if (lane + 64 * k < nq) {
                    am_take(bv, bi, q[k].x, c); am_take(bv, bi, q[k].y, c + 1); am_take(bv, bi, q[k].z, c + 2); am_take(bv, bi, q[k].w, c + 3);
                }
            }
            m = wave_fmax(m);                               // skips a NaN: the sums find it again
            const int y = wave_argmax(bv, bi);
            const double shift = isfinite(m) ? m : 0.0;     // an infinite maximum is not subtracted
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = 4 * (lane + 64 * k);
                e[k][0] = e[k][1] = e[k][2] = e[k][3] = 0.0;
                if (lane + 64 * k < nq) {
                    e[k][0] = tex(q[k].x, shift, T); e[k][1] = tex(q[k].y, shift, T); e[k][2] = tex(q[k].z, shift, T); e[k][3] = tex(q[k].w, shift, T);
                    s += e[k][0] + e[k][1] + e[k][2] + e[k][3];
                    r += (c == y ? 0.0 : e[k][0]) + (c + 1 == y ? 0.0 : e[k][1]) + (c + 2 == y ? 0.0 : e[k][2]) + (c + 3 == y ? 0.0 : e[k][3]);
                }
            }
            s = wave_sum(s);
            r = wave_sum(r);
            if (dr) {
                const double gy = -r / s;
                const bool vec = ((uintptr_t)dr & 15) == 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = lane + 64 * k, c = 4 * i;
                    if (i < nq) {
                        const float4 g = make_float4((float)(c == y ? gy : e[k][0] / s), (float)(c + 1 == y ? gy : e[k][1] / s),
                                                     (float)(c + 2 == y ? gy : e[k][2] / s), (float)(c + 3 == y ? gy : e[k][3] / s));
                        if (vec) reinterpret_cast<float4*>(dr)[i] = g;
                        else { dr[c] = g.x; dr[c + 1] = g.y; dr[c + 2] = g.z; dr[c + 3] = g.w; }
                    }
                }
            }
            if (lane == 0) {
                if (pred) pred[row] = (long long)y;
                score[row] = (float)(exp((m - shift) / T) / s);
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float v = lr[c];
                m = fmax(m, (double)v);
                am_take(bv, bi, v, c);
            }
            m = wave_fmax(m);
            const int y = wave_argmax(bv, bi);
            const double shift = isfinite(m) ? m : 0.0;
            for (int c = lane; c < C; c += 64) {
                const double ec = tex(lr[c], shift, T);
                s += ec;
                r += c == y ? 0.0 : ec;
            }
            s = wave_sum(s);
            r = wave_sum(r);
            if (dr) {
                const double gy = -r / s;
                for (int c = lane; c < C; c += 64) dr[c] = (float)(c == y ? gy : tex(lr[c], shift, T) / s);
            }
            if (lane == 0) {
                if (pred) pred[row] = (long long)y;
                score[row] = (float)(exp((m - shift) / T) / s);
            }
        }
    }
}

template <bool QUADS>
__global__ __launch_bounds__(NT) void k_gradnorm(const float* __restrict__ features, const float* __restrict__ logits, int M, int F, int C,
                                                 double T, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * NW;
    for (long long row = (long long)blockIdx.x * NW + (threadIdx.x >> 6); row < M; row += waves) {
        const float* __restrict__ lr = logits + (size_t)row * C;
        const float* __restrict__ fr = features + (size_t)row * F;
        // the L1 norm: quads l, l + 64, ... where F is a multiple of 4, columns l, l + 64, ... otherwise
        double l1 = 0.0;
        if (F % 4 == 0) {
            const bool vec = ((uintptr_t)fr & 15) == 0;
            for (int i = lane; i < (F >> 2); i += 64) {
                const float4 v = vec ? reinterpret_cast<const float4*>(fr)[i] : make_float4(fr[4 * i], fr[4 * i + 1], fr[4 * i + 2], fr[4 * i + 3]);
                l1 += fabs((double)v.x) + fabs((double)v.y) + fabs((double)v.z) + fabs((double)v.w);
            }
        } else {
            for (int c = lane; c < F; c += 64) l1 += fabs((double)fr[c]);
        }
        l1 = wave_sum(l1);
        double m = -INFINITY, s = 0.0, u = 0.0;
        const double n = (double)C;
        if (QUADS) {
            const int nq = C >> 2;
            float4 q[4];
            double e[4][4];
            load_quads(lr, nq, lane, q);
#pragma unroll
            for (int k = 0; k < 4; ++k) m = fmax(fmax(fmax(m, (double)q[k].x), fmax((double)q[k].y, (double)q[k].z)), (double)q[k].w);
            m = wave_fmax(m);
            const double shift = isfinite(m) ? m : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                e[k][0] = e[k][1] = e[k][2] = e[k][3] = 0.0;
                if (lane + 64 * k < nq) {
                    e[k][0] = tex(q[k].x, shift, T); e[k][1] = tex(q[k].y, shift, T); e[k][2] = tex(q[k].z, shift, T); e[k][3] = tex(q[k].w, shift, T);
                    s += e[k][0] + e[k][1] + e[k][2] + e[k][3];
                }
            }
            s = wave_sum(s);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k < nq)
                    u += fabs(n * (e[k][0] / s) - 1.0) + fabs(n * (e[k][1] / s) - 1.0) + fabs(n * (e[k][2] / s) - 1.0) + fabs(n * (e[k][3] / s) - 1.0);
        } else {
            for (int c = lane; c < C; c += 64) m = fmax(m, (double)lr[c]);
            m = wave_fmax(m);
            const double shift = isfinite(m) ? m : 0.0;
            for (int c = lane; c < C; c += 64) s += tex(lr[c], shift, T);
            s = wave_sum(s);
            for (int c = lane; c < C; c += 64) u += fabs(n * (tex(lr[c], shift, T) / s) - 1.0);
        }
        u = wave_sum(u);                                    // a NaN in either row is a NaN here or in l1
        if (lane == 0) out[row] = (float)(l1 * u / T);
    }
}

static unsigned grid_for(long long units) { return (unsigned)(units < MAX_BLOCKS ? (units > 0 ? units : 1) : MAX_BLOCKS); }
static bool good_temperature(float T) { return isfinite(T) && T > 0.0f; }

}  // namespace

extern "C" {

int osi_odin_head(const float* logits, int M, int C, float T, float* dlogits, long long* pred, float* score, osi_stream_t stream) {
    OSI_REQUIRE(logits && score);
    OSI_REQUIRE(M > 0 && C > 0);
    OSI_REQUIRE(good_temperature(T));
    OSI_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)score & 3) == 0 && ((uintptr_t)dlogits & 3) == 0 && ((uintptr_t)pred & 7) == 0);
    const size_t bytes = (size_t)M * C * sizeof(float);
    OSI_REQUIRE(!dlogits || (uintptr_t)dlogits + bytes <= (uintptr_t)logits || (uintptr_t)logits + bytes <= (uintptr_t)dlogits);   // no aliasing
    const unsigned grid = grid_for(((long long)M + NW - 1) / NW);
    if (C % 4 == 0 && C <= 1024)
        hipLaunchKernelGGL(k_odin_head<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, logits, M, C, (double)T, dlogits, pred, score);
    else
        hipLaunchKernelGGL(k_odin_head<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, logits, M, C, (double)T, dlogits, pred, score);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_gradnorm_scores(const float* features, const float* logits, int M, int F, int C, float T, float* out, osi_stream_t stream) {
    OSI_REQUIRE(features && logits && out);
    OSI_REQUIRE(M > 0 && F > 0 && C > 0);
    OSI_REQUIRE(good_temperature(T));
    OSI_REQUIRE(((uintptr_t)features & 3) == 0 && ((uintptr_t)logits & 3) == 0 && ((uintptr_t)out & 3) == 0);
    const unsigned grid = grid_for(((long long)M + NW - 1) / NW);
    if (C % 4 == 0 && C <= 1024)
        hipLaunchKernelGGL(k_gradnorm<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, features, logits, M, F, C, (double)T, out);
    else
        hipLaunchKernelGGL(k_gradnorm<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, features, logits, M, F, C, (double)T, out);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
