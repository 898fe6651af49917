// OpenMax (Bendale & Boult, CVPR 2016) on the GPU: class means of the correctly classified training rows, a Weibull fit to the largest
// distances of every class, and the recalibration of test logits by the probability of lying in that tail. include/osi.h (ABI 21) is
// the definition; openset_imagenet/openmax.py is the user's face of it.
//
// Five steps, every one bit-reproducible (no floating-point atomics; integer counts only where blocks meet):
//   class means   a row pass marks the correct rows (first maximum == label, no NaN); one workgroup per class then walks the marks in
//                 row order, compacts each chunk's hits with a ballot prefix and adds their features in fp64, one thread per column.
//   distances     one thread per (row, class) pair (tiles of 32 rows x 64 classes staged in LDS), or per row against the class it
//                 names: fp64 sums in index order.
//   tail fit      a row pass turns the eligible distances into order-preserving 32-bit keys; one workgroup per class selects the T
//                 largest with a four-pass radix select over the key bytes, sorts them in LDS (bitonic), and solves the Weibull
//                 likelihood equation by Newton steps kept inside a bracket. The sums run over the SORTED tail in a fixed tree, so the
//                 fit depends on the multiset only. Select, sort and solver live in tail_fit.h, shared with evm.hip.
//   w-scores      element-wise Weibull CDF in fp64.
//   recalibrate   one wave per row: stable descending ranks by counting, the unknown activation, a softmax over C + 1 in fp64.
#include "osi_common.h"
#include "tail_fit.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_BLOCKS = 2048;            // grid cap of the grid-stride passes
constexpr int RECAL_MAX_C = 2048;           // row ranking in LDS: 4 rows x C x (fp32 logit + 16-bit rank) = 48 KB at the cap

inline int stride_blocks(long long n) {
    const long long b = (n + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

using osi_tail::fkey;

// ----------------------------------------------------------------------------------------------------------- class means
// mark[i] = the class row i is correct for, -1 otherwise
__global__ __launch_bounds__(NT) void k_om_rows(const float* __restrict__ logits, const long long* __restrict__ gt, int N, int C,
                                               unsigned char* __restrict__ correct, int* __restrict__ mark) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < N; i += (long long)gridDim.x * NT) {
        const float* r = logits + (size_t)i * C;
        float best = r[0];
        int arg = 0;
        bool nan = best != best;
        for (int c = 1; c < C; ++c) {
            const float v = r[c];
            nan |= v != v;
            if (v > best) { best = v; arg = c; }            // strict: the lowest index wins a tie
        }
        const long long y = gt[i];
        const bool ok = !nan && y >= 0 && y < C && arg == (int)y;
        correct[i] = ok ? 1 : 0;
        mark[i] = ok ? (int)y : -1;
    }
}

// One workgroup per class; thread t owns feature column j0 + t. Rows are walked in chunks of NT: the hits of a chunk are compacted in
// row order (ballot prefix inside the wave, wave counts in order), then every column adds them one after the other.
__global__ __launch_bounds__(NT) void k_om_means(const float* __restrict__ features, const int* __restrict__ mark, int N, int F,
                                                float* __restrict__ mav, long long* __restrict__ count) {
    __shared__ int list[NT];
    __shared__ int wcnt[NW];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j0 = 0; j0 < F; j0 += NT) {
        const int j = j0 + threadIdx.x;
        const bool jin = j < F;
        double s = 0.0;
        long long n = 0;
        for (long long r0 = 0; r0 < N; r0 += NT) {
            const long long i = r0 + threadIdx.x;
            const bool hit = i < N && mark[i] == c;
            const unsigned long long m = __ballot(hit);
            if (lane == 0) wcnt[wave] = __popcll(m);
            __syncthreads();
            int off = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                off += w < wave ? wcnt[w] : 0;
                tot += wcnt[w];
            }
            if (hit) list[off + __popcll(m & ((1ull << lane) - 1ull))] = threadIdx.x;
            __syncthreads();
            if (jin) {
                const float* base = features + (size_t)r0 * F + j;
#pragma unroll 4
                for (int k = 0; k < tot; ++k) s += (double)base[(size_t)list[k] * F];
            }
            n += tot;
            __syncthreads();                                // list and wcnt are rewritten by the next chunk
        }
        if (jin) mav[(size_t)c * F + j] = n ? (float)(s / (double)n) : 0.f;
        if (j0 == 0 && threadIdx.x == 0) count[c] = n;
    }
}

// ------------------------------------------------------------------------------------------------------------- distances
__device__ __forceinline__ float om_distance(const float* __restrict__ f, const float* __restrict__ m, int F, int metric) {
    double out;
    if (metric == OSI_OPENMAX_EUCLIDEAN) {
        double s = 0.0;
        for (int j = 0; j < F; ++j) {
            const double d = (double)f[j] - (double)m[j];
            s = __dadd_rn(s, __dmul_rn(d, d));              // the product is rounded before the add: no contraction
        }
        out = __dsqrt_rn(s);
    } else {
        double dot = 0.0, ff = 0.0, mm = 0.0;
        for (int j = 0; j < F; ++j) {
            const double a = (double)f[j], b = (double)m[j];
            dot = __dadd_rn(dot, __dmul_rn(a, b));
            ff = __dadd_rn(ff, __dmul_rn(a, a));
            mm = __dadd_rn(mm, __dmul_rn(b, b));
        }
        out = 1.0 - dot / __dsqrt_rn(__dmul_rn(ff, mm));   // 0 / 0 = NaN
    }
    return (float)out;
}

// row i against the class it names
__global__ __launch_bounds__(NT) void k_om_dist_own(const float* __restrict__ features, const float* __restrict__ mav,
                                                   const long long* __restrict__ cls, int N, int C, int F, int metric,
                                                   float* __restrict__ dist) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < N; i += (long long)gridDim.x * NT) {
        const long long c = cls[i];
        dist[i] = (c < 0 || c >= C) ? NAN : om_distance(features + (size_t)i * F, mav + (size_t)c * F, F, metric);
    }
}

// Every row against every class: a workgroup owns DT_ROWS rows x DT_C classes and walks F in chunks of DT_J columns staged in LDS as
// fp64. Lane l of every wave owns class c0 + l (its mean's column sits in its own LDS row, read without bank conflicts thanks to the
// padding), wave w the rows w, w + 4, ... (one broadcast read per row). Every pair still adds its terms in index order in one thread:
// the bits are those of om_distance.
constexpr int DT_C = 64, DT_R = 8, DT_ROWS = NW * DT_R, DT_J = 32;

__global__ __launch_bounds__(NT) void k_om_dist_all(const float* __restrict__ features, const float* __restrict__ mav, int N, int C,
                                                   int F, int metric, float* __restrict__ dist) {
    __shared__ double sm[DT_C][DT_J + 1];
    __shared__ double sf[DT_ROWS][DT_J];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const long long row0 = (long long)blockIdx.x * DT_ROWS;
    const int c0 = blockIdx.y * DT_C;
    double acc[DT_R], ff[DT_R], mm = 0.0;
#pragma unroll
    for (int k = 0; k < DT_R; ++k) acc[k] = ff[k] = 0.0;
    for (int j0 = 0; j0 < F; j0 += DT_J) {
        const int jn = F - j0 < DT_J ? F - j0 : DT_J;
        __syncthreads();                                    // the previous chunk has been consumed
        for (int e = threadIdx.x; e < DT_C * DT_J; e += NT) {
            const int c = e / DT_J, j = e % DT_J;
            sm[c][j] = (c0 + c < C && j < jn) ? (double)mav[(size_t)(c0 + c) * F + j0 + j] : 0.0;
        }
        for (int e = threadIdx.x; e < DT_ROWS * DT_J; e += NT) {
            const int r = e / DT_J, j = e % DT_J;
            sf[r][j] = (row0 + r < N && j < jn) ? (double)features[(size_t)(row0 + r) * F + j0 + j] : 0.0;
        }
        __syncthreads();
        if (metric == OSI_OPENMAX_EUCLIDEAN) {
            for (int j = 0; j < jn; ++j) {
                const double m = sm[cl][j];
#pragma unroll
                for (int k = 0; k < DT_R; ++k) {
                    const double d = sf[rg + NW * k][j] - m;
                    acc[k] = __dadd_rn(acc[k], __dmul_rn(d, d));
                }
            }
        } else {
            for (int j = 0; j < jn; ++j) {
                const double m = sm[cl][j];
                mm = __dadd_rn(mm, __dmul_rn(m, m));
#pragma unroll
                for (int k = 0; k < DT_R; ++k) {
                    const double f = sf[rg + NW * k][j];
                    acc[k] = __dadd_rn(acc[k], __dmul_rn(f, m));
                    ff[k] = __dadd_rn(ff[k], __dmul_rn(f, f));
                }
            }
        }
    }
    if (c0 + cl < C) {
#pragma unroll
        for (int k = 0; k < DT_R; ++k) {
            const long long row = row0 + rg + NW * k;
            if (row < N) {
                const double out = metric == OSI_OPENMAX_EUCLIDEAN ? __dsqrt_rn(acc[k])
                                                                   : 1.0 - acc[k] / __dsqrt_rn(__dmul_rn(ff[k], mm));
                dist[(size_t)row * C + c0 + cl] = (float)out;
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------- tail fit
// mark[i] = c for an eligible row of class c with a finite distance (key[i] = its key), -2 - c for an eligible row whose distance
// is not finite, -1 for every other row
__global__ __launch_bounds__(NT) void k_om_keys(const float* __restrict__ dist, const long long* __restrict__ gt,
                                               const unsigned char* __restrict__ correct, int N, int C, unsigned* __restrict__ key,
                                               int* __restrict__ mark) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < N; i += (long long)gridDim.x * NT) {
        const long long y = gt[i];
        float d = dist[i];
        int mk = -1;
        unsigned k = 0;
        if (correct[i] && y >= 0 && y < C) {
            if (d - d == 0.f) {                             // finite
                if (d == 0.f) d = 0.f;                      // -0 and +0 are one value
                mk = (int)y;
                k = fkey(d);
            } else {
                mk = -2 - (int)y;
            }
        }
        mark[i] = mk;
        key[i] = k;
    }
}

// One workgroup per class; the select, the sort and the solver are tail_fit.h's, over the rows the key pass marked for the class.
__global__ __launch_bounds__(NT) void k_om_fit(const unsigned* __restrict__ key, const int* __restrict__ mark, int N, int T,
                                              double* __restrict__ shape, double* __restrict__ scale, double* __restrict__ shift,
                                              unsigned char* __restrict__ fitted, long long* __restrict__ tail_count,
                                              long long* __restrict__ flags2) {
    __shared__ osi_tail::Shared sm;
    const int c = blockIdx.x;
    const osi_tail::Result r = osi_tail::tail_fit(sm, N, T, [&](long long i, unsigned& k) {
        const int mk = mark[i];
        if (mk == c) { k = key[i]; return 1; }
        return mk == -2 - c ? 2 : 0;
    });
    if (threadIdx.x == 0) {
        shape[c] = r.shape;
        scale[c] = r.scale;
        shift[c] = r.shift;
        fitted[c] = r.fit ? 1 : 0;
        tail_count[c] = r.K;
        if (r.bad) atomicAdd((unsigned long long*)&flags2[0], (unsigned long long)r.bad);     // integer atomics: order-free
        if (!r.fit) atomicAdd((unsigned long long*)&flags2[1], 1ull);
    }
}

// -------------------------------------------------------------------------------------------------------------- w-scores
__global__ __launch_bounds__(NT) void k_om_wscores(const float* __restrict__ dist, unsigned long long total, int C,
                                                  const double* __restrict__ shape, const double* __restrict__ scale,
                                                  const double* __restrict__ shift, const unsigned char* __restrict__ fitted,
                                                  float* __restrict__ w) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * NT + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * NT) {
        const int c = (int)(t % (unsigned)C);
        const double d = (double)dist[t];
        double out = 0.0;
        if (d != d) {
            out = NAN;
        } else if (fitted[c]) {
            const double z = d - shift[c] + 1.0;
            if (z > 0.0) out = 1.0 - exp(-pow(z / scale[c], shape[c]));
        }
        w[t] = (float)out;
    }
}

// ----------------------------------------------------------------------------------------------------------- recalibrate
// One wave per row, NW rows per workgroup. Lane l owns the columns l, l + 64, ... in every pass, so only the logits are shared.
__global__ __launch_bounds__(NT) void k_om_recal(const float* __restrict__ logits, const float* __restrict__ w, int N, int C, int a,
                                                float* __restrict__ probs) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* v = (float*)smem + (size_t)wave * C;
    unsigned short* rk = (unsigned short*)((float*)smem + (size_t)NW * C) + (size_t)wave * C;
    for (long long row0 = (long long)blockIdx.x * NW; row0 < N; row0 += (long long)gridDim.x * NW) {   // uniform trip count
        const long long row = row0 + wave;
        const bool in = row < N;
        int nan = 0;
        if (in)
            for (int c = lane; c < C; c += 64) {
                const float x = logits[(size_t)row * C + c];
                nan |= x != x;
                v[c] = x;
            }
        nan = __any(nan);
        __syncthreads();
        if (in) {
            float* out = probs + (size_t)row * (C + 1);
            const float* wr = w + (size_t)row * C;
            if (nan) {
                for (int c = lane; c <= C; c += 64) out[c] = NAN;
            } else {
                double unk = 0.0, mx = -INFINITY;
                for (int c = lane; c < C; c += 64) {
                    const float vc = v[c];
                    int r = 0;
                    for (int c2 = 0; c2 < C; ++c2) {
                        const float v2 = v[c2];
                        r += (v2 > vc || (v2 == vc && c2 < c)) ? 1 : 0;
                    }
                    rk[c] = (unsigned short)r;
                    const double om = r < a ? 1.0 - (double)wr[c] * (double)(a - r) / (double)a : 1.0;
                    unk += (double)vc * (1.0 - om);
                    mx = fmax(mx, (double)vc * om);
                }
                unk = wave_sum(unk);
                mx = fmax(wave_fmax(mx), unk);
                double s = 0.0;
                for (int c = lane; c < C; c += 64) {
                    const int r = rk[c];
                    const double om = r < a ? 1.0 - (double)wr[c] * (double)(a - r) / (double)a : 1.0;
                    s += exp((double)v[c] * om - mx);
                }
                const double eu = exp(unk - mx);
                s = wave_sum(s) + eu;
                for (int c = lane; c < C; c += 64) {
                    const int r = rk[c];
                    const double om = r < a ? 1.0 - (double)wr[c] * (double)(a - r) / (double)a : 1.0;
                    out[c] = (float)(exp((double)v[c] * om - mx) / s);
                }
                if (lane == 0) out[C] = (float)(eu / s);
            }
        }
        __syncthreads();                                    // v is reloaded by the next round
    }
}

inline size_t om_ws_bytes(int N) { return (size_t)N * (sizeof(unsigned) + sizeof(int)) + 64; }

}  // namespace

extern "C" {

size_t osi_openmax_workspace(int N, int C, int F) { return (N > 0 && C > 0 && F > 0) ? om_ws_bytes(N) : 0; }

int osi_openmax_class_means(const float* features, const float* logits, const long long* gt, int N, int C, int F, float* mav,
                            long long* count, unsigned char* correct, void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(features && logits && gt && mav && count && correct && ws);
    OSI_REQUIRE(N > 0 && N <= INT_MAX - NT && C > 0 && F > 0);
    OSI_REQUIRE(ws_bytes >= om_ws_bytes(N) && ((uintptr_t)ws & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    int* mark = (int*)ws;
    hipLaunchKernelGGL(k_om_rows, dim3(stride_blocks(N)), dim3(NT), 0, st, logits, gt, N, C, correct, mark);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_om_means, dim3(C), dim3(NT), 0, st, features, (const int*)mark, N, F, mav, count);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_openmax_distances(const float* features, const float* mav, const long long* cls, int N, int C, int F, int metric, float* dist,
                          osi_stream_t stream) {
    OSI_REQUIRE(features && mav && dist);
    OSI_REQUIRE(N > 0 && N <= INT_MAX - NT && C > 0 && F > 0);
    OSI_REQUIRE(metric == OSI_OPENMAX_EUCLIDEAN || metric == OSI_OPENMAX_COSINE);
    hipStream_t st = (hipStream_t)stream;
    if (cls) {
        hipLaunchKernelGGL(k_om_dist_own, dim3(stride_blocks(N)), dim3(NT), 0, st, features, mav, cls, N, C, F, metric, dist);
    } else {
        OSI_REQUIRE(osi_cdiv(C, DT_C) <= 65535);
        hipLaunchKernelGGL(k_om_dist_all, dim3(osi_cdiv(N, DT_ROWS), osi_cdiv(C, DT_C)), dim3(NT), 0, st, features, mav, N, C, F, metric,
                           dist);
    }
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_openmax_fit_tails(const float* dist, const long long* gt, const unsigned char* correct, int N, int C, int T, double* shape,
                          double* scale, double* shift, unsigned char* fitted, long long* tail_count, long long* flags2, void* ws,
                          size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(dist && gt && correct && shape && scale && shift && fitted && tail_count && flags2 && ws);
    OSI_REQUIRE(N > 0 && N <= INT_MAX - NT && C > 0);
    OSI_REQUIRE(T >= 2 && T <= OSI_OPENMAX_MAX_TAIL);
    OSI_REQUIRE(ws_bytes >= om_ws_bytes(N) && ((uintptr_t)ws & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flags2, 0, 2 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    int* mark = (int*)ws;
    unsigned* key = (unsigned*)ws + N;
    hipLaunchKernelGGL(k_om_keys, dim3(stride_blocks(N)), dim3(NT), 0, st, dist, gt, correct, N, C, key, mark);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_om_fit, dim3(C), dim3(NT), 0, st, (const unsigned*)key, (const int*)mark, N, T, shape, scale, shift, fitted,
                       tail_count, flags2);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_openmax_wscores(const float* dist, int N, int C, const double* shape, const double* scale, const double* shift,
                        const unsigned char* fitted, float* w, osi_stream_t stream) {
    OSI_REQUIRE(dist && shape && scale && shift && fitted && w);
    OSI_REQUIRE(N > 0 && N <= INT_MAX - NT && C > 0);
    const unsigned long long total = (unsigned long long)N * (unsigned long long)C;
    hipLaunchKernelGGL(k_om_wscores, dim3(stride_blocks((long long)total)), dim3(NT), 0, (hipStream_t)stream, dist, total, C, shape, scale,
                       shift, fitted, w);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_openmax_recalibrate(const float* logits, const float* w, int N, int C, int alpha, float* probs, osi_stream_t stream) {
    OSI_REQUIRE(logits && w && probs);
    OSI_REQUIRE(N > 0 && N <= INT_MAX - NT && C > 0 && C <= RECAL_MAX_C && alpha >= 1);
    const int a = alpha < C ? alpha : C;
    const long long b = ((long long)N + NW - 1) / NW;
    const int blocks = (int)(b > 8 * MAX_BLOCKS ? 8 * MAX_BLOCKS : b);
    const size_t lds = (size_t)NW * C * (sizeof(float) + sizeof(unsigned short));
    hipLaunchKernelGGL(k_om_recal, dim3(blocks), dim3(NT), lds, (hipStream_t)stream, logits, w, N, C, a, probs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
