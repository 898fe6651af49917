// The Extreme Value Machine (Rudd, Jain, Scheirer, Boult, TPAMI 2018) on the GPU: all-pairs distances between feature rows, one
// Weibull fit per training row to its nearest negatives, the greedy set cover that keeps a class's extreme vectors, and the class
// scores of test rows. include/osi.h (ABI 22) is the definition; openset_imagenet/evm.py is the user's face of it.
//
// Five kernels, every one bit-reproducible (no floating-point atomics):
//   norms         one thread per row: the squared norm in fp64, index order.
//   pairwise      A * B^T on v_mfma_f32_32x32x2_f32. A workgroup owns 128 x 128 outputs and walks K in steps of 32 staged in LDS; its
//                 four waves hold 64 x 64 each (2 x 2 MFMA tiles). Both operands are K-contiguous, so a lane reads four consecutive k
//                 of its row with one 16-byte LDS read and feeds four MFMAs; the K order that results is fixed. Global reads are
//                 buffer loads whose range check zero-fills the ragged row edges, and past F the offset is the out-of-bounds sentinel.
//                 The epilogue turns the dot product into the distance in fp64 from the two norm vectors; 32 lanes store 128
//                 consecutive bytes of one output row.
//   fit rows      one workgroup per row: tail_fit.h over y = -(multiplier * d) of the row's negatives.
//   set cover     a bit matrix "row i covers row j" built with wave ballots, then ONE workgroup picks greedily: every thread owns the
//                 rows i = t, t + 1024, ... and keeps their uncovered counts up to date from the words a pick changed.
//   probs         one thread per (query, class): the maximum inclusion probability over the class's extreme vectors.
#include "conv_common.h"
#include "tail_fit.h"

#include <limits.h>
#include <math.h>

namespace {

using namespace osi_conv;

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_BLOCKS = 2048;            // grid cap of the grid-stride passes
constexpr long long DESC_LIMIT = 1ll << 31; // 32-bit buffer descriptors (conv_common.h)

inline int stride_blocks(long long n) {
    const long long b = (n + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

// ----------------------------------------------------------------------------------------------------------------- norms
// rows 0 .. R-1 are a's, rows R .. R+N-1 are b's; out[R + N]
__global__ __launch_bounds__(NT) void k_evm_norms(const float* __restrict__ a, int R, const float* __restrict__ b, int N, int F,
                                                 double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < (long long)R + N; i += (long long)gridDim.x * NT) {
        const float* r = i < R ? a + (size_t)i * F : b + (size_t)(i - R) * F;
        double s = 0.0;
        for (int j = 0; j < F; ++j) {
            const double v = (double)r[j];
            s = __dadd_rn(s, __dmul_rn(v, v));
        }
        out[i] = s;
    }
}

// -------------------------------------------------------------------------------------------------------------- pairwise
constexpr int PB = 128;                     // outputs per workgroup along each of R and N
constexpr int PK = 32;                      // K step
constexpr int PLD = PK + 4;                 // LDS row stride in floats: 16-byte aligned rows, 16 consecutive rows hit 16 bank groups

__device__ __forceinline__ float evm_distance(float dot, double naa, double nbb, int metric) {
    if (metric == OSI_EVM_COSINE) return (float)(1.0 - (double)dot / __dsqrt_rn(__dmul_rn(naa, nbb)));     // 0 / 0 = NaN
    const double t = __dadd_rn(__dadd_rn(naa, nbb), -2.0 * (double)dot);
    return (float)__dsqrt_rn(t < 0.0 ? 0.0 : t);            // a NaN passes the clamp
}

// One 128 x 32 operand tile: thread t owns the four k of column group t & 7 in the rows (t >> 3) + 32 i.
template <bool VEC>
__device__ __forceinline__ void evm_load_tile(__amdgpu_buffer_rsrc_t rs, int row0, int rows, int F, int k0, f32x4 (&v)[4]) {
    const int kq = k0 + 4 * (threadIdx.x & 7);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = row0 + (threadIdx.x >> 3) + 32 * i;
        const uint32_t base = (uint32_t)row * (uint32_t)F * 4u + (uint32_t)kq * 4u;       // < 2^31 for row < rows (host check)
        if (VEC) {
            v[i] = bld4(rs, (row < rows && kq < F) ? base : OOB, 0);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[i][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (row < rows && kq + e < F) ? base + 4u * e : OOB, 0, 0));
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void k_evm_pairwise(const float* __restrict__ a, int R, const float* __restrict__ b, int N, int F,
                                                    int metric, const double* __restrict__ naa, const double* __restrict__ nbb,
                                                    float* __restrict__ dist) {
    __shared__ __align__(16) float sA[PB * PLD];
    __shared__ __align__(16) float sB[PB * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 31, lh = lane >> 5;
    const int r0 = blockIdx.y * PB, n0 = blockIdx.x * PB;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(a, R * F * 4), rb = make_rsrc(b, N * F * 4);

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    f32x4 va[4], vb[4];
    evm_load_tile<VEC>(ra, r0, R, F, 0, va);
    evm_load_tile<VEC>(rb, n0, N, F, 0, vb);
    const int st_off = (tid >> 3) * PLD + 4 * (tid & 7);
    for (int k0 = 0; k0 < F; k0 += PK) {
        __syncthreads();                                    // the previous step's readers are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(&sA[st_off + 32 * i * PLD]) = va[i];
            *reinterpret_cast<f32x4*>(&sB[st_off + 32 * i * PLD]) = vb[i];
        }
        __syncthreads();
        if (k0 + PK < F) {                                  // the next step's operands travel while this one multiplies
            evm_load_tile<VEC>(ra, r0, R, F, k0 + PK, va);
            evm_load_tile<VEC>(rb, n0, N, F, k0 + PK, vb);
        }
#pragma unroll
        for (int q = 0; q < PK / 8; ++q) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = *reinterpret_cast<const f32x4*>(&sA[(wm * 64 + t * 32 + lr) * PLD + 8 * q + 4 * lh]);
                fb[t] = *reinterpret_cast<const f32x4*>(&sB[(wn * 64 + t * 32 + lr) * PLD + 8 * q + 4 * lh]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)                     // MFMA step (q, e) adds k = k0 + 8 q + e, then k0 + 8 q + 4 + e
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[mi][e], fb[ni][e], acc[mi][ni], 0, 0, 0);
        }
    }

    // accumulator register r of lane: output row acc_row(r, lane) of the a tile, column lane & 31 of the b tile
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = n0 + wn * 64 + ni * 32 + lr;
        if (col >= N) continue;
        const double nb = nbb[col];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = r0 + wm * 64 + mi * 32 + acc_row(r, lane);
                if (row < R) dist[(size_t)row * N + col] = evm_distance(acc[mi][ni][r], naa[row], nb, metric);
            }
    }
}

// -------------------------------------------------------------------------------------------------------------- fit rows
__global__ __launch_bounds__(NT) void k_evm_fit(const float* __restrict__ dist, int N, long long ld, const long long* __restrict__ gt,
                                               long long cls, int T, float multiplier, double* __restrict__ shape,
                                               double* __restrict__ scale, double* __restrict__ shift, unsigned char* __restrict__ fitted,
                                               long long* __restrict__ tail_count, long long* __restrict__ flags2) {
    __shared__ osi_tail::Shared sm;
    const int r = blockIdx.x;
    const float* drow = dist + (size_t)r * (size_t)ld;
    const osi_tail::Result res = osi_tail::tail_fit(sm, N, T, [&](long long j, unsigned& k) {
        if (gt[j] == cls) return 0;
        float y = -__fmul_rn(multiplier, drow[j]);
        if (!(y - y == 0.f)) return 2;                      // not finite
        if (y == 0.f) y = 0.f;                              // -0 and +0 are one value
        k = osi_tail::fkey(y);
        return 1;
    });
    if (threadIdx.x == 0) {
        shape[r] = res.shape;
        scale[r] = res.scale;
        shift[r] = res.shift;
        fitted[r] = res.fit ? 1 : 0;
        tail_count[r] = res.K;
        if (res.bad) atomicAdd((unsigned long long*)&flags2[0], (unsigned long long)res.bad);  // integer atomics: order-free
        if (!res.fit) atomicAdd((unsigned long long*)&flags2[1], 1ull);
    }
}

// ------------------------------------------------------------------------------------------------- inclusion probability
__device__ __forceinline__ float evm_psi(float d, float multiplier, double shape, double scale, double shift, bool fitted) {
    if (d != d) return NAN;
    double out = 0.0;
    if (fitted) {
        const double z = (double)(-__fmul_rn(multiplier, d)) - shift + 1.0;
        if (z > 0.0) out = 1.0 - exp(-pow(z / scale, shape));
    }
    return (float)out;
}

// ------------------------------------------------------------------------------------------------------------- set cover
constexpr int CV_NT = 1024;
constexpr int CV_MAX_W = OSI_EVM_MAX_COVER_ROWS / 64;
inline size_t cover_bytes(long long R) {
    if (R <= 0 || R > OSI_EVM_MAX_COVER_ROWS) return 0;
    const size_t W = (size_t)((R + 63) / 64);
    return (size_t)R * W * 8 + (size_t)R * 4;
}

// One workgroup per row i: word w of its cover row holds the rows 64 w .. 64 w + 63 it covers; cnt[i] = their number.
__global__ __launch_bounds__(NT) void k_evm_cover_build(const float* __restrict__ dpp, int R, int W, const double* __restrict__ shape,
                                                       const double* __restrict__ scale, const double* __restrict__ shift,
                                                       const unsigned char* __restrict__ fitted, float multiplier, float thr,
                                                       unsigned long long* __restrict__ cover, int* __restrict__ cnt) {
    __shared__ int wsum[NW];
    const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool fi = fitted[i] != 0;
    const double k = shape[i], lam = scale[i], sh = shift[i];
    int n = 0;
    for (int j0 = 0; j0 < W * 64; j0 += NT) {               // uniform trip count
        const int j = j0 + threadIdx.x;
        bool bit = false;
        if (fi && j < R && fitted[j]) bit = j == i || evm_psi(dpp[(size_t)i * R + j], multiplier, k, lam, sh, true) >= thr;
        const unsigned long long m = __ballot(bit);
        if (lane == 0 && (j >> 6) < W) cover[(size_t)i * W + (j >> 6)] = m;
        n += __popcll(m);
    }
    if (lane == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += wsum[w];
        cnt[i] = t;
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// ONE workgroup. U = the rows still to cover (bits), cnt[i] = |cover[i] & U|. Thread t alone reads and writes cnt[t + 1024 m]. A pick p
// removes newly = cover[p] & U from U; every row then takes popcount(cover[i][w] & newly[w]) off its count over the words w that
// changed. A picked row's count falls to 0 by that very update (it covers itself), so it is never picked again.
__global__ __launch_bounds__(CV_NT) void k_evm_cover_pick(const unsigned long long* __restrict__ cover, int* __restrict__ cnt, int R, int W,
                                                         const unsigned char* __restrict__ fitted, long long* __restrict__ order,
                                                         long long* __restrict__ n_ev) {
    __shared__ unsigned long long U[CV_MAX_W], newly[CV_MAX_W], wbest[CV_NT / 64];
    __shared__ int list[CV_MAX_W];
    __shared__ int s_left, s_nw, s_pick;
    const int tid = threadIdx.x;
    for (int w = tid; w < W; w += CV_NT) {
        unsigned long long m = 0;
        for (int b = 0; b < 64; ++b) {
            const int j = 64 * w + b;
            if (j < R && fitted[j]) m |= 1ull << b;
        }
        U[w] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int left = 0;
        for (int w = 0; w < W; ++w) left += __popcll(U[w]);
        s_left = left;
    }
    __syncthreads();
    int n = 0;
    while (s_left > 0 && n < R) {                           // uniform: s_left changes between barriers only
        // the largest count, the lowest index on ties
        unsigned long long best = 0;
        for (int i = tid; i < R; i += CV_NT) {
            const int c = cnt[i];
            const unsigned long long key = c > 0 ? ((unsigned long long)c << 32) | (unsigned)(0x7fffffff - i) : 0ull;
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) wbest[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long m = wbest[0];
            for (int w = 1; w < CV_NT / 64; ++w) m = wbest[w] > m ? wbest[w] : m;
            s_pick = m ? 0x7fffffff - (int)(unsigned)(m & 0xffffffffull) : -1;
        }
        __syncthreads();
        const int p = s_pick;
        if (p < 0) break;                                   // cannot happen: an uncovered row covers itself
        for (int w = tid; w < W; w += CV_NT) {
            const unsigned long long nw = cover[(size_t)p * W + w] & U[w];
            newly[w] = nw;
            U[w] &= ~nw;
        }
        __syncthreads();
        if (tid == 0) {
            order[n] = p;
            int k = 0, gone = 0;
            for (int w = 0; w < W; ++w)
                if (newly[w]) { list[k++] = w; gone += __popcll(newly[w]); }
            s_nw = k;
            s_left -= gone;
        }
        __syncthreads();
        const int nw = s_nw;
        for (int i = tid; i < R; i += CV_NT) {
            const unsigned long long* row = cover + (size_t)i * W;
            int d = 0;
            for (int l = 0; l < nw; ++l) d += __popcll(row[list[l]] & newly[list[l]]);
            if (d) cnt[i] -= d;
        }
        ++n;
        __syncthreads();                                    // newly, list and s_* are rewritten by the next round
    }
    for (int i = n + tid; i < R; i += CV_NT) order[i] = -1;
    if (tid == 0) n_ev[0] = n;
}

// ----------------------------------------------------------------------------------------------------------------- probs
__global__ __launch_bounds__(NT) void k_evm_probs(const float* __restrict__ dist, unsigned long long total, long long ld, int V, int C,
                                                 const double* __restrict__ shape, const double* __restrict__ scale,
                                                 const double* __restrict__ shift, const long long* __restrict__ ev_start,
                                                 float multiplier, float* __restrict__ probs) {
    for (unsigned long long t = (unsigned long long)blockIdx.x * NT + threadIdx.x; t < total; t += (unsigned long long)gridDim.x * NT) {
        const int c = (int)(t % (unsigned)C);
        const float* drow = dist + (size_t)(t / (unsigned)C) * (size_t)ld;
        long long v0 = ev_start[c], v1 = ev_start[c + 1];
        v0 = v0 < 0 ? 0 : v0;                               // a damaged offset table reads nothing outside the row
        v1 = v1 > V ? V : v1;
        float best = 0.f;
        for (long long v = v0; v < v1; ++v) {
            const double lam = scale[v];
            best = osi_max(best, evm_psi(drow[v], multiplier, shape[v], lam, shift[v], lam != 0.0));   // NaN-keeping
        }
        probs[t] = best;
    }
}

inline size_t evm_ws_bytes(long long R, long long N) {
    const size_t d = (size_t)(R + N) * sizeof(double), c = cover_bytes(R);
    return (d > c ? d : c) + 64;
}

}  // namespace

extern "C" {

size_t osi_evm_workspace(int R, int N, int F) { return (R > 0 && N > 0 && F > 0) ? evm_ws_bytes(R, N) : 0; }

int osi_evm_distances(const float* a, int R, const float* b, int N, int F, int metric, float* dist, void* ws, size_t ws_bytes,
                      osi_stream_t stream) {
    OSI_REQUIRE(a && b && dist && ws);
    OSI_REQUIRE(R > 0 && N > 0 && F > 0);
    OSI_REQUIRE(metric == OSI_EVM_EUCLIDEAN || metric == OSI_EVM_COSINE);
    OSI_REQUIRE((long long)R * N * 4 < DESC_LIMIT && (long long)R * F * 4 < DESC_LIMIT && (long long)N * F * 4 < DESC_LIMIT);
    OSI_REQUIRE(ws_bytes >= (size_t)((long long)R + N) * sizeof(double) && ((uintptr_t)ws & 7) == 0);
    OSI_REQUIRE(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0);
    hipStream_t st = (hipStream_t)stream;
    double* norms = (double*)ws;
    hipLaunchKernelGGL(k_evm_norms, dim3(stride_blocks((long long)R + N)), dim3(NT), 0, st, a, R, b, N, F, norms);
    OSI_LAUNCH_CHECK();
    const dim3 grid(osi_cdiv(N, PB), osi_cdiv(R, PB));
    if (F % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0)
        hipLaunchKernelGGL(k_evm_pairwise<true>, grid, dim3(NT), 0, st, a, R, b, N, F, metric, (const double*)norms,
                           (const double*)(norms + R), dist);
    else
        hipLaunchKernelGGL(k_evm_pairwise<false>, grid, dim3(NT), 0, st, a, R, b, N, F, metric, (const double*)norms,
                           (const double*)(norms + R), dist);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_evm_fit_rows(const float* dist, int R, int N, long long ld, const long long* gt, long long cls, int T, float multiplier,
                     double* shape, double* scale, double* shift, unsigned char* fitted, long long* tail_count, long long* flags2,
                     void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(dist && gt && shape && scale && shift && fitted && tail_count && flags2 && ws);
    OSI_REQUIRE(R > 0 && N > 0 && ld >= N);
    OSI_REQUIRE(T >= 2 && T <= OSI_EVM_MAX_TAIL);
    OSI_REQUIRE(multiplier > 0.f && multiplier - multiplier == 0.f);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(flags2, 0, 2 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    hipLaunchKernelGGL(k_evm_fit, dim3(R), dim3(NT), 0, st, dist, N, ld, gt, cls, T, multiplier, shape, scale, shift, fitted, tail_count,
                       flags2);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_evm_set_cover(const float* dpp, int R, const double* shape, const double* scale, const double* shift,
                      const unsigned char* fitted, float multiplier, float cover_threshold, long long* order, long long* n_ev, void* ws,
                      size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(dpp && shape && scale && shift && fitted && order && n_ev && ws);
    OSI_REQUIRE(R > 0 && R <= OSI_EVM_MAX_COVER_ROWS);
    OSI_REQUIRE(multiplier > 0.f && multiplier - multiplier == 0.f && cover_threshold == cover_threshold);
    OSI_REQUIRE(ws_bytes >= cover_bytes(R) && ((uintptr_t)ws & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    const int W = (R + 63) / 64;
    unsigned long long* cover = (unsigned long long*)ws;
    int* cnt = (int*)(cover + (size_t)R * W);
    hipLaunchKernelGGL(k_evm_cover_build, dim3(R), dim3(NT), 0, st, dpp, R, W, shape, scale, shift, fitted, multiplier, cover_threshold,
                       cover, cnt);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_evm_cover_pick, dim3(1), dim3(CV_NT), 0, st, (const unsigned long long*)cover, cnt, R, W, fitted, order, n_ev);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_evm_probs(const float* dist, int M, int V, long long ld, const double* shape, const double* scale, const double* shift,
                  const long long* ev_start, int C, float multiplier, float* probs, osi_stream_t stream) {
    OSI_REQUIRE(dist && shape && scale && shift && ev_start && probs);
    OSI_REQUIRE(M > 0 && V > 0 && C > 0 && ld >= V);
    OSI_REQUIRE(multiplier > 0.f && multiplier - multiplier == 0.f);
    const unsigned long long total = (unsigned long long)M * (unsigned long long)C;
    hipLaunchKernelGGL(k_evm_probs, dim3(stride_blocks((long long)total)), dim3(NT), 0, (hipStream_t)stream, dist, total, ld, V, C, shape,
                       scale, shift, ev_start, multiplier, probs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
