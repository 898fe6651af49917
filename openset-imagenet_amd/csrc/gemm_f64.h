// The fp64 tile routine shared by mahalanobis.hip and vim.hip: gemm_tile feeds v_mfma_f64_16x16x4_f64. A workgroup of four waves owns a
// 64 x 64 tile of C = A B^T, a wave a 32 x 32 quarter of it (2 x 2 MFMA tiles, 16 accumulator doubles per lane). Both operands are
// staged through LDS K-major, 16 values of the summed index per stage, the next stage's global loads in flight in registers while this
// one multiplies. What differs between the callers is only where an operand element comes from (a loader) and where a result element
// goes (the kernel's epilogue). The two files' workgroup sum (block_sum) and element limit are here too. Everything lives in the
// including file's anonymous namespace.
#pragma once
#include "osi_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int NT = 256;
constexpr int TM = 64;                      // tile edge of gemm_tile
constexpr int KT = 16;                      // summed indices per LDS stage
constexpr int LDT = TM + 4;                 // LDS row stride in doubles
constexpr int EPT = KT * TM / NT;           // operand elements per thread and stage (4)
constexpr long long MAX_ELEMS = 1ll << 31;  // a call takes fewer elements than this in each of its matrices (include/osi.h)

template <class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {                   // a fixed tree over the 256 threads; every thread gets the sum
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

struct Tile {
    double a[KT][LDT];
    double b[KT][LDT];
};

// ---- operand loaders: element (k, i) of a K x 64 operand slab, zero outside the matrix --------------------------------------------
// K-minor: the matrix is [rows][ld] with the summed index along a row. Thread t takes k = t & 15 of the rows (t >> 4) + 16 e.
template <class T>
struct RowsOfMatrix {
    const T* p;
    size_t ld;
    int r0, rows;                           // first row of the slab, rows of the matrix
    __device__ __forceinline__ void fetch(int k0, int kend, double (&r)[EPT]) const {
        const int k = k0 + (int)(threadIdx.x & 15), ii = (int)(threadIdx.x >> 4);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int row = r0 + ii + 16 * e;
            r[e] = (row < rows && k < kend) ? (double)p[(size_t)row * ld + (size_t)k] : 0.0;
        }
    }
    __device__ __forceinline__ void put(double (*s)[LDT], const double (&r)[EPT]) const {
        const int k = (int)(threadIdx.x & 15), ii = (int)(threadIdx.x >> 4);
#pragma unroll
        for (int e = 0; e < EPT; ++e) s[k][ii + 16 * e] = r[e];
    }
};
// K-major: the matrix is [K][ld] with the summed index down a column. Thread t takes column t & 63 of the rows (t >> 6) + 4 e.
struct ColsOfMatrix {
    const double* p;
    size_t ld;
    int c0, cols;
    __device__ __forceinline__ void fetch(int k0, int kend, double (&r)[EPT]) const {
        const int col = c0 + (int)(threadIdx.x & 63), kk = k0 + (int)(threadIdx.x >> 6);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int k = kk + 4 * e;
            r[e] = (col < cols && k < kend) ? p[(size_t)k * ld + (size_t)col] : 0.0;
        }
    }
    __device__ __forceinline__ void put(double (*s)[LDT], const double (&r)[EPT]) const {
        const int j = (int)(threadIdx.x & 63), kk = (int)(threadIdx.x >> 6);
#pragma unroll
        for (int e = 0; e < EPT; ++e) s[kk + 4 * e][j] = r[e];
    }
};
// K-major over the rows of X, centred: (double)x[n][col] - mean[class of n or C][col]; an uncounted row is a row of zeros.
struct CentredRows {
    const float* x;
    const long long* gt;
    const double* mean;
    int C, F, mode, c0;
    __device__ __forceinline__ void fetch(int k0, int kend, double (&r)[EPT]) const {
        const int col = c0 + (int)(threadIdx.x & 63), kk = k0 + (int)(threadIdx.x >> 6);
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int n = kk + 4 * e;
            double v = 0.0;
            if (col < F && n < kend) {
                const long long g = gt[n];
                if (g >= 0 && g < (long long)C) {
                    const size_t mrow = mode == OSI_MAHA_WITHIN ? (size_t)g : (size_t)C;
                    v = __dsub_rn((double)x[(size_t)n * (size_t)F + (size_t)col], mean[mrow * (size_t)F + (size_t)col]);
                }
            }
            r[e] = v;
        }
    }
    __device__ __forceinline__ void put(double (*s)[LDT], const double (&r)[EPT]) const {
        const int j = (int)(threadIdx.x & 63), kk = (int)(threadIdx.x >> 6);
#pragma unroll
        for (int e = 0; e < EPT; ++e) s[kk + 4 * e][j] = r[e];
    }
};

// acc[ti][tj][r] = sum over k in [kbegin, kend) of A(k, i) B(k, j) with i = wm + 16 ti + (lane >> 4) + 4 r, j = wn + 16 tj + (lane & 15)
// (tile_i / tile_j below). The summation order is fixed by (kbegin, kend) alone.
template <class LA, class LB>
__device__ __forceinline__ void gemm_tile(Tile& sm, const LA& la, const LB& lb, int kbegin, int kend, f64x4 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double ra[EPT], rb[EPT];
    la.fetch(kbegin, kend, ra);
    lb.fetch(kbegin, kend, rb);
    for (int k0 = kbegin; k0 < kend; k0 += KT) {
        __syncthreads();                                    // the previous stage is read
        la.put(sm.a, ra);
        lb.put(sm.b, rb);
        __syncthreads();
        if (k0 + KT < kend) {
            la.fetch(k0 + KT, kend, ra);
            lb.fetch(k0 + KT, kend, rb);
        }
#pragma unroll
        for (int ks = 0; ks < KT; ks += 4) {
            const double a0 = sm.a[ks + lk][wm + lr], a1 = sm.a[ks + lk][wm + 16 + lr];
            const double b0 = sm.b[ks + lk][wn + lr], b1 = sm.b[ks + lk][wn + 16 + lr];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}
__device__ __forceinline__ int tile_i(int ti, int r) {
    return (int)((threadIdx.x >> 7) * 32) + 16 * ti + (int)((threadIdx.x & 63) >> 4) + 4 * r;
}
__device__ __forceinline__ int tile_j(int tj) { return (int)(((threadIdx.x >> 6) & 1) * 32) + 16 * tj + (int)(threadIdx.x & 15); }

}  // namespace
