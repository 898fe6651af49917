// Mahalanobis / Relative Mahalanobis open-set scores (Lee, Lee, Lee, Shin, NeurIPS 2018; Ren et al., 2021) on the GPU: the fp64 dense
// linear algebra of a tied-covariance class-conditional Gaussian. include/osi.h (ABI 25) is the definition; openset_imagenet/
// mahalanobis.py is the user's face of it.
//
// ONE tile routine, gemm_tile (gemm_f64.h), feeds v_mfma_f64_16x16x4_f64: a workgroup of four waves owns a 64 x 64 tile of C = A B^T, a wave a
// 32 x 32 quarter of it (2 x 2 MFMA tiles, 16 accumulator doubles per lane). Both operands are staged through LDS K-major, 16 values of
// the summed index per stage, the next stage's global loads in flight in registers while this one multiplies. What differs between the
// callers is only where an operand element comes from (a loader) and where a result element goes (the kernel's epilogue):
//   scatter   the summed index is the ROW of X: both operands read rows of X contiguously along F, centred on the fly (one rounded fp64
//             subtraction). Lower-triangle tiles only; the rows are cut into a fixed number of splits (a function of N and F alone), every
//             split writes its partial tile to the workspace and k_scatter_reduce adds them in split order and mirrors. No atomics.
//   factor    right-looking blocked Cholesky, panel width NB = 64, three launches per panel: the diagonal block by one workgroup in LDS
//             (k_potrf_diag), the panel below it by substitution, one thread per row (k_trsm_rows), the trailing matrix by gemm_tile
//             (k_syrk_update). W = L^-1 by rows: W starts as I, and for the panels from the last to the first W[:, J] <- W[:, J] L_JJ^-1
//             (k_trsm_rows again) and W[:, < J] -= W[:, J] L[J, < J] (k_winv_update, gemm_tile). A failed pivot sets info; every later
//             launch reads it and leaves, so the launch sequence depends on F only and nothing waits on another workgroup.
//   whiten    z = x W^T, the K range of a column tile ends at its diagonal.
// The remaining kernels (means, trace, form, finish, sqdist) are plain fp64 vector code with fixed-order reductions.
// Addressing is 64-bit throughout; the argument checks keep every element count below 2^31 (include/osi.h).
#include "gemm_f64.h"                       // gemm_tile, Tile, the operand loaders, tile_i / tile_j (shared with vim.hip)

#include <math.h>

namespace {

constexpr int NB = 64;                      // panel width of the factorisation
constexpr int LDB = NB + 1;
constexpr int MAX_F = OSI_MAHA_MAX_F;
constexpr size_t WS_HEAD = 64;              // bytes in front of the scatter partials: [0] the trace
constexpr int MAX_SPLITS = 64;
static_assert(NB == TM, "panel offsets are tile offsets");

// tile t of a lower triangle, row by row: t = bi (bi + 1) / 2 + bj, bj <= bi
__device__ __forceinline__ void tri_tile(int t, int& bi, int& bj) {
    int b = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((long long)(b + 1) * (b + 2) / 2 <= t) ++b;
    while ((long long)b * (b + 1) / 2 > t) --b;
    bi = b;
    bj = t - (int)((long long)b * (b + 1) / 2);
}

// ------------------------------------------------------------------------------------------------------------------- means
constexpr int MC = 32, MS = NT / MC;        // lanes along the columns, row segments summed side by side
constexpr int ME = 4;                       // columns per thread (MC apart): a workgroup's scan of the labels serves MC * ME columns
constexpr int MU = 8;                       // rows whose labels and loads are in flight together
__global__ __launch_bounds__(NT) void k_maha_means(const float* __restrict__ x, const long long* __restrict__ gt, int N, int C, int F,
                                                  double* __restrict__ mean, long long* __restrict__ count) {
    __shared__ double ps[MS][ME][MC];
    __shared__ long long pc[MS];
    const int c = blockIdx.x, lc = threadIdx.x & (MC - 1), seg = threadIdx.x / MC;
    const int col0 = blockIdx.y * (MC * ME) + lc;
    const int per = (N + MS - 1) / MS;
    const int n0 = seg * per < N ? seg * per : N, n1 = n0 + per < N ? n0 + per : N;
    double s[ME] = {0.0, 0.0, 0.0, 0.0};
    long long cnt = 0;
    int colc[ME];                                           // a column past F reads the last one and is never stored
#pragma unroll
    for (int e = 0; e < ME; ++e) colc[e] = col0 + MC * e < F ? col0 + MC * e : F - 1;
    for (int nb = n0; nb < n1; nb += MU) {                  // rows in ascending order within a segment
        long long g[MU];
#pragma unroll
        for (int u = 0; u < MU; ++u) g[u] = gt[nb + u < n1 ? nb + u : n1 - 1];
        // every load is issued before the first add: a row that does not match reads row n0 again (cached) and adds an exact zero,
        // so no load waits behind a branch on a label
        bool hit[MU];
        float v[MU][ME];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            const int n = nb + u;
            hit[u] = n < n1 && (c < C ? g[u] == (long long)c : (g[u] >= 0 && g[u] < (long long)C));
            const float* row = x + (size_t)(hit[u] ? n : n0) * (size_t)F;
#pragma unroll
            for (int e = 0; e < ME; ++e) v[u][e] = row[colc[e]];
        }
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            cnt += hit[u] ? 1 : 0;
#pragma unroll
            for (int e = 0; e < ME; ++e) s[e] += hit[u] ? (double)v[u][e] : 0.0;
        }
    }
#pragma unroll
    for (int e = 0; e < ME; ++e) ps[seg][e][lc] = s[e];
    if (lc == 0) pc[seg] = cnt;
    __syncthreads();
    if (seg == 0) {
        long long n = pc[0];
        for (int q = 1; q < MS; ++q) n += pc[q];
#pragma unroll
        for (int e = 0; e < ME; ++e) {
            double tot = ps[0][e][lc];
            for (int q = 1; q < MS; ++q) tot += ps[q][e][lc];
            if (col0 + MC * e < F) mean[(size_t)c * (size_t)F + (size_t)(col0 + MC * e)] = n > 0 ? tot / (double)n : 0.0;
        }
        if (blockIdx.y == 0 && lc == 0) count[c] = n;
    }
}

// ----------------------------------------------------------------------------------------------------------------- scatter
__global__ __launch_bounds__(NT) void k_scatter_partial(CentredRows ld, int N, int rows_per, double* __restrict__ part, int ntri) {
    __shared__ Tile sm;
    int bi, bj;
    tri_tile(blockIdx.x, bi, bj);
    const int s = blockIdx.y;
    const long long nb = (long long)s * rows_per;
    const int n0 = (int)(nb < N ? nb : N), n1 = (int)(nb + rows_per < N ? nb + rows_per : N);
    CentredRows la = ld, lb = ld;
    la.c0 = bi * TM;
    lb.c0 = bj * TM;
    f64x4 acc[2][2];
    gemm_tile(sm, la, lb, n0, n1, acc);
    double* out = part + ((size_t)s * (size_t)ntri + (size_t)blockIdx.x) * (size_t)(TM * TM);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[tile_i(ti, r) * TM + tile_j(tj)] = acc[ti][tj][r];
}

__global__ __launch_bounds__(NT) void k_scatter_reduce(const double* __restrict__ part, int ntri, int splits, int F, int accumulate,
                                                      double* __restrict__ S) {
    int bi, bj;
    tri_tile(blockIdx.x, bi, bj);
    for (int e = threadIdx.x; e < TM * TM; e += NT) {
        const int gi = bi * TM + e / TM, gj = bj * TM + e % TM;
        if (gi >= F || gj > gi) continue;
        const double* p = part + (size_t)blockIdx.x * (size_t)(TM * TM) + (size_t)e;
        double v = p[0];
        for (int s = 1; s < splits; ++s) v += p[(size_t)s * (size_t)ntri * (size_t)(TM * TM)];
        if (accumulate) v = S[(size_t)gi * (size_t)F + (size_t)gj] + v;
        S[(size_t)gi * (size_t)F + (size_t)gj] = v;
        S[(size_t)gj * (size_t)F + (size_t)gi] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ factor
__global__ __launch_bounds__(NT) void k_trace(const double* __restrict__ S, int F, double* __restrict__ head, int* __restrict__ info) {
    __shared__ double sh[NT];
    double s = 0.0;
    for (int i = threadIdx.x; i < F; i += NT) s += S[(size_t)i * (size_t)F + (size_t)i];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        head[0] = s;
        info[0] = 0;
    }
}

// L <- the lower triangle of Sigma = c1 S + alpha (scale tr S / F) I, zeros above; W <- I
__global__ __launch_bounds__(NT) void k_form(const double* __restrict__ S, int F, double c1, double alpha, double scale,
                                            const double* __restrict__ head, double* __restrict__ L, double* __restrict__ W) {
    const double ridge = alpha * (scale * head[0] / (double)F);
    const size_t total = (size_t)F * (size_t)F;
    for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
        const int i = (int)(e / (size_t)F), j = (int)(e - (size_t)i * (size_t)F);
        double v = 0.0;
        if (j < i) v = c1 * S[e];
        else if (j == i) v = c1 * S[e] + ridge;
        L[e] = v;
        W[e] = i == j ? 1.0 : 0.0;
    }
}

// the nbw x nbw diagonal block at p, in place: unblocked right-looking Cholesky in LDS by one workgroup
__global__ __launch_bounds__(NT) void k_potrf_diag(double* __restrict__ L, int F, int p, int nbw, int* __restrict__ info) {
    __shared__ double a[NB][LDB];
    __shared__ double dg[NB];
    if (info[0] != 0) return;                               // uniform
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += NT) {
        const int i = e / NB, j = e % NB;
        a[i][j] = (i < nbw && j <= i) ? L[(size_t)(p + i) * (size_t)F + (size_t)(p + j)] : 0.0;
    }
    for (int j = 0; j < nbw; ++j) {
        __syncthreads();                                    // the block is loaded / column j has its last update
        const double piv = a[j][j];
        if (!(piv > 0.0) || piv == INFINITY) {              // uniform: every thread reads the same pivot
            if (tid == 0) info[0] = p + j + 1;
            return;
        }
        const double d = sqrt(piv);
        if (tid == 0) dg[j] = d;
        for (int i = j + 1 + tid; i < nbw; i += NT) a[i][j] = a[i][j] / d;
        __syncthreads();
        const int m = nbw - j - 1;                          // the trailing m x m block, lower triangle
        for (int e = tid; e < m * m; e += NT) {
            const int i = j + 1 + e / m, k = j + 1 + e % m;
            if (k <= i) a[i][k] = fma(-a[i][j], a[k][j], a[i][k]);
        }
    }
    __syncthreads();
    for (int e = tid; e < nbw * nbw; e += NT) {
        const int i = e / nbw, j = e % nbw;
        if (j <= i) L[(size_t)(p + i) * (size_t)F + (size_t)(p + j)] = j == i ? dg[i] : a[i][j];
    }
}

// Rows r0 + ... of X[:, p : p + nbw] <- X T^-1 with T the diagonal block of L at p: T = L_pp^T (REVERSE = false, the panel solve of the
// factorisation) or T = L_pp (REVERSE = true, the inverse). One thread per row, substitution with true divisions; the block and the 64
// rows live in LDS (a thread touches its own column of xs only, so the loops need no barrier).
template <bool REVERSE>
__global__ __launch_bounds__(64) void k_trsm_rows(double* X, const double* L, int F, int p, int nbw, int r0, const int* __restrict__ info) {
    __shared__ double l[NB][NB];
    __shared__ double xs[NB][64];
    if (info[0] != 0) return;
    const int t = threadIdx.x;
    for (int e = t; e < NB * NB; e += 64) {
        const int i = e / NB, j = e % NB;
        l[i][j] = (i < nbw && j <= i) ? L[(size_t)(p + i) * (size_t)F + (size_t)(p + j)] : (i == j ? 1.0 : 0.0);
    }
    const int row = r0 + (int)blockIdx.x * 64 + t;
    double* xr = X + (size_t)(row < F ? row : 0) * (size_t)F + (size_t)p;
    for (int j = 0; j < nbw; ++j) xs[j][t] = row < F ? xr[j] : 0.0;
    __syncthreads();
    if (!REVERSE) {
        for (int j = 0; j < nbw; ++j) {
            const double v = xs[j][t] / l[j][j];
            xs[j][t] = v;
#pragma unroll 4
            for (int k = j + 1; k < nbw; ++k) xs[k][t] = fma(-v, l[k][j], xs[k][t]);
        }
    } else {
        for (int j = nbw - 1; j >= 0; --j) {
            const double v = xs[j][t] / l[j][j];
            xs[j][t] = v;
#pragma unroll 4
            for (int k = 0; k < j; ++k) xs[k][t] = fma(-v, l[j][k], xs[k][t]);
        }
    }
    if (row < F)
        for (int j = 0; j < nbw; ++j) xr[j] = xs[j][t];
}

// trailing matrix at q = p + nbw: L[q + i][q + j] -= sum over the panel's columns k of L[q + i][k] L[q + j][k], lower-triangle tiles
__global__ __launch_bounds__(NT) void k_syrk_update(double* __restrict__ L, int F, int p, int nbw, const int* __restrict__ info) {
    __shared__ Tile sm;
    if (info[0] != 0) return;
    int bi, bj;
    tri_tile(blockIdx.x, bi, bj);
    const int q = p + nbw;
    const RowsOfMatrix<double> la{L, (size_t)F, q + bi * TM, F}, lb{L, (size_t)F, q + bj * TM, F};
    f64x4 acc[2][2];
    gemm_tile(sm, la, lb, p, q, acc);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = q + bi * TM + tile_i(ti, r), gj = q + bj * TM + tile_j(tj);
                if (gi < F && gj <= gi) L[(size_t)gi * (size_t)F + (size_t)gj] -= acc[ti][tj][r];
            }
}

// W[p + i][j] -= sum over the panel's columns k of W[p + i][k] L[k][j] for the columns j < p
__global__ __launch_bounds__(NT) void k_winv_update(double* __restrict__ W, const double* __restrict__ L, int F, int p, int nbw,
                                                   const int* __restrict__ info) {
    __shared__ Tile sm;
    if (info[0] != 0) return;
    const int i0 = p + (int)blockIdx.x * TM, j0 = (int)blockIdx.y * TM;
    const RowsOfMatrix<double> la{W, (size_t)F, i0, F};
    const ColsOfMatrix lb{L, (size_t)F, j0, p};
    f64x4 acc[2][2];
    gemm_tile(sm, la, lb, p, p + nbw, acc);
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + tile_i(ti, r), gj = j0 + tile_j(tj);
                if (gi < F && gj < p) W[(size_t)gi * (size_t)F + (size_t)gj] -= acc[ti][tj][r];
            }
}

// success: logdet = 2 sum ln L_ii (workgroup 0, fixed order). failure: L = W = 0, logdet = NaN.
__global__ __launch_bounds__(NT) void k_finish(double* __restrict__ L, double* __restrict__ W, int F, double* __restrict__ logdet,
                                              const int* __restrict__ info) {
    __shared__ double sh[NT];
    const bool failed = info[0] != 0;                       // uniform
    if (failed) {
        const size_t total = (size_t)F * (size_t)F;
        for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < total; e += (size_t)gridDim.x * NT) {
            L[e] = 0.0;
            W[e] = 0.0;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) logdet[0] = NAN;
        return;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < F; i += NT) s += log(L[(size_t)i * (size_t)F + (size_t)i]);
    s = block_sum(s, sh);
    if (threadIdx.x == 0) logdet[0] = 2.0 * s;
}

// ------------------------------------------------------------------------------------------------------------------ whiten
template <class T>
__global__ __launch_bounds__(NT) void k_whiten(const T* __restrict__ x, int M, int F, const double* __restrict__ W, double* __restrict__ z) {
    __shared__ Tile sm;
    const int i0 = (int)blockIdx.x * TM, j0 = (int)blockIdx.y * TM;
    const RowsOfMatrix<T> la{x, (size_t)F, i0, M};
    const RowsOfMatrix<double> lb{W, (size_t)F, j0, F};
    f64x4 acc[2][2];
    gemm_tile(sm, la, lb, 0, j0 + TM < F ? j0 + TM : F, acc);     // W is lower triangular: nothing past the tile's last column
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = i0 + tile_i(ti, r), gj = j0 + tile_j(tj);
                if (gi < M && gj < F) z[(size_t)gi * (size_t)F + (size_t)gj] = acc[ti][tj][r];
            }
}

// ------------------------------------------------------------------------------------------------------------------ sqdist
constexpr int SQ_R = 4;                     // rows a wave scores against one class at a time
__global__ __launch_bounds__(NT) void k_maha_sqdist(const double* __restrict__ z, int M, const double* __restrict__ zm, int C, int F,
                                                   const double* __restrict__ minus, int transform, float* __restrict__ o32,
                                                   double* __restrict__ o64) {
    const int lane = threadIdx.x & 63;
    const long long units = (long long)((M + SQ_R - 1) / SQ_R) * C;
    for (long long u = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6); u < units; u += (long long)gridDim.x * (NT / 64)) {
        const long long g = u / C;
        const int c = (int)(u - g * C), i0 = (int)g * SQ_R;
        const double* zc = zm + (size_t)c * (size_t)F;
        const double* zr[SQ_R];
#pragma unroll
        for (int r = 0; r < SQ_R; ++r) zr[r] = z + (size_t)(i0 + r < M ? i0 + r : M - 1) * (size_t)F;
        double acc[SQ_R] = {0.0, 0.0, 0.0, 0.0};
        for (int j = lane; j < F; j += 64) {
            const double m = zc[j];
#pragma unroll
            for (int r = 0; r < SQ_R; ++r) {
                const double d = zr[r][j] - m;
                acc[r] = fma(d, d, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < SQ_R; ++r) acc[r] = wave_sum(acc[r]);
        double v = acc[0];
#pragma unroll
        for (int r = 1; r < SQ_R; ++r) v = lane == r ? acc[r] : v;
        const int i = i0 + lane;
        if (lane < SQ_R && i < M) {
            if (minus) v -= minus[i];
            const double h = 2.0 * (double)F;
            if (transform == OSI_MAHA_SIM_GAUSS) v = v != v ? v : exp(-fmax(v, 0.0) / h);
            else if (transform == OSI_MAHA_SIM_LOGISTIC) v = 1.0 / (1.0 + exp(v / h));
            const size_t o = (size_t)i * (size_t)C + (size_t)c;
            if (o32) o32[o] = (float)v;
            else o64[o] = v;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------- host
inline int tiles_of(int n) { return (n + TM - 1) / TM; }
inline long long tri_of(int nt) { return (long long)nt * (nt + 1) / 2; }
inline int scatter_splits(int N, int F) {                   // a function of N and F alone: the summation order is part of the result
    const long long ntri = tri_of(tiles_of(F));
    long long by_rows = ((long long)N + 511) / 512, by_grid = 4096 / ntri;
    long long s = by_rows < by_grid ? by_rows : by_grid;
    if (s > MAX_SPLITS) s = MAX_SPLITS;
    return (int)(s < 1 ? 1 : s);
}
inline size_t scatter_ws(int N, int F) { return WS_HEAD + (size_t)scatter_splits(N, F) * (size_t)tri_of(tiles_of(F)) * (size_t)(TM * TM) * 8; }
inline bool sizes_ok(long long rows, int F) { return rows > 0 && F > 0 && F <= MAX_F && rows * (long long)F < MAX_ELEMS; }
inline bool ws_ok(const void* ws, size_t have, size_t need) { return ws && have >= need && ((uintptr_t)ws & 7) == 0; }
inline int flat_grid(size_t elems) {
    const size_t b = (elems + NT - 1) / NT;
    return (int)(b < 4096 ? (b < 1 ? 1 : b) : 4096);
}

template <class T>
int whiten(const T* x, int M, int F, const double* W, double* z, void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(x && W && z);
    OSI_REQUIRE(sizes_ok(M, F));
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    hipLaunchKernelGGL(k_whiten<T>, dim3(tiles_of(M), tiles_of(F)), dim3(NT), 0, (hipStream_t)stream, x, M, F, W, z);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // namespace

extern "C" {

size_t osi_maha_workspace(int N, int C, int F) {
    if (N <= 0 || C <= 0 || F <= 0 || F > MAX_F) return 0;
    return scatter_ws(N, F);
}

int osi_maha_class_means(const float* features, const long long* gt, int N, int C, int F, double* mean, long long* count, void* ws,
                         size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(features && gt && mean && count);
    OSI_REQUIRE(sizes_ok(N, F) && C > 0 && sizes_ok((long long)C + 1, F));
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    hipLaunchKernelGGL(k_maha_means, dim3(C + 1, (F + MC * ME - 1) / (MC * ME)), dim3(NT), 0, (hipStream_t)stream, features, gt, N, C, F, mean, count);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_maha_scatter(const float* features, const long long* gt, const double* mean, int N, int C, int F, int mode, int accumulate,
                     double* S, void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(features && gt && mean && S);
    OSI_REQUIRE(sizes_ok(N, F) && C > 0 && sizes_ok((long long)C + 1, F));
    OSI_REQUIRE(mode == OSI_MAHA_WITHIN || mode == OSI_MAHA_TOTAL);
    OSI_REQUIRE(accumulate == 0 || accumulate == 1);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, scatter_ws(N, F)));
    const int splits = scatter_splits(N, F), ntri = (int)tri_of(tiles_of(F));
    const int rows_per = ((N + splits - 1) / splits + KT - 1) / KT * KT;
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + WS_HEAD);
    const CentredRows ld{features, gt, mean, C, F, mode, 0};
    hipLaunchKernelGGL(k_scatter_partial, dim3(ntri, splits), dim3(NT), 0, (hipStream_t)stream, ld, N, rows_per, part, ntri);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_scatter_reduce, dim3(ntri), dim3(NT), 0, (hipStream_t)stream, part, ntri, splits, F, accumulate, S);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_maha_factor(const double* S, int F, double scale, double shrinkage, double* L, double* W, double* logdet, int* info, void* ws,
                    size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(S && L && W && logdet && info);
    OSI_REQUIRE(F > 0 && F <= MAX_F);
    OSI_REQUIRE(scale > 0.0 && scale <= 1.7976931348623157e308);            // false for a NaN
    OSI_REQUIRE(shrinkage >= 0.0 && shrinkage <= 1.0);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    const hipStream_t st = (hipStream_t)stream;
    double* head = static_cast<double*>(ws);
    const size_t total = (size_t)F * (size_t)F;
    hipLaunchKernelGGL(k_trace, dim3(1), dim3(NT), 0, st, S, F, head, info);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_form, dim3(flat_grid(total)), dim3(NT), 0, st, S, F, (1.0 - shrinkage) * scale, shrinkage, scale, head, L, W);
    OSI_LAUNCH_CHECK();
    for (int p = 0; p < F; p += NB) {
        const int nbw = F - p < NB ? F - p : NB, q = p + nbw;
        hipLaunchKernelGGL(k_potrf_diag, dim3(1), dim3(NT), 0, st, L, F, p, nbw, info);
        OSI_LAUNCH_CHECK();
        if (q < F) {
            hipLaunchKernelGGL(k_trsm_rows<false>, dim3((F - q + 63) / 64), dim3(64), 0, st, L, L, F, p, nbw, q, info);
            OSI_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_syrk_update, dim3((int)tri_of(tiles_of(F - q))), dim3(NT), 0, st, L, F, p, nbw, info);
            OSI_LAUNCH_CHECK();
        }
    }
    for (int p = (F - 1) / NB * NB; p >= 0; p -= NB) {
        const int nbw = F - p < NB ? F - p : NB;
        hipLaunchKernelGGL(k_trsm_rows<true>, dim3((F - p + 63) / 64), dim3(64), 0, st, W, L, F, p, nbw, p, info);
        OSI_LAUNCH_CHECK();
        if (p > 0) {
            hipLaunchKernelGGL(k_winv_update, dim3(tiles_of(F - p), tiles_of(p)), dim3(NT), 0, st, W, L, F, p, nbw, info);
            OSI_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_finish, dim3(flat_grid(total)), dim3(NT), 0, st, L, W, F, logdet, info);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_maha_whiten_f32(const float* x, int M, int F, const double* W, double* z, void* ws, size_t ws_bytes, osi_stream_t stream) {
    return whiten<float>(x, M, F, W, z, ws, ws_bytes, stream);
}
int osi_maha_whiten_f64(const double* x, int M, int F, const double* W, double* z, void* ws, size_t ws_bytes, osi_stream_t stream) {
    return whiten<double>(x, M, F, W, z, ws, ws_bytes, stream);
}

int osi_maha_sqdist(const double* z, int M, const double* zm, int C, int F, const double* minus, int transform, float* out_f32,
                    double* out_f64, void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(z && zm);
    OSI_REQUIRE((out_f32 != nullptr) != (out_f64 != nullptr));
    OSI_REQUIRE(sizes_ok(M, F) && C > 0 && sizes_ok(C, F) && (long long)M * C < MAX_ELEMS);
    OSI_REQUIRE(transform == OSI_MAHA_RAW || transform == OSI_MAHA_SIM_GAUSS || transform == OSI_MAHA_SIM_LOGISTIC);
    OSI_REQUIRE(ws_ok(ws, ws_bytes, WS_HEAD));
    const long long units = (long long)((M + SQ_R - 1) / SQ_R) * C, blocks = (units + NT / 64 - 1) / (NT / 64);
    hipLaunchKernelGGL(k_maha_sqdist, dim3((int)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(NT), 0, (hipStream_t)stream, z, M, zm, C,
                       F, minus, transform, out_f32, out_f64);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
