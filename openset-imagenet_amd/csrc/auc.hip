// ROC-AUC on the GPU: the counting behind metrics.auc_score_binary / auc_score_multiclass (reference openset_imagenet/
// metrics.py:65-106, two thin wrappers around sklearn.metrics.roc_auc_score).
//
// The area under the ROC curve of positives against negatives is the Mann-Whitney quotient
//     auc = (2 * #{pos > neg} + #{pos == neg}) / (2 * #pos * #neg)
// over all positive x negative pairs, and sklearn's trapezoid sum over the sorted thresholds is that quotient up to fp64 rounding.
// As for the OSCR curve (oscr.hip) the device therefore only COUNTS: all-pairs comparisons on the VALU, LDS-staged tiles, 32-bit
// partial counts inside a tile, 64-bit integer atomics per workgroup. No sort, no float accumulation, order-free by construction;
// the one division per curve is left to the host mirror.
//
//   binary       positives = rows with gt != unk_class, compared value = max over ALL columns (np.max(pred_scores, axis=1)).
//                A row pass partitions the row maxima (positives from the front of the workspace, negatives from its back; the
//                slot order inside each side is whatever the atomics hand out, which no count depends on), a pair pass tiles
//                positives x negatives in two dimensions.
//   one-vs-rest  row i is a positive of exactly one class c_i = gt[i] and meets column c_i of every row j with gt[j] != c_i:
//                O(N^2) comparisons in total, not O(C N^2). One thread per i, the j rows pass through LDS as [rows][C] tiles.
#include "osi_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int OVR_TILE_BYTES = 32768;   // LDS budget of one [rows][C] score tile
constexpr int OVR_MAX_C = 2048;         // widest row the LDS tiling takes: 16 KB in fp64 (2 rows a tile) + 2 x 8 KB class counters
constexpr int OVR_BLOCKS = 2048;        // workgroups a one-vs-rest launch aims for (8 per CU)
constexpr int OVR_MAX_CHUNK = 1 << 23;  // most j rows per workgroup: 256 threads x 2^23 stays inside its 32-bit LDS class counters

// lanes that share one row in the row passes: the largest power of two <= min(C, 64), so that a wave reads whole rows side by side
inline int row_lanes(int C) {
    int l = 1;
    while (l * 2 <= C && l < 64) l *= 2;
    return l;
}

// One row over L lanes (L a power of two <= C, groups aligned in the wave): maximum over all columns with NaNs skipped, "any NaN",
// and the fp64 row sum. Every lane of the wave runs the shuffles; rows past N contribute nothing and are ignored by the caller.
template <typename T>
__device__ __forceinline__ void scan_row(const T* __restrict__ scores, int row, int N, int C, int L, int sub, T& best, int& nan,
                                         double& sum) {
    best = (T)(-INFINITY);
    nan = 0;
    sum = 0.0;
    if (row < N) {
        const T* r = scores + (size_t)row * C;
        for (int c = sub; c < C; c += L) {
            const T v = r[c];
            nan |= (v != v) ? 1 : 0;
            best = v > best ? v : best;
            sum += (double)v;
        }
    }
    for (int o = L >> 1; o > 0; o >>= 1) {
        const T b = __shfl_xor(best, o, 64);
        best = b > best ? b : best;
        nan |= __shfl_xor(nan, o, 64);
        sum += __shfl_xor(sum, o, 64);
    }
}

// ---------------------------------------------------------------------------------------------------------------- binary
// counts: {gt, eq, P, Nn, #NaN rows}. vals[0 .. P) = maxima of the positives, vals[N-1 .. N-Nn] = maxima of the negatives.
// One integer atomic per wave and side hands out the slots (ballot + prefix popcount inside the wave).
template <typename T>
__global__ __launch_bounds__(NT) void k_auc_bin_rows(const T* __restrict__ scores, const long long* __restrict__ gt, int N, int C, int L,
                                                    long long unk_class, T* __restrict__ vals, long long* counts) {
    const int sub = threadIdx.x & (L - 1);
    const int row = blockIdx.x * (NT / L) + threadIdx.x / L;
    T best;
    int nan;
    double sum;
    scan_row(scores, row, N, C, L, sub, best, nan, sum);
    const bool lead = row < N && sub == 0;
    const bool pos = lead && gt[row] != unk_class;
    const bool neg = lead && !pos;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mp = __ballot(pos), mn = __ballot(neg);
    int base_p = 0, base_n = 0;
    if (mp) {
        const int first = __ffsll((long long)mp) - 1;
        if (lane == first) base_p = (int)atomicAdd((unsigned long long*)&counts[2], (unsigned long long)__popcll(mp));
        base_p = __shfl(base_p, first, 64);
    }
    if (mn) {
        const int first = __ffsll((long long)mn) - 1;
        if (lane == first) base_n = (int)atomicAdd((unsigned long long*)&counts[3], (unsigned long long)__popcll(mn));
        base_n = __shfl(base_n, first, 64);
    }
    if (pos) vals[base_p + __popcll(mp & below)] = best;
    if (neg) vals[N - 1 - (base_n + __popcll(mn & below))] = best;
    if (lead && nan) atomicAdd((unsigned long long*)&counts[4], 1ull);
}

// Workgroup (x, y) counts the pairs of positive tile x with negative tiles y, y + gridDim.y, ... Slots past either side hold a NaN
// in registers / LDS: every comparison with it is false, so the inner loop has a fixed length and no bound check.
template <typename T>
__global__ __launch_bounds__(NT) void k_auc_bin_pairs(const T* __restrict__ vals, int N, long long* counts) {
    __shared__ T sn[NT];
    __shared__ unsigned red[2][NT / 64];
    const int P = (int)counts[2], Nn = (int)counts[3];
    const int p0 = blockIdx.x * NT;
    if (p0 >= P) return;                                  // whole workgroup: uniform
    const int i = p0 + threadIdx.x;
    const T none = (T)NAN;
    const T v = i < P ? vals[i] : none;
    unsigned g = 0, e = 0;
    for (long long n0 = (long long)blockIdx.y * NT; n0 < Nn; n0 += (long long)gridDim.y * NT) {
        const long long j = n0 + threadIdx.x;
        sn[threadIdx.x] = j < Nn ? vals[N - 1 - j] : none;
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < NT; ++k) {
            const T x = sn[k];
            g += v > x ? 1u : 0u;
            e += v == x ? 1u : 0u;
        }
        __syncthreads();
    }
    g = wave_sum(g);
    e = wave_sum(e);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = g; red[1][threadIdx.x >> 6] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sg = 0, se = 0;
        for (int w = 0; w < NT / 64; ++w) { sg += red[0][w]; se += red[1][w]; }
        if (sg) atomicAdd((unsigned long long*)&counts[0], sg);
        if (se) atomicAdd((unsigned long long*)&counts[1], se);
    }
}

template <typename T>
int auc_binary_impl(const T* scores, const long long* gt, int N, int C, long long unk_class, void* ws, size_t ws_bytes,
                    long long* counts5, osi_stream_t stream) {
    OSI_REQUIRE(scores && gt && ws && counts5 && N > 0 && C > 0 && N <= INT_MAX - NT);
    OSI_REQUIRE(ws_bytes >= osi_auc_workspace(N));
    hipStream_t st = (hipStream_t)stream;
    T* vals = (T*)ws;
    if (hipMemsetAsync(counts5, 0, 5 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    const int L = row_lanes(C);
    hipLaunchKernelGGL(k_auc_bin_rows<T>, dim3(osi_cdiv(N, NT / L)), dim3(NT), 0, st, scores, gt, N, C, L, unk_class, vals, counts5);
    OSI_LAUNCH_CHECK();
    // the split of N into positives and negatives is only known on the device: the grid covers N x N, tiles past P or Nn leave at once
    const int tiles = osi_cdiv(N, NT);
    hipLaunchKernelGGL(k_auc_bin_pairs<T>, dim3(tiles, tiles < 65535 ? tiles : 65535), dim3(NT), 0, st, (const T*)vals, N, counts5);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

// ----------------------------------------------------------------------------------------------------------- one-vs-rest
// per row: label as an int (-1 = outside [0, C)) for the pair pass, the class histogram pos_c, and the three refusal counters
// flags3 = {labels outside [0, C), NaN rows, rows whose fp64 sum is not 1 within sklearn's allclose bound 1e-8 + 1e-5}.
template <typename T>
__global__ __launch_bounds__(NT) void k_auc_ovr_rows(const T* __restrict__ scores, const long long* __restrict__ gt, int N, int C, int L,
                                                    int* __restrict__ lbl, long long* pos_c, long long* flags3) {
    const int sub = threadIdx.x & (L - 1);
    const int row = blockIdx.x * (NT / L) + threadIdx.x / L;
    T best;
    int nan;
    double sum;
    scan_row(scores, row, N, C, L, sub, best, nan, sum);
    if (row >= N || sub != 0) return;
    const long long y = gt[row];
    const bool valid = y >= 0 && y < C;
    lbl[row] = valid ? (int)y : -1;
    if (valid) atomicAdd((unsigned long long*)&pos_c[y], 1ull);
    else atomicAdd((unsigned long long*)&flags3[0], 1ull);
    if (nan) atomicAdd((unsigned long long*)&flags3[1], 1ull);
    if (!(fabs(sum - 1.0) <= 1e-8 + 1e-5)) atomicAdd((unsigned long long*)&flags3[2], 1ull);
}

// Workgroup (x, y): rows i of tile x against the j rows [y * chunk, (y + 1) * chunk), staged `rows` at a time as a contiguous
// [rows][C] slice of the score matrix. Dynamic LDS: the tile, its labels, then two 32-bit counters per class that collect the
// workgroup's counts before one 64-bit atomic per class touched.
template <typename T>
__global__ __launch_bounds__(NT) void k_auc_ovr_pairs(const T* __restrict__ scores, const int* __restrict__ lbl, int N, int C, int rows,
                                                     int chunk, long long* gt_c, long long* eq_c) {
    extern __shared__ __align__(16) unsigned char smem[];
    T* tile = (T*)smem;
    int* sl = (int*)(tile + (size_t)rows * C);
    unsigned* ag = (unsigned*)(sl + rows);
    unsigned* ae = ag + C;
    const int i = blockIdx.x * NT + threadIdx.x;
    const int ci_raw = i < N ? lbl[i] : -1;
    const bool act = ci_raw >= 0;
    const int ci = act ? ci_raw : 0;
    const T v = act ? scores[(size_t)i * C + ci] : (T)NAN;     // NaN: every comparison below is false
    for (int c = threadIdx.x; c < C; c += NT) { ag[c] = 0; ae[c] = 0; }
    const long long jlo = (long long)blockIdx.y * chunk;
    const int jhi = (int)(jlo + chunk < N ? jlo + chunk : N);
    unsigned g = 0, e = 0;
    for (int j0 = (int)jlo; j0 < jhi; j0 += rows) {
        const int rj = jhi - j0 < rows ? jhi - j0 : rows;
        const int n = rj * C;
        const T* src = scores + (size_t)j0 * C;
        for (int x = threadIdx.x; x < n; x += NT) tile[x] = src[x];
        if ((int)threadIdx.x < rj) sl[threadIdx.x] = lbl[j0 + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < rj; ++k) {
            const T x = tile[k * C + ci];
            const bool other = sl[k] != ci_raw;               // an inactive thread never counts: its v is NaN
            g += (other && v > x) ? 1u : 0u;
            e += (other && v == x) ? 1u : 0u;
        }
        __syncthreads();
    }
    if (g) atomicAdd(&ag[ci], g);
    if (e) atomicAdd(&ae[ci], e);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
        if (ag[c]) atomicAdd((unsigned long long*)&gt_c[c], (unsigned long long)ag[c]);
        if (ae[c]) atomicAdd((unsigned long long*)&eq_c[c], (unsigned long long)ae[c]);
    }
}

template <typename T>
int auc_ovr_impl(const T* scores, const long long* gt, int N, int C, void* ws, size_t ws_bytes, long long* gt_c, long long* eq_c,
                 long long* pos_c, long long* flags3, osi_stream_t stream) {
    OSI_REQUIRE(scores && gt && ws && gt_c && eq_c && pos_c && flags3 && N > 0 && C > 0 && N <= INT_MAX - NT);
    OSI_REQUIRE(ws_bytes >= osi_auc_workspace(N));
    OSI_REQUIRE(C <= OVR_MAX_C);                           // a wider row does not fit the LDS tiling: refused before any launch
    hipStream_t st = (hipStream_t)stream;
    int* lbl = (int*)ws;
    if (hipMemsetAsync(gt_c, 0, (size_t)C * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(eq_c, 0, (size_t)C * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(pos_c, 0, (size_t)C * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(flags3, 0, 3 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    const int L = row_lanes(C);
    hipLaunchKernelGGL(k_auc_ovr_rows<T>, dim3(osi_cdiv(N, NT / L)), dim3(NT), 0, st, scores, gt, N, C, L, lbl, pos_c, flags3);
    OSI_LAUNCH_CHECK();
    int rows = OVR_TILE_BYTES / (C * (int)sizeof(T));      // >= 2 for C <= OVR_MAX_C
    if (rows > NT) rows = NT;                              // one thread loads one label of the tile
    // j chunks: at least 1024 rows each (the staging has to amortise), enough of them to reach OVR_BLOCKS workgroups, never longer
    // than the 32-bit class counters of a workgroup allow
    const int gx = osi_cdiv(N, NT);
    int gy = OVR_BLOCKS / gx;
    if (gy > osi_cdiv(N, 1024)) gy = osi_cdiv(N, 1024);
    if (gy < osi_cdiv(N, OVR_MAX_CHUNK)) gy = osi_cdiv(N, OVR_MAX_CHUNK);
    if (gy < 1) gy = 1;
    const int chunk = osi_cdiv(N, gy);
    gy = osi_cdiv(N, chunk);
    const size_t lds = (size_t)rows * C * sizeof(T) + (size_t)rows * sizeof(int) + 2 * (size_t)C * sizeof(unsigned);
    hipLaunchKernelGGL(k_auc_ovr_pairs<T>, dim3(gx, gy), dim3(NT), lds, st, scores, (const int*)lbl, N, C, rows, chunk, gt_c, eq_c);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // namespace

extern "C" {

size_t osi_auc_workspace(int N) { return N > 0 ? (size_t)N * 8 + 64 : 0; }

int osi_auc_binary_f32(const float* scores, const long long* gt, int N, int C, long long unk_class, void* ws, size_t ws_bytes,
                       long long* counts5, osi_stream_t stream) {
    return auc_binary_impl<float>(scores, gt, N, C, unk_class, ws, ws_bytes, counts5, stream);
}
int osi_auc_binary_f64(const double* scores, const long long* gt, int N, int C, long long unk_class, void* ws, size_t ws_bytes,
                       long long* counts5, osi_stream_t stream) {
    return auc_binary_impl<double>(scores, gt, N, C, unk_class, ws, ws_bytes, counts5, stream);
}
int osi_auc_ovr_f32(const float* scores, const long long* gt, int N, int C, void* ws, size_t ws_bytes, long long* gt_c,
                    long long* eq_c, long long* pos_c, long long* flags3, osi_stream_t stream) {
    return auc_ovr_impl<float>(scores, gt, N, C, ws, ws_bytes, gt_c, eq_c, pos_c, flags3, stream);
}
int osi_auc_ovr_f64(const double* scores, const long long* gt, int N, int C, void* ws, size_t ws_bytes, long long* gt_c,
                    long long* eq_c, long long* pos_c, long long* flags3, osi_stream_t stream) {
    return auc_ovr_impl<double>(scores, gt, N, C, ws, ws_bytes, gt_c, eq_c, pos_c, flags3, stream);
}

}  // extern "C"
