// Detection metrics and the OSCR curve by rejection score on the GPU: what metrics.detection_metrics and util.oscr_by_rejection count.
//
// Every post-hoc detector of this package leaves one value per sample, u[N], higher = more unknown. The figures its papers report
// (AUROC, AUPR-in, AUPR-out, FPR at a TPR) and the OSCR curve with u as the rejector are all functions of six integers per row: how
// many known / unknown / correctly classified rows lie strictly below and at-or-below that row's value. One all-pairs pass counts
// them (the idiom of auc.hip and oscr.hip: VALU comparisons over LDS-staged tiles, integer partial counts, no sort, no float
// accumulation, order-free by construction); everything after it is O(N) or a selection over the known rows:
//
//   osi_det_ranks_*   ranks[6][N] = kn_lt, kn_le, unk_lt, unk_le, cor_lt, cor_le and counts = {K, U, Kc, NaN rows}
//   osi_det_summary   Mann-Whitney pair counts, the two average-precision sums (fp64, fixed order), FPR counts at TPR levels
//   osi_det_curve_*   the distinct values of the known rows in descending order with cor_lt / unk_lt of each: the OSCR curve
//
// A row whose value is NaN belongs to no population: its side word is 0, every comparison with it is false, its ranks are 0.
#include "osi_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int PAIR_BLOCKS = 2048;    // workgroups the all-pairs launch aims for (8 per CU)
constexpr int DET_MAX_Q = 8;
// side word of a row: one bit per population, 10 bits apart, so that one 32-bit add per comparison counts all three populations of a
// 256-row tile at once (a field reaches 256 at the most); the fields are unpacked into 32-bit registers after every tile
constexpr unsigned S_KNOWN = 1u, S_UNK = 1u << 10, S_CORRECT = 1u << 20, S_FIELD = 1023u;

// layout of the summary's workspace: two 64-bit population counts, DET_MAX_Q 32-bit minima, then two fp64 partials per workgroup
constexpr size_t SUM_HDR = 64;

template <typename T>
__device__ __forceinline__ unsigned side_of(T v, long long y, long long unk_label, const unsigned char* correct, int i) {
    if (v != v) return 0u;
    if (y >= 0) return S_KNOWN | ((correct && correct[i]) ? S_CORRECT : 0u);
    return y == unk_label ? S_UNK : 0u;
}

__device__ __forceinline__ void count_lanes(bool flag, long long* slot) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == 0) atomicAdd((unsigned long long*)slot, (unsigned long long)__popcll(m));
}

// -------------------------------------------------------------------------------------------------------------------- ranks
template <typename T>
__global__ __launch_bounds__(NT) void k_det_rows(const T* __restrict__ u, const long long* __restrict__ gt,
                                                const unsigned char* __restrict__ correct, int N, long long unk_label,
                                                unsigned* __restrict__ side, long long* counts) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool in = i < N;
    const T v = in ? u[i] : T(0);
    const unsigned s = in ? side_of(v, gt[i], unk_label, correct, i) : 0u;
    if (in) side[i] = s;
    count_lanes(s & S_KNOWN, &counts[0]);
    count_lanes(s & S_UNK, &counts[1]);
    count_lanes(s & S_CORRECT, &counts[2]);
    count_lanes(in && v != v, &counts[3]);
}

// Workgroup (x, y): rows i of tile x against the j rows [y * chunk, (y + 1) * chunk), chunk a multiple of NT. Slots past N hold a NaN
// and an empty side word, so the inner loop has a fixed length and no bound check. The j range is split over gridDim.y workgroups:
// 32-bit integer atomics merge their counts into the zeroed ranks array, in any order with the same result.
template <typename T>
__global__ __launch_bounds__(NT) void k_det_pairs(const T* __restrict__ u, const unsigned* __restrict__ side, int N, int chunk,
                                                 int* ranks) {
    __shared__ T sv[NT];
    __shared__ unsigned ss[NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    const T none = (T)NAN;
    const T v = i < N ? u[i] : none;
    const long long jlo = (long long)blockIdx.y * chunk;
    const long long jhi = jlo + chunk < N ? jlo + chunk : N;
    unsigned c[6] = {0, 0, 0, 0, 0, 0};
    for (long long j0 = jlo; j0 < jhi; j0 += NT) {
        const long long j = j0 + threadIdx.x;
        sv[threadIdx.x] = j < jhi ? u[j] : none;
        ss[threadIdx.x] = j < jhi ? side[j] : 0u;
        __syncthreads();
        unsigned lt = 0, le = 0;
#pragma unroll 8
        for (int k = 0; k < NT; ++k) {
            const T x = sv[k];
            const unsigned s = ss[k];
            lt += x < v ? s : 0u;
            le += x <= v ? s : 0u;
        }
        __syncthreads();
        c[0] += lt & S_FIELD; c[2] += (lt >> 10) & S_FIELD; c[4] += lt >> 20;
        c[1] += le & S_FIELD; c[3] += (le >> 10) & S_FIELD; c[5] += le >> 20;
    }
    if (i < N) {
#pragma unroll
        for (int r = 0; r < 6; ++r)
            if (c[r]) atomicAdd(&ranks[(size_t)r * N + i], (int)c[r]);
    }
}

template <typename T>
int det_ranks_impl(const T* u, const long long* gt, const unsigned char* correct, int N, long long unk_label, void* ws,
                   size_t ws_bytes, int* ranks, long long* counts4, osi_stream_t stream) {
    OSI_REQUIRE(u && gt && ws && ranks && counts4 && N > 0 && N <= INT_MAX - NT && unk_label < 0);
    OSI_REQUIRE(ws_bytes >= osi_det_workspace(N));
    hipStream_t st = (hipStream_t)stream;
    unsigned* side = (unsigned*)ws;
    if (hipMemsetAsync(counts4, 0, 4 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(ranks, 0, (size_t)6 * N * sizeof(int), st) != hipSuccess) return OSI_ERR_LAUNCH;
    const int tiles = osi_cdiv(N, NT);
    hipLaunchKernelGGL(k_det_rows<T>, dim3(tiles), dim3(NT), 0, st, u, gt, correct, N, unk_label, side, counts4);
    OSI_LAUNCH_CHECK();
    // j chunks of whole tiles, enough of them to reach PAIR_BLOCKS workgroups
    int gy = PAIR_BLOCKS / tiles;
    if (gy < 1) gy = 1;
    if (gy > tiles) gy = tiles;
    const int per = osi_cdiv(tiles, gy);
    gy = osi_cdiv(tiles, per);
    hipLaunchKernelGGL(k_det_pairs<T>, dim3(tiles, gy), dim3(NT), 0, st, u, (const unsigned*)side, N, per * NT, ranks);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

// ------------------------------------------------------------------------------------------------------------------ summary
// The summary reads no values: a row is a member of the known (unknown) population when its label says so and it is counted in its own
// kn_le (unk_le), which a NaN row is not.
__device__ __forceinline__ bool is_known(const int* ranks, const long long* gt, int N, int i) {
    return gt[i] >= 0 && ranks[(size_t)1 * N + i] > 0;
}
__device__ __forceinline__ bool is_unk(const int* ranks, const long long* gt, int N, long long unk_label, int i) {
    return gt[i] == unk_label && ranks[(size_t)3 * N + i] > 0;
}

__global__ __launch_bounds__(NT) void k_det_sum_count(const int* __restrict__ ranks, const long long* __restrict__ gt, int N,
                                                     long long unk_label, long long* ku, int* fmin) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < DET_MAX_Q) fmin[threadIdx.x] = INT_MAX;
    count_lanes(i < N && is_known(ranks, gt, N, i), &ku[0]);
    count_lanes(i < N && is_unk(ranks, gt, N, unk_label, i), &ku[1]);
}

// fixed-order sum of one fp64 per thread over the workgroup: xor butterfly inside a wave, the four waves in index order
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < NT / 64; ++w) s += red[w];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(NT) void k_det_sum_terms(const int* __restrict__ ranks, const long long* __restrict__ gt, int N,
                                                     long long unk_label, const double* __restrict__ q, int Q,
                                                     const long long* __restrict__ ku, int* fmin, double* __restrict__ partials,
                                                     long long* ints) {
    __shared__ double red[NT / 64];
    const int i = blockIdx.x * NT + threadIdx.x;
    const long long K = ku[0], U = ku[1];
    const bool kn = i < N && is_known(ranks, gt, N, i);
    const bool un = i < N && is_unk(ranks, gt, N, unk_label, i);
    long long kn_lt = 0, kn_le = 0, unk_lt = 0, unk_le = 0;
    if (kn || un) {
        kn_lt = ranks[i]; kn_le = ranks[(size_t)1 * N + i]; unk_lt = ranks[(size_t)2 * N + i]; unk_le = ranks[(size_t)3 * N + i];
    }
    // every denominator below is at least 1: a member is counted in its own at-or-below count
    const double a_in = kn ? (double)kn_le / (double)(kn_le + unk_le) : 0.0;
    const double a_out = un ? (double)(U - unk_lt) / (double)((U - unk_lt) + (K - kn_lt)) : 0.0;
    const double s_in = block_sum(a_in, red);
    const double s_out = block_sum(a_out, red);
    if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = s_in; partials[2 * (size_t)blockIdx.x + 1] = s_out; }
    unsigned long long g = un ? (unsigned long long)kn_lt : 0ull, e = un ? (unsigned long long)(kn_le - kn_lt) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { g += __shfl_xor(g, o, 64); e += __shfl_xor(e, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (g) atomicAdd((unsigned long long*)&ints[0], g);
        if (e) atomicAdd((unsigned long long*)&ints[1], e);
    }
    for (int t = 0; t < Q; ++t) {
        int cand = (kn && (double)kn_le / (double)K >= q[t]) ? (int)unk_le : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(cand, o, 64); cand = other < cand ? other : cand; }
        if ((threadIdx.x & 63) == 0 && cand != INT_MAX) atomicMin(&fmin[t], cand);
    }
}

// one workgroup: the per-workgroup partials in a fixed order (thread t takes t, t + NT, ..., then block_sum), the minima as int64.
// No known row reaches a level only when there is no known row; the count is then U (every unknown row passes).
__global__ __launch_bounds__(NT) void k_det_sum_final(const double* __restrict__ partials, int nb, int Q, const long long* __restrict__ ku,
                                                     const int* __restrict__ fmin, long long* ints, double* sums) {
    __shared__ double red[NT / 64];
    double a = 0.0, b = 0.0;
    for (int p = threadIdx.x; p < nb; p += NT) { a += partials[2 * (size_t)p]; b += partials[2 * (size_t)p + 1]; }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) { sums[0] = a; sums[1] = b; }
    if ((int)threadIdx.x < Q) ints[2 + threadIdx.x] = fmin[threadIdx.x] == INT_MAX ? ku[1] : (long long)fmin[threadIdx.x];
}

// -------------------------------------------------------------------------------------------------------------------- curve
// val[i] = u[i] on the known rows, NaN elsewhere (also on a known row whose value is NaN); totals[1], totals[2] = K, U
template <typename T>
__global__ __launch_bounds__(NT) void k_det_curve_rows(const T* __restrict__ u, const long long* __restrict__ gt, int N,
                                                      long long unk_label, T* __restrict__ val, long long* totals) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool in = i < N;
    const T v = in ? u[i] : (T)NAN;
    const long long y = in ? gt[i] : 0;
    const bool kn = in && v == v && y >= 0;
    if (in) val[i] = kn ? v : (T)NAN;
    count_lanes(kn, &totals[1]);
    count_lanes(in && v == v && y == unk_label, &totals[2]);
}

// first[i] = val[i] where no earlier known row holds an equal value (np.unique keeps one of each), NaN elsewhere; totals[0] = #distinct
template <typename T>
__global__ __launch_bounds__(NT) void k_det_curve_first(const T* __restrict__ val, int N, T* __restrict__ first, long long* totals) {
    __shared__ T sv[NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    const T none = (T)NAN;
    const T v = i < N ? val[i] : none;
    bool dup = false;
    // only j < i matters: the tiles up to this workgroup's own; slots past N hold a NaN, which equals nothing
    for (int j0 = 0; j0 <= (int)blockIdx.x * NT; j0 += NT) {
        const int j = j0 + threadIdx.x;
        sv[threadIdx.x] = j < N ? val[j] : none;
        __syncthreads();
        const int lim = i - j0 < NT ? i - j0 : NT;
        for (int k = 0; k < lim; ++k) dup |= sv[k] == v;
        __syncthreads();
    }
    const bool lead = v == v && !dup;
    if (i < N) first[i] = lead ? v : none;
    count_lanes(lead, &totals[0]);
}

// position of a distinct value = number of distinct values above it: thresholds in descending order, with the counts of their row
template <typename T>
__global__ __launch_bounds__(NT) void k_det_curve_rank(const T* __restrict__ first, const int* __restrict__ ranks, int N,
                                                      T* __restrict__ taus, long long* __restrict__ ccr_count,
                                                      long long* __restrict__ fpr_count) {
    __shared__ T sv[NT];
    const int i = blockIdx.x * NT + threadIdx.x;
    const T none = (T)NAN;
    const T v = i < N ? first[i] : none;
    int pos = 0;
    for (int j0 = 0; j0 < N; j0 += NT) {
        const int j = j0 + threadIdx.x;
        sv[threadIdx.x] = j < N ? first[j] : none;
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < NT; ++k) pos += sv[k] > v ? 1 : 0;
        __syncthreads();
    }
    if (v == v) {                                  // pos < #distinct <= N
        taus[pos] = v;
        ccr_count[pos] = ranks[(size_t)4 * N + i];
        fpr_count[pos] = ranks[(size_t)2 * N + i];
    }
}

template <typename T>
int det_curve_impl(const T* u, const long long* gt, const int* ranks, int N, long long unk_label, void* ws, size_t ws_bytes, T* taus,
                   long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream) {
    OSI_REQUIRE(u && gt && ranks && ws && taus && ccr_count && fpr_count && totals && N > 0 && N <= INT_MAX - NT && unk_label < 0);
    OSI_REQUIRE(ws_bytes >= osi_det_workspace(N));
    hipStream_t st = (hipStream_t)stream;
    T* val = (T*)ws;                                   // both sized for double
    T* first = (T*)((char*)ws + (size_t)N * 8);
    if (hipMemsetAsync(totals, 0, 3 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(taus, 0, (size_t)N * sizeof(T), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(ccr_count, 0, (size_t)N * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(fpr_count, 0, (size_t)N * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    const int grid = osi_cdiv(N, NT);
    hipLaunchKernelGGL(k_det_curve_rows<T>, dim3(grid), dim3(NT), 0, st, u, gt, N, unk_label, val, totals);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_det_curve_first<T>, dim3(grid), dim3(NT), 0, st, (const T*)val, N, first, totals);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_det_curve_rank<T>, dim3(grid), dim3(NT), 0, st, (const T*)first, ranks, N, taus, ccr_count, fpr_count);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // namespace

extern "C" {

// the largest need of the three calls: two fp64 arrays of the curve (the side words of the ranks and the summary's header and
// partials fit inside them)
size_t osi_det_workspace(int N) { return N > 0 && N <= INT_MAX - NT ? (size_t)N * 16 + 256 : 0; }

int osi_det_ranks_f32(const float* u, const long long* gt, const unsigned char* correct, int N, long long unk_label, void* ws,
                      size_t ws_bytes, int* ranks, long long* counts4, osi_stream_t stream) {
    return det_ranks_impl<float>(u, gt, correct, N, unk_label, ws, ws_bytes, ranks, counts4, stream);
}
int osi_det_ranks_f64(const double* u, const long long* gt, const unsigned char* correct, int N, long long unk_label, void* ws,
                      size_t ws_bytes, int* ranks, long long* counts4, osi_stream_t stream) {
    return det_ranks_impl<double>(u, gt, correct, N, unk_label, ws, ws_bytes, ranks, counts4, stream);
}

int osi_det_summary(const int* ranks, const long long* gt, int N, long long unk_label, const double* q, int Q, void* ws,
                    size_t ws_bytes, long long* ints, double* sums, osi_stream_t stream) {
    OSI_REQUIRE(ranks && gt && q && ws && ints && sums && N > 0 && N <= INT_MAX - NT && unk_label < 0 && Q >= 1 && Q <= DET_MAX_Q);
    OSI_REQUIRE(ws_bytes >= osi_det_workspace(N));
    hipStream_t st = (hipStream_t)stream;
    long long* ku = (long long*)ws;
    int* fmin = (int*)((char*)ws + 16);
    double* partials = (double*)((char*)ws + SUM_HDR);
    const int nb = osi_cdiv(N, NT);                    // SUM_HDR + 16 * nb <= osi_det_workspace(N)
    if (hipMemsetAsync(ws, 0, SUM_HDR, st) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipMemsetAsync(ints, 0, (size_t)(2 + Q) * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    hipLaunchKernelGGL(k_det_sum_count, dim3(nb), dim3(NT), 0, st, ranks, gt, N, unk_label, ku, fmin);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_det_sum_terms, dim3(nb), dim3(NT), 0, st, ranks, gt, N, unk_label, q, Q, (const long long*)ku, fmin, partials,
                       ints);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_det_sum_final, dim3(1), dim3(NT), 0, st, (const double*)partials, nb, Q, (const long long*)ku,
                       (const int*)fmin, ints, sums);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_det_curve_f32(const float* u, const long long* gt, const int* ranks, int N, long long unk_label, void* ws, size_t ws_bytes,
                      float* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream) {
    return det_curve_impl<float>(u, gt, ranks, N, unk_label, ws, ws_bytes, taus, ccr_count, fpr_count, totals, stream);
}
int osi_det_curve_f64(const double* u, const long long* gt, const int* ranks, int N, long long unk_label, void* ws, size_t ws_bytes,
                      double* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream) {
    return det_curve_impl<double>(u, gt, ranks, N, unk_label, ws, ws_bytes, taus, ccr_count, fpr_count, totals, stream);
}

}  // extern "C"
