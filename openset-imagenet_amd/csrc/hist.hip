// Evaluation histograms on the GPU: the counting behind util.get_histogram (reference openset_imagenet/util.py:202-228), i.e. the
// softmax-score histograms of plot_all.plot_softmax and the feature-norm histograms of the objectosphere plots.
//
// Two steps, both order-free (integer counts and min/max of stored values; no float accumulation across threads):
//   row values   per row the two compared values and a side byte: the known side takes scores[i][gt] (or the feature norm), the
//                unknown side the maximum over the class columns (or the same norm). The finite range of each side and five counters
//                come along, so that the host can form numpy's bin edges from {min, max} alone and raise numpy's errors.
//   histogram    np.histogram over an explicit, non-decreasing edge table: edges (fp64) and 32-bit counters live in LDS, every value
//                is placed by a binary search in fp64, equal bins are merged inside the wave before they touch an LDS word, and a
//                workgroup ends with one 64-bit integer add per counter that is not zero.
// The edges themselves are always made by numpy on the host (linspace roundings, the min == max widening, the empty-input [0, 1]).
#include "osi_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int VAL_MAX_BLOCKS = 1024;    // grid cap of the row pass = partials the finishing launch reads (4 doubles each)
constexpr int HIST_MAX_BLOCKS = 1024;
constexpr int PEEL_ROUNDS = 4;          // wave-level merges of equal bins before the lanes left over add on their own

// lanes that share one row of the score matrix: the largest power of two <= min(C, 64) (whole rows side by side in a wave)
inline int row_lanes(int C) {
    int l = 1;
    while (l * 2 <= C && l < 64) l *= 2;
    return l;
}

// ------------------------------------------------------------------------------------------------------------ row values
// L lanes per row (L = 1 for the norm: its fp64 sum runs in index order in one thread). Rows are walked grid-stride; every lane of a
// wave runs every shuffle. The workgroup leaves {kn_min, kn_max, unk_min, unk_max} in part[blockIdx.x] and adds its five counters.
template <typename T>
__global__ __launch_bounds__(NT) void k_eval_rows(const T* __restrict__ scores, const T* __restrict__ features,
                                                 const long long* __restrict__ gt, int N, int C, int F, int Cc, int metric, int L,
                                                 long long unk_label, T* __restrict__ kn_val, T* __restrict__ unk_val,
                                                 unsigned char* __restrict__ side, double* __restrict__ part, long long* counts6) {
    __shared__ double red_d[4][NT / 64];
    __shared__ unsigned red_u[5][NT / 64];
    const int sub = threadIdx.x & (L - 1);
    const int rows_per_block = NT / L;
    double mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    unsigned cnt[5] = {0, 0, 0, 0, 0};               // known, unknown, NaN among known, NaN among unknown, bad labels
    for (long long r0 = (long long)blockIdx.x * rows_per_block; r0 < N; r0 += (long long)gridDim.x * rows_per_block) {
        const long long row = r0 + threadIdx.x / L;
        const bool in = row < N;
        const long long y = in ? gt[row] : -1;
        T kv = 0, uv = 0;
        bool known = in && y >= 0;
        bool bad = false;
        if (metric == OSI_EVAL_NORM) {
            if (in) {
                const T* f = features + (size_t)row * F;
                double s = 0.0;
                for (int c = 0; c < F; ++c) {
                    const double d = (double)f[c];
                    s = __dadd_rn(s, __dmul_rn(d, d));      // the square is rounded before the add, also for fp64 inputs
                }
                kv = uv = (T)__dsqrt_rn(s);
            }
        } else {
            T best = (T)(-INFINITY);
            int nan = 0;
            if (in) {
                const T* r = scores + (size_t)row * C;
                for (int c = sub; c < Cc; c += L) {
                    const T v = r[c];
                    nan |= (v != v) ? 1 : 0;
                    best = v > best ? v : best;
                }
            }
            for (int o = L >> 1; o > 0; o >>= 1) {
                const T b = __shfl_xor(best, o, 64);
                best = b > best ? b : best;
                nan |= __shfl_xor(nan, o, 64);
            }
            uv = nan ? (T)NAN : best;                       // np.amax hands a NaN on
            bad = known && y >= Cc;                         // the reference raises IndexError there
            known = known && !bad;
            if (known) kv = scores[(size_t)row * C + y];
        }
        if (in && sub == 0) {
            const bool unk = y == unk_label;
            kn_val[row] = kv;
            unk_val[row] = uv;
            side[row] = (unsigned char)((known ? 1 : 0) | (unk ? 2 : 0));
            cnt[4] += bad ? 1u : 0u;
            if (known) {
                cnt[0] += 1u;
                const double d = (double)kv;
                if (d != d) cnt[2] += 1u;
                else { mn[0] = fmin(mn[0], d); mx[0] = fmax(mx[0], d); }
            }
            if (unk) {
                cnt[1] += 1u;
                const double d = (double)uv;
                if (d != d) cnt[3] += 1u;
                else { mn[1] = fmin(mn[1], d); mx[1] = fmax(mx[1], d); }
            }
        }
    }
    const int wave = threadIdx.x >> 6;
    const double v4[4] = {wave_fmin(mn[0]), wave_fmax(mx[0]), wave_fmin(mn[1]), wave_fmax(mx[1])};
    unsigned u5[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) u5[k] = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) red_d[k][wave] = v4[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) red_u[k][wave] = u5[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double o[4] = {red_d[0][0], red_d[1][0], red_d[2][0], red_d[3][0]};
        for (int w = 1; w < NT / 64; ++w) {
            o[0] = fmin(o[0], red_d[0][w]); o[1] = fmax(o[1], red_d[1][w]);
            o[2] = fmin(o[2], red_d[2][w]); o[3] = fmax(o[3], red_d[3][w]);
        }
        for (int k = 0; k < 4; ++k) part[(size_t)blockIdx.x * 4 + k] = o[k];
        for (int k = 0; k < 5; ++k) {
            unsigned long long s = 0;
            for (int w = 0; w < NT / 64; ++w) s += red_u[k][w];
            if (s) atomicAdd((unsigned long long*)&counts6[k], s);      // integer atomics: order-free
        }
    }
}

// one workgroup: min / max over the nparts partials of the row pass
__global__ __launch_bounds__(NT) void k_eval_range(const double* __restrict__ part, int nparts, double* __restrict__ range4) {
    __shared__ double red_d[4][NT / 64];
    double o[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int p = threadIdx.x; p < nparts; p += NT) {
        o[0] = fmin(o[0], part[(size_t)p * 4 + 0]); o[1] = fmax(o[1], part[(size_t)p * 4 + 1]);
        o[2] = fmin(o[2], part[(size_t)p * 4 + 2]); o[3] = fmax(o[3], part[(size_t)p * 4 + 3]);
    }
    o[0] = wave_fmin(o[0]); o[1] = wave_fmax(o[1]); o[2] = wave_fmin(o[2]); o[3] = wave_fmax(o[3]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) red_d[k][threadIdx.x >> 6] = o[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        double v = red_d[k][0];
        for (int w = 1; w < NT / 64; ++w) v = (k & 1) ? fmax(v, red_d[k][w]) : fmin(v, red_d[k][w]);
        range4[k] = v;
    }
}

inline int eval_blocks(int N, int L) {
    const int b = osi_cdiv(N, NT / L);
    return b < VAL_MAX_BLOCKS ? b : VAL_MAX_BLOCKS;
}

template <typename T>
int eval_values_impl(const T* scores, const T* features, const long long* gt, int N, int C, int F, int metric, long long unk_label,
                     int drop_last, T* kn_val, T* unk_val, unsigned char* side, double* range4, long long* counts6, void* ws,
                     size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(gt && kn_val && unk_val && side && range4 && counts6 && ws && N > 0 && N <= INT_MAX - NT);
    OSI_REQUIRE(metric == OSI_EVAL_SCORE || metric == OSI_EVAL_NORM);
    OSI_REQUIRE(drop_last == 0 || drop_last == 1);
    OSI_REQUIRE(ws_bytes >= osi_eval_values_workspace(N));
    if (metric == OSI_EVAL_SCORE) OSI_REQUIRE(scores && C - drop_last >= 1);   // np.amax over no column has no value
    else OSI_REQUIRE(features && F > 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts6, 0, 6 * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    const int Cc = C - drop_last;
    const int L = metric == OSI_EVAL_SCORE ? row_lanes(Cc) : 1;
    const int blocks = eval_blocks(N, L);
    double* part = (double*)ws;
    hipLaunchKernelGGL(k_eval_rows<T>, dim3(blocks), dim3(NT), 0, st, scores, features, gt, N, C, F, Cc, metric, L, unk_label, kn_val,
                       unk_val, side, part, counts6);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eval_range, dim3(1), dim3(NT), 0, st, (const double*)part, blocks, range4);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

// -------------------------------------------------------------------------------------------------------------- histogram
// Dynamic LDS: edges[nb + 1] as fp64, then nb 32-bit counters (at most 32 776 + 16 384 bytes).
//
// place(): every lane of the wave calls it, `on` says whether the lane holds a value. The bin is searchsorted(edges, x, 'right') - 1
// with x == edges[nb] moved into the last bin; both ends are clamped, so a table that is not sorted still indexes inside [0, nb).
// Equal bins are merged inside the wave: up to PEEL_ROUNDS times the first lane still holding a value names its bin, every lane with
// that bin leaves, and one lane adds their number. A whole wave in one bin is one LDS add; lanes left after the rounds (a wave
// spread over many bins) add 1 on their own, on distinct words except for whatever the rounds did not reach.
__device__ __forceinline__ void place(double x, bool on, const double* __restrict__ e, unsigned* __restrict__ cnt, int nb) {
    on = on && x >= e[0] && x <= e[nb];                     // NaN fails both
    int bin = -1;
    if (on) {
        int lo = 0, hi = nb + 1;                            // first index with e[index] > x, in [0, nb + 1]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;                 // <= nb
            if (e[mid] <= x) lo = mid + 1; else hi = mid;
        }
        bin = lo - 1;
        bin = bin > nb - 1 ? nb - 1 : bin;
        bin = bin < 0 ? 0 : bin;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long left = __ballot(on);
    for (int r = 0; r < PEEL_ROUNDS && left; ++r) {
        const int first = __ffsll((long long)left) - 1;
        const int b = __shfl(bin, first, 64);
        const unsigned long long same = __ballot(on && bin == b);
        if (lane == first) atomicAdd(&cnt[b], (unsigned)__popcll(same));
        on = on && bin != b;
        left &= ~same;
    }
    if (on) atomicAdd(&cnt[bin], 1u);
}

template <typename T>
__global__ __launch_bounds__(NT) void k_hist(const T* __restrict__ val, const unsigned char* __restrict__ side, int side_bit, int N,
                                            const double* __restrict__ edges, int nb, long long* counts) {
    extern __shared__ __align__(16) unsigned char smem[];
    double* e = (double*)smem;
    unsigned* cnt = (unsigned*)(e + nb + 1);
    constexpr int V = 16 / (int)sizeof(T);
    for (int k = threadIdx.x; k <= nb; k += NT) e[k] = edges[k];
    for (int k = threadIdx.x; k < nb; k += NT) cnt[k] = 0;
    __syncthreads();
    // [0, head): scalars up to the first 16-byte boundary of val; then nvec vectors; then the scalar tail
    const int mis = (int)(((uintptr_t)val & 15) / sizeof(T));
    int head = mis ? V - mis : 0;
    head = head < N ? head : N;
    const int nvec = (N - head) / V;
    const int tail0 = head + nvec * V;
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const vec_t* vv = (const vec_t*)(val + head);
    const long long stride = (long long)gridDim.x * NT;
    for (long long base = (long long)blockIdx.x * NT; base < nvec; base += stride) {    // uniform trip count inside a workgroup
        const long long i = base + threadIdx.x;
        const bool in = i < nvec;
        vec_t x;
        bool on[V];
        if (in) {
            x = vv[i];
            const unsigned char* s = side + head + i * V;
#pragma unroll
            for (int k = 0; k < V; ++k) on[k] = (s[k] & side_bit) != 0;
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) { x[k] = 0; on[k] = false; }
        }
#pragma unroll
        for (int k = 0; k < V; ++k) place((double)x[k], on[k], e, cnt, nb);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {              // head and tail: fewer than 2 V <= 8 scalars, one lane each
        const int n_extra = head + (N - tail0);
        const int t = threadIdx.x;
        const int i = t < head ? t : tail0 + (t - head);
        const bool in = t < n_extra;
        const double x = in ? (double)val[i] : 0.0;
        place(x, in && (side[in ? i : 0] & side_bit) != 0, e, cnt, nb);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nb; k += NT)
        if (cnt[k]) atomicAdd((unsigned long long*)&counts[k], (unsigned long long)cnt[k]);
}

template <typename T>
int hist_impl(const T* val, const unsigned char* side, int side_bit, int N, const double* edges, int nb, long long* counts,
              osi_stream_t stream) {
    OSI_REQUIRE(val && side && edges && counts && N > 0 && N <= INT_MAX - NT);
    OSI_REQUIRE(nb >= 1 && nb <= OSI_HIST_MAX_BINS);
    OSI_REQUIRE(side_bit > 0 && side_bit <= 255);
    OSI_REQUIRE(((uintptr_t)val % sizeof(T)) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)nb * sizeof(long long), st) != hipSuccess) return OSI_ERR_LAUNCH;
    // a workgroup stages the whole table and ends with up to nb adds: give it at least nb vectors, and four per thread
    constexpr int V = 16 / (int)sizeof(T);
    const int per_block = nb > 4 * NT ? nb : 4 * NT;
    int blocks = osi_cdiv(osi_cdiv(N, V), per_block);
    blocks = blocks < 1 ? 1 : (blocks > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : blocks);
    const size_t lds = (size_t)(nb + 1) * sizeof(double) + (size_t)nb * sizeof(unsigned);
    hipLaunchKernelGGL(k_hist<T>, dim3(blocks), dim3(NT), lds, st, val, side, side_bit, N, edges, nb, counts);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // namespace

extern "C" {

size_t osi_eval_values_workspace(int N) { return N > 0 ? (size_t)VAL_MAX_BLOCKS * 4 * sizeof(double) + 64 : 0; }

int osi_eval_values_f32(const float* scores, const float* features, const long long* gt, int N, int C, int F, int metric,
                        long long unk_label, int drop_last, float* kn_val, float* unk_val, unsigned char* side, double* range4,
                        long long* counts6, void* ws, size_t ws_bytes, osi_stream_t stream) {
    return eval_values_impl<float>(scores, features, gt, N, C, F, metric, unk_label, drop_last, kn_val, unk_val, side, range4, counts6,
                                   ws, ws_bytes, stream);
}
int osi_eval_values_f64(const double* scores, const double* features, const long long* gt, int N, int C, int F, int metric,
                        long long unk_label, int drop_last, double* kn_val, double* unk_val, unsigned char* side, double* range4,
                        long long* counts6, void* ws, size_t ws_bytes, osi_stream_t stream) {
    return eval_values_impl<double>(scores, features, gt, N, C, F, metric, unk_label, drop_last, kn_val, unk_val, side, range4, counts6,
                                    ws, ws_bytes, stream);
}
int osi_hist_f32(const float* val, const unsigned char* side, int side_bit, int N, const double* edges, int nb, long long* counts,
                 osi_stream_t stream) {
    return hist_impl<float>(val, side, side_bit, N, edges, nb, counts, stream);
}
int osi_hist_f64(const double* val, const unsigned char* side, int side_bit, int N, const double* edges, int nb, long long* counts,
                 osi_stream_t stream) {
    return hist_impl<double>(val, side, side_bit, N, edges, nb, counts, stream);
}

}  // extern "C"
