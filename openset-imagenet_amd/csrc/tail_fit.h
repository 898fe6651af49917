// The Weibull tail fit shared by OpenMax (openmax.hip: one workgroup per class) and the Extreme Value Machine (evm.hip: one workgroup
// per row): select the T largest of a workgroup's candidates with a four-pass radix select over order-preserving 32-bit keys, sort
// them in LDS (bitonic), and solve the Weibull likelihood equation by Newton steps kept inside a bracket. The sums run over the SORTED
// tail in a fixed tree, so the fit depends on the multiset of the candidates only. include/osi.h (osi_openmax_fit_tails) is the
// definition; the two callers differ only in how a workgroup enumerates its candidates.
#pragma once
#include "osi_common.h"

#include <math.h>

namespace osi_tail {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_TAIL = 4096;
constexpr int EXPAND_MAX = 1100;            // bracket doublings / halvings: more than the exponent range of fp64
constexpr int SOLVE_MAX = 128;              // Newton / bisection steps inside a bracket of one binade (53 bisections exhaust it)
static_assert(MAX_TAIL == OSI_OPENMAX_MAX_TAIL && MAX_TAIL == OSI_EVM_MAX_TAIL, "one tail capacity");

// order-preserving key of a finite float (larger value = larger unsigned key) and back
__device__ __forceinline__ unsigned fkey(float d) {
    const unsigned b = __float_as_uint(d);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float funkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct Shared {                             // 49 KB of LDS, one per workgroup
    double lnx[MAX_TAIL];
    double red[3][NW];
    unsigned keys[MAX_TAIL];
    unsigned hist[256];
    unsigned prefix, rem, K, cursor, bad;
};

struct Result {                             // the same bits in every thread
    double shape, scale, shift;
    bool fit;
    int K;                                  // tail length
    unsigned bad;                           // candidates left out by the enumerator
};

struct FitSums {
    double s0, s1, s2;      // sum e, sum e l, sum e l^2 with e = exp(k (l - lmax))
};

// Fixed tree: per thread in index order of its strided elements, xor butterfly in the wave, the waves in order. Every thread
// returns the same bits, so the solver's branches are uniform.
__device__ __forceinline__ FitSums fit_sums(const double* __restrict__ lnx, int K, double k, double lmax, double (*red)[NW]) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int t = threadIdx.x; t < K; t += NT) {
        const double l = lnx[t], e = exp(k * (l - lmax));
        s0 += e;
        s1 += e * l;
        s2 += e * l * l;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    __syncthreads();                                        // the previous call's readers are done with red
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = s0; red[1][w] = s1; red[2][w] = s2;
    }
    __syncthreads();
    FitSums r = {red[0][0], red[1][0], red[2][0]};
#pragma unroll
    for (int w = 1; w < NW; ++w) { r.s0 += red[0][w]; r.s1 += red[1][w]; r.s2 += red[2][w]; }
    return r;
}

// cand(i, key) for 0 <= i < N: 1 = element i is a candidate and `key` its fkey, 2 = a candidate left out (counted in Result::bad),
// 0 = no candidate. It must answer the same every time it is asked. Called by all NT threads of the workgroup.
template <class Cand>
__device__ __forceinline__ Result tail_fit(Shared& sm, long long N, int T, Cand cand) {
    const int tid = threadIdx.x;
    if (tid == 0) { sm.prefix = 0; sm.rem = 0; sm.K = 0; sm.cursor = 0; sm.bad = 0; }

    // radix select of the K-th largest key, most significant byte first; the first pass also counts the candidates
    unsigned mask = 0;
    for (int p = 0; p < 4; ++p) {
        const int sh = 24 - 8 * p;
        sm.hist[tid] = 0;                                   // NT == 256 bins
        __syncthreads();
        const unsigned prefix = sm.prefix;
        unsigned bad = 0;
        for (long long i = tid; i < N; i += NT) {
            unsigned k;
            const int what = cand(i, k);
            if (what == 1) {
                if ((k & mask) == prefix) atomicAdd(&sm.hist[(k >> sh) & 255u], 1u);
            } else if (p == 0 && what == 2) {
                ++bad;
            }
        }
        if (p == 0 && bad) atomicAdd(&sm.bad, bad);
        __syncthreads();
        if (tid == 0) {
            unsigned rem = sm.rem;
            if (p == 0) {
                unsigned n = 0;
                for (int d = 0; d < 256; ++d) n += sm.hist[d];
                rem = n < (unsigned)T ? n : (unsigned)T;
                sm.K = rem;
            }
            if (rem) {
                int d = 255;
                for (; d > 0; --d) {
                    if (sm.hist[d] >= rem) break;
                    rem -= sm.hist[d];
                }
                sm.prefix = prefix | ((unsigned)d << sh);
            }
            sm.rem = rem;                                   // copies of the digit's keys still to take
        }
        mask |= 255u << sh;
        __syncthreads();
    }
    unsigned* keys = sm.keys;
    double* lnx = sm.lnx;
    const int K = (int)sm.K;
    const unsigned thr = sm.prefix;
    const int n_thr = (int)sm.rem, n_gt = K - n_thr;        // the tail: every key above thr, and n_thr copies of thr
    bool fit = K >= 2;
    if (fit) {
        for (long long i = tid; i < N; i += NT) {
            unsigned k;
            if (cand(i, k) == 1) {
                if (k > thr) {
                    const unsigned pos = atomicAdd(&sm.cursor, 1u);
                    if (pos < (unsigned)n_gt) keys[pos] = k;    // always true: n_gt was counted from the same keys
                }
            }
        }
        int P = 2;
        while (P < K) P <<= 1;                              // <= 4096
        __syncthreads();
        for (int t = n_gt + tid; t < P; t += NT) keys[t] = t < K ? thr : 0xffffffffu;
        __syncthreads();
        for (int k2 = 2; k2 <= P; k2 <<= 1)                 // bitonic sort, ascending; the padding ends up behind the tail
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P; t += NT) {
                    const int u = t ^ j;
                    if (u > t) {
                        const unsigned a = keys[t], b = keys[u];
                        if ((a > b) == ((t & k2) == 0)) { keys[t] = b; keys[u] = a; }
                    }
                }
                __syncthreads();
            }
        // equal ends, in fp32 or after the translation to x = d - shift + 1 in fp64 (distances below 2^-53): nothing to fit
        fit = keys[0] != keys[K - 1] && (double)funkey(keys[K - 1]) - (double)funkey(keys[0]) + 1.0 > 1.0;
    }
    double k_out = 0.0, lam_out = 0.0, shift_out = 0.0;
    if (fit) {                                              // uniform: keys[] is shared
        const float dmin = funkey(keys[0]);
        for (int t = tid; t < K; t += NT) lnx[t] = log((double)funkey(keys[t]) - (double)dmin + 1.0);
        __syncthreads();
        const double xmax = (double)funkey(keys[K - 1]) - (double)dmin + 1.0;
        const double lmax = lnx[K - 1];
        double ls = 0.0;
        for (int t = tid; t < K; t += NT) ls += lnx[t];
        ls = wave_sum(ls);
        if ((tid & 63) == 0) sm.red[0][tid >> 6] = ls;
        __syncthreads();
        double lmean = sm.red[0][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) lmean += sm.red[0][w];
        lmean /= (double)K;
        // g(k) = s1 / s0 - 1 / k - lmean, increasing; g < 0 near 0 and g -> lmax - lmean > 0
        auto g_of = [&](double k, double& dg) {
            const FitSums s = fit_sums(lnx, K, k, lmax, sm.red);
            const double m1 = s.s1 / s.s0;
            dg = s.s2 / s.s0 - m1 * m1 + 1.0 / (k * k);
            return m1 - 1.0 / k - lmean;
        };
        double lo = 1.0, hi = 1.0, dg;
        double g = g_of(1.0, dg);
        if (g < 0.0) {
            for (int it = 0; it < EXPAND_MAX && g < 0.0; ++it) { lo = hi; hi *= 2.0; g = g_of(hi, dg); }
        } else {
            for (int it = 0; it < EXPAND_MAX && g >= 0.0; ++it) { hi = lo; lo *= 0.5; g = g_of(lo, dg); }
        }
        double k = 0.5 * (lo + hi);
        for (int it = 0; it < SOLVE_MAX; ++it) {
            g = g_of(k, dg);
            if (g == 0.0) break;
            if (g < 0.0) lo = k; else hi = k;
            double kn = k - g / dg;
            if (!(kn > lo && kn < hi)) kn = 0.5 * (lo + hi);
            const double step = fabs(kn - k);
            k = kn;
            if (step <= 4.0e-16 * kn || !(hi > lo)) break;
        }
        const FitSums s = fit_sums(lnx, K, k, lmax, sm.red);
        k_out = k;
        lam_out = xmax * exp(log(s.s0 / (double)K) / k);
        shift_out = (double)dmin;
    }
    return Result{k_out, lam_out, shift_out, fit, K, sm.bad};
}

}  // namespace osi_tail
