// Deep nearest neighbours (Sun, Ming, Zhu, Li, ICML 2022) on the GPU: ordered selection over the rows of a distance matrix that
// osi_evm_distances produced. include/osi.h (ABI 24) is the definition; openset_imagenet/knn.py is the user's face of it.
//
// Two kernels around ONE streaming select; a workgroup owns a unit (a row for topk, a row's class segment for class_kth):
//   stream   the segment is read from global memory once, in tiles of 2048 columns (eight coalesced 4-byte loads per thread, the next
//            tile's loads in flight while this one is handled). A column becomes the order-preserving 32-bit key of d + 0.0f (every NaN
//            the largest key); a column whose key is below the running threshold is a candidate and is appended to a buffer in LDS,
//            IN COLUMN ORDER: wave ballots give the position inside a wave's 64 columns, a 32-entry table of wave counts the rest.
//   shrink   when the buffer holds more than a limit (>= K), a four-pass radix select over the buffer (LDS only, integer histogram)
//            finds the K-th smallest key T and the number r of T-copies that belong to the K smallest; the buffer is compacted in place,
//            in order, to the keys below T and the FIRST r copies of T (the buffer is in column order, so these are the lowest columns),
//            and T becomes the threshold: a later column with key T has a higher index than all kept ones and cannot enter.
//   finish   topk: shrink to K, bitonic sort of (key, column) pairs in LDS, 4- and 8-byte stores. class_kth: one more select, one store.
// class_kth gives segments of up to 2048 columns to ONE WAVE each instead (k_knn_class_kth_wave: keys in registers, a bitwise select on
// wave ballots, no LDS and no barrier); the workgroup form above takes the longer ones. Both launches walk all units and pick their own.
// No floating-point arithmetic but d + 0.0f and the stored transform; no atomics on the tie path; unit choices depend on blockIdx only.
#include "tail_fit.h"                       // fkey / funkey

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int E = 8;                        // columns per thread and tile
constexpr int TILE = NT * E;                // 2048
constexpr int KEEP = 2048;                  // most buffer entries left behind by a tile's handling (>= OSI_KNN_MAX_K)
constexpr int CAP = KEEP + TILE;
constexpr int MAX_BLOCKS = 1 << 20;
constexpr unsigned NAN_KEY = 0xffffffffu;
static_assert(OSI_KNN_MAX_K <= KEEP && OSI_KNN_MAX_K <= 1024, "the sort stage holds 1024 pairs");
static_assert(E * NW <= 64, "one wave scans the table of wave counts");

// ascending order-preserving key (osi_tail::fkey, undone by osi_tail::funkey) of the canonical value:
// -Inf < ... < -0 = +0 < ... < +Inf < every NaN
__device__ __forceinline__ unsigned knn_key(float d) {
    const float v = __fadd_rn(d, 0.0f);     // -0 -> +0
    return v != v ? NAN_KEY : osi_tail::fkey(v);
}

struct Shared {
    __attribute__((aligned(16))) unsigned key[CAP];
    unsigned idx[CAP];
    unsigned hist[4][256];
    unsigned wc[2][64];
};

// Ordered append of one group of E * NT elements; element e of thread t is the (e * NT + t)-th of the group. what[e]: 0 = drop, 1 = keep,
// 2 = keep while fewer than r elements of kind 2 came before it (counted from `eq_seen` on). Kept elements go to base + (kept before).
// lt_seen / eq_seen: elements of kind 1 / 2 in the groups before this one; both are advanced. `par` alternates between groups.
// The caller's reads of this group (when it compacts in place) are complete before the barrier in here; writes follow it.
template <bool IDX>
__device__ __forceinline__ void append_group(Shared& sm, int par, const int (&what)[E], const unsigned (&key)[E], const unsigned (&idx)[E],
                                             int base, int r, int& lt_seen, int& eq_seen) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const unsigned long long b1 = __ballot(what[e] == 1), b2 = __ballot(what[e] == 2);
        if (lane == e) sm.wc[par][e * NW + wave] = (unsigned)__popcll(b1) | ((unsigned)__popcll(b2) << 16);
    }
    __syncthreads();
    // every wave scans the same E * NW packed counts (each half stays below 2^16: at most TILE elements)
    const unsigned own = lane < E * NW ? sm.wc[par][lane] : 0u;
    unsigned incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    const unsigned excl = incl - own;
    const unsigned total = __shfl(incl, 63, 64);
    if (total != 0u) {                                      // uniform
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const unsigned before = __shfl(excl, e * NW + wave, 64);
            const unsigned long long b1 = __ballot(what[e] == 1), b2 = __ballot(what[e] == 2);
            const int lt = lt_seen + (int)(before & 0xffffu) + __popcll(b1 & below);
            const int eq = eq_seen + (int)(before >> 16) + __popcll(b2 & below);
            if (what[e] == 1 || (what[e] == 2 && eq < r)) {
                const int pos = base + lt + (eq < r ? eq : r);
                sm.key[pos] = key[e];
                if (IDX) sm.idx[pos] = idx[e];
            }
        }
    }
    lt_seen += (int)(total & 0xffffu);
    eq_seen += (int)(total >> 16);
}

// The rank-th smallest (1 <= rank <= count) of key[0 .. count): four passes over the buffer, most significant byte first. Returns the
// key; `ties` = how many copies of it the `rank` smallest hold. Every thread returns the same values. Starts with a barrier between
// itself and the buffer's writers and the previous call's histogram readers; the buffer is only read.
__device__ __forceinline__ unsigned select_rank(Shared& sm, int count, int rank, int& ties) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();                                        // the buffer is written; the previous call's histograms are read
#pragma unroll
    for (int p = 0; p < 4; ++p) sm.hist[p][tid] = 0u;       // NT == 256 bins
    __syncthreads();
    unsigned prefix = 0u, mask = 0u, rem = (unsigned)rank;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int sh = 24 - 8 * p;
        for (int i = tid; i < count; i += NT) {
            const unsigned k = sm.key[i];
            if ((k & mask) == prefix) atomicAdd(&sm.hist[p][(k >> sh) & 255u], 1u);     // integer counts: order-free
        }
        __syncthreads();
        // every wave walks the 256 bins alike: lane l owns bins 4 l .. 4 l + 3
        const uint4 h = *reinterpret_cast<const uint4*>(&sm.hist[p][4 * lane]);
        const unsigned own = h.x + h.y + h.z + h.w;
        unsigned incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        const unsigned long long reach = __ballot(incl >= rem);     // never empty: the candidates number at least rem
        const int l = __ffsll((long long)reach) - 1;
        unsigned left = rem - (__shfl(incl, l, 64) - __shfl(own, l, 64));
        const unsigned hx = __shfl(h.x, l, 64), hy = __shfl(h.y, l, 64), hz = __shfl(h.z, l, 64);
        unsigned d = 4u * (unsigned)l;
        if (left > hx) { left -= hx; ++d;
            if (left > hy) { left -= hy; ++d;
                if (left > hz) { left -= hz; ++d; } } }
        prefix |= d << sh;
        mask |= 255u << sh;
        rem = left;
    }
    ties = (int)rem;
    return prefix;
}

// In-place ordered compaction of the buffer to its K smallest (count > K): keys below T, then-in buffer order-the first r copies of T.
template <bool IDX>
__device__ __forceinline__ void compact(Shared& sm, int count, unsigned T, int r) {
    int lt_seen = 0, eq_seen = 0, par = 0;
    for (int g0 = 0; g0 < count; g0 += TILE, par ^= 1) {
        int what[E];
        unsigned key[E], idx[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = g0 + e * NT + (int)threadIdx.x;
            what[e] = 0; key[e] = 0u; idx[e] = 0u;
            if (i < count) {
                key[e] = sm.key[i];
                if (IDX) idx[e] = sm.idx[i];
                what[e] = key[e] < T ? 1 : (key[e] == T ? 2 : 0);
            }
        }
        append_group<IDX>(sm, par, what, key, idx, 0, r, lt_seen, eq_seen);
    }
    __syncthreads();                                        // the caller's next group may take either half of the count table
}

__device__ __forceinline__ void load_tile(const float* __restrict__ row, long long c0, long long c1, float (&v)[E]) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const long long col = c0 + e * NT + (long long)threadIdx.x;
        v[e] = col < c1 ? row[col] : 0.f;
    }
}

// Streams the columns [c0, c1) of `row` but `skip` through the buffer. On return (no barrier after the last writes) the buffer holds
// `count` <= CAP entries in column order, among them the min(K, n) smallest of the segment by (key, column).
template <bool IDX>
__device__ __forceinline__ int stream_segment(Shared& sm, const float* __restrict__ row, long long c0, long long c1, long long skip, int K) {
    const int limit = K > 1024 - 32 ? KEEP : 2 * K + 64;    // K <= limit <= KEEP: a tighter threshold sooner for a small K
    int count = 0, par = 0;
    unsigned long long thr = 1ull << 32;                    // above every key: no threshold yet
    float cur[E], nxt[E] = {};
    load_tile(row, c0, c1, cur);
    for (long long t0 = c0; t0 < c1; t0 += TILE, par ^= 1) {
        if (t0 + TILE < c1) load_tile(row, t0 + TILE, c1, nxt);
        int what[E];
        unsigned key[E], idx[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const long long col = t0 + e * NT + (long long)threadIdx.x;
            key[e] = knn_key(cur[e]);
            idx[e] = (unsigned)col;
            what[e] = (col < c1 && col != skip && (unsigned long long)key[e] < thr) ? 1 : 0;
        }
        int added = 0, none = 0;
        append_group<IDX>(sm, par, what, key, idx, count, 0, added, none);
        count += added;                                     // <= KEEP + TILE = CAP
        if (count > limit && t0 + TILE < c1) {              // uniform; after the last tile the caller's own select does the work
            int r;
            const unsigned T = select_rank(sm, count, K, r);
            compact<IDX>(sm, count, T, r);
            count = K;
            thr = T;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) cur[e] = nxt[e];
    }
    return count;
}

// -------------------------------------------------------------------------------------------------------------------- topk
__global__ __launch_bounds__(NT) void k_knn_topk(const float* __restrict__ dist, int M, int N, long long ld, int K,
                                                const long long* __restrict__ skip, float* __restrict__ out_dist,
                                                long long* __restrict__ out_idx) {
    __shared__ Shared sm;
    unsigned long long* pairs = reinterpret_cast<unsigned long long*>(&sm.key[KEEP]);   // 1024 pairs behind the kept entries
    const int tid = threadIdx.x;
    for (int m = blockIdx.x; m < M; m += gridDim.x) {
        const float* row = dist + (size_t)m * (size_t)ld;
        const long long sk = skip ? skip[m] : -1;
        int count = stream_segment<true>(sm, row, 0, N, sk, K);
        if (count > K) {
            int r;
            const unsigned T = select_rank(sm, count, K, r);
            compact<true>(sm, count, T, r);
            count = K;
        }
        __syncthreads();
        int P = 2;
        while (P < count) P <<= 1;                          // <= 1024
        for (int t = tid; t < P; t += NT)
            pairs[t] = t < count ? ((unsigned long long)sm.key[t] << 32) | sm.idx[t] : ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= P; k2 <<= 1)                 // bitonic sort, ascending by (key, column); the padding ends up last
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < P; t += NT) {
                    const int u = t ^ j;
                    if (u > t) {
                        const unsigned long long a = pairs[t], b = pairs[u];
                        if ((a > b) == ((t & k2) == 0)) { pairs[t] = b; pairs[u] = a; }
                    }
                }
                __syncthreads();
            }
        for (int t = tid; t < K; t += NT) {
            const unsigned long long p = t < count ? pairs[t] : 0ull;
            out_dist[(size_t)m * K + t] = t < count ? osi_tail::funkey((unsigned)(p >> 32)) : INFINITY;
            out_idx[(size_t)m * K + t] = t < count ? (long long)(unsigned)p : -1ll;
        }
        __syncthreads();                                    // the next row rewrites the buffer
    }
}

// --------------------------------------------------------------------------------------------------------------- class_kth
__device__ __forceinline__ float knn_transform(float v, int transform) {
    if (transform == OSI_KNN_RAW) return v;
    if (v != v) return NAN;
    if (transform == OSI_KNN_SIM_COSINE) return fminf(fmaxf(__fsub_rn(1.0f, __fmul_rn(0.5f, v)), 0.0f), 1.0f);
    return __fdiv_rn(1.0f, __fadd_rn(1.0f, v));
}

// A segment of at most WAVE_MAX columns is one wave's work: its keys stay in registers (lane l holds the columns c0 + 64 e + l, in 1, 4,
// 8, 16 or 32 registers by the segment's length) and the rank-th smallest is found bit by bit from the top, each step a count of the
// still-matching keys whose bit is clear - wave ballots and scalar adds, no LDS, no barrier. Longer segments are left to k_knn_class_kth, which in turn leaves these alone.
constexpr int WE = 32;
constexpr int WAVE_MAX = 64 * WE;

struct Unit {
    long long m, c0, c1;
};
__device__ __forceinline__ Unit knn_unit(long long u, const long long* __restrict__ start, int C, int N) {
    Unit r;
    r.m = u / C;
    const int c = (int)(u - r.m * C);
    const long long a = start[c], b = start[c + 1];
    r.c0 = a < 0 ? 0 : (a > N ? N : a);
    r.c1 = b < 0 ? 0 : (b > N ? N : b);
    return r;
}

// The rank-th smallest key (1 <= rank <= columns taking part) of the columns [c0, c1) of `row` but `sk`, c1 - c0 <= 64 * NE, by one
// wave. A key that no longer matches the prefix - or never took part - is replaced by all ones, which no step counts: a step costs
// an AND, a compare and a select per register. The same value in every lane.
template <int NE>
__device__ __forceinline__ unsigned wave_select(const float* __restrict__ row, long long c0, long long c1, long long sk, unsigned rank) {
    const int lane = threadIdx.x & 63;
    float d[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {                          // every load is issued before the first key is built: a lane past the
        const long long col = c0 + e * 64 + lane;           // segment's end reads its last column again (c1 > c0 here)
        d[e] = row[col < c1 ? col : c1 - 1];
    }
    unsigned key[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const long long col = c0 + e * 64 + lane;
        key[e] = (col < c1 && col != sk) ? knn_key(d[e]) : NAN_KEY;
    }
    unsigned rem = __builtin_amdgcn_readfirstlane(rank), prefix = 0u;      // scalar: the loop's branches are scalar branches
#pragma unroll 1
    for (unsigned bit = 0x80000000u; bit != 0u; bit >>= 1) {
        bool clear[NE];
        unsigned zeros = 0u;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            clear[e] = (key[e] & bit) == 0u;
            zeros += (unsigned)__popcll(__ballot(clear[e]));
        }
        if (rem > zeros) {                                  // uniform: the rank lies among the keys with the bit set
            rem -= zeros;
            prefix |= bit;
#pragma unroll
            for (int e = 0; e < NE; ++e) key[e] = clear[e] ? NAN_KEY : key[e];
        } else {
#pragma unroll
            for (int e = 0; e < NE; ++e) key[e] = clear[e] ? key[e] : NAN_KEY;
        }
    }
    return prefix;
}

__global__ __launch_bounds__(NT) void k_knn_class_kth_wave(const float* __restrict__ dist, long long units, int N, long long ld,
                                                          const long long* __restrict__ start, int C, int K,
                                                          const long long* __restrict__ skip, int transform, float* __restrict__ out) {
    for (long long u = (long long)blockIdx.x * NW + (threadIdx.x >> 6); u < units; u += (long long)gridDim.x * NW) {     // per wave
        const Unit un = knn_unit(u, start, C, N);
        const long long n = un.c1 - un.c0;
        if (n > WAVE_MAX) continue;
        float v = INFINITY;
        const long long sk = skip ? skip[un.m] : -1;
        const int nv = n <= 0 ? 0 : (int)n - ((sk >= un.c0 && sk < un.c1) ? 1 : 0);
        if (nv > 0) {                                       // uniform, as is the choice of the register count
            const float* row = dist + (size_t)un.m * (size_t)ld;
            const unsigned rank = (unsigned)(K < nv ? K : nv);
            unsigned k;
            if (n <= 64) k = wave_select<1>(row, un.c0, un.c1, sk, rank);
            else if (n <= 256) k = wave_select<4>(row, un.c0, un.c1, sk, rank);
            else if (n <= 512) k = wave_select<8>(row, un.c0, un.c1, sk, rank);
            else if (n <= 1024) k = wave_select<16>(row, un.c0, un.c1, sk, rank);
            else k = wave_select<WE>(row, un.c0, un.c1, sk, rank);
            v = osi_tail::funkey(k);
        }
        if ((threadIdx.x & 63) == 0) out[u] = knn_transform(v, transform);
    }
}

__global__ __launch_bounds__(NT) void k_knn_class_kth(const float* __restrict__ dist, long long units, int N, long long ld,
                                                     const long long* __restrict__ start, int C, int K,
                                                     const long long* __restrict__ skip, int transform, float* __restrict__ out) {
    __shared__ Shared sm;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const Unit un = knn_unit(u, start, C, N);
        if (un.c1 - un.c0 <= WAVE_MAX) continue;            // uniform, before any barrier: the one-wave kernel's unit
        const long long m = un.m, c0 = un.c0, c1 = un.c1;
        const float* row = dist + (size_t)m * (size_t)ld;
        const long long sk = skip ? skip[m] : -1;
        const int count = stream_segment<false>(sm, row, c0, c1, sk, K);
        float v = INFINITY;
        if (count > 0) {                                    // uniform
            int r;
            v = osi_tail::funkey(select_rank(sm, count, count < K ? count : K, r));
        }
        if (threadIdx.x == 0) out[u] = knn_transform(v, transform);
        __syncthreads();                                    // the next unit rewrites the buffer and the histograms
    }
}

constexpr size_t KNN_WS_BYTES = 64;         // nothing is staged in global memory; a fixed, non-zero size keeps the calling convention

inline int grid_for(long long units) { return (int)(units < MAX_BLOCKS ? units : MAX_BLOCKS); }

}  // namespace

extern "C" {

size_t osi_knn_workspace(int M, int N, int K) { return (M > 0 && N > 0 && K > 0) ? KNN_WS_BYTES : 0; }

int osi_knn_topk(const float* dist, int M, int N, long long ld, int K, const long long* skip, float* out_dist, long long* out_idx,
                 void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(dist && out_dist && out_idx && ws);
    OSI_REQUIRE(M > 0 && N > 0 && ld >= N);
    OSI_REQUIRE(K >= 1 && K <= OSI_KNN_MAX_K);
    OSI_REQUIRE(ws_bytes >= KNN_WS_BYTES && ((uintptr_t)ws & 7) == 0);
    OSI_REQUIRE(((uintptr_t)dist & 3) == 0);
    hipLaunchKernelGGL(k_knn_topk, dim3(grid_for(M)), dim3(NT), 0, (hipStream_t)stream, dist, M, N, ld, K, skip, out_dist, out_idx);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_knn_class_kth(const float* dist, int M, int N, long long ld, const long long* start, int C, int K, const long long* skip,
                      int transform, float* out, void* ws, size_t ws_bytes, osi_stream_t stream) {
    OSI_REQUIRE(dist && start && out && ws);
    OSI_REQUIRE(M > 0 && N > 0 && C > 0 && ld >= N);
    OSI_REQUIRE(K >= 1 && K <= OSI_KNN_MAX_K);
    OSI_REQUIRE(transform == OSI_KNN_RAW || transform == OSI_KNN_SIM_COSINE || transform == OSI_KNN_SIM_INVERSE);
    OSI_REQUIRE(ws_bytes >= KNN_WS_BYTES && ((uintptr_t)ws & 7) == 0);
    OSI_REQUIRE(((uintptr_t)dist & 3) == 0);
    const long long units = (long long)M * C;
    // every unit is written by exactly one of the two launches: which one, the kernels read from start[] themselves
    hipLaunchKernelGGL(k_knn_class_kth_wave, dim3(grid_for((units + NW - 1) / NW)), dim3(NT), 0, (hipStream_t)stream, dist, units, N, ld,
                       start, C, K, skip, transform, out);
    OSI_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_knn_class_kth, dim3(grid_for(units)), dim3(NT), 0, (hipStream_t)stream, dist, units, N, ld, start, C, K, skip,
                       transform, out);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
