// Activation shaping (ReAct: Sun, Guo, Li, NeurIPS 2021; ASH: Djurisic et al., ICLR 2023; SCALE: Xu et al., ICLR 2024) and the
// logit scores they are read with (energy: Liu et al., NeurIPS 2020) on the GPU. include/osi.h (ABI 27) is the definition;
// openset_imagenet/shaping.py is the user's face of it, tests/shaping_oracle.py the numpy restatement.
//
//   osi_order_stats_f32   exact order statistics of n values: a four-pass radix select (8 bits a pass, most significant first) over the
//                         order-preserving 32-bit keys of v + 0.0f (every NaN the largest key). Each rank keeps its own key prefix and
//                         its remaining rank in the workspace. A pass is two launches: k_os_hist counts the next digit of the keys under a
//                         rank's prefix into per-workgroup LDS histograms and flushes them to 64-bit global counters (integer atomics:
//                         the counts do not depend on their order); k_os_select, one workgroup, scans the 256 counters of every rank
//                         and fixes its next digit. Ranks whose prefixes agree share one histogram (the two ranks of a percentile do
//                         so for most passes). Nothing is read back between passes; the last select stores the values.
//   osi_shape_rows        one workgroup per row, thread t holds columns e * 256 + t in registers. The kept set (the `keep` largest,
//                         ties by ascending column) is found as in knn.hip: a four-pass radix select in LDS gives the threshold key
//                         and the number r of its copies that are kept; wave ballots and a 64-entry table of (e, wave) counts give
//                         every copy its position in column order, and the first r stay. Row sums in fp64: per thread in e order,
//                         xor butterfly in the wave, the four waves in order. ReAct is a plain element-wise launch.
//   osi_logit_scores      one wave per row, fp64: maximum, then the max-shifted sum of exponentials; a row of at most 1024 columns
//                         stays in registers between the two.
// No floating-point arithmetic on the selection paths but v + 0.0f; no floating-point atomics anywhere.
#include "tail_fit.h"                       // fkey / funkey

#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int MAX_E = OSI_SHAPE_MAX_F / NT;  // 16 columns per thread
constexpr int MAX_R = OSI_ORDER_STATS_MAX_R;
constexpr int MAX_BLOCKS = 1 << 20;
constexpr unsigned NAN_KEY = 0xffffffffu;
static_assert(MAX_E * NW <= 64, "one wave scans the table of (e, wave) counts");
static_assert(MAX_R == 8, "the rank table travels in the kernel arguments");

// ascending order-preserving key of the canonical value (the order of ABI 24): -Inf < ... < -0 = +0 < ... < +Inf < every NaN
__device__ __forceinline__ unsigned shp_key(float d) {
    const float v = __fadd_rn(d, 0.0f);     // -0 -> +0
    return v != v ? NAN_KEY : osi_tail::fkey(v);
}
__device__ __forceinline__ float shp_unkey(unsigned k) { return k == NAN_KEY ? __uint_as_float(0x7fc00000u) : osi_tail::funkey(k); }

// ---------------------------------------------------------------------------------------------------------------- order statistics
// workspace: the head, then hist[4 passes][R][256] 64-bit counters
struct OsHead {
    unsigned long long rem[MAX_R];          // the rank that is left among the keys under `prefix`
    unsigned prefix[MAX_R];                 // the digits fixed so far, in place
};
constexpr size_t OS_HEAD_BYTES = 128;
static_assert(sizeof(OsHead) <= OS_HEAD_BYTES, "head");
struct OsRanks { long long r[MAX_R]; };

static size_t os_ws_bytes(int R) { return OS_HEAD_BYTES + (size_t)4 * R * 256 * sizeof(unsigned long long); }

// the rank whose histogram rank r reads: the first one with the same prefix
__device__ __forceinline__ int os_owner(const unsigned (&prefix)[MAX_R], int r) {
    int o = r;
#pragma unroll
    for (int q = MAX_R - 1; q >= 0; --q)
        if (q < r && prefix[q] == prefix[r]) o = q;
    return o;
}

__global__ __launch_bounds__(NT) void k_os_init(void* ws, OsRanks ranks, int R) {
    OsHead* head = (OsHead*)ws;
    unsigned long long* hist = (unsigned long long*)((char*)ws + OS_HEAD_BYTES);
    for (int i = threadIdx.x; i < 4 * R * 256; i += NT) hist[i] = 0ull;
    if ((int)threadIdx.x < R) {
        head->rem[threadIdx.x] = (unsigned long long)ranks.r[threadIdx.x];
        head->prefix[threadIdx.x] = 0u;
    }
}

__global__ __launch_bounds__(NT) void k_os_hist(const float* __restrict__ v, unsigned long long n, void* ws, int R, int p) {
    __shared__ unsigned h[MAX_R][256];
    const OsHead* head = (const OsHead*)ws;
    unsigned long long* hist = (unsigned long long*)((char*)ws + OS_HEAD_BYTES) + (size_t)p * R * 256;
    const int tid = threadIdx.x;
    unsigned prefix[MAX_R];
    bool own[MAX_R];
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) prefix[r] = r < R ? head->prefix[r] : 0u;
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) own[r] = r < R && os_owner(prefix, r) == r;
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) h[r][tid] = 0u;
    __syncthreads();
    const int sh = 24 - 8 * p;
    const unsigned mask = p == 0 ? 0u : 0xffffffffu << (32 - 8 * p);
    auto count = [&](float d) {
        const unsigned k = shp_key(d);
#pragma unroll
        for (int r = 0; r < MAX_R; ++r)     // the owners' prefixes differ: at most one of them takes the key
            if (own[r] && (k & mask) == prefix[r]) atomicAdd(&h[r][(k >> sh) & 255u], 1u);
    };
    // 16-byte loads over the aligned body; the up to 3 + 3 elements before and after it go to workgroup 0
    const unsigned long long lead = (unsigned long long)((0u - (unsigned)((uintptr_t)v >> 2)) & 3u);
    const unsigned long long before = lead < n ? lead : n;
    const unsigned long long n4 = (n - before) >> 2;
    const float4* __restrict__ v4 = reinterpret_cast<const float4*>(v + before);
    const unsigned long long step = (unsigned long long)gridDim.x * NT;
    for (unsigned long long i = (unsigned long long)blockIdx.x * NT + tid; i < n4; i += step) {
        const float4 q = v4[i];
        count(q.x); count(q.y); count(q.z); count(q.w);
    }
    if (blockIdx.x == 0 && tid < 4) {
        if ((unsigned long long)tid < before) count(v[tid]);
        const unsigned long long j = before + 4ull * n4 + tid;
        if (j < n) count(v[j]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MAX_R; ++r)
        if (own[r] && h[r][tid] != 0u) atomicAdd(&hist[r * 256 + tid], (unsigned long long)h[r][tid]);
}

// one workgroup: thread t owns digit t of every rank
__global__ __launch_bounds__(NT) void k_os_select(void* ws, int R, int p, float* __restrict__ out) {
    __shared__ unsigned long long wt[MAX_R][NW];
    __shared__ unsigned long long new_rem[MAX_R];
    __shared__ unsigned new_prefix[MAX_R];
    OsHead* head = (OsHead*)ws;
    const unsigned long long* hist = (const unsigned long long*)((char*)ws + OS_HEAD_BYTES) + (size_t)p * R * 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix[MAX_R];
    unsigned long long rem[MAX_R], c[MAX_R], incl[MAX_R];
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) {
        prefix[r] = r < R ? head->prefix[r] : 0u;
        rem[r] = r < R ? head->rem[r] : 0ull;
    }
    if (tid < MAX_R) {                                      // a rank keeps what it has unless a digit below claims it
        new_prefix[tid] = tid < R ? head->prefix[tid] : 0u;
        new_rem[tid] = tid < R ? head->rem[tid] : 0ull;
    }
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) {
        c[r] = 0ull; incl[r] = 0ull;
        if (r < R) {                                        // uniform
            c[r] = hist[os_owner(prefix, r) * 256 + tid];
            unsigned long long s = c[r];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long u = __shfl_up(s, o, 64);
                if (lane >= o) s += u;
            }
            incl[r] = s;
            if (lane == 63) wt[r][wave] = s;
        }
    }
    __syncthreads();
    const int sh = 24 - 8 * p;
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) {
        if (r < R) {
            unsigned long long base = 0ull;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (w < wave) base += wt[r][w];
            const unsigned long long excl = base + incl[r] - c[r];
            if (excl <= rem[r] && rem[r] < excl + c[r]) {   // exactly one digit: the keys under the prefix number more than rem
                new_prefix[r] = prefix[r] | ((unsigned)tid << sh);
                new_rem[r] = rem[r] - excl;
            }
        }
    }
    __syncthreads();
    if (tid < R) {
        head->prefix[tid] = new_prefix[tid];
        head->rem[tid] = new_rem[tid];
        if (p == 3) out[tid] = shp_unkey(new_prefix[tid]);
    }
}

// ------------------------------------------------------------------------------------------------------------------------- shaping
__device__ __forceinline__ float react(float v, float clip) { return v > clip ? clip : v; }       // a NaN compares false and stays

// VEC: both pointers are 16-byte aligned; the n % 4 elements after the last whole quad go to workgroup 0
template <bool VEC>
__global__ __launch_bounds__(NT) void k_shape_react(const float* __restrict__ x, size_t n, float clip, float* __restrict__ out) {
    const size_t step = (size_t)gridDim.x * NT, first = (size_t)blockIdx.x * NT + threadIdx.x;
    if (VEC) {
        const size_t n4 = n >> 2;
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        float4* __restrict__ o4 = reinterpret_cast<float4*>(out);
        for (size_t i = first; i < n4; i += step) {
            const float4 v = x4[i];
            o4[i] = make_float4(react(v.x, clip), react(v.y, clip), react(v.z, clip), react(v.w, clip));
        }
        const size_t j = 4 * n4 + threadIdx.x;
        if (blockIdx.x == 0 && threadIdx.x < 4 && j < n) out[j] = react(x[j], clip);
    } else {
        for (size_t i = first; i < n; i += step) out[i] = react(x[i], clip);
    }
}

struct RowShared {
    __attribute__((aligned(16))) unsigned hist[4][256];    // read back as uint4
    unsigned wc[64];
    double red[2][NW];
};

template <int NE>
__global__ __launch_bounds__(NT) void k_shape_rows(const float* __restrict__ x, int M, int F, int mode, int keep, float* __restrict__ out) {
    __shared__ RowShared sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int row = blockIdx.x; row < M; row += gridDim.x) {
        const float* __restrict__ xr = x + (size_t)row * F;
        float* __restrict__ yr = out + (size_t)row * F;
        float v[NE];
        unsigned dk[NE];                    // ~key: ascending dk = descending value, every NaN first
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int col = e * NT + tid;
            v[e] = col < F ? xr[col] : 0.f;
            dk[e] = ~shp_key(v[e]);
        }
        // the keep-th smallest dk: T, and how many copies of it the kept set holds (the select of knn.hip)
        __syncthreads();                                    // the previous row's readers are done
#pragma unroll
        for (int p = 0; p < 4; ++p) sm.hist[p][tid] = 0u;
        __syncthreads();
        unsigned prefix = 0u, mask = 0u, rem = (unsigned)keep;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int sh = 24 - 8 * p;
#pragma unroll
            for (int e = 0; e < NE; ++e)
                if (e * NT + tid < F && (dk[e] & mask) == prefix) atomicAdd(&sm.hist[p][(dk[e] >> sh) & 255u], 1u);
            __syncthreads();
            const uint4 h = *reinterpret_cast<const uint4*>(&sm.hist[p][4 * lane]);
            const unsigned own = h.x + h.y + h.z + h.w;
            unsigned incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned u = __shfl_up(incl, o, 64);
                if (lane >= o) incl += u;
            }
            const unsigned long long reach = __ballot(incl >= rem);     // never empty: keep <= F
            const int l = reach ? __ffsll((long long)reach) - 1 : 63;
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
        const unsigned T = prefix, r = rem;
        // copies of T in column order: element (e, wave, lane) comes after all of e' < e, then the waves before, then the lanes below
        unsigned mine = 0u;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const unsigned long long b2 = __ballot(e * NT + tid < F && dk[e] == T);
            if (lane == e) mine = (unsigned)__popcll(b2);
        }
        if (lane < MAX_E) sm.wc[lane * NW + wave] = mine;   // lanes NE .. 15: no such columns
        __syncthreads();
        const unsigned cnt = sm.wc[lane];
        unsigned scan = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = __shfl_up(scan, o, 64);
            if (lane >= o) scan += u;
        }
        const unsigned excl = scan - cnt;
        unsigned kept = 0u;
        double a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const bool present = e * NT + tid < F;
            const bool is_t = present && dk[e] == T;
            const unsigned long long b2 = __ballot(is_t);
            const unsigned eq = __shfl(excl, e * NW + wave, 64) + (unsigned)__popcll(b2 & below);
            const bool k = present && (dk[e] < T || (is_t && eq < r));
            if (k) kept |= 1u << e;
            if (present) a1 += (double)v[e];
            if (k) a2 += (double)v[e];
        }
        a1 = wave_sum(a1);
        a2 = wave_sum(a2);
        if (lane == 0) { sm.red[0][wave] = a1; sm.red[1][wave] = a2; }
        __syncthreads();
        double s1 = sm.red[0][0], s2 = sm.red[1][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) { s1 += sm.red[0][w]; s2 += sm.red[1][w]; }
        const float fill = (float)(s1 / (double)keep);
        const float scale = (mode == OSI_SHAPE_ASH_S || mode == OSI_SHAPE_SCALE) ? (float)exp(s1 / s2) : 1.0f;    // 0 / 0 stays a NaN
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int col = e * NT + tid;
            if (col < F) {
                const bool k = (kept >> e) & 1u;
                float y;
                if (mode == OSI_SHAPE_ASH_P) y = k ? v[e] : 0.f;
                else if (mode == OSI_SHAPE_ASH_B) y = k ? fill : 0.f;
                else if (mode == OSI_SHAPE_ASH_S) y = k ? v[e] * scale : 0.f;
                else y = v[e] * scale;
                yr[col] = y;
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------------- scores
// QUADS: C is a multiple of 4 and at most 1024: lane l owns the quads l, l + 64, ... of the row and keeps them in registers between
// the two passes (16-byte loads where the row is aligned: the same elements in the same order either way). Otherwise lane l owns
// columns l, l + 64, ... and the second pass reads the row again. Which of the two runs is a function of C alone.
template <bool QUADS>
__global__ __launch_bounds__(NT) void k_logit_scores(const float* __restrict__ logits, int M, int C, int mode, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * NW;
    for (long long row = (long long)blockIdx.x * NW + (threadIdx.x >> 6); row < M; row += waves) {
        const float* __restrict__ lr = logits + (size_t)row * C;
        double m = -INFINITY, s = 0.0;
        bool nan = false;
        if (QUADS) {
            const int nq = C >> 2;
            const bool vec = ((uintptr_t)lr & 15) == 0;     // uniform in the wave
            float4 q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = lane + 64 * k;
                q[k] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);     // neutral for the maximum, exp = 0 in the sum
                if (i < nq) q[k] = vec ? reinterpret_cast<const float4*>(lr)[i] : make_float4(lr[4 * i], lr[4 * i + 1], lr[4 * i + 2], lr[4 * i + 3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m = fmax(fmax(fmax(m, (double)q[k].x), fmax((double)q[k].y, (double)q[k].z)), (double)q[k].w);
                nan = nan || q[k].x != q[k].x || q[k].y != q[k].y || q[k].z != q[k].z || q[k].w != q[k].w;
            }
            m = wave_fmax(m);
            nan = __any(nan);
            if (mode != OSI_SCORE_MAXLOGIT) {
                const double shift = isfinite(m) ? m : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (lane + 64 * k < nq)
                        s += exp((double)q[k].x - shift) + exp((double)q[k].y - shift) + exp((double)q[k].z - shift) + exp((double)q[k].w - shift);
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float v = lr[c];
                m = fmax(m, (double)v);                     // skips a NaN: `nan` keeps it
                nan = nan || v != v;
            }
            m = wave_fmax(m);
            nan = __any(nan);
            if (mode != OSI_SCORE_MAXLOGIT) {
                const double shift = isfinite(m) ? m : 0.0;
                for (int c = lane; c < C; c += 64) s += exp((double)lr[c] - shift);
            }
        }
        const double shift = isfinite(m) ? m : 0.0;         // an infinite maximum is not subtracted
        double y;
        if (mode == OSI_SCORE_MAXLOGIT) y = nan ? (double)NAN : m;
        else {
            s = wave_sum(s);                                // a NaN in the row is a NaN here
            y = mode == OSI_SCORE_ENERGY ? shift + log(s) : exp(m - shift) / s;
        }
        if (lane == 0) out[row] = (float)y;
    }
}

static unsigned grid_for(long long units) { return (unsigned)(units < MAX_BLOCKS ? (units > 0 ? units : 1) : MAX_BLOCKS); }

}  // namespace

extern "C" {

size_t osi_order_stats_workspace(long long n, int R) { return (n > 0 && R >= 1 && R <= MAX_R) ? os_ws_bytes(R) : 0; }

int osi_order_stats_f32(const float* v, long long n, const long long* ranks, int R, float* out, void* ws, size_t ws_bytes,
                        osi_stream_t stream) {
    OSI_REQUIRE(v && ranks && out && ws);
    OSI_REQUIRE(n > 0 && R >= 1 && R <= MAX_R);
    OSI_REQUIRE(ws_bytes >= os_ws_bytes(R) && ((uintptr_t)ws & 7) == 0);
    OSI_REQUIRE(((uintptr_t)v & 3) == 0);
    OsRanks rk = {};
    for (int r = 0; r < R; ++r) {
        OSI_REQUIRE(ranks[r] >= 0 && ranks[r] < n);
        rk.r[r] = ranks[r];
    }
    hipStream_t st = (hipStream_t)stream;
    // 1024 workgroups of 16-byte loads, and never 2^31 or more elements in one workgroup's 32-bit LDS counters
    long long blocks = (n / 4 + NT * 8 - 1) / (NT * 8);
    blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
    const long long least = (n + (1ll << 31) - 1) >> 31;
    if (blocks < least) blocks = least;
    OSI_REQUIRE(blocks <= 0x7fffffffll);
    hipLaunchKernelGGL(k_os_init, dim3(1), dim3(NT), 0, st, ws, rk, R);
    OSI_LAUNCH_CHECK();
    for (int p = 0; p < 4; ++p) {
        hipLaunchKernelGGL(k_os_hist, dim3((unsigned)blocks), dim3(NT), 0, st, v, (unsigned long long)n, ws, R, p);
        OSI_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_os_select, dim3(1), dim3(NT), 0, st, ws, R, p, out);
        OSI_LAUNCH_CHECK();
    }
    return OSI_OK;
}

constexpr size_t SHAPE_WS_BYTES = 64;       // the kernels stage nothing in it
size_t osi_shape_rows_workspace(int M, int F) { return (M > 0 && F >= 1 && F <= OSI_SHAPE_MAX_F) ? SHAPE_WS_BYTES : 0; }

int osi_shape_rows(const float* x, int M, int F, int mode, int keep, float clip, float* out, void* ws, size_t ws_bytes,
                   osi_stream_t stream) {
    OSI_REQUIRE(x && out && ws);
    OSI_REQUIRE(M > 0 && F >= 1 && F <= OSI_SHAPE_MAX_F);
    OSI_REQUIRE(mode >= OSI_SHAPE_REACT && mode <= OSI_SHAPE_SCALE);
    OSI_REQUIRE(mode == OSI_SHAPE_REACT ? keep == 0 : (keep >= 1 && keep <= F));
    OSI_REQUIRE(ws_bytes >= SHAPE_WS_BYTES && ((uintptr_t)ws & 7) == 0);
    OSI_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0);
    const size_t n = (size_t)M * F;
    OSI_REQUIRE((uintptr_t)out + n * sizeof(float) <= (uintptr_t)x || (uintptr_t)x + n * sizeof(float) <= (uintptr_t)out);   // no aliasing
    hipStream_t st = (hipStream_t)stream;
    if (mode == OSI_SHAPE_REACT) {
        const unsigned grid = grid_for((long long)((n + NT * 4 - 1) / (NT * 4)));
        if ((((uintptr_t)x | (uintptr_t)out) & 15) == 0) hipLaunchKernelGGL(k_shape_react<true>, dim3(grid), dim3(NT), 0, st, x, n, clip, out);
        else hipLaunchKernelGGL(k_shape_react<false>, dim3(grid), dim3(NT), 0, st, x, n, clip, out);
        OSI_LAUNCH_CHECK();
        return OSI_OK;
    }
    // columns per thread: the smallest power of two that covers the row
    int ne = 1;
    while (ne * NT < F) ne *= 2;
    return pick<1, 2, 4, 8, 16>(ne, [&](auto NE) -> int {
        hipLaunchKernelGGL(k_shape_rows<decltype(NE)::value>, dim3(grid_for(M)), dim3(NT), 0, st, x, M, F, mode, keep, out);
        OSI_LAUNCH_CHECK();
        return OSI_OK;
    });
}

int osi_logit_scores(const float* logits, int M, int C, int mode, float* out, osi_stream_t stream) {
    OSI_REQUIRE(logits && out);
    OSI_REQUIRE(M > 0 && C > 0);
    OSI_REQUIRE(mode >= OSI_SCORE_ENERGY && mode <= OSI_SCORE_MSP);
    OSI_REQUIRE(((uintptr_t)logits & 3) == 0 && ((uintptr_t)out & 3) == 0);
    const unsigned grid = grid_for(((long long)M + NW - 1) / NW);
    if (C % 4 == 0 && C <= 1024) hipLaunchKernelGGL(k_logit_scores<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, logits, M, C, mode, out);
    else hipLaunchKernelGGL(k_logit_scores<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, logits, M, C, mode, out);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
