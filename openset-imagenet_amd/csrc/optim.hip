// Fused optimizer steps over the flat fp32 parameter arena (one launch for all 162 tensors).
// Reference: torch.optim.Adam(lr) / torch.optim.SGD(lr, momentum=0.9) built at openset_imagenet/train.py:356-359 and
// stepped at train.py:139. Arithmetic follows torch's single-tensor rules:
//   Adam: m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
//   SGD : buf = g (first step) | mu*buf + g ; p -= lr*buf
// Also: arena utilities used by the loop (zero fill, int64 counter bump for num_batches_tracked, scale for DP averaging, and the
// sum of two gradient arenas: the clean and the adversarial backward of one step, openset_imagenet/adversary.py), and the averaged
// copy of the weights (EMA / SWA, openset_imagenet/averaging.py): avg = lerp(avg, cur, weight) over several arenas in one launch.
#include "osi_common.h"

#include <cmath>
#include <cstring>

namespace {

__global__ __launch_bounds__(256) void k_adam(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m, f32x4* __restrict__ v,
                                             size_t n4, float step_size, float b2, float omb1, float omb2, float eps,
                                             float sqrt_bc2, float gscale) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t step = (size_t)gridDim.x * 256;
    for (; i < n4; i += step) {
        f32x4 gg = g[i] * gscale, mm = m[i], vv = v[i], pp = p[i];
        mm = mm + (gg - mm) * omb1;              // torch: exp_avg.lerp_(grad, 1-beta1)
        vv = vv * b2 + gg * gg * omb2;         // torch: exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
        f32x4 den;
        den.x = sqrtf(vv.x) / sqrt_bc2 + eps; den.y = sqrtf(vv.y) / sqrt_bc2 + eps;
        den.z = sqrtf(vv.z) / sqrt_bc2 + eps; den.w = sqrtf(vv.w) / sqrt_bc2 + eps;
        pp = pp - (mm / den) * step_size;       // torch: param.addcdiv_(exp_avg, denom, value=-step_size)
        m[i] = mm; v[i] = vv; p[i] = pp;
    }
}

__global__ __launch_bounds__(256) void k_sgd(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ buf, size_t n4, float lr,
                                            float mu, int first, float gscale) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t step = (size_t)gridDim.x * 256;
    for (; i < n4; i += step) {
        f32x4 gg = g[i] * gscale;
        f32x4 b = first ? gg : buf[i] * mu + gg;
        buf[i] = b;
        p[i] = p[i] - b * lr;
    }
}

// Per-group scalars of the grouped kernels, prepared on the host in double (osi_*_step_groups).
enum : uint32_t { OPT_DECOUPLED = 1, OPT_AMSGRAD = 2, OPT_MAXIMIZE = 4, OPT_NESTEROV = 8, OPT_FIRST = 16, OPT_MOMENTUM = 32 };
struct AdamScal {
    float step_size, sqrt_bc2, b2, omb1, omb2, eps, wd, decay_mul;   // lr/bc1, sqrt(bc2), beta2, 1-beta1, 1-beta2, eps, wd, 1-lr*wd
    uint32_t flags;
};
struct SgdScal {
    float lr, mu, omd, wd;   // omd = 1 - dampening
    uint32_t flags;
};

__device__ __forceinline__ f32x4 splat4(float s) { return f32x4{s, s, s, s}; }
__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(a, b, c); }

// The per-element rules of the grouped kernels. The contractions are spelled out as the compiler forms them in k_adam / k_sgd above
// (whose bodies stay as they are: routing them through these functions changed their register allocation and schedule), so a group
// with default options (no flags besides OPT_MOMENTUM / OPT_FIRST, wd 0, omd 1) gives the bits of the plain kernel:
//   k_adam: d = fma(g, gscale, -m); m = fma(d, 1-b1, m); v = fma(v, b2, ((g*gscale)^2)*(1-b2)); p = fma(-step_size, m/den, p)
//   k_sgd : b = fma(mu, buf, g*gscale); p = fma(-lr, b, p)
// g is the raw gradient; vmax is read and written only under OPT_AMSGRAD.
__device__ __forceinline__ void adam_update(f32x4& pp, f32x4 g, f32x4& mm, f32x4& vv, f32x4& vmax, const AdamScal& s, float gscale) {
    f32x4 gg = g * gscale;
    f32x4 d = fma4(g, splat4(gscale), -mm);      // (g*gscale - m) in one rounding
    const bool l2 = s.wd != 0.f && !(s.flags & OPT_DECOUPLED);
    if (s.flags & OPT_MAXIMIZE) gg = -gg;
    if (s.flags & OPT_DECOUPLED) pp = pp * s.decay_mul;     // torch AdamW: param.mul_(1 - lr*wd)
    if (l2) gg = fma4(splat4(s.wd), pp, gg);                // torch Adam: grad.add(param, alpha=wd)
    if (l2 || (s.flags & OPT_MAXIMIZE)) d = gg - mm;
    mm = fma4(d, splat4(s.omb1), mm);                       // torch: exp_avg.lerp_(grad, 1-beta1)
    vv = fma4(vv, splat4(s.b2), gg * gg * s.omb2);          // torch: exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    f32x4 vd = vv;
    if (s.flags & OPT_AMSGRAD) {                            // torch: max_exp_avg_sq = max(max_exp_avg_sq, exp_avg_sq)
        vmax.x = fmaxf(vmax.x, vv.x); vmax.y = fmaxf(vmax.y, vv.y); vmax.z = fmaxf(vmax.z, vv.z); vmax.w = fmaxf(vmax.w, vv.w);
        vd = vmax;
    }
    f32x4 den;
    den.x = sqrtf(vd.x) / s.sqrt_bc2 + s.eps; den.y = sqrtf(vd.y) / s.sqrt_bc2 + s.eps;
    den.z = sqrtf(vd.z) / s.sqrt_bc2 + s.eps; den.w = sqrtf(vd.w) / s.sqrt_bc2 + s.eps;
    pp = fma4(-(mm / den), splat4(s.step_size), pp);         // torch: param.addcdiv_(exp_avg, denom, value=-step_size)
}

// b: the momentum buffer, read by the caller unless OPT_FIRST, written back under OPT_MOMENTUM.
__device__ __forceinline__ void sgd_update(f32x4& pp, f32x4 g, f32x4& b, const SgdScal& s, float gscale) {
    f32x4 gg = g * gscale;
    if (s.flags & OPT_MAXIMIZE) gg = -gg;
    if (s.wd != 0.f) gg = fma4(splat4(s.wd), pp, gg);
    if (s.flags & OPT_MOMENTUM) {
        b = (s.flags & OPT_FIRST) ? gg : fma4(splat4(s.mu), b, gg * s.omd);
        gg = (s.flags & OPT_NESTEROV) ? fma4(splat4(s.mu), b, gg) : b;
    }
    pp = fma4(-gg, splat4(s.lr), pp);
}

// ---- grouped forms: one launch over the arena, every 16-byte unit under the rule of the segment it lies in -------------------
// The host cuts the arena into contiguous chunks of whole 256-unit tiles, one per workgroup, so a thread's unit index only grows and
// its segment index only advances. The tables arrive by value in the kernel arguments and are staged in LDS once per workgroup
// (so that the divergent lookups below index LDS, not the argument struct); a thread keeps its current segment's bounds and
// its group's scalars in registers and touches LDS again only when it crosses a segment end.
struct SegTable {
    uint32_t begin[OSI_OPT_MAX_SEGMENTS], end[OSI_OPT_MAX_SEGMENTS];
    uint8_t group[OSI_OPT_MAX_SEGMENTS];
    int n;
};
struct AdamGroups { AdamScal g[OSI_OPT_MAX_GROUPS]; };
struct SgdGroups { SgdScal g[OSI_OPT_MAX_GROUPS]; };

template <class Scal, class Groups>
struct SegWalker {
    uint32_t* s_begin; uint32_t* s_end; uint32_t* s_group; Scal* s_scal;
    int nseg, st;
    uint32_t cb, ce;   // bounds of segment st; both ~0u past the last one
    Scal sc;

    __device__ __forceinline__ void stage(const SegTable& tab, const Groups& grp) {
        const int t = threadIdx.x;
        if (t < OSI_OPT_MAX_SEGMENTS) { s_begin[t] = tab.begin[t]; s_end[t] = tab.end[t]; s_group[t] = tab.group[t]; }
        constexpr int words = (int)(sizeof(Groups) / 4);
        static_assert(words <= 256, "group table is staged by one pass of the workgroup");
        if (t < words) ((uint32_t*)s_scal)[t] = ((const uint32_t*)&grp)[t];
        __syncthreads();
        nseg = tab.n;
    }
    __device__ __forceinline__ void load() {
        if (st < nseg) { cb = s_begin[st]; ce = s_end[st]; sc = s_scal[s_group[st]]; }
        else cb = ce = ~0u;
    }
    // first segment that ends after unit i
    __device__ __forceinline__ void seek(uint32_t i) {
        int a = 0, b = nseg;
        while (a < b) { const int mid = (a + b) >> 1; if (s_end[mid] <= i) a = mid + 1; else b = mid; }
        st = a;
        load();
    }
    // i only grows between calls; true when unit i lies in a segment (sc then holds its group)
    __device__ __forceinline__ bool covers(uint32_t i) {
        if (i >= ce) { do ++st; while (st < nseg && s_end[st] <= i); load(); }
        return i >= cb;
    }
};

// GS: the gradient scalar as the kernels take it. float = in the kernel arguments (osi_*_step_groups); const float* = one float in
// device memory, written by an earlier launch on the stream (osi_*_step_groups_dev, after osi_grad_clip_scale): a uniform load, after
// which the body is the same code on the same value, hence the same bits.
__device__ __forceinline__ float gs_value(float s) { return s; }
__device__ __forceinline__ float gs_value(const float* s) { return *s; }

template <class GS>
__global__ __launch_bounds__(256) void k_adam_groups(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m,
                                                    f32x4* __restrict__ v, f32x4* __restrict__ vmax, uint32_t n4, uint32_t chunk4,
                                                    GS gs, SegTable tab, AdamGroups grp) {
    const float gscale = gs_value(gs);
    __shared__ uint32_t s_begin[OSI_OPT_MAX_SEGMENTS], s_end[OSI_OPT_MAX_SEGMENTS], s_group[OSI_OPT_MAX_SEGMENTS];
    __shared__ AdamScal s_scal[OSI_OPT_MAX_GROUPS];
    SegWalker<AdamScal, AdamGroups> w{s_begin, s_end, s_group, s_scal};
    w.stage(tab, grp);
    const uint32_t lo = blockIdx.x * chunk4;                       // lo < n4 <= 2^32 - 512 (fill_seg_table), so i += 256 cannot wrap
    const uint32_t hi = n4 - lo < chunk4 ? n4 : lo + chunk4;
    uint32_t i = lo + threadIdx.x;
    w.seek(i);
    for (; i < hi && w.st < w.nseg; i += 256) {
        if (!w.covers(i)) continue;
        const AdamScal& s = w.sc;
        f32x4 mm = m[i], vv = v[i], pp = p[i], vm = {};
        if (s.flags & OPT_AMSGRAD) vm = vmax[i];
        adam_update(pp, g[i], mm, vv, vm, s, gscale);
        m[i] = mm; v[i] = vv; p[i] = pp;
        if (s.flags & OPT_AMSGRAD) vmax[i] = vm;
    }
}

template <class GS>
__global__ __launch_bounds__(256) void k_sgd_groups(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ buf,
                                                   uint32_t n4, uint32_t chunk4, GS gs, SegTable tab, SgdGroups grp) {
    const float gscale = gs_value(gs);
    __shared__ uint32_t s_begin[OSI_OPT_MAX_SEGMENTS], s_end[OSI_OPT_MAX_SEGMENTS], s_group[OSI_OPT_MAX_SEGMENTS];
    __shared__ SgdScal s_scal[OSI_OPT_MAX_GROUPS];
    SegWalker<SgdScal, SgdGroups> w{s_begin, s_end, s_group, s_scal};
    w.stage(tab, grp);
    const uint32_t lo = blockIdx.x * chunk4;
    const uint32_t hi = n4 - lo < chunk4 ? n4 : lo + chunk4;
    uint32_t i = lo + threadIdx.x;
    w.seek(i);
    for (; i < hi && w.st < w.nseg; i += 256) {
        if (!w.covers(i)) continue;
        const SgdScal& s = w.sc;
        f32x4 b = {}, pp = p[i];
        if ((s.flags & (OPT_MOMENTUM | OPT_FIRST)) == OPT_MOMENTUM) b = buf[i];   // a momentum-free group never touches the buffer arena
        sgd_update(pp, g[i], b, s, gscale);
        if (s.flags & OPT_MOMENTUM) buf[i] = b;
        p[i] = pp;
    }
}

__global__ __launch_bounds__(256) void k_fill(f32x4* __restrict__ p, size_t n4, float val) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t step = (size_t)gridDim.x * 256;
    for (; i < n4; i += step) p[i] = f32x4{val, val, val, val};
}
__global__ __launch_bounds__(256) void k_scale(f32x4* __restrict__ p, size_t n4, float s) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t step = (size_t)gridDim.x * 256;
    for (; i < n4; i += step) p[i] = p[i] * s;
}
__global__ __launch_bounds__(256) void k_accumulate(f32x4* __restrict__ dst, const f32x4* __restrict__ src, size_t n4) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t step = (size_t)gridDim.x * 256;
    for (; i < n4; i += step) dst[i] = dst[i] + src[i];
}
__global__ void k_i64_add(long long* p, int n, long long inc) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] += inc;
}

// ---- weight averaging (osi_average_update): avg = lerp(avg, cur, weight) over up to OSI_AVG_MAX_SPANS arena pairs, one launch ------
// The spans are cut into tiles of AVG_TILE floats (one 16-byte unit per lane); tile_end[s] = tiles of spans 0..s, so a workgroup's
// virtual tile index names a span and a tile in it (a uniform search over at most four bounds), and at most AVG_MAX_GRID workgroups
// walk the tiles in a grid stride. The table arrives by value in the kernel arguments.
constexpr uint32_t AVG_TILE = 1024;       // floats per workgroup tile = 256 lanes x one f32x4
constexpr uint32_t AVG_MAX_GRID = 2048;   // grid cap, as the other arena kernels
struct AvgTable {
    f32x4* avg[OSI_AVG_MAX_SPANS];
    const f32x4* cur[OSI_AVG_MAX_SPANS];
    uint32_t n4[OSI_AVG_MAX_SPANS];
    uint32_t tile_end[OSI_AVG_MAX_SPANS];  // <= 4 * 2^24 tiles
    int n;
};

// torch.lerp on fp32: d = cur - avg; weight < 0.5 (LOW): fma(w, d, avg) with w = weight; else fma(w, d, cur) with w = weight - 1
template <bool LOW>
__global__ __launch_bounds__(256) void k_average(AvgTable tab, float w) {
    const uint32_t tiles = tab.tile_end[tab.n - 1];
    const f32x4 w4 = splat4(w);
    for (uint32_t v = blockIdx.x; v < tiles; v += gridDim.x) {
        int s = 0;
        uint32_t first = 0;
#pragma unroll
        for (int k = 0; k < OSI_AVG_MAX_SPANS - 1; ++k)
            if (k + 1 < tab.n && v >= tab.tile_end[k]) { s = k + 1; first = tab.tile_end[k]; }
        const uint32_t i = (v - first) * 256 + threadIdx.x;    // < n4 + 256 <= 2^32 - 256: cannot wrap
        if (i < tab.n4[s]) {
            f32x4* __restrict__ pa = tab.avg[s];
            const f32x4 a = pa[i], c = tab.cur[s][i];
            const f32x4 d = c - a;
            pa[i] = fma4(w4, d, LOW ? a : c);
        }
    }
}

static int sgrid(size_t n4) {
    size_t g = (n4 + 255) / 256;
    return (int)(g > 2048 ? 2048 : (g ? g : 1));
}

// Validates the caller's segment table against the arena (n floats) and packs it for the kernel arguments; false = malformed.
static bool fill_seg_table(SegTable& tab, const osi_opt_segment* seg, int n_segments, int n_groups, size_t n) {
    if (!seg || n == 0 || n % 4 != 0 || n / 4 > 0xFFFFFFFFull - 511) return false;   // unit indices are 32 bits; room for one stride past the end
    if (n_segments < 1 || n_segments > OSI_OPT_MAX_SEGMENTS || n_groups < 1 || n_groups > OSI_OPT_MAX_GROUPS) return false;
    memset(&tab, 0, sizeof tab);
    uint32_t prev_end = 0;
    for (int i = 0; i < n_segments; ++i) {
        if (seg[i].begin4 < prev_end || seg[i].end4 <= seg[i].begin4 || seg[i].end4 > n / 4) return false;
        if (seg[i].group < 0 || seg[i].group >= n_groups) return false;
        tab.begin[i] = seg[i].begin4; tab.end[i] = seg[i].end4; tab.group[i] = (uint8_t)seg[i].group;
        prev_end = seg[i].end4;
    }
    tab.n = n_segments;
    return true;
}

// One contiguous chunk of whole 256-unit tiles per workgroup, at most 2048 workgroups (the plain kernels' grid).
static int chunk_grid(size_t n4, uint32_t& chunk4) {
    const size_t tiles = (n4 + 255) / 256;
    const size_t per = (tiles + 2047) / 2048;
    chunk4 = (uint32_t)(per * 256);
    return (int)((tiles + per - 1) / per);
}

// ---- gradient norm over spans of the arena, and the clipping scalar (osi_grad_clip_scale) ---------------------------------------
// A span is a tensor: units [begin, end) of 4 floats, of whose last unit only `last` floats (1..4) belong to it; the alignment lanes
// behind them, like every unit outside every span, are skipped by selection (never multiplied by zero: they may hold anything).
// The arena is cut as chunk_grid cuts it for the grouped kernels. Fixed order, no atomics: a lane adds its units in index order,
// xor-butterfly over the wave, the four waves in order, one 8-byte partial per workgroup; k_grad_norm_final gives eight consecutive
// partials to a lane, added in index order, then the same tree. L2 squares and sums in double ((double)g * g is exact); the
// maximum norm compares the bit patterns of |g| as integers: the order of the non-negative floats with every NaN above +inf, so a NaN
// element comes out as a NaN norm, as torch's does.
struct SpanTable {
    uint32_t begin[OSI_OPT_MAX_SEGMENTS], end[OSI_OPT_MAX_SEGMENTS];
    uint8_t last[OSI_OPT_MAX_SEGMENTS];
    int n;
};

template <int NORM> struct NormAcc;
template <> struct NormAcc<OSI_NORM_L2> {
    double v = 0.0;
    __device__ __forceinline__ void add(float x, bool on) { const double d = (double)x; v += on ? d * d : 0.0; }
    __device__ __forceinline__ void merge(unsigned long long bits) { v += __longlong_as_double((long long)bits); }
    __device__ __forceinline__ void wave() { v = wave_sum(v); }
    __device__ __forceinline__ unsigned long long bits() const { return (unsigned long long)__double_as_longlong(v); }
    __device__ __forceinline__ double norm() const { return sqrt(v); }
};
template <> struct NormAcc<OSI_NORM_INF> {
    uint32_t v = 0;
    __device__ __forceinline__ void add(float x, bool on) { const uint32_t b = __float_as_uint(x) & 0x7FFFFFFFu; v = on && b > v ? b : v; }
    __device__ __forceinline__ void merge(unsigned long long bits) { v = (uint32_t)bits > v ? (uint32_t)bits : v; }
    __device__ __forceinline__ void wave() {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
    }
    __device__ __forceinline__ unsigned long long bits() const { return v; }
    __device__ __forceinline__ double norm() const { return (double)__uint_as_float(v); }
};

// wave, then the four waves in order; the total is valid in thread 0
template <int NORM>
__device__ __forceinline__ void block_reduce(NormAcc<NORM>& acc, unsigned long long* s_part) {
    acc.wave();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc.bits();
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = NormAcc<NORM>();
        for (int w = 0; w < 4; ++w) acc.merge(s_part[w]);
    }
}

template <int NORM>
__global__ __launch_bounds__(256) void k_grad_norm(const f32x4* __restrict__ g, uint32_t n4, uint32_t chunk4, SpanTable tab,
                                                  unsigned long long* __restrict__ ws) {
    __shared__ uint32_t s_begin[OSI_OPT_MAX_SEGMENTS], s_end[OSI_OPT_MAX_SEGMENTS], s_last[OSI_OPT_MAX_SEGMENTS];
    __shared__ unsigned long long s_part[4];
    const int t = threadIdx.x;
    if (t < OSI_OPT_MAX_SEGMENTS) { s_begin[t] = tab.begin[t]; s_end[t] = tab.end[t]; s_last[t] = tab.last[t]; }
    __syncthreads();
    const int nseg = tab.n;
    const uint32_t lo = blockIdx.x * chunk4;                       // as in k_adam_groups: n4 <= 2^32 - 512, i += 256 cannot wrap
    const uint32_t hi = n4 - lo < chunk4 ? n4 : lo + chunk4;
    uint32_t i = lo + t;
    int a = 0, b = nseg;                                           // first span that ends after unit i
    while (a < b) { const int mid = (a + b) >> 1; if (s_end[mid] <= i) a = mid + 1; else b = mid; }
    int st = a;
    uint32_t cb = ~0u, ce = ~0u, cl = 4;
    if (st < nseg) { cb = s_begin[st]; ce = s_end[st]; cl = s_last[st]; }
    NormAcc<NORM> acc;
    for (; i < hi && st < nseg; i += 256) {
        if (i >= ce) {
            do ++st; while (st < nseg && s_end[st] <= i);
            if (st < nseg) { cb = s_begin[st]; ce = s_end[st]; cl = s_last[st]; }
            else cb = ce = ~0u;
        }
        if (i < cb) continue;
        const f32x4 x = g[i];
        const uint32_t keep = i + 1 == ce ? cl : 4u;
        acc.add(x.x, true); acc.add(x.y, keep > 1); acc.add(x.z, keep > 2); acc.add(x.w, keep > 3);
    }
    block_reduce(acc, s_part);
    if (t == 0) ws[blockIdx.x] = acc.bits();                       // every workgroup writes its slot, an empty chunk its zero
}

// out2[0] = |grad_scale| * norm; out2[1] = grad_scale * min(1, max_norm / (out2[0] + 1e-6f)) in fp32 with torch's roundings: its
// `max_norm / tensor` is reciprocal(tensor) * max_norm, and its clamp keeps a NaN
template <int NORM>
__global__ __launch_bounds__(256) void k_grad_norm_final(const unsigned long long* __restrict__ ws, int parts, float grad_scale,
                                                        float max_norm, float* __restrict__ out2) {
    __shared__ unsigned long long s_part[4];
    NormAcc<NORM> acc;
    const int first = threadIdx.x * 8;
    for (int k = first; k < first + 8 && k < parts; ++k) acc.merge(ws[k]);
    block_reduce(acc, s_part);
    if (threadIdx.x == 0) {
        const float norm = (float)(fabs((double)grad_scale) * acc.norm());
        float coef = (1.0f / (norm + 1e-6f)) * max_norm;
        coef = coef != coef ? coef : (coef < 1.0f ? coef : 1.0f);
        out2[0] = norm;
        out2[1] = grad_scale * coef;
    }
}

static bool norm_arena_ok(size_t n) { return n > 0 && n % 4 == 0 && n / 4 <= 0xFFFFFFFFull - 511; }

// Validates the caller's span table against the arena (n floats) and packs it; spans == NULL with n_spans == 0 is [0, n).
static bool fill_span_table(SpanTable& tab, const osi_grad_span* spans, int n_spans, size_t n) {
    memset(&tab, 0, sizeof tab);
    if (!spans) {
        if (n_spans != 0) return false;
        tab.begin[0] = 0; tab.end[0] = (uint32_t)(n / 4); tab.last[0] = 4; tab.n = 1;
        return true;
    }
    if (n_spans < 1 || n_spans > OSI_OPT_MAX_SEGMENTS) return false;
    unsigned long long prev_end = 0;
    for (int i = 0; i < n_spans; ++i) {
        const unsigned long long b = spans[i].begin, m = spans[i].numel;
        if (b % 4 != 0 || m < 1 || b < prev_end || b >= n || m > n - b) return false;
        tab.begin[i] = (uint32_t)(b / 4); tab.end[i] = (uint32_t)((b + m + 3) / 4); tab.last[i] = (uint8_t)(m % 4 ? m % 4 : 4);
        prev_end = b + m;
    }
    tab.n = n_spans;
    return true;
}

// The per-group scalars of osi_*_step_groups(_dev), prepared in double; false = a refused option.
static bool fill_adam_groups(AdamGroups& gs, const osi_adam_group* groups, int n_groups, const float* max_exp_avg_sq) {
    memset(&gs, 0, sizeof gs);
    for (int i = 0; i < n_groups; ++i) {
        const osi_adam_group& u = groups[i];
        if (!(u.step >= 1 && (!u.amsgrad || max_exp_avg_sq))) return false;
        const double bc1 = 1.0 - pow(u.beta1, (double)u.step);
        const double bc2 = 1.0 - pow(u.beta2, (double)u.step);
        gs.g[i] = AdamScal{(float)(u.lr / bc1), (float)sqrt(bc2), (float)u.beta2, (float)(1.0 - u.beta1), (float)(1.0 - u.beta2),
                           (float)u.eps, (float)u.weight_decay, (float)(1.0 - u.lr * u.weight_decay),
                           (u.decoupled ? OPT_DECOUPLED : 0u) | (u.amsgrad ? OPT_AMSGRAD : 0u) | (u.maximize ? OPT_MAXIMIZE : 0u)};
    }
    return true;
}
static bool fill_sgd_groups(SgdGroups& gs, const osi_sgd_group* groups, int n_groups) {
    memset(&gs, 0, sizeof gs);
    for (int i = 0; i < n_groups; ++i) {
        const osi_sgd_group& u = groups[i];
        if (!(!u.nesterov || (u.momentum > 0.0 && u.dampening == 0.0))) return false;
        gs.g[i] = SgdScal{(float)u.lr, (float)u.momentum, (float)(1.0 - u.dampening), (float)u.weight_decay,
                          (u.nesterov ? OPT_NESTEROV : 0u) | (u.maximize ? OPT_MAXIMIZE : 0u) |
                              (u.momentum != 0.0 ? OPT_MOMENTUM | (u.first_step ? OPT_FIRST : 0u) : 0u)};
    }
    return true;
}

// GS = float (the scalar by value) or const float* (in device memory): one host path for both forms of the grouped steps
template <class GS>
static int adam_groups_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                              const osi_opt_segment* segments, int n_segments, const osi_adam_group* groups, int n_groups, GS gs_arg,
                              osi_stream_t stream) {
    OSI_REQUIRE(param && grad && exp_avg && exp_avg_sq && groups);
    SegTable tab;
    OSI_REQUIRE(fill_seg_table(tab, segments, n_segments, n_groups, n));
    AdamGroups gs;
    OSI_REQUIRE(fill_adam_groups(gs, groups, n_groups, max_exp_avg_sq));
    uint32_t chunk4;
    const int grid = chunk_grid(n / 4, chunk4);
    hipLaunchKernelGGL(k_adam_groups<GS>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (f32x4*)param, (const f32x4*)grad,
                       (f32x4*)exp_avg, (f32x4*)exp_avg_sq, (f32x4*)max_exp_avg_sq, (uint32_t)(n / 4), chunk4, gs_arg, tab, gs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}
template <class GS>
static int sgd_groups_launch(float* param, const float* grad, float* momentum_buf, size_t n, const osi_opt_segment* segments,
                             int n_segments, const osi_sgd_group* groups, int n_groups, GS gs_arg, osi_stream_t stream) {
    OSI_REQUIRE(param && grad && momentum_buf && groups);
    SegTable tab;
    OSI_REQUIRE(fill_seg_table(tab, segments, n_segments, n_groups, n));
    SgdGroups gs;
    OSI_REQUIRE(fill_sgd_groups(gs, groups, n_groups));
    uint32_t chunk4;
    const int grid = chunk_grid(n / 4, chunk4);
    hipLaunchKernelGGL(k_sgd_groups<GS>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (f32x4*)param, (const f32x4*)grad,
                       (f32x4*)momentum_buf, (uint32_t)(n / 4), chunk4, gs_arg, tab, gs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // namespace

extern "C" {

int osi_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                  double beta2, double eps, long long step, float grad_scale, osi_stream_t stream) {
    OSI_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n % 4 == 0 && step >= 1);
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(k_adam, dim3(sgrid(n / 4)), dim3(256), 0, (hipStream_t)stream, (f32x4*)param, (const f32x4*)grad,
                       (f32x4*)exp_avg, (f32x4*)exp_avg_sq, n / 4, (float)(lr / bc1), (float)beta2, (float)(1.0 - beta1),
                       (float)(1.0 - beta2), (float)eps, (float)sqrt(bc2), grad_scale);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_sgd_step(float* param, const float* grad, float* momentum_buf, size_t n, float lr, float momentum, int first_step,
                 float grad_scale, osi_stream_t stream) {
    OSI_REQUIRE(param && grad && momentum_buf && n > 0 && n % 4 == 0);
    hipLaunchKernelGGL(k_sgd, dim3(sgrid(n / 4)), dim3(256), 0, (hipStream_t)stream, (f32x4*)param, (const f32x4*)grad,
                       (f32x4*)momentum_buf, n / 4, lr, momentum, first_step, grad_scale);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_adam_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                         const osi_opt_segment* segments, int n_segments, const osi_adam_group* groups, int n_groups,
                         float grad_scale, osi_stream_t stream) {
    return adam_groups_launch<float>(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, segments, n_segments, groups, n_groups,
                                     grad_scale, stream);
}

int osi_sgd_step_groups(float* param, const float* grad, float* momentum_buf, size_t n, const osi_opt_segment* segments,
                        int n_segments, const osi_sgd_group* groups, int n_groups, float grad_scale, osi_stream_t stream) {
    return sgd_groups_launch<float>(param, grad, momentum_buf, n, segments, n_segments, groups, n_groups, grad_scale, stream);
}

int osi_adam_step_groups_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                             const osi_opt_segment* segments, int n_segments, const osi_adam_group* groups, int n_groups,
                             const float* grad_scale_dev, osi_stream_t stream) {
    OSI_REQUIRE(grad_scale_dev && ((uintptr_t)grad_scale_dev & 3) == 0);
    return adam_groups_launch<const float*>(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, n, segments, n_segments, groups,
                                            n_groups, grad_scale_dev, stream);
}

int osi_sgd_step_groups_dev(float* param, const float* grad, float* momentum_buf, size_t n, const osi_opt_segment* segments,
                            int n_segments, const osi_sgd_group* groups, int n_groups, const float* grad_scale_dev,
                            osi_stream_t stream) {
    OSI_REQUIRE(grad_scale_dev && ((uintptr_t)grad_scale_dev & 3) == 0);
    return sgd_groups_launch<const float*>(param, grad, momentum_buf, n, segments, n_segments, groups, n_groups, grad_scale_dev, stream);
}

size_t osi_grad_norm_workspace(size_t n) {
    if (!norm_arena_ok(n)) return 0;
    uint32_t chunk4;
    return (size_t)chunk_grid(n / 4, chunk4) * sizeof(unsigned long long);
}

int osi_grad_clip_scale(const float* grad, size_t n, const osi_grad_span* spans, int n_spans, int norm_type, float grad_scale,
                        float max_norm, void* ws, size_t ws_bytes, float* out2, osi_stream_t stream) {
    OSI_REQUIRE(grad && ws && out2 && norm_arena_ok(n));
    OSI_REQUIRE(((uintptr_t)grad & 15) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)out2 & 3) == 0);
    OSI_REQUIRE(ws_bytes >= osi_grad_norm_workspace(n));
    OSI_REQUIRE(norm_type == OSI_NORM_L2 || norm_type == OSI_NORM_INF);
    OSI_REQUIRE(max_norm >= 0.0f && std::isfinite(grad_scale));      // a NaN max_norm fails the comparison
    SpanTable tab;
    OSI_REQUIRE(fill_span_table(tab, spans, n_spans, n));
    uint32_t chunk4;
    const int grid = chunk_grid(n / 4, chunk4);
    unsigned long long* parts = (unsigned long long*)ws;
    if (norm_type == OSI_NORM_L2) {
        hipLaunchKernelGGL(k_grad_norm<OSI_NORM_L2>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)grad,
                           (uint32_t)(n / 4), chunk4, tab, parts);
        OSI_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_grad_norm_final<OSI_NORM_L2>, dim3(1), dim3(256), 0, (hipStream_t)stream, parts, grid, grad_scale,
                           max_norm, out2);
    } else {
        hipLaunchKernelGGL(k_grad_norm<OSI_NORM_INF>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)grad,
                           (uint32_t)(n / 4), chunk4, tab, parts);
        OSI_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_grad_norm_final<OSI_NORM_INF>, dim3(1), dim3(256), 0, (hipStream_t)stream, parts, grid, grad_scale,
                           max_norm, out2);
    }
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_fill_f32(float* p, size_t n, float value, osi_stream_t stream) {
    OSI_REQUIRE(p && n > 0 && n % 4 == 0);
    hipLaunchKernelGGL(k_fill, dim3(sgrid(n / 4)), dim3(256), 0, (hipStream_t)stream, (f32x4*)p, n / 4, value);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}
int osi_scale_f32(float* p, size_t n, float s, osi_stream_t stream) {
    OSI_REQUIRE(p && n > 0 && n % 4 == 0);
    hipLaunchKernelGGL(k_scale, dim3(sgrid(n / 4)), dim3(256), 0, (hipStream_t)stream, (f32x4*)p, n / 4, s);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}
int osi_grad_accumulate(float* dst, const float* src, size_t n, osi_stream_t stream) {
    OSI_REQUIRE(dst && src && dst != src && n > 0 && n % 4 == 0);
    OSI_REQUIRE(((uintptr_t)dst & 15) == 0 && ((uintptr_t)src & 15) == 0);
    hipLaunchKernelGGL(k_accumulate, dim3(sgrid(n / 4)), dim3(256), 0, (hipStream_t)stream, (f32x4*)dst, (const f32x4*)src, n / 4);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}
int osi_average_update(const osi_avg_span* spans, int n_spans, float weight, osi_stream_t stream) {
    OSI_REQUIRE(spans && n_spans >= 1 && n_spans <= OSI_AVG_MAX_SPANS);
    OSI_REQUIRE(weight >= 0.0f && weight <= 1.0f);                   // a NaN fails both comparisons
    AvgTable tab;
    memset(&tab, 0, sizeof tab);
    uint32_t tiles = 0;
    for (int i = 0; i < n_spans; ++i) {
        const osi_avg_span& s = spans[i];
        OSI_REQUIRE(s.avg && s.cur && ((uintptr_t)s.avg & 15) == 0 && ((uintptr_t)s.cur & 15) == 0);
        OSI_REQUIRE(norm_arena_ok(s.n));                             // n > 0, n % 4 == 0, n/4 <= 2^32 - 512
        const uintptr_t a0 = (uintptr_t)s.avg, a1 = a0 + s.n * sizeof(float);
        for (int j = 0; j < n_spans; ++j) {                          // an avg range meets no cur range and no other avg range
            const uintptr_t c0 = (uintptr_t)spans[j].cur, c1 = c0 + spans[j].n * sizeof(float);
            OSI_REQUIRE(a1 <= c0 || c1 <= a0);
            const uintptr_t b0 = (uintptr_t)spans[j].avg, b1 = b0 + spans[j].n * sizeof(float);
            OSI_REQUIRE(j == i || a1 <= b0 || b1 <= a0);
        }
        tab.avg[i] = (f32x4*)s.avg; tab.cur[i] = (const f32x4*)s.cur; tab.n4[i] = (uint32_t)(s.n / 4);
        tiles += (uint32_t)((s.n + AVG_TILE - 1) / AVG_TILE);
        tab.tile_end[i] = tiles;
    }
    tab.n = n_spans;
    const uint32_t grid = tiles < AVG_MAX_GRID ? tiles : AVG_MAX_GRID;
    if (weight < 0.5f)
        hipLaunchKernelGGL(k_average<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tab, weight);
    else
        hipLaunchKernelGGL(k_average<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, tab, weight - 1.0f);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}
int osi_i64_add(long long* p, int n, long long inc, osi_stream_t stream) {
    OSI_REQUIRE(p && n > 0);
    hipLaunchKernelGGL(k_i64_add, dim3(osi_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, p, n, inc);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
