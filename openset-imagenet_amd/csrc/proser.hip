// PROSER (Zhou, Ye, Zhan: "Learning Placeholders for Open-Set Recognition", CVPR 2021) on the device; include/osi.h (ABI 23) is the
// definition, tests/proser_oracle.py its fp64 restatement.
//   osi_mix_rows_pairs       manifold mixup as an in-place pairwise mix of the rows of one activation tensor (the executor runs it on the
//                            input of the first trainable unit: osi_resnet50_set_mix)
//   osi_proser_loss_fwd_bwd  the three-term cross-entropy over [logits, max dummy] and its gradients, one launch
//   osi_proser_scores        softmax([logits, max dummy + bias]): the unknown class in the last column
// No floating-point atomics and fixed summation orders: the same bits on every run.
#include "osi_common.h"

namespace {

// ---- the mix -------------------------------------------------------------------------------------------------------------------------
// A row i with i < partner[i] < B OWNS the pair (i, partner[i]). The s-th owner in row order is served by the workgroups of slot s; the
// launch has floor(B / 2) slots, which is every pair of an involution (a table that is none may leave owners unserved and may race on the
// values; it never leaves the buffer). A slot's workgroups walk the row in tiles of MIX_TILE 16-byte units: every lane loads its unit of
// both rows (MIX_UNROLL units per row in flight), mixes, and stores both — each element is read once and written once, in place.
constexpr int MIX_THREADS = 256;
constexpr int MIX_UNROLL = 4;
constexpr int MIX_TILE = MIX_THREADS * MIX_UNROLL;   // 16-byte units per workgroup tile and row (16 KiB)
constexpr int MIX_MAX_BLOCKS = 8192;                 // grid cap: the tiles beyond it are walked in a grid stride

// x' = fma(w, x, (1 - w) * y): 1 - w rounded once (by the caller), the product rounded once, then the fma
__device__ __forceinline__ f32x4 mix4(float w, float omw, f32x4 x, f32x4 y) {
#pragma clang fp contract(off)
    const f32x4 t = omw * y;
    f32x4 r;
    r.x = __builtin_fmaf(w, x.x, t.x); r.y = __builtin_fmaf(w, x.y, t.y); r.z = __builtin_fmaf(w, x.z, t.z); r.w = __builtin_fmaf(w, x.w, t.w);
    return r;
}

// the s-th owner row in row order, -1 when there are fewer: the same value in every lane of the wave (each wave searches for itself:
// B / 64 ballots, no LDS, no barrier)
__device__ __forceinline__ int mix_owner(const int* __restrict__ partner, int B, int s) {
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < B; base += 64) {
        const int r = base + lane;
        const int j = r < B ? partner[r] : -1;
        const bool own = j > r && j < B;
        const unsigned long long m = __ballot(own);
        const int c = __popcll(m);
        if (s < c) {
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            const unsigned long long hit = __ballot(own && rank == s);
            return base + (int)__builtin_ctzll(hit);
        }
        s -= c;
    }
    return -1;
}

__global__ __launch_bounds__(MIX_THREADS) void k_mix_rows_pairs(f32x4* __restrict__ x, const int* __restrict__ partner,
                                                               const float* __restrict__ weight, int B, size_t L4, unsigned gx) {
    const unsigned slot = blockIdx.x / gx, t0 = blockIdx.x - slot * gx;
    const int i = __builtin_amdgcn_readfirstlane(mix_owner(partner, B, (int)slot));
    if (i < 0) return;
    const int j = __builtin_amdgcn_readfirstlane(partner[i]);    // i < j < B: checked by mix_owner
    const float wi = weight[i], wj = weight[j];
    const float omwi = 1.0f - wi, omwj = 1.0f - wj;
    f32x4* __restrict__ xi = x + (size_t)i * L4;
    f32x4* __restrict__ xj = x + (size_t)j * L4;
    const size_t tiles = (L4 + MIX_TILE - 1) / MIX_TILE;
    for (size_t t = t0; t < tiles; t += gx) {
        const size_t u0 = t * MIX_TILE + threadIdx.x;
        f32x4 a[MIX_UNROLL], b[MIX_UNROLL];
#pragma unroll
        for (int k = 0; k < MIX_UNROLL; ++k) {
            const size_t u = u0 + (size_t)k * MIX_THREADS;
            if (u < L4) { a[k] = xi[u]; b[k] = xj[u]; }
        }
#pragma unroll
        for (int k = 0; k < MIX_UNROLL; ++k) {
            const size_t u = u0 + (size_t)k * MIX_THREADS;
            if (u < L4) {
                xi[u] = mix4(wi, omwi, a[k], b[k]);
                xj[u] = mix4(wj, omwj, b[k], a[k]);
            }
        }
    }
}

// ---- the loss ------------------------------------------------------------------------------------------------------------------------
constexpr int PL_THREADS = 1024;
constexpr int PL_WAVES = PL_THREADS / 64;

struct ProserP {
    const float* z; const float* d; const long long* y;
    float* loss4; float* dz; float* dd;
    int B, C, D, n_mixed;
    float l0, l1, l2;
};

// (value, index) of the first largest entry of a row of dummy logits; a NaN counts as largest (torch.max): wave-wide
__device__ __forceinline__ void dummy_argmax(const float* __restrict__ dr, int D, int lane, float& m, int& a) {
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    bool bn = false;
    for (int c = lane; c < D; c += 64) {        // ascending per lane: a strict compare keeps the first
        const float v = dr[c];
        const bool vn = v != v;
        if (bi == 0x7fffffff || (!bn && (vn || v > bv))) { bv = v; bi = c; bn = vn; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const bool on = ov != ov;
        const bool valid = oi != 0x7fffffff, mine = bi != 0x7fffffff;
        bool take;
        if (!valid) take = false;
        else if (!mine) take = true;
        else if (on != bn) take = on;
        else if (on) take = oi < bi;
        else take = ov > bv || (ov == bv && oi < bi);
        if (take) { bv = ov; bi = oi; bn = on; }
    }
    m = bv; a = bi;
}

// One workgroup for the batch, a wave per row. The batch-level count (the clean rows with a label inside [0, C)) comes from a first sweep
// over the labels alone; with it every row's terms and its finished gradient come out of ONE sweep over the logits. The three sums are
// added in a fixed order: per wave in row order (double), then the waves in index order.
__global__ __launch_bounds__(PL_THREADS) void k_proser_loss(ProserP p) {
    __shared__ int cnt_s[PL_WAVES];
    __shared__ double red[3][PL_WAVES];
    __shared__ int s_n2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = p.C, D = p.D;

    int cnt = 0;
    for (int i = p.n_mixed + (int)threadIdx.x; i < p.B; i += PL_THREADS) {
        const long long yi = p.y[i];
        cnt += yi >= 0 && yi < C;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < PL_WAVES; ++k) t += cnt_s[k];
        s_n2 = t;
    }
    __syncthreads();
    const int n1 = p.n_mixed, n2 = s_n2;
    const float c1 = n1 ? p.l0 / (float)n1 : 0.f;
    const float c2 = n2 ? p.l1 / (float)n2 : 0.f, c3 = n2 ? p.l2 / (float)n2 : 0.f;

    double s1 = 0, s2 = 0, s3 = 0;
    for (int i = wave; i < p.B; i += PL_WAVES) {
        const float* zr = p.z + (size_t)i * C;
        const float* dr = p.d + (size_t)i * D;
        const bool mixed = i < n1;
        const long long yl = p.y[i];
        const bool lab_ok = yl >= 0 && yl < C;
        const int y = lab_ok && !mixed ? (int)yl : -1;     // the column the third term leaves out; -1: none
        const bool counts = mixed || lab_ok;
        float m; int a;
        dummy_argmax(dr, D, lane, m, a);
        float mx = -__builtin_inff(), mx2 = -__builtin_inff();     // over e, and over e without column y
        for (int c = lane; c < C; c += 64) {
            const float v = zr[c];
            mx = osi_max(mx, v);
            if (c != y) mx2 = osi_max(mx2, v);
        }
        mx = osi_max(wave_max(mx), m); mx2 = osi_max(wave_max(mx2), m);
        float se = 0.f, se2 = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float v = zr[c];
            se += expf(v - mx);
            if (c != y) se2 += expf(v - mx2);
        }
        se = wave_sum(se) + expf(m - mx); se2 = wave_sum(se2) + expf(m - mx2);
        // lse(e) - v as (max - v) + log(sum): the difference first, so a large common magnitude of the logits costs no digits
        const float lg = logf(se), lg2 = logf(se2);
        if (mixed) s1 += (double)((mx - m) + lg);
        else if (lab_ok) { s2 += (double)((mx - zr[y]) + lg); s3 += (double)((mx2 - m) + lg2); }
        if (!p.dz) continue;
        // gradient row: g = c1 * (s - onehot(C)) for a mixed row, c2 * (s - onehot(y)) + c3 * (s' - onehot(C)) with s'_y = 0 for a clean
        // one; a row without a term is an exact zero row by a select, whatever its logits hold
        float* gz = p.dz + (size_t)i * C;
        float* gd = p.dd + (size_t)i * D;
        // softmax entries as exp(v - max) / sum (not exp(v - lse): the rounding of lse would scale every entry of the row)
        const float ca = mixed ? c1 : c2, cb = mixed ? 0.f : c3;
        const float ka = ca / se, kb = cb / se2;
        for (int c = lane; c < C; c += 64) {
            const float v = zr[c];
            float g = ka * expf(v - mx);
            if (!mixed) g = c == y ? g - ca : g + kb * expf(v - mx2);
            gz[c] = counts ? g : 0.f;
        }
        const float gm = mixed ? ka * expf(m - mx) - ca : ka * expf(m - mx) + (kb * expf(m - mx2) - cb);
        for (int c = lane; c < D; c += 64) gd[c] = counts && c == a ? gm : 0.f;
    }
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; red[2][wave] = s3; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0, t2 = 0, t3 = 0;
        for (int k = 0; k < PL_WAVES; ++k) { t1 += red[0][k]; t2 += red[1][k]; t3 += red[2][k]; }
        const float m1 = n1 ? (float)(t1 / n1) : 0.f, m2 = n2 ? (float)(t2 / n2) : 0.f, m3 = n2 ? (float)(t3 / n2) : 0.f;
        // a term without rows is an exact zero, whatever its factor holds
        const float j1 = n1 ? p.l0 * m1 : 0.f, j2 = n2 ? p.l1 * m2 : 0.f, j3 = n2 ? p.l2 * m3 : 0.f;
        p.loss4[0] = j1 + j2 + j3; p.loss4[1] = m1; p.loss4[2] = m2; p.loss4[3] = m3;
    }
}

// probs[i] = softmax([z_i, max_d dummy_i + bias]); a wave per row
__global__ __launch_bounds__(256) void k_proser_scores(const float* __restrict__ z, const float* __restrict__ d, float bias, int B, int C,
                                                      int D, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;
    const float* zr = z + (size_t)i * C;
    const float* dr = d + (size_t)i * D;
    float m = -__builtin_inff();
    for (int c = lane; c < D; c += 64) m = osi_max(m, dr[c]);
    m = wave_max(m) + bias;
    float mx = -__builtin_inff();
    for (int c = lane; c < C; c += 64) mx = osi_max(mx, zr[c]);
    mx = osi_max(wave_max(mx), m);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(zr[c] - mx);
    const float em = expf(m - mx);
    se = wave_sum(se) + em;
    float* o = out + (size_t)i * (C + 1);
    for (int c = lane; c < C; c += 64) o[c] = expf(zr[c] - mx) / se;
    if (lane == 0) o[C] = em / se;
}

}  // namespace

extern "C" {

int osi_mix_rows_pairs(float* x, const int* partner, const float* weight, int B, size_t L, osi_stream_t stream) {
    OSI_REQUIRE(x && partner && weight && B > 0 && L > 0 && L % 4 == 0 && ((uintptr_t)x & 15) == 0);
    const unsigned slots = (unsigned)B / 2;
    if (!slots) return OSI_OK;         // a single row has no pair
    const size_t L4 = L / 4, tiles = (L4 + MIX_TILE - 1) / MIX_TILE;
    size_t gx = MIX_MAX_BLOCKS / slots;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    OSI_REQUIRE(gx * slots <= 0x7fffffffull);
    hipLaunchKernelGGL(k_mix_rows_pairs, dim3((unsigned)(gx * slots)), dim3(MIX_THREADS), 0, (hipStream_t)stream, (f32x4*)x, partner, weight,
                       B, L4, (unsigned)gx);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_proser_loss_fwd_bwd(const float* logits, const float* dummy, const long long* target, int B, int C, int D, int n_mixed, float l0,
                            float l1, float l2, float* loss4, float* dlogits, float* ddummy, osi_stream_t stream) {
    OSI_REQUIRE(logits && dummy && target && loss4 && B > 0 && C > 0 && D >= 1);
    OSI_REQUIRE(B <= 15 * 1024 && n_mixed >= 0 && n_mixed <= B);
    OSI_REQUIRE((dlogits == nullptr) == (ddummy == nullptr));
    ProserP p;
    p.z = logits; p.d = dummy; p.y = target; p.loss4 = loss4; p.dz = dlogits; p.dd = ddummy;
    p.B = B; p.C = C; p.D = D; p.n_mixed = n_mixed; p.l0 = l0; p.l1 = l1; p.l2 = l2;
    hipLaunchKernelGGL(k_proser_loss, dim3(1), dim3(PL_THREADS), 0, (hipStream_t)stream, p);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_proser_scores(const float* logits, const float* dummy, float bias, int B, int C, int D, float* probs, osi_stream_t stream) {
    OSI_REQUIRE(logits && dummy && probs && B > 0 && C > 0 && D >= 1);
    hipLaunchKernelGGL(k_proser_scores, dim3(osi_cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, logits, dummy, bias, B, C, D, probs);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
