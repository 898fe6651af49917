// Input gradient of the ResNet stem (conv1: 7x7 / stride 2 / pad 3, 3 -> 64 channels; torchvision.models.resnet50 under reference
// openset_imagenet/model.py:17): dJ/dimage for adversarial samples and input attribution in the training loop. dY is the stem conv's
// output gradient in NHWC [B][Hs][Ws][64], W its weight in the arena layout [64][7][7][3]; dx is written as the reference's input
// layout, NCHW fp32 [B][3][H][W].
//
//   dx[b][c][h][w] = sum_k sum_(r,s) dY[b][(h+3-r)/2][(w+3-s)/2][k] * W[k][r][s][c]   over the taps where h+3-r, w+3-s are even
//
// Each output parity class (h % 2, w % 2) is a stride-1 correlation with a 3x3, 3x4, 4x3 or 4x4 sub-kernel (49 taps over the four
// classes). With 3 output channels there is no matrix shape worth an MFMA; the kernel runs on the vector pipe with packed fp32 FMAs:
//   * a workgroup owns a 32 x 64 pixel tile of dx; wave p is parity class p, so the weights a wave multiplies by are wave-uniform
//     and come from scalar loads (no LDS traffic, no VGPRs);
//   * lane = one row x 8 columns (stride 2) of its class; the dY halo of the tile (19 x 35 pixels) is staged in LDS 16 channels at a
//     time with channel PAIRS innermost, so one 16-byte LDS read gives two columns x two channels and every FMA is a v_pk_fma_f32
//     over (even k, odd k); the two partial sums are added once at the end (fixed order: deterministic, no atomics);
//   * every element of dx is written once, out-of-range pixels of the last tiles are masked; out-of-range dY pixels read as zero
//     through the buffer range check.
//
// Second form (SG_FGSM, osi_stem_dgrad_fgsm): the same K loop, another epilogue. dx is not written at all; the lane already holds
// the three channel sums of each of its pixels, so it loads the clean pixel from the NHWC4 batch the forward read (16 bytes), moves
// each channel by eps along the sign of its gradient, clamps and stores the adversarial pixel into an NHWC4 batch (16 bytes, 4th lane
// zero): one vector store per pixel where the NCHW form needs three scattered 4-byte stores.
//
// Third form (SG_PGD, osi_stem_dgrad_pgd): one step of a projected attack. The lane loads the iterate's pixel AND the anchor's (the clean
// batch: one more 16-byte load), moves the iterate by alpha along the sign, projects onto the eps-ball around the anchor, clamps and stores
// the next iterate. The epilogue is a compile-time mode of the one kernel template: the K loop is the same code in all three.
#include "conv_common.h"

using namespace osi_conv;

namespace {

constexpr int SG_TH = 32, SG_TW = 64;             // dx tile
constexpr int SG_HR = SG_TH / 2 + 3;              // dY halo rows (19)
constexpr int SG_HC = SG_TW / 2 + 3;              // dY halo columns (35)
constexpr int SG_ROW = 36;                        // LDS row pitch in channel pairs (16-byte aligned rows)
constexpr int SG_KC = 16;                         // channels per LDS chunk
constexpr int SG_PLANE = SG_HR * SG_ROW;          // channel pairs per halo plane
constexpr int SG_LDS_F2 = (SG_KC / 2) * SG_PLANE; // 5472 float2 = 43.8 KB
constexpr int SG_NLD = SG_HR * SG_HC * (SG_KC / 4);   // float4 loads per chunk (2660)

// One wave = one parity class (PH, PW). Lane: row i = lane >> 2 of the class, column group q = lane & 3 (8 columns each).
// Taps of the class: r = 1 - PH + 2u (u < 3 + PH) reads halo row i + PH + 2 - u; s = 1 - PW + 2v reads halo column 8q + j + PW + 2 - v.
template <int PH, int PW>
__device__ __forceinline__ void sg_chunk(const f32x2* __restrict__ sd, const float* __restrict__ w, int kc, int i, int q, f32x2 (&acc)[8][3]) {
#pragma unroll 1
    for (int kp = 0; kp < SG_KC / 2; ++kp) {
        const int k = kc + 2 * kp;
        const float* w0 = w + k * 147;            // W[k][.][.][.], wave-uniform
        const float* w1 = w0 + 147;               // W[k + 1]
#pragma unroll
        for (int u = 0; u < 3 + PH; ++u) {
            const int r = 1 - PH + 2 * u;
            const f32x2* row = sd + kp * SG_PLANE + (i + PH + 2 - u) * SG_ROW + 8 * q;
            f32x2 d[12];
#pragma unroll
            for (int x = 0; x < 12; x += 2) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + x);
                d[x] = f32x2{v[0], v[1]};
                d[x + 1] = f32x2{v[2], v[3]};
            }
#pragma unroll
            for (int v = 0; v < 3 + PW; ++v) {
                const int s = 1 - PW + 2 * v, t = PW + 2 - v;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x2 wv = f32x2{w0[(r * 7 + s) * 3 + c], w1[(r * 7 + s) * 3 + c]};
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j][c] = __builtin_elementwise_fma(d[j + t], wv, acc[j][c]);
                }
            }
        }
    }
}

enum : int { SG_NCHW = 0, SG_FGSM = 1, SG_PGD = 2 };   // epilogue of k_stem_dgrad

template <int MODE>
__global__ __launch_bounds__(256) void k_stem_dgrad(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                    int H, int W, int Hs, int Ws, int tiles_x, int tiles_y, int dy_bytes,
                                                    const float* __restrict__ x4, float eps, float lo, float hi,
                                                    const float* __restrict__ xa4, float alpha) {
    __shared__ __attribute__((aligned(16))) f32x2 sd[SG_LDS_F2];   // read as 16-byte vectors (ds_read_b128)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ph = wave >> 1, pw = wave & 1;
    const int i = lane >> 2, q = lane & 3;
    const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
    const int h0 = ty * SG_TH, w0 = tx * SG_TW;
    const int oy0 = h0 / 2 - 1, ox0 = w0 / 2 - 1;     // halo origin in dY
    const __amdgpu_buffer_rsrc_t rdy = make_rsrc(dy, dy_bytes);
    f32x2 acc[8][3];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] = f32x2{0.f, 0.f};
#pragma unroll 1
    for (int kc = 0; kc < 64; kc += SG_KC) {
        __syncthreads();                               // every wave is done with the previous chunk
        for (int e = tid; e < SG_NLD; e += 256) {
            const int k4 = e & 3, pix = e >> 2;        // 4 consecutive lanes read one pixel's 16 channels (64 contiguous bytes)
            const int py = pix / SG_HC, px = pix - py * SG_HC;
            const int oy = oy0 + py, ox = ox0 + px;
            const bool ok = ((unsigned)oy < (unsigned)Hs) & ((unsigned)ox < (unsigned)Ws);
            const uint32_t off = ok ? (uint32_t)((((size_t)b * Hs + oy) * Ws + ox) * 64 + kc + 4 * k4) * 4u : OOB;
            const f32x4 v = bld4(rdy, off, 0);
            // channels kc + 4 k4 .. + 3 = pairs 2 k4 and 2 k4 + 1 of this chunk
            sd[(2 * k4) * SG_PLANE + py * SG_ROW + px] = f32x2{v[0], v[1]};
            sd[(2 * k4 + 1) * SG_PLANE + py * SG_ROW + px] = f32x2{v[2], v[3]};
        }
        __syncthreads();
        switch (wave) {
            case 0: sg_chunk<0, 0>(sd, w, kc, i, q, acc); break;
            case 1: sg_chunk<0, 1>(sd, w, kc, i, q, acc); break;
            case 2: sg_chunk<1, 0>(sd, w, kc, i, q, acc); break;
            default: sg_chunk<1, 1>(sd, w, kc, i, q, acc); break;
        }
    }
    const int h = h0 + ph + 2 * i;
    if (h >= H) return;
    if constexpr (MODE != SG_NCHW) {
        // dx = the NHWC4 output batch here, the gradient itself stays in registers. FGSM: x_adv = clamp(x + eps * sign(dJ/dx)).
        // PGD: x4 = the iterate, xa4 = the anchor (it may be the iterate itself; both are only read), x_next = clamp(the iterate moved
        // by alpha along the sign, projected onto [anchor - eps, anchor + eps]); alpha * sign is exact, so every line is one rounding
        const size_t row = ((size_t)b * H + h) * W;
        const f32x4* xin = reinterpret_cast<const f32x4*>(x4) + row;
        f32x4* xout = reinterpret_cast<f32x4*>(dx) + row;
        const float step = MODE == SG_PGD ? alpha : eps;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = w0 + pw + 2 * (8 * q + j);
            if (x < W) {
                const f32x4 p = xin[x];
                f32x4 a = p;
                if constexpr (MODE == SG_PGD) a = (reinterpret_cast<const f32x4*>(xa4) + row)[x];
                f32x4 o;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float t = acc[j][c][0] + acc[j][c][1];                    // the sum the NCHW form stores
                    const float sg = (float)((t > 0.f) - (t < 0.f));                // torch.sign
                    float v = p[c] + step * sg;
                    if constexpr (MODE == SG_PGD) v = fminf(fmaxf(v, a[c] - eps), a[c] + eps);
                    o[c] = fminf(hi, fmaxf(lo, v));
                }
                o[3] = 0.f;
                xout[x] = o;
            }
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* out = dx + (((size_t)b * 3 + c) * H + h) * W;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int x = w0 + pw + 2 * (8 * q + j);
            if (x < W) out[x] = acc[j][c][0] + acc[j][c][1];
        }
    }
}

}  // namespace

extern "C" {

int osi_stem_dgrad(const float* dy, const float* w_krsc3, float* dx_nchw, int B, int H, int W, osi_stream_t stream) {
    OSI_REQUIRE(dy && w_krsc3 && dx_nchw && B > 0 && H >= 32 && W >= 32);
    OSI_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w_krsc3 & 3) == 0 && ((uintptr_t)dx_nchw & 3) == 0);
    const int Hs = (H - 1) / 2 + 1, Ws = (W - 1) / 2 + 1;
    const size_t dy_bytes = (size_t)B * Hs * Ws * 64 * sizeof(float);
    OSI_REQUIRE(dy_bytes < ((size_t)1 << 31));        // 32-bit buffer offsets (the executor's tensors obey the same bound)
    const int tiles_x = osi_cdiv(W, SG_TW), tiles_y = osi_cdiv(H, SG_TH);
    const size_t grid = (size_t)B * tiles_x * tiles_y;
    OSI_REQUIRE(grid < ((size_t)1 << 31));
    hipLaunchKernelGGL(k_stem_dgrad<SG_NCHW>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, dy, w_krsc3, dx_nchw, H, W, Hs, Ws,
                       tiles_x, tiles_y, (int)dy_bytes, (const float*)nullptr, 0.f, 0.f, 0.f, (const float*)nullptr, 0.f);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_stem_dgrad_fgsm(const float* dy, const float* w_krsc3, const float* x_nhwc4, float* x_adv_nhwc4, float eps, float lo, float hi,
                        int B, int H, int W, osi_stream_t stream) {
    OSI_REQUIRE(dy && w_krsc3 && x_nhwc4 && x_adv_nhwc4 && B > 0 && H >= 32 && W >= 32);
    OSI_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w_krsc3 & 3) == 0);
    OSI_REQUIRE(((uintptr_t)x_nhwc4 & 15) == 0 && ((uintptr_t)x_adv_nhwc4 & 15) == 0);
    OSI_REQUIRE(eps >= 0.f && lo <= hi);              // (a NaN fails both comparisons)
    const int Hs = (H - 1) / 2 + 1, Ws = (W - 1) / 2 + 1;
    const size_t dy_bytes = (size_t)B * Hs * Ws * 64 * sizeof(float);
    OSI_REQUIRE(dy_bytes < ((size_t)1 << 31));
    // the two batches may not overlap: a workgroup reads clean pixels other workgroups may already have replaced
    const size_t img_bytes = (size_t)B * H * W * 4 * sizeof(float);
    const uintptr_t xa = (uintptr_t)x_nhwc4, xb = (uintptr_t)x_adv_nhwc4;
    OSI_REQUIRE(xa + img_bytes <= xb || xb + img_bytes <= xa);
    const int tiles_x = osi_cdiv(W, SG_TW), tiles_y = osi_cdiv(H, SG_TH);
    const size_t grid = (size_t)B * tiles_x * tiles_y;
    OSI_REQUIRE(grid < ((size_t)1 << 31));
    hipLaunchKernelGGL(k_stem_dgrad<SG_FGSM>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, dy, w_krsc3, x_adv_nhwc4, H, W, Hs, Ws,
                       tiles_x, tiles_y, (int)dy_bytes, x_nhwc4, eps, lo, hi, (const float*)nullptr, 0.f);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_stem_dgrad_pgd(const float* dy, const float* w_krsc3, const float* x_cur_nhwc4, const float* x_anchor_nhwc4, float* x_next_nhwc4,
                       float alpha, float eps, float lo, float hi, int B, int H, int W, osi_stream_t stream) {
    OSI_REQUIRE(dy && w_krsc3 && x_cur_nhwc4 && x_anchor_nhwc4 && x_next_nhwc4 && B > 0 && H >= 32 && W >= 32);
    OSI_REQUIRE(((uintptr_t)dy & 15) == 0 && ((uintptr_t)w_krsc3 & 3) == 0);
    OSI_REQUIRE(((uintptr_t)x_cur_nhwc4 & 15) == 0 && ((uintptr_t)x_anchor_nhwc4 & 15) == 0 && ((uintptr_t)x_next_nhwc4 & 15) == 0);
    OSI_REQUIRE(eps >= 0.f && lo <= hi);              // (a NaN fails both comparisons; eps = +inf: no projection)
    OSI_REQUIRE(alpha - alpha == 0.f);                // finite, either sign (negative descends)
    const int Hs = (H - 1) / 2 + 1, Ws = (W - 1) / 2 + 1;
    const size_t dy_bytes = (size_t)B * Hs * Ws * 64 * sizeof(float);
    OSI_REQUIRE(dy_bytes < ((size_t)1 << 31));
    // the next iterate may overlap neither batch it is made from (the anchor may BE the iterate: step 0 of an attack)
    const size_t img_bytes = (size_t)B * H * W * 4 * sizeof(float);
    const uintptr_t xn = (uintptr_t)x_next_nhwc4;
    for (const float* src : {x_cur_nhwc4, x_anchor_nhwc4}) {
        const uintptr_t xs = (uintptr_t)src;
        OSI_REQUIRE(xs + img_bytes <= xn || xn + img_bytes <= xs);
    }
    const int tiles_x = osi_cdiv(W, SG_TW), tiles_y = osi_cdiv(H, SG_TH);
    const size_t grid = (size_t)B * tiles_x * tiles_y;
    OSI_REQUIRE(grid < ((size_t)1 << 31));
    hipLaunchKernelGGL(k_stem_dgrad<SG_PGD>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, dy, w_krsc3, x_next_nhwc4, H, W, Hs, Ws,
                       tiles_x, tiles_y, (int)dy_bytes, x_cur_nhwc4, eps, lo, hi, x_anchor_nhwc4, alpha);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

}  // extern "C"
