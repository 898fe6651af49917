// Shared device/host helpers for the gfx950 kernels of the open-set ImageNet hot path.
// Everything here is CDNA4-only (wave64, MFMA f32 32x32x2); there is no other backend.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/osi.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define OSI_LAUNCH_CHECK()                                     \
    do {                                                       \
        hipError_t e__ = hipGetLastError();                    \
        if (e__ != hipSuccess) return OSI_ERR_LAUNCH;          \
    } while (0)

#define OSI_REQUIRE(cond)                                      \
    do {                                                       \
        if (!(cond)) return OSI_ERR_ARG;                       \
    } while (0)

// Process-wide tuning knobs (development A/B switches). Written only by osi_set_tuning() (abi.hip); launch functions read them
// and never touch the environment, so they stay stateless and re-entrant as include/osi.h promises. Defaults = measured optimum.
// THE list: one row per knob, X(name, default, lo, hi, plan_relevant). The fields of OsiTuning and their defaults, the name lookup and
// range check of osi_set_tuning / osi_tuning_info (abi.hip) and the executor's plan_unchanged() (resnet50_exec.hip) are generated from
// it; the Python binding reads it through osi_tuning_info, and tests/test_abi.py holds the table in include/osi.h to it.
// plan_relevant: an executor sizes its workspace for the value in force at create and refuses to run under another one.
#define OSI_TUNING_KNOBS(X)                                                                                                              \
    X(wgrad_tile, 0, 0, 64, 1)        /* 64 forces 64x64 weight-gradient tiles, 0 = 128-wide tiles wherever the channel counts allow (0 or 64 only: osi_set_tuning) */ \
    X(wgrad_blocks, 2048, 1, 1 << 20, 1)   /* split-K footprint budget of one weight-gradient launch, in 64x64-workgroup units */       \
    X(wgrad_nst, 1, 1, 2, 0)          /* LDS stages of the weight-gradient kernel (1 or 2) */                                           \
    X(bn_grid, 1024, 1, 1 << 20, 0)   /* grid cap of the BatchNorm stream kernels */                                                    \
    X(bn_single_p, 128, 1, 1 << 20, 0)     /* BatchNorm statistics: row-tile partials merged by ONE launch up to this count, two-level above it */ \
    X(wgrad3, 2, 0, 2, 1)             /* 0 = per-tap kernel everywhere, 1 = 3x3 stride-1 weight gradients use the all-taps kernel (k_conv_wgrad3), 2 = stride 2 too */ \
    X(wgrad3_blocks, 768, 1, 1 << 20, 1)   /* workgroups per launch the all-taps kernel's split-K plan aims for */                      \
    X(fwd_wide, 0, 0, 1, 0)           /* A/B: 64x128 forward tiles wherever the channel count allows (default 0: measured rule) */      \
    X(dgrad_wide, 0, 0, 1, 0)         /* A/B: the same for the input gradient */                                                        \
    X(wgrad_group, 2, 0, 2, 1)        /* weight-gradient block -> XCD mapping: 0 plain 2-D grid, 1 the R*S taps of a cell share an XCD, 2 whole K splits do */ \
    X(tail_split, 1, 0, 1, 1)         /* 1 = forward / input-gradient launches split the tiles of their ragged last round along K (plan_tail_split) */ \
    X(tail_cus, 0, 0, 4096, 1)        /* CU count the tail plan balances for; 0 = ask the device (256 on MI355X) */                     \
    X(tail_smax, 8, 1, 64, 1)         /* most K splits a remainder tile is cut into */                                                  \
    X(tail_mint, 16, 1, 4096, 1)      /* fewest K tiles (of 32) a split keeps */                                                        \
    X(stem_direct, 1, 0, 1, 1)        /* 1 = the stem convolution runs its direct form (k_stem_fwd_direct) where the geometry allows, 0 = implicit GEMM */ \
    X(tail_gain, 8, 0, 100, 1)        /* balanced remainder: least modelled gain of a launch, in percent, for its ragged round to be split */ \
    X(tail_qmax, 8, 0, 4096, 1)       /* ... and most full rounds a launch may have */                                                  \
    X(bn_grid_bwd, 1024, 1, 1 << 20, 0)    /* grid cap of the BatchNorm BACKWARD apply kernels (they run beside the weight gradients) */ \
    X(bn_wide_p, 2048, 0, 2048, 0)    /* BatchNorm finalisation (forward statistics and backward sums): ONE 1024-thread launch up to this many partials */ \
    X(fwd_rows, 1, 0, 2, 0)           /* fwd: 1x1 stride-1 convolutions with Cin = 64 / 128 on the persistent row walker (k_conv1x1_rows): 0 off, 1 Cin = 64 at >= 8 row tiles per CU, 2 every eligible shape (tests) */ \
    X(fwd_w3, 1, 0, 1, 0)             /* fwd: 3x3 stride-1 convolutions stage one activation window per tap row (k_conv_fwd W3): 0 off, 1 on */ \
    X(dgrad_w3, 1, 0, 1, 0)           /* dgrad: the same for the in-block fused 3x3 stride-1 input gradients (k_conv_dgrad W3): 0 off, 1 on */ \
    X(fwd_wino, 1, 0, 1, 1)           /* fwd: the executor runs its 3x3 stride-1 convolutions in the Winograd F(2x2,3x3) form (conv_wino.hip): 0 off, 1 on */ \
    X(dgrad_wino, 1, 0, 1, 1)         /* dgrad: the same for the in-block fused 3x3 stride-1 input gradients */                         \
    X(wgrad_wino, 1, 0, 1, 1)         /* wgrad: the executor's 3x3 stride-1 weight gradients (conv2, fused input activation) in the Winograd F(3x3,2x2) form */ \
    X(wino_wide, 1, 0, 1, 0)          /* Winograd fwd / dgrad: units of 32 tiles x 128 channels where the channel count allows (the patch transform serves 2x the channels) */ \
    X(wino_streamk, 2, 0, 3, 0)       /* Winograd forms: the units of the ragged last round are cut along K over all workgroups (stream-K): 0 = never, 1 = forward and input gradient, 2 = forward only (default), 3 = input gradient only */ \
    X(dp_reserved_cus, 0, 0, 128, 1)  /* CUs' worth of wave slots the launch plans leave to co-resident communication kernels (data parallel); 0 = none */

struct OsiTuning {
#define OSI_KNOB_FIELD(name, def, lo, hi, plan) int name = def;
    OSI_TUNING_KNOBS(OSI_KNOB_FIELD)
#undef OSI_KNOB_FIELD
};
extern OsiTuning g_osi_tuning;

static inline int osi_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- run-time values -> template instances ---------------------------------------------------------------------------------------
// f(Int<V>{}) for the V of the list that equals v, OSI_ERR_ARG when none does: a chain of compares, nothing indirect on the launch path.
// The dispatchers guard every combination with `if constexpr`: only the kernels those conditions name are built.
template <int V> using Int = std::integral_constant<int, V>;
template <int... Vs, class F>
static int pick(int v, F&& f) {
    int r = OSI_ERR_ARG;
    (void)((v == Vs && ((r = f(Int<Vs>{})), true)) || ...);
    return r;
}

// BatchNorm statistics partials as a convolution's forward epilogue writes them and osi_bn_finalize_stats (bn.hip) reads them: [P][C]
// row-tile means, [P][C] M2, then the scratch of the two-level finalisation ([C][S] group means and M2, S <= OSI_BN_GROUPS)
constexpr int OSI_BN_GROUPS = 32;  // level-1 groups of the two-level statistics finalisation
static inline size_t bn_pstats_floats(int P, int C) { return (size_t)2 * P * C + (size_t)2 * OSI_BN_GROUPS * C; }

// Unsigned division by a runtime-constant divisor: q = (n * mul) >> (32 + sh), exact for n < 2^31.
struct FastDiv {
    uint32_t mul, sh, d;
};
static inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    if (d == 1) { f.mul = 0; f.sh = 0; return f; }
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;           // l = ceil(log2 d)
    uint64_t m = ((1ull << (32 + l)) + d - 1) / d;  // ceil(2^(32+l)/d), fits 33 bits
    f.mul = (uint32_t)(m - (1ull << 32));  // low 32 bits; the implicit 2^32 is added back in the divide
    f.sh = l;
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
    uint32_t t = __umulhi(n, f.mul);
    // q = (t + n) >> sh without overflow: ((n - t) >> 1) + t, then >> (sh-1). d == 1 (mul = sh = 0) is a select, not an early
    // return: a branch here, uniform as it is, splits every caller's basic block and with it the compiler's load scheduling
    const uint32_t q = (((n - t) >> 1) + t) >> ((f.sh - 1) & 31);
    return f.d == 1 ? n : q;
}

// Chan/Welford merge of two (count, mean, M2) triples: a <- a (+) b. Exact in the counts, no E[x^2]-E[x]^2 cancellation.
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& sa, float nb, float mb, float sb) {
    if (nb == 0.f) return;
    if (na == 0.f) { na = nb; ma = mb; sa = sb; return; }
    const float n = na + nb, d = mb - ma;
    ma += d * (nb / n);
    sa += sb + d * d * (na * nb / n);
    na = n;
}

// NaN-keeping maximum (IEEE-754-2019 maximum, one v_maximum3_f32): fmaxf returns the other operand for a NaN, which would turn a
// diverged activation into a clean zero at the next ReLU. Non-finite values propagate as in torch (include/osi.h, conventions).
__device__ __forceinline__ float osi_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float osi_relu(float t) { return __builtin_elementwise_maximum(t, 0.f); }
__device__ __forceinline__ f32x4 osi_relu(f32x4 t) { return __builtin_elementwise_maximum(t, f32x4{0.f, 0.f, 0.f, 0.f}); }

// Xor butterflies over the 64 lanes of a wave. a + b == b + a, so every lane ends with the same bits.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Two behaviours towards a NaN, both relied on, hence two names. wave_max KEEPS one (osi_max): a diverged logit reaches the loss as
// a NaN. wave_fmax / wave_fmin SKIP one (fmax / fmin): their callers want the range of the finite values, or find the NaN again in
// the sums that follow.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = osi_max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_fmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_fmin(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
