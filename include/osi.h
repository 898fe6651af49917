/*
 * osi.h — C ABI of libosi_hip.so: the MI355X (gfx950) implementation of the open-set ImageNet training hot path.
 *
 * The reference (AIML-IfI/openset-imagenet) is pure Python and has no operator / plugin / FFI layer of its own
 * (SURVEY.md §8b); the arithmetic it runs lives in torch / torchvision calls. Each entry point below therefore cites
 * the reference CALL SITE whose arithmetic it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - plain C: raw device pointers, ints, floats, one opaque stream handle (a hipStream_t); no torch types.
 *   - every function returns OSI_OK (0) or a negative OSI_ERR_* code; nothing throws across the ABI.
 *   - no allocation, no host synchronisation, no implicit stream: the caller owns every buffer (workspace sizes
 *     come from the matching *_workspace query) and passes the stream to launch on. Launch functions are
 *     re-entrant and safe to capture into a hipGraph.
 *   - activations are fp32 NHWC ([B][H][W][C], C contiguous); conv weights are fp32 KRSC ([Cout][R][S][Cin]) —
 *     byte-identical to a torch OIHW tensor kept in channels_last strides, which is how the Python module owns them.
 *   - all pointers must be 16-byte aligned; channel counts must be multiples of 4 (64 for conv GEMM dimensions).
 *   - non-finite values propagate as in torch: given the same NaN / +-Inf inputs, the SET of non-finite output elements of every
 *     entry point equals that of the torch fp64 reference of the same operation, and every finite output element keeps the accuracy
 *     it has on finite inputs. Every ReLU, variance clamp, pooling comparison and row maximum keeps a NaN (IEEE-754-2019 maximum,
 *     not fmaxf): relu(NaN) = NaN, a BatchNorm channel holding one NaN / Inf gets non-finite statistics and a NaN output, a pooling
 *     window holding a NaN gives NaN and its index names a NaN element. Which non-finite value comes out (NaN or +-Inf) is not
 *     specified (the Winograd transforms turn Inf - Inf into NaN). Not specified either: (a) a non-finite value multiplied by a
 *     structural zero (padding taps, rows past M, the fourth stem channel); (b) which NaN of a pooling window the index names when
 *     it holds several; (c) the backward gate of an element whose forward activation was NaN (mask bit, bit 7 of the pool index,
 *     recomputed gate: closed here, open in torch; the upstream gradient of a real step is NaN by then). A gate that is closed
 *     takes its element out by a select: a NaN gradient behind it does not spread.
 */
#ifndef OSI_H
#define OSI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSI_OK 0
#define OSI_ERR_ARG (-1)    /* shape / pointer / alignment precondition violated; nothing was launched */
#define OSI_ERR_LAUNCH (-2) /* the HIP runtime refused a launch or an attribute */
#define OSI_ERR_STATE (-3)  /* executor called out of order (backward before forward, wrong batch, ...) */

typedef void* osi_stream_t; /* hipStream_t */

int osi_abi_version(void);            /* bumped on any signature change; 22 = the Extreme Value Machine (osi_evm_*); 21 = OpenMax (osi_openmax_*); 20 = weight averaging (osi_average_update) and the executor's BatchNorm momentum (osi_resnet50_set_bn_momentum / _get_bn_momentum); 19 =projected attack steps (osi_stem_dgrad_pgd, osi_resnet50_backward_attack); 18 = evaluation histograms (osi_eval_values_*, osi_hist_*); 17 = gradient-norm clipping (osi_grad_clip_scale, osi_*_step_groups_dev); 16 = the ROC-AUC entry points (osi_auc_*) */
const char* osi_build_arch(void);     /* "gfx950" */
const char* osi_strerror(int code);
/* Process-wide development knobs (A/B measurements; every default is the measured optimum). Launch functions only READ them and never
 * consult the environment. Unknown name or a value outside the knob's range -> OSI_ERR_ARG (nothing is changed). Not to be changed while
 * launches are in flight; an executor (osi_resnet50_create) sizes its workspace for the values in force at create and refuses to run
 * (OSI_ERR_STATE) once a plan-relevant one (marked *) differs. The table below documents the one list the library is built from
 * (OSI_TUNING_KNOBS in csrc/osi_common.h); osi_tuning_info enumerates that list, and tests/test_abi.py holds this table to it.
 *   name             range         default  meaning
 *   wgrad_tile *     0 | 64        0        64 forces 64x64 weight-gradient tiles; 0 = 128-wide wherever the channel counts allow
 *   wgrad_blocks *   1 .. 2^20     2048     split-K footprint budget of one weight-gradient launch, in 64x64-workgroup units
 *   wgrad_nst        1 | 2         1        LDS stages of the per-tap weight-gradient kernel
 *   wgrad_group *    0 .. 2        2        weight-gradient block -> XCD mapping: 0 plain 2-D grid, 1 the taps of a cell share an XCD, 2 whole K splits do
 *   wgrad3 *         0 .. 2        2        all-taps 3x3 weight-gradient kernel: 0 never, 1 stride-1 layers, 2 stride-2 layers too
 *   wgrad3_blocks *  1 .. 2^20     768      workgroups per launch its split-K plan aims for
 *   fwd_wide         0 | 1         0        A/B: 64x128 forward tiles wherever Cout % 128 == 0
 *   fwd_rows         0 .. 2        1        1x1 stride-1 forward convolutions with Cin = 64 on the persistent row walker (weight tile resident in LDS,
 *                                           next row tile prefetched) when the launch has >= 8 row tiles per CU; 2 = every eligible shape (Cin = 64 | 128)
 *   fwd_w3           0 | 1         1        3x3 stride-1 forward convolutions stage ONE activation window per tap row and 32-channel slice (column-
 *                                           padded coordinates, the three taps of the row run from it) instead of one 64-row tile per tap
 *   dgrad_w3         0 | 1         1        the same row windows for the in-block fused 3x3 stride-1 input gradients (dY rows per tap row)
 *   dgrad_wide       0 | 1         0        A/B: 64x128 input-gradient tiles wherever Cin % 128 == 0
 *   fwd_wino *       0 | 1         1        the executor runs its 3x3 stride-1 forward convolutions in the Winograd F(2x2,3x3) form (osi_conv_fwd_wino)
 *   dgrad_wino *     0 | 1         1        the same for the in-block fused 3x3 stride-1 input gradients (osi_conv_dgrad_fused_wino)
 *   wgrad_wino *     0 | 1         1        the executor's 3x3 stride-1 weight gradients in the Winograd F(3x3,2x2) form (osi_conv_wgrad_wino)
 *   wino_wide        0 | 1         1        Winograd forward / input gradient: units of 32 tiles x 128 channels (instead of 64 x 64) where the channel count allows
 *   wino_streamk     0 .. 3        2        Winograd forms: the units of the ragged last round are cut along K over all workgroups (fix-up pass): 0 = whole
 *                                           units only, 1 = forward and input gradient, 2 = forward only, 3 = input gradient only
 *   bn_grid          1 .. 2^20     1024     grid cap of the BatchNorm stream kernels
 *   bn_grid_bwd      1 .. 2^20     1024     the same for the backward apply kernels
 *   bn_single_p      1 .. 2^20     128      BatchNorm partials merged by ONE 256-thread launch up to this many row tiles
 *   bn_wide_p        0 .. 2048     2048     ... by ONE 1024-thread launch up to this many (0 = two levels above bn_single_p)
 *   tail_split *     0 | 1         1        forward / input-gradient launches split the tiles of their ragged last round along K
 *   tail_cus *       0 .. 4096     0        CU count the tail plan balances for; 0 = the device's (minus dp_reserved_cus). Affects ONLY that
 *                                           plan: the stem weight-gradient grid always follows the hardware CU count
 *   tail_smax *      1 .. 64       8        most K splits a remainder tile is cut into
 *   tail_mint *      1 .. 4096     16       fewest K tiles (of 32) a split keeps
 *   tail_gain *      0 .. 100      8        least modelled gain of a launch, in percent, for its ragged round to be split
 *   tail_qmax *      0 .. 4096     8        most full rounds a launch may have and still be split
 *   stem_direct *    0 | 1         1        conv1 runs the direct kernels (forward, weight gradient, fused tail) where the geometry allows
 *   dp_reserved_cus * 0 .. 128     0        data parallel: CUs' worth of wave slots the tail plan leaves to co-resident communication kernels */
int osi_set_tuning(const char* name, int value);
int osi_get_tuning(const char* name, int* value);
/* Row i of the knob list: name (a static string), default, inclusive range, and whether the knob is plan-relevant (* above). Any
 * output pointer may be NULL. OSI_ERR_ARG for i past the end: callers enumerate from 0 until it says so. */
int osi_tuning_info(int i, const char** name, int* def, int* lo, int* hi, int* plan_relevant);

/* ---- convolution (torchvision.models.resnet50 body constructed at openset_imagenet/model.py:17, run at model.py:37) --- */
typedef struct {
    int B, H, W, Cin; /* input  [B][H][W][Cin]   */
    int Ho, Wo, Cout; /* output [B][Ho][Wo][Cout] */
    int R, S, stride, pad;
} osi_conv_desc;

enum { OSI_TILE_AUTO = 0, OSI_TILE_128x128 = 1, OSI_TILE_128x64 = 2, OSI_TILE_64x128 = 3, OSI_TILE_64x64 = 4,
       OSI_TILE_64x64_S1 = 5, OSI_TILE_64x128_S1 = 6, OSI_TILE_128x128_S1 = 7, OSI_TILE_128x64_S1 = 8 /* _S1: single-buffered LDS */ };

/* y = conv2d(x, w), bias-free. The 7x7 stem is described with Cin = 4 (image staged by osi_nchw3_to_nhwc4) and takes
 * weights packed by osi_stem_weight_pack ([Cout][56 taps][4]). Otherwise Cin % 32 == 0, Cout % 64 == 0. */
int osi_conv_fwd(const osi_conv_desc* d, const float* x, const float* w, float* y, int tile, osi_stream_t stream);
/* Same convolution, and the epilogue also emits per-row-tile BatchNorm partials (mean, M2 per channel, *P tiles of
 * *rows_per_block rows) into pstats, to be finished by osi_bn_finalize_stats — the statistics never re-read y from HBM.
 * pstats: osi_conv_fwd_bnstats_workspace(d) bytes = the partials, the scratch of osi_bn_finalize_stats and the slab of a K-split tail
 * (a caller that offers less gets the un-split launch); workspace contents are never assumed. The same holds for pstats of
 * osi_conv_fwd_act / osi_conv_fwd_act2. */
size_t osi_conv_fwd_bnstats_workspace(const osi_conv_desc* d);
int osi_conv_fwd_bnstats(const osi_conv_desc* d, const float* x, const float* w, float* y, int tile, float* pstats,
                         size_t pstats_bytes, int* P, int* rows_per_block, osi_stream_t stream);
/* Forward convolution whose INPUT is the previous layer's BatchNorm + ReLU applied on the fly: the A operand is
 * relu(x * in_scale[c] + in_shift[c]) computed in the loader (x = the producer's pre-BN output, in_scale / in_shift [Cin] from
 * osi_bn_finalize_stats / osi_bn_eval_coeffs), zero padding applied AFTER the activation as conv2d pads the activation tensor.
 * Replaces conv2d(relu(bn(x)), w) of the Bottleneck (conv2 / conv3) without the activation ever touching HBM. pstats may be NULL
 * (then P / rows_per_block are ignored); tiles: OSI_TILE_AUTO, OSI_TILE_64x64_S1, OSI_TILE_64x128_S1. */
int osi_conv_fwd_act(const osi_conv_desc* d, const float* x, const float* in_scale, const float* in_shift, const float* w, float* y,
                     int tile, float* pstats, size_t pstats_bytes, int* P, int* rows_per_block, osi_stream_t stream);
/* 1x1 stride-1 convolution whose input is a whole bottleneck OUTPUT recomputed in the loader: A = relu(x * in_scale[c] + in_shift[c]
 * + res) with x = conv3's pre-BN output and res = the identity shortcut (same shape). conv1 of the next bottleneck can start
 * without waiting for the block-output pass (which still materialises the tensor for the later consumers, on another stream).
 * The value is bit-identical to what osi_bn_apply_relu_mask writes (one fma, one add, max). */
int osi_conv_fwd_act2(const osi_conv_desc* d, const float* x, const float* in_scale, const float* in_shift, const float* res,
                      const float* w, float* y, int tile, float* pstats, size_t pstats_bytes, int* P, int* rows_per_block,
                      osi_stream_t stream);
/* Winograd F(2x2, 3x3) forms of the two calls above for 3x3 / stride 1 / pad 1 convolutions (conv2 of the bottlenecks without a stride;
 * csrc/conv_wino.hip): 2.25x fewer multiplies, every product and sum still fp32 (exact-f32 MFMA), error against fp64 below the direct
 * kernels' on the network's shapes. `ws` = osi_conv_wino_workspace(d) bytes for the transformed weights (rebuilt by every call: the
 * weights change every step) and the stream-K slab; workspace contents are never assumed (ws, the slab of the `_pre` calls, pstats,
 * f->partials). osi_conv_wino_eligible: 1 when the shape is taken (Cin % 16 == 0 and Cout % 64 == 0 forward, swapped for the
 * input gradient; forward: every 16-tile statistics group must hold the same number of pixels — H, W even and B * H/2 * W/2 % 16 == 0, or
 * whole images per group as at 7 x 7).
 * osi_conv_fwd_wino = osi_conv_fwd_act (in_scale / in_shift given) or osi_conv_fwd_bnstats (NULL): *P = ceil(tiles / 16) partials of
 * *rows_per_block pixels for osi_bn_finalize_stats; pstats may be NULL.
 * osi_conv_dgrad_fused_wino = osi_conv_dgrad_fused restricted to the executor's "in-block" fusion: f->scale0 / shift0 / y0 required (gate
 * recomputed), no addend / relu_mask / y1 / pool mode; f->partials optional ([3][*P][Cin], planes 0 and 1 written). */
int osi_conv_wino_eligible(const osi_conv_desc* d, int input_gradient);
size_t osi_conv_wino_workspace(const osi_conv_desc* d);
/* The transformed weights of a convolution can be built AHEAD of its launches (they are the same for the forward and the backward pass of a
 * step): osi_conv_wino_transform_weights writes them into `u` (osi_conv_wino_weights_bytes(d) bytes; input_gradient = 1: the flipped /
 * transposed form of the input gradient), and the `_pre` calls take `u` instead of the raw weights plus the shared stream-K slab
 * (osi_conv_wino_slab_bytes() bytes, the same for every convolution). The executor does this for all its 3x3 layers on the side stream at
 * the start of a forward pass. */
size_t osi_conv_wino_weights_bytes(const osi_conv_desc* d);
size_t osi_conv_wino_slab_bytes(void);
int osi_conv_wino_transform_weights(const osi_conv_desc* d, const float* w, int input_gradient, float* u, size_t u_bytes, osi_stream_t stream);
int osi_conv_fwd_wino_pre(const osi_conv_desc* d, const float* x, const float* in_scale, const float* in_shift, const float* u, float* y,
                          void* slab, size_t slab_bytes, float* pstats, size_t pstats_bytes, int* P, int* rows_per_block, osi_stream_t stream);
int osi_conv_fwd_wino(const osi_conv_desc* d, const float* x, const float* in_scale, const float* in_shift, const float* w, float* y,
                      void* ws, size_t ws_bytes, float* pstats, size_t pstats_bytes, int* P, int* rows_per_block, osi_stream_t stream);
/* Inference forms (validate() / get_arrays(), openset_imagenet/train.py:142-234: model.eval(), BatchNorm on running statistics). In eval
 * mode a BatchNorm's scale / shift are known before its convolution is launched, so the convolution's epilogue applies them — plus the
 * Bottleneck's shortcut and ReLU (torchvision Bottleneck.forward under model.py:37) — and the pre-BN tensor is never written:
 *     out = [relu](conv2d(x, w) * scale[n] + shift[n] [+ residual])          one fma, one add, one max per element
 * (the roundings of osi_bn_apply: bit-identical to osi_conv_fwd followed by osi_bn_apply on the same accumulators). residual: same
 * shape as out, may be NULL, must not alias out. ws: osi_conv_fwd_epilogue_workspace(d) bytes (slab of a K-split tail; may be 0 / NULL:
 * the launch is then single-pass); workspace contents are never assumed. Not for the stem (its tail is osi_bn_relu_maxpool_fwd). Cin % 32 == 0, Cout % 64 == 0. */
typedef struct {
    const float* scale;     /* [Cout], e.g. from osi_bn_eval_coeffs */
    const float* shift;     /* [Cout] */
    const float* residual;  /* [B][Ho][Wo][Cout] or NULL */
    int relu;
} osi_conv_epilogue;
size_t osi_conv_fwd_epilogue_workspace(const osi_conv_desc* d);
int osi_conv_fwd_epilogue(const osi_conv_desc* d, const float* x, const float* w, float* out, const osi_conv_epilogue* e, void* ws,
                          size_t ws_bytes, osi_stream_t stream);
/* The Winograd form of the same for the shapes osi_conv_wino_eligible(d, 0) takes; e->residual must be NULL (conv2 of a Bottleneck has
 * no shortcut); u / slab as osi_conv_fwd_wino_pre. */
int osi_conv_fwd_wino_epilogue_pre(const osi_conv_desc* d, const float* x, const float* u, float* out, const osi_conv_epilogue* e, void* slab,
                                   size_t slab_bytes, osi_stream_t stream);
/* dx (+)= conv2d_input_grad(dy, w). accumulate = 1 adds into dx (skip-connection sum); accumulate = 2 ("sparse", ABI 4) writes
 * only the input pixels some filter tap reaches and leaves every other element of dx UNTOUCHED (a stride-2 1x1 convolution reaches
 * the pixels with even h and even w: a quarter of the tensor) — for a consumer that knows the pattern, see
 * osi_dgrad_fusion.addend_stride. Cout % 32 == 0, Cin % 64 == 0. */
int osi_conv_dgrad(const osi_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate, int tile,
                   osi_stream_t stream);
/* Input gradient with a fused epilogue: dx = relu_mask . (conv2d_input_grad(dy, w) + addend), i.e. the gradient already passed
 * through the ReLU that produced this conv's input (bitmask written by osi_bn_apply_relu_mask); when `partials` is set the
 * epilogue also emits, per row tile, the column sums of g, g*xhat0 and (y1 != NULL) g*xhat1 (xhat = (y - mean)*invstd) — the
 * BatchNorm-backward reductions of the layer(s) that produced that input — as partials[3][*P][Cin], to be finished by
 * osi_bn_backward_fused. addend may be dx. f->partials: osi_conv_dgrad_fused_workspace(d) bytes (the partial sums, then the slab of a
 * K-split tail); workspace contents are never assumed (also for osi_conv_dgrad_fused_frozen). */
typedef struct {
    const void* relu_mask;  /* may be NULL: no mask */
    const float* y0;        /* pre-BN tensor of the consumer BatchNorm, same shape as dx */
    const float* mean0;     /* its batch mean [Cin] */
    const float* invstd0;   /* its batch 1/sqrt(var + eps) [Cin] */
    const float* y1;        /* second consumer (downsample branch) or NULL */
    const float* mean1;
    const float* invstd1;
    float* partials;        /* NULL: no reductions */
    size_t partials_bytes;  /* >= osi_conv_dgrad_fused_workspace(d) */
    const float* scale0;    /* alternative gate when relu_mask == NULL: the producer's activation relu(y0 * scale0 + shift0) was */
    const float* shift0;    /* never stored (osi_conv_fwd_act consumed y0 directly), so the gate is recomputed: on where > 0 */
    /* Pool mode (ABI 3; stride-1 convs, relu_mask = scale0 = NULL): this conv's input is the output of the stem's fused
     * bn -> ReLU -> max-pool 3x3 / 2 (osi_bn_relu_maxpool_fwd), so dx is the gradient w.r.t. the POOLED activation. pool_idx = that
     * kernel's arg-max bytes; y0 / mean0 / invstd0 describe the BatchNorm BEFORE the pool, y0 being [B][pool_H][pool_W][Cin]. dx is
     * written unmasked; the partials become the BatchNorm-backward reductions of the max-pool-scattered, ReLU-gated gradient
     * (sum g and sum g * xhat(arg-max pixel) per row tile): bn1's dgamma / dbeta need no pass over the 112 x 112 tensor of their own.
     * Finish them with osi_bn_backward_reduce. */
    const void* pool_idx;
    int pool_H, pool_W;
    /* ABI 4. 0 / 1: `addend` is dense. 2: `addend` holds values only at pixels with even h AND even w (what osi_conv_dgrad with
     * accumulate = 2 wrote for a stride-2 1x1 convolution); every other pixel of it is never read and counts as zero. */
    int addend_stride;
} osi_dgrad_fusion;
size_t osi_conv_dgrad_fused_workspace(const osi_conv_desc* d);
int osi_conv_dgrad_fused(const osi_conv_desc* d, const float* dy, const float* w, float* dx, const float* addend,
                         const osi_dgrad_fusion* f, int tile, int* P, osi_stream_t stream);
/* ABI 12, frozen BatchNorm statistics. The in-block form of osi_conv_dgrad_fused (f->scale0 / shift0 / y0 set: gate recomputed as
 * fma(y0, scale0, shift0) > 0; relu_mask, y1, pool_idx NULL, no addend: OSI_ERR_ARG otherwise) for a producer BatchNorm that ran on
 * FIXED statistics: g = gate . conv2d_input_grad(dy, w), and the store is the producer's BatchNorm backward itself,
 *   dx = scale0[c] * g        (dy0 = gamma * invstd * g: with constant mean / variance no mean(g) or mean(g * xhat) term exists),
 * so no BatchNorm-backward apply pass follows. f->partials set: the per-row-tile column sums of the UNSCALED g and of g * xhat0
 * (xhat0 from mean0 / invstd0) as partials[2][*P][Cin], to be finished by osi_bn_backward_reduce into dbeta / dgamma; partials = NULL:
 * nothing but dx is written (input-only backward; P may be NULL). tile: OSI_TILE_AUTO or OSI_TILE_64x64_S1 — the 64x64 single-buffered
 * tile in all its forms (stride-2 parity classes, 3x3 row windows, K-split tail + fix-up when the partials' workspace has room). */
int osi_conv_dgrad_fused_frozen(const osi_conv_desc* d, const float* dy, const float* w, float* dx, const osi_dgrad_fusion* f, int tile,
                                int* P, osi_stream_t stream);
int osi_conv_dgrad_fused_wino(const osi_conv_desc* d, const float* dy, const float* w, float* dx, const osi_dgrad_fusion* f, void* ws,
                              size_t ws_bytes, int* P, osi_stream_t stream);
int osi_conv_dgrad_fused_wino_pre(const osi_conv_desc* d, const float* dy, const float* u, float* dx, const osi_dgrad_fusion* f, void* slab,
                                  size_t slab_bytes, int* P, osi_stream_t stream);
/* dw = conv2d_weight_grad(dy, x), deterministic split-K through `ws` (size from osi_conv_wgrad_workspace; 0 / NULL when the plan has
 * one split); workspace contents are never assumed. The stem writes the packed [Cout][224] form; osi_stem_grad_unpack converts to
 * [Cout][7][7][3]. */
size_t osi_conv_wgrad_workspace(const osi_conv_desc* d);
int osi_conv_wgrad(const osi_conv_desc* d, const float* dy, const float* x, float* dw, void* ws, size_t ws_bytes,
                   osi_stream_t stream);
/* The same with x replaced by relu(x * in_scale[c] + in_shift[c]) in the loader (the conv's input activation was never stored). */
int osi_conv_wgrad_act(const osi_conv_desc* d, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dw,
                       void* ws, size_t ws_bytes, osi_stream_t stream);
/* Winograd F(3x3, 2x2) form of the two calls above for 3x3 / stride 1 / pad 1 convolutions with Cin % 64 == 0 and Cout % 64 == 0
 * (csrc/conv_wino.hip): the sum over output tiles is taken in the transformed domain (16 multiplies per tile and (cout, cin) pair
 * instead of 36), deterministic (split-K over the tile axis into partial slabs, fixed-order reduce). in_scale / in_shift may be NULL.
 * ws: osi_conv_wgrad_wino_workspace(d) bytes; 0 = the shape is not taken; workspace contents are never assumed. */
size_t osi_conv_wgrad_wino_workspace(const osi_conv_desc* d);
int osi_conv_wgrad_wino(const osi_conv_desc* d, const float* dy, const float* x, const float* in_scale, const float* in_shift, float* dw,
                        void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_stem_weight_pack(const float* w_krsc3, float* w_packed, int Cout, osi_stream_t stream);
/* Direct form of the stem weight gradient (7x7 / stride 2 / pad 3, Cout = 64, Ho % 8 == 0, Wo % 16 == 0 — the conv1 of
 * torchvision's resnet50 under model.py:17 at any image size that is a multiple of 16 x 32): writes the gradient in the PARAMETER
 * layout [64][7][7][3] directly (no packed form, no unpack pass), deterministic (one partial per workgroup, fixed-order reduce).
 * osi_stem_wgrad_direct_workspace returns 0 for a geometry it does not take (use osi_conv_wgrad + osi_stem_grad_unpack then);
 * osi_stem_wgrad_direct returns OSI_ERR_ARG for it. x4 = the NHWC4 image the forward read. workspace contents are never assumed. */
size_t osi_stem_wgrad_direct_workspace(const osi_conv_desc* d);
int osi_stem_wgrad_direct(const osi_conv_desc* d, const float* dy, const float* x4, float* dw_krsc3, void* ws, size_t ws_bytes,
                          osi_stream_t stream);
/* The same gradient with the whole stem tail fused into the operand loader: dY = BatchNorm backward of the ReLU-gated max-pool
 * scatter of gpool (the gradient w.r.t. the pooled activation) is built per tile in LDS from gpool, the arg-max bytes of
 * osi_bn_relu_maxpool_fwd and the stem's conv output y, and never written to memory. dgamma / dbeta: the stem BatchNorm's reductions
 * (osi_bn_relu_maxpool_bwd with dy = NULL computes exactly those). ws: osi_stem_wgrad_fused_workspace(d) bytes; workspace contents are
 * never assumed. */
size_t osi_stem_wgrad_fused_workspace(const osi_conv_desc* d);
int osi_stem_wgrad_fused(const osi_conv_desc* d, const float* gpool, const void* pool_idx, const float* y, const float* x4,
                         const float* gamma, const float* mean, const float* invstd, const float* dgamma, const float* dbeta,
                         float* dw_krsc3, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_stem_grad_unpack(const float* g_packed, float* g_krsc3, int Cout, osi_stream_t stream);
/* ABI 8. Input gradient of the stem conv (7x7 / stride 2 / pad 3, 3 input channels) for an image batch [B][3][H][W]:
 *   dx[b][c][h][w] = sum_k sum_(r,s) dy[b][(h+3-r)/2][(w+3-s)/2][k] * w_krsc3[k][r][s][c]   (taps with h+3-r, w+3-s even, inside dy)
 * dy = the stem conv's output gradient, NHWC [B][Hs][Ws][64] with Hs = (H-1)/2 + 1, Ws = (W-1)/2 + 1 (16-byte aligned); w_krsc3 =
 * conv1's weight in the arena layout [64][7][7][3]; dx_nchw = fp32 [B][3][H][W], every element written (no pre-zeroing), no atomics
 * (two calls give equal bits). H, W >= 32 (any size osi_resnet50_create takes, odd ones included); OSI_ERR_ARG before any launch. */
int osi_stem_dgrad(const float* dy, const float* w_krsc3, float* dx_nchw, int B, int H, int W, osi_stream_t stream);
/* ABI 10. The same input gradient ending in an FGSM epilogue: dx is never written; with dx as above (the two partial sums added exactly
 * as osi_stem_dgrad adds them)
 *   x_adv[b][h][w][c] = min(hi, max(lo, x[b][h][w][c] + eps * sgn(dx[b][c][h][w])))   c = 0, 1, 2;   x_adv[b][h][w][3] = 0
 * sgn = +1 / 0 / -1 (torch.sign). x_nhwc4 = the clean batch in the executor's input layout [B][H][W][4], x_adv_nhwc4 = the output batch
 * of the same layout, every element written, one 16-byte load and one 16-byte store per pixel, deterministic. Argument rules of
 * osi_stem_dgrad, plus: both image pointers 16-byte aligned, eps >= 0, lo <= hi, the two batches do not overlap; OSI_ERR_ARG before any
 * launch. */
int osi_stem_dgrad_fgsm(const float* dy, const float* w_krsc3, const float* x_nhwc4, float* x_adv_nhwc4, float eps, float lo, float hi,
                        int B, int H, int W, osi_stream_t stream);
/* ABI 19. The same input gradient ending in one step of a projected attack (PGD): dx is never written; with dx as above, per pixel and
 * per channel c = 0, 1, 2, every operation one fp32 rounding,
 *   t      = x_cur + alpha * sgn(dx)                  (alpha * sgn is exact)
 *   t      = min(max(t, a - eps), a + eps)            a = the pixel of x_anchor (the clean batch): projection onto its eps-ball
 *   x_next = min(hi, max(lo, t));   x_next[b][h][w][3] = 0
 * = torch.clamp(torch.min(torch.max(x + alpha * torch.sign(g), a - eps), a + eps), lo, hi) on fp32 tensors. All three batches are
 * NHWC4 [B][H][W][4]; one 16-byte load more than the FGSM form per pixel (the anchor), one 16-byte store, every element written,
 * deterministic. Argument rules of osi_stem_dgrad_fgsm, plus: x_anchor_nhwc4 non-NULL and 16-byte aligned; alpha finite (negative
 * descends); eps >= 0, +inf allowed (no projection); x_next overlaps neither x_cur nor x_anchor; x_anchor may be x_cur (step 0 of an
 * attack). OSI_ERR_ARG before any launch. With x_anchor == x_cur and 0 <= alpha <= eps, and with eps = +inf for any anchor, the result
 * is the bits of osi_stem_dgrad_fgsm(eps := alpha). Non-finite pixels behave as in osi_stem_dgrad_fgsm. */
int osi_stem_dgrad_pgd(const float* dy, const float* w_krsc3, const float* x_cur_nhwc4, const float* x_anchor_nhwc4, float* x_next_nhwc4,
                       float alpha, float eps, float lo, float hi, int B, int H, int W, osi_stream_t stream);

/* ---- BatchNorm2d in training mode + ReLU + residual (torchvision Bottleneck under model.py:37; train() at train.py:125) --- */
size_t osi_bn_workspace(int M, int C);
/* batch statistics of y[M][C]: mean, invstd = 1/sqrt(biased var + eps), scale = gamma*invstd, shift = beta - mean*scale;
 * running stats updated with the unbiased variance when running_mean/var are non-NULL. ws: osi_bn_workspace(M, C) bytes; workspace
 * contents are never assumed. */
int osi_bn_train_stats(const float* y, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* mean, float* invstd, float* scale, float* shift,
                       void* ws, size_t ws_bytes, osi_stream_t stream);
/* second half of osi_bn_train_stats for partials produced elsewhere (osi_conv_fwd_bnstats): pstats = [P][C] means then [P][C] M2 (only
 * read), then the scratch of the two-level merge, 64 * C floats: pstats_bytes >= (2 * P + 64) * C * 4 (OSI_ERR_ARG below that), and
 * what the scratch holds is never assumed. */
int osi_bn_finalize_stats(float* pstats, size_t pstats_bytes, int P, int rows_per_block, int M, int C, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                          float* invstd, float* scale, float* shift, osi_stream_t stream);
/* eval mode (validate(), train.py:142-196): scale/shift from the running statistics */
int osi_bn_eval_coeffs(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps,
                       int C, float* scale, float* shift, osi_stream_t stream);
/* the same for up to OSI_BN_MULTI_MAX BatchNorm layers in one launch (the executor's inference forward: all 53 at once) */
#define OSI_BN_MULTI_MAX 64
typedef struct {
    const float *running_mean, *running_var, *gamma, *beta;
    float *scale, *shift;
    int C;
} osi_bn_eval_layer;
int osi_bn_eval_coeffs_multi(const osi_bn_eval_layer* layers, int n, float eps, osi_stream_t stream);
/* ABI 12. Frozen statistics for a differentiable forward: scale / shift with the bits of osi_bn_eval_coeffs, plus mean = running_mean and
 * invstd = 1 / sqrt(running_var + eps) where the backward kernels read them; up to OSI_BN_FROZEN_MAX layers in one launch. The running
 * statistics are only read. */
#define OSI_BN_FROZEN_MAX 54
typedef struct {
    const float *running_mean, *running_var, *gamma, *beta;
    float *scale, *shift, *mean, *invstd;
    int C;
} osi_bn_frozen_layer;
int osi_bn_frozen_coeffs_multi(const osi_bn_frozen_layer* layers, int n, float eps, osi_stream_t stream);
/* out = [relu](y*scale + shift [+ residual]) */
int osi_bn_apply(const float* y, const float* residual, const float* scale, const float* shift, float* out, int M, int C,
                 int relu, osi_stream_t stream);
/* g = dout * (act > 0) (act NULL: g = dout); dgamma, dbeta; dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)).
 * gmasked (optional) receives g, the gradient that continues along the skip connection. dy may alias dout. ws:
 * osi_bn_backward_workspace(M, C) bytes, here and for every BatchNorm backward below that names this query (osi_bn_backward_relu_mask,
 * osi_bn_backward_fused, osi_bn_backward_frozen, osi_bn_backward_reduce); workspace contents are never assumed by any of them. */
size_t osi_bn_backward_workspace(int M, int C);
int osi_bn_backward(const float* dout, const float* act, const float* y, const float* mean, const float* invstd,
                    const float* gamma, float* dy, float* gmasked, float* dgamma, float* dbeta, int M, int C, void* ws,
                    size_t ws_bytes, osi_stream_t stream);

/* Bitmask forms: the forward writes one bit per element ((BN(+res)) > 0; osi_bn_relu_mask_bytes of storage) next to the ReLU
 * output, and the backward takes that mask instead of re-reading the activation tensor in both of its passes. */
size_t osi_bn_relu_mask_bytes(int M, int C);
int osi_bn_apply_relu_mask(const float* y, const float* residual, const float* scale, const float* shift, float* out,
                           void* relu_mask, int M, int C, osi_stream_t stream);
/* Block output of a Bottleneck with a projection shortcut in one pass: out = relu(y * scale + shift + (res_y * res_scale +
 * res_shift)) — bn3(conv3) + downsample BatchNorm(downsample conv) + ReLU — plus the ReLU bitmask; the shortcut's normalised
 * tensor is never stored. Bit-identical to osi_bn_apply on the shortcut followed by osi_bn_apply_relu_mask. */
int osi_bn_apply_relu_mask2(const float* y, const float* scale, const float* shift, const float* res_y, const float* res_scale,
                            const float* res_shift, float* out, void* relu_mask, int M, int C, osi_stream_t stream);
int osi_bn_backward_relu_mask(const float* dout, const void* relu_mask, const float* y, const float* mean, const float* invstd,
                              const float* gamma, float* dy, float* gmasked, float* dgamma, float* dbeta, int M, int C, void* ws,
                              size_t ws_bytes, osi_stream_t stream);

/* BatchNorm backward when g (already ReLU-masked) and its reductions come from osi_conv_dgrad_fused: psum_g / psum_gx are
 * [P][C] row-tile partials of sum g and sum g*xhat. Finishes dbeta = sum g, dgamma = sum g*xhat and applies
 * dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)). dy may alias g. ws: osi_bn_backward_workspace(M, C) bytes. */
int osi_bn_backward_fused(const float* g, const float* y, const float* mean, const float* invstd, const float* gamma,
                          const float* psum_g, const float* psum_gx, int P, float* dy, float* dgamma, float* dbeta, int M, int C,
                          void* ws, size_t ws_bytes, osi_stream_t stream);

/* ABI 14. osi_bn_backward_fused for the TWO BatchNorms that read one gated gradient (a projection block's bn3 and its shortcut's
 * BatchNorm): g is streamed once, both sets of sums are finished in one launch (two for P beyond the one-launch limit), and every
 * consumer's dy, dgamma and dbeta are bit for bit those of its own osi_bn_backward_fused call. psum_g [P][C] is shared (dbeta = sum g for
 * both), psum_gx [P][C] is per consumer. consumers[0].dy may alias g; consumers[1].dy is a third buffer.
 * ws: osi_bn_backward_fused2_workspace(C) bytes (any P); workspace contents are never assumed. */
typedef struct {
    const float *y, *mean, *invstd, *gamma;   /* pre-BN tensor, batch statistics, scale parameter */
    const float* psum_gx;                     /* [P][C] row-tile partials of sum g * xhat */
    float* dy;
    float *dgamma, *dbeta;
} osi_bn_fused_consumer;
size_t osi_bn_backward_fused2_workspace(int C);
int osi_bn_backward_fused2(const float* g, const osi_bn_fused_consumer* consumers, const float* psum_g, int P, int M, int C, void* ws,
                           size_t ws_bytes, osi_stream_t stream);

/* ABI 12. BatchNorm backward on FROZEN statistics (mean / invstd are constants of the graph): with g = dout gated by relu_mask (NULL:
 * dout is already gated, e.g. by a dgrad epilogue), every consumer k < n (n = 1 or 2: bn3 and the projection shortcut's BatchNorm read
 * the same gated gradient) gets dy_k = scale_k[c] * g in ONE pass that does not read y. dgamma_k / dbeta_k non-NULL (both or neither):
 * dbeta = sum g, dgamma = sum g * xhat_k first (y, mean, invstd needed; ws >= osi_bn_backward_workspace(M, C)); NULL: no reduction is
 * launched (the sums may also arrive as dgrad-epilogue partials: osi_bn_backward_reduce). gmasked (optional) receives g. consumers[0].dy
 * may alias dout. */
typedef struct {
    const float *y, *mean, *invstd;   /* pre-BN tensor and frozen statistics: read only for dgamma */
    const float* scale;               /* gamma * invstd [C] */
    float* dy;
    float *dgamma, *dbeta;            /* NULL: no parameter gradient */
} osi_bn_frozen_consumer;
int osi_bn_backward_frozen(const float* dout, const void* relu_mask, const osi_bn_frozen_consumer* consumers, int n, float* gmasked, int M,
                           int C, void* ws, size_t ws_bytes, osi_stream_t stream);

/* ---- pooling / layout (ResNet.maxpool, ResNet.avgpool, flatten; image batch of train.py:128) --- */
int osi_nchw3_to_nhwc4(const float* x_nchw, float* y_nhwc4, int B, int H, int W, osi_stream_t stream);
/* uint8 [B][H][W][3] -> fp32 [B][H][W][4] = value / 255 (ToTensor(), train.py:263), horizontally flipped where flip[b] != 0
 * (RandomHorizontalFlip, train.py:262; flip may be NULL), 4th channel zero: the input pipeline's last mile on the device. */
int osi_u8hwc3_to_nhwc4(const unsigned char* x_u8_nhwc, const unsigned char* flip, float* y_nhwc4, int B, int H, int W,
                        osi_stream_t stream);
/* The device side of the reference's input transform Compose([Resize(256), RandomCrop(224) | CenterCrop(224), RandomHorizontalFlip,
 * ToTensor]) (train.py:259-268) after decode + resize: canvas = uint8 [B][Hc][Wc][3] holding the resized image (or a window of it
 * that contains the crop), crop_xy = int32 [B][2] top-left corner (x0, y0) of the HxW crop inside the canvas (NULL = (0, 0); read-only:
 * the kernel clamps each corner into the valid range in registers), flip[b] != 0 mirrors the CROPPED image (NULL = none);
 * y = fp32 [B][H][W][4], value / 255, 4th channel zero. */
int osi_u8_crop_flip_to_nhwc4(const unsigned char* canvas_u8, const int* crop_xy, const unsigned char* flip, float* y_nhwc4, int B, int Hc,
                              int Wc, int H, int W, osi_stream_t stream);
/* idx: B*Ho*Wo*C bytes (argmax position 0..8 per element) */
int osi_maxpool3x3s2_fwd(const float* x, float* y, void* idx, int B, int H, int W, int C, osi_stream_t stream);
int osi_maxpool3x3s2_bwd(const float* dy, const void* idx, float* dx, int B, int H, int W, int C, osi_stream_t stream);
/* The ResNet stem tail (bn1 -> relu -> maxpool, torchvision ResNet.forward under model.py:37) as one pass each way:
 *   fwd: pooled = maxpool3x3s2(relu(y*scale + shift)); the post-ReLU activation is never stored. idx bytes as above with bit 7 =
 *        "window maximum > 0" (the ReLU gate of the pixel the gradient will return to).
 *   bwd: gpool = dJ/dpooled -> dgamma, dbeta and dy = BatchNorm backward of the pool-scattered, ReLU-gated gradient, gathered on
 *        the fly (no [B][H][W][C] gradient tensor). ws: osi_bn_backward_workspace(B*H*W, C) bytes; workspace contents are never
 *        assumed (osi_bn_relu_maxpool_bwd and osi_bn_relu_maxpool_bwd_frozen). */
/* The reduction half of osi_bn_backward_fused alone: merges per-row-tile partials (psum_g, psum_gx: [P][C], e.g. from a pool-mode
 * osi_conv_dgrad_fused) into dgamma / dbeta. M = elements per channel of the BatchNorm (c1 = dbeta / M, c2 = dgamma / M are left in ws
 * for callers that want them). ws: osi_bn_backward_workspace(M, C) bytes. */
int osi_bn_backward_reduce(const float* psum_g, const float* psum_gx, int P, float* dgamma, float* dbeta, int M, int C, void* ws,
                           size_t ws_bytes, osi_stream_t stream);
int osi_bn_relu_maxpool_fwd(const float* y, const float* scale, const float* shift, float* pooled, void* idx, int B, int H, int W,
                            int C, osi_stream_t stream);
int osi_bn_relu_maxpool_bwd(const float* gpool, const void* idx, const float* y, const float* mean, const float* invstd,
                            const float* gamma, float* dy, float* dgamma, float* dbeta, int B, int H, int W, int C, void* ws,
                            size_t ws_bytes, osi_stream_t stream);
/* ABI 12. The stem tail's backward on frozen statistics: dy = scale * (pool-scattered, bit-7-gated gpool); dgamma / dbeta (both or
 * neither; NULL: no reduction launched) = sum g * xhat / sum g. */
int osi_bn_relu_maxpool_bwd_frozen(const float* gpool, const void* idx, const float* y, const float* mean, const float* invstd,
                                   const float* scale, float* dy, float* dgamma, float* dbeta, int B, int H, int W, int C, void* ws,
                                   size_t ws_bytes, osi_stream_t stream);
int osi_avgpool_fwd(const float* x, float* y, int B, int HW, int C, osi_stream_t stream);
int osi_avgpool_bwd(const float* dy, float* dx, int B, int HW, int C, osi_stream_t stream);

/* ---- head: resnet_base.fc (model.py:19-20) and logits (model.py:23-26) --- */
int osi_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int O, osi_stream_t stream);
int osi_linear_bwd(const float* dy, const float* x, const float* w, float* dx, int dx_accumulate, float* dw, float* db, int B,
                   int K, int O, osi_stream_t stream);

/* ---- losses (losses.py:16-29; train.py:343; train.py:344-347; objectosphere term: SURVEY.md §8 a9) --- */
enum { OSI_LOSS_ENTROPIC = 0, OSI_LOSS_SOFTMAX = 1, OSI_LOSS_GARBAGE = 2 };
/* loss (1 float) and dlogits = dJ/dlogits in one launch. features != NULL adds alpha/B * sum r_i^2 and writes dfeatures.
 * dlogits may be NULL (validation: loss only). A row with target >= C has no term in the loss and an all-zero dlogits row in
 * every mode (entropic: the divisor stays B). B <= 15360 (OSI_ERR_ARG above, nothing written). */
int osi_loss_fwd_bwd(int mode, const float* logits, const long long* target, int B, int C, float unk_weight,
                     long long ignore_index, const float* class_weights, const float* features, int F, float xi, float alpha,
                     float* loss, float* dlogits, float* dfeatures, osi_stream_t stream);
int osi_softmax(const float* logits, float* out, int B, int C, osi_stream_t stream); /* train.py:177 */
/* validation confidences of metrics.py:8-42 accumulated on the device across batches: acc4 (double[4], caller-zeroed) +=
 * {sum known score[y], #known, sum negatives (1 + offset - max score[:last_valid_class]), #negatives}.
 * last_valid_class: 0 = all columns (Python None), negative = Python negative slice end (-1: drop the background column). */
int osi_confidence_accumulate(const float* logits, const long long* target, int B, int C, float offset, long long unknown_class,
                              int last_valid_class, double* acc4, osi_stream_t stream);
/* the same sums from a matrix of softmax SCORES, i.e. metrics.confidence(scores, target_labels, offset, unknown_class,
 * last_valid_class) itself (metrics.py:8-42) */
int osi_confidence_from_scores(const float* scores, const long long* target, int B, int C, float offset, long long unknown_class,
                               int last_valid_class, double* acc4, osi_stream_t stream);

/* Open-Set Classification Rate curve, util.calculate_oscr (util.py:90-122), on device-resident scores[N][C] (f32 or f64) and
 * int64 labels. Outputs: taus[0 .. totals[0]) = the distinct target-class scores of the known samples in ascending order;
 * for the totals[0] - 1 thresholds tau = taus[u] (the largest is dropped, util.py:114): ccr_count[u] = #{known, argmax == label,
 * score[label] > tau}, fpr_count[u] = #{label == unk_label, max score > tau}; totals = {#distinct, #known, #unk_label}.
 * The curve is ccr_count / totals[1], fpr_count / totals[2] in float64 (integer counts: bit-identical to the reference).
 * taus / ccr_count / fpr_count hold N entries each, totals 3; ws: osi_oscr_workspace(N) bytes. */
size_t osi_oscr_workspace(int N);
int osi_oscr_f32(const float* scores, const long long* gt, int N, int C, long long unk_label, void* ws, size_t ws_bytes,
                 float* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream);
int osi_oscr_f64(const double* scores, const long long* gt, int N, int C, long long unk_label, void* ws, size_t ws_bytes,
                 double* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream);

/* ABI 16. ROC-AUC counting for metrics.auc_score_binary / auc_score_multiclass (metrics.py:65-106, sklearn.metrics.roc_auc_score) on
 * device-resident scores[N][C] (f32 or f64) and int64 labels. The device counts pairs in integers; the host forms the Mann-Whitney
 * quotient (2 * gt + eq) / (2 * P * Nn) with one division. ws: osi_auc_workspace(N) bytes for either entry point. Every output is
 * zeroed by the call. OSI_ERR_ARG before any launch on a null pointer, N <= 0, C <= 0 or a short workspace.
 *   binary: positives are the rows with gt != unk_class, everything else is a negative, the compared value is the row maximum over
 *     all C columns. counts5 = {gt = #{max_pos > max_neg}, eq = #{max_pos == max_neg}, P, Nn, rows holding a NaN}.
 *   one-vs-rest: for class c the positives are the rows with gt == c, the negatives all other rows, the compared value column c;
 *     O(N^2) comparisons in total. gt_c / eq_c / pos_c hold C entries each (pairs above, pairs tied, positives of class c; the
 *     negatives of class c are N - pos_c[c]); flags3 = {rows whose label is outside [0, C), rows holding a NaN, rows whose fp64 sum s
 *     violates |s - 1| <= 1e-8 + 1e-5}. C above 2048 does not fit the LDS tiling: OSI_ERR_ARG. */
size_t osi_auc_workspace(int N);
int osi_auc_binary_f32(const float* scores, const long long* gt, int N, int C, long long unk_class, void* ws, size_t ws_bytes,
                       long long* counts5, osi_stream_t stream);
int osi_auc_binary_f64(const double* scores, const long long* gt, int N, int C, long long unk_class, void* ws, size_t ws_bytes,
                       long long* counts5, osi_stream_t stream);
int osi_auc_ovr_f32(const float* scores, const long long* gt, int N, int C, void* ws, size_t ws_bytes, long long* gt_c,
                    long long* eq_c, long long* pos_c, long long* flags3, osi_stream_t stream);
int osi_auc_ovr_f64(const double* scores, const long long* gt, int N, int C, void* ws, size_t ws_bytes, long long* gt_c,
                    long long* eq_c, long long* pos_c, long long* flags3, osi_stream_t stream);

/* ABI 28. Detection metrics and the OSCR curve by rejection score (metrics.detection_metrics, util.oscr_by_rejection; csrc/
 * detection.hip) for the one-value-per-sample output of the post-hoc detectors: u[N] (f32 or f64), higher = more unknown, int64 labels
 * gt[N], a negative unk_label and, optionally, correct[N] (unsigned char, non-zero = the closed-set prediction of the row is right;
 * NULL = no row is). Populations: known = {gt >= 0}, unk = {gt == unk_label}, correct = {known, correct[i] != 0}. A row whose u is NaN
 * belongs to no population and is counted in nan_rows; so does no row with another negative label. +-Inf are ordinary values;
 * comparison is IEEE (-0 == +0). Everything counted is an integer, merged with integer atomics where at all: results do not depend on
 * the grid or on the run. Every output is written or zeroed by the call; nothing allocates or synchronises. OSI_ERR_ARG before any
 * launch on a null required pointer, N <= 0, unk_label >= 0, Q outside [1, 8] or ws_bytes < osi_det_workspace(N) (one size for the
 * three calls, 0 for an N they refuse; the workspace is 16-byte aligned and its contents are never assumed).
 *   osi_det_ranks_*: ranks is int32[6][N], rows kn_lt, kn_le, unk_lt, unk_le, cor_lt, cor_le: for row i and each population the
 *     numbers #{j in population: u_j < u_i} and #{j in population: u_j <= u_i}; zeros for a NaN row. counts4 = {K, U, Kc, nan_rows},
 *     the sizes of known, unk and correct. The one O(N^2) pass (all pairs, LDS-staged tiles, 32-bit partial counts).
 *   osi_det_summary: from ranks, gt and a DEVICE array q[Q] of TPR levels in (0, 1] (K and U are re-counted from ranks: a member
 *     counts itself in its own kn_le / unk_le):
 *     ints[0] = gt_pairs = sum over unk of kn_lt; ints[1] = eq_pairs = sum over unk of (kn_le - kn_lt): with them the ROC-AUC of known
 *       against unk is the Mann-Whitney quotient (2 gt_pairs + eq_pairs) / (2 K U);
 *     ints[2 + t] = fpr_count[t] = min{unk_le[i] : i known, (double)kn_le[i] / (double)K >= q[t]}, the comparison in fp64 exactly as
 *       written (U when there is no known row): fpr[argmax(tpr >= q)] * U of the ROC curve with known as the positive class, -u as score;
 *     sums[0] = ap_in_sum = sum over known of kn_le / (kn_le + unk_le); sums[1] = ap_out_sum = sum over unk of
 *       (U - unk_lt) / ((U - unk_lt) + (K - kn_lt)); each quotient one fp64 division of exact integers, each sum in fp64 in an order
 *       fixed by N alone. ap_in_sum / K and ap_out_sum / U are the average precisions of known (score -u) and of unk (score u).
 *   osi_det_curve_*: the OSCR curve with u as the rejector, osi_oscr_* with confidence -u: taus[0 .. totals[0]) = the distinct u of
 *     the known rows in DESCENDING order (of equal values the one of the lowest row, so -0 or +0 as that row holds it); for position p
 *     ccr_count[p] = #{correct: u < taus[p]} and fpr_count[p] = #{unk: u < taus[p]}, read from ranks (cor_lt, unk_lt) of that row;
 *     totals = {#distinct, K, U}. The curve is the first totals[0] - 1 positions (the smallest value is dropped), ccr_count / K and
 *     fpr_count / U in fp64. taus / ccr_count / fpr_count hold N entries each, zero past totals[0]. ranks must come from
 *     osi_det_ranks_* on the same u, gt, unk_label. */
size_t osi_det_workspace(int N);
int osi_det_ranks_f32(const float* u, const long long* gt, const unsigned char* correct, int N, long long unk_label, void* ws,
                      size_t ws_bytes, int* ranks, long long* counts4, osi_stream_t stream);
int osi_det_ranks_f64(const double* u, const long long* gt, const unsigned char* correct, int N, long long unk_label, void* ws,
                      size_t ws_bytes, int* ranks, long long* counts4, osi_stream_t stream);
int osi_det_summary(const int* ranks, const long long* gt, int N, long long unk_label, const double* q, int Q, void* ws,
                    size_t ws_bytes, long long* ints, double* sums, osi_stream_t stream);
int osi_det_curve_f32(const float* u, const long long* gt, const int* ranks, int N, long long unk_label, void* ws, size_t ws_bytes,
                      float* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream);
int osi_det_curve_f64(const double* u, const long long* gt, const int* ranks, int N, long long unk_label, void* ws, size_t ws_bytes,
                      double* taus, long long* ccr_count, long long* fpr_count, long long* totals, osi_stream_t stream);

/* ABI 18. Evaluation histograms for util.get_histogram (util.py:202-228): the softmax-score and feature-norm histograms of known
 * against negative / unknown samples, on device-resident scores[N][C], features[N][F] (f32 or f64, type T) and int64 labels. All
 * results are integer counts or min / max of stored values: order-free. Every output is zeroed or written by the call; no
 * allocation, no host synchronisation. OSI_ERR_ARG before any launch on a null pointer, N <= 0, a short workspace or a bad enum.
 *
 * osi_eval_values_*: per row the value each side compares, and side[i]: bit 0 = known (gt >= 0), bit 1 = gt == unk_label. The bits are
 *   independent (unk_label >= 0 gives rows that carry both). Both values are written for every row, whatever its side byte.
 *   OSI_EVAL_SCORE: Cc = C - drop_last class columns (drop_last = 1: the last column is the background class, not a class; Cc >= 1).
 *     kn_val = scores[i][gt], 0 on a row without the known bit; a row with gt >= Cc gets no known bit and counts as a bad label
 *     (the reference raises IndexError).
 *     unk_val = maximum over the first Cc columns, NaN if one of them is NaN (np.amax). features may be NULL.
 *   OSI_EVAL_NORM: both values are the L2 norm of features[i]: squares and their sum in fp64 in index order, one fp64 sqrt, one
 *     rounding to T. scores may be NULL; labels are not range-checked.
 *   range4 = {kn_min, kn_max, unk_min, unk_max} over the non-NaN values of each side, infinities included; +inf / -inf for an empty
 *     side, which the caller does not read. counts6 = {#known, #unk, NaN values among known, NaN among unk, bad labels, 0}.
 *   ws: osi_eval_values_workspace(N) bytes (per-workgroup min / max partials, reduced by a finishing launch).
 *
 * osi_hist_*: np.histogram over the rows with side[i] & side_bit, for an explicit edge table: edges is double[nb + 1] in device
 *   memory, non-decreasing; counts is int64[nb]; 1 <= nb <= OSI_HIST_MAX_BINS (edges as fp64 plus 32-bit counters stay inside 64 KB
 *   of LDS). Bin i counts edges[i] <= x < edges[i + 1], the last bin is closed on the right, NaN and values outside
 *   [edges[0], edges[nb]] are not counted, a zero-width bin stays empty except that x == edges[nb] always lands in bin nb - 1.
 *   Comparisons run in fp64 (a float converts exactly). A table that is not sorted causes no out-of-range access; its counts are
 *   unspecified. val must be aligned to its element size. */
enum { OSI_EVAL_SCORE = 0, OSI_EVAL_NORM = 1 };
#define OSI_HIST_MAX_BINS 4096
size_t osi_eval_values_workspace(int N);
int osi_eval_values_f32(const float* scores, const float* features, const long long* gt, int N, int C, int F, int metric,
                        long long unk_label, int drop_last, float* kn_val, float* unk_val, unsigned char* side, double* range4,
                        long long* counts6, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_eval_values_f64(const double* scores, const double* features, const long long* gt, int N, int C, int F, int metric,
                        long long unk_label, int drop_last, double* kn_val, double* unk_val, unsigned char* side, double* range4,
                        long long* counts6, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_hist_f32(const float* val, const unsigned char* side, int side_bit, int N, const double* edges, int nb, long long* counts,
                 osi_stream_t stream);
int osi_hist_f64(const double* val, const unsigned char* side, int side_bit, int N, const double* edges, int nb, long long* counts,
                 osi_stream_t stream);

/* ABI 21. OpenMax (Bendale & Boult, CVPR 2016; openset_imagenet/openmax.py): class means of the correctly classified training rows, a
 * Weibull fit to the largest distances of every class, and test logits recalibrated by the probability of lying in that tail. The
 * method is not part of the reference snapshot; this block is its definition. Inputs are the device-resident arrays of get_arrays:
 * features[N][F] and logits[N][C] in fp32, int64 labels; F and C are independent. No floating-point atomics: every output is
 * bit-identical from run to run. Every output is zeroed or written by the call; no allocation, no host synchronisation; workspace
 * contents are never assumed (ws: osi_openmax_workspace(N, C, F) bytes, 4-byte aligned, overwritten; 0 for non-positive arguments).
 * OSI_ERR_ARG before any launch on a null pointer (cls excepted), N, C or F <= 0, a short workspace or a bad enum / range.
 *
 * osi_openmax_class_means: row i is correct for class c when gt[i] == c, 0 <= c < C, and the first maximum of logits[i] (lowest index
 *   on ties) is column c; a row holding a NaN logit is never correct, labels outside [0, C) are ignored. correct[i] = 1 / 0.
 *   count[c] = the correct rows of class c; mav[c] = the mean of their features: summed in fp64 in ascending row order, divided once
 *   in fp64, rounded once to fp32; all zeros for a class without a correct row.
 * osi_openmax_distances: d(f, m) with every sum in fp64 in index order, each product rounded before it is added, one fp64 sqrt /
 *   divide and one rounding to fp32. OSI_OPENMAX_EUCLIDEAN: sqrt(sum (f_j - m_j)^2). OSI_OPENMAX_COSINE:
 *   1 - (sum f_j m_j) / sqrt(sum f_j^2 * sum m_j^2), NaN for a zero denominator. cls == NULL: dist[N][C], every row against every
 *   class mean (C <= 64 * 65535: one grid row per 64 classes). Otherwise dist[N], row i against mav[cls[i]], NaN where cls[i] is
 *   outside [0, C).
 * osi_openmax_fit_tails: for class c, D_c = the finite dist[i] over the rows with correct[i] and gt[i] == c (-0 counts as +0). The
 *   tail is the min(T, |D_c|) largest values (tail_count[c]), 2 <= T <= OSI_OPENMAX_MAX_TAIL; shift[c] = its smallest value; the
 *   fitted data are x = tail - shift[c] + 1 in fp64 (libMR's FitHigh translation, x >= 1). shape[c] = k is the root of
 *   g(k) = sum x^k ln x / sum x^k - 1/k - mean(ln x) (the maximum-likelihood equation of the two-parameter Weibull), with x^k taken
 *   as exp(k ln x - k ln x_max); scale[c] = x_max * (mean exp(k ln x - k ln x_max))^(1/k). A class whose tail has fewer than two
 *   values, or equal largest and smallest values (in fp32, or x_max == 1 after the translation in fp64: a spread below 2^-53), is
 *   unfitted: fitted[c] = 0 and shape = scale = shift = 0.
 *   flags2 = {eligible rows whose distance is not finite (left out), unfitted classes}.
 *   One workgroup per class: radix select over the float bits (four passes over the rows), bitonic sort of the tail in LDS, sums over
 *   the sorted tail in a fixed tree, so the fit depends on the multiset of the tail alone (permuting the rows changes no bit).
 *   The solver doubles / halves from k = 1 to a bracket (at most 1100 steps), then takes Newton steps that fall back to bisection
 *   whenever they leave the bracket (at most 128 steps): the iteration count is bounded whatever the data.
 * osi_openmax_wscores: w[i][c] = 1 - exp(-(z / scale[c])^shape[c]) with z = dist[i][c] - shift[c] + 1, in fp64 from the fp32
 *   distance, rounded once to fp32; 0 when z <= 0 or the class is unfitted; NaN for a NaN distance.
 * osi_openmax_recalibrate: a = min(alpha, C), alpha >= 1. Per row the logits are ranked descending and stably (lower index first on
 *   ties); the column of rank r < a gets omega = 1 - w * (a - r) / a, every other column omega = 1 (the authors' released code: rank
 *   0 gets full weight). v^_c = v_c * omega_c, v^_unk = sum_c v_c * (1 - omega_c), probs[i] = softmax([v^_0 .. v^_{C-1}, v^_unk]) in
 *   fp64 with the row maximum subtracted, rounded once to fp32: probs is [N][C + 1], the unknown column LAST (the background-class
 *   convention of this package). A row whose logits hold a NaN is NaN throughout. C above 2048 does not fit the row ranking in LDS:
 *   OSI_ERR_ARG. */
enum { OSI_OPENMAX_EUCLIDEAN = 0, OSI_OPENMAX_COSINE = 1 };
#define OSI_OPENMAX_MAX_TAIL 4096
size_t osi_openmax_workspace(int N, int C, int F);
int osi_openmax_class_means(const float* features, const float* logits, const long long* gt, int N, int C, int F, float* mav,
                            long long* count, unsigned char* correct, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_openmax_distances(const float* features, const float* mav, const long long* cls, int N, int C, int F, int metric, float* dist,
                          osi_stream_t stream);
int osi_openmax_fit_tails(const float* dist, const long long* gt, const unsigned char* correct, int N, int C, int T, double* shape,
                          double* scale, double* shift, unsigned char* fitted, long long* tail_count, long long* flags2, void* ws,
                          size_t ws_bytes, osi_stream_t stream);
int osi_openmax_wscores(const float* dist, int N, int C, const double* shape, const double* scale, const double* shift,
                        const unsigned char* fitted, float* w, osi_stream_t stream);
int osi_openmax_recalibrate(const float* logits, const float* w, int N, int C, int alpha, float* probs, osi_stream_t stream);

/* ABI 22. The Extreme Value Machine (Rudd, Jain, Scheirer, Boult, TPAMI 2018; openset_imagenet/evm.py): one Weibull distribution per
 * training row, fitted to the row's nearest negatives; a greedy set cover keeps the rows of a class that explain the others (the
 * extreme vectors); the score of a class for a query is the largest inclusion probability over the class's extreme vectors. The
 * method is not part of the reference snapshot; this block is its definition, after libMR's FitLow as the authors' code uses it.
 * Inputs are features[N][F] in fp32 and int64 labels gt[N]. A positive of class c is a row with gt == c; EVERY other row is a negative
 * of c: other classes, negative labels, labels >= C. No floating-point atomics: every output is bit-identical from run to run. Every
 * output is zeroed or written by the call; no allocation, no host synchronisation; workspace contents are never assumed (ws:
 * osi_evm_workspace(R, N, F) bytes cover all five calls, 8-byte aligned, overwritten; 0 for non-positive arguments). OSI_ERR_ARG before
 * any launch on a null pointer, a non-positive size, a short workspace or a bad enum / range.
 *
 * osi_evm_distances: dist[R][N], every row of a[R][F] against every row of b[N][F] (4-byte aligned). dot = the fp32 matrix-core product
 *   a_i . b_j: a chain of fp32 fused multiply-adds (v_mfma_f32_32x32x2_f32) from 0 over K in steps of 32; inside a step the order is
 *   k = 8q + e, 8q + 4 + e for q = 0..3, e = 0..3; K is zero-filled past F. The order is fixed: same bits from run to run, and the
 *   same bits for a pair whatever R, N and the pair's position. naa, nbb = the squared row norms: fp64 sums in index order (every
 *   product of two fp32 values is exact in fp64), one pre-pass into the workspace.
 *   OSI_EVM_COSINE: (float)(1 - (double)dot / sqrt(naa * nbb)), the product rounded to fp64 before the root; NaN for a zero denominator.
 *   OSI_EVM_EUCLIDEAN: t = (naa + nbb) - 2 * (double)dot in fp64, (float)sqrt(t < 0 ? 0 : t): a NaN passes the clamp.
 *   NaN and Inf in the inputs propagate as these formulas say. R * N * 4, R * F * 4 or N * F * 4 >= 2^31 -> OSI_ERR_ARG (32-bit buffer
 *   descriptors).
 * osi_evm_fit_rows: one Weibull per row r of dist[R][ld], ld >= N. The candidates are y_j = -(multiplier * dist[r][j]), the product
 *   rounded to fp32, over the columns j < N with gt[j] != cls and a finite y_j (a finite distance, and no overflow of the product);
 *   -0 counts as +0. From here it is exactly the tail fit of osi_openmax_fit_tails applied to y: the min(T, candidates) largest y (the
 *   nearest negatives; tail_count[r]), shift[r] = the smallest of them, x = y - shift[r] + 1 in fp64, the same likelihood equation with
 *   x^k as exp(k ln x - k ln x_max), the same solver and step limits; a row with fewer than two candidates or a collapsed tail (equal
 *   ends in fp32, or x_max == 1 in fp64) is unfitted: fitted[r] = 0, shape = scale = shift = 0. 2 <= T <= OSI_EVM_MAX_TAIL,
 *   multiplier > 0 and finite (the paper's 0.5 is exact). flags2 = {candidates left out for a non-finite value, summed over the rows;
 *   unfitted rows}. One workgroup per row; the result depends on the multiset of the row's candidates only (permuting the columns of
 *   dist and gt together changes no bit). The workspace is not used.
 * Inclusion probability: Psi_r(d) = 1 - exp(-(z / scale[r])^shape[r]) with y = -(multiplier * d) rounded to fp32 and
 *   z = (double)y - shift[r] + 1, in fp64, rounded once to fp32; 0 when z <= 0 or row r is unfitted; NaN for a NaN d (fitted or not).
 * osi_evm_set_cover: dpp[R][R] = the distances among one class's own rows. Row i covers row j when both are fitted and i == j or
 *   Psi_i(dpp[i][j]) >= cover_threshold (the fp32 value against the fp32 threshold; a NaN covers nothing). U starts as the fitted
 *   rows; every step picks the not yet picked fitted row that covers most rows of U, the lowest index on ties, and takes what it covers
 *   out of U; it stops when U is empty. order[k] = the k-th pick, -1 from n_ev[0] on. Unfitted rows are never picked and never need
 *   covering. R <= OSI_EVM_MAX_COVER_ROWS; the cover is a bit matrix in the workspace (R * ceil(R / 64) words) with one count per row
 *   that each pick updates from the words it changed: a pick costs at most one pass over the matrix. Integer arithmetic only.
 *   cover_threshold NaN -> OSI_ERR_ARG.
 * osi_evm_probs: dist[M][ld] = the queries against the V extreme vectors, ld >= V; the extreme vectors are sorted by class and
 *   ev_start[C + 1] holds the offsets (values outside [0, V] are clamped). probs[m][c] = the maximum of Psi_v(dist[m][v]) over
 *   ev_start[c] <= v < ev_start[c + 1]: 0 for a class without any, NaN if any term is NaN (as torch.max). An entry with scale == 0
 *   counts as unfitted. probs is [M][C] fp32. */
enum { OSI_EVM_EUCLIDEAN = 0, OSI_EVM_COSINE = 1 };
#define OSI_EVM_MAX_TAIL 4096
#define OSI_EVM_MAX_COVER_ROWS 16384
size_t osi_evm_workspace(int R, int N, int F);
int osi_evm_distances(const float* a, int R, const float* b, int N, int F, int metric, float* dist, void* ws, size_t ws_bytes,
                      osi_stream_t stream);
int osi_evm_fit_rows(const float* dist, int R, int N, long long ld, const long long* gt, long long cls, int T, float multiplier,
                     double* shape, double* scale, double* shift, unsigned char* fitted, long long* tail_count, long long* flags2,
                     void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_evm_set_cover(const float* dpp, int R, const double* shape, const double* scale, const double* shift,
                      const unsigned char* fitted, float multiplier, float cover_threshold, long long* order, long long* n_ev, void* ws,
                      size_t ws_bytes, osi_stream_t stream);
int osi_evm_probs(const float* dist, int M, int V, long long ld, const double* shape, const double* scale, const double* shift,
                  const long long* ev_start, int C, float multiplier, float* probs, osi_stream_t stream);

/* ABI 23. PROSER (Zhou, Ye, Zhan, "Learning Placeholders for Open-Set Recognition", CVPR 2021; openset_imagenet/proser.py): a short
 * fine-tuning stage from a closed-set checkpoint that mixes activations in the middle of the network (manifold mixup), adds a small
 * "dummy" classifier on the deep features and trains both with a three-term cross-entropy. The method is not part of the reference
 * snapshot; this block is its definition, tests/proser_oracle.py its fp64 restatement. No floating-point atomics, fixed summation
 * orders: every output is bit-identical from run to run. Nothing is allocated or synchronised (graph-capturable).
 *
 * osi_mix_rows_pairs: x is [B][L] fp32, mixed IN PLACE; partner and weight are device arrays of B entries. Row i with j = partner[i]:
 *   j == i, j < 0 or j >= B: the row is neither read nor written (every bit stays, NaN payloads included), and no access leaves the
 *   buffer whatever the arrays hold. j > i: row i OWNS the pair and its workgroups write both rows,
 *     x_i' = fmaf(w_i, x_i, (1 - w_i) * x_j)      x_j' = fmaf(w_j, x_j, (1 - w_j) * x_i)
 *   both from the old values of both rows; 1 - w is rounded once to fp32, its product is rounded once, then the fma (explicit: no
 *   contraction setting changes the bits). w = 1 gives the row back and w = 0 gives the partner's row, both exactly for finite
 *   values. j < i: the row is written by its owner. The callers pass an involution (partner[partner[i]] == i), for which this is the
 *   pairwise mix; the launch serves the first floor(B / 2) owners in row order, which is every pair of an involution (another table
 *   stays in range, but its rows may be written from values another pair has already replaced). One lane reads its 16-byte unit of
 *   both rows and writes both: each element is read once and written once, no staging buffer. The grid is sized to the pairs: a
 *   pair's workgroups walk the row in tiles of 1024 units, at most 8192 workgroups in all; the row decisions are wave-uniform.
 *   OSI_ERR_ARG before any launch: a null pointer, B <= 0, L == 0, L % 4 != 0, x not 16-byte aligned.
 * osi_proser_loss_fwd_bwd: logits[B][C], dummy[B][D] (D >= 1), int64 target[B]; rows [0, n_mixed) are the mixed rows. Per row a = the
 *   first index of the largest dummy logit (a NaN counts as largest, as torch.max), m = dummy[a], e = [logits, m] with C + 1 columns.
 *     mixed row (whatever its label):        t1 = lse(e) - m
 *     clean row (i >= n_mixed), 0 <= y < C:  t2 = lse(e) - e_y,  t3 = lse(e without column y) - m
 *   (the published implementations set e_y = -1e9 for t3; leaving the column out is the same in fp32 and is the definition here). A
 *   clean row with a label outside [0, C) has no term, is not counted and gets exact zero gradient rows.
 *   J = l0 * mean(t1) + l1 * mean(t2) + l2 * mean(t3), each mean over its n1 = n_mixed / n2 counting rows; a term without rows is
 *   exactly 0 and so are its gradients. loss4 = {J, mean t1, mean t2, mean t3}. With s = softmax(e) and s' = the softmax without
 *   column y (s'_y = 0): g = l0 / n1 * (s - onehot(C)) for a mixed row, g = l1 / n2 * (s - onehot(y)) + l2 / n2 * (s' - onehot(C))
 *   for a clean one; dlogits = g[:C], ddummy[a] = g[C], the other D - 1 entries of the ddummy row exact zeros. dlogits and ddummy may
 *   both be NULL (loss only; one of them NULL: OSI_ERR_ARG). One launch in the form of osi_loss_fwd_bwd: one workgroup for the batch,
 *   a wave per row; a first sweep over the labels alone gives n2, one sweep over the rows gives every term and finished gradient
 *   row. A row's term is evaluated as (max - v) + log(sum exp(e - max)) and its softmax as exp(e - max) / sum, so a large common
 *   magnitude of the logits costs no digits. Sums: fp32 in a row (lanes stride the columns, the butterfly of the wave, then the
 *   dummy column), double over the rows (per wave in row order, then the waves in index order). A NaN logit in a counting row gives a NaN loss and a NaN gradient row, as in
 *   torch. B <= 15360, 0 <= n_mixed <= B, C >= 1: OSI_ERR_ARG otherwise.
 * osi_proser_scores: probs[B][C + 1] = softmax([logits, max_d dummy + bias]) per row, the unknown class in the LAST column (the layout
 *   of osi_openmax_recalibrate); a NaN propagates through the maximum. */
int osi_mix_rows_pairs(float* x, const int* partner, const float* weight, int B, size_t L, osi_stream_t stream);
int osi_proser_loss_fwd_bwd(const float* logits, const float* dummy, const long long* target, int B, int C, int D, int n_mixed, float l0,
                            float l1, float l2, float* loss4, float* dlogits, float* ddummy, osi_stream_t stream);
int osi_proser_scores(const float* logits, const float* dummy, float bias, int B, int C, int D, float* probs, osi_stream_t stream);

/* ABI 24. Deep nearest neighbours (Sun, Ming, Zhu, Li, "Out-of-Distribution Detection with Deep Nearest Neighbors", ICML 2022;
 * openset_imagenet/knn.py): ordered selection over the rows of a distance matrix dist[M][ld] (ld >= N columns used) as
 * osi_evm_distances writes it. The method is not part of the reference snapshot; this block is its definition, tests/knn_oracle.py
 * its numpy restatement. There is no floating-point arithmetic on the selection path: every output is an element of the input (its
 * canonical value, below) or an index, bit-identical from run to run and independent of the grid. Nothing is allocated or
 * synchronised; every output element is written by the call; workspace contents are never assumed (ws: osi_knn_workspace(M, N, K)
 * bytes, 8-byte aligned; 0 for non-positive arguments; the kernels stage nothing in it and the size is a small constant). OSI_ERR_ARG
 * before any launch on a null required pointer (skip may be NULL), a non-positive size, ld < N, K outside [1, OSI_KNN_MAX_K], a short
 * workspace or a bad enum. The matrix is read with plain 64-bit addressing: no 2 GiB limit of its own.
 *
 * Order, shared by both calls. A distance is read as d + 0.0f (-0 becomes +0): that canonical value is compared and returned. Values
 *   rank by IEEE order, every NaN after +Inf (a NaN's payload is not part of the definition); equal values, and NaNs among themselves,
 *   rank by ascending column. skip[m] (int64) names one column of row m that does not take part (leave-one-out on the bank); a value
 *   outside [0, N) skips nothing.
 * osi_knn_topk: per row the first min(K, n) columns in that order, n = N minus a skipped column: out_dist[M][K] the canonical values,
 *   out_idx[M][K] (int64) their columns, ascending by (value, column); the remaining entries hold +Inf and -1.
 * osi_knn_class_kth: the columns are sorted by class, class c owns start[c] .. start[c + 1] - 1 (start[C + 1] int64; values are clamped
 *   to [0, N], a descending pair is an empty class). out[m][c] = the min(K, n_c)-th element of the segment in that order, n_c = the
 *   segment length minus a skipped column inside it; +Inf for n_c = 0. `transform` says what is stored for that value v:
 *   OSI_KNN_RAW v; OSI_KNN_SIM_COSINE fminf(fmaxf(1 - 0.5f * v, 0), 1) in fp32 (the product, then one rounded subtraction);
 *   OSI_KNN_SIM_INVERSE 1.0f / (1.0f + v), each operation rounded to fp32. Under both similarities a NaN v stores NaN and +Inf stores 0.
 * One workgroup per row / per (row, class): the segment is read once in tiles of 2048 columns; columns below the running threshold are
 * appended IN COLUMN ORDER (wave ballots) to a buffer in LDS; a four-pass radix select over the buffer and an ordered in-place
 * compaction cut it back to K, which resolves threshold ties by the lowest column. Segments of any length, no staging limit. A class
 * segment of at most 2048 columns is one wave's work instead: keys in registers, a bitwise select on wave ballots (the k-th VALUE
 * needs no tie rule). Two launches for osi_knn_class_kth, one for osi_knn_topk. */
enum { OSI_KNN_RAW = 0, OSI_KNN_SIM_COSINE = 1, OSI_KNN_SIM_INVERSE = 2 };
#define OSI_KNN_MAX_K 1024
size_t osi_knn_workspace(int M, int N, int K);
int osi_knn_topk(const float* dist, int M, int N, long long ld, int K, const long long* skip, float* out_dist, long long* out_idx,
                 void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_knn_class_kth(const float* dist, int M, int N, long long ld, const long long* start, int C, int K, const long long* skip,
                      int transform, float* out, void* ws, size_t ws_bytes, osi_stream_t stream);

/* ABI 25. Mahalanobis and Relative Mahalanobis open-set scores (Lee, Lee, Lee, Shin, "A Simple Unified Framework for Detecting
 * Out-of-Distribution Samples and Adversarial Attacks", NeurIPS 2018; Ren et al., "A Simple Fix to Mahalanobis Distance for Improving
 * Near-OOD Detection", 2021; openset_imagenet/mahalanobis.py): class-conditional Gaussians with ONE tied covariance on features
 * [N][F] fp32 with labels gt[N] int64; every fitted quantity is fp64. The method is not part of the reference snapshot; this block is
 * its definition, tests/mahalanobis_oracle.py its numpy restatement. The products run on the fp64 matrix instruction of gfx950
 * (v_mfma_f64_16x16x4_f64), 64 x 64 tiles staged through LDS. No floating-point atomics: every sum has a fixed order that depends on
 * the sizes alone, so every output is bit-identical from run to run. Nothing is allocated or synchronised; every output element is
 * written by the call; workspace contents are never assumed (ws: osi_maha_workspace(N, C, F) bytes, 8-byte aligned, 0 for a
 * non-positive argument or F > OSI_MAHA_MAX_F; the scatter alone needs more than its first 64 bytes, and for it N is the rows of the
 * call). OSI_ERR_ARG before any launch on a null required pointer, a non-positive size, a short or misaligned workspace, a bad enum, a
 * scalar that is not finite or out of range, and on sizes past the limit: addressing is 64-bit, and a call takes F <= OSI_MAHA_MAX_F
 * and fewer than 2^31 ELEMENTS in each of its matrices (N * F, (C + 1) * F, M * F, M * C); longer inputs go in row chunks.
 *
 * A row is COUNTED when 0 <= gt[i] < C; every other row is ignored everywhere.
 * osi_maha_class_means: mean[C + 1][F], count[C + 1] (int64). Row c < C = the mean of the counted rows of class c, row C = the mean of
 *   all counted rows; fp64 sums divided once; an empty class gives zeros and count 0.
 * osi_maha_scatter: S[F][F] = the sum over the counted rows of a a^T, a = (double)x - m in one rounded subtraction per element, m =
 *   mean[gt[i]] (OSI_MAHA_WITHIN) or mean[C] (OSI_MAHA_TOTAL); `mean` is an input like any other. accumulate = 1 adds the sum to what
 *   S holds (row chunks), 0 overwrites. The lower triangle is computed and mirrored: S is bitwise symmetric. The rows are cut into a
 *   number of splits fixed by (N, F); partial tiles go to the workspace and are added in split order.
 * osi_maha_factor: Sigma = (1 - a) scale S + a (scale tr S / F) I with a = shrinkage in [0, 1], scale > 0 finite. L = the lower
 *   Cholesky factor of Sigma, W = L^-1, logdet[0] = 2 sum ln L_ii; strict upper triangles are exact zeros. info[0] = 0 on success,
 *   else the 1-based index of the first pivot p with !(p > 0) or p = +Inf: L and W are then all zeros and logdet NaN. Right-looking,
 *   panels of 64 columns: the diagonal block in LDS by one workgroup, the panel by substitution (true divisions), the trailing update
 *   on the matrix cores; W by rows from the last panel to the first (W L = I is the small residual). 5 ceil(F / 64) launches, a
 *   function of F alone; after a failed pivot the remaining launches read info and leave. S is read only.
 * osi_maha_whiten_f32 / _f64: z[M][F] (fp64), z[i] = W x[i] with W lower triangular: tiles above the diagonal are skipped.
 * osi_maha_sqdist: v[i][c] = sum_j (z[i][j] - zm[c][j])^2 in the difference form, minus[i] (fp64, may be NULL) subtracted, then
 *   OSI_MAHA_RAW v; OSI_MAHA_SIM_GAUSS exp(-max(v, 0) / (2 F)); OSI_MAHA_SIM_LOGISTIC 1 / (1 + exp(v / (2 F))), in fp64; a NaN
 *   propagates. Exactly one of out_f32[M][C] (rounded once from fp64) and out_f64[M][C] is non-null. */
enum { OSI_MAHA_WITHIN = 0, OSI_MAHA_TOTAL = 1 };
enum { OSI_MAHA_RAW = 0, OSI_MAHA_SIM_GAUSS = 1, OSI_MAHA_SIM_LOGISTIC = 2 };
#define OSI_MAHA_MAX_F 32768
size_t osi_maha_workspace(int N, int C, int F);
int osi_maha_class_means(const float* features, const long long* gt, int N, int C, int F, double* mean, long long* count, void* ws,
                         size_t ws_bytes, osi_stream_t stream);
int osi_maha_scatter(const float* features, const long long* gt, const double* mean, int N, int C, int F, int mode, int accumulate,
                     double* S, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_maha_factor(const double* S, int F, double scale, double shrinkage, double* L, double* W, double* logdet, int* info, void* ws,
                    size_t ws_bytes, osi_stream_t stream);
int osi_maha_whiten_f32(const float* x, int M, int F, const double* W, double* z, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_maha_whiten_f64(const double* x, int M, int F, const double* W, double* z, void* ws, size_t ws_bytes, osi_stream_t stream);
int osi_maha_sqdist(const double* z, int M, const double* zm, int C, int F, const double* minus, int transform, float* out_f32,
                    double* out_f64, void* ws, size_t ws_bytes, osi_stream_t stream);

/* ABI 26. ViM open-set scores (Wang, Li, Feng, Zhang, "ViM: Out-Of-Distribution with Virtual-logit Matching", CVPR 2022;
 * openset_imagenet/vim.py) and the symmetric eigensolver they need. The method is not part of the reference snapshot; this block is its
 * definition, tests/vim_oracle.py its numpy restatement. Everything is fp64 except the features and logits (fp32). No floating-point
 * atomics: every sum has a fixed order that depends on the sizes alone, so every output is bit-identical from run to run. Nothing is
 * allocated or synchronised; every output element is written by the call; workspace contents are never assumed (ws:
 * osi_vim_workspace(M, K, F) bytes, 8-byte aligned, 0 for a non-positive argument or F or K > OSI_EIGH_MAX_F; the eigensolver alone
 * needs more than its first 64 bytes, and for it M and K are anything positive). OSI_ERR_ARG before any launch on a null required
 * pointer, a non-positive size, a short or misaligned workspace, a bad enum, an alpha that is not finite, F or K > OSI_EIGH_MAX_F and
 * 2^31 or more ELEMENTS in a matrix (M * F, M * K, M * (C + 1)); longer inputs go in row chunks.
 *
 * The eigensolver is parallel cyclic Jacobi on S[F][F], symmetric, of the kind osi_maha_scatter writes (the second moment
 * sum (x - o)(x - o)^T is osi_maha_scatter with C = 1, OSI_MAHA_TOTAL, mean = [anything; o] and labels 0). The caller owns A[F][F],
 * Vt[F][F], head[2], info[1] and hands the same ones to the three calls; two rows of OSI_EIGH_MAX_F doubles are the 64 KB of LDS of
 * one workgroup.
 * osi_eigh_begin: A <- S, Vt <- I, head[0] = ||S||_F (sum of squares in a fixed order: an entry above 1e154 overflows it),
 *   head[1] = tau = 2^-52 ||S||_F, info[0] = 1 when the norm is not finite, else 0.
 * osi_eigh_sweep: one sweep of the round-robin ordering over n = F rounded up to even players: n - 1 rounds (F - 1 for an even F, F
 *   with one bye each for an odd F) of floor(F / 2) disjoint pairs p < q; round r pairs the fixed player n - 1 with r and
 *   (r + m) mod (n - 1) with (r - m) mod (n - 1), m = 1 .. n / 2 - 1: a function of F and r alone. Every round takes its angles from the
 *   matrix as the previous round left it: the pair is rotated iff |a_pq| > tau, with theta = (a_qq - a_pp) / (2 a_pq),
 *   t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = 1), c = 1 / sqrt(t^2 + 1), s = t c; A <- J^T A J with a_pq = a_qp = 0
 *   set exactly, Vt <- J^T Vt (rows of Vt are the vectors). rotations[0] (int64) = the rotations of this sweep. Two launches a round,
 *   a function of F alone; with info[0] != 0 they leave at once and rotations[0] = 0. Only a_pq with p < q is tested: the two
 *   triangles of A are kept by different workgroups and may differ in their last bits.
 * osi_eigh_finish: evals[F] = the diagonal of A, descending, ties by index (a NaN last); evecs[k] = the matching row of Vt, signed so
 *   that its entry of largest magnitude (the first of equals) is positive. info[0] != 0: NaN values and zero vectors.
 *   Convergence is the caller's loop: begin, sweep until a sweep reports 0 rotations (one read-back per sweep), finish.
 * osi_vim_project_f32: z[M][K] (fp64), z[i][k] = sum_j ((double)x[i][j] - origin[j]) R[k][j] for R[K][F], one rounded fp64 subtraction
 *   per element, the products on the fp64 matrix instruction (the tile routine of ABI 25).
 * osi_vim_scores: from z[M][K] and logits[M][C] (fp32; not read by OSI_VIM_NORM, which takes NULL and any C), in fp64, row sums in an
 *   order fixed by K and C: OSI_VIM_NORM n_i = sqrt(sum_k z_ik^2), [M]; OSI_VIM_UNKNOWN alpha n_i - logsumexp(logits_i), [M];
 *   OSI_VIM_PROBS the max-subtracted softmax of [logits_i, alpha n_i], [M][C + 1], the virtual class last. An infinite maximum is not
 *   subtracted; a NaN in z or in the logits of a row propagates to every output of the row. Exactly one of out_f32 (rounded once from
 *   fp64) and out_f64 is non-null. */
enum { OSI_VIM_NORM = 0, OSI_VIM_UNKNOWN = 1, OSI_VIM_PROBS = 2 };
#define OSI_EIGH_MAX_F 4096
size_t osi_vim_workspace(int M, int K, int F);
int osi_eigh_begin(const double* S, int F, double* A, double* Vt, double* head, int* info, void* ws, size_t ws_bytes,
                   osi_stream_t stream);
int osi_eigh_sweep(double* A, double* Vt, int F, const double* head, const int* info, long long* rotations, void* ws, size_t ws_bytes,
                   osi_stream_t stream);
int osi_eigh_finish(const double* A, const double* Vt, int F, const int* info, double* evals, double* evecs, void* ws, size_t ws_bytes,
                    osi_stream_t stream);
int osi_vim_project_f32(const float* x, const double* origin, int M, int F, const double* R, int K, double* z, void* ws, size_t ws_bytes,
                        osi_stream_t stream);
int osi_vim_scores(const double* z, int M, int K, const float* logits, int C, double alpha, int mode, float* out_f32, double* out_f64,
                   void* ws, size_t ws_bytes, osi_stream_t stream);

/* ABI 27. Activation shaping on the pooled layer, scored with the energy of the re-computed logits (Sun, Guo, Li, "ReAct: Out-of-
 * distribution Detection With Rectified Activations", NeurIPS 2021; Djurisic, Bozanic, Ashok, Liu, "Extremely Simple Activation Shaping
 * for Out-of-Distribution Detection", ICLR 2023; Xu, Chen, Fang, Wang, Pan, "Scaling for Training Time and Post-hoc Out-of-distribution
 * Detection Enhancement", ICLR 2024; Liu, Wang, Owens, Li, "Energy-based Out-of-distribution Detection", NeurIPS 2020;
 * openset_imagenet/shaping.py). The methods are not part of the reference snapshot; this block is their definition,
 * tests/shaping_oracle.py its numpy restatement. They shape the network's penultimate activation (osi_resnet50_pooled, below, beside
 * the executor's other read-outs) and push it through the two head layers again (osi_linear_fwd). Nothing is allocated or
 * synchronised; every output element is written by the call; workspace contents are never assumed (8-byte aligned; the *_workspace
 * queries return 0 for arguments the call refuses). Every result is bit-identical from run to run and independent of the grid: the
 * only atomics count integers, every floating-point sum has a fixed order. OSI_ERR_ARG before any launch on a null required pointer, a
 * non-positive size, a size past its limit, a bad enum, a bad rank or keep, a short or misaligned workspace.
 *
 * The order, that of ABI 24: a value is read as v + 0.0f (-0 becomes +0), that canonical value is compared; values rank by IEEE order,
 *   every NaN after +Inf ascending, hence before +Inf descending (a NaN's payload is not part of the definition).
 * osi_order_stats_f32: out[r] (device, [R]) = the canonical value of the ranks[r]-th element, 0-based and ascending, of the n values
 *   v[0 .. n); a NaN is returned as the quiet NaN 0x7fc00000. ranks is a HOST array of R entries in [0, n), read during the call; they
 *   may repeat and come in any order. 1 <= R <= OSI_ORDER_STATS_MAX_R. n is 64-bit and v is read with plain 64-bit addressing: no
 *   2 GiB limit. No floating-point arithmetic but v + 0.0f: every output is an element of the input. Four radix passes of 8 bits over
 *   all n values, two launches a pass and one before them: 9 launches, a function of nothing; no host read-back between passes.
 *   ws: osi_order_stats_workspace(n, R) bytes.
 * osi_shape_rows: out[M][F] from x[M][F], 1 <= F <= OSI_SHAPE_MAX_F; out and x may not overlap. ws: osi_shape_rows_workspace(M, F)
 *   bytes (the kernels stage nothing in it and the size is a small constant).
 *   OSI_SHAPE_REACT: out = x > clip ? clip : x, so a NaN stays a NaN (and a NaN clip changes nothing); keep must be 0.
 *   Every other mode: 1 <= keep <= F, clip is ignored. The KEPT SET of a row is its first `keep` columns in descending order of the
 *   canonical values, NaN first; equal values, and NaNs among themselves, rank by ascending column. s1 = the sum of the whole row,
 *   s2 = the sum over the kept set, both of x as stored, in fp64 in an order fixed by F alone.
 *   OSI_SHAPE_ASH_P: x on the kept set (its bits), +0 elsewhere. OSI_SHAPE_ASH_B: (float)(s1 / keep) on the kept set, +0 elsewhere.
 *   OSI_SHAPE_ASH_S: x * (float)exp(s1 / s2) on the kept set, +0 elsewhere; the quotient and the exponential in fp64, rounded once to
 *   fp32, one fp32 product. OSI_SHAPE_SCALE: that product in every column. An all-zero row is not a special case: s1 / s2 = 0 / 0 is
 *   a NaN and so is every product with it (ASH_S: the kept columns, SCALE: all of them). A NaN or an Inf in a row reaches the sums
 *   as it is.
 * osi_logit_scores: out[M] from logits[M][C], computed in fp64 and rounded once, row sums in an order fixed by C. With m the row's
 *   maximum and m' = m when finite, else 0 (an infinite maximum is not subtracted), s = sum exp(l - m'): OSI_SCORE_ENERGY m' + ln s (the
 *   log-sum-exp); OSI_SCORE_MAXLOGIT m; OSI_SCORE_MSP exp(m - m') / s (the largest softmax probability). A row of -Inf gives -Inf,
 *   -Inf and NaN; a NaN in a row gives NaN under every mode. */
enum { OSI_SHAPE_REACT = 0, OSI_SHAPE_ASH_P = 1, OSI_SHAPE_ASH_B = 2, OSI_SHAPE_ASH_S = 3, OSI_SHAPE_SCALE = 4 };
enum { OSI_SCORE_ENERGY = 0, OSI_SCORE_MAXLOGIT = 1, OSI_SCORE_MSP = 2 };
#define OSI_ORDER_STATS_MAX_R 8
#define OSI_SHAPE_MAX_F 4096
size_t osi_order_stats_workspace(long long n, int R);
int osi_order_stats_f32(const float* v, long long n, const long long* ranks, int R, float* out, void* ws, size_t ws_bytes,
                        osi_stream_t stream);
size_t osi_shape_rows_workspace(int M, int F);
int osi_shape_rows(const float* x, int M, int F, int mode, int keep, float clip, float* out, void* ws, size_t ws_bytes,
                   osi_stream_t stream);
int osi_logit_scores(const float* logits, int M, int C, int mode, float* out, osi_stream_t stream);

/* ABI 29. Gradient-based open-set scores: the head of ODIN (Liang, Li, Srikant, "Enhancing The Reliability of Out-of-distribution Image
 * Detection in Neural Networks", ICLR 2018) and GradNorm's closed form for the last linear layer (Huang, Geng, Li, "On the Importance of
 * Gradients for Detecting Distributional Shifts in the Wild", NeurIPS 2021; openset_imagenet/odin.py). Neither is part of the reference
 * snapshot; this block is their definition, tests/odin_oracle.py its numpy restatement. One wave per row, everything in fp64 and
 * rounded once to fp32, row sums in an order fixed by C (respectively F) alone, the order of osi_logit_scores. No atomics, no workspace;
 * nothing is allocated or synchronised; every output element is written by the call; results are bit-identical from run to run and do
 * not depend on the alignment of the buffers. OSI_ERR_ARG before any launch on a null required pointer, a non-positive size, a
 * misaligned pointer (4 bytes; pred 8), T not finite or <= 0, dlogits overlapping logits.
 *
 * osi_odin_head: from logits[M][C] and the temperature T, per row
 *     y   = the index torch.argmax returns: a NaN counts as the largest value, the lowest index wins among equal maxima (and among NaNs)
 *     m   = the row's maximum (a NaN skipped), m' = m when it is finite, else 0 (the convention of osi_logit_scores)
 *     e_c = exp((l_c - m') / T)
 *     r   = sum over c != y of e_c: the predicted column is left out of the sum, not subtracted afterwards
 *     s   = sum over all c of e_c, in the order of osi_logit_scores (e_y + r up to the rounding of fp64 sums)
 *   score[M]      = e_y / s, the largest temperature-softmax probability S_y(x; T); at T = 1 the bits of OSI_SCORE_MSP
 *   pred[M]       = y (int64; may be NULL)
 *   dlogits[M][C] = e_c / s for c != y and -r / s for c = y (may be NULL). This is d(T J) / dlogits for J = -log S_y(x; T): T times the
 *     textbook gradient of one row, without the 1 / B of a batch mean. Only the sign of dJ/dx is used by ODIN, and this scaling keeps the
 *     seed's magnitude independent of T. -r / s rather than p_y - 1: no cancellation when one logit dominates.
 *   A NaN in a row gives NaN in score and in every dlogits element of the row; pred is the first NaN's column. A +Inf maximum is not
 *   subtracted, as under OSI_SCORE_MSP: score is Inf / Inf = NaN, dlogits is 0 in every finite column and -r / s = -0 or NaN in
 *   column y (NaN in every +Inf column when there are several). A row of -Inf gives score NaN, dlogits NaN and pred 0. C = 1 gives
 *   score 1 and dlogits -0 for a finite logit.
 * osi_gradnorm_scores: out[M] = ||f||_1 * (sum_c |C p_c - 1|) / T from features[M][F] and logits[M][C], with p_c = e_c / s as above: the
 *   L1 norm of d/dW sum_c -log p_c for the last linear layer logits = W features (the paper's loss with the all-ones target; a bias
 *   does not enter). Higher means more known. Features of either sign. A NaN in either row, or an infinite maximum, gives NaN. */
int osi_odin_head(const float* logits, int M, int C, float T, float* dlogits /* [M][C] or NULL */, long long* pred /* [M] or NULL */,
                  float* score /* [M] */, osi_stream_t stream);
int osi_gradnorm_scores(const float* features, const float* logits, int M, int F, int C, float T, float* out, osi_stream_t stream);

/* ---- optimizer + arena utilities (train.py:356-359 construction, train.py:127,139 zero_grad/step) --- */
int osi_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                  double beta2, double eps, long long step, float grad_scale, osi_stream_t stream);
int osi_sgd_step(float* param, const float* grad, float* momentum_buf, size_t n, float lr, float momentum, int first_step,
                 float grad_scale, osi_stream_t stream);
/* ABI 11. The same steps with parameter groups: ONE launch over the arena, every 16-byte unit (4 floats) updated under the options of
 * the segment it lies in. A segment is a run [begin4, end4) of units with a group index; segments are sorted by begin4, do not overlap,
 * are not empty, end at or before n/4 and need not cover the arena: units outside every segment are neither read nor written, in the
 * parameter arena or any state arena. segments and groups are HOST pointers, read during the call (they travel in the kernel
 * arguments) and not needed afterwards. Arithmetic is torch's single-tensor path (torch.optim.Adam / AdamW / SGD); the scalars are
 * prepared in double as osi_adam_step does, and a group with default options (weight_decay 0, not decoupled, no amsgrad, no nesterov,
 * dampening 0, no maximize) gives the bits of osi_adam_step / osi_sgd_step. OSI_ERR_ARG before any launch on: a null pointer
 * (max_exp_avg_sq may be NULL unless a group has amsgrad), n % 4 != 0 or n/4 > 2^32 - 512, n_segments outside 1..OSI_OPT_MAX_SEGMENTS,
 * n_groups outside 1..OSI_OPT_MAX_GROUPS, a malformed segment table, a group index out of range, step < 1, nesterov with
 * momentum <= 0 or dampening != 0. */
#define OSI_OPT_MAX_SEGMENTS 192
#define OSI_OPT_MAX_GROUPS 16
typedef struct {
    unsigned int begin4, end4; /* in units of 4 floats */
    int group;
} osi_opt_segment;
typedef struct {
    double lr, beta1, beta2, eps, weight_decay;
    long long step;     /* step count of this group's parameters AFTER this step (>= 1) */
    int decoupled;      /* 1: AdamW, p *= 1 - lr*weight_decay; 0: L2, g += weight_decay*p */
    int amsgrad, maximize;
} osi_adam_group;
typedef struct {
    double lr, momentum, dampening, weight_decay;
    int nesterov;
    int first_step;     /* 1: the momentum buffer is initialised with the gradient (torch's first step) */
    int maximize;
} osi_sgd_group;
int osi_adam_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                         const osi_opt_segment* segments, int n_segments, const osi_adam_group* groups, int n_groups,
                         float grad_scale, osi_stream_t stream);
int osi_sgd_step_groups(float* param, const float* grad, float* momentum_buf, size_t n, const osi_opt_segment* segments,
                        int n_segments, const osi_sgd_group* groups, int n_groups, float grad_scale, osi_stream_t stream);
/* ABI 17. Gradient-norm clipping without a host read: osi_grad_clip_scale leaves the norm and the scalar of the step in device memory,
 * and the *_dev forms of the grouped steps take that scalar from there.
 *
 * osi_grad_clip_scale writes two floats: out2[0] = |grad_scale| * ||g||, the norm (OSI_NORM_L2, or OSI_NORM_INF: the largest |g|)
 * over the elements inside the spans, and out2[1] = grad_scale * min(1, max_norm / (out2[0] + 1e-6f)), evaluated in fp32 as
 * torch.nn.utils.clip_grad_norm_ evaluates its coefficient on the gradients grad_scale * g (the quotient with torch's roundings:
 * reciprocal(out2[0] + 1e-6f) * max_norm). A NaN norm gives a NaN scalar (torch's clamp keeps a NaN); max_norm = +inf gives exactly grad_scale for a finite norm ("measure only").
 * A span is one tensor: numel floats from float index begin (begin % 4 == 0, numel >= 1). spans is a HOST table of 1 ..
 * OSI_OPT_MAX_SEGMENTS entries, sorted and not overlapping, read during the call (it travels in the kernel arguments); spans == NULL
 * with n_spans == 0 means [0, n). The up to 3 alignment floats behind a span with numel % 4 != 0, and every float outside every span,
 * contribute nothing, whatever bits they hold.
 * L2 squares and sums in double ((double)g * g is exact), so magnitudes whose squares leave the fp32 range give correct norms. The
 * reduction has a fixed order and no atomics: the arena is cut into one contiguous chunk of whole 256-unit tiles per workgroup (at most
 * 2048, as the grouped steps cut it); per lane in index order, then wave, workgroup, one 8-byte partial in ws per workgroup; a second
 * launch of one workgroup adds the partials, eight consecutive ones per lane in index order, then the same tree, and writes out2. Two
 * calls on the same data give the same bits. Two launches, nothing allocated, nothing synchronised (graph-capturable).
 * ws: osi_grad_norm_workspace(n) bytes (0 for an n the call would refuse), 8-byte aligned, overwritten (workspace contents are never
 * assumed). grad 16-byte aligned.
 * OSI_ERR_ARG before any launch on: a null or misaligned grad, ws or out2; n == 0, n % 4 != 0 or n/4 > 2^32 - 512; ws_bytes too
 * small; a malformed span table (begin % 4 != 0, numel == 0, unsorted, overlapping, past n, n_spans outside 1..OSI_OPT_MAX_SEGMENTS,
 * or NULL with n_spans != 0); a norm_type other than the two constants; max_norm negative or NaN; a non-finite grad_scale.
 *
 * osi_adam_step_groups_dev / osi_sgd_step_groups_dev: the contract of osi_adam_step_groups / osi_sgd_step_groups, with the scalar
 * read by the kernel from *grad_scale_dev (device memory, 4-byte aligned, written by earlier work on the stream, e.g. out2 + 1): the
 * result is the bits of the host-scalar entry point called with grad_scale = that value. */
#define OSI_NORM_INF 0
#define OSI_NORM_L2 2
typedef struct {
    unsigned long long begin, numel; /* in floats; begin % 4 == 0, numel >= 1 */
} osi_grad_span;
size_t osi_grad_norm_workspace(size_t n);
int osi_grad_clip_scale(const float* grad, size_t n, const osi_grad_span* spans, int n_spans, int norm_type, float grad_scale,
                        float max_norm, void* ws, size_t ws_bytes, float* out2, osi_stream_t stream);
int osi_adam_step_groups_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                             const osi_opt_segment* segments, int n_segments, const osi_adam_group* groups, int n_groups,
                             const float* grad_scale_dev, osi_stream_t stream);
int osi_sgd_step_groups_dev(float* param, const float* grad, float* momentum_buf, size_t n, const osi_opt_segment* segments,
                            int n_segments, const osi_sgd_group* groups, int n_groups, const float* grad_scale_dev,
                            osi_stream_t stream);
int osi_fill_f32(float* p, size_t n, float value, osi_stream_t stream);
int osi_scale_f32(float* p, size_t n, float s, osi_stream_t stream);
/* ABI 10. dst[i] += src[i] (one fp32 add per element): the sum of two gradient arenas, e.g. the clean and the adversarial backward of
 * one training step. 16-byte aligned, distinct pointers, n % 4 == 0 (OSI_ERR_ARG otherwise). */
int osi_grad_accumulate(float* dst, const float* src, size_t n, osi_stream_t stream);
int osi_i64_add(long long* p, int n, long long inc, osi_stream_t stream);
/* ABI 20. Weight averaging (EMA / SWA, openset_imagenet/averaging.py): avg = lerp(avg, cur, weight) over up to OSI_AVG_MAX_SPANS pairs
 * of arenas in ONE launch, with the roundings of torch.lerp on fp32: d = cur - avg (one rounding), then avg = fma(weight, d, avg) for
 * weight < 0.5 and avg = fma(weight - 1, d, cur) otherwise (weight - 1 rounded once to fp32); the fma is explicit, so no contraction
 * setting changes the bits. weight = 1 reproduces cur exactly whenever d is finite (the difference does not overflow), weight = 0
 * leaves finite values unchanged, and NaN / Inf come out where torch.lerp puts them.
 * A span is n floats of `avg` (read and written) and of `cur` (only read); nothing outside [avg, avg + n) is written. spans is a HOST
 * table, read during the call (it travels in the kernel arguments) and not needed afterwards. The spans are cut into tiles of 1024
 * floats (one 16-byte unit per lane of a 256-thread workgroup) that at most 2048 workgroups walk in a grid stride, whichever span a
 * tile lies in. 16-byte loads and stores, no atomics, nothing allocated, nothing synchronised (graph-capturable).
 * OSI_ERR_ARG before any launch on: a NULL table or n_spans outside 1..OSI_AVG_MAX_SPANS; a NULL or not 16-byte aligned avg or cur;
 * n == 0, n % 4 != 0 or n/4 > 2^32 - 512; weight NaN or outside [0, 1]; an avg range that overlaps any cur range (its own included)
 * or another avg range. */
#define OSI_AVG_MAX_SPANS 4
typedef struct {
    float* avg;
    const float* cur;
    size_t n; /* floats; n % 4 == 0, both pointers 16-byte aligned */
} osi_avg_span;
int osi_average_update(const osi_avg_span* spans, int n_spans, float weight, osi_stream_t stream);

/* ---- whole-network executor: ResNet50.forward (model.py:28-39) and its autograd backward (train.py:138) ---------------
 * One call enqueues the full forward (or a range of backward stages) on `stream`. The caller owns three flat arenas whose
 * layout is reported by the *_info queries:
 *   params   fp32   all 161 weight tensors in nn.Module registration order (conv KRSC, BN gamma/beta, fc, logits)
 *   grads    fp32   same layout as params
 *   buffers  fp32   BN running_mean / running_var (53 x 2)      nbt: int64[53] num_batches_tracked
 * and a workspace of osi_resnet50_workspace_bytes() holding activations, saved statistics and scratch. */
typedef struct osi_resnet50* osi_resnet50_t;

int osi_resnet50_create(osi_resnet50_t* out, int B, int H, int W, int fc_dim, int out_features, int logit_bias);
void osi_resnet50_destroy(osi_resnet50_t net);
int osi_resnet50_num_tensors(osi_resnet50_t net);             /* parameter tensors */
/* name: reference state_dict key ("resnet_base.layer1.0.conv1.weight"); shape in torch order (OIHW for convs), ndim <= 4;
 * offset/numel in floats inside the params/grads arena */
int osi_resnet50_tensor_info(osi_resnet50_t net, int i, char* name, int name_cap, int* ndim, int* shape, size_t* offset,
                             size_t* numel);
size_t osi_resnet50_param_floats(osi_resnet50_t net);         /* arena length, multiple of 4 */
int osi_resnet50_num_bn(osi_resnet50_t net);
/* BN layer j: prefix ("resnet_base.layer1.0.bn1"), channel count, offsets of running_mean / running_var in `buffers` */
int osi_resnet50_bn_info(osi_resnet50_t net, int j, char* prefix, int cap, int* C, size_t* rm_offset, size_t* rv_offset);
size_t osi_resnet50_buffer_floats(osi_resnet50_t net);
size_t osi_resnet50_workspace_bytes(osi_resnet50_t net);
int osi_resnet50_num_stages(osi_resnet50_t net);              /* backward stages (gradient buckets), head first */
/* the fixed geometry the executor was created for: batch, image height, image width (any pointer may be NULL) */
int osi_resnet50_geometry(osi_resnet50_t net, int* B, int* H, int* W);
/* floats [lo, hi) of the grads arena that are final once backward stage s has run */
int osi_resnet50_stage_grad_range(osi_resnet50_t net, int s, size_t* lo, size_t* hi);

/* Optional input staging from a uint8 [B][H][W][3] batch (osi_u8hwc3_to_nhwc4 into the executor's input buffer inside
 * `workspace`); the next osi_resnet50_forward on that workspace passes image = NULL (OSI_ERR_STATE without a staged input). */
int osi_resnet50_stage_input_u8(osi_resnet50_t net, const unsigned char* images_u8_nhwc, const unsigned char* flip,
                                void* workspace, osi_stream_t stream);
/* Alternative to staging: bind an NHWC4 fp32 batch [B][H][W][4] that already lives in device memory (e.g. written by
 * osi_u8_crop_flip_to_nhwc4 on a copy stream, one batch ahead); the next osi_resnet50_forward with image = NULL reads it in place
 * and that step's stem weight gradient reads it again, so it must stay untouched until the step's backward has run. */
int osi_resnet50_bind_input_nhwc4(osi_resnet50_t net, const float* x_nhwc4);
/* image: [B][3][H][W] fp32 NCHW as the reference feeds it (or NULL after osi_resnet50_stage_input_u8 /
 * osi_resnet50_bind_input_nhwc4). training != 0: batch statistics + running-stat update. */
int osi_resnet50_forward(osi_resnet50_t net, const float* params, float* buffers, long long* nbt, const float* image,
                         void* workspace, float* logits, float* features, int training, osi_stream_t stream);
/* ABI 12. Differentiable forward on FROZEN BatchNorm statistics (eval-mode gradients, fine-tuning with frozen statistics): the training
 * topology (pre-BN tensors, block-output bitmasks, arg-max bytes) on the running statistics, all 53 coefficient sets from one launch
 * (osi_bn_frozen_coeffs_multi). buffers are only read; num_batches_tracked is not an argument. Outputs: the bits of
 * osi_resnet50_forward(training = 0) under option eval_fused = 0. The backward that follows (osi_resnet50_backward / _ex / _adv, any
 * stage split) runs the frozen dataflow: dy = scale * g in the in-block input-gradient epilogues (osi_conv_dgrad_fused_frozen, the 3x3
 * stride-1 layers included: no Winograd form), osi_bn_backward_frozen at block outputs, osi_bn_relu_maxpool_bwd_frozen + the
 * materialised stem tail; param_grads = 0 launches no reduction at all. A later osi_resnet50_forward of any kind replaces this state
 * (a backward after an inference forward: OSI_ERR_STATE). */
int osi_resnet50_forward_frozen(osi_resnet50_t net, const float* params, const float* buffers, const float* image, void* workspace,
                                float* logits, float* features, osi_stream_t stream);
/* runs backward stages [stage_lo, stage_hi) given dJ/dlogits and (optionally, may be NULL) dJ/dfeatures */
int osi_resnet50_backward(osi_resnet50_t net, const float* params, float* grads, void* workspace, const float* dlogits,
                          const float* dfeatures, int stage_lo, int stage_hi, osi_stream_t stream);

/* ABI 8. osi_resnet50_backward plus: dimage != NULL -> the last stage also writes dJ/dimage, [B][3][H][W] fp32 NCHW (the stem tail then
 * materialises the stem's output gradient: bn1 backward into a scratch buffer, the stem weight gradient from it, osi_stem_dgrad);
 * param_grads == 0 -> no parameter gradient is computed or written (grads may be NULL): no weight-gradient launch, no fc / logits
 * dw / db, nothing on the side stream; the BatchNorm reductions dY needs still run (into workspace). dimage / param_grads are fixed by
 * the call that runs stage 0; a later stage of the same backward with other values -> OSI_ERR_STATE. param_grads == 0 with
 * dimage == NULL, or param_grads == 1 with grads == NULL -> OSI_ERR_ARG. osi_resnet50_backward(...) = _ex(..., NULL, 1, ...). */
int osi_resnet50_backward_ex(osi_resnet50_t net, const float* params, float* grads, void* workspace, const float* dlogits,
                             const float* dfeatures, float* dimage, int param_grads, int stage_lo, int stage_hi,
                             osi_stream_t stream);

/* ABI 10. The full training backward (parameter gradients exactly as osi_resnet50_backward_ex(dimage != NULL, param_grads = 1) writes
 * them: the stem tail takes the same dY-materialising branch) whose last stage, instead of dJ/dimage, writes the FGSM batch
 *   x_adv = clamp(x + eps * sign(dJ/dimage), lo, hi)     [B][H][W][4] fp32, 4th lane zero (osi_stem_dgrad_fgsm)
 * built from the NHWC4 input the forward read — the converted copy in the workspace, the staged uint8 batch or the batch bound with
 * osi_resnet50_bind_input_nhwc4; the caller does not pass it. x_adv_nhwc4: 16-byte aligned, outside `workspace` and apart from the bound
 * input (conv1's weight gradient still reads the clean batch), eps >= 0, lo <= hi: OSI_ERR_ARG otherwise. The request (pointer, eps, lo,
 * hi) is fixed by the call that runs stage 0; a later stage with other values -> OSI_ERR_STATE. */
int osi_resnet50_backward_adv(osi_resnet50_t net, const float* params, float* grads, void* workspace, const float* dlogits,
                              const float* dfeatures, float* x_adv_nhwc4, float eps, float lo, float hi, int stage_lo, int stage_hi,
                              osi_stream_t stream);

/* ABI 19. A backward whose last launch is one step of a projected attack (osi_stem_dgrad_pgd) from the batch the forward read (the
 * iterate) towards x_next, projected onto the eps-ball around x_anchor:
 *   x_next = clamp(min(max(x + alpha * sign(dJ/dimage), a - eps), a + eps), lo, hi)     [B][H][W][4] fp32, 4th lane zero.
 * param_grads = 1: parameter gradients are the bits of osi_resnet50_backward_adv (the same dY-materialising stem tail).
 * param_grads = 0: the input-only dataflow of osi_resnet50_backward_ex(dimage, 0) — grads may be NULL, no weight-gradient launch, no
 * fc / logits dw / db, nothing on the side stream, the BatchNorm reductions dY needs go into the workspace — and only its last launch
 * differs: the attack epilogue instead of osi_stem_dgrad. Valid after osi_resnet50_forward(training = 1) and after
 * osi_resnet50_forward_frozen; after a forward with an inference-form prefix -> OSI_ERR_STATE, as _adv. x_next: 16-byte aligned,
 * outside `workspace`, apart from the input the forward read and from x_anchor; x_anchor: 16-byte aligned or NULL; alpha finite,
 * eps >= 0 (+inf allowed), lo <= hi; param_grads 0 or 1, grads non-NULL when 1: OSI_ERR_ARG otherwise. The request (all six fields and
 * param_grads) is fixed by the call that runs stage 0; a later stage with another request -> OSI_ERR_STATE.
 * osi_resnet50_backward_adv(x_adv, eps, lo, hi) = _attack({x_adv, NULL, eps, eps, lo, hi}, 1), the same bits: with the anchor the
 * iterate itself and alpha = eps the projection changes nothing. */
typedef struct {
    float* x_next;          /* [B][H][W][4], 16-byte aligned, outside workspace, apart from the input the forward read and from x_anchor */
    const float* x_anchor;  /* [B][H][W][4] or NULL = the batch the forward read (NCHW-converted copy, staged uint8 batch or bound NHWC4) */
    float alpha, eps, lo, hi;
} osi_attack;
int osi_resnet50_backward_attack(osi_resnet50_t net, const float* params, float* grads, void* workspace, const float* dlogits,
                                 const float* dfeatures, const osi_attack* a, int param_grads, int stage_lo, int stage_hi,
                                 osi_stream_t stream);

/* Data-parallel hand-off (ABI 5). With option "stage_join" = 0 a staged osi_resnet50_backward call (stage_hi < stages) does NOT make
 * `stream` wait for the side stream's weight gradients (the last stage always does); instead the caller makes its COMMUNICATION stream
 * wait for everything the finished stages produced: osi_resnet50_grads_ready(net, main, waiter) records the progress of `main` (the
 * stream the backward calls were issued on) and of the executor's side stream and makes `waiter` wait for both — `main` itself waits
 * for nothing and goes on with the next stage while the collective runs (reference intent: config/train.yaml:18,35-39). */
int osi_resnet50_grads_ready(osi_resnet50_t net, osi_stream_t main_stream, osi_stream_t waiter_stream);

/* ABI 13. Fine-tuning a suffix. The network is 18 UNITS in forward order: 0 = the stem (conv1, bn1), 1 .. 16 = the bottlenecks
 * layer1.0 .. layer4.2 (three convolutions, three BatchNorms, plus the downsample pair on block 0 of a layer), 17 = the head (fc,
 * logits). tensor_unit / bn_unit: the unit of parameter tensor i / BatchNorm j, -1 on a bad index.
 * osi_resnet50_set_trainable(net, unit_mask, eval_prefix_units): bit u of unit_mask = unit u has a parameter somebody trains; c = the
 * lowest set bit is the CUT, the units below it the frozen prefix. Default (0x3FFFF, 0): every launch of every entry point as before.
 *   backward without an image gradient (osi_resnet50_backward; _ex with dimage = NULL, param_grads = 1): runs from the head down to
 *     unit c and launches nothing more. The gradient w.r.t. unit c's input is not computed: block c leaves out conv1's input gradient
 *     (the one fused with the previous block's gate and reductions) and the downsample's input gradient; c = 1 leaves out block 0's
 *     pool-mode input gradient and the whole stem tail; c = 17 leaves out fc's dx and osi_avgpool_bwd. Unit c's own BatchNorm
 *     reductions arrive as ever (in-unit input-gradient epilogues; the block above, or the stage-entry BatchNorm backward). A stage
 *     wholly below the cut is accepted in order, launches nothing, advances and joins; the last stage ends the backward.
 *   every backward (plain, _ex with dimage, _adv): a frozen unit (bit clear) gets no conv / fc / logits weight-gradient launch and
 *     its slices of `grads` are not written; under frozen statistics its parameter-only BatchNorm reductions are left out, under batch
 *     statistics the reductions dx needs still run (into workspace). With dimage / x_adv the input gradients run to full depth.
 *   forward with eval_prefix_units = p > 0 (osi_resnet50_forward(training = 1), osi_resnet50_forward_frozen; training = 0 ignores
 *     p): units 0 .. p-1 run the inference forms on the running statistics (coefficients from one osi_bn_eval_coeffs_multi launch over
 *     their BatchNorms), keep no backward state, update neither running statistics nor num_batches_tracked; units p .. 17 run the
 *     requested topology (running-statistics update and num_batches_tracked + 1, or osi_bn_frozen_coeffs_multi, over their BatchNorms
 *     only). After such a forward a backward with dimage / x_adv returns OSI_ERR_STATE and launches nothing, and
 *     osi_resnet50_debug_gate returns OSI_ERR_STATE for the gates of units below p.
 * The setting takes effect at the next forward and holds for it and its backward: a call between a differentiable forward and the last
 * stage of its backward returns OSI_ERR_STATE (option "forget_forward" gives such a forward up). OSI_ERR_ARG: unit_mask == 0 (that is
 * param_grads = 0), a bit at or above 18, eval_prefix_units < 0 or > c. */
int osi_resnet50_num_units(osi_resnet50_t net);                 /* 18 */
int osi_resnet50_tensor_unit(osi_resnet50_t net, int i);
int osi_resnet50_bn_unit(osi_resnet50_t net, int j);
int osi_resnet50_set_trainable(osi_resnet50_t net, unsigned unit_mask, int eval_prefix_units);
int osi_resnet50_get_trainable(osi_resnet50_t net, unsigned* unit_mask, int* eval_prefix_units);

/* ABI 20. The running-statistics update factor of the executor: running = (1 - momentum) * running + momentum * batch for every
 * BatchNorm a training-mode forward finalises (all of them go through osi_bn_finalize_stats, the stem's included). Default 0.1f: the
 * launches and bits of every earlier ABI. The value takes effect at the next osi_resnet50_forward(training = 1); inference and frozen
 * forwards never read it, and no kernel's arithmetic changes. momentum = 1 leaves exactly the batch statistics in the buffers
 * ((1 - 1) * running is an exact zero for a finite running value); 1 / k before batch k = 1, 2, ... from reset buffers is the
 * cumulative average of torch's BatchNorm with momentum = None (update_bn). OSI_ERR_ARG: NaN, momentum <= 0 or > 1, a NULL pointer. */
int osi_resnet50_set_bn_momentum(osi_resnet50_t net, float momentum);
int osi_resnet50_get_bn_momentum(osi_resnet50_t net, float* momentum);

/* ABI 23. Manifold mixup at the frozen cut (PROSER). osi_resnet50_set_mix is a ONE-SHOT request for the next differentiable forward
 * (osi_resnet50_forward(training = 1) or osi_resnet50_forward_frozen): partner / weight are device arrays of B entries as
 * osi_mix_rows_pairs takes them and must stay valid until that forward's launches are enqueued; both NULL clears the request (one
 * NULL: OSI_ERR_ARG). With the request pending and eval_prefix_units = p in 1 .. 16 (osi_resnet50_set_trainable) the forward launches
 * osi_mix_rows_pairs on the input of unit p — [B][H * W * C] in the workspace, written by unit p - 1 (the stem's pool for p = 1) —
 * after unit p - 1 has written it and before anything of unit p reads it: conv1, the projection shortcut (the side stream forks
 * after the launch) and the residual add of an identity block. The weight gradients of conv1 and the shortcut in the backward read
 * the same tensor and therefore see the mixed input, which is the correct gradient. The prefix below the cut is frozen, the backward
 * ends at the cut, no gradient ever crosses the mix: it has no backward. p outside 1 .. 16: the forward returns OSI_ERR_STATE, launches
 * nothing and leaves the request pending. An inference forward ignores the request and leaves it pending; the differentiable forward
 * that runs it consumes it. After a forward with a mix a backward with dimage / x_adv returns OSI_ERR_STATE (the rule of every forward
 * with an inference-form prefix). Without a request every entry point issues the launches of ABI 22. */
int osi_resnet50_set_mix(osi_resnet50_t net, const int* partner, const float* weight);

/* ABI 27. The penultimate activation of the latest forward: the [B][2048] average-pooled output of layer4 (non-negative: the mean of
 * a block-output ReLU) as it lies in `workspace`, copied to `out` (device memory) on `stream`; *floats = B * 2048. out = NULL only
 * reports the size (workspace may then be NULL too). Read-only: no executor state changes. Valid after a forward of ANY kind -
 * training, inference (fused or not) and frozen: every entry point runs the one head (average pool -> fc -> logits) that writes the
 * tensor, and no backward overwrites it (the head's backward reads it). This is the activation ReAct, ASH and SCALE shape (above,
 * osi_shape_rows); features = fc(pooled) and logits = logits(features) are osi_linear_fwd on it, bit for bit.
 * OSI_ERR_ARG on a NULL net or floats, or a NULL workspace with out; OSI_ERR_STATE for a copy before any forward. */
int osi_resnet50_pooled(osi_resnet50_t net, void* workspace, float* out, size_t* floats, osi_stream_t stream);

/* Per-executor switches: "overlap" (default 1: weight gradients on a low-priority side stream, overlapped with dgrad / BatchNorm
 * backward and joined back into `stream` at the end of every backward call unless "stage_join" = 0; 0 serialises everything on the
 * caller's stream), "fwd_fork" (projection shortcut of the forward pass on the side stream, default 1), "side_priority_normal" (side
 * stream at default instead of lowest priority; only before the first training call, else OSI_ERR_STATE), "stage_join" (default 1; see
 * osi_resnet50_grads_ready), "eval_fused" (default 1: a forward with training = 0 runs the inference forms — every BatchNorm +
 * shortcut + ReLU in its convolution's epilogue, no pre-BN tensor, no block-output pass, no bitmask, one coefficient launch for all 53
 * BatchNorms; 0 = the training topology on running statistics, kept for A/B: bit-identical when both run the same launch plans (knob
 * "tail_split" off), fp32-rounding-level differences otherwise), "forget_forward" (an action, value != 0: the latest differentiable
 * forward will get no backward; its state is given up, so osi_resnet50_set_trainable is accepted again).
 * Unknown name -> OSI_ERR_ARG; so are the settled A/B switches retired with ABI 9. */
int osi_resnet50_set_option(osi_resnet50_t net, const char* name, int value);

/* Optional HIP-event instrumentation of the executor (bench.py's roofline leg): one event after every op on the launch
 * stream, attributed to a kernel class. profile_read synchronises on the last event — call it outside timed regions. */
enum { OSI_PROF_START = 0, OSI_PROF_CONV_FWD = 1, OSI_PROF_CONV_DGRAD = 2, OSI_PROF_CONV_WGRAD = 3, OSI_PROF_BN_FWD = 4,
       OSI_PROF_BN_BWD = 5, OSI_PROF_OTHER = 6, OSI_PROF_NCLASS = 7 };
int osi_resnet50_profile(osi_resnet50_t net, int enable);
int osi_resnet50_profile_read(osi_resnet50_t net, double* ms_per_class, int* ops_per_class);
/* osi_resnet50_profile(net, 2) = timeline mode: the side-stream overlap stays on and each op's completion event remembers its
 * stream. timeline_read synchronises, then fills completion times (ms since the first event), classes and stream flags of up to
 * `cap` ops and resets the log. Dev instrumentation (tools/timeline.py): how far the weight gradients trail the critical path. */
int osi_resnet50_timeline_read(osi_resnet50_t net, double* t_ms, int* cls, int* on_side, int cap, int* count);


/* ---- debug: the non-smooth decisions of the latest forward (TEST INFRASTRUCTURE — nothing on the product path calls these) ----
 * The reference's backward (j.backward(), openset_imagenet/train.py:138) differentiates through 49 ReLUs (torchvision's stem ReLU +
 * three per Bottleneck) and one max-pool arg-max (model.py:17); a whole-network gradient comparison is only tight when both sides
 * take the same branch at every one of them. Gate i of osi_resnet50_debug_num_gates() = 1 + 3 x 16, in forward order: 0 = the
 * stem ReLU as the max-pool output sees it (shape [B][64][Hp][Wp]: the gate of the pooled element, all the backward ever uses),
 * then per bottleneck the ReLU after bn1, after bn2 and the block-output ReLU. Each is read from what the backward kernels
 * themselves consume (stored bitmask / the gate recomputed from the pre-BN tensor / the arg-max byte). Output: one byte (0 / 1)
 * per element in NCHW order [B][C][H][W]; pool_argmax_nchw (gate 0 only, may be NULL): int32 flat index h * Ws + w into the
 * stem's [Hs][Ws] plane, the convention of torch.nn.functional.max_pool2d(return_indices=True). OSI_ERR_STATE before any forward. */
int osi_resnet50_debug_num_gates(osi_resnet50_t net);
int osi_resnet50_debug_gate_shape(osi_resnet50_t net, int i, int* C, int* H, int* W);
int osi_resnet50_debug_gate(osi_resnet50_t net, void* workspace, int i, unsigned char* gate_nchw, int* pool_argmax_nchw,
                            osi_stream_t stream);
/* ABI 23. The input tensor of block unit 1 .. 16 as the latest forward of any kind left it in `workspace` (what that unit's conv1
 * consumed: the mixed tensor after a forward with osi_resnet50_set_mix): [B][H][W][C] fp32, copied to out_nhwc (device memory) on
 * `stream`; *floats = B * H * W * C. out_nhwc = NULL only reports the size (workspace may then be NULL too). OSI_ERR_ARG on a unit
 * outside 1 .. 16 or floats == NULL; OSI_ERR_STATE for a copy before any forward. */
int osi_resnet50_debug_unit_input(osi_resnet50_t net, void* workspace, int unit, float* out_nhwc, size_t* floats, osi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* OSI_H */
