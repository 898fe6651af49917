// Whole-network executor: one C call enqueues the complete ResNet-50 forward (or a range of backward stages)
// of the reference model on a HIP stream — no per-layer host round trips, graph-capturable.
//
// Topology restated from the reference's only constructor call, openset_imagenet/model.py:17-26
// (torchvision.models.resnet50 = ResNet v1.5: stride on the 3x3 of the first block of stages 2-4, Bottleneck
// expansion 4, 1x1-stride-s + BN downsample on block 0 of each stage; then fc = Linear(2048, fc_dim) and
// logits = Linear(fc_dim, out_features, bias=logit_bias)); forward = model.py:28-39; backward = the autograd
// graph that openset_imagenet/train.py:138 (j.backward()) walks. Parameter order and names = nn.Module
// registration order, i.e. the reference checkpoint's state_dict keys.
#include "osi_common.h"
#include <string>
#include <vector>
#include <cstring>
#include <cstdio>

#define OSI_TRY(x)                 \
    do {                           \
        int e__ = (x);             \
        if (e__ != OSI_OK) return e__; \
    } while (0)

namespace {

constexpr size_t WS_NONE = (size_t)-1;   // workspace offset of a tensor the layer does not have

struct Tensor {
    std::string name;
    int ndim; int shape[4];
    size_t off, numel;  // floats in the param arena
    int unit;           // fine-tuning unit (0 = stem, 1..16 = bottlenecks in forward order, 17 = head)
};
struct BN {
    std::string prefix;
    int C, M;
    size_t g_off, b_off;    // param arena
    size_t rm_off, rv_off;  // buffer arena
    size_t mean, invstd, scale, shift;  // workspace (floats)
    size_t dsink;           // workspace: [2][C] dgamma / dbeta of a backward that writes no parameter gradient
    int unit;
};
struct Conv {
    osi_conv_desc d;
    size_t w_off;  // param arena
    int bn;
    size_t y;      // workspace: conv output (pre-BN)
    size_t a;      // workspace: BN(+res)+ReLU output (WS_NONE unless it is a block output)
    size_t mask;   // workspace: ReLU bitmask of `a` (1 bit per element)
    size_t u_fw = WS_NONE, u_bw = WS_NONE;   // workspace: Winograd-transformed weights (forward / input-gradient form), 3x3 stride-1 layers only
    int unit;
};
struct Block {
    int c1, c2, c3, ds;  // conv indices, ds = -1 if identity skip
    size_t x_in;         // workspace offset of the block input
    size_t out;          // = convs[c3].a
    int stage;           // backward stage this block belongs to
};

constexpr size_t ALIGN_F = 64;  // floats (256 B)
// The executor's INTERNAL events only order streams of ONE device against each other (fork / join of the weight-gradient side stream,
// reader events of the scratch buffers). By default a HIP event performs a SYSTEM-scope fence when it is recorded — a cache writeback +
// invalidate that makes device memory visible to the host and to other devices — which none of them needs: the kernels on both sides
// carry their own agent-scope acquire / release. ~115 records per step.
constexpr unsigned EV_FLAGS = hipEventDisableTiming | hipEventDisableSystemFence;
// The two events of the data-parallel hand-off (osi_resnet50_grads_ready) are different: their consumer is RCCL's all-reduce, whose
// peers read this device's gradient arena over xGMI. They keep the system-scope release (<= 8 records per step).
constexpr unsigned EV_FLAGS_HANDOFF = hipEventDisableTiming;
static size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static void grow(size_t& m, size_t v) { if (v > m) m = v; }
static int device_cus() {   // CUs of the CURRENT device (the launch plans are balanced for them): 0 when no device answers
    int v = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return v;
}

// What a backward is asked for (osi_resnet50_backward_ex / _adv / _attack). dimage != NULL: the stem tail materialises dY and its input gradient
// writes dJ/dimage. param_grads = 0: input-only (no weight gradient, nothing into grads). x_adv != NULL: the stem tail materialises dY as
// for dJ/dimage and the stem's input gradient ends in the FGSM epilogue (osi_stem_dgrad_fgsm) that writes the adversarial NHWC4 batch;
// dJ/dimage itself is never written. x_anchor / alpha (osi_resnet50_backward_attack): the epilogue is the projected step of
// osi_stem_dgrad_pgd, alpha along the sign and back onto the eps-ball around x_anchor (NULL: around the batch the forward read).
// osi_resnet50_backward_adv is the request {x_anchor = NULL, alpha = eps}, for which the projection is the identity.
struct BwRequest {
    float* dimage = nullptr;
    int param_grads = 1;
    float* x_adv = nullptr;
    float eps = 0.f, lo = 0.f, hi = 0.f;
    const float* x_anchor = nullptr;
    float alpha = 0.f;
    bool operator==(const BwRequest& o) const {
        return dimage == o.dimage && param_grads == o.param_grads && x_adv == o.x_adv && eps == o.eps && lo == o.lo && hi == o.hi &&
               x_anchor == o.x_anchor && alpha == o.alpha;
    }
};

}  // namespace

struct osi_resnet50 {
    int B, H, W, F, O, logit_bias;
    std::vector<Tensor> tensors;
    std::vector<BN> bns;
    std::vector<Conv> convs;
    std::vector<Block> blocks;
    size_t param_floats = 0, buffer_floats = 0, ws_floats = 0;
    // head tensors
    int t_fc_w, t_fc_b, t_lg_w, t_lg_b;
    // stem
    int Hs, Ws, Hp, Wp;              // stem conv output, maxpool output
    size_t x4, wpack, gpack, a_pool, pool_idx, pooled, feat;
    size_t bn_ws, bn_ws2, bn_ws_bytes, wg_ws, wg_ws_bytes, dg_ws, dg_ws_bytes;   // bn_ws2: BatchNorm scratch of the side-stream branch
    size_t stem_ws = 0, stem_ws_bytes = 0;
    size_t wino_ws = 0, wino_ws_bytes = 0;   // transformed weights of the Winograd forms (main stream only: forward conv2, in-block input gradients)
    static constexpr int NSCR = 12;   // scratch activations-gradient buffers (each = largest activation)
    size_t scratch[NSCR], scratch_floats;
    size_t dfeat, dpooled;
    int Hf, Wf;                      // final spatial size
    // stage bookkeeping
    int n_stages = 4;
    size_t stage_lo[4], stage_hi[4];
    // (everything above is the layout osi_resnet50_create builds and nothing changes afterwards)

    // ---- run state: what one forward leaves for its backward, and one backward stage for the next --------------------------------------
    bool fwd_done = false;           // a differentiable forward ran and its backward has not finished
    bool any_fwd = false;            // the workspace holds the ReLU / arg-max decisions of a forward (osi_resnet50_debug_gate refuses to read an
                                     // empty workspace — or one an inference forward ran in: that one stores activations, not pre-BN tensors or bitmasks)
    bool frozen = false;             // osi_resnet50_forward_frozen ran last: every BatchNorm's mean / invstd slots hold the running statistics and
                                     // the backward that follows takes the frozen dataflow (dy = scale * g; the fused stem tail and the Winograd
                                     // input gradients are training-only)
    int fw_prefix = 0;               // eval_prefix of the latest differentiable forward: the gates of those units do not exist
    bool ran_fwd = false;            // a forward of any kind has run: the block inputs exist (osi_resnet50_debug_unit_input)
    const int* mix_partner = nullptr;    // osi_resnet50_set_mix: the one-shot request of the next differentiable forward (device arrays of
    const float* mix_weight = nullptr;   // B entries); that forward mixes the rows of the first trainable unit's input and clears it
    const float* x4_cur = nullptr;   // input of the step in flight (forward sets it, the stem weight gradient reads it)
    int next_stage = 0;
    BwRequest rq;                    // request of the backward in flight, fixed by the call that runs stage 0 (block 0's dgrad form depends on it)
    int cur_grad = -1;               // scratch index holding the upstream gradient between stages
    bool go_fused = false;           // cur_grad is already ReLU-masked and its BatchNorm reductions wait in dg_ws
    int fused_P = 0;                 // row tiles of the partials in dg_ws
    int stem_stats_P = 0;            // row tiles of bn1's backward partial sums in dg_ws (left by the pool-mode epilogue of layer1.0.conv1's dgrad)
    std::vector<int> free_list;      // scratch buffers nobody holds, oldest release first
    // --------------------------------------------------------------------------------------------------------------------------------------
    // optional HIP-event instrumentation: one event after every op, tagged with the op's class
    bool prof_on = false;
    bool prof_timeline = false;      // mode 2: keep the side-stream overlap, record where each op ran (osi_resnet50_timeline_read)
    std::vector<int> prof_side;      // per event: 1 = recorded on the side stream
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_cls;
    int prof_n = 0;
    int mark(int cls, hipStream_t st) {
        if (!prof_on) return OSI_OK;
        if (prof_n == (int)prof_ev.size()) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return OSI_ERR_LAUNCH;
            prof_ev.push_back(e); prof_cls.push_back(0); prof_side.push_back(0);
        }
        prof_cls[prof_n] = cls;
        prof_side[prof_n] = (side != nullptr && st == side) ? 1 : 0;
        if (hipEventRecord(prof_ev[prof_n], st) != hipSuccess) return OSI_ERR_LAUNCH;
        ++prof_n;
        return OSI_OK;
    }

    // Fine-tuning units (osi_resnet50_set_trainable). unit_mask: bit u = unit u has a trainable parameter; the units below the lowest set
    // bit (the cut) are the frozen prefix. A backward that owes nobody an image gradient stops at the cut, and a frozen unit gets no
    // weight gradient in any backward. eval_prefix: that many leading units run the inference forms in a differentiable forward.
    // The setting cannot change between a differentiable forward and the end of its backward, so the backward reads it as it stands.
    static constexpr int NUNITS = 18;
    int cur_unit = 0;                // unit of the tensors being registered (osi_resnet50_create)
    unsigned unit_mask = (1u << NUNITS) - 1;
    int eval_prefix = 0;
    float bn_momentum = 0.1f;        // running-statistics update factor of a training-mode forward (osi_resnet50_set_bn_momentum)
    bool trainable(int unit) const { return (unit_mask >> unit) & 1u; }
    int cut() const { int c = 0; while (!((unit_mask >> c) & 1u)) ++c; return c; }
    // first unit the backward in flight computes: the cut, unless the image gradient is wanted (then full depth)
    int bw_stop() const { return (rq.param_grads && !rq.dimage && !rq.x_adv) ? cut() : 0; }

    size_t add_tensor(const std::string& name, int ndim, const int* shape) {
        Tensor t; t.name = name; t.ndim = ndim; t.numel = 1;
        for (int i = 0; i < 4; ++i) t.shape[i] = i < ndim ? shape[i] : 1;
        for (int i = 0; i < ndim; ++i) t.numel *= (size_t)shape[i];
        t.off = param_floats;
        t.unit = cur_unit;
        param_floats = up(param_floats + t.numel, 4);
        tensors.push_back(t);
        return t.off;
    }
    size_t ws_alloc(size_t floats) {
        size_t o = ws_floats;
        ws_floats = up(ws_floats + floats, ALIGN_F);
        return o;
    }
    int add_conv_bn(const std::string& cname, const std::string& bname, int Bn, int Hin, int Win, int Cin, int Cout, int k, int s,
                    int pad, bool keep_act) {
        Conv c{};
        c.d.B = Bn; c.d.H = Hin; c.d.W = Win; c.d.Cin = Cin; c.d.Cout = Cout; c.d.R = k; c.d.S = k; c.d.stride = s; c.d.pad = pad;
        c.d.Ho = (Hin + 2 * pad - k) / s + 1; c.d.Wo = (Win + 2 * pad - k) / s + 1;
        int shp[4] = {Cout, Cin == 4 && k == 7 ? 3 : Cin, k, k};
        c.w_off = add_tensor(cname + ".weight", 4, shp);
        BN b; b.prefix = bname; b.C = Cout; b.M = Bn * c.d.Ho * c.d.Wo;
        int s1[1] = {Cout};
        b.g_off = add_tensor(bname + ".weight", 1, s1);
        b.b_off = add_tensor(bname + ".bias", 1, s1);
        b.rm_off = buffer_floats; buffer_floats += up(Cout, 4);
        b.rv_off = buffer_floats; buffer_floats += up(Cout, 4);
        b.mean = ws_alloc(Cout); b.invstd = ws_alloc(Cout); b.scale = ws_alloc(Cout); b.shift = ws_alloc(Cout);
        b.unit = c.unit = cur_unit;
        c.bn = (int)bns.size();
        bns.push_back(b);
        size_t n = (size_t)b.M * Cout;
        c.y = ws_alloc(n);
        c.a = keep_act ? ws_alloc(n) : WS_NONE;
        c.mask = keep_act ? ws_alloc(osi_bn_relu_mask_bytes(b.M, Cout) / sizeof(float)) : WS_NONE;
        convs.push_back(c);
        return (int)convs.size() - 1;
    }
    // Weight gradients run on a low-priority side stream: they are off the critical path of backward (nothing downstream
    // reads them before the optimizer) and fill the matrix pipes while the main stream is in HBM-bound BatchNorm kernels
    // or in the ragged last round of a dgrad launch. buf_ev[i] = last side-stream reader of scratch buffer i.
    void* staged_ws = nullptr;   // workspace whose input buffer was filled by osi_resnet50_stage_input_u8 (consumed by one forward)
    bool overlap = true;
    bool fwd_fork = true;            // projection shortcut of the forward pass on the side stream
    bool side_prio_normal = false;   // side stream at default instead of lowest priority (read when the stream is created)
    const float* x4_ext = nullptr;   // external NHWC4 input bound by osi_resnet50_bind_input_nhwc4 (consumed by one forward)
    // does the backward in flight write the parameter gradients of `unit`? (input-only request, frozen unit: nobody reads that slice of the arena)
    bool wants_grads(int unit) const { return rq.param_grads && trainable(unit); }
    // where a BatchNorm backward writes dgamma / dbeta (reductions the batch-statistics dx needs but nobody reads land in the layer's sink)
    float* dgam(float* grads, float* ws, const BN& b) const { return wants_grads(b.unit) ? grads + b.g_off : ws + b.dsink; }
    float* dbet(float* grads, float* ws, const BN& b) const { return wants_grads(b.unit) ? grads + b.b_off : ws + b.dsink + b.C; }
    // column `col` of the [P row tiles][C] partial sums a dgrad epilogue left in dg_ws: 0 = sum g (shared by both consumers),
    // 1 = sum g * xhat of the main branch, 2 = of the downsample branch
    const float* dg_col(const float* ws, int col, int P, int C) const { return ws + dg_ws + (size_t)col * P * C; }
    // The stem tail's form, decided by what the backward can observe. Block 0's last input gradient and the tail both ask here, so they
    // cannot disagree: the fused form (bn1's reductions out of that input gradient's pool-mode epilogue, dY built inside
    // osi_stem_wgrad_fused's loader) unless dJ/dimage (or the adversarial batch made from it) needs dY in memory or the geometry /
    // knobs leave the fused form no workspace.
    bool stem_tail_fused() const { return !frozen && !rq.dimage && !rq.x_adv && stem_ws_bytes > 0; }
    bool eval_fused = true;          // option "eval_fused": a forward with training = 0 runs the inference forms (block_fwd_eval); 0 = the
                                     // training topology on running statistics (A/B: the same bits when both run the same launch plans,
                                     // i.e. tail_split off; fp32-rounding-level differences otherwise)
    bool stage_join = true;          // option "stage_join": a staged backward call (stage_hi < stages) ends by joining the side stream into
                                     // the caller's stream. 0 (data parallel): only the LAST stage joins; the caller hands each finished
                                     // stage to its communication stream with osi_resnet50_grads_ready, and the compute stream runs on
    OsiTuning plan_knobs;            // the process-wide knobs the workspace was sized for (osi_resnet50_create); a launch under other
    int plan_hw_cus = 0;             // values (or on a device with another CU count) is refused (OSI_ERR_STATE) instead of running a
                                     // plan the workspace does not fit
    bool plan_unchanged() const {      // the rows of OSI_TUNING_KNOBS flagged plan-relevant, and the CU count
        const OsiTuning &a = plan_knobs, &b = g_osi_tuning;
        bool same = plan_hw_cus == device_cus();
#define OSI_KNOB_SAME(name, def, lo, hi, plan) same = same && (!(plan) || a.name == b.name);
        OSI_TUNING_KNOBS(OSI_KNOB_SAME)
#undef OSI_KNOB_SAME
        return same;
    }
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_rmain = nullptr, ev_rside = nullptr, ev_wt = nullptr;
    bool wt_pending = false;         // the Winograd weight transforms of this forward run on the side stream: the first consumer waits for ev_wt
    hipEvent_t buf_ev[NSCR] = {};
    bool buf_pending[NSCR] = {};
    bool side_dirty = false;
    int ensure_side() {
        if (side) return OSI_OK;
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return OSI_ERR_LAUNCH;
        const int prio = side_prio_normal ? 0 : lo;   // option "side_priority_normal": default priority for the side stream (A/B)
        if (hipStreamCreateWithPriority(&side, hipStreamNonBlocking, prio) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipEventCreateWithFlags(&ev_fork, EV_FLAGS) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipEventCreateWithFlags(&ev_join, EV_FLAGS) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipEventCreateWithFlags(&ev_wt, EV_FLAGS) != hipSuccess) return OSI_ERR_LAUNCH;
        for (int i = 0; i < NSCR; ++i)
            if (hipEventCreateWithFlags(&buf_ev[i], EV_FLAGS) != hipSuccess) return OSI_ERR_LAUNCH;
        return OSI_OK;
    }
    // the side stream is wanted (the class-attributing profile serialises everything on the caller's stream; the timeline mode does not)
    bool wants_side() const { return overlap && (!prof_on || prof_timeline); }
    bool async_wgrad() const { return wants_side() && side != nullptr; }
    // *idx = a free scratch buffer; it may only be rewritten on `st` after its last side-stream reader has finished
    int take(hipStream_t st, int* idx) {
        if (free_list.empty()) return OSI_ERR_STATE;
        // FIFO: hand out the buffer that was released longest ago, so its side-stream reader has most likely finished
        int i = free_list.front(); free_list.erase(free_list.begin());
        if (buf_pending[i]) {
            if (hipStreamWaitEvent(st, buf_ev[i], 0) != hipSuccess) return OSI_ERR_LAUNCH;
            buf_pending[i] = false;
        }
        *idx = i;
        return OSI_OK;
    }
    void give(int i) { free_list.push_back(i); }
    // the side stream continues from everything enqueued on `st` so far
    int fork_side(hipStream_t st) {
        if (hipEventRecord(ev_fork, st) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipStreamWaitEvent(side, ev_fork, 0) != hipSuccess) return OSI_ERR_LAUNCH;
        return OSI_OK;
    }
    // the first consumer of the Winograd-transformed weights on `st` waits for the side stream's transforms
    int wait_weight_transforms(hipStream_t st) {
        if (!wt_pending) return OSI_OK;
        if (hipStreamWaitEvent(st, ev_wt, 0) != hipSuccess) return OSI_ERR_LAUNCH;
        wt_pending = false;
        return OSI_OK;
    }
    int join_side(hipStream_t st) {
        if (!side_dirty) return OSI_OK;
        if (hipEventRecord(ev_join, side) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipStreamWaitEvent(st, ev_join, 0) != hipSuccess) return OSI_ERR_LAUNCH;
        for (int i = 0; i < NSCR; ++i) buf_pending[i] = false;
        side_dirty = false;
        return OSI_OK;
    }
    ~osi_resnet50() {
        for (hipEvent_t e : prof_ev) (void)hipEventDestroy(e);
        if (side) {
            (void)hipStreamSynchronize(side);
            (void)hipEventDestroy(ev_fork); (void)hipEventDestroy(ev_join); (void)hipEventDestroy(ev_wt);
            for (int i = 0; i < NSCR; ++i) (void)hipEventDestroy(buf_ev[i]);
            (void)hipStreamDestroy(side);
        }
        if (ev_rmain) (void)hipEventDestroy(ev_rmain);
        if (ev_rside) (void)hipEventDestroy(ev_rside);
    }
};

extern "C" {

int osi_resnet50_create(osi_resnet50_t* out, int B, int H, int W, int fc_dim, int out_features, int logit_bias) {
    OSI_REQUIRE(out && B > 0 && H >= 32 && W >= 32 && fc_dim > 0 && out_features > 0);
    osi_resnet50* n = new osi_resnet50();
    n->B = B; n->H = H; n->W = W; n->F = fc_dim; n->O = out_features; n->logit_bias = logit_bias ? 1 : 0;
    const std::string rb = "resnet_base.";
    // stem
    n->x4 = n->ws_alloc((size_t)B * H * W * 4);
    n->wpack = n->ws_alloc(64 * 224);
    n->gpack = n->ws_alloc(64 * 224);
    n->cur_unit = 0;
    int stem = n->add_conv_bn(rb + "conv1", rb + "bn1", B, H, W, 4, 64, 7, 2, 3, false);   // its activation only exists max-pooled
    n->Hs = n->convs[stem].d.Ho; n->Ws = n->convs[stem].d.Wo;
    n->Hp = (n->Hs + 2 - 3) / 2 + 1; n->Wp = (n->Ws + 2 - 3) / 2 + 1;
    n->a_pool = n->ws_alloc((size_t)B * n->Hp * n->Wp * 64);
    n->pool_idx = n->ws_alloc((size_t)B * n->Hp * n->Wp * 64 / 4);
    // stages
    const int planes[4] = {64, 128, 256, 512}, nblk[4] = {3, 4, 6, 3}, strides[4] = {1, 2, 2, 2};
    int inpl = 64, h = n->Hp, w = n->Wp;
    size_t x = n->a_pool;
    for (int s = 0; s < 4; ++s) {
        size_t lo = n->param_floats;
        for (int b = 0; b < nblk[s]; ++b) {
            const std::string pre = rb + "layer" + std::to_string(s + 1) + "." + std::to_string(b) + ".";
            const int st = b == 0 ? strides[s] : 1;
            Block blk{};
            n->cur_unit = (int)n->blocks.size() + 1;
            blk.x_in = x; blk.stage = 3 - s;
            // conv1 / conv2: only the pre-BN output is kept (their activation is recomputed in the consumers' loaders)
            blk.c1 = n->add_conv_bn(pre + "conv1", pre + "bn1", B, h, w, inpl, planes[s], 1, 1, 0, false);
            blk.c2 = n->add_conv_bn(pre + "conv2", pre + "bn2", B, h, w, planes[s], planes[s], 3, st, 1, false);
            const int ho = n->convs[blk.c2].d.Ho, wo = n->convs[blk.c2].d.Wo;
            blk.c3 = n->add_conv_bn(pre + "conv3", pre + "bn3", B, ho, wo, planes[s], planes[s] * 4, 1, 1, 0, true);
            blk.ds = -1;
            if (b == 0) blk.ds = n->add_conv_bn(pre + "downsample.0", pre + "downsample.1", B, h, w, inpl, planes[s] * 4, 1, st, 0, false);
            blk.out = n->convs[blk.c3].a;
            n->blocks.push_back(blk);
            x = blk.out; inpl = planes[s] * 4; h = ho; w = wo;
        }
        n->stage_lo[3 - s] = lo; n->stage_hi[3 - s] = n->param_floats;
    }
    n->stage_lo[3] = 0;  // the stem belongs to the last backward stage
    n->Hf = h; n->Wf = w;
    // head
    n->cur_unit = osi_resnet50::NUNITS - 1;
    { int shp[2] = {fc_dim, 2048}; n->t_fc_w = (int)n->tensors.size(); n->add_tensor(rb + "fc.weight", 2, shp); }
    { int shp[1] = {fc_dim}; n->t_fc_b = (int)n->tensors.size(); n->add_tensor(rb + "fc.bias", 1, shp); }
    { int shp[2] = {out_features, fc_dim}; n->t_lg_w = (int)n->tensors.size(); n->add_tensor("logits.weight", 2, shp); }
    n->t_lg_b = -1;
    if (n->logit_bias) { int shp[1] = {out_features}; n->t_lg_b = (int)n->tensors.size(); n->add_tensor("logits.bias", 1, shp); }
    n->stage_hi[0] = n->param_floats;  // head gradients are final after stage 0 (head + layer4)
    n->pooled = n->ws_alloc((size_t)B * 2048);
    n->feat = n->ws_alloc((size_t)B * fc_dim);
    n->dfeat = n->ws_alloc((size_t)B * fc_dim);
    n->dpooled = n->ws_alloc((size_t)B * 2048);
    // scratch sizing
    size_t maxact = 0, bnws = 0, wgws = 0, dgws = 0, winows = 0;
    for (auto& c : n->convs) {
        grow(maxact, (size_t)c.d.B * c.d.Ho * c.d.Wo * c.d.Cout);
        grow(maxact, (size_t)c.d.B * c.d.H * c.d.W * c.d.Cin);
        grow(bnws, osi_bn_workspace(n->bns[c.bn].M, c.d.Cout));
        grow(bnws, osi_bn_backward_workspace(n->bns[c.bn].M, c.d.Cout));
        grow(bnws, osi_conv_fwd_bnstats_workspace(&c.d));
        grow(bnws, osi_bn_backward_fused2_workspace(c.d.Cout));   // a projection block's two BatchNorm backwards in one pass
        grow(wgws, osi_conv_wgrad_workspace(&c.d));
        grow(wgws, osi_stem_wgrad_direct_workspace(&c.d));
        grow(wgws, osi_conv_wgrad_wino_workspace(&c.d));
        if (!(c.d.Cin == 4 && c.d.R == 7)) grow(dgws, osi_conv_dgrad_fused_workspace(&c.d));
        if (osi_conv_wino_eligible(&c.d, 0) || osi_conv_wino_eligible(&c.d, 1)) {
            // Winograd forms: one (mean, M2) / (sum g, sum g xhat) partial per 16 tiles (+ the merge scratch behind the statistics); the
            // transformed weights of both directions live per layer (built on the side stream at the start of a forward pass)
            const size_t Pw = ((size_t)c.d.B * ((c.d.H + 1) / 2) * ((c.d.W + 1) / 2) + 15) / 16;
            if (osi_conv_wino_eligible(&c.d, 0)) c.u_fw = n->ws_alloc(osi_conv_wino_weights_bytes(&c.d) / sizeof(float));
            if (osi_conv_wino_eligible(&c.d, 1)) c.u_bw = n->ws_alloc(osi_conv_wino_weights_bytes(&c.d) / sizeof(float));
            grow(winows, osi_conv_wino_slab_bytes());
            grow(bnws, (2 * Pw + 64) * c.d.Cout * sizeof(float));
            grow(dgws, 3 * Pw * c.d.Cin * sizeof(float));
        }
    }
    n->wino_ws_bytes = winows; n->wino_ws = n->ws_alloc(winows / 4 + 4);
    n->bn_ws_bytes = bnws; n->bn_ws = n->ws_alloc(bnws / 4 + 4); n->bn_ws2 = n->ws_alloc(bnws / 4 + 4);
    n->wg_ws_bytes = wgws; n->wg_ws = n->ws_alloc(wgws / 4 + 4);
    // the fused stem weight gradient has its own slab: it may run on the main stream while the side stream still owns wg_ws
    // (0 bytes = a geometry / knob setting the fused form does not take: the executor then never calls it — see stem_tail_fused)
    n->stem_ws_bytes = osi_stem_wgrad_fused_workspace(&n->convs[0].d);
    n->stem_ws = n->stem_ws_bytes ? n->ws_alloc(n->stem_ws_bytes / 4 + 4) : n->wg_ws;
    n->plan_knobs = g_osi_tuning;
    n->plan_hw_cus = device_cus();
    n->dg_ws_bytes = dgws; n->dg_ws = n->ws_alloc(dgws / 4 + 4);
    n->scratch_floats = maxact;
    for (int i = 0; i < osi_resnet50::NSCR; ++i) n->scratch[i] = n->ws_alloc(maxact);
    for (auto& b : n->bns) b.dsink = n->ws_alloc(2 * (size_t)b.C);
    *out = n;
    return OSI_OK;
}

void osi_resnet50_destroy(osi_resnet50_t net) { delete net; }
int osi_resnet50_num_tensors(osi_resnet50_t net) { return net ? (int)net->tensors.size() : 0; }
size_t osi_resnet50_param_floats(osi_resnet50_t net) { return net ? net->param_floats : 0; }
int osi_resnet50_num_bn(osi_resnet50_t net) { return net ? (int)net->bns.size() : 0; }
size_t osi_resnet50_buffer_floats(osi_resnet50_t net) { return net ? net->buffer_floats : 0; }
size_t osi_resnet50_workspace_bytes(osi_resnet50_t net) { return net ? net->ws_floats * sizeof(float) : 0; }
int osi_resnet50_num_stages(osi_resnet50_t net) { return net ? net->n_stages : 0; }
int osi_resnet50_num_units(osi_resnet50_t net) { return net ? osi_resnet50::NUNITS : 0; }
int osi_resnet50_tensor_unit(osi_resnet50_t net, int i) { return net && i >= 0 && i < (int)net->tensors.size() ? net->tensors[i].unit : -1; }
int osi_resnet50_bn_unit(osi_resnet50_t net, int j) { return net && j >= 0 && j < (int)net->bns.size() ? net->bns[j].unit : -1; }
int osi_resnet50_set_trainable(osi_resnet50_t net, unsigned unit_mask, int eval_prefix_units) {
    OSI_REQUIRE(net && unit_mask != 0 && (unit_mask >> osi_resnet50::NUNITS) == 0 && eval_prefix_units >= 0);
    int c = 0;
    while (!((unit_mask >> c) & 1u)) ++c;
    OSI_REQUIRE(eval_prefix_units <= c);
    if (net->fwd_done) return OSI_ERR_STATE;   // a backward is owed to the forward that ran under the current setting
    net->unit_mask = unit_mask;
    net->eval_prefix = eval_prefix_units;
    return OSI_OK;
}
int osi_resnet50_get_trainable(osi_resnet50_t net, unsigned* unit_mask, int* eval_prefix_units) {
    OSI_REQUIRE(net && unit_mask && eval_prefix_units);
    *unit_mask = net->unit_mask;
    *eval_prefix_units = net->eval_prefix;
    return OSI_OK;
}
int osi_resnet50_set_bn_momentum(osi_resnet50_t net, float momentum) {
    OSI_REQUIRE(net && momentum > 0.0f && momentum <= 1.0f);   // a NaN fails both comparisons
    net->bn_momentum = momentum;
    return OSI_OK;
}
int osi_resnet50_set_mix(osi_resnet50_t net, const int* partner, const float* weight) {
    OSI_REQUIRE(net && (partner == nullptr) == (weight == nullptr));
    net->mix_partner = partner; net->mix_weight = weight;
    return OSI_OK;
}
int osi_resnet50_get_bn_momentum(osi_resnet50_t net, float* momentum) {
    OSI_REQUIRE(net && momentum);
    *momentum = net->bn_momentum;
    return OSI_OK;
}
int osi_resnet50_geometry(osi_resnet50_t net, int* B, int* H, int* W) {
    OSI_REQUIRE(net);
    if (B) *B = net->B;
    if (H) *H = net->H;
    if (W) *W = net->W;
    return OSI_OK;
}

int osi_resnet50_tensor_info(osi_resnet50_t net, int i, char* name, int name_cap, int* ndim, int* shape, size_t* offset,
                             size_t* numel) {
    OSI_REQUIRE(net && i >= 0 && i < (int)net->tensors.size());
    const Tensor& t = net->tensors[i];
    if (name && name_cap > 0) { std::strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (ndim) *ndim = t.ndim;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = t.shape[k];
    if (offset) *offset = t.off;
    if (numel) *numel = t.numel;
    return OSI_OK;
}
int osi_resnet50_bn_info(osi_resnet50_t net, int j, char* prefix, int cap, int* C, size_t* rm_offset, size_t* rv_offset) {
    OSI_REQUIRE(net && j >= 0 && j < (int)net->bns.size());
    const BN& b = net->bns[j];
    if (prefix && cap > 0) { std::strncpy(prefix, b.prefix.c_str(), cap - 1); prefix[cap - 1] = 0; }
    if (C) *C = b.C;
    if (rm_offset) *rm_offset = b.rm_off;
    if (rv_offset) *rv_offset = b.rv_off;
    return OSI_OK;
}
int osi_resnet50_stage_grad_range(osi_resnet50_t net, int s, size_t* lo, size_t* hi) {
    OSI_REQUIRE(net && s >= 0 && s < net->n_stages && lo && hi);
    *lo = net->stage_lo[s]; *hi = net->stage_hi[s];
    return OSI_OK;
}

int osi_resnet50_profile(osi_resnet50_t n, int enable) {
    OSI_REQUIRE(n);
    n->prof_on = enable != 0;
    n->prof_timeline = enable == 2;
    n->prof_n = 0;
    return OSI_OK;
}
// Timeline mode (osi_resnet50_profile(net, 2)): the overlapped schedule is kept and every op's completion event carries the stream
// it ran on. Host-synchronising read-out: t_ms[i] = completion time of op i relative to the first recorded event.
int osi_resnet50_timeline_read(osi_resnet50_t n, double* t_ms, int* cls, int* on_side, int cap, int* count) {
    OSI_REQUIRE(n && t_ms && cls && on_side && count && cap > 0);
    *count = 0;
    if (n->prof_n == 0) return OSI_OK;
    for (int i = 0; i < n->prof_n; ++i)
        if (hipEventSynchronize(n->prof_ev[i]) != hipSuccess) return OSI_ERR_LAUNCH;
    const int m = n->prof_n < cap ? n->prof_n : cap;
    for (int i = 0; i < m; ++i) {
        float t = 0.f;
        if (i > 0 && hipEventElapsedTime(&t, n->prof_ev[0], n->prof_ev[i]) != hipSuccess) return OSI_ERR_LAUNCH;
        t_ms[i] = t; cls[i] = n->prof_cls[i]; on_side[i] = n->prof_side[i];
    }
    *count = m;
    n->prof_n = 0;
    return OSI_OK;
}
// Host-synchronising read-out (not a launch function): per-class elapsed milliseconds and op counts since enable/last read.
int osi_resnet50_profile_read(osi_resnet50_t n, double* ms, int* count) {
    OSI_REQUIRE(n && ms && count);
    for (int k = 0; k < OSI_PROF_NCLASS; ++k) { ms[k] = 0; count[k] = 0; }
    if (n->prof_n == 0) return OSI_OK;
    if (hipEventSynchronize(n->prof_ev[n->prof_n - 1]) != hipSuccess) return OSI_ERR_LAUNCH;
    for (int i = 1; i < n->prof_n; ++i) {
        int c = n->prof_cls[i];
        if (c == OSI_PROF_START) continue;  // gap between two executor calls (loss kernel, host work): not attributed
        float t = 0.f;
        if (hipEventElapsedTime(&t, n->prof_ev[i - 1], n->prof_ev[i]) != hipSuccess) return OSI_ERR_LAUNCH;
        ms[c] += t; count[c] += 1;
    }
    n->prof_n = 0;
    return OSI_OK;
}

// How a forward finishes its BatchNorms: on the running statistics without backward state (validate()), on batch statistics with the
// running-statistics update (training), or on the running statistics with the backward state kept (osi_resnet50_forward_frozen).
enum class BnMode { Inference, Batch, Frozen };

// conv ci + its BatchNorm coefficients. in_bn >= 0: the conv's input is the PRE-BN output of the layer whose BatchNorm is `in_bn`;
// that BatchNorm + ReLU is applied inside the conv's operand loader (osi_conv_fwd_act) — the activation never exists in HBM.
static int conv_bn_fwd(osi_resnet50* n, int ci, const float* params, float* buffers, float* ws, const float* x, const float* w,
                       BnMode mode, hipStream_t st, size_t bn_ws_off, int in_bn = -1) {
    Conv& c = n->convs[ci];
    BN& b = n->bns[c.bn];
    const float* isc = in_bn >= 0 ? ws + n->bns[in_bn].scale : nullptr;
    const float* ish = in_bn >= 0 ? ws + n->bns[in_bn].shift : nullptr;
    // 3x3 / stride 1 (conv2 of a bottleneck without a stride): Winograd F(2x2,3x3), 2.25x fewer multiplies (csrc/conv_wino.hip); main stream only
    const bool wino = n->plan_knobs.fwd_wino && isc && (n->side == nullptr || st != n->side) && c.u_fw != WS_NONE;
    if (wino) OSI_TRY(n->wait_weight_transforms(st));
    // batch statistics come out of the conv epilogue (per row tile), only a tiny per-channel merge follows; the other modes pass no slab
    const bool stats = mode == BnMode::Batch;
    float* sws = stats ? ws + bn_ws_off : nullptr;
    const size_t sbytes = stats ? n->bn_ws_bytes : 0;
    int P = 0, rows = 0;
    int *pP = stats ? &P : nullptr, *prows = stats ? &rows : nullptr;
    if (wino) OSI_TRY(osi_conv_fwd_wino_pre(&c.d, x, isc, ish, ws + c.u_fw, ws + c.y, ws + n->wino_ws, n->wino_ws_bytes, sws, sbytes, pP, prows, st));
    else if (isc) OSI_TRY(osi_conv_fwd_act(&c.d, x, isc, ish, w, ws + c.y, OSI_TILE_AUTO, sws, sbytes, pP, prows, st));
    else if (stats) OSI_TRY(osi_conv_fwd_bnstats(&c.d, x, w, ws + c.y, OSI_TILE_AUTO, sws, sbytes, pP, prows, st));
    else OSI_TRY(osi_conv_fwd(&c.d, x, w, ws + c.y, OSI_TILE_AUTO, st));
    OSI_TRY(n->mark(OSI_PROF_CONV_FWD, st));
    if (mode == BnMode::Batch)
        OSI_TRY(osi_bn_finalize_stats(sws, sbytes, P, rows, b.M, b.C, params + b.g_off, params + b.b_off, 1e-5f, n->bn_momentum, buffers + b.rm_off,
                                      buffers + b.rv_off, ws + b.mean, ws + b.invstd, ws + b.scale, ws + b.shift, st));
    else if (mode == BnMode::Inference)   // (frozen: one launch wrote every layer's coefficients up front)
        OSI_TRY(osi_bn_eval_coeffs(buffers + b.rm_off, buffers + b.rv_off, params + b.g_off, params + b.b_off, 1e-5f, b.C, ws + b.scale,
                                   ws + b.shift, st));
    return n->mark(OSI_PROF_BN_FWD, st);
}

// Input staged from a uint8 [B][H][W][3] batch (+ optional per-image horizontal flip flags) straight into the executor's NHWC4
// input buffer; the following osi_resnet50_forward call passes image = NULL.
int osi_resnet50_stage_input_u8(osi_resnet50_t n, const unsigned char* images_u8_nhwc, const unsigned char* flip, void* workspace,
                                osi_stream_t stream) {
    OSI_REQUIRE(n && images_u8_nhwc && workspace);
    OSI_TRY(osi_u8hwc3_to_nhwc4(images_u8_nhwc, flip, (float*)workspace + n->x4, n->B, n->H, n->W, stream));
    n->staged_ws = workspace;
    return OSI_OK;
}

int osi_resnet50_bind_input_nhwc4(osi_resnet50_t n, const float* x_nhwc4) {
    OSI_REQUIRE(n && x_nhwc4 && ((size_t)x_nhwc4 & 15) == 0);
    n->x4_ext = x_nhwc4;
    return OSI_OK;
}

// avgpool -> fc -> logits; the logits are written to the caller's tensor, the features are copied there
static int head_fwd(osi_resnet50* n, const float* params, float* ws, float* logits, float* features, hipStream_t st) {
    const float* last = ws + n->blocks.back().out;
    OSI_TRY(osi_avgpool_fwd(last, ws + n->pooled, n->B, n->Hf * n->Wf, 2048, st));
    const Tensor& fw = n->tensors[n->t_fc_w]; const Tensor& fb = n->tensors[n->t_fc_b]; const Tensor& lw = n->tensors[n->t_lg_w];
    OSI_TRY(osi_linear_fwd(ws + n->pooled, params + fw.off, params + fb.off, ws + n->feat, n->B, 2048, n->F, st));
    const float* lb = n->t_lg_b >= 0 ? params + n->tensors[n->t_lg_b].off : nullptr;
    // the logits have no later reader in the workspace: straight into the caller's tensor (the features are read by the head's backward)
    OSI_TRY(osi_linear_fwd(ws + n->feat, params + lw.off, lb, logits, n->B, n->F, n->O, st));
    if (hipMemcpyAsync(features, ws + n->feat, (size_t)n->B * n->F * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return OSI_ERR_LAUNCH;
    return OSI_OK;
}

// Inference forward (training == 0; validate() / get_arrays(), reference train.py:142-234: model.eval() under no_grad). In eval mode
// every BatchNorm's scale / shift exist before its convolution is launched, so nothing of the training topology's bookkeeping is
// needed: ONE launch computes the coefficients of all 53 BatchNorms, and every convolution applies its own BatchNorm in its epilogue —
// conv1 / conv2 write relu(bn(conv)), the projection shortcut writes bn(conv), conv3 writes the block output relu(bn3(conv3) + shortcut)
// (osi_conv_fwd_epilogue / osi_conv_fwd_wino_epilogue_pre). No pre-BN tensor, no block-output pass, no ReLU bitmask, no fused-loader
// activation on the consumer side (every consumer reads a finished activation with its plain loader): 53 + 16 + 53 launches fewer, the 16
// HBM-bound block-output passes and the loader-side activation arithmetic gone. Values: the same fmas on the same accumulators as the
// training topology on running statistics (option eval_fused = 0) — bit-identical outputs when both run the same launch plans
// (tail_split off); where the plans differ, the two differ at fp32-rounding level.
// Buffers: conv1 / conv2 / shortcut activations live where the training forward keeps those layers' pre-BN tensors, the block outputs
// where it keeps them; the workspace then holds no backward state (fwd_done and any_fwd are cleared).
// The pieces of the inference forward, shared with the frozen prefix of a differentiable forward (osi_resnet50_set_trainable,
// eval_prefix_units > 0). Coefficients of the BatchNorms of units [0, units) from ONE launch:
static int eval_coeffs(osi_resnet50* n, const float* params, const float* buffers, float* ws, int units, hipStream_t st) {
    osi_bn_eval_layer tab[OSI_BN_MULTI_MAX];
    int nb = 0;
    for (const BN& b : n->bns) {
        if (b.unit >= units) continue;
        if (nb == OSI_BN_MULTI_MAX) return OSI_ERR_STATE;
        tab[nb++] = osi_bn_eval_layer{buffers + b.rm_off, buffers + b.rv_off, params + b.g_off, params + b.b_off, ws + b.scale, ws + b.shift, b.C};
    }
    OSI_TRY(osi_bn_eval_coeffs_multi(tab, nb, 1e-5f, st));
    return n->mark(OSI_PROF_BN_FWD, st);
}
// The same for the frozen forward: scale / shift (forward) and mean / invstd (backward) of the BatchNorms of units [from, NUNITS)
static int frozen_coeffs(osi_resnet50* n, const float* params, const float* buffers, float* ws, int from, hipStream_t st) {
    osi_bn_frozen_layer tab[OSI_BN_FROZEN_MAX];
    int nb = 0;
    for (const BN& b : n->bns) {
        if (b.unit < from) continue;
        if (nb == OSI_BN_FROZEN_MAX) return OSI_ERR_STATE;
        tab[nb++] = osi_bn_frozen_layer{buffers + b.rm_off, buffers + b.rv_off, params + b.g_off, params + b.b_off, ws + b.scale, ws + b.shift,
                                        ws + b.mean, ws + b.invstd, b.C};
    }
    if (!nb) return OSI_OK;
    OSI_TRY(osi_bn_frozen_coeffs_multi(tab, nb, 1e-5f, st));
    return n->mark(OSI_PROF_BN_FWD, st);
}

// Winograd weight transforms of every 3x3 stride-1 layer, both directions: the weights are the same for this forward and its backward.
// On the side stream beside the stem (26 launches of 4 - 16 us that used to sit in front of their convolutions); the first Winograd
// convolution waits for them. `p`: units below it run the inference forms and no backward ever reaches them.
static int transform_weights(osi_resnet50* n, const float* params, float* ws, BnMode mode, int p, hipStream_t st) {
    const bool bw = mode == BnMode::Batch && n->plan_knobs.dgrad_wino;   // (a frozen backward has no Winograd input gradient)
    if (!n->plan_knobs.fwd_wino && !bw) return OSI_OK;
    // (training forwards only: an inference forward has 13 transforms and nothing but the stem beside them — the fork / join costs more
    // than they do: 7.96 in line vs 8.00 ms aside per batch of 128, profiles/NOTES_r06.md)
    const bool aside = mode == BnMode::Batch && n->async_wgrad();
    hipStream_t wt = aside ? n->side : st;
    if (aside) OSI_TRY(n->fork_side(st));
    for (auto& c : n->convs)
        if (n->plan_knobs.fwd_wino && c.u_fw != WS_NONE)
            OSI_TRY(osi_conv_wino_transform_weights(&c.d, params + c.w_off, 0, ws + c.u_fw, osi_conv_wino_weights_bytes(&c.d), wt));
    OSI_TRY(n->mark(OSI_PROF_CONV_FWD, wt));
    if (bw) {
        int nt = 0;
        for (auto& c : n->convs)
            if (c.u_bw != WS_NONE && c.unit >= p) {
                OSI_TRY(osi_conv_wino_transform_weights(&c.d, params + c.w_off, 1, ws + c.u_bw, osi_conv_wino_weights_bytes(&c.d), wt));
                ++nt;
            }
        if (nt) OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, wt));
    }
    if (aside) {
        if (hipEventRecord(n->ev_wt, n->side) != hipSuccess) return OSI_ERR_LAUNCH;
        n->wt_pending = true;
    }
    return OSI_OK;
}

// conv1 + bn1 + relu + maxpool in one pass: the 112x112x64 post-ReLU tensor is never materialised. inference_form: bn1's coefficients
// already exist (eval_coeffs), so the plain convolution is all that precedes the pass; otherwise `mode` finishes bn1 after the convolution.
static int stem_fwd(osi_resnet50* n, const float* params, float* buffers, float* ws, const float* x4, BnMode mode, bool inference_form,
                    hipStream_t st) {
    Conv& c0 = n->convs[0];
    BN& b0 = n->bns[c0.bn];
    if (inference_form) {
        OSI_TRY(osi_conv_fwd(&c0.d, x4, ws + n->wpack, ws + c0.y, OSI_TILE_AUTO, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_FWD, st));
    } else {
        OSI_TRY(conv_bn_fwd(n, 0, params, buffers, ws, x4, ws + n->wpack, mode, st, n->bn_ws));
    }
    OSI_TRY(osi_bn_relu_maxpool_fwd(ws + c0.y, ws + b0.scale, ws + b0.shift, ws + n->a_pool, ws + n->pool_idx, n->B, n->Hs, n->Ws, 64, st));
    return n->mark(OSI_PROF_BN_FWD, st);
}

// The projection shortcut of block k only depends on the block input: it runs beside the main branch where a side stream exists (own
// BatchNorm scratch). launch(stream, BatchNorm scratch offset) enqueues it; *forked: the main branch calls shortcut_wait before it reads
// the shortcut. An identity block launches nothing.
extern "C++" template <class Launch>
static int shortcut_beside(osi_resnet50* n, const Block& k, hipStream_t st, bool* forked, Launch launch) {
    *forked = k.ds >= 0 && n->fwd_fork && n->async_wgrad();
    if (k.ds < 0) return OSI_OK;
    if (*forked) OSI_TRY(n->fork_side(st));
    OSI_TRY(launch(*forked ? n->side : st, *forked ? n->bn_ws2 : n->bn_ws));
    if (*forked && hipEventRecord(n->ev_join, n->side) != hipSuccess) return OSI_ERR_LAUNCH;
    return OSI_OK;
}
static int shortcut_wait(osi_resnet50* n, bool forked, hipStream_t st) {
    return forked && hipStreamWaitEvent(st, n->ev_join, 0) != hipSuccess ? OSI_ERR_LAUNCH : OSI_OK;
}

// One bottleneck in the inference form; it leaves the finished block output where the next block reads it.
static int block_fwd_eval(osi_resnet50* n, Block& k, const float* params, float* ws, hipStream_t st) {
    const float* x = ws + k.x_in;
    Conv &c1 = n->convs[k.c1], &c2 = n->convs[k.c2], &c3 = n->convs[k.c3];
    // conv `c` with its BatchNorm (+ residual) (+ ReLU) in the epilogue
    auto conv = [&](Conv& c, const float* in, float* out, const float* res, int relu, hipStream_t s, size_t bn_ws_off) {
        const BN& b = n->bns[c.bn];
        const osi_conv_epilogue e{ws + b.scale, ws + b.shift, res, relu};
        OSI_TRY(osi_conv_fwd_epilogue(&c.d, in, params + c.w_off, out, &e, ws + bn_ws_off, n->bn_ws_bytes, s));
        return n->mark(OSI_PROF_CONV_FWD, s);
    };
    bool forked = false;
    OSI_TRY(shortcut_beside(n, k, st, &forked, [&](hipStream_t s, size_t bn_ws_off) {
        Conv& cd = n->convs[k.ds];
        return conv(cd, x, ws + cd.y, nullptr, 0, s, bn_ws_off);
    }));
    OSI_TRY(conv(c1, x, ws + c1.y, nullptr, 1, st, n->bn_ws));
    if (n->plan_knobs.fwd_wino && c2.u_fw != WS_NONE) {     // 3x3 / stride 1: Winograd F(2x2,3x3)
        const BN& b2 = n->bns[c2.bn];
        const osi_conv_epilogue e{ws + b2.scale, ws + b2.shift, nullptr, 1};
        OSI_TRY(n->wait_weight_transforms(st));
        OSI_TRY(osi_conv_fwd_wino_epilogue_pre(&c2.d, ws + c1.y, ws + c2.u_fw, ws + c2.y, &e, ws + n->wino_ws, n->wino_ws_bytes, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_FWD, st));
    } else {
        OSI_TRY(conv(c2, ws + c1.y, ws + c2.y, nullptr, 1, st, n->bn_ws));
    }
    OSI_TRY(shortcut_wait(n, forked, st));
    return conv(c3, ws + c2.y, ws + c3.a, k.ds >= 0 ? ws + n->convs[k.ds].y : x, 1, st, n->bn_ws);
}

// One bottleneck in the training topology. Only the block output (the residual sum) is materialised: conv2 / conv3 read the pre-BN output
// of the conv before them and apply its BatchNorm + ReLU in their operand loader; the projection shortcut's BatchNorm is applied inside the
// block-output kernel. 3 (4) convs + one block-output pass instead of 3 (4) convs + 3 (4) apply passes.
static int block_fwd_train(osi_resnet50* n, Block& k, const float* params, float* buffers, float* ws, BnMode mode, hipStream_t st) {
    const float* x = ws + k.x_in;
    Conv &c1 = n->convs[k.c1], &c2 = n->convs[k.c2], &c3 = n->convs[k.c3];
    bool forked = false;
    OSI_TRY(shortcut_beside(n, k, st, &forked, [&](hipStream_t s, size_t bn_ws_off) {
        return conv_bn_fwd(n, k.ds, params, buffers, ws, x, params + n->convs[k.ds].w_off, mode, s, bn_ws_off);
    }));
    OSI_TRY(conv_bn_fwd(n, k.c1, params, buffers, ws, x, params + c1.w_off, mode, st, n->bn_ws));
    OSI_TRY(conv_bn_fwd(n, k.c2, params, buffers, ws, ws + c1.y, params + c2.w_off, mode, st, n->bn_ws, c1.bn));
    OSI_TRY(conv_bn_fwd(n, k.c3, params, buffers, ws, ws + c2.y, params + c3.w_off, mode, st, n->bn_ws, c2.bn));
    OSI_TRY(shortcut_wait(n, forked, st));
    BN& b3 = n->bns[c3.bn];
    if (k.ds >= 0) {
        Conv& cd = n->convs[k.ds];
        BN& bd = n->bns[cd.bn];
        OSI_TRY(osi_bn_apply_relu_mask2(ws + c3.y, ws + b3.scale, ws + b3.shift, ws + cd.y, ws + bd.scale, ws + bd.shift, ws + c3.a,
                                        ws + c3.mask, b3.M, b3.C, st));
    } else {
        OSI_TRY(osi_bn_apply_relu_mask(ws + c3.y, x, ws + b3.scale, ws + b3.shift, ws + c3.a, ws + c3.mask, b3.M, b3.C, st));
    }
    return n->mark(OSI_PROF_BN_FWD, st);
}

static int forward_impl(osi_resnet50_t n, const float* params, float* buffers, long long* nbt, const float* image, void* workspace,
                        float* logits, float* features, BnMode mode, osi_stream_t stream) {
    if (!n->plan_unchanged()) return OSI_ERR_STATE;   // a plan-relevant knob changed after create: the workspace no longer fits the plans
    // a pending mix (osi_resnet50_set_mix) belongs to the input of the first trainable block: it needs a block cut, and nothing runs without one
    const bool mix = mode != BnMode::Inference && n->mix_partner;
    if (mix && (n->eval_prefix < 1 || n->eval_prefix > (int)n->blocks.size())) return OSI_ERR_STATE;
    // input binding
    const float* ext = n->x4_ext;
    n->x4_ext = nullptr;
    if (!image && !ext && n->staged_ws != workspace) return OSI_ERR_STATE;   // image = NULL needs a staged or bound input
    n->staged_ws = nullptr;
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    const float* x4 = (!image && ext) ? ext : ws + n->x4;
    n->x4_cur = x4;
    n->fwd_done = false;
    n->frozen = false;
    const bool differentiable = mode != BnMode::Inference;
    // units [0, p) of a differentiable forward run the inference forms on the running statistics (an inference forward ignores the setting);
    // units [0, ev) run them in this forward: all of them in an inference forward under option eval_fused
    const int p = differentiable ? n->eval_prefix : 0;
    const int ev = !differentiable && n->eval_fused ? osi_resnet50::NUNITS : p;
    if (differentiable && n->wants_side()) OSI_TRY(n->ensure_side());
    OSI_TRY(n->mark(OSI_PROF_START, st));
    OSI_TRY(transform_weights(n, params, ws, mode, p, st));
    // stem: input layout, packed weights, every coefficient set that exists up front, conv1 + bn1 + relu + maxpool
    if (image) OSI_TRY(osi_nchw3_to_nhwc4(image, ws + n->x4, n->B, n->H, n->W, st));
    OSI_TRY(osi_stem_weight_pack(params + n->convs[0].w_off, ws + n->wpack, 64, st));
    OSI_TRY(n->mark(OSI_PROF_OTHER, st));
    if (ev > 0) OSI_TRY(eval_coeffs(n, params, buffers, ws, ev, st));
    if (mode == BnMode::Frozen) OSI_TRY(frozen_coeffs(n, params, buffers, ws, p, st));
    OSI_TRY(stem_fwd(n, params, buffers, ws, x4, mode, ev > 0, st));
    // bottleneck blocks
    for (Block& k : n->blocks) {
        if (mix && n->convs[k.c1].unit == p) {   // unit p - 1 has written this tensor, nothing of unit p has read it; the shortcut's fork comes later
            const osi_conv_desc& d = n->convs[k.c1].d;
            OSI_TRY(osi_mix_rows_pairs(ws + k.x_in, n->mix_partner, n->mix_weight, n->B, (size_t)d.H * d.W * d.Cin, st));
            OSI_TRY(n->mark(OSI_PROF_OTHER, st));
        }
        if (n->convs[k.c1].unit < ev) OSI_TRY(block_fwd_eval(n, k, params, ws, st));
        else OSI_TRY(block_fwd_train(n, k, params, buffers, ws, mode, st));
    }
    OSI_TRY(head_fwd(n, params, ws, logits, features, st));
    // state. An all-inference-form forward leaves no pre-BN tensors, bitmasks or arg-max decisions of a training forward (osi_resnet50_debug_gate)
    n->any_fwd = ev < osi_resnet50::NUNITS;
    n->ran_fwd = true;
    if (mix) { n->mix_partner = nullptr; n->mix_weight = nullptr; }   // one-shot
    if (mode == BnMode::Batch) {      // the BatchNorms that ran on batch statistics: those of units >= p, the tail of the forward-ordered table
        int j0 = 0;
        while (j0 < (int)n->bns.size() && n->bns[j0].unit < p) ++j0;
        if (j0 < (int)n->bns.size()) OSI_TRY(osi_i64_add(nbt + j0, (int)n->bns.size() - j0, 1, st));
    }
    if (differentiable) {
        n->fw_prefix = p;
        n->frozen = mode == BnMode::Frozen;
        n->fwd_done = true;
        n->next_stage = 0;
    }
    return n->mark(OSI_PROF_OTHER, st);
}

int osi_resnet50_forward(osi_resnet50_t n, const float* params, float* buffers, long long* nbt, const float* image,
                         void* workspace, float* logits, float* features, int training, osi_stream_t stream) {
    OSI_REQUIRE(n && params && buffers && workspace && logits && features);
    OSI_REQUIRE(!training || nbt);
    return forward_impl(n, params, buffers, nbt, image, workspace, logits, features, training ? BnMode::Batch : BnMode::Inference, stream);
}

// The training topology on the running statistics, differentiable: `buffers` are only read (the frozen mode of forward_impl never passes them
// to a kernel that writes), num_batches_tracked is not touched, and the backward that follows runs the frozen dataflow.
int osi_resnet50_forward_frozen(osi_resnet50_t n, const float* params, const float* buffers, const float* image, void* workspace,
                                float* logits, float* features, osi_stream_t stream) {
    OSI_REQUIRE(n && params && buffers && workspace && logits && features);
    return forward_impl(n, params, const_cast<float*>(buffers), nullptr, image, workspace, logits, features, BnMode::Frozen, stream);
}

// weight gradient of conv `ci` from dy (scratch buffer index gi): on the side stream when overlap is on
// in_bn >= 0: conv_in is the PRE-BN output of the layer with BatchNorm `in_bn`; its BN + ReLU is applied in the loader
static int wgrad_launch(osi_resnet50* n, int ci, float* grads, float* ws, int gi, const float* conv_in, hipStream_t st, int in_bn,
                        bool async) {
    Conv& c = n->convs[ci];
    const float* dy = ws + n->scratch[gi];
    hipStream_t ws_st = st;
    if (async) {
        OSI_TRY(n->fork_side(st));
        ws_st = n->side;
    }
    if (ci == 0) {
        if (osi_stem_wgrad_direct_workspace(&c.d) > 0) {      // direct form: the parameter-layout gradient in one go
            OSI_TRY(osi_stem_wgrad_direct(&c.d, dy, conv_in, grads + c.w_off, ws + n->wg_ws, n->wg_ws_bytes, ws_st));
        } else {
            OSI_TRY(osi_conv_wgrad(&c.d, dy, conv_in, ws + n->gpack, ws + n->wg_ws, n->wg_ws_bytes, ws_st));
            OSI_TRY(osi_stem_grad_unpack(ws + n->gpack, grads + c.w_off, 64, ws_st));
        }
    } else if (in_bn >= 0 && n->plan_knobs.wgrad_wino && osi_conv_wgrad_wino_workspace(&c.d) > 0) {
        // 3x3 / stride 1 (conv2 of a bottleneck without a stride): Winograd F(3x3, 2x2), the sum over tiles in the transformed domain
        OSI_TRY(osi_conv_wgrad_wino(&c.d, dy, conv_in, ws + n->bns[in_bn].scale, ws + n->bns[in_bn].shift, grads + c.w_off, ws + n->wg_ws,
                                    n->wg_ws_bytes, ws_st));
    } else if (in_bn >= 0) {
        OSI_TRY(osi_conv_wgrad_act(&c.d, dy, conv_in, ws + n->bns[in_bn].scale, ws + n->bns[in_bn].shift, grads + c.w_off, ws + n->wg_ws,
                                   n->wg_ws_bytes, ws_st));
    } else {
        OSI_TRY(osi_conv_wgrad(&c.d, dy, conv_in, grads + c.w_off, ws + n->wg_ws, n->wg_ws_bytes, ws_st));
    }
    if (async) {
        if (hipEventRecord(n->buf_ev[gi], n->side) != hipSuccess) return OSI_ERR_LAUNCH;
        n->buf_pending[gi] = true;
        n->side_dirty = true;
    }
    OSI_TRY(n->mark(OSI_PROF_CONV_WGRAD, ws_st));
    return OSI_OK;
}

static int wgrad(osi_resnet50* n, int ci, float* grads, float* ws, int gi, const float* conv_in, hipStream_t st, int in_bn = -1) {
    if (!n->wants_grads(n->convs[ci].unit)) return OSI_OK;   // input-only backward, or a frozen unit: no weight gradient of any kind
    return wgrad_launch(n, ci, grads, ws, gi, conv_in, st, in_bn, n->async_wgrad());
}

// plain input gradient (no fused epilogue)
static int dgrad_plain(osi_resnet50* n, const osi_conv_desc* d, const float* dy, const float* w, float* dx, int accumulate, hipStream_t st) {
    OSI_TRY(osi_conv_dgrad(d, dy, w, dx, accumulate, OSI_TILE_AUTO, st));
    return n->mark(OSI_PROF_CONV_DGRAD, st);
}

// BatchNorm backward of conv `ci` from a RAW block-output gradient in buffer gi: gated by the stored bitmask here, dy in place, the gated
// gradient itself (it continues down the identity shortcut) into buffer `gmasked`
static int bn_bwd_raw(osi_resnet50* n, int ci, const float* params, float* grads, float* ws, int gi, int gmasked, hipStream_t st) {
    Conv& c = n->convs[ci];
    BN& b = n->bns[c.bn];
    float* g = ws + n->scratch[gi];
    OSI_TRY(osi_bn_backward_relu_mask(g, ws + c.mask, ws + c.y, ws + b.mean, ws + b.invstd, params + b.g_off, g, ws + n->scratch[gmasked],
                                      n->dgam(grads, ws, b), n->dbet(grads, ws, b), b.M, b.C, ws + n->bn_ws, n->bn_ws_bytes, st));
    return n->mark(OSI_PROF_BN_BWD, st);
}

// BatchNorm backward of conv `ci` from a gradient buffer that the producing dgrad epilogue already ReLU-masked, with the
// reductions waiting in dg_ws (column `which` = 0: main branch, 1: downsample branch). dy goes to buffer `dyi` (may equal gi).
static int bn_bwd_fused(osi_resnet50* n, int ci, const float* params, float* grads, float* ws, int gi, int dyi, int which,
                        hipStream_t st) {
    Conv& c = n->convs[ci];
    BN& b = n->bns[c.bn];
    const int P = n->fused_P;
    OSI_TRY(osi_bn_backward_fused(ws + n->scratch[gi], ws + c.y, ws + b.mean, ws + b.invstd, params + b.g_off, n->dg_col(ws, 0, P, b.C),
                                  n->dg_col(ws, 1 + which, P, b.C), P, ws + n->scratch[dyi], n->dgam(grads, ws, b), n->dbet(grads, ws, b),
                                  b.M, b.C, ws + n->bn_ws, n->bn_ws_bytes, st));
    return n->mark(OSI_PROF_BN_BWD, st);
}

// The same for the two BatchNorms of a projection block in one pass over the gated gradient in buffer gi: conv `ci` (bn3, column 0 of
// dg_ws) -> buffer dyi, conv `cj` (the shortcut, column 1) -> buffer dyj. Every result is the one of the two bn_bwd_fused calls.
static int bn_bwd_fused_pair(osi_resnet50* n, int ci, int cj, const float* params, float* grads, float* ws, int gi, int dyi, int dyj,
                             hipStream_t st) {
    osi_bn_fused_consumer cs[2];
    const int idx[2] = {ci, cj}, out[2] = {dyi, dyj};
    for (int k = 0; k < 2; ++k) {
        Conv& c = n->convs[idx[k]];
        BN& b = n->bns[c.bn];
        cs[k] = osi_bn_fused_consumer{ws + c.y, ws + b.mean, ws + b.invstd, params + b.g_off, n->dg_col(ws, 1 + k, n->fused_P, b.C),
                                      ws + n->scratch[out[k]], n->dgam(grads, ws, b), n->dbet(grads, ws, b)};
    }
    BN& b = n->bns[n->convs[ci].bn];
    OSI_TRY(osi_bn_backward_fused2(ws + n->scratch[gi], cs, n->dg_col(ws, 0, n->fused_P, b.C), n->fused_P, b.M, b.C, ws + n->bn_ws,
                                   n->bn_ws_bytes, st));
    return n->mark(OSI_PROF_BN_BWD, st);
}

// Frozen statistics. Finish the dgamma / dbeta of conv `ci`'s BatchNorm from the row-tile partials a dgrad epilogue left in dg_ws (column
// `which` as in bn_bwd_fused). Nothing is launched in an input-only backward.
static int bn_reduce_frozen(osi_resnet50* n, int ci, float* grads, float* ws, int which, hipStream_t st) {
    BN& b = n->bns[n->convs[ci].bn];
    if (!n->wants_grads(b.unit)) return OSI_OK;    // parameter-only reduction: input-only backward, or a frozen unit
    const int P = n->fused_P;
    OSI_TRY(osi_bn_backward_reduce(n->dg_col(ws, 0, P, b.C), n->dg_col(ws, 1 + which, P, b.C), P, grads + b.g_off, grads + b.b_off, b.M, b.C,
                                   ws + n->bn_ws, n->bn_ws_bytes, st));
    return n->mark(OSI_PROF_BN_BWD, st);
}
// Frozen statistics. BatchNorm backward of conv `ci` (and `cj` >= 0, the projection shortcut: same gated gradient) from buffer gi:
// dy = scale * g into buffer dyi (dyj). masked: the gradient is raw and the block-output bitmask of conv `ci` gates it here, the
// reductions run here too; otherwise they arrive through bn_reduce_frozen. gmasked >= 0: buffer that receives g (identity shortcut).
static int bn_bwd_frozen(osi_resnet50* n, int ci, int cj, float* grads, float* ws, int gi, int dyi, int dyj, int gmasked, bool masked,
                         hipStream_t st) {
    osi_bn_frozen_consumer cs[2];
    const int idx[2] = {ci, cj}, out[2] = {dyi, dyj};
    const int nc = cj >= 0 ? 2 : 1;
    for (int k = 0; k < nc; ++k) {
        Conv& c = n->convs[idx[k]];
        BN& b = n->bns[c.bn];
        const bool red = masked && n->wants_grads(b.unit);
        cs[k] = osi_bn_frozen_consumer{ws + c.y, ws + b.mean, ws + b.invstd, ws + b.scale, ws + n->scratch[out[k]],
                                       red ? grads + b.g_off : nullptr, red ? grads + b.b_off : nullptr};
    }
    Conv& c = n->convs[ci];
    BN& b = n->bns[c.bn];
    OSI_TRY(osi_bn_backward_frozen(ws + n->scratch[gi], masked ? ws + c.mask : nullptr, cs, nc, gmasked >= 0 ? ws + n->scratch[gmasked] : nullptr,
                                   b.M, b.C, ws + n->bn_ws, n->bn_ws_bytes, st));
    return n->mark(OSI_PROF_BN_BWD, st);
}
// Frozen statistics. Input gradient of conv `ci` (dy in buffer dyi) into buffer dxi, ending in the BatchNorm backward of the in-block
// producer `pc`: dxi = scale * gate * dgrad (osi_conv_dgrad_fused_frozen), the producer's dgamma / dbeta merged from the epilogue's partials.
// The partials are emitted in an input-only backward as well (and dropped): the launch plan — a K-split tail needs their workspace — and
// with it every bit of dJ/dimage stays the one of the backward with parameter gradients.
static int dgrad_frozen(osi_resnet50* n, int ci, const float* params, float* grads, float* ws, int dyi, int dxi, int pc, hipStream_t st) {
    Conv& c = n->convs[ci];
    Conv& p0 = n->convs[pc];
    BN& b0 = n->bns[p0.bn];
    osi_dgrad_fusion f{};
    f.scale0 = ws + b0.scale; f.shift0 = ws + b0.shift;
    f.y0 = ws + p0.y; f.mean0 = ws + b0.mean; f.invstd0 = ws + b0.invstd;
    f.partials = ws + n->dg_ws; f.partials_bytes = n->dg_ws_bytes;
    int P = 0;
    OSI_TRY(osi_conv_dgrad_fused_frozen(&c.d, ws + n->scratch[dyi], params + c.w_off, ws + n->scratch[dxi], &f, OSI_TILE_AUTO, &P, st));
    n->fused_P = P;
    OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, st));
    return bn_reduce_frozen(n, pc, grads, ws, 0, st);
}

// dgrad of conv `ci` (dy in buffer dyi) into buffer dxi, adding buffer addi (-1: none), with the epilogue fused for the layer
// that produced this conv's input: its ReLU bitmask and the BatchNorm reductions of conv `pc` (and `pd`, the downsample twin).
static int dgrad_fused(osi_resnet50* n, int ci, const float* params, float* ws, int dyi, int dxi, int addi, int pc, int pd,
                       hipStream_t st, bool add_even = false) {
    Conv& c = n->convs[ci];
    Conv& p0 = n->convs[pc];
    BN& b0 = n->bns[p0.bn];
    osi_dgrad_fusion f{};
    if (p0.mask != WS_NONE) f.relu_mask = ws + p0.mask;           // block output: stored ReLU bitmask
    else { f.scale0 = ws + b0.scale; f.shift0 = ws + b0.shift; }     // in-block activation: gate recomputed from y0
    f.y0 = ws + p0.y; f.mean0 = ws + b0.mean; f.invstd0 = ws + b0.invstd;
    if (pd >= 0) {
        Conv& p1 = n->convs[pd];
        BN& b1 = n->bns[p1.bn];
        f.y1 = ws + p1.y; f.mean1 = ws + b1.mean; f.invstd1 = ws + b1.invstd;
    }
    f.partials = ws + n->dg_ws; f.partials_bytes = n->dg_ws_bytes;
    f.addend_stride = add_even ? 2 : 1;
    int P = 0;
    // the in-block 3x3 / stride 1 input gradients (gate recomputed, one consumer, no addend) take the Winograd form
    OSI_TRY(n->wait_weight_transforms(st));   // (forward Winograd off: nobody has waited for the side-stream weight transforms yet)
    if (n->plan_knobs.dgrad_wino && f.scale0 && pd < 0 && addi < 0 && c.u_bw != WS_NONE)
        OSI_TRY(osi_conv_dgrad_fused_wino_pre(&c.d, ws + n->scratch[dyi], ws + c.u_bw, ws + n->scratch[dxi], &f, ws + n->wino_ws,
                                              n->wino_ws_bytes, &P, st));
    else
    OSI_TRY(osi_conv_dgrad_fused(&c.d, ws + n->scratch[dyi], params + c.w_off, ws + n->scratch[dxi],
                                 addi >= 0 ? ws + n->scratch[addi] : nullptr, &f, OSI_TILE_AUTO, &P, st));
    n->fused_P = P;
    return n->mark(OSI_PROF_CONV_DGRAD, st);
}

// In-block step of the backward chain: input gradient of conv `ci` (dy in buffer dyi) into buffer dxi, then the BatchNorm backward of its
// in-block producer `pc` in place, so that dxi holds dy of `pc`. Frozen statistics: both in the epilogue (dgrad_frozen).
static int dgrad_bn_inblock(osi_resnet50* n, int ci, int pc, const float* params, float* grads, float* ws, int dyi, int dxi, hipStream_t st) {
    if (n->frozen) return dgrad_frozen(n, ci, params, grads, ws, dyi, dxi, pc, st);
    OSI_TRY(dgrad_fused(n, ci, params, ws, dyi, dxi, -1, pc, -1, st));
    return bn_bwd_fused(n, pc, params, grads, ws, dxi, dxi, 0, st);
}

// Block backward, entry: the block-output gradient in n->cur_grad becomes *d3 (dy of bn3) and, for a projection block, *t1 (dy of the
// shortcut's BatchNorm: both BatchNorms read the same gated gradient, one pass streams it once and writes both), for an identity block
// *dxbase (the gated gradient itself continues to the block input). The gradient is gated already, its reductions in dg_ws
// (n->go_fused, left by the conv1 dgrad epilogue of the block above), or raw (from the average pool), gated by the stored bitmask here.
static int block_bwd_entry(osi_resnet50* n, const Block& k, const float* params, float* grads, float* ws, hipStream_t st, int* d3, int* t1,
                           int* dxbase) {
    const int go = n->cur_grad;
    const bool has_ds = k.ds >= 0;
    if (!n->go_fused) {
        // A raw gradient reaches a block in one place only, the stage-0 entry from the average pool, and the block it reaches is the last
        // one (layer4.2), an identity block: every block with bi > 0 hands a gated gradient down (go_fused survives stage boundaries), and
        // where the chain ends earlier (no_dx, block 0) no block follows. A raw gradient at a projection block is a broken invariant.
        if (has_ds) return OSI_ERR_STATE;
        OSI_TRY(n->take(st, dxbase));
        if (n->frozen) OSI_TRY(bn_bwd_frozen(n, k.c3, -1, grads, ws, go, go, -1, *dxbase, true, st));
        else OSI_TRY(bn_bwd_raw(n, k.c3, params, grads, ws, go, *dxbase, st));
        *d3 = go;
        return OSI_OK;
    }
    if (has_ds) OSI_TRY(n->take(st, t1));
    if (n->frozen) {            // parameter-only reductions; dy = scale * g needs none
        OSI_TRY(bn_reduce_frozen(n, k.c3, grads, ws, 0, st));
        if (has_ds) OSI_TRY(bn_reduce_frozen(n, k.ds, grads, ws, 1, st));
    }
    OSI_TRY(n->take(st, d3));
    if (n->frozen) OSI_TRY(bn_bwd_frozen(n, k.c3, k.ds, grads, ws, go, *d3, *t1, -1, false, st));
    else if (has_ds) OSI_TRY(bn_bwd_fused_pair(n, k.c3, k.ds, params, grads, ws, go, *d3, *t1, st));
    else OSI_TRY(bn_bwd_fused(n, k.c3, params, grads, ws, go, *d3, 0, st));
    if (has_ds) n->give(go);
    else *dxbase = go;
    return OSI_OK;
}

// Block backward, exit: conv1's input gradient (dy in buffer t3) completes the gradient w.r.t. the block input on top of `dxbase` (the
// shortcut's share) and leaves it in n->cur_grad for the block below.
static int block_bwd_exit(osi_resnet50* n, int bi, const float* params, float* ws, hipStream_t st, int t3, int dxbase, bool no_dx,
                          bool ds_sparse) {
    const Block& k = n->blocks[bi];
    Conv& c1 = n->convs[k.c1];
    auto S = [&](int i) { return ws + n->scratch[i]; };
    if (no_dx) {                   // the chain ends: no launch, the buffers go back
        if (dxbase >= 0) n->give(dxbase);
        n->cur_grad = -1;
        n->go_fused = false;
    } else if (bi > 0) {
        // the block input is the previous block's output: fuse that block's final ReLU mask and its bn3 (+ downsample BN) reductions
        const Block& pk = n->blocks[bi - 1];
        int dxn = dxbase;          // downsample case: add in place (each lane reads then writes its own element)
        if (k.ds < 0) OSI_TRY(n->take(st, &dxn));
        OSI_TRY(dgrad_fused(n, k.c1, params, ws, t3, dxn, dxbase, pk.c3, pk.ds, st, ds_sparse));
        if (dxn != dxbase) n->give(dxbase);
        n->cur_grad = dxn;
        n->go_fused = true;
    } else {
        // first block: its input is the stem's max-pooled activation. With the fused stem tail the epilogue of this LAST input gradient
        // (it completes the gradient w.r.t. the pooled activation) also emits bn1's backward reductions through the arg-max bytes, so the
        // stem needs no reduction pass over its 112 x 112 tensor (pool mode of osi_conv_dgrad_fused)
        // (not when this backward also writes dJ/dimage: the stem tail then materialises dY and reduces bn1 itself)
        if (n->stem_tail_fused()) {
            Conv& c0 = n->convs[0];
            BN& b0 = n->bns[c0.bn];
            osi_dgrad_fusion f{};
            f.y0 = ws + c0.y; f.mean0 = ws + b0.mean; f.invstd0 = ws + b0.invstd;
            f.partials = ws + n->dg_ws; f.partials_bytes = n->dg_ws_bytes;
            f.pool_idx = ws + n->pool_idx; f.pool_H = n->Hs; f.pool_W = n->Ws;
            int P = 0;
            OSI_TRY(osi_conv_dgrad_fused(&c1.d, S(t3), params + c1.w_off, S(dxbase), S(dxbase), &f, OSI_TILE_AUTO, &P, st));
            n->stem_stats_P = P;
            OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, st));
        } else {
            OSI_TRY(dgrad_plain(n, &c1.d, S(t3), params + c1.w_off, S(dxbase), 1, st));
        }
        n->cur_grad = dxbase;
        n->go_fused = false;
    }
    return OSI_OK;
}

// One bottleneck block of the backward pass: entry, shortcut, chain, exit.
// no_dx: the block is the first trainable unit of a backward that stops at the cut: nothing below reads the gradient w.r.t. its
// input, so the two launches that produce it (the shortcut's and conv1's input gradient) are left out and the gradient chain ends here.
// The order of take / give is part of the schedule (FIFO free list: it decides which buffer a launch gets and which reader event it
// waits for): projection block t1, d3, dxbase; identity block d3 (gated) or dxbase (raw); then t2, t3 and the exit's buffer.
static int block_backward(osi_resnet50* n, int bi, const float* params, float* grads, float* ws, hipStream_t st, bool no_dx) {
    const Block& k = n->blocks[bi];
    Conv &c1 = n->convs[k.c1], &c2 = n->convs[k.c2];
    const float* x = ws + k.x_in;
    int d3 = -1, t1 = -1, dxbase = -1, t2 = -1, t3 = -1;
    OSI_TRY(block_bwd_entry(n, k, params, grads, ws, st, &d3, &t1, &dxbase));
    // A stride-2 1x1 shortcut reaches only the even-even pixels of the block input: its input gradient writes just those (a quarter
    // of the tensor, no zero fill) and conv1's input gradient, which completes the sum in place, reads the addend only there.
    // bi == 0 keeps the dense form (pool mode).
    const bool ds_sparse = k.ds >= 0 && bi > 0 && n->convs[k.ds].d.stride == 2 && n->convs[k.ds].d.R == 1;
    if (k.ds >= 0) {               // shortcut: its weight gradient, and its share of the gradient w.r.t. the block input
        Conv& cd = n->convs[k.ds];
        OSI_TRY(wgrad(n, k.ds, grads, ws, t1, x, st));
        if (!no_dx) {
            OSI_TRY(n->take(st, &dxbase));
            OSI_TRY(dgrad_plain(n, &cd.d, ws + n->scratch[t1], params + cd.w_off, ws + n->scratch[dxbase], ds_sparse ? 2 : 0, st));
        }
        n->give(t1);
    }
    // chain: conv3 -> (mask a2, bn2) -> conv2 -> (mask a1, bn1) -> conv1
    OSI_TRY(wgrad(n, k.c3, grads, ws, d3, ws + c2.y, st, c2.bn));
    OSI_TRY(n->take(st, &t2));
    OSI_TRY(dgrad_bn_inblock(n, k.c3, k.c2, params, grads, ws, d3, t2, st));
    n->give(d3);
    OSI_TRY(wgrad(n, k.c2, grads, ws, t2, ws + c1.y, st, c1.bn));
    OSI_TRY(n->take(st, &t3));
    OSI_TRY(dgrad_bn_inblock(n, k.c2, k.c1, params, grads, ws, t2, t3, st));
    n->give(t2);
    OSI_TRY(wgrad(n, k.c1, grads, ws, t3, x, st));
    OSI_TRY(block_bwd_exit(n, bi, params, ws, st, t3, dxbase, no_dx, ds_sparse));
    n->give(t3);
    return OSI_OK;
}

// Stage 0 opens the backward: logits -> fc -> average pool. Leaves the raw gradient w.r.t. the last block's output in n->cur_grad
// (-1 when the backward stops at the head: nobody below reads the gradient w.r.t. the pooled features).
static int head_backward(osi_resnet50* n, const float* params, float* grads, float* ws, const float* dlogits, const float* dfeatures,
                         hipStream_t st) {
    OSI_REQUIRE(dlogits);
    const int head = osi_resnet50::NUNITS - 1;
    n->free_list.clear();
    for (int i = 0; i < osi_resnet50::NSCR; ++i) { n->free_list.push_back(i); n->buf_pending[i] = false; }
    const Tensor& fw = n->tensors[n->t_fc_w]; const Tensor& fb = n->tensors[n->t_fc_b]; const Tensor& lw = n->tensors[n->t_lg_w];
    float* dfeat = ws + n->dfeat;
    int acc = 0;
    if (dfeatures) {
        if (hipMemcpyAsync(dfeat, dfeatures, (size_t)n->B * n->F * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return OSI_ERR_LAUNCH;
        acc = 1;
    }
    const bool pg = n->wants_grads(head);
    float* dlb = pg && n->t_lg_b >= 0 ? grads + n->tensors[n->t_lg_b].off : nullptr;
    OSI_TRY(osi_linear_bwd(dlogits, ws + n->feat, params + lw.off, dfeat, acc, pg ? grads + lw.off : nullptr, dlb, n->B, n->F, n->O, st));
    const bool below = n->bw_stop() < head;
    OSI_TRY(osi_linear_bwd(dfeat, ws + n->pooled, params + fw.off, below ? ws + n->dpooled : nullptr, 0, pg ? grads + fw.off : nullptr,
                           pg ? grads + fb.off : nullptr, n->B, 2048, n->F, st));
    n->cur_grad = -1;
    n->go_fused = false;
    if (below) {
        OSI_TRY(n->take(st, &n->cur_grad));
        OSI_TRY(osi_avgpool_bwd(ws + n->dpooled, ws + n->scratch[n->cur_grad], n->B, n->Hf * n->Wf, 2048, st));
    }
    return n->mark(OSI_PROF_OTHER, st);
}

// The last stage closes the backward: max-pool + stem from the gradient w.r.t. the pooled activation in n->cur_grad.
static int stem_tail(osi_resnet50* n, const float* params, float* grads, float* ws, hipStream_t st) {
    auto S = [&](int i) { return ws + n->scratch[i]; };
    Conv& c0 = n->convs[0];
    BN& b0 = n->bns[c0.bn];
    const BwRequest& rq = n->rq;
    const int go = n->cur_grad;
    int t = -1;
    OSI_TRY(n->take(st, &t));
    const float* x4c = n->x4_cur ? n->x4_cur : ws + n->x4;
    if (n->stem_tail_fused()) {      // its own slab, sized at create: never the side stream's wg_ws
        // reductions of bn1's backward (dgamma, dbeta) on the main stream: they arrived with block 0's last input gradient, two tiny
        // merge launches. Then the weight gradient with the max-pool scatter, ReLU gate and BatchNorm backward applied inside its
        // operand loader: the 112x112x64 gradient is never written
        n->give(t);
        const int P = n->stem_stats_P;
        OSI_TRY(osi_bn_backward_reduce(n->dg_col(ws, 0, P, 64), n->dg_col(ws, 1, P, 64), P, grads + b0.g_off, grads + b0.b_off,
                                       n->B * n->Hs * n->Ws, 64, ws + n->bn_ws, n->bn_ws_bytes, st));
        OSI_TRY(n->mark(OSI_PROF_BN_BWD, st));
        // the stem's weight gradient is the last kernel of the step; on the MAIN stream it runs beside the side stream's
        // backlog (layer1's weight gradients) instead of behind it
        OSI_TRY(osi_stem_wgrad_fused(&c0.d, S(go), ws + n->pool_idx, ws + c0.y, x4c, params + b0.g_off, ws + b0.mean, ws + b0.invstd,
                                     grads + b0.g_off, grads + b0.b_off, grads + c0.w_off, ws + n->stem_ws, n->stem_ws_bytes, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_WGRAD, st));
        n->give(go);
        return OSI_OK;
    }
    // dJ/dimage (or the adversarial batch) wanted, or a geometry the fused form does not take: the stem's dY is materialised (max-pool
    // scatter + ReLU gate + bn1 backward gathered on the fly from the pooled gradient into a scratch buffer), its weight gradient comes
    // from that dY unless input-only, then — for dJ/dimage — the stem's input gradient straight into the caller's NCHW tensor
    if (n->frozen) {   // frozen statistics: dY = scale * (scattered, gated gradient); reductions only for the parameter gradients
        const bool red = n->wants_grads(0);
        OSI_TRY(osi_bn_relu_maxpool_bwd_frozen(S(go), ws + n->pool_idx, ws + c0.y, ws + b0.mean, ws + b0.invstd, ws + b0.scale, S(t),
                                               red ? grads + b0.g_off : nullptr, red ? grads + b0.b_off : nullptr, n->B, n->Hs, n->Ws, 64,
                                               ws + n->bn_ws, n->bn_ws_bytes, st));
    } else {
        OSI_TRY(osi_bn_relu_maxpool_bwd(S(go), ws + n->pool_idx, ws + c0.y, ws + b0.mean, ws + b0.invstd, params + b0.g_off, S(t),
                                        n->dgam(grads, ws, b0), n->dbet(grads, ws, b0), n->B, n->Hs, n->Ws, 64, ws + n->bn_ws,
                                        n->bn_ws_bytes, st));
    }
    OSI_TRY(n->mark(OSI_PROF_BN_BWD, st));
    n->give(go);
    OSI_TRY(wgrad(n, 0, grads, ws, t, x4c, st));
    if (rq.dimage) {
        OSI_TRY(osi_stem_dgrad(S(t), params + c0.w_off, rq.dimage, n->B, n->H, n->W, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, st));
    } else if (rq.x_adv && !rq.x_anchor && rq.alpha == rq.eps) {
        // the same input gradient, ending in the FGSM epilogue: x_adv from the batch the forward read (a projected step of alpha = eps
        // anchored at its own iterate is this one: no second load of the same pixel)
        OSI_TRY(osi_stem_dgrad_fgsm(S(t), params + c0.w_off, x4c, rq.x_adv, rq.eps, rq.lo, rq.hi, n->B, n->H, n->W, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, st));
    } else if (rq.x_adv) {     // ending in the projected step: the next iterate from the batch the forward read and the anchor
        OSI_TRY(osi_stem_dgrad_pgd(S(t), params + c0.w_off, x4c, rq.x_anchor ? rq.x_anchor : x4c, rq.x_adv, rq.alpha, rq.eps, rq.lo, rq.hi,
                                   n->B, n->H, n->W, st));
        OSI_TRY(n->mark(OSI_PROF_CONV_DGRAD, st));
    }
    n->give(t);
    return OSI_OK;
}

static int backward_stages(osi_resnet50_t n, const float* params, float* grads, void* workspace, const float* dlogits,
                           const float* dfeatures, const BwRequest& rq, int stage_lo, int stage_hi, osi_stream_t stream) {
    OSI_REQUIRE(stage_lo >= 0 && stage_lo < stage_hi && stage_hi <= n->n_stages);
    if (!n->fwd_done || stage_lo != n->next_stage || !n->plan_unchanged()) return OSI_ERR_STATE;
    // the inference-form prefix of the forward kept no backward state: no image gradient exists behind it
    if (n->fw_prefix > 0 && (rq.dimage || rq.x_adv)) return OSI_ERR_STATE;
    // the request is fixed by the call that runs stage 0 (block 0's dgrad form depends on it)
    if (stage_lo == 0) n->rq = rq;
    else if (!(n->rq == rq)) return OSI_ERR_STATE;
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (n->wants_side()) OSI_TRY(n->ensure_side());
    OSI_TRY(n->mark(OSI_PROF_START, st));
    // Units below `stop` launch nothing; unit `stop` leaves out its input gradient. A stage wholly below it is still accepted in order.
    const int stop = n->bw_stop();
    for (int stage = stage_lo; stage < stage_hi; ++stage) {
        if (stage == 0) OSI_TRY(head_backward(n, params, grads, ws, dlogits, dfeatures, st));
        for (int bi = (int)n->blocks.size() - 1; bi >= 0; --bi)
            if (n->blocks[bi].stage == stage && bi + 1 >= stop) OSI_TRY(block_backward(n, bi, params, grads, ws, st, bi + 1 == stop));
        if (stage == n->n_stages - 1) {
            if (stop == 0) OSI_TRY(stem_tail(n, params, grads, ws, st));   // (else the stem is frozen and nobody wants the image gradient)
            n->cur_grad = -1;
            n->fwd_done = false;
        }
        n->next_stage = stage + 1;
    }
    // Join once per call: every gradient of the stages just run is final on `st` from here on. A data-parallel caller issues
    // one stage per call (and reduces that slice next); a single-GPU caller issues all stages in one call and pays one join.
    if (n->stage_join || stage_hi == n->n_stages) OSI_TRY(n->join_side(st));
    return OSI_OK;
}

int osi_resnet50_backward(osi_resnet50_t n, const float* params, float* grads, void* workspace, const float* dlogits,
                          const float* dfeatures, int stage_lo, int stage_hi, osi_stream_t stream) {
    return osi_resnet50_backward_ex(n, params, grads, workspace, dlogits, dfeatures, nullptr, 1, stage_lo, stage_hi, stream);
}

int osi_resnet50_backward_ex(osi_resnet50_t n, const float* params, float* grads, void* workspace, const float* dlogits,
                             const float* dfeatures, float* dimage, int param_grads, int stage_lo, int stage_hi, osi_stream_t stream) {
    OSI_REQUIRE(n && params && workspace);
    OSI_REQUIRE(param_grads == 0 || param_grads == 1);
    OSI_REQUIRE(!param_grads || grads);
    OSI_REQUIRE(param_grads || dimage);                 // a backward that produces nothing is a caller error
    OSI_REQUIRE(((uintptr_t)dimage & 3) == 0);
    return backward_stages(n, params, grads, workspace, dlogits, dfeatures, BwRequest{dimage, param_grads, nullptr, 0.f, 0.f, 0.f, nullptr, 0.f}, stage_lo,
                           stage_hi, stream);
}

// The batch an attack epilogue writes may not touch the batch the forward read (bound in place, or the copy inside the workspace), anything
// else in the workspace, or the anchor: other workgroups still read those pixels — and conv1's weight gradient on the side stream reads
// the forward's batch — while the epilogue writes.
static bool attack_output_apart(const osi_resnet50* n, const void* workspace, const float* x_out, const float* x_anchor) {
    const size_t img_bytes = (size_t)n->B * n->H * n->W * 4 * sizeof(float);
    auto apart = [&](const void* p, size_t bytes) {
        const uintptr_t a = (uintptr_t)x_out, b = (uintptr_t)p;
        return a + img_bytes <= b || b + bytes <= a;
    };
    return apart(workspace, n->ws_floats * sizeof(float)) && (!n->x4_cur || apart(n->x4_cur, img_bytes)) &&
           (!x_anchor || apart(x_anchor, img_bytes));
}

int osi_resnet50_backward_adv(osi_resnet50_t n, const float* params, float* grads, void* workspace, const float* dlogits,
                              const float* dfeatures, float* x_adv_nhwc4, float eps, float lo, float hi, int stage_lo, int stage_hi,
                              osi_stream_t stream) {
    OSI_REQUIRE(n && params && grads && workspace && x_adv_nhwc4);
    OSI_REQUIRE(((uintptr_t)x_adv_nhwc4 & 15) == 0 && eps >= 0.f && lo <= hi);
    OSI_REQUIRE(attack_output_apart(n, workspace, x_adv_nhwc4, nullptr));
    return backward_stages(n, params, grads, workspace, dlogits, dfeatures, BwRequest{nullptr, 1, x_adv_nhwc4, eps, lo, hi, nullptr, eps},
                           stage_lo, stage_hi, stream);
}

int osi_resnet50_backward_attack(osi_resnet50_t n, const float* params, float* grads, void* workspace, const float* dlogits,
                                 const float* dfeatures, const osi_attack* a, int param_grads, int stage_lo, int stage_hi,
                                 osi_stream_t stream) {
    OSI_REQUIRE(n && params && workspace && a && a->x_next);
    OSI_REQUIRE(param_grads == 0 || param_grads == 1);
    OSI_REQUIRE(!param_grads || grads);
    OSI_REQUIRE(((uintptr_t)a->x_next & 15) == 0 && ((uintptr_t)a->x_anchor & 15) == 0);
    OSI_REQUIRE(a->eps >= 0.f && a->lo <= a->hi && a->alpha - a->alpha == 0.f);
    OSI_REQUIRE(attack_output_apart(n, workspace, a->x_next, a->x_anchor));
    return backward_stages(n, params, grads, workspace, dlogits, dfeatures,
                           BwRequest{nullptr, param_grads, a->x_next, a->eps, a->lo, a->hi, a->x_anchor, a->alpha}, stage_lo, stage_hi, stream);
}

// Hand the gradients of the stages enqueued so far to another stream WITHOUT stalling the compute stream: `waiter` waits for the
// work enqueued on `main` up to now and for the side stream's weight gradients; `main` waits for nothing.
int osi_resnet50_grads_ready(osi_resnet50_t n, osi_stream_t main_stream, osi_stream_t waiter_stream) {
    OSI_REQUIRE(n);
    hipStream_t mn = (hipStream_t)main_stream, wt = (hipStream_t)waiter_stream;
    if (!n->ev_rmain) {
        if (hipEventCreateWithFlags(&n->ev_rmain, EV_FLAGS_HANDOFF) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipEventCreateWithFlags(&n->ev_rside, EV_FLAGS_HANDOFF) != hipSuccess) return OSI_ERR_LAUNCH;
    }
    if (hipEventRecord(n->ev_rmain, mn) != hipSuccess) return OSI_ERR_LAUNCH;
    if (hipStreamWaitEvent(wt, n->ev_rmain, 0) != hipSuccess) return OSI_ERR_LAUNCH;
    if (n->side && n->side_dirty) {
        if (hipEventRecord(n->ev_rside, n->side) != hipSuccess) return OSI_ERR_LAUNCH;
        if (hipStreamWaitEvent(wt, n->ev_rside, 0) != hipSuccess) return OSI_ERR_LAUNCH;
    }
    return OSI_OK;
}

// ---- debug: the non-smooth decisions of the latest forward (tests only; the product path never calls these) -------------------
// The network's only non-differentiable points are its 49 ReLUs and the max-pool's arg-max. A whole-network gradient check
// against an fp64 oracle is dominated by the few elements where fp32 rounding flips such a decision (2e-2 relative); with the
// oracle taking THIS run's decisions the comparison is 400x tighter (tests/test_gate_pinned_gpu.py). Each gate is read from what
// the backward itself consumes: the stored bitmask for block outputs, fma(y0, scale0, shift0) > 0 for the in-block activations
// that were never materialised (the expression the forward loader and the dgrad epilogue evaluate), bit 7 / the low bits of the
// arg-max byte for the fused stem tail. Output order is the oracle's NCHW.
namespace {
__global__ __launch_bounds__(256) void k_dbg_gate_bits(const unsigned long long* __restrict__ bits, unsigned char* __restrict__ out,
                                                       size_t n, int HW, int C) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;   // NHWC element index
    if (e >= n) return;
    const size_t i4 = e >> 2;
    const unsigned long long w = bits[(i4 >> 6) * 4 + (e & 3)];
    const size_t pix = e / C;
    const int c = (int)(e - pix * C);
    const size_t b = pix / HW, hw = pix - b * HW;
    out[(b * C + c) * HW + hw] = (unsigned char)((w >> (i4 & 63)) & 1);
}
__global__ __launch_bounds__(256) void k_dbg_gate_fma(const float* __restrict__ y, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, unsigned char* __restrict__ out, size_t n, int HW,
                                                      int C) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t pix = e / C;
    const int c = (int)(e - pix * C);
    const size_t b = pix / HW, hw = pix - b * HW;
    out[(b * C + c) * HW + hw] = __builtin_fmaf(y[e], scale[c], shift[c]) > 0.f ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_dbg_gate_pool(const uint32_t* __restrict__ idx, unsigned char* __restrict__ gate,
                                                       int* __restrict__ argmax, size_t n, int Ws, int Hp, int Wp, int C) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;   // NHWC element of the pooled tensor
    if (e >= n) return;
    const uint32_t byte = (idx[e >> 2] >> (8 * (e & 3))) & 0xffu;
    const size_t pix = e / C;
    const int c = (int)(e - pix * C);
    const size_t b = pix / ((size_t)Hp * Wp), hw = pix - b * Hp * Wp;
    const int ho = (int)(hw / Wp), wo = (int)(hw - (size_t)ho * Wp);
    const int tap = byte & 0x7f, r = tap / 3, s = tap - 3 * r;
    const size_t o = (b * C + c) * ((size_t)Hp * Wp) + hw;
    gate[o] = (unsigned char)(byte >> 7);
    if (argmax) argmax[o] = (ho * 2 - 1 + r) * Ws + (wo * 2 - 1 + s);
}
}  // namespace

int osi_resnet50_debug_num_gates(osi_resnet50_t n) { return n ? 1 + 3 * (int)n->blocks.size() : 0; }

int osi_resnet50_debug_gate_shape(osi_resnet50_t n, int i, int* C, int* H, int* W) {
    OSI_REQUIRE(n && C && H && W && i >= 0 && i < 1 + 3 * (int)n->blocks.size());
    if (i == 0) { *C = 64; *H = n->Hp; *W = n->Wp; return OSI_OK; }
    const Block& k = n->blocks[(i - 1) / 3];
    const int which = (i - 1) % 3;
    const osi_conv_desc& d = n->convs[which == 0 ? k.c1 : which == 1 ? k.c2 : k.c3].d;
    *C = d.Cout; *H = d.Ho; *W = d.Wo;
    return OSI_OK;
}

int osi_resnet50_debug_gate(osi_resnet50_t n, void* workspace, int i, unsigned char* gate_nchw, int* pool_argmax_nchw,
                            osi_stream_t stream) {
    OSI_REQUIRE(n && workspace && gate_nchw && i >= 0 && i < 1 + 3 * (int)n->blocks.size());
    OSI_REQUIRE(i == 0 || !pool_argmax_nchw);
    if (!n->any_fwd) return OSI_ERR_STATE;
    if ((i == 0 ? 0 : (i - 1) / 3 + 1) < n->fw_prefix) return OSI_ERR_STATE;   // a unit that ran the inference form stored no decision
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (i == 0) {
        const size_t e = (size_t)n->B * n->Hp * n->Wp * 64;
        hipLaunchKernelGGL(k_dbg_gate_pool, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, (const uint32_t*)(ws + n->pool_idx),
                           gate_nchw, pool_argmax_nchw, e, n->Ws, n->Hp, n->Wp, 64);
        OSI_LAUNCH_CHECK();
        return OSI_OK;
    }
    const Block& k = n->blocks[(i - 1) / 3];
    const int which = (i - 1) % 3;
    const Conv& c = n->convs[which == 0 ? k.c1 : which == 1 ? k.c2 : k.c3];
    const BN& b = n->bns[c.bn];
    const size_t e = (size_t)b.M * b.C;
    const int HW = c.d.Ho * c.d.Wo;
    if (which == 2)
        hipLaunchKernelGGL(k_dbg_gate_bits, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st,
                           (const unsigned long long*)(ws + c.mask), gate_nchw, e, HW, b.C);
    else
        hipLaunchKernelGGL(k_dbg_gate_fma, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, st, ws + c.y, ws + b.scale, ws + b.shift,
                           gate_nchw, e, HW, b.C);
    OSI_LAUNCH_CHECK();
    return OSI_OK;
}

int osi_resnet50_debug_unit_input(osi_resnet50_t n, void* workspace, int unit, float* out_nhwc, size_t* floats, osi_stream_t stream) {
    OSI_REQUIRE(n && floats && unit >= 1 && unit <= (int)n->blocks.size());
    const Block& k = n->blocks[unit - 1];
    const osi_conv_desc& d = n->convs[k.c1].d;
    *floats = (size_t)n->B * d.H * d.W * d.Cin;
    if (!out_nhwc) return OSI_OK;
    OSI_REQUIRE(workspace);
    if (!n->ran_fwd) return OSI_ERR_STATE;
    if (hipMemcpyAsync(out_nhwc, (const float*)workspace + k.x_in, *floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
        hipSuccess)
        return OSI_ERR_LAUNCH;
    return OSI_OK;
}

// The head's input as the latest forward left it: forward_impl is the one body of osi_resnet50_forward (training or not, eval_fused or
// not) and osi_resnet50_forward_frozen, and it always ends in head_fwd, which writes ws + pooled. Nothing else writes that tensor.
int osi_resnet50_pooled(osi_resnet50_t n, void* workspace, float* out, size_t* floats, osi_stream_t stream) {
    OSI_REQUIRE(n && floats);
    *floats = (size_t)n->B * 2048;
    if (!out) return OSI_OK;
    OSI_REQUIRE(workspace);
    if (!n->ran_fwd) return OSI_ERR_STATE;
    if (hipMemcpyAsync(out, (const float*)workspace + n->pooled, *floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) !=
        hipSuccess)
        return OSI_ERR_LAUNCH;
    return OSI_OK;
}

int osi_resnet50_set_option(osi_resnet50_t n, const char* name, int value) {
    OSI_REQUIRE(n && name);
    if (!strcmp(name, "overlap")) n->overlap = value != 0;
    else if (!strcmp(name, "fwd_fork")) n->fwd_fork = value != 0;
    else if (!strcmp(name, "stage_join")) n->stage_join = value != 0;
    else if (!strcmp(name, "eval_fused")) n->eval_fused = value != 0;
    else if (!strcmp(name, "forget_forward")) { if (value) n->fwd_done = false; }
    else if (!strcmp(name, "side_priority_normal")) {
        if (n->side) return OSI_ERR_STATE;   // the side stream already exists with the other priority
        n->side_prio_normal = value != 0;
    } else return OSI_ERR_ARG;
    return OSI_OK;
}

}  // extern "C"
