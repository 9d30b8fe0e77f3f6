// libgance_hip.so: the StyleGAN2 engine (the skip generator of config-f and config-e) behind include/gance_hip.h.
//
// Owns one network's weights (re-laid-out for the kernels) and a workspace sized for max_batch
// frames in HBM, and turns a batch of dlatents (or z vectors) into uint8 NHWC frames with a fixed
// sequence of kernel launches on the caller's stream. Replaces the TF1 session behind
// gance/network_interface/network_functions.py:114-192 (wrap_loaded_network) for the reference's
// two call forms (`network.run`, `network.components.synthesis.run`).
//
// There is NO CPU fallback: without a HIP device every entry point fails with an error code.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/gance_hip.h"
#include "kernels.h"
#include "engine_plan.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& message) {
    g_last_error = message;
    return code;
}
}  // namespace
namespace gance {
int set_last_error(int code, const std::string& message) { return fail(code, message); }
}  // namespace gance
namespace {

#define GANCE_HIP_CHECK(expr)                                                              \
    do {                                                                                   \
        hipError_t gance_err_ = (expr);                                                    \
        if (gance_err_ != hipSuccess) {                                                    \
            return fail(gance_err_ == hipErrorOutOfMemory ? GANCE_ERR_OUT_OF_MEMORY        \
                                                          : GANCE_ERR_HIP,                 \
                        std::string(#expr) + ": " + hipGetErrorString(gance_err_));        \
        }                                                                                  \
    } while (0)

constexpr int kDlatent = 512;
constexpr int kMappingLayers = 8;
constexpr float kMappingLrmul = 0.01f;

// feature maps at a stage (stage = res_log2 - 1): fmap_base = 16 << 10 in config-f, 8 << 10 in config-e (GANCE_FLAG_FMAP_BASE_8K)
int fmap_base_of_flags(int flags) { return (flags & GANCE_FLAG_FMAP_BASE_8K) ? (8 << 10) : (16 << 10); }
int nf(int stage, int fmap_base) {
    const int v = fmap_base >> stage;
    return std::min(std::max(v, 1), 512);
}
int round_up32(int n) { return (n + 31) & ~31; }  // style / demod columns are dealt out in blocks of 32 (styles_kernel, demod_kernel)

struct RgbLayerHost {
    int res_log2, cin, row;
};

void build_spec(int res_log2, int fmap_base, std::vector<ConvLayerHost>* convs, std::vector<RgbLayerHost>* rgbs) {
    const auto fm = [fmap_base](int stage) { return nf(stage, fmap_base); };
    convs->push_back({0, 2, fm(1), fm(1), false});
    rgbs->push_back({2, fm(1), 1});
    for (int res = 3; res <= res_log2; ++res) {
        convs->push_back({res * 2 - 5, res, fm(res - 2), fm(res - 1), true});
        convs->push_back({res * 2 - 4, res, fm(res - 1), fm(res - 1), false});
        rgbs->push_back({res, fm(res - 1), res * 2 - 3});
    }
}

uint64_t blob_floats(int res_log2, int fmap_base) {
    std::vector<ConvLayerHost> convs;
    std::vector<RgbLayerHost> rgbs;
    build_spec(res_log2, fmap_base, &convs, &rgbs);
    const auto nf = [fmap_base](int stage) { return ::nf(stage, fmap_base); };
    uint64_t n = 0;
    n += (uint64_t)kMappingLayers * (kDlatent * kDlatent + kDlatent);
    n += kDlatent;
    n += (uint64_t)nf(1) * 16;
    for (const auto& c : convs)
        n += (uint64_t)9 * c.cin * c.cout + (uint64_t)kDlatent * c.cin + c.cin + 1 + c.cout;
    for (const auto& r : rgbs) n += (uint64_t)r.cin * 3 + (uint64_t)kDlatent * r.cin + r.cin + 3;
    for (const auto& c : convs) n += (uint64_t)1 << (2 * c.res_log2);
    return n;
}

int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

// zero-bordered geometry
size_t act_plane(int res) { return (size_t)(res + 2) * (res + 8); }       // one channel, interior at [y+1][x+4]
size_t t_plane(int h) { return (size_t)(h + 3) * (h + 8); }               // one channel, one class

// weight slot t of the transposed conv reads filter tap kUpTapWeight[t] (= wy*3+wx); order must
// match conv_mfma.hip's tap tables: EE (0,0) (0,-1) (-1,0) (-1,-1) | EO (0,0) (-1,0) | OE (0,0) (0,-1) | OO
const int kUpTapWeight[9] = {8, 6, 2, 0, 7, 1, 5, 3, 4};

struct StepRecord {
    char name[64];
    double flops, bytes;
    hipEvent_t start, stop;
};

}  // namespace

// Per-call scratch (activations, parity planes, split-K slabs, skip images, styles ...): about 0.8 GB per frame
// of batch capacity at 1024^2 against 0.55 GB of weights per network (135 MB as trained, the rest the same weights as each kernel form's LDS image). It holds nothing between calls except its
// zero borders, which depend only on the resolution, so every engine of one (device, resolution, max_batch)
// shares ONE workspace: 20 resident networks cost 20 x weights + 1 x workspace. Calls that share it are ordered
// by an event (a call waits for the previous user's last kernel, on whatever stream that ran).
struct gance_workspace {
    int device = 0, resolution = 0, max_batch = 0;
    float *dlat = nullptr, *map_a = nullptr, *map_b_buf = nullptr, *z_in = nullptr;
    float *styles = nullptr, *demod = nullptr;
    // whose call last filled styles / demod, and with how many samples (the debug taps that read them back check both)
    const void* front_owner = nullptr;
    int front_batch = 0;
    std::vector<float*> act;      // per conv layer: zero-bordered output [Bmax][cout][res+2][res+8]
    std::vector<float*> tplanes;  // per up layer: [4 cls][max_units][cout][H+3][W+8] (else nullptr)
    float* slabs = nullptr;       // split-K scratch of the small stride-1 convs (dense)
    float *up_packed = nullptr, *up_prod = nullptr;  // the GEMM forms' operand images and products (gemm_forms.hip: scatter-form up layers, Winograd at 8x8 / 16x16)
    float* ybuf[2] = {nullptr, nullptr};
    float* rgb_coef = nullptr;  // [Bmax][8 m tiles][16][64]: A operands of a ToRGB product fused into a Winograd conv epilogue
    float* rgb_part = nullptr;  // [m tiles][Bmax][3][R][R]: its partial images where a pixel's channels span several blocks
    uint8_t* u8buf = nullptr;  // staging for the host-buffer entry points
    size_t u8_bytes = 0;
    std::vector<std::pair<float*, size_t>> dense;  // every float buffer above but act / tplanes, with its floats (gance_engine_debug_poison_scratch)
    hipEvent_t last_use = nullptr;
    bool used = false;
    size_t bytes = 0;
    // host-buffer entry points: their own stream and pinned staging (latents in, uint8 frames out)
    hipStream_t host_stream = nullptr;
    int* fault_flag = nullptr;  // host-mapped word: kernels whose wave-placement assumption failed at run time set it (ConvArgs::fault_flag)
    float* pinned_in = nullptr;
    uint8_t* pinned_out = nullptr;
    ~gance_workspace() {
        gance::DeviceGuard guard(device);
        if (host_stream) hipStreamDestroy(host_stream);
        if (pinned_in) hipHostFree(pinned_in);
        if (fault_flag) hipHostFree(fault_flag);
        if (pinned_out) hipHostFree(pinned_out);
        hipFree(dlat);
        hipFree(map_a);
        hipFree(map_b_buf);
        hipFree(z_in);
        hipFree(styles);
        hipFree(demod);
        for (float* ptr : act) hipFree(ptr);
        for (float* ptr : tplanes) hipFree(ptr);
        hipFree(slabs);
        hipFree(up_packed);
        hipFree(up_prod);
        hipFree(ybuf[0]);
        hipFree(ybuf[1]);
        hipFree(rgb_coef);
        hipFree(rgb_part);
        hipFree(u8buf);
        if (last_use) hipEventDestroy(last_use);
    }
};

struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    bool warmed = false;
    bool disabled = false;  // capture failed once: this combination stays on eager launches
};

struct gance_engine {
    gance_engine_config cfg{};
    int res_log2 = 0;
    int fmap_base = 16 << 10;  // the channel table: nf(stage, fmap_base)
    int num_rows = 0;  // W
    std::vector<ConvLayerHost> convs;
    std::vector<RgbLayerHost> rgbs;

    // device weight pool
    float* pool = nullptr;
    size_t pool_floats = 0;
    // offsets into pool
    size_t map_w[kMappingLayers]{}, map_b[kMappingLayers]{};
    size_t avg_off = 0, const_off = 0, A_off = 0, bias1_off = 0, w2_off = 0;
    std::vector<size_t> conv_bias, conv_noise;
    Tuning tune;                  // the process's tuning, with the per-engine knobs as they stood when this engine was created
    std::vector<LayerCaps> caps;  // per conv layer: the forms this engine may run it in, and where their weight images sit in the pool
    // randomize_noise (the vector path): per-sample planes drawn by gance_engine_randomize_noise, layer li at
    // noise_rand + noise_rand_off[li] as [max_batch][res][res] (SIZE_MAX: the layer's strength is zero, it reads no noise);
    // while noise_randomized the conv launches read these (a plane per sample), else the stored buffers in the pool
    float* noise_rand = nullptr;
    std::vector<size_t> noise_rand_off;
    int noise_rand_count = 0;  // samples the last draw covered
    bool noise_randomized = false;
    size_t up_packed_floats = 0, up_prod_floats = 0;
    int num_cus = 256;
    std::vector<float> conv_ns;
    std::vector<int> conv_s_off, conv_d_off;
    std::vector<size_t> rgb_w, rgb_bias;
    std::vector<int> rgb_s_off;
    int ctot = 0, dtot = 0;
    int* blk_row = nullptr;
    gance::DemodLayer* demod_layers = nullptr;

    // workspace (shared with the other engines of the same device, resolution and max_batch)
    std::shared_ptr<gance_workspace> ws;
    // captured launch sequences of the host-buffer entry points, by (batch, entry kind, psi bits, float image wanted, noise source)
    std::map<std::tuple<int, int, unsigned, int, int>, GraphEntry> graphs;
    std::vector<int> t_units;     // max_units of each up layer's parity planes
    size_t slab_floats = 0, y_floats = 0, rgb_part_floats = 0;

    // profiling / debug
    std::vector<StepRecord> steps;
    std::string profile_only;  // non-empty: bracket only launches whose name contains it
    int steps_used = 0;
    int debug_stop_after = 0;
    bool keep_skip_image = false;  // the caller will read the final fp32 skip image out of ybuf
    int last_act_layer = 0, last_act_c = 0, last_act_side = 0;
    // the fp32 skip image the last ToRGB of the last eagerly launched call stored (nullptr: none ran, or it stored bytes only)
    const float* last_rgb_y = nullptr;
    int last_rgb_side = 0, last_rgb_batch = 0;
    hipStream_t last_stream = nullptr;
};

namespace {

void free_engine(gance_engine* e) {
    if (!e) return;
    gance::DeviceGuard guard(e->cfg.device);
    for (auto& s : e->steps) {
        hipEventDestroy(s.start);
        hipEventDestroy(s.stop);
    }
    hipFree(e->pool);
    hipFree(e->noise_rand);
    hipFree(e->blk_row);
    hipFree(e->demod_layers);
    if (e->ws && e->ws->used) hipEventSynchronize(e->ws->last_use);  // nothing of this engine still runs on the shared scratch
    for (auto& kv : e->graphs)
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
    e->ws.reset();  // the last engine of a (device, resolution, max_batch) frees the workspace
    delete e;
}

// Profiling bracket around one launch.
struct StepScope {
    gance_engine* e;
    hipStream_t stream;
    StepRecord* rec = nullptr;
    StepScope(gance_engine* engine, hipStream_t s, const char* name, double flops, double bytes)
        : e(engine), stream(s) {
        if (!(e->cfg.flags & GANCE_FLAG_PROFILE_STEPS)) return;
        if (!e->profile_only.empty() && std::strstr(name, e->profile_only.c_str()) == nullptr) return;
        if (e->steps_used == (int)e->steps.size()) {
            StepRecord r{};
            hipEventCreate(&r.start);
            hipEventCreate(&r.stop);
            e->steps.push_back(r);
        }
        rec = &e->steps[e->steps_used++];
        std::snprintf(rec->name, sizeof(rec->name), "%s", name);
        rec->flops = flops;
        rec->bytes = bytes;
        hipEventRecord(rec->start, stream);
    }
    ~StepScope() {
        if (rec) hipEventRecord(rec->stop, stream);
    }
};

// the ToRGB a last-layer conv launch absorbs (kEpilogueRgb)
struct FusedRgb {
    const float *w, *s, *bias, *y_prev;
    float* y;
    uint8_t* u8;
};

// The noise conv layer li adds, and the distance between the planes of two samples: the stored buffer [res][res] shared by
// the batch (stride 0), or after gance_engine_randomize_noise the drawn planes [sample][res][res]; nullptr where the
// layer's strength is zero.
const float* layer_noise(const gance_engine* e, int li, int* b_stride) {
    *b_stride = 0;
    if (e->conv_ns[li] == 0.0f) return nullptr;
    if (e->noise_randomized && e->noise_rand != nullptr && e->noise_rand_off[li] != SIZE_MAX) {
        *b_stride = 1 << (2 * e->convs[li].res_log2);
        return e->noise_rand + e->noise_rand_off[li];
    }
    return e->pool + e->conv_noise[li];
}

// ---- one helper per argument struct: (engine, layer, its plan record, where the data is) -> what the launcher takes ----

// where a conv launch writes: the layer's zero-bordered activation, dense split-K slabs, or an up layer's parity planes
struct ConvOut {
    float* out;
    int epilogue, row_stride, y_off, x_off;
    long long b_stride, c_stride, slab_stride, cls_stride;
};

// the pool offset of the weight image a run_conv launch reads
size_t conv_weights(const LayerCaps& caps, Form form) {
    switch (form) {
        case Form::Wino64: return caps.w[kWino64];
        case Form::Wino43: return caps.w[kWino43];
        default: return caps.direct_w;  // Direct, DirectSplitK, DirectTorgb, UpTwoPass
    }
}

gance::ConvArgs conv_args(const gance_engine* e, int li, const LayerStep& step, const float* x, long long x_b_stride, int H, int W,
                          const ConvOut& o, int B, const FusedRgb* rgb, const float* s_next) {
    const ConvLayerHost& c = e->convs[li];
    const LayerCaps& caps = e->caps[li];
    const LayerPlan& p = step.p;
    gance::ConvArgs a{};
    a.s_next = s_next;
    if (o.epilogue == gance::kEpilogueFullRgbPart) {  // (rgb->y: the partial image; the coefficient table is the workspace's)
        a.rgb_y = rgb->y;
        a.rgb_coef = e->ws->rgb_coef;
    } else if (rgb != nullptr) {
        a.rgb_w = rgb->w;
        a.rgb_s = rgb->s;
        a.rgb_bias = rgb->bias;
        a.rgb_y_prev = rgb->y_prev;
        a.rgb_y = rgb->y;
        a.rgb_u8 = rgb->u8;
    }
    a.x = x;
    // (F(4x4,3x3) and the 16x16x4 kernel's 32-channel geometry take the input multiplied by this layer's style: plan_call arranged
    // that with the producing layer)
    a.w = e->pool + conv_weights(caps, step.form);
    a.s = e->ws->styles + e->conv_s_off[li];
    a.d = e->ws->demod + e->conv_d_off[li];
    a.noise = layer_noise(e, li, &a.noise_b_stride);
    a.bias = e->pool + e->conv_bias[li];
    a.out = o.out;
    a.B = B;
    a.Cin = c.cin;
    a.Cout = c.cout;
    a.H = H;
    a.W = W;
    a.OH = p.OH;
    a.OW = p.OW;
    a.s_stride = e->ctot;
    a.d_stride = e->dtot;
    a.noise_strength = e->conv_ns[li];
    a.tiles_x = p.tiles_x;
    a.tiles_y = p.tiles_y;
    a.row_tiles = p.row_tiles;
    a.col_tiles = p.col_tiles;
    a.m_tiles = p.m_tiles;
    a.nsplit = p.nsplit;
    a.chunks_per_split = p.chunks_per_split;
    a.total_chunks = p.total_chunks;
    a.epilogue = o.epilogue;
    a.out_row_stride = o.row_stride;
    a.out_y_off = o.y_off;
    a.out_x_off = o.x_off;
    a.out_b_stride = o.b_stride;
    a.out_c_stride = o.c_stride;
    a.slab_stride = o.slab_stride;
    a.cls_stride = o.cls_stride;
    a.x_b_stride = x_b_stride;
    a.grid_rounds = e->tune.w43_rounds;
    a.xcd_blocking = 1;  // (the launcher drops it where the launch's pixel tiles are not a multiple of four)
    a.fault_flag = e->ws->fault_flag;
    return a;
}

int run_conv(gance_engine* e, int li, const LayerStep& step, const float* x, long long x_b_stride, int H, int W, const ConvOut& o, int B,
             hipStream_t stream, const FusedRgb* rgb = nullptr, const float* s_next = nullptr) {
    const ConvLayerHost& c = e->convs[li];
    const LayerPlan& p = step.p;
    const char* name = step.name;
    gance::ConvArgs a = conv_args(e, li, step, x, x_b_stride, H, W, o, B, rgb, s_next);
    double flops = 2.0 * 9 * (double)c.cin * c.cout * H * W * B;
    const double out_elems = (double)B * c.cout * (c.up ? 4.0 * H * W : (double)H * W) * p.nsplit;
    double bytes = 4.0 * ((double)B * c.cin * H * W + out_elems + 9.0 * c.cin * c.cout);
    if (o.epilogue == gance::kEpilogueFullRgbPart) {  // + the ToRGB product and its fp32 partial image; no activation when out is null
        flops += 2.0 * 3 * (double)c.cout * H * W * B;
        bytes = 4.0 * ((double)B * c.cin * H * W + (o.out != nullptr ? out_elems : 0.0) + 9.0 * c.cin * c.cout + 3.0 * B * H * W);
    } else if (rgb != nullptr) {  // no activation leaves the chip: the uint8 image and the half-size skip image instead
        flops += 2.0 * 3 * (double)c.cout * H * W * B;
        bytes = 4.0 * ((double)B * c.cin * H * W + 9.0 * c.cin * c.cout + 0.75 * B * H * W) + 3.0 * B * H * W;
    }
    StepScope scope(e, stream, name, flops, bytes);
    if (step.form == Form::Wino43) {
        GANCE_HIP_CHECK(gance::launch_winograd43_conv(a, stream));
        return GANCE_OK;
    }
    if (step.form == Form::Wino64) {
        GANCE_HIP_CHECK(gance::launch_winograd64_conv(a, stream));
        return GANCE_OK;
    }
    GANCE_HIP_CHECK(gance::launch_modconv(p.tile_id, a, p.total_blocks, stream));
    return GANCE_OK;
}

gance::WinoGemmArgs winogemm_args(const gance_engine* e, int li, const float* x, long long x_b_stride, float* out, long long out_b_stride, int B) {
    const ConvLayerHost& c = e->convs[li];
    const int res = 1 << c.res_log2;
    gance::WinoGemmArgs g{};
    g.x = x;
    g.w = e->pool + e->caps[li].w[kWinoGemm];
    g.s = e->ws->styles + e->conv_s_off[li];
    g.d = e->ws->demod + e->conv_d_off[li];
    g.noise = layer_noise(e, li, &g.noise_b_stride);
    g.bias = e->pool + e->conv_bias[li];
    g.packed = e->ws->up_packed;
    g.prod = e->ws->up_prod;
    g.out = out;
    g.x_b_stride = x_b_stride;
    g.out_b_stride = out_b_stride;
    g.noise_strength = e->conv_ns[li];
    g.B = B;
    g.Cin = c.cin;
    g.Cout = c.cout;
    g.H = res;
    g.W = res;
    g.s_stride = e->ctot;
    g.d_stride = e->dtot;
    g.n_tiles = gance::winogemm_n_tiles(B, res, res);
    return g;
}

gance::UpGemmArgs upgemm_args(const gance_engine* e, int li, const float* x, long long x_b_stride, long long cls_stride, long long unit, int B) {
    const ConvLayerHost& c = e->convs[li];
    const int H = (1 << c.res_log2) / 2;
    gance::UpGemmArgs g{};
    g.x = x;
    g.w = e->pool + e->caps[li].w[kUpGemm];
    g.s = e->ws->styles + e->conv_s_off[li];
    g.d = e->ws->demod + e->conv_d_off[li];
    g.packed = e->ws->up_packed;
    g.prod = e->ws->up_prod;
    g.t = e->ws->tplanes[li];
    g.x_b_stride = x_b_stride;
    g.cls_stride = cls_stride;
    g.unit_stride = unit;
    g.B = B;
    g.Cin = c.cin;
    g.Cout = c.cout;
    g.H = H;
    g.W = H;
    g.s_stride = e->ctot;
    g.d_stride = e->dtot;
    g.n_tiles = gance::upgemm_n_tiles(B, H, H);
    return g;
}

// (the geometry comes planned in step.up)
gance::UpFirArgs upfir_args(const gance_engine* e, int li, const LayerStep& step, const float* x, long long x_b_stride, float* out, int B,
                            const float* s_next) {
    const ConvLayerHost& c = e->convs[li];
    const LayerCaps& caps = e->caps[li];
    gance::UpFirArgs u = step.up;
    u.pair_form = step.form == Form::UpFused16x ? 1 : 0;
    u.x = x;
    u.w = e->pool + (step.form == Form::UpSplit ? caps.w[kUpfirSplit] : (step.form == Form::UpFused16x ? caps.w[kUpfir16x] : caps.w[kUpfir16]));
    u.s = e->ws->styles + e->conv_s_off[li];
    u.d = e->ws->demod + e->conv_d_off[li];
    u.noise = layer_noise(e, li, &u.noise_b_stride);
    u.bias = e->pool + e->conv_bias[li];
    u.out = out;
    u.B = B;
    u.Cin = c.cin;
    u.Cout = c.cout;
    u.H = (1 << c.res_log2) / 2;
    u.W = u.H;
    u.s_stride = e->ctot;
    u.d_stride = e->dtot;
    u.noise_strength = e->conv_ns[li];
    u.x_b_stride = x_b_stride;
    u.s_next = s_next;
    u.input_prescaled = step.input_prescaled ? 1 : 0;
    return u;
}

gance::FirArgs fir_args(const gance_engine* e, int li, const LayerStep& step, long long cls_stride, long long unit, float* out, int B,
                        const float* s_next) {
    const ConvLayerHost& c = e->convs[li];
    gance::FirArgs f{};
    f.t = e->ws->tplanes[li];
    f.cls_stride = cls_stride;
    f.unit_stride = unit;
    f.noise = layer_noise(e, li, &f.noise_b_stride);
    f.bias = e->pool + e->conv_bias[li];
    f.out = out;
    f.noise_strength = e->conv_ns[li];
    f.B = B;
    f.C = c.cout;
    f.H = (1 << c.res_log2) / 2;
    f.W = f.H;
    f.nsplit = step.form == Form::UpGemm ? 1 : step.p.nsplit;
    f.s_next = s_next;
    f.s_next_stride = e->ctot;
    return f;
}

// (after a conv launch that did the channel sum: partial image in, bias and skip image added, image and/or bytes out)
gance::ToRgbArgs torgb_args(const gance_engine* e, int ri, const LayerStep& step, const float* x, const float* y_prev, float* y, uint8_t* u8,
                            bool skip_y_store, int B) {
    gance::ToRgbArgs t{};
    t.x = x;
    t.w = e->pool + e->rgb_w[ri];
    t.s = e->ws->styles + e->rgb_s_off[ri];
    t.bias = e->pool + e->rgb_bias[ri];
    t.y_prev = y_prev;
    t.y = y;
    t.u8 = u8;
    t.partial = step.rgb_sum ? (step.rgb_partials == 1 ? t.y : e->ws->rgb_part) : nullptr;  // (one piece: in place)
    t.partials = step.rgb_partials;
    t.skip_y_store = skip_y_store;
    t.B = B;
    t.Cin = e->rgbs[ri].cin;
    t.R = 1 << e->rgbs[ri].res_log2;
    t.s_stride = e->ctot;
    return t;
}

// Plans the call (plan_call: every form decision is made there), then walks the records: fill the argument struct, open the
// profiling bracket under the record's name, launch.
int synthesize_from_dlat(gance_engine* e, const float* d_dlat, int B, uint8_t* d_u8, float* d_f32,
                         hipStream_t stream) {
    {
        StepScope scope(e, stream, "styles", 2.0 * B * kDlatent * e->ctot,
                        4.0 * ((double)kDlatent * e->ctot + (double)B * e->ctot));
        GANCE_HIP_CHECK(gance::launch_styles(d_dlat, e->pool + e->A_off, e->pool + e->bias1_off,
                                             e->blk_row, e->ws->styles, B, e->num_rows, e->ctot,
                                             stream));
    }
    {
        StepScope scope(e, stream, "demod", 0.0, 0.0);
        GANCE_HIP_CHECK(gance::launch_demod(e->ws->styles, e->pool + e->w2_off, e->demod_layers,
                                            (int)e->convs.size(), e->ws->demod, B, e->ctot, e->dtot,
                                            stream));
    }
    e->ws->front_owner = e;
    e->ws->front_batch = B;
    const std::vector<LayerStep> plan = plan_call(e->convs, e->caps, e->tune, e->cfg.flags, e->num_cus, B, e->debug_stop_after);

    int ycur = 0;  // ybuf index holding the current skip image
    bool have_y = false;
    e->last_rgb_y = nullptr;
    e->last_rgb_batch = B;
    const float* x_in = e->pool + e->const_off;  // zero-bordered [512][6][12], shared by the batch
    long long x_b_stride = 0;
    for (int li = 0; li < (int)plan.size(); ++li) {
        const LayerStep& step = plan[li];
        const ConvLayerHost& c = e->convs[li];
        const int res = 1 << c.res_log2, H = res / 2, ri = c.res_log2 - 2;
        float* x_out = e->ws->act[li];
        const long long out_c = (long long)act_plane(res), out_b = out_c * c.cout;
        const ConvOut activation{x_out, gance::kEpilogueFull, res + 8, 1, 4, out_b, out_c, 0, 0};
        const float* const s_next = step.scales_stores ? e->ws->styles + e->conv_s_off[li + 1] : nullptr;
        const long long tc = (long long)t_plane(H), unit = tc * c.cout, cls_stride = unit * e->t_units[li];  // (up layers: the parity planes)
        switch (step.form) {
            case Form::WinoGemm: {
                const gance::WinoGemmArgs g = winogemm_args(e, li, x_in, x_b_stride, x_out, out_b, B);
                const double n = (double)g.n_tiles * 128;
                StepScope scope(e, stream, step.name, 2.0 * 9 * c.cin * c.cout * (double)B * res * res,
                                4.0 * (36.0 * c.cin * c.cout + 2.0 * 36 * (c.cin + c.cout) * n + (double)B * (c.cin + c.cout) * res * res));
                GANCE_HIP_CHECK(gance::launch_winogemm(g, stream));
                break;
            }
            case Form::DirectTorgb: {
                FusedRgb rgb{e->pool + e->rgb_w[ri], e->ws->styles + e->rgb_s_off[ri], e->pool + e->rgb_bias[ri],
                             e->ws->ybuf[ycur], (d_f32 != nullptr || e->keep_skip_image) ? e->ws->ybuf[1 - ycur] : nullptr, d_u8};
                ConvOut o = activation;
                o.epilogue = gance::kEpilogueRgb;
                if (int rc = run_conv(e, li, step, x_in, x_b_stride, res, res, o, B, stream, &rgb)) return rc;
                ycur = 1 - ycur;
                e->last_rgb_y = (d_f32 != nullptr || e->keep_skip_image) ? e->ws->ybuf[ycur] : nullptr;
                e->last_rgb_side = res;
                break;
            }
            case Form::Direct:
            case Form::Wino64:
            case Form::Wino43: {
                if (!step.rgb_sum) {
                    if (int rc = run_conv(e, li, step, x_in, x_b_stride, res, res, activation, B, stream, nullptr, s_next)) return rc;
                    break;
                }
                GANCE_HIP_CHECK(gance::launch_winograd64_rgb_coef(e->pool + e->rgb_w[ri], e->ws->styles + e->rgb_s_off[ri], e->ctot, B, c.cout,
                                                                  e->ws->rgb_coef, stream));
                // (one partial image: straight into the skip buffer ToRGB finishes in place; several: the workspace's)
                FusedRgb part{nullptr, nullptr, nullptr, nullptr, step.rgb_partials == 1 ? e->ws->ybuf[have_y ? 1 - ycur : ycur] : e->ws->rgb_part, nullptr};
                ConvOut o = activation;
                o.epilogue = gance::kEpilogueFullRgbPart;
                if (!step.stores_activation) o.out = nullptr;
                if (int rc = run_conv(e, li, step, x_in, x_b_stride, res, res, o, B, stream, &part, s_next)) return rc;
                break;
            }
            case Form::DirectSplitK: {
                const long long dense_c = (long long)res * res, slab = dense_c * c.cout * B;
                const ConvOut slabs{e->ws->slabs, gance::kEpilogueRaw, res, 0, 0, dense_c * c.cout, dense_c, slab, 0};
                if (int rc = run_conv(e, li, step, x_in, x_b_stride, res, res, slabs, B, stream)) return rc;
                int noise_b_stride = 0;
                const float* noise = layer_noise(e, li, &noise_b_stride);
                StepScope scope(e, stream, step.second, 0.0, 4.0 * (double)slab * (step.p.nsplit + 1));
                GANCE_HIP_CHECK(gance::launch_splitk_finish(e->ws->slabs, slab, step.p.nsplit, noise, e->conv_ns[li], noise_b_stride,
                                                            e->pool + e->conv_bias[li], x_out, B, c.cout, res, res, stream));
                break;
            }
            case Form::UpFused16:
            case Form::UpFused16x:
            case Form::UpSplit: {
                const gance::UpFirArgs u = upfir_args(e, li, step, x_in, x_b_stride, x_out, B, s_next);
                StepScope scope(e, stream, step.name, 2.0 * 9 * (double)c.cin * c.cout * H * H * B,
                                4.0 * ((double)B * c.cin * H * H + (double)B * c.cout * res * res + 9.0 * c.cin * c.cout));
                GANCE_HIP_CHECK(step.form == Form::UpSplit ? gance::launch_upfir_split(u, stream) : gance::launch_upfir16_fused(u, stream));
                break;
            }
            case Form::UpGemm:
            case Form::UpTwoPass: {
                if (step.form == Form::UpGemm) {
                    const gance::UpGemmArgs g = upgemm_args(e, li, x_in, x_b_stride, cls_stride, unit, B);
                    const double n = (double)g.n_tiles * 128;
                    StepScope scope(e, stream, step.name, 2.0 * 9 * c.cin * c.cout * (double)B * H * H,
                                    4.0 * (9.0 * c.cin * c.cout + 2.0 * c.cin * n + 2.0 * 9 * c.cout * n + 4.0 * unit * B));
                    GANCE_HIP_CHECK(gance::launch_upgemm(g, stream));
                } else {
                    const ConvOut planes{e->ws->tplanes[li], gance::kEpilogueRaw, H + 8, 1, 4, unit, tc, unit * B, cls_stride};
                    if (int rc = run_conv(e, li, step, x_in, x_b_stride, H, H, planes, B, stream)) return rc;
                }
                const gance::FirArgs f = fir_args(e, li, step, cls_stride, unit, x_out, B, s_next);
                StepScope scope(e, stream, step.second, 0.0, 4.0 * (double)B * c.cout * res * res * (step.p.nsplit + 1));
                GANCE_HIP_CHECK(gance::launch_fir_epilogue(f, stream));
                break;
            }
        }
        x_in = x_out;
        x_b_stride = out_b;
        e->last_act_layer = li;
        e->last_act_c = c.cout;
        e->last_act_side = res;

        if (step.torgb[0] != '\0') {
            const bool last = (c.res_log2 == e->res_log2);
            // (a call stopped by a debug tap keeps the image: gance_engine_debug_read_skip_image reads it)
            const bool skip_y_store = step.may_skip_y_store && d_u8 != nullptr && d_f32 == nullptr && !e->keep_skip_image && e->debug_stop_after <= 0;
            const gance::ToRgbArgs t = torgb_args(e, ri, step, x_in, have_y ? e->ws->ybuf[ycur] : nullptr, e->ws->ybuf[have_y ? 1 - ycur : ycur],
                                                  last ? d_u8 : nullptr, skip_y_store, B);
            const double px = (double)B * res * res;
            StepScope scope(e, stream, step.torgb, step.rgb_sum ? 0.0 : 2.0 * 3 * (double)t.Cin * px,
                            step.rgb_sum ? px * (12.0 * step.rgb_partials + 3.0 + (t.skip_y_store ? 0.0 : 12.0) + (t.u8 != nullptr ? 3.0 : 0.0))
                                         : 4.0 * px * (t.Cin + 3 + 0.75) + 3.0 * px);
            GANCE_HIP_CHECK(gance::launch_torgb(t, stream));
            if (have_y) ycur = 1 - ycur;
            have_y = true;
            e->last_rgb_y = skip_y_store ? nullptr : e->ws->ybuf[ycur];
            e->last_rgb_side = res;
        }
    }
    if (d_f32 != nullptr && (int)plan.size() == (int)e->convs.size()) {
        const size_t bytes = (size_t)B * 3 * e->cfg.resolution * e->cfg.resolution * sizeof(float);
        GANCE_HIP_CHECK(hipMemcpyAsync(d_f32, e->ws->ybuf[ycur], bytes, hipMemcpyDeviceToDevice, stream));
    }
    e->last_stream = stream;
    return GANCE_OK;
}

// the workspaces alive in this process, by (device, resolution, max_batch, channel table: its buffers are sized by the layers' channels)
std::mutex g_workspace_mutex;
std::map<std::tuple<int, int, int, int>, std::weak_ptr<gance_workspace>> g_workspaces;

int acquire_workspace(gance_engine* e) {
    const bool shared = !(e->cfg.flags & GANCE_FLAG_PRIVATE_WORKSPACE);
    const auto key = std::make_tuple((int)e->cfg.device, (int)e->cfg.resolution, (int)e->cfg.max_batch, (int)(e->cfg.flags & GANCE_FLAG_FMAP_BASE_8K));
    std::lock_guard<std::mutex> lock(g_workspace_mutex);
    if (shared) {
        auto it = g_workspaces.find(key);
        if (it != g_workspaces.end())
            if (auto alive = it->second.lock()) {
                e->ws = alive;
                return GANCE_OK;
            }
    }
    auto ws = std::make_shared<gance_workspace>();
    ws->device = e->cfg.device;
    ws->resolution = e->cfg.resolution;
    ws->max_batch = e->cfg.max_batch;
    const int nconv = (int)e->convs.size(), Bmax = e->cfg.max_batch;
    ws->act.assign(nconv, nullptr);
    ws->tplanes.assign(nconv, nullptr);
    auto alloc = [&](void** ptr, size_t bytes, bool zero) {
        hipError_t err = hipMalloc(ptr, bytes);
        if (err == hipSuccess && zero) err = hipMemset(*ptr, 0, bytes);
        if (err != hipSuccess) {
            fail(err == hipErrorOutOfMemory ? GANCE_ERR_OUT_OF_MEMORY : GANCE_ERR_HIP,
                 std::string("workspace allocation of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(err));
            return false;
        }
        ws->bytes += bytes;
        return true;
    };
    bool ok = alloc((void**)&ws->dlat, (size_t)Bmax * e->num_rows * kDlatent * sizeof(float), false) &&
              alloc((void**)&ws->map_a, (size_t)Bmax * kDlatent * sizeof(float), false) &&
              alloc((void**)&ws->map_b_buf, (size_t)Bmax * kDlatent * sizeof(float), false) &&
              alloc((void**)&ws->z_in, (size_t)Bmax * kDlatent * sizeof(float), false) &&
              alloc((void**)&ws->styles, (size_t)Bmax * e->ctot * sizeof(float), false) &&
              alloc((void**)&ws->demod, (size_t)Bmax * e->dtot * sizeof(float), false);
    for (int i = 0; ok && i < nconv; ++i) {
        // every layer owns its zero-bordered output (and parity planes): kernels only ever write
        // interiors, so the borders are zeroed exactly once, here
        const ConvLayerHost& c = e->convs[i];
        ok = alloc((void**)&ws->act[i], (size_t)Bmax * c.cout * act_plane(1 << c.res_log2) * sizeof(float), true);
        if (ok && c.up)
            ok = alloc((void**)&ws->tplanes[i], (size_t)4 * e->t_units[i] * c.cout * t_plane((1 << c.res_log2) / 2) * sizeof(float), true);
    }
    ok = ok && alloc((void**)&ws->up_packed, std::max<size_t>(1, e->up_packed_floats) * sizeof(float), false) &&
         alloc((void**)&ws->up_prod, std::max<size_t>(1, e->up_prod_floats) * sizeof(float), false);
    ok = ok && alloc((void**)&ws->slabs, e->slab_floats * sizeof(float), false) &&
         alloc((void**)&ws->ybuf[0], e->y_floats * sizeof(float), false) && alloc((void**)&ws->ybuf[1], e->y_floats * sizeof(float), false) &&
         alloc((void**)&ws->rgb_coef, (size_t)Bmax * 8 * 16 * 64 * sizeof(float), false) &&
         alloc((void**)&ws->rgb_part, std::max<size_t>(1, e->rgb_part_floats) * sizeof(float), false) && alloc((void**)&ws->u8buf, e->y_floats, false);
    if (ok && (hipEventCreateWithFlags(&ws->last_use, hipEventDisableTiming) != hipSuccess ||
               hipStreamCreateWithFlags(&ws->host_stream, hipStreamNonBlocking) != hipSuccess ||
               hipHostMalloc((void**)&ws->fault_flag, sizeof(int), hipHostMallocMapped) != hipSuccess ||
               hipHostMalloc((void**)&ws->pinned_in, (size_t)Bmax * e->num_rows * kDlatent * sizeof(float), hipHostMallocDefault) != hipSuccess ||
               hipHostMalloc((void**)&ws->pinned_out, e->y_floats, hipHostMallocDefault) != hipSuccess)) {
        fail(GANCE_ERR_HIP, "stream / event / pinned staging creation failed");
        ok = false;
    }
    if (!ok) return GANCE_ERR_OUT_OF_MEMORY;  // (the partial workspace frees itself; the message is already recorded)
    *ws->fault_flag = 0;
    ws->u8_bytes = e->y_floats;
    ws->dense = {{ws->dlat, (size_t)Bmax * e->num_rows * kDlatent}, {ws->map_a, (size_t)Bmax * kDlatent}, {ws->map_b_buf, (size_t)Bmax * kDlatent},
                 {ws->z_in, (size_t)Bmax * kDlatent}, {ws->styles, (size_t)Bmax * e->ctot}, {ws->demod, (size_t)Bmax * e->dtot},
                 {ws->up_packed, std::max<size_t>(1, e->up_packed_floats)}, {ws->up_prod, std::max<size_t>(1, e->up_prod_floats)},
                 {ws->slabs, e->slab_floats}, {ws->ybuf[0], e->y_floats}, {ws->ybuf[1], e->y_floats},
                 {ws->rgb_coef, (size_t)Bmax * 8 * 16 * 64}, {ws->rgb_part, std::max<size_t>(1, e->rgb_part_floats)}};
    if (shared) g_workspaces[key] = ws;
    e->ws = ws;
    return GANCE_OK;
}

// calls that share a workspace run one after the other, whatever streams they were given
struct WorkspaceTurn {
    gance_workspace* ws;
    hipStream_t stream;
    WorkspaceTurn(gance_workspace* w, hipStream_t s) : ws(w), stream(s) {
        if (ws->used) hipStreamWaitEvent(stream, ws->last_use, 0);
    }
    ~WorkspaceTurn() {
        hipEventRecord(ws->last_use, stream);
        ws->used = true;
    }
};

int check_call(gance_engine* e, const void* in, int batch) {
    if (e == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (in == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "input pointer is NULL");
    if (batch < 1 || batch > e->cfg.max_batch)
        return fail(GANCE_ERR_INVALID_ARGUMENT,
                    "batch " + std::to_string(batch) + " outside [1, max_batch=" +
                        std::to_string(e->cfg.max_batch) + "]");
    if (e->ws && e->ws->fault_flag != nullptr && *(volatile int*)e->ws->fault_flag != 0) {
        // (sticky: the frames of the call that raised it, and of any call queued behind it, are invalid)
        return fail(GANCE_ERR_HIP, "a two-waves-per-SIMD kernel (code " + std::to_string(*(volatile int*)e->ws->fault_flag) +
                                       ") found its waves placed otherwise than its roles assume: frames since the previous successful call are "
                                       "invalid; rebuild libgance_hip.so with tools/check_w43_isa.py passing, or run with conv_form=\"winograd\"");
    }
    if (e->noise_randomized && e->noise_rand != nullptr && batch > e->noise_rand_count)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_randomize_noise drew noise for " + std::to_string(e->noise_rand_count) +
                                                    " samples, this call has " + std::to_string(batch));
    return GANCE_OK;
}

}  // namespace

extern "C" {

const char* gance_last_error(void) { return g_last_error.c_str(); }
int gance_abi_version(void) { return GANCE_ABI_VERSION; }

uint64_t gance_weight_blob_floats_flags(int32_t resolution, int32_t flags) {
    const int l = ilog2_exact(resolution);
    if (l < 3 || l > 10) return 0;
    return blob_floats(l, fmap_base_of_flags(flags));
}
uint64_t gance_weight_blob_floats(int32_t resolution) { return gance_weight_blob_floats_flags(resolution, 0); }

int gance_engine_create(const gance_engine_config* config, const float* host_weights,
                        uint64_t num_floats, gance_engine** out_engine) {
    if (config == nullptr || host_weights == nullptr || out_engine == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_engine_create");
    *out_engine = nullptr;
    const int res_log2 = ilog2_exact(config->resolution);
    if (res_log2 < 3 || res_log2 > 10)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "resolution must be a power of two in [8, 1024]");
    if (config->max_batch < 1 || config->max_batch > 64)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "max_batch must be in [1, 64]");
    const int fmap_base = fmap_base_of_flags(config->flags);
    if (num_floats != blob_floats(res_log2, fmap_base))
        return fail(GANCE_ERR_BAD_WEIGHTS,
                    "weight blob has " + std::to_string(num_floats) + " floats, expected " +
                        std::to_string(blob_floats(res_log2, fmap_base)) + (fmap_base == (8 << 10) ? " (config-e)" : ""));
    int device_count = 0;
    const hipError_t count_err = hipGetDeviceCount(&device_count);
    if (count_err != hipSuccess || device_count < 1)
        return fail(GANCE_ERR_NO_DEVICE,
                    std::string("no HIP device visible (hipGetDeviceCount: ") +
                        hipGetErrorString(count_err) + ", count " + std::to_string(device_count) +
                        "); libgance_hip has no CPU path");
    if (config->device < 0 || config->device >= device_count)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    gance::DeviceGuard guard(config->device);  // the caller's current device is restored on return
    GANCE_HIP_CHECK(guard.status());
    int num_cus = 0;
    GANCE_HIP_CHECK(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, config->device));

    gance_engine* e = new gance_engine();
    e->tune = engine_tuning();  // (the per-engine knobs as they stand now: a test creates engines with and without them)
    e->cfg = *config;
    e->num_cus = num_cus > 0 ? num_cus : 256;
    e->res_log2 = res_log2;
    e->fmap_base = fmap_base;
    const auto nf = [fmap_base](int stage) { return ::nf(stage, fmap_base); };
    e->num_rows = res_log2 * 2 - 2;
    build_spec(res_log2, fmap_base, &e->convs, &e->rgbs);
    const int nconv = (int)e->convs.size();
    const int nrgb = (int)e->rgbs.size();

    // ---- style / demod column layout ----
    e->conv_s_off.resize(nconv);
    e->conv_d_off.resize(nconv);
    e->rgb_s_off.resize(nrgb);
    int ctot = 0, dtot = 0;
    for (int i = 0; i < nconv; ++i) {
        // (every layer's columns start a block of 32: a 16-channel layer -- config-e at 1024^2 -- leaves half a block unused)
        e->conv_s_off[i] = ctot;
        ctot += round_up32(e->convs[i].cin);
        e->conv_d_off[i] = dtot;
        dtot += round_up32(e->convs[i].cout);
    }
    for (int i = 0; i < nrgb; ++i) {
        e->rgb_s_off[i] = ctot;
        ctot += round_up32(e->rgbs[i].cin);
    }
    e->ctot = ctot;
    e->dtot = dtot;

    // ---- build the processed weight pool on the host ----
    std::vector<float> pool;
    auto reserve = [&](size_t n) {
        const size_t off = pool.size();
        pool.resize(off + ((n + 3) & ~(size_t)3), 0.f);  // keep every array 16-B aligned
        return off;
    };
    const float* src = host_weights;
    // mapping
    const float map_coef = (float)(1.0 / std::sqrt((double)kDlatent) * kMappingLrmul);
    for (int i = 0; i < kMappingLayers; ++i) {
        e->map_w[i] = reserve((size_t)kDlatent * kDlatent);
        for (size_t k = 0; k < (size_t)kDlatent * kDlatent; ++k) pool[e->map_w[i] + k] = src[k] * map_coef;
        src += (size_t)kDlatent * kDlatent;
        e->map_b[i] = reserve(kDlatent);
        for (int k = 0; k < kDlatent; ++k) pool[e->map_b[i] + k] = src[k] * kMappingLrmul;
        src += kDlatent;
    }
    e->avg_off = reserve(kDlatent);
    std::memcpy(&pool[e->avg_off], src, kDlatent * sizeof(float));
    src += kDlatent;
    e->const_off = reserve((size_t)nf(1) * act_plane(4));  // zero-bordered [512][6][12]
    for (int ch = 0; ch < nf(1); ++ch)
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 4; ++x)
                pool[e->const_off + (size_t)ch * act_plane(4) + (size_t)(y + 1) * 12 + x + 4] =
                    src[(size_t)ch * 16 + y * 4 + x];
    src += (size_t)nf(1) * 16;

    e->A_off = reserve((size_t)kDlatent * ctot);
    e->bias1_off = reserve(ctot);
    size_t w2_total = 0;
    for (const auto& c : e->convs) w2_total += (size_t)c.cin * c.cout;
    e->w2_off = reserve(w2_total + 32);  // (demod_kernel reads whole blocks of 32 columns: 16 past a 16-channel layer's)
    const float mod_coef = (float)(1.0 / std::sqrt((double)kDlatent));
    std::vector<gance::DemodLayer> demod_layers(nconv);
    // every form's weight image beyond the direct one, in the pool's order (enum WeightImage): its size and how it is arranged
    // from the scaled HWIO weights
    struct WeightImageKind {
        size_t (*floats)(int cin, int cout);
        void (*arrange)(const float* scaled, int cin, int cout, float* out);
    };
    static const WeightImageKind kinds[kNumWeightImages] = {
        {gance::winograd64_weight_floats, gance::winograd64_transform_weights},
        {gance::winograd43_weight_floats, gance::winograd43_transform_weights},
        {gance::upfir16_weight_floats, [](const float* w, int ci, int co, float* out) { gance::upfir16_arrange_weights(w, ci, co, kUpTapWeight, out); }},
        {gance::winogemm_weight_floats, gance::winogemm_arrange_weights},
        {gance::upgemm_weight_floats, [](const float* w, int ci, int co, float* out) { gance::upgemm_arrange_weights(w, ci, co, kUpTapWeight, out); }},
        {gance::upfirs_weight_floats, [](const float* w, int ci, int co, float* out) { gance::upfirs_arrange_weights(w, ci, co, kUpTapWeight, out); }},
        {gance::upfir16x_weight_floats, [](const float* w, int ci, int co, float* out) { gance::upfir16x_arrange_weights(w, ci, co, kUpTapWeight, out); }},
    };
    e->caps.resize(nconv);
    e->conv_bias.resize(nconv);
    e->conv_noise.resize(nconv);
    e->conv_ns.resize(nconv);
    size_t w2_cursor = 0;
    std::vector<float> scaled;
    for (int i = 0; i < nconv; ++i) {
        const ConvLayerHost& c = e->convs[i];
        const size_t wn = (size_t)9 * c.cin * c.cout;
        const float coef = (float)(1.0 / std::sqrt(9.0 * c.cin));
        scaled.resize(wn);  // the layer's scaled HWIO weights: what every form's image is arranged from
        for (size_t j = 0; j < wn; ++j) scaled[j] = src[j] * coef;
        LayerCaps& caps = e->caps[i] = layer_caps(e->convs, i, e->cfg.flags, e->tune);
        caps.direct_w = reserve(wn);
        {
            // the direct form's LDS image:
            // [m tile][K chunk][tap slot][KC][BM], slot t of an up layer = filter tap kUpTapWeight[t]
            const int BM = layer_bm(c.cout), KC = layer_kc(c.cout, c.up);
            const int m_tiles = c.cout / BM, chunks = c.cin / KC;
            float* w = &pool[caps.direct_w];
            float* w2 = &pool[e->w2_off + w2_cursor];
            for (int mt = 0; mt < m_tiles; ++mt)
                for (int ch = 0; ch < chunks; ++ch)
                    for (int t = 0; t < 9; ++t) {
                        const int tap = c.up ? kUpTapWeight[t] : t;
                        for (int kc = 0; kc < KC; ++kc)
                            for (int m = 0; m < BM; ++m) {
                                const int ci = ch * KC + kc, co = mt * BM + m;
                                const float v = scaled[((size_t)tap * c.cin + ci) * c.cout + co];
                                w[((((size_t)mt * chunks + ch) * 9 + t) * KC + kc) * BM + m] = v;
                                w2[(size_t)ci * c.cout + co] += v * v;
                            }
                    }
        }
        for (int f = 0; f < kNumWeightImages; ++f) {
            if (!caps.has[f]) continue;
            caps.w[f] = reserve(kinds[f].floats(c.cin, c.cout));
            kinds[f].arrange(scaled.data(), c.cin, c.cout, &pool[caps.w[f]]);
        }
        src += wn;
        demod_layers[i] = {(long long)w2_cursor, e->conv_s_off[i], e->conv_d_off[i], c.cin, c.cout};
        w2_cursor += (size_t)c.cin * c.cout;
        // mod_weight [512][cin] -> A[k][s_off + ci]
        for (int k = 0; k < kDlatent; ++k)
            for (int ci = 0; ci < c.cin; ++ci)
                pool[e->A_off + (size_t)k * ctot + e->conv_s_off[i] + ci] =
                    src[(size_t)k * c.cin + ci] * mod_coef;
        src += (size_t)kDlatent * c.cin;
        for (int ci = 0; ci < c.cin; ++ci)
            pool[e->bias1_off + e->conv_s_off[i] + ci] = src[ci] + 1.0f;
        src += c.cin;
        e->conv_ns[i] = src[0];
        src += 1;
        e->conv_bias[i] = reserve(c.cout);
        std::memcpy(&pool[e->conv_bias[i]], src, c.cout * sizeof(float));
        src += c.cout;
    }
    e->rgb_w.resize(nrgb);
    e->rgb_bias.resize(nrgb);
    for (int i = 0; i < nrgb; ++i) {
        const RgbLayerHost& r = e->rgbs[i];
        const float coef = (float)(1.0 / std::sqrt((double)r.cin));
        e->rgb_w[i] = reserve((size_t)r.cin * 3);
        for (int k = 0; k < r.cin * 3; ++k) pool[e->rgb_w[i] + k] = src[k] * coef;
        src += (size_t)r.cin * 3;
        for (int k = 0; k < kDlatent; ++k)
            for (int ci = 0; ci < r.cin; ++ci)
                pool[e->A_off + (size_t)k * ctot + e->rgb_s_off[i] + ci] =
                    src[(size_t)k * r.cin + ci] * mod_coef;
        src += (size_t)kDlatent * r.cin;
        for (int ci = 0; ci < r.cin; ++ci)
            pool[e->bias1_off + e->rgb_s_off[i] + ci] = src[ci] + 1.0f;
        src += r.cin;
        e->rgb_bias[i] = reserve(3);
        std::memcpy(&pool[e->rgb_bias[i]], src, 3 * sizeof(float));
        src += 3;
    }
    for (int i = 0; i < nconv; ++i) {
        const size_t n = (size_t)1 << (2 * e->convs[i].res_log2);
        e->conv_noise[i] = reserve(n);
        std::memcpy(&pool[e->conv_noise[i]], src, n * sizeof(float));
        src += n;
    }
    if ((uint64_t)(src - host_weights) != num_floats) {
        delete e;
        return fail(GANCE_ERR_BAD_WEIGHTS, "internal: blob walk does not match blob size");
    }

    // dlatent row of every 32-column style block
    std::vector<int> blk_row(ctot / 32);
    for (int i = 0; i < nconv; ++i)
        for (int cb = e->conv_s_off[i] / 32; cb < (e->conv_s_off[i] + round_up32(e->convs[i].cin)) / 32; ++cb)
            blk_row[cb] = e->convs[i].layer_idx;
    for (int i = 0; i < nrgb; ++i)
        for (int cb = e->rgb_s_off[i] / 32; cb < (e->rgb_s_off[i] + round_up32(e->rgbs[i].cin)) / 32; ++cb)
            blk_row[cb] = e->rgbs[i].row;

    // ---- workspace sizes ----
    const int Bmax = config->max_batch;
    e->t_units.assign(nconv, 0);
    size_t slab_max = 4;
    for (int i = 0; i < nconv; ++i) {
        const ConvLayerHost& c = e->convs[i];
        for (int B = 1; B <= Bmax; ++B) {
            const LayerPlan p = plan_layer(c, B);
            if (c.up) e->t_units[i] = std::max(e->t_units[i], p.nsplit * B);
            else if (p.nsplit > 1)
                slab_max = std::max(slab_max, (size_t)p.nsplit * B * c.cout << (2 * c.res_log2));
        }
    }
    e->slab_floats = slab_max;
    // the scatter-form up layers' GEMM buffers (whatever this engine's knobs say: the workspace is shared)
    for (int i = 0; i < nconv; ++i) {
        const ConvLayerHost& c = e->convs[i];
        const int H = (1 << c.res_log2) / 2;
        if (c.up && gance::upgemm_supported(c.cin, c.cout, H, H)) {
            const int samples = std::max(1, std::min(Bmax, gance::upgemm_max_columns(c.cout, e->tune.upgemm_buffer_columns) / (H * H)));
            e->up_packed_floats = std::max(e->up_packed_floats, gance::upgemm_packed_floats(samples, c.cin, H, H));
            e->up_prod_floats = std::max(e->up_prod_floats, gance::upgemm_prod_floats(samples, c.cout, H, H));
        }
        if (!c.up && i > 0 && gance::winogemm_supported(c.cin, c.cout, 2 * H, 2 * H)) {
            const int tiles = (H / 2) * (H / 2);  // 4x4 output tiles per sample
            const int samples = std::max(1, std::min(Bmax, gance::kWinoGemmMaxColumns / tiles));
            e->up_packed_floats = std::max(e->up_packed_floats, gance::winogemm_packed_floats(samples, c.cin, 2 * H, 2 * H));
            e->up_prod_floats = std::max(e->up_prod_floats, gance::winogemm_prod_floats(samples, c.cout, 2 * H, 2 * H));
        }
    }
    e->y_floats = (size_t)3 * config->resolution * config->resolution * Bmax;
    // partial ToRGB images of the Winograd conv launches whose pixels span several channel tiles: [Cout / 64][Bmax][3][R][R]
    for (int i = 0; i < nconv; ++i) {
        const ConvLayerHost& c = e->convs[i];
        if (!c.up && c.cout > 64 && gance::winograd64_rgb_supported(c.cout))
            e->rgb_part_floats = std::max(e->rgb_part_floats, (size_t)gance::winograd64_rgb_partials(c.cout) * Bmax * 3 << (2 * c.res_log2));
        // ... and of the F(4x4,3x3) launches: one partial image per block of 32 channels. Whatever THIS engine's flags say
        // about that form: the buffer belongs to the workspace, which every engine of the (device, resolution, max_batch)
        // shares -- an engine that never runs the form may be the one that allocates it for one that does.
        if (!c.up && i > 0 && e->convs[i - 1].up && (1 << c.res_log2) >= 32 &&
            gance::winograd43_supported(c.cin, c.cout, 1 << c.res_log2, 1 << c.res_log2) && gance::winograd43_rgb_supported(c.cout))
            e->rgb_part_floats = std::max(e->rgb_part_floats, (size_t)gance::winograd43_rgb_partials(c.cout) * Bmax * 3 << (2 * c.res_log2));
    }

#define GANCE_CREATE_CHECK(expr)                                                            \
    do {                                                                                    \
        hipError_t gance_err_ = (expr);                                                     \
        if (gance_err_ != hipSuccess) {                                                     \
            free_engine(e);                                                                 \
            return fail(gance_err_ == hipErrorOutOfMemory ? GANCE_ERR_OUT_OF_MEMORY         \
                                                          : GANCE_ERR_HIP,                  \
                        std::string(#expr) + ": " + hipGetErrorString(gance_err_));         \
        }                                                                                   \
    } while (0)

    e->pool_floats = pool.size();
    GANCE_CREATE_CHECK(hipMalloc((void**)&e->pool, pool.size() * sizeof(float)));
    GANCE_CREATE_CHECK(hipMemcpy(e->pool, pool.data(), pool.size() * sizeof(float), hipMemcpyHostToDevice));
    GANCE_CREATE_CHECK(hipMalloc((void**)&e->blk_row, blk_row.size() * sizeof(int)));
    GANCE_CREATE_CHECK(hipMemcpy(e->blk_row, blk_row.data(), blk_row.size() * sizeof(int), hipMemcpyHostToDevice));
    GANCE_CREATE_CHECK(hipMalloc((void**)&e->demod_layers, demod_layers.size() * sizeof(gance::DemodLayer)));
    GANCE_CREATE_CHECK(hipMemcpy(e->demod_layers, demod_layers.data(),
                                 demod_layers.size() * sizeof(gance::DemodLayer), hipMemcpyHostToDevice));
#undef GANCE_CREATE_CHECK
    if (int rc = acquire_workspace(e)) {
        const std::string message = g_last_error;
        free_engine(e);
        return fail(rc, message);
    }
    *out_engine = e;
    return GANCE_OK;
}

void gance_engine_destroy(gance_engine* engine) { free_engine(engine); }

int32_t gance_engine_vector_length(const gance_engine* engine) { return engine ? kDlatent : 0; }
int32_t gance_engine_num_layers(const gance_engine* engine) { return engine ? engine->num_rows : 0; }
int32_t gance_engine_resolution(const gance_engine* engine) { return engine ? engine->cfg.resolution : 0; }
int32_t gance_engine_max_batch(const gance_engine* engine) { return engine ? engine->cfg.max_batch : 0; }

int gance_synthesize_w(gance_engine* engine, const float* d_dlatents, int32_t batch,
                       uint8_t* d_out_u8, float* d_out_f32, void* stream) {
    if (int rc = check_call(engine, d_dlatents, batch)) return rc;
    gance::DeviceGuard guard(engine->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    // filtered profiling keeps its records across calls (bench.py averages them); else one call's worth
    if (engine->profile_only.empty() || engine->steps_used >= 4096) engine->steps_used = 0;
    WorkspaceTurn turn(engine->ws.get(), (hipStream_t)stream);
    return synthesize_from_dlat(engine, d_dlatents, batch, d_out_u8, d_out_f32, (hipStream_t)stream);
}

// The first `num_layers` dense layers of the mapping network (pixel-norm of z in the first), ping-ponging between the
// workspace's two buffers; *out is where the last of them wrote [batch][512]. The whole network for a call, fewer for the
// debug tap.
static int run_mapping(gance_engine* engine, const float* d_z, int32_t batch, int num_layers, hipStream_t stream, const float** out) {
    const float* in = d_z;
    float* bufs[2] = {engine->ws->map_a, engine->ws->map_b_buf};
    for (int i = 0; i < num_layers; ++i) {
        StepScope scope(engine, stream, "mapping_dense", 2.0 * batch * kDlatent * kDlatent,
                        4.0 * kDlatent * kDlatent);
        GANCE_HIP_CHECK(gance::launch_mapping_dense(in, engine->pool + engine->map_w[i],
                                                    engine->pool + engine->map_b[i], bufs[i & 1],
                                                    batch, i == 0, stream));
        in = bufs[i & 1];
    }
    *out = in;
    return GANCE_OK;
}

// mapping network + truncation into the workspace's dlatent buffer [batch][num_rows][512]
static int run_mapping_and_truncation(gance_engine* engine, const float* d_z, int32_t batch, float truncation_psi, hipStream_t stream) {
    const float* mapped = nullptr;
    if (int rc = run_mapping(engine, d_z, batch, kMappingLayers, stream, &mapped)) return rc;
    StepScope scope(engine, stream, "truncate", 0.0, 0.0);
    GANCE_HIP_CHECK(gance::launch_broadcast_truncate(mapped, engine->pool + engine->avg_off,
                                                     truncation_psi, engine->ws->dlat, batch,
                                                     engine->num_rows, stream));
    return GANCE_OK;
}

// mapping network + truncation + synthesis (no ordering against other users of the workspace: the callers do that)
static int synthesize_from_z(gance_engine* engine, const float* d_z, int32_t batch, float truncation_psi, uint8_t* d_out_u8,
                             float* d_out_f32, hipStream_t stream) {
    if (int rc = run_mapping_and_truncation(engine, d_z, batch, truncation_psi, stream)) return rc;
    return synthesize_from_dlat(engine, engine->ws->dlat, batch, d_out_u8, d_out_f32, stream);
}

int gance_synthesize_z(gance_engine* engine, const float* d_z, int32_t batch, float truncation_psi,
                       uint8_t* d_out_u8, float* d_out_f32, void* stream_) {
    if (int rc = check_call(engine, d_z, batch)) return rc;
    gance::DeviceGuard guard(engine->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    hipStream_t stream = (hipStream_t)stream_;
    // filtered profiling keeps its records across calls (bench.py averages them); else one call's worth
    if (engine->profile_only.empty() || engine->steps_used >= 4096) engine->steps_used = 0;
    WorkspaceTurn turn(engine->ws.get(), stream);
    return synthesize_from_z(engine, d_z, batch, truncation_psi, d_out_u8, d_out_f32, stream);
}

// The host-buffer entry (the reference's own call form: one frame per call, numpy in, numpy out,
// network_functions.py:289-301). Latency path: pinned staging buffers, a private stream, and the ~50-launch
// sequence of a (batch, entry, psi, outputs) combination captured ONCE into a hipGraph and replayed
// (the first call of a combination runs eagerly: it also performs the launchers' one-time attribute setup,
// which may not happen under capture). GANCE_TUNE_GRAPH=0 keeps every call eager.
static int host_call(gance_engine* e, const float* h_in, size_t in_floats, int batch, bool is_z,
                     float psi, uint8_t* h_u8, float* h_f32) {
    if (int rc = check_call(e, h_in, batch)) return rc;
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    gance_workspace* ws = e->ws.get();
    const size_t px = (size_t)e->cfg.resolution * e->cfg.resolution * 3;
    float* d_in = is_z ? ws->z_in : ws->dlat;
    if (ws->used) GANCE_HIP_CHECK(hipEventSynchronize(ws->last_use));  // another engine's call may still read the shared scratch
    hipStream_t hs = ws->host_stream;
    std::memcpy(ws->pinned_in, h_in, in_floats * sizeof(float));
    GANCE_HIP_CHECK(hipMemcpyAsync(d_in, ws->pinned_in, in_floats * sizeof(float), hipMemcpyHostToDevice, hs));
    e->keep_skip_image = h_f32 != nullptr;
    struct KeepSkipReset {  // every return path below leaves the flag cleared
        gance_engine* engine;
        ~KeepSkipReset() { engine->keep_skip_image = false; }
    } keep_skip_reset{e};
    auto run = [&]() {
        return is_z ? synthesize_from_z(e, d_in, batch, psi, ws->u8buf, nullptr, hs)
                    : synthesize_from_dlat(e, d_in, batch, ws->u8buf, nullptr, hs);
    };
    const bool plain = !e->tune.graph || (e->cfg.flags & GANCE_FLAG_PROFILE_STEPS) || e->debug_stop_after > 0;
    int rc = GANCE_OK;
    if (plain) {
        if (e->profile_only.empty() || e->steps_used >= 4096) e->steps_used = 0;
        rc = run();
    } else {
        unsigned psi_bits = 0;
        std::memcpy(&psi_bits, &psi, sizeof(psi_bits));
        const auto key = std::make_tuple(batch, is_z ? 1 : 0, is_z ? psi_bits : 0u, h_f32 != nullptr ? 1 : 0, e->noise_randomized ? 1 : 0);
        GraphEntry& entry = e->graphs[key];
        if (entry.disabled) {
            rc = run();
        } else if (entry.exec != nullptr) {
            GANCE_HIP_CHECK(hipGraphLaunch(entry.exec, hs));
        } else if (!entry.warmed) {
            rc = run();
            entry.warmed = true;
        } else {
            hipGraph_t graph = nullptr;
            GANCE_HIP_CHECK(hipStreamBeginCapture(hs, hipStreamCaptureModeThreadLocal));
            rc = run();
            const hipError_t end = hipStreamEndCapture(hs, &graph);
            if (rc == GANCE_OK && end == hipSuccess && hipGraphInstantiate(&entry.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                hipGraphDestroy(graph);
                GANCE_HIP_CHECK(hipGraphLaunch(entry.exec, hs));
            } else {
                // capture refused (it never should): eager launches for this combination from now on
                if (graph != nullptr) hipGraphDestroy(graph);
                (void)hipGetLastError();
                entry.exec = nullptr;
                entry.disabled = true;
                rc = run();
            }
        }
    }
    if (rc) return rc;
    if (!plain) e->last_rgb_y = nullptr;  // (a replayed graph's launches were recorded by another call)
    ws->front_owner = e;  // (a replayed graph does not pass through synthesize_from_dlat)
    ws->front_batch = batch;
    if (e->debug_stop_after > 0) {
        GANCE_HIP_CHECK(hipStreamSynchronize(hs));
        hipEventRecord(ws->last_use, hs);
        ws->used = true;
        return GANCE_OK;
    }
    if (h_u8) GANCE_HIP_CHECK(hipMemcpyAsync(ws->pinned_out, ws->u8buf, px * batch, hipMemcpyDeviceToHost, hs));
    hipEventRecord(ws->last_use, hs);
    ws->used = true;
    GANCE_HIP_CHECK(hipStreamSynchronize(hs));
    if (int rc_fault = check_call(e, h_in, batch)) return rc_fault;  // (a kernel of this very call may have raised the workspace's fault flag)
    if (h_u8) std::memcpy(h_u8, ws->pinned_out, px * batch);
    if (h_f32) {
        // the final skip image is in whichever ybuf the last ToRGB wrote
        const int n_rgb = (int)e->rgbs.size();
        const int ycur = (n_rgb - 1) & 1;
        GANCE_HIP_CHECK(hipMemcpy(h_f32, ws->ybuf[ycur], px * batch * sizeof(float), hipMemcpyDeviceToHost));
    }
    return GANCE_OK;
}

int gance_synthesize_w_host(gance_engine* engine, const float* h_dlatents, int32_t batch,
                            uint8_t* h_out_u8, float* h_out_f32) {
    if (engine == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    return host_call(engine, h_dlatents, (size_t)batch * engine->num_rows * kDlatent, batch, false,
                     0.f, h_out_u8, h_out_f32);
}

int gance_synthesize_z_host(gance_engine* engine, const float* h_z, int32_t batch,
                            float truncation_psi, uint8_t* h_out_u8, float* h_out_f32) {
    if (engine == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    return host_call(engine, h_z, (size_t)batch * kDlatent, batch, true, truncation_psi, h_out_u8,
                     h_out_f32);
}

int gance_engine_set_profiling(gance_engine* engine, int32_t flags, const char* only_step) {
    if (engine == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL engine");
    engine->cfg.flags = (engine->cfg.flags & ~GANCE_FLAG_PROFILE_STEPS) | (flags & GANCE_FLAG_PROFILE_STEPS);
    engine->profile_only = only_step ? only_step : "";
    engine->steps_used = 0;
    return GANCE_OK;
}

int32_t gance_engine_step_count(const gance_engine* engine) { return engine ? engine->steps_used : 0; }

int gance_engine_step_info(gance_engine* engine, int32_t index, char* name64, float* ms,
                           double* flops, double* bytes) {
    if (engine == nullptr || index < 0 || index >= engine->steps_used)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "step index out of range");
    StepRecord& r = engine->steps[index];
    GANCE_HIP_CHECK(hipEventSynchronize(r.stop));
    float elapsed = 0.f;
    GANCE_HIP_CHECK(hipEventElapsedTime(&elapsed, r.start, r.stop));
    if (name64) std::snprintf(name64, 64, "%s", r.name);
    if (ms) *ms = elapsed;
    if (flops) *flops = r.flops;
    if (bytes) *bytes = r.bytes;
    return GANCE_OK;
}

int gance_engine_randomize_noise(gance_engine* e, uint64_t seed, int32_t count, uint64_t first_sample, const int64_t* d_sample_ids, void* stream_) {
    if (e == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    if (count == 0) count = e->cfg.max_batch;
    if (count < 1 || count > e->cfg.max_batch)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "count " + std::to_string(count) + " outside [1, max_batch=" + std::to_string(e->cfg.max_batch) + "]");
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    hipStream_t stream = (hipStream_t)stream_;
    const int nconv = (int)e->convs.size();
    if (e->noise_rand_off.empty()) {  // planes for max_batch samples of every layer that reads noise (none at random init)
        size_t total = 0;
        e->noise_rand_off.assign(nconv, SIZE_MAX);
        for (int i = 0; i < nconv; ++i) {
            if (e->conv_ns[i] == 0.0f) continue;
            e->noise_rand_off[i] = total;
            total += ((size_t)e->cfg.max_batch << (2 * e->convs[i].res_log2));
        }
        if (total > 0) {
            const hipError_t err = hipMalloc((void**)&e->noise_rand, total * sizeof(float));
            if (err != hipSuccess) {
                e->noise_rand_off.clear();
                return fail(err == hipErrorOutOfMemory ? GANCE_ERR_OUT_OF_MEMORY : GANCE_ERR_HIP, std::string("noise planes: ") + hipGetErrorString(err));
            }
        }
    }
    // (the planes may still be read by a call in flight on another stream of the shared workspace: order behind it)
    if (e->ws && e->ws->used) GANCE_HIP_CHECK(hipStreamWaitEvent(stream, e->ws->last_use, 0));
    for (int i = 0; i < nconv; ++i) {
        if (e->noise_rand_off[i] == SIZE_MAX) continue;  // (a layer whose strength is zero never reads its noise)
        GANCE_HIP_CHECK(gance::launch_normal_noise(e->noise_rand + e->noise_rand_off[i], (size_t)1 << (2 * e->convs[i].res_log2), count, seed,
                                                   (unsigned long long)i, first_sample, (const long long*)d_sample_ids, stream));
    }
    e->noise_rand_count = count;
    e->noise_randomized = true;
    if (stream == nullptr) GANCE_HIP_CHECK(hipStreamSynchronize(nullptr));  // (the host-buffer entries run on a private stream)
    return GANCE_OK;
}

int gance_engine_restore_noise(gance_engine* e, void* stream_) {
    if (e == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    (void)stream_;  // (nothing to copy: the stored buffers were never overwritten, the launches go back to reading them)
    e->noise_randomized = false;
    return GANCE_OK;
}

int gance_engine_debug_read_noise(gance_engine* e, int32_t conv_layer, int32_t sample, float* h_out, uint64_t count) {
    if (e == nullptr || h_out == nullptr || conv_layer < 0 || conv_layer >= (int)e->convs.size() || sample < 0 || sample >= e->cfg.max_batch)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "bad argument to gance_engine_debug_read_noise");
    const uint64_t n = (uint64_t)1 << (2 * e->convs[conv_layer].res_log2);
    if (count != n) return fail(GANCE_ERR_INVALID_ARGUMENT, "the layer's noise buffer holds " + std::to_string(n) + " floats");
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    GANCE_HIP_CHECK(hipDeviceSynchronize());
    int b_stride = 0;
    const float* src = layer_noise(e, conv_layer, &b_stride);
    if (src == nullptr) src = e->pool + e->conv_noise[conv_layer];  // (strength zero: the stored buffer, which no launch reads)
    GANCE_HIP_CHECK(hipMemcpy(h_out, src + (size_t)sample * b_stride, n * sizeof(float), hipMemcpyDeviceToHost));
    return GANCE_OK;
}

// The plan of a full call without a device: capabilities from the config alone (layer_caps needs no weights), the same
// plan_call and the same names (name_step) as synthesize_from_dlat.
int gance_engine_describe_plan(const gance_engine_config* config, int32_t num_cus, int32_t batch, char* out, uint64_t capacity) {
    if (config == nullptr || out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument to gance_engine_describe_plan");
    const int res_log2 = ilog2_exact(config->resolution);
    if (res_log2 < 3 || res_log2 > 10 || config->max_batch < 1 || config->max_batch > 64 || batch < 1 || batch > config->max_batch || num_cus < 1)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_describe_plan: resolution, max_batch, batch or num_cus out of range");
    std::vector<ConvLayerHost> convs;
    std::vector<RgbLayerHost> rgbs;
    build_spec(res_log2, fmap_base_of_flags(config->flags), &convs, &rgbs);
    const Tuning tune = engine_tuning();
    std::vector<LayerCaps> caps;
    for (int i = 0; i < (int)convs.size(); ++i) caps.push_back(layer_caps(convs, i, config->flags, tune));
    std::string text = "styles\ndemod\n";
    for (const LayerStep& step : plan_call(convs, caps, tune, config->flags, num_cus, batch, 0))
        for (const char* name : {step.name, step.second, step.torgb})
            if (name[0] != '\0') text += std::string(name) + "\n";
    if (text.size() + 1 > capacity) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_describe_plan: capacity too small");
    std::memcpy(out, text.c_str(), text.size() + 1);
    return GANCE_OK;
}

int gance_engine_debug_stop_after(gance_engine* engine, int32_t num_conv_layers) {
    if (engine == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "engine is NULL");
    engine->debug_stop_after = num_conv_layers;
    return GANCE_OK;
}

int gance_engine_debug_read_activation(gance_engine* engine, int32_t batch, float* h_out,
                                       uint64_t max_floats, int32_t* out_channels,
                                       int32_t* out_side) {
    if (engine == nullptr || h_out == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument");
    gance::DeviceGuard guard(engine->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    const int C = engine->last_act_c, R = engine->last_act_side;
    const size_t n = (size_t)batch * C * R * R;
    if (n == 0 || n > max_floats) return fail(GANCE_ERR_INVALID_ARGUMENT, "activation does not fit");
    GANCE_HIP_CHECK(hipDeviceSynchronize());
    const size_t padded = (size_t)batch * C * act_plane(R);
    std::vector<float> tmp(padded);
    GANCE_HIP_CHECK(hipMemcpy(tmp.data(), engine->ws->act[engine->last_act_layer], padded * sizeof(float),
                              hipMemcpyDeviceToHost));
    for (size_t bc = 0; bc < (size_t)batch * C; ++bc)
        for (int y = 0; y < R; ++y)
            std::memcpy(h_out + (bc * R + y) * R, &tmp[bc * act_plane(R) + (size_t)(y + 1) * (R + 8) + 4],
                        R * sizeof(float));
    if (out_channels) *out_channels = C;
    if (out_side) *out_side = R;
    return GANCE_OK;
}

int gance_engine_debug_read_skip_image(gance_engine* engine, int32_t batch, float* h_out, uint64_t max_floats, int32_t* out_side) {
    if (engine == nullptr || h_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "NULL argument");
    if (engine->last_rgb_y == nullptr)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_skip_image: the engine's last call stored no fp32 skip image");
    if (batch != engine->last_rgb_batch)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_skip_image: the engine's last call had " +
                                                    std::to_string(engine->last_rgb_batch) + " frames, not " + std::to_string(batch));
    gance::DeviceGuard guard(engine->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    const int R = engine->last_rgb_side;
    const size_t n = (size_t)batch * 3 * R * R;
    if (n == 0 || n > max_floats) return fail(GANCE_ERR_INVALID_ARGUMENT, "skip image does not fit");
    GANCE_HIP_CHECK(hipDeviceSynchronize());
    GANCE_HIP_CHECK(hipMemcpy(h_out, engine->last_rgb_y, n * sizeof(float), hipMemcpyDeviceToHost));
    if (out_side) *out_side = R;
    return GANCE_OK;
}

// The front end of a z call alone, eagerly on the workspace's host stream: z from host memory, the first `num_dense_layers`
// mapping layers (run_mapping, the call's own loop) or, with `truncate`, all of them and the truncation; then the result,
// [batch][512] or [batch][num_rows][512], to host memory. Ordered against the other users of the shared workspace as host_call is.
static int debug_front_end_of_z(gance_engine* e, const float* h_z, int batch, int num_dense_layers, bool truncate, float psi,
                                float* h_out, uint64_t max_floats, const char* who) {
    if (h_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": output pointer is NULL");
    if (int rc = check_call(e, h_z, batch)) return rc;
    if (num_dense_layers < 1 || num_dense_layers > kMappingLayers)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": the mapping network has " + std::to_string(kMappingLayers) +
                                                    " dense layers, asked for " + std::to_string(num_dense_layers));
    const size_t n = (size_t)batch * (truncate ? e->num_rows : 1) * kDlatent;
    if (n > max_floats)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": the result holds " + std::to_string(n) + " floats, the buffer " + std::to_string(max_floats));
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    gance_workspace* ws = e->ws.get();
    if (ws->used) GANCE_HIP_CHECK(hipEventSynchronize(ws->last_use));  // another engine's call may still read the shared scratch
    hipStream_t hs = ws->host_stream;
    const size_t in_floats = (size_t)batch * kDlatent;
    std::memcpy(ws->pinned_in, h_z, in_floats * sizeof(float));
    GANCE_HIP_CHECK(hipMemcpyAsync(ws->z_in, ws->pinned_in, in_floats * sizeof(float), hipMemcpyHostToDevice, hs));
    if (e->profile_only.empty() || e->steps_used >= 4096) e->steps_used = 0;
    const float* result = ws->dlat;
    const int rc = truncate ? run_mapping_and_truncation(e, ws->z_in, batch, psi, hs) : run_mapping(e, ws->z_in, batch, num_dense_layers, hs, &result);
    hipEventRecord(ws->last_use, hs);
    ws->used = true;
    if (rc) return rc;
    GANCE_HIP_CHECK(hipStreamSynchronize(hs));
    GANCE_HIP_CHECK(hipMemcpy(h_out, result, n * sizeof(float), hipMemcpyDeviceToHost));
    return GANCE_OK;
}

int gance_engine_debug_mapping(gance_engine* engine, const float* h_z, int32_t batch, int32_t num_dense_layers, float* h_out,
                               uint64_t max_floats) {
    return debug_front_end_of_z(engine, h_z, batch, num_dense_layers, false, 0.f, h_out, max_floats, "gance_engine_debug_mapping");
}

int gance_engine_debug_dlatents(gance_engine* engine, const float* h_z, int32_t batch, float truncation_psi, float* h_out,
                                uint64_t max_floats) {
    return debug_front_end_of_z(engine, h_z, batch, kMappingLayers, true, truncation_psi, h_out, max_floats, "gance_engine_debug_dlatents");
}

// `width` columns from `column` on of the rows [batch][row_floats] that the engine's last w-call left at `d_rows`
static int debug_read_front_columns(gance_engine* e, const float* d_rows, int row_floats, int column, int width, int batch, float* h_out,
                                    uint64_t max_floats, const char* who) {
    const gance_workspace* ws = e->ws.get();
    if (ws->front_owner != e || ws->front_batch < 1)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": the workspace's last call was not this engine's");
    if (batch != ws->front_batch)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": the engine's last call had " + std::to_string(ws->front_batch) +
                                                    " samples, not " + std::to_string(batch));
    const size_t n = (size_t)batch * width;
    if (n > max_floats)
        return fail(GANCE_ERR_INVALID_ARGUMENT, std::string(who) + ": the result holds " + std::to_string(n) + " floats, the buffer " + std::to_string(max_floats));
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    GANCE_HIP_CHECK(hipDeviceSynchronize());
    GANCE_HIP_CHECK(hipMemcpy2D(h_out, (size_t)width * sizeof(float), d_rows + column, (size_t)row_floats * sizeof(float),
                                (size_t)width * sizeof(float), (size_t)batch, hipMemcpyDeviceToHost));
    return GANCE_OK;
}

int gance_engine_debug_read_style(gance_engine* e, int32_t kind, int32_t index, int32_t batch, float* h_out, uint64_t max_floats) {
    if (e == nullptr || h_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_style: NULL argument");
    if (kind != 0 && kind != 1) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_style: kind is 0 (a conv layer) or 1 (a ToRGB)");
    const int count = kind == 0 ? (int)e->convs.size() : (int)e->rgbs.size();
    if (index < 0 || index >= count)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_style: layer " + std::to_string(index) + " outside [0, " + std::to_string(count) + ")");
    const int column = kind == 0 ? e->conv_s_off[index] : e->rgb_s_off[index];
    const int width = kind == 0 ? e->convs[index].cin : e->rgbs[index].cin;
    return debug_read_front_columns(e, e->ws->styles, e->ctot, column, width, batch, h_out, max_floats, "gance_engine_debug_read_style");
}

int gance_engine_debug_read_demod(gance_engine* e, int32_t conv_layer, int32_t batch, float* h_out, uint64_t max_floats) {
    if (e == nullptr || h_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_demod: NULL argument");
    if (conv_layer < 0 || conv_layer >= (int)e->convs.size())
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_read_demod: layer " + std::to_string(conv_layer) + " outside [0, " +
                                                    std::to_string(e->convs.size()) + ")");
    return debug_read_front_columns(e, e->ws->demod, e->dtot, e->conv_d_off[conv_layer], e->convs[conv_layer].cout, batch, h_out, max_floats,
                                    "gance_engine_debug_read_demod");
}

// The two buffers of conv layer li as the border taps see them: its activation planes [max_batch][cout] of [res+2][res+8], and
// for an up layer the parity planes [4 classes][t_units][cout] of [H+3][W+8] (base nullptr: a stride-1 layer has none).
static gance::BorderPlanes act_border_planes(const gance_engine* e, int li) {
    const ConvLayerHost& c = e->convs[li];
    const int res = 1 << c.res_log2;
    const unsigned long long planes = (unsigned long long)e->ws->max_batch * c.cout;
    return {e->ws->act[li], planes, planes, res + 2, res + 8, res, res};
}
static gance::BorderPlanes parity_border_planes(const gance_engine* e, int li) {
    const ConvLayerHost& c = e->convs[li];
    const int H = (1 << c.res_log2) / 2;
    const unsigned long long per_class = (unsigned long long)e->t_units[li] * c.cout;
    return {e->ws->tplanes[li], 4 * per_class, per_class, H + 3, H + 8, H + 1, H + 1};
}

int gance_engine_debug_border_residue(gance_engine* e, uint64_t* h_out, uint64_t count) {
    if (e == nullptr || h_out == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_border_residue: NULL argument");
    const int nconv = (int)e->convs.size();
    if (count != (uint64_t)6 * nconv)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_border_residue: six words for each of " + std::to_string(nconv) + " conv layers, not " +
                                                    std::to_string(count));
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    gance_workspace* ws = e->ws.get();
    if (ws->used) GANCE_HIP_CHECK(hipEventSynchronize(ws->last_use));
    hipStream_t hs = ws->host_stream;
    unsigned long long* d_counts = nullptr;  // [layer][act, parity planes][nonzero, scanned]
    const size_t bytes = (size_t)nconv * 4 * sizeof(unsigned long long);
    GANCE_HIP_CHECK(hipMalloc((void**)&d_counts, bytes));
    std::vector<unsigned long long> counts((size_t)nconv * 4, 0);
    hipError_t err = hipMemsetAsync(d_counts, 0, bytes, hs);
    for (int li = 0; li < nconv && err == hipSuccess; ++li) {
        err = gance::launch_border_residue(act_border_planes(e, li), d_counts + 4 * li, hs);
        if (err == hipSuccess && ws->tplanes[li] != nullptr) err = gance::launch_border_residue(parity_border_planes(e, li), d_counts + 4 * li + 2, hs);
    }
    if (err == hipSuccess) err = hipMemcpyAsync(counts.data(), d_counts, bytes, hipMemcpyDeviceToHost, hs);
    if (err == hipSuccess) err = hipStreamSynchronize(hs);
    (void)hipFree(d_counts);
    GANCE_HIP_CHECK(err);
    for (int li = 0; li < nconv; ++li) {
        const bool up = ws->tplanes[li] != nullptr;
        h_out[6 * li + 0] = counts[4 * li + 0];
        h_out[6 * li + 1] = counts[4 * li + 1];
        h_out[6 * li + 2] = act_border_planes(e, li).planes;
        h_out[6 * li + 3] = counts[4 * li + 2];
        h_out[6 * li + 4] = counts[4 * li + 3];
        h_out[6 * li + 5] = up ? parity_border_planes(e, li).planes : 0;
    }
    return GANCE_OK;
}

int gance_engine_debug_poison_scratch(gance_engine* e, float value, int32_t include_borders) {
    if (e == nullptr) return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_poison_scratch: engine is NULL");
    if (include_borders != 0 && !(e->cfg.flags & GANCE_FLAG_PRIVATE_WORKSPACE))
        return fail(GANCE_ERR_INVALID_ARGUMENT, "gance_engine_debug_poison_scratch: the borders of a shared workspace are every engine's: "
                                                "include_borders needs an engine created with GANCE_FLAG_PRIVATE_WORKSPACE");
    gance::DeviceGuard guard(e->cfg.device);
    GANCE_HIP_CHECK(guard.status());
    gance_workspace* ws = e->ws.get();
    if (ws->used) GANCE_HIP_CHECK(hipEventSynchronize(ws->last_use));
    hipStream_t hs = ws->host_stream;
    int bits = 0;
    std::memcpy(&bits, &value, sizeof(bits));
    for (int li = 0; li < (int)e->convs.size(); ++li) {
        GANCE_HIP_CHECK(gance::launch_poison_planes(act_border_planes(e, li), value, include_borders, hs));
        if (ws->tplanes[li] != nullptr) GANCE_HIP_CHECK(gance::launch_poison_planes(parity_border_planes(e, li), value, include_borders, hs));
    }
    for (const auto& buffer : ws->dense) GANCE_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)buffer.first, bits, buffer.second, hs));
    GANCE_HIP_CHECK(hipMemsetAsync(ws->u8buf, 0xA5, ws->u8_bytes, hs));
    ws->front_owner = nullptr;  // nobody's styles, nobody's skip image
    ws->front_batch = 0;
    e->last_rgb_y = nullptr;
    hipEventRecord(ws->last_use, hs);
    ws->used = true;
    GANCE_HIP_CHECK(hipStreamSynchronize(hs));
    return GANCE_OK;
}

int gance_resize_bicubic_u8(const uint8_t* d_in, int32_t batch, int32_t src_side, uint8_t* d_out,
                            int32_t dst_side, void* stream) {
    if (d_in == nullptr || d_out == nullptr || batch < 1 || src_side < 1 || dst_side < 1)
        return fail(GANCE_ERR_INVALID_ARGUMENT, "bad argument to gance_resize_bicubic_u8");
    gance::DeviceGuard guard(gance::device_of_pointer(d_in));  // launch where the frames live
    GANCE_HIP_CHECK(guard.status());
    GANCE_HIP_CHECK(gance::launch_resize_bicubic_u8(d_in, batch, src_side, d_out, dst_side, (hipStream_t)stream));
    return GANCE_OK;
}

}  // extern "C"
