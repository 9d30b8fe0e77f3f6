// The engine's host-side decisions, split from engine.hip (its only includer) so that they read in one piece: the tuning
// record, what an engine may run each layer in (LayerCaps), and plan_call, which turns (capabilities, tuning, flags, CUs, batch)
// into one record per conv layer. Nothing here makes a HIP call, and only read_tuning() looks at the environment.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace {

struct ConvLayerHost {
    int layer_idx, res_log2, cin, cout;
    bool up;
};

// One launch of the conv kernel: a stride-1 conv, or a transposed conv with its four parity classes
// fused. Wide transposed convs (BM = 128) tile the H x W position grid exactly with 8x8 tiles and
// cover the extra position row y' = H / column x' = W with 1x64 / 64x1 strip tiles in the SAME
// launch (runtime tile geometry); the narrow ones tile the (H+1) x (W+1) grid directly.
struct LayerPlan {
    int tile_id;
    int OH, OW;  // output bound for masking: H x W, or (H+1) x (W+1) positions when up
    int tiles_x, tiles_y, tiles_b, row_tiles, col_tiles;
    int m_tiles, nsplit, chunks_per_split, total_chunks, total_blocks;
};

int ceil_div(int a, int b) { return (a + b - 1) / b; }

int layer_bm(int cout) { return cout == 16 ? 16 : (cout == 32 ? 32 : (cout == 64 ? 64 : 128)); }  // (16: conv16_mfma.hip, config-e at 1024^2)

// Every GANCE_TUNE_* value the library reads: read_tuning() is the only place in csrc/ that looks at the environment. All fields
// are read ONCE PER PROCESS (several size the workspace, which engines share) except `engine`, read each time an engine is created
// (tests set those between engines of one process).
struct Tuning {
    // GANCE_TUNE_UPFIR16X = 0: the fused up layers whose input the 64-column strips tile stay in direct form; 1 (default): they run in
    // the pair form (F(2,2) along x) when their input arrives pre-scaled.
    int upfir16x = 1;
    // GANCE_TUNE_UPGEMM: the two smallest up layers (4x4 -> 8x8, 8x8 -> 16x16) run in scatter form (gemm_forms.hip: one dense GEMM, no
    // position grid to tile) when a call has at least this many GEMM columns (samples x input positions); 0 = never. Default 128 (one
    // column tile): from 2 samples at 8x8, 8 at 4x4. Measured (tools/gpu_gemm_threshold_sweep.sh, frames/s at 4 ... 32 frames per call):
    // every threshold from 32 to 128 within 0.3 %, 256 / 512 -0.5 ... -1.5 %, 1 (always) -2 % at one frame per call.
    int upgemm_min_columns = 128;
    // GANCE_TUNE_UPGEMM_COLUMNS: the scatter form's product buffer, in GEMM columns of a 512-channel layer (75 MB per 4096; at least
    // 4096). Default 16384 (302 MB): every up layer from 4 -> 8 to 128 -> 256 of a call of up to 4 ... 8 frames fits, i.e. up to where the
    // fused up kernel takes over (tools/gpu_upgemm_cap_sweep.sh: +2 ... 4 % frames/s at 2 ... 7 frames per call against 4096).
    int upgemm_buffer_columns = 16384;
    // GANCE_TUNE_WINOGEMM: the stride-1 layers at 8x8 and 16x16 run in Winograd F(4x4,3x3) GEMM form (gemm_forms.hip) when a call has at
    // least this many GEMM columns (samples x 4x4 output tiles); 0 = never. Default 64: from 4 samples at 16x16, 16 at 8x8 (the same
    // sweep). Like every Winograd form it is off in engines created with conv_form "direct" (or "winograd": F(2x2,3x3) only).
    int winogemm_min_columns = 64;
    int wino43 = -1;  // GANCE_TUNE_WINO43: overrides the default F(4x4,3x3) resolution limit (wino43_max_res): 0 = off, else a resolution
    // GANCE_TUNE_PRESCALE_UP = 0: a Winograd launch never scales its stores by the next (fused up) layer's style; that kernel then
    // scales in its own K loop
    bool prescale_up = true;
    bool w64_rgb = true;  // GANCE_TUNE_W64_RGB = 0: no ToRGB channel sum in the epilogue of the 16x16x4 Winograd / F(4x4,3x3) launches
    // GANCE_TUNE_W43_ROUNDS: blocks per CU of the F(4x4,3x3) launches (ConvArgs::grid_rounds). Four: measured as fast as one persistent
    // block per CU (1234 ... 1236 frames/s with 2 / 4 / 8 / 16 against 1228 with 1: the prologue of a block is a few k-steps of
    // thousands), and a CU that something else holds for a while -- the RCCL copy kernels of the frame gather on a multi-GPU job --
    // then delays a quarter of its share instead of the tail of the launch. 1: one block per CU.
    int w43_rounds = 4;
    bool graph = true;  // GANCE_TUNE_GRAPH = 0 keeps every host-buffer call eager (host_call)
    struct PerEngine {
        int upfir_split = 1;  // GANCE_TUNE_UPFIR_SPLIT: 0 never, 1 (default) where a launch fills the chip without row segments, 2 wherever supported
        int upfir_split_narrow = 1;  // GANCE_TUNE_UPFIR_SPLIT_NARROW: the split form's narrow geometries (inputs 32 and 16 wide) in mode 1 and 2 by the fill rule; 0 never
    } engine;
};

Tuning read_tuning() {
    Tuning t;
    const auto number = [](const char* name, int unset) { const char* v = std::getenv(name); return v ? std::atoi(v) : unset; };
    t.upfir16x = number("GANCE_TUNE_UPFIR16X", 1);
    t.upgemm_min_columns = number("GANCE_TUNE_UPGEMM", 128);
    t.upgemm_buffer_columns = std::max(4096, number("GANCE_TUNE_UPGEMM_COLUMNS", 16384));
    t.winogemm_min_columns = number("GANCE_TUNE_WINOGEMM", 64);
    t.wino43 = number("GANCE_TUNE_WINO43", -1);
    t.prescale_up = number("GANCE_TUNE_PRESCALE_UP", 1) != 0;
    t.w64_rgb = number("GANCE_TUNE_W64_RGB", 1) != 0;
    const int rounds = number("GANCE_TUNE_W43_ROUNDS", 0);
    t.w43_rounds = rounds > 0 ? rounds : 4;
    t.graph = number("GANCE_TUNE_GRAPH", 1) != 0;
    t.engine.upfir_split = std::max(0, std::min(2, number("GANCE_TUNE_UPFIR_SPLIT", 1)));
    t.engine.upfir_split_narrow = number("GANCE_TUNE_UPFIR_SPLIT_NARROW", 1) == 0 ? 0 : 1;
    return t;
}
const Tuning& process_tuning() {
    static const Tuning tuning = read_tuning();
    return tuning;
}
Tuning engine_tuning() {  // the process's values, with the per-engine ones as the environment has them now
    Tuning t = process_tuning();
    t.engine = read_tuning().engine;
    return t;
}

// K chunk (input channels per LDS stage) of the direct form's tiles: 16 in the 16-channel tiles, 8 in the narrow transposed convs
// (Cout 32 / 64), 4 everywhere else
int layer_kc(int cout, bool up) { return layer_bm(cout) == 16 ? 16 : (up && layer_bm(cout) != 128 ? 8 : 4); }

// The direct form's tile (gance::kConvTiles) of a layer
int choose_tile(int cout, bool up, int OH, int OW, int B) {
    if (cout == 16) return up ? 10 : 9;  // config-e: 512 -> 1024 / the 1024^2 layers (conv16_mfma.hip)
    if (cout == 32) return up ? 6 : 4;  // config-f: 512 -> 1024 / the 1024^2 layers; config-e: the same at half the side
    if (cout == 64) return up ? 7 : 5;  // 256 -> 512 / the 512^2 layers
    if (up) return 8;                   // every up layer with Cout >= 128: runtime geometry
    // the stride-1 layers with Cout >= 128 (4^2 ... 256^2): the tile that covers the grid and the samples in the fewest blocks
    const int first = 0, last = 3;
    int best = first;
    long best_tiles = -1;
    for (int id = first; id <= last; ++id) {
        const auto& t = gance::kConvTiles[id];
        const long tiles = (long)ceil_div(B, t.TB) * ceil_div(OH, t.TH) * ceil_div(OW, t.TW);
        if (best_tiles < 0 || tiles < best_tiles) {
            best_tiles = tiles;
            best = id;
        }
    }
    return best;
}

int choose_nsplit(int base_blocks, int chunks) {
    if (base_blocks >= 384) return 1;
    const int want = ceil_div(768, base_blocks);
    for (int d = 1; d <= chunks; ++d)
        if (chunks % d == 0 && d >= want) return d;
    return chunks;
}

// Smallest input side whose wide transposed conv takes the strip tiles. Strips pay once the position grid has several tiles per
// side; below that the launch is latency-bound and extra blocks only hurt
constexpr int kStripsMinSide = 16;

LayerPlan plan_layer(const ConvLayerHost& c, int B) {
    LayerPlan p{};
    const int res = 1 << c.res_log2;
    const bool strips = c.up && layer_bm(c.cout) == 128 && res / 2 >= kStripsMinSide;
    const int grid = c.up ? (strips ? res / 2 : res / 2 + 1) : res;  // the tiled grid
    p.OH = p.OW = c.up ? res / 2 + 1 : res;
    p.tile_id = choose_tile(c.cout, c.up, grid, grid, B);
    const auto& t = gance::kConvTiles[p.tile_id];
    p.tiles_x = ceil_div(grid, t.TW);
    p.tiles_y = ceil_div(grid, t.TH);
    p.tiles_b = ceil_div(B, t.TB);
    p.row_tiles = strips ? ceil_div(res / 2 + 1, 64) : 0;
    p.col_tiles = strips ? ceil_div(res / 2, 64) : 0;
    p.m_tiles = c.cout / t.BM;
    p.total_chunks = c.cin / t.KC;
    const int base = p.m_tiles * (p.tiles_x * p.tiles_y + p.row_tiles + p.col_tiles) * p.tiles_b;
    p.nsplit = layer_bm(c.cout) == 16 ? 1 : choose_nsplit(base, p.total_chunks);  // (the 16-channel tiles have no split-K; their layers are 1024 wide)
    if (c.up) p.nsplit = std::min(p.nsplit, 8);  // the FIR pass re-reads every slab
    while (p.total_chunks % p.nsplit) --p.nsplit;
    p.chunks_per_split = p.total_chunks / p.nsplit;
    p.total_blocks = base * p.nsplit;
    return p;
}

constexpr int kWino43DefaultMaxRes = 1024;  // every Conv1 from 32x32 up (measured faster than the F(2x2,3x3) kernels on all six: DESIGN.md §3)

// Largest resolution whose Conv1 runs in Winograd F(4x4, 3x3) form (winograd43_conv.hip) in an engine with these
// flags: GANCE_FLAG_WINOGRAD43 = every resolution the kernel supports; otherwise the default limit, which
// Tuning::wino43 overrides.
int wino43_max_res(int flags, const Tuning& tune) {
    if (flags & GANCE_FLAG_DIRECT_CONV) return 0;
    if (flags & GANCE_FLAG_WINOGRAD43) return 1 << 20;
    if (flags & GANCE_FLAG_FORCE_WINOGRAD) return 0;  // FORCE_WINOGRAD alone = the F(2x2,3x3) kernels on every layer (parity tests of that form)
    return tune.wino43 >= 0 ? tune.wino43 : kWino43DefaultMaxRes;
}

// ---- what an engine may run a layer in: decided once, at creation, from (layer spec, engine flags, tuning) ----
// The forms beyond the direct one (conv_mfma.hip, which every layer has); each reads a weight image of its own. In the pool's order.
enum WeightImage {
    kWino64,      // Winograd F(2x2,3x3) on 16x16x4 MFMAs (winograd64_conv.hip: layers with >= 64 output channels, and the 32-channel last layer)
    kWino43,      // Winograd F(4x4,3x3) (winograd43_conv.hip)
    kUpfir16,     // fused transposed conv + FIR on the fp32 matrix cores, 16 channels per block, two blocks per CU (upfir16_fused.hip)
    kWinoGemm,    // Winograd F(4x4,3x3) as 36 dense GEMMs, the stride-1 layers at 8x8 ... 128x128 (gemm_forms.hip)
    kUpGemm,      // scatter-form GEMM of the small up layers (gemm_forms.hip)
    kUpfirSplit,  // split-operand form of the fused up kernel (upfir_split.hip: three bf16 parts per value, six terms, fp32 accumulation)
    kUpfir16x,    // the 16-channel geometry's pair form (F(2,2) along x: 15 MFMAs per pair of columns instead of 18)
    kNumWeightImages
};
struct LayerCaps {
    bool has[kNumWeightImages] = {};  // this engine may run the layer in that form ...
    size_t w[kNumWeightImages] = {};  // ... from the image at this pool offset
    size_t direct_w = 0;              // the direct form's image
};

LayerCaps layer_caps(const std::vector<ConvLayerHost>& convs, int i, int flags, const Tuning& tune) {
    const ConvLayerHost& c = convs[i];
    const int res = 1 << c.res_log2, H = res / 2;
    LayerCaps k;
    if (!c.up) {
        const bool after_up = i > 0 && convs[i - 1].up;
        k.has[kWino64] = gance::winograd64_supported(c.cin, c.cout, res, res);
        k.has[kWino43] = after_up && res >= 32 && res <= wino43_max_res(flags, tune) && gance::winograd43_supported(c.cin, c.cout, res, res);
        k.has[kWinoGemm] = i > 0 && tune.winogemm_min_columns > 0 && wino43_max_res(flags, tune) >= 16 && gance::winogemm_supported(c.cin, c.cout, res, res);
    } else {
        k.has[kUpfir16] = gance::upfir16_supported(c.cin, c.cout, H, H);
        k.has[kUpGemm] = tune.upgemm_min_columns > 0 && gance::upgemm_supported(c.cin, c.cout, H, H);
        // (the split-operand and pair forms keep to the channel tables they were measured on: a 16-channel layer -- config-e,
        // 512 -> 1024 -- has the fp32 form, 16 channels per block, as its one fused form)
        k.has[kUpfirSplit] = tune.engine.upfir_split != 0 && c.cout >= 32 &&
                             (gance::upfirs_supported(c.cin, c.cout, H, H) || (tune.engine.upfir_split_narrow != 0 && gance::upfirs_narrow_supported(c.cin, c.cout, H, H)));
        k.has[kUpfir16x] = tune.upfir16x != 0 && c.cout >= 32 && gance::upfir16x_supported(c.cin, c.cout, H, H);
    }
    return k;
}

// ---- the plan of one call: which kernel runs which layer, and what the neighbours owe each other ----
enum class Form {
    Direct,        // conv_mfma.hip, one launch
    DirectSplitK,  // ... split-K into slabs + the finish pass
    DirectTorgb,   // ... the last layer with its whole ToRGB (and the uint8 conversion) in the epilogue
    Wino64, Wino43, WinoGemm,  // the stride-1 forms of WeightImage
    UpTwoPass,     // conv_mfma.hip's transposed conv into parity planes + the FIR pass
    UpGemm,        // scatter-form GEMM + the FIR pass
    UpFused16, UpFused16x, UpSplit  // one fused launch: kUpfir16, kUpfir16x, kUpfirSplit
};
bool is_fused_up(Form f) { return f == Form::UpFused16 || f == Form::UpFused16x || f == Form::UpSplit; }

struct LayerStep {
    Form form = Form::Direct;
    LayerPlan p{};          // the direct form's geometry (its split-K factor also sizes the FIR pass)
    gance::UpFirArgs up{};  // the fused up forms' geometry (pointers unset)
    bool rgb_sum = false;   // the conv launch also does the channel sum of the layer's ToRGB ...
    int rgb_partials = 1;   // ... in this many partial images (one per channel tile of a pixel)
    bool stores_activation = true;  // false: the last layer's activation has no reader (its launch did the ToRGB sum, no debug tap)
    bool scales_stores = false;     // the next layer's style rides on this layer's stores
    bool input_prescaled = false;   // (up layers) the input arrives multiplied by this layer's style
    bool last_of_all = false;  // the network's last layer in a call that runs every layer ...
    bool may_skip_y_store = false;  // ... whose ToRGB pass need not store the fp32 image when the caller wants bytes only
    char name[64] = "", second[64] = "", torgb[64] = "";  // launch names: the conv, its finish / fir pass, its ToRGB pass ("" = no such launch)
};

struct PlanContext {
    const std::vector<ConvLayerHost>& convs;
    const std::vector<LayerCaps>& caps;
    const Tuning& tune;
    int flags, num_cus, B, stop_after;  // stop_after > 0: a debug call that runs only that many conv layers
    int num_convs() const { return (int)convs.size(); }
    int limit() const { return stop_after > 0 ? std::min(stop_after, num_convs()) : num_convs(); }
};

// Which form conv layer idx (a stride-1 conv, direct-form geometry p) runs in for this batch. The layer BEFORE a conv on the
// 16x16x4 Winograd kernel has to know: that kernel takes its input multiplied by its own style (plan_call's second pass).
struct ConvForm {
    bool fused_rgb, winograd, wino64, wino43;
};
ConvForm conv_form_of(const PlanContext& ctx, int idx, const LayerPlan& p, bool have_y_then) {
    const ConvLayerHost& c = ctx.convs[idx];
    const LayerCaps& caps = ctx.caps[idx];
    const int res = 1 << c.res_log2, B = ctx.B;
    ConvForm form{};
    // the network's last conv absorbs its ToRGB when one block holds all channels of a pixel
    // (BM = Cout = 32, i.e. the 1024^2 generator of config-f and the 512^2 one of config-e, or BM = Cout = 16, config-e at
    // 1024^2): neither its activation nor the fp32 image is
    // written, only the uint8 frame -- so not where a debug tap reads that activation:
    // gance_engine_debug_read_activation would return whatever an earlier call left in the buffer
    const auto& tile = gance::kConvTiles[p.tile_id];
    form.fused_rgb = c.res_log2 == ctx.convs.back().res_log2 && ctx.limit() == ctx.num_convs() && p.nsplit == 1 &&
                     p.m_tiles == 1 && tile.TB == 1 && (tile.BM == 32 || tile.BM == 16) && have_y_then && ctx.stop_after <= 0;
    // Winograd form: the engine flags choose (0 never: DIRECT_CONV, 1 where the launch fills the chip, 2 whatever the block count: FORCE_WINOGRAD)
    const int wino_mode = (ctx.flags & GANCE_FLAG_DIRECT_CONV) ? 0 : ((ctx.flags & GANCE_FLAG_FORCE_WINOGRAD) ? 2 : 1);
    // ... unless the layer runs in Winograd form on the 16x16x4 kernel's 32-channel geometry (or in F(4x4,3x3) form) with the ToRGB
    // channel sum in its epilogue (measured: see DESIGN.md §3): where the launch fills the chip, or Winograd is forced
    const long long last_tiles = (long long)(res / 16) * (res / 32) * B;
    if (form.fused_rgb && c.cout == 32 && caps.has[kWino64] && !(ctx.flags & GANCE_FLAG_DIRECT_CONV) &&
        (wino_mode == 2 || last_tiles >= ctx.num_cus))
        form.fused_rgb = false;
    // Winograd F(2x2,3x3) form where the layer supports it and the launch fills the chip (one block per CU).
    // The fill rule counts the tiles of round 1's 32-channel kernel (HISTORY.md section D, item 20), which the plans were measured
    // with: 8 x 64 pixels, or 16 x 32 on the 32-pixel-wide layer; no split-K. That kernel's support predicate was cin % 8 == 0,
    // 24 <= cin <= 512, cout % 32 == 0, side a multiple of 32: on a square layer exactly winograd64_supported (cout % 64 == 0
    // wants the side a multiple of 8 and of 32, cout % 32 == 0 of 16 and of 32), so kWino64 names the same set of layers.
    const long long wino_tiles = (long long)(c.cout / 32) * (res % 64 == 0 ? (res / 8) * (res / 64) : (res / 16) * (res / 32)) * B;
    form.winograd = !c.up && wino_mode != 0 && caps.has[kWino64] && (wino_mode == 2 || (p.nsplit == 1 && wino_tiles >= 256));
    // the kernel on 16x16x4 MFMAs: every stride-1 conv it supports that follows an up layer (all of them do: Conv1 follows Conv0_up)
    form.wino64 = !form.fused_rgb && form.winograd && idx > 0 && ctx.convs[idx - 1].up;
    // F(4x4, 3x3) where the layer has the weights for it (layer_caps: resolution limit, geometry, an up layer in
    // front) and the launch fills the chip; never the network's last layer while that one carries the fused ToRGB
    const long long w43_tiles = (long long)(c.cout / 32) * (res >= 64 ? (res / 16) * (res / 64) : 1) * B;  // (32 x 32 pixels per tile on the 32-wide layer)
    form.wino43 = !form.fused_rgb && form.winograd && caps.has[kWino43] && (w43_tiles >= ctx.num_cus || wino_mode == 2);
    if (form.wino43) form.wino64 = false;
    return form;
}

// Whether up layer idx runs as the fused kernel (transposed conv + FIR in one launch): where it is supported and fills
// the chip; the engine flags choose (0 never: SPLIT_UPFIR, 1 by that rule, 2 wherever supported: FORCE_FUSED_UPFIR). The layer BEFORE
// it has to know: fed by a 16x16x4 Winograd launch the fused kernel takes its input pre-scaled by its style (plan_call's second pass).
// split: the split-operand form (launch_upfir_split); fp32: the fp32-MFMA forms (launch_upfir16_fused)
enum class FusedUp { no, fp32, split };
FusedUp up_runs_fused(const PlanContext& ctx, int idx, gance::UpFirArgs* plan) {
    const ConvLayerHost& c = ctx.convs[idx];
    const LayerCaps& caps = ctx.caps[idx];
    const Tuning::PerEngine& knobs = ctx.tune.engine;
    const int H = (1 << c.res_log2) / 2, B = ctx.B;
    const int upfir_mode = (ctx.flags & GANCE_FLAG_SPLIT_UPFIR) ? 0 : ((ctx.flags & GANCE_FLAG_FORCE_FUSED_UPFIR) ? 2 : 1);
    if (!c.up || upfir_mode == 0 || !caps.has[kUpfir16]) return FusedUp::no;
    gance::UpFirArgs u{};
    u.Cin = c.cin;
    // the split-operand form (upfir_split.hip; a block sweeps the image's height, or a row segment of it where whole images would leave
    // CUs idle: upfirs_plan): where its launch has blocks for 9/16 of the CUs
    if (caps.has[kUpfirSplit] && upfir_mode != 0) {
        gance::upfirs_plan(B, c.cout, H, H, ctx.num_cus, &u);
        // (9/16: measured without row segments, 16 blocks per frame at every layer -- whole calls of 8 / 9 / 10 / 11 frames ran at 1053 / 842 / 909 / 940
        // frames/s in the fp32 forms, at 953 / ~1000 / 1045 / 1106 in this one; with row segments 1 ... 8 frames per call take it too wherever 16-row
        // segments reach that many blocks: 645 / 895 / 899 / 1080 / 934 / 1055 / 1136 / 1202 frames/s against 614 / 817 / 861 / 960 / - / 980 / - / 1047)
        // (mode 2 forces the wide geometry only; the narrow ones -- 64 / W channel tiles per block -- take the fill rule in both modes)
        const bool narrow = !gance::upfirs_supported(c.cin, c.cout, H, H);
        if ((knobs.upfir_split == 2 && !narrow) || u.total_blocks >= ctx.num_cus * 9 / 16) {
            *plan = u;
            return FusedUp::split;
        }
        u = gance::UpFirArgs{};
        u.Cin = c.cin;
    }
    gance::upfir16_plan(B, c.cout, H, H, ctx.num_cus, &u);
    const int steps_per_seg = u.rows_per_seg / u.step_rows;
    *plan = u;
    // (the narrow strip geometries -- inputs 32 and 16 wide -- have one or two steps per image: never cut into segments)
    return (upfir_mode == 2 || (u.total_blocks >= ctx.num_cus * 3 / 4 && (u.segs == 1 || steps_per_seg >= 4))) ? FusedUp::fp32 : FusedUp::no;
}

// The launch names of a layer's step, as gance_engine_step_info reports them (the launch loop and gance_engine_describe_plan both
// read them from here). conv<N> direct form, convW F(2x2,3x3), convV F(4x4,3x3), convVG the same as 36 dense GEMMs (input transform +
// GEMMs + output transform); +rgb: the ToRGB channel sum in the epilogue, +torgb: the whole ToRGB. convT the two-pass up layer,
// convTG its scatter form (pack + GEMM + gather), convTF one fused up kernel, convTFp with its input pre-scaled by its style
// (the *_pre_kernel variants); a trailing "/16": the fp32 form, 16 channels per block (upfir16_fused*_kernel), "/16x": its pair
// form, "/s3": the split-operand form (upfirs_fused*_kernel: bf16 x 3 parts, six product terms, fp32 accumulation).
void name_step(const ConvLayerHost& c, LayerStep* s) {
    const int res = 1 << c.res_log2;
    const char* kind = "";
    switch (s->form) {
        case Form::Direct: case Form::DirectSplitK: case Form::DirectTorgb: break;
        case Form::Wino64: kind = "W"; break;
        case Form::Wino43: kind = "V"; break;
        case Form::WinoGemm: kind = "VG"; break;
        case Form::UpTwoPass: kind = "T"; break;
        case Form::UpGemm: kind = "TG"; break;
        case Form::UpFused16: case Form::UpFused16x: case Form::UpSplit: kind = s->input_prescaled ? "TFp" : "TF"; break;
    }
    const char* suffix = s->form == Form::UpFused16 ? "/16" : (s->form == Form::UpFused16x ? "/16x" : (s->form == Form::UpSplit ? "/s3" : ""));
    const bool absorbs_torgb = s->form == Form::DirectTorgb;
    std::snprintf(s->name, sizeof(s->name), "conv%s%d%s_%dx%d_%d->%d%s", kind, c.layer_idx, absorbs_torgb ? "+torgb" : (s->rgb_sum ? "+rgb" : ""),
                  res, res, c.cin, c.cout, suffix);
    if (s->form == Form::DirectSplitK) std::snprintf(s->second, sizeof(s->second), "finish%d_%dx%d", c.layer_idx, res, res);
    if (s->form == Form::UpTwoPass || s->form == Form::UpGemm) std::snprintf(s->second, sizeof(s->second), "fir%d_%dx%d", c.layer_idx, res, res);
    if (!c.up && !absorbs_torgb) std::snprintf(s->torgb, sizeof(s->torgb), "torgb_%dx%d", res, res);  // ToRGB after the 4x4 conv and after every Conv1
}

// One record per conv layer of a call of B frames. First every layer's own form, which depends only on (layer, B, flags):
// conv_form_of / up_runs_fused, each asked once per layer. Then the links between neighbours (who scales whose input) from the
// finished list. No plan cache: this is cheaper than the per-launch decisions it replaced.
std::vector<LayerStep> plan_call(const std::vector<ConvLayerHost>& convs, const std::vector<LayerCaps>& caps, const Tuning& tune, int flags,
                                 int num_cus, int B, int stop_after) {
    const PlanContext ctx{convs, caps, tune, flags, num_cus, B, stop_after};
    const int limit = ctx.limit();
    std::vector<LayerStep> steps(limit);
    std::vector<ConvForm> forms(limit, ConvForm{});
    for (int li = 0; li < limit; ++li) {
        const ConvLayerHost& c = convs[li];
        const int res = 1 << c.res_log2, H = res / 2;
        LayerStep& s = steps[li];
        s.p = plan_layer(c, B);
        s.last_of_all = c.res_log2 == convs.back().res_log2 && limit == ctx.num_convs();
        s.may_skip_y_store = s.last_of_all && res > 128;
        if (!c.up) {
            // (a skip image exists from the 4x4 layer's ToRGB on: have_y)
            const ConvForm form = forms[li] = conv_form_of(ctx, li, s.p, li > 0);
            // Winograd F(4x4,3x3) as 36 dense GEMMs: at 8x8 / 16x16 always (from Tuning::winogemm_min_columns columns up), at 32x32 ... 128x128 for the
            // calls too small for the fused F(4x4,3x3) kernel (one tile per CU): one frame per call at 128x128, up to 4 at 64x64, 16 at 32x32
            const int gemm_columns = B * (res / 4) * (res / 4);
            if (caps[li].has[kWinoGemm] && gemm_columns >= tune.winogemm_min_columns && gemm_columns <= gance::kWinoGemmMaxColumns && !form.wino43) {
                s.form = Form::WinoGemm;
            } else if (form.fused_rgb) {
                s.form = Form::DirectTorgb;
            } else if (s.p.nsplit == 1 || form.wino64 || form.wino43) {
                s.form = form.wino43 ? Form::Wino43 : (form.wino64 ? Form::Wino64 : Form::Direct);
                // Where the 64-channel Winograd kernel holds every channel of a pixel in one block (Cout = 64 at 512^2,
                // Cout = 32 at 1024^2) its epilogue also does the channel sum of the layer's ToRGB on the matrix pipe; the
                // ToRGB pass then only adds bias and skip image (and converts). The LAST layer's activation has no
                // other reader and is not stored (unless a debug tap wants it). Tuning::w64_rgb turns this off.
                s.rgb_sum = tune.w64_rgb && ((form.wino64 && gance::winograd64_rgb_supported(c.cout)) || (form.wino43 && gance::winograd43_rgb_supported(c.cout)));
                if (s.rgb_sum) {
                    s.rgb_partials = form.wino43 ? gance::winograd43_rgb_partials(c.cout) : gance::winograd64_rgb_partials(c.cout);
                    s.stores_activation = !(s.last_of_all && stop_after <= 0);
                }
            } else {
                s.form = Form::DirectSplitK;
            }
        } else {
            const FusedUp fused = up_runs_fused(ctx, li, &s.up);
            // (the scatter form: at 4x4 / 8x8 inputs from Tuning::upgemm_min_columns columns up, at 32x32 / 64x64 inputs for calls this small)
            const bool scatter = caps[li].has[kUpGemm] && B * H * H >= tune.upgemm_min_columns &&
                                 B * H * H <= gance::upgemm_max_columns(c.cout, tune.upgemm_buffer_columns);
            s.form = fused == FusedUp::split ? Form::UpSplit
                                             : (fused == FusedUp::fp32 ? Form::UpFused16 : (scatter ? Form::UpGemm : Form::UpTwoPass));
        }
    }
    for (int li = 0; li < limit; ++li) {
        const ConvLayerHost& c = convs[li];
        LayerStep& s = steps[li];
        const bool has_next = li + 1 < limit;
        if (!c.up) {
            // the next layer's style rides on this launch's stores when that layer is a fused up kernel — and only when this
            // launch also does the ToRGB channel sum (from the plain values): torgb_kernel would otherwise read the scaled ones
            // (only the 16x16x4 Winograd kernels scale their stores)
            s.scales_stores = s.rgb_sum && (s.form == Form::Wino64 || s.form == Form::Wino43) && c.cout % 64 == 0 && tune.prescale_up && has_next &&
                              is_fused_up(steps[li + 1].form);
            if (s.scales_stores) steps[li + 1].input_prescaled = true;
        } else {
            // ... and on an up layer's activation when the next layer takes its input pre-scaled
            s.scales_stores = has_next && !convs[li + 1].up &&
                              ((forms[li + 1].wino64 && gance::winograd64_input_prescaled(convs[li + 1].cout)) || forms[li + 1].wino43);
            if (s.form == Form::UpFused16 && caps[li].has[kUpfir16x] && s.input_prescaled) s.form = Form::UpFused16x;
        }
        name_step(c, &s);
    }
    return steps;
}

}  // namespace
