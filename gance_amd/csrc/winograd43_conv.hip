// Winograd F(4x4, 3x3) form of the modulated 3x3 stride-1 convolution on v_mfma_f32_16x16x4_f32 (SURVEY.md §8 a18:
// `modulated_conv2d_layer` -> tf.nn.conv2d), for the Conv1 layers whose K loop is deep (64^2 ... 256^2).
//
// Why. F(2x2,3x3) (winograd64_conv.hip) spends 16 multiplies on 4 outputs, F(4x4,3x3) 36 on 16: 2.25 instead of 4 per
// output, i.e. 0.5625 of the matrix work. In float32 the larger transform costs nothing measurable in accuracy on this
// network (tools/experiments/winograd_f43_error.py: max |image - fp64 oracle| 1.4e-5 with F(4x4,3x3) on the 64^2 ...
// 256^2 layers against 0.8e-5 with F(2x2,3x3), bar 1e-3; interpolation points 0, +-1, +-2, weights transformed in
// float64 on the host).
//
// What it costs on gfx950. The fp32 MFMA runs at the fp32 VECTOR rate and shares the vector ALUs, so the 144 vector
// operations of a 6x6 input transform (84 instructions here: packed column pass, eight-instruction row pass) are not hidden
// beside the 36 MFMAs they feed -- they add their issue time. This kernel runs TWO waves per SIMD (8 per block, <= 256
// registers each): 36 positions x one 16 x 16 accumulator tile = 144 accumulators per wave, 36 MFMAs (1152 cycles) per
// k-step of four input channels against ~340 cycles of transform; while one wave waits for LDS, a barrier or the issue
// of an LDS-DMA piece the other keeps the matrix pipe busy. (One wave per SIMD with 32 channels x 16 tiles does the
// transform once for two channel tiles, but pays every such wait in full: measured 12 % slower)
//
// Geometry. Block = 8 waves = 2 channel tiles of 16 x 4 tile rows; a wave owns 16 channels x one row of sixteen 4x4 output
// tiles (4 x 64 pixels): the block 32 channels x 16 x 64 pixels. The two waves of a SIMD take the two channel tiles of the
// SAME tile row (tile row = SIMD id, channel tile = the wave's ticket on that SIMD): they run the two halves of the pipeline,
// and their ToRGB sums meet in LDS, so a block writes ONE partial ToRGB image. Lane (n = lane % 16, g = lane / 16) transforms the 6x6
// window of tile n for input channel 4 ks + g; as A operand it holds output channel n of its channel tile for the same
// input channel. The input arrives ALREADY multiplied by this layer's style (ConvArgs::x contract, as for the
// 32-channel geometry of winograd64_conv.hip: the producing up layer folds s[b][ci] into its leaky ReLU; V is linear in d).
//
// Staging. K chunk = 4 input channels = one k-step: transformed weights [channel tile][ci][co % 16][36 positions] (a
// lane's 36 weights are contiguous: six 8-byte reads per window column; (tile, ci) units padded to 578 floats so the four
// g groups of a read fall into different banks) + the haloed patch [4][18][72], together 40 LDS-DMA pieces of 1 KB, five
// per wave, three ring slots (120 KB). One wait + barrier per k-step; chunk q+2 is issued right behind the barrier of
// k-step q into the slot k-step q-1 read.
//
// Epilogue: output transform A^T M A in registers (the 36 positions of a (channel, tile) pair live in ONE lane),
// demodulation, noise, bias, leaky ReLU, optional scale by the next layer's style, 16-byte stores (256 contiguous
// bytes per 16 lanes; buffer stores: one lane offset per tile, scalar offsets per store), (RGB) the ToRGB channel sum as per-lane FMAs
// added over the four lane rows by two lane swaps. What a tile costs outside its K loop is the issue time of this code: it is written
// for few instructions, and scalar fp32 where packed would be shorter (HISTORY.md section D item 21). The two epilogues of a tile (one per channel tile = per wave of a SIMD) run in the SAME interval between two
// barriers, the first interval of the block's next tile, beside that interval's multiplies: the wave that finishes a tile's K loop
// first defers its epilogue by one interval (see the stream loop). One after the other, each with its SIMD partner parked at
// the barrier, they cost 7.5 us per tile, which is 1.9 ms of the 1024^2 layer's 5.4.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kernels.h"

#ifndef GANCE_W43_ABLATE
#define GANCE_W43_ABLATE 0  // timing ablations (wrong results; Makefile w43ab%): 1 no DMA inside the stream, 2 no input transform,
                            // 4 no weight reads, 8 no window reads (nor transform), 16 no barrier per k-step
#endif

namespace gance {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr int kKC = 4;                         // input channels per chunk = one k-step of the 16x16x4 MFMA
constexpr int kBM = 32;                        // output channels per block (2 channel tiles of 16)
constexpr int kUnit = 16 * 36;                 // a (channel tile, ci) unit of weights: [co % 16][36]: a lane's 36 weights are nine aligned float4
constexpr int kWPieces = 18;                   // 8 units = 4608 floats = 18 pieces of 256 floats
constexpr int kWFloats = kWPieces * 256;
constexpr int kPiecesPerWave = 5;
// Pixel geometry of a block: TW x (1024 / TW) pixels = 64 tiles of 4x4; a wave's sixteen tiles are TW / 4 tile columns x
// 16 / (TW / 4) tile rows. <64>: 16 x 64 pixels, a wave = one row of 16 tiles (layers >= 64 wide); <32>: 32 x 32 pixels,
// a wave = two rows of 8 tiles (the 32x32 layer).
template <int TW>
struct Geo43 {
    static constexpr int kTW = TW, kTH = 1024 / TW;
    static constexpr int kTC = TW / 4, kTR = 16 / kTC;           // tile columns / tile rows of a wave
    static constexpr int kPW = kTW + 8, kPH = kTH + 2;            // haloed patch (16-byte aligned row segments): 18 x 72 / 34 x 40
    static constexpr int kPlane = kPH * kPW;                      // 1296 / 1360 floats per input channel
    static constexpr int kPatchF4 = kKC * kPlane / 4;
    static constexpr int kPPieces = (kPatchF4 + 63) / 64;         // 21 / 22 (the last one a quarter full)
    static constexpr int kPieces = kWPieces + kPPieces;           // 39 (+ one repeat of patch piece 0: every wave issues five) / 40
    static_assert(kPieces <= 8 * kPiecesPerWave && kPieces > 7 * kPiecesPerWave, "five LDS-DMA pieces per wave and chunk");
    static constexpr int kSlot = kPieces * 256;                   // 39 / 40 KB
    static constexpr int kNoiseRowsPerPiece = 256 / kTW;          // noise rows one 1 KB piece covers: 4 / 8
};
constexpr int kNBUF = 3;                       // ring slots: chunk G + 2 is issued during k-step G
// constants of a tile, fetched by LDS-DMA with its first chunk (a global load in the epilogue costs its whole latency once
// per tile, and the wait behind it would drain the ring): demod | bias | next layer's style (32 each, padded to 64) |
// noise [16][64] | (RGB) the ToRGB coefficients in launch_winograd64_rgb_coef's layout [2 channel tiles][4 r][16 g + colour]
constexpr int kConstD = 0, kConstB = 64, kConstS = 128, kConstNoise = 192, kConstRgb = kConstNoise + 1024, kConstFloats = kConstRgb + 512;
constexpr int kStoresPerEpilogue = 16, kRgbStores = 12;
// (RGB) the ToRGB sums of a wave's sixteen channels, left in LDS for the add with the sums of the wave that holds the OTHER sixteen
// channels of the same pixels: [tile row][output row x colour = 12][16 lanes] float4, one such buffer per role
constexpr int kRgbXchgFloats = 4 * 12 * 16 * 4;

// B^T of F(4,3), points 0, +-1, +-2 (Lavin & Gray): 12 vector instructions, on one window line or on two at once
template <typename T>
__device__ __forceinline__ void input_transform6(T d0, T d1, T d2, T d3, T d4, T d5, T (&t)[6]) {
    const T a = d4 - 4.f * d2;
    const T b = d3 - 4.f * d1;
    const T c = d4 - d2;
    const T e = d3 - d1;
    t[0] = 4.f * d0 + (d4 - 5.f * d2);
    t[1] = a + b;
    t[2] = a - b;
    t[3] = c + 2.f * e;
    t[4] = c - 2.f * e;
    t[5] = 4.f * d1 + (d5 - 5.f * d3);
}

// The same B^T along a window ROW whose six values lie in three register pairs (d0, d5), (d1, d2), (d3, d4) -- which is how
// the packed column pass leaves them: eight vector instructions instead of twelve. (b, a), (e, c) are one packed operation
// each; t1 = a + b | t2 = a - b and t3 = c + 2 e | t4 = c - 2 e are one each with both result halves reading BOTH halves of
// the same source pair (op_sel), which hipcc does not form by itself; t0 and t5 mix three pairs and stay scalar.
__device__ __forceinline__ void input_transform6_row(f32x2 r05, f32x2 r12, f32x2 r34, float (&t)[6]) {
    const f32x2 ba = r34 - 4.f * r12;
    const f32x2 ec = r34 - r12;
    f32x2 t12, t34;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(t12) : "v"(ba));
    asm("v_pk_fma_f32 %0, %1, 2.0, %1 op_sel:[0,0,1] op_sel_hi:[0,0,1] neg_hi:[1,0,0]" : "=v"(t34) : "v"(ec));
    t[0] = 4.f * r05[0] + (r34[1] - 5.f * r12[1]);
    t[1] = t12[0];
    t[2] = t12[1];
    t[3] = t34[0];
    t[4] = t34[1];
    t[5] = 4.f * r12[0] + (r05[1] - 5.f * r34[0]);
}

// A^T of F(4,3): 10 vector instructions
__device__ __forceinline__ void output_transform6(float m0, float m1, float m2, float m3, float m4, float m5, float (&y)[4]) {
    const float s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
    y[0] = m0 + s1 + s2;
    y[1] = fmaf(2.f, d2, d1);
    y[2] = fmaf(4.f, s2, s1);
    y[3] = fmaf(8.f, d2, d1) + m5;
}

// f / D for 0 <= f < MAX as one 24-bit multiply and a shift: with m = ceil(2^16 / D), floor(f m / 2^16) = floor(f / D) as long as
// f (m D - 2^16) < 2^16
template <int D, int MAX>
__device__ __forceinline__ unsigned div_small(unsigned f) {
    constexpr unsigned m = (65536 + D - 1) / D;
    static_assert((unsigned long long)MAX * (m * D - 65536) < 65536 && (unsigned long long)MAX * m < (1ull << 32) && MAX < (1 << 24), "multiplier exact over the range");
    return __umul24(f, m) >> 16;
}

// One step of a sum over lane rows: v_permlane32_swap (v_permlane16_swap) exchanges the upper 32 lanes (the odd rows of 16) of `a` with
// the lower 32 (the even rows) of `b`; a + b then holds the sums of a over the row pairs in the lower lanes (even rows) and those of b in
// the upper (odd rows). Written as assembly: with the two results of __builtin_amdgcn_permlane32_swap feeding one add, hipcc added the instruction's
// FIRST result to itself (v_add v0, v12, v12 behind v_permlane32_swap v12, v8). The s_nop covers the two wait states the instruction
// needs behind a vector write of its operands, which the compiler cannot see into an asm statement to provide.
template <int ROWS>
__device__ __forceinline__ float swap_add(float a, float b) {
    if constexpr (ROWS == 32)
        asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    else
        asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}

struct Tile43 {
    int m_tile, y0, x0, b0;
};

// The lane id, computed where it is used: per-lane values derived once at kernel entry would be live across the epilogue,
// where every register is taken; hipcc spills them, and a scratch reload inside the k-steps is a vector-memory load whose
// wait drains the LDS-DMA ring. Everything per-lane is therefore re-derived from this after every epilogue.
__device__ __forceinline__ int fresh_lane() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

}  // namespace

template <bool RGB, int TW>
__device__ __forceinline__ void winograd43_body(const ConvArgs& p) {
    using Geo = Geo43<TW>;
    constexpr int kTW = Geo::kTW, kTH = Geo::kTH, kPW = Geo::kPW, kPH = Geo::kPH, kPlane = Geo::kPlane, kPatchF4 = Geo::kPatchF4;
    constexpr int kPieces = Geo::kPieces, kSlot = Geo::kSlot, kTC = Geo::kTC, kTR = Geo::kTR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const const0 = smem + kNBUF * kSlot;  // two sets of tile constants (tile parity)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Work of this wave: tile row = the SIMD it runs on, channel tile = its ticket there (two waves of 256 registers fill a
    // SIMD, so each SIMD holds exactly two of the block's eight). The two waves of a SIMD then hold the two channel tiles of
    // the SAME pixels and run the two halves of the pipeline (see the stream loop): the ticket is the wave's role as well, and
    // their ToRGB sums are added without an atomic: each role leaves its own in LDS, role 0 adds them a barrier later (finish_rgb).
    // Which waves share a SIMD is the dispatcher's choice, so the wave asks the hardware (HW_ID.simd_id).
    __shared__ int simd_tickets[4];
    if (tid < 4) simd_tickets[tid] = 0;
    __syncthreads();
    const int pg = __builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4) & 3;  // hwreg(HW_REG_HW_ID, 4, 2)
    int ticket = 0;
    if ((tid & 63) == 0) ticket = atomicAdd(&simd_tickets[pg], 1) & 1;
    const int cot = __builtin_amdgcn_readfirstlane(ticket);
    const int role = cot;
    // Run-time guard of that assumption: were a SIMD ever given one or three of the block's waves (a build whose register
    // count let a third wave fit, tools/check_w43_isa.py skipped), two waves would share a role and write wrong pixels in
    // silence. Every wave of the block sees the same four counts: the block records the fault where the host reads it
    // before the next call (engine.hip: check_call) and leaves, uniformly, before its first barrier-dependent step.
    __syncthreads();
    if (simd_tickets[0] != 2 || simd_tickets[1] != 2 || simd_tickets[2] != 2 || simd_tickets[3] != 2) {
        if (wave == 0 && fresh_lane() == 0 && p.fault_flag != nullptr) __hip_atomic_store(p.fault_flag, 43, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const int Hp = p.H + 2, Wp = p.W + 8;
    const int n = p.total_chunks;               // chunks per tile
    const int my_tiles = (p.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int total = my_tiles * n;             // chunks of this block's stream

    // tile i of this block -> tile, XCD-aware (a persistent block strides by a multiple of 8; consecutive ids run on one XCD:
    // the channel tiles of a pixel tile share its L2)
    auto decode = [&](int i) {
        const int v = (int)blockIdx.x + i * (int)gridDim.x;
        const int nwg = p.total_tiles;
        const int q = nwg >> 3, r = nwg & 7, xcd = v & 7;
        int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (v >> 3);
        Tile43 t;
        if (p.m_tiles == 16 && p.xcd_blocking) {
            // An XCD's 32 CUs work on 32 consecutive ids at a time: with the channel tile fastest that is 2 pixel tiles x 16
            // channel tiles -- every XCD streams the layer's whole 37.7 MB of transformed weights per 5.2 MB of patches (x5.6 of the
            // algorithmic bytes at 32^2 / 64^2). 4 pixel tiles x 8 channel tiles move 29 MB per round instead of 43: blocks walk K in
            // step, so the sharing is by timing, not by L2 capacity.
            const int j = id & 63, sg = id >> 6;  // (64 ids = 4 pixel tiles x 16 channel tiles)
            t.m_tile = 8 * (j >> 5) + (j & 7);
            id = 4 * sg + ((j & 31) >> 3);
        } else if (p.tile_shifts >= 0) {
            const int sh = p.tile_shifts & 31;
            t.m_tile = id & ~(-1 << sh);
            id >>= sh;
        } else {
            t.m_tile = id % p.m_tiles;
            id /= p.m_tiles;
        }
        // (every shape winograd43_supported admits from this network has power-of-two counts: shifts on the scalar unit; an integer
        // division is a reciprocal sequence on the vector unit with its result read back by lane, three per decode)
        if (p.tile_shifts >= 0) {
            const int shx = (p.tile_shifts >> 8) & 31, shy = (p.tile_shifts >> 16) & 31;
            t.x0 = (id & ~(-1 << shx)) * kTW;
            id >>= shx;
            t.y0 = (id & ~(-1 << shy)) * kTH;
            t.b0 = id >> shy;
        } else {
            t.x0 = (id % p.tiles_x) * kTW;
            id /= p.tiles_x;
            t.y0 = (id % p.tiles_y) * kTH;
            t.b0 = id / p.tiles_y;
        }
        return t;
    };

    // ---- per-lane values of the k-steps (re-derived after every epilogue: see fresh_lane) ----
    // LDS-DMA pieces of this wave: piece wave * 5 + r; < 18: weights (linear), else patch piece (per-lane source offset);
    // operand offsets of the lane inside a slot (floats): its window (rows 4 pg .. + 5, columns 4 n + 3 .. + 8) and its weights
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, 0x7fffffff, 0x00020000);
    int piece_voff[kPiecesPerWave];
    int win_off, a_off;
    auto lane_setup = [&]() {
        const int lane = fresh_lane();
        const int n16 = lane & 15, g = lane >> 4;
#pragma unroll
        for (int r = 0; r < kPiecesPerWave; ++r) {
            int piece = wave * kPiecesPerWave + r;
            if (piece >= kPieces) piece = kWPieces;  // (the fortieth slot repeats patch piece 0: same bytes to the same place)
            if (piece < kWPieces) {
                piece_voff[r] = piece * 1024 + lane * 16;
            } else {
                int f = (piece - kWPieces) * 64 + lane;
                if (f >= kPatchF4) f = (piece - kWPieces) * 64;  // (the last piece is a quarter full: the rest re-copy its first float4 into padding)
                // f -> (channel, patch row, float4 of the row): this runs after every epilogue, so the two divisions are 24-bit multiplies
                // and shifts (div_small) and the products 24-bit too (c Hp + row < 2^13, Wp < 2^11); a 32-bit v_mul_lo / v_mul_hi, which
                // is what `/`, `%` and `*` compile to here, issues at a quarter of the rate
                const unsigned t = div_small<kPW / 4, 64 * Geo::kPPieces>((unsigned)f);
                const unsigned q4 = (unsigned)f - __umul24(t, kPW / 4);
                const unsigned c = div_small<kPH, 64 * Geo::kPPieces>(t);
                const unsigned row = t - __umul24(c, kPH);
                piece_voff[r] = (int)((__umul24(__umul24(c, (unsigned)Hp) + row, (unsigned)Wp) + 4 * q4) * 4);
            }
        }
        win_off = kWFloats + g * kPlane + 4 * (pg * kTR + n16 / kTC) * kPW + 4 * (n16 % kTC);
        a_off = (cot * 4 + g) * kUnit + n16 * 36;
    };
    lane_setup();
    // Staging side of the stream (all scalar): the next chunk to fetch = chunk st_q of this block's tile st_tile, into ring
    // slot st_slot; byte offsets of its weights and its patch; the patch's buffer resource (one per sample).
    int st_tile = 0, st_q = 0, st_slot = 0, st_w = 0, st_x = 0, st_count = 0;
    __amdgpu_buffer_rsrc_t st_x_rsrc = w_rsrc;
    const int x_chunk_step = kKC * Hp * Wp * 4;
    int cur_slot = 0, cur_w = 0, cur_x = 0;  // of the chunk being staged
    bool cur_valid = false;
    // Opens the next chunk of the stream (runs once per k-step, outside the MFMA weave: it branches). A chunk that opens a
    // tile also brings the tile's constants: up to two extra DMA instructions per wave, issued here, i.e. BEFORE the
    // chunk's five pieces (the counted waits allow the five youngest operations to be in flight).
    auto stage_begin = [&]() {
        cur_valid = st_count < total;
        if (!cur_valid) return;
        if (st_q == 0) {
            const Tile43 t = decode(st_tile);
            const int lane = fresh_lane();
            st_x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (size_t)t.b0 * p.x_b_stride), 0, 0x7fffffff, 0x00020000);
            st_w = t.m_tile * n * (kWFloats * 4);  // bytes: [m tile][chunk][kWFloats]
            st_x = (t.y0 * Wp + t.x0) * 4;         // patch row 0 = image row y0 - 1 = buffer row y0; column x0 - 4 = buffer column x0
            float* const set = const0 + (st_tile & 1) * kConstFloats;
            const int co = t.m_tile * kBM;
            if (wave < 3) {  // demod / bias / next style of the block's 32 channels: one dword piece each (the resource's bound clips the other lanes)
                const float* src = wave == 0 ? p.d + (size_t)t.b0 * p.d_stride + co
                                             : (wave == 1 ? p.bias + co : (p.s_next != nullptr ? p.s_next + (size_t)t.b0 * p.s_stride + co : nullptr));
                if (src != nullptr) {
                    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, kBM * 4, 0x00020000);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(c_rsrc, (lds_ptr_t)(set + wave * 64), 4, lane * 4, 0, 0, 0);
                }
            } else if (wave < 7) {  // a quarter of the tile's noise (256 floats = 4 rows of 64 / 8 rows of 32): one 16-byte piece
                if (p.noise != nullptr) {
                    const __amdgpu_buffer_rsrc_t nz_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.noise, 0, 0x7fffffff, 0x00020000);
                    const int row = Geo::kNoiseRowsPerPiece * (wave - 3) + lane / kTC;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(nz_rsrc, (lds_ptr_t)(set + kConstNoise + (wave - 3) * 256), 16,
                                                             ((t.y0 + row) * p.OW + t.x0 + 4 * (lane % kTC)) * 4, t.b0 * p.noise_b_stride * 4, 0, 0);
                }
            } else if (RGB) {  // the ToRGB coefficients (laid out as MFMA A operands): [b][Cout / 4 steps][64 lanes], steps 8 m_tile .. + 7: two 16-byte pieces
                const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(p.rgb_coef + ((size_t)t.b0 * (p.Cout / 4) + 8 * t.m_tile) * 64), 0, 512 * 4, 0x00020000);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (lds_ptr_t)(set + kConstRgb), 16, lane * 16, 0, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (lds_ptr_t)(set + kConstRgb + 256), 16, lane * 16, 1024, 0, 0);
            }
        }
        cur_slot = st_slot;
        cur_w = st_w;
        cur_x = st_x;
        st_w += kWFloats * 4;
        st_x += x_chunk_step;
        st_slot = st_slot == kNBUF - 1 ? 0 : st_slot + 1;
        ++st_count;
        if (++st_q == n) {
            st_q = 0;
            ++st_tile;
        }
    };
    // piece r of the chunk stage_begin() opened: one instruction, no control flow beyond the wave-uniform choice of its kind
    auto stage_piece = [&](int r) {
        float* const base = smem + cur_slot * kSlot;
        int piece = wave * kPiecesPerWave + r;  // (wave is scalar: the branches are uniform)
        if (piece >= kPieces) piece = kWPieces;
        if (piece < kWPieces)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_ptr_t)(base + piece * 256), 16, piece_voff[r], cur_w, 0, 0);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(st_x_rsrc, (lds_ptr_t)(base + kWFloats + (piece - kWPieces) * 256), 16, piece_voff[r], cur_x, 0, 0);
    };

    float* const rgb_xchg = const0 + 2 * kConstFloats;  // [role][kRgbXchgFloats]
    size_t rgb_off = 0;  // (RGB) where the partial image of the tile whose sums lie in rgb_xchg begins (scalar; set by the epilogue)

    f32x4 acc[36];  // (every tile's first k-step overwrites them: multiply(first))

    // L + T: this lane's weights of the chunk (position j * 6 + i) and V = B^T d B of its window, both into registers.
    // Column pass first, two window columns per packed instruction (the pairs (4,5), (6,7) are aligned 8-byte reads,
    // (3, 8) one ds_read2_b32: fewest bytes; three aligned 16-byte reads per row -- no bank conflicts, twice the bytes -- and
    // one 16-byte read + two DPP row shifts both measured slower), then the row pass line by line.
    float V[36], A[36];
#if GANCE_W43_ABLATE & 12
    for (int k = 0; k < 36; ++k) V[k] = A[k] = 0.f;
#endif
    auto load_transform = [&](int slot) {
        const float* const P = smem + slot * kSlot + win_off;
        const float* const U = smem + slot * kSlot + a_off;
#if GANCE_W43_ABLATE & 8
#pragma unroll
        for (int k = 0; k < 36; ++k) asm volatile("" : "+v"(V[k]));
#if GANCE_W43_ABLATE & 4
#pragma unroll
        for (int k = 0; k < 36; ++k) asm volatile("" : "+v"(A[k]));
#else
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(U + 4 * k);
            A[4 * k + 0] = t[0], A[4 * k + 1] = t[1], A[4 * k + 2] = t[2], A[4 * k + 3] = t[3];
        }
#endif
        return;
#endif
        f32x2 c45[6], c67[6], c38[6];
#pragma unroll
        for (int y = 0; y < 6; ++y) {
            c45[y] = *reinterpret_cast<const f32x2*>(P + y * kPW + 4);
            c67[y] = *reinterpret_cast<const f32x2*>(P + y * kPW + 6);
            c38[y][0] = P[y * kPW + 3];
            c38[y][1] = P[y * kPW + 8];
        }
#if GANCE_W43_ABLATE & 4
#pragma unroll
        for (int k = 0; k < 36; ++k) asm volatile("" : "+v"(A[k]));
#else
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(U + 4 * k);
            A[4 * k + 0] = t[0];
            A[4 * k + 1] = t[1];
            A[4 * k + 2] = t[2];
            A[4 * k + 3] = t[3];
        }
#endif
#if GANCE_W43_ABLATE & 2
#pragma unroll
        for (int y = 0; y < 6; ++y) {
            V[y * 6 + 0] = c38[y][0], V[y * 6 + 1] = c45[y][0], V[y * 6 + 2] = c45[y][1];
            V[y * 6 + 3] = c67[y][0], V[y * 6 + 4] = c67[y][1], V[y * 6 + 5] = c38[y][1];
        }
        return;
#endif
        f32x2 t45[6], t67[6], t38[6];
        input_transform6<f32x2>(c45[0], c45[1], c45[2], c45[3], c45[4], c45[5], t45);
        input_transform6<f32x2>(c67[0], c67[1], c67[2], c67[3], c67[4], c67[5], t67);
        input_transform6<f32x2>(c38[0], c38[1], c38[2], c38[3], c38[4], c38[5], t38);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            // (kept opaque: where a packed result is only read by element, hipcc splits the packed operation again)
            asm("" : "+v"(t45[i]), "+v"(t67[i]), "+v"(t38[i]));
            float v[6];
            input_transform6_row(t38[i], t45[i], t67[i], v);
#pragma unroll
            for (int j = 0; j < 6; ++j) V[j * 6 + i] = v[j];
        }
    };
    // The 36 MFMAs of a k-step, and woven between them (one per seven MFMAs: an LDS-DMA instruction takes the wave about
    // 120 cycles to issue, behind the barrier that sat on every wave's critical path) the five DMA pieces of the chunk
    // stage_begin() opened, if there is one.
    // `first_tag`: the tile's first k-step takes C = 0 instead of the accumulators (144 clears per tile and wave saved).
    auto multiply = [&](auto first_tag) {
        constexpr bool kFirst = decltype(first_tag)::value;
#pragma unroll
        for (int pos = 0; pos < 36; ++pos) {
            acc[pos] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[pos], V[pos], kFirst ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[pos], 0, 0, 0);
            if (pos % 7 == 3 && cur_valid && !(GANCE_W43_ABLATE & 1)) stage_piece(pos / 7);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);  // 4 MFMAs, then 4 x (one LDS-DMA issue, 7 MFMAs), one issue, 4 MFMAs
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 7, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    };

    // ---- epilogue of this block's tile i: lane (n16, g) holds channels 4 g + r (r = 0 .. 3) of tile n16 for all 36
    // positions. Output transform, demodulation, noise, bias, leaky ReLU, (RGB) ToRGB channel sum, stores. ----
    auto epilogue = [&](int i) {
        const Tile43 t = decode(i);
        const float* const set = const0 + (i & 1) * kConstFloats;
        const int lane = fresh_lane();
        const int n16 = lane & 15, g = lane >> 4;
        const int ty4 = 4 * (pg * kTR + n16 / kTC), tx4 = 4 * (n16 % kTC);  // the lane's tile inside the block's pixel tile
        const int ct = t.m_tile * 2 + cot;  // 16-channel tile of the layer
        const f32x4 dm = *reinterpret_cast<const f32x4*>(set + kConstD + cot * 16 + 4 * g);
        const f32x4 bm = *reinterpret_cast<const f32x4*>(set + kConstB + cot * 16 + 4 * g);
        f32x4 sn = f32x4{1.f, 1.f, 1.f, 1.f};
        if (p.s_next != nullptr) sn = *reinterpret_cast<const f32x4*>(set + kConstS + cot * 16 + 4 * g);
        // (RGB) the layer's ToRGB channel sum over this wave's 16 channels, on the vector unit: the lane adds its own four channels
        // (colour c of channel 16 ct + 4 g + r: style x weight at [cot * 4 + r][16 g + c] of the table launch_winograd64_rgb_coef
        // prepares as MFMA A operands), 3 colours x 16 pixels = 48 sums; the four lane rows are added behind the channel loop. (As a
        // 16x16x4 MFMA product with 3 of 16 rows used, the sum held the matrix pipe for 2048 cycles per wave and tile and took 64
        // accumulators.)
        float rgb[3][4][4];  // [colour][output row][output column]
        // The activation stores go through a buffer resource at the tile's origin (its sample, 16-channel tile and pixel tile: scalar
        // arithmetic): the lane's part of an address is then ONE 32-bit offset for all sixteen stores and the (channel r, row oy) part a
        // scalar offset, where a flat store wants a 64-bit address per store, built on the vector unit (launch_winograd43_conv checks that
        // the offsets fit)
        const int c_step = (int)p.out_c_stride * 4, row_step = p.out_row_stride * 4;  // bytes
        __amdgpu_buffer_rsrc_t out_rsrc = w_rsrc;
        int out_voff = 0;
        if (p.out != nullptr) {
            out_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + (size_t)t.b0 * p.out_b_stride + (size_t)(ct * 16) * p.out_c_stride +
                                                                 (size_t)(t.y0 + p.out_y_off) * p.out_row_stride + t.x0 + p.out_x_off),
                                                         0, 0x7fffffff, 0x00020000);
            out_voff = 4 * g * c_step + ty4 * row_step + tx4 * 4;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __builtin_amdgcn_sched_barrier(0);  // one channel's 36 accumulators at a time (unfenced, hipcc hoists all four and spills)
            f32x4 a_rgb = f32x4{0.f, 0.f, 0.f, 0.f};  // (R, G, B, unused) coefficients of channel 4 g + r; the leaky ReLU's gain rides on them
            if constexpr (RGB) a_rgb = *reinterpret_cast<const f32x4*>(set + kConstRgb + (cot * 4 + r) * 64 + 16 * g) * 1.4142135623730951f;
            const float s2 = sn[r] * 1.4142135623730951f;
            float tr[4][6];  // A^T M: [output row][position column]
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                float col[4];
                output_transform6(acc[j * 6 + 0][r], acc[j * 6 + 1][r], acc[j * 6 + 2][r], acc[j * 6 + 3][r], acc[j * 6 + 4][r], acc[j * 6 + 5][r], col);
#pragma unroll
                for (int oy = 0; oy < 4; ++oy) tr[oy][j] = col[oy];
            }
#pragma unroll
            for (int oy = 0; oy < 4; ++oy) {
                float yrow[4];
                output_transform6(tr[oy][0], tr[oy][1], tr[oy][2], tr[oy][3], tr[oy][4], tr[oy][5], yrow);
                f32x4 nz = f32x4{0.f, 0.f, 0.f, 0.f};
                if (p.noise != nullptr) nz = *reinterpret_cast<const f32x4*>(set + kConstNoise + (ty4 + oy) * kTW + tx4) * p.noise_strength;
                // (element by element: as f32x4 arithmetic this becomes v_pk_mul / v_pk_fma / v_pk_add_f32 on register pairs the compiler first
                // builds with moves, and beside the partner wave's MFMAs a packed fp32 instruction costs more than the two it replaces)
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = yrow[k] * dm[r] + nz[k] + bm[r];
                    v[k] = fmaxf(v[k], 0.2f * v[k]);  // (x sqrt(2): in a_rgb and s2)
                }
                if constexpr (RGB) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int ox = 0; ox < 4; ++ox) rgb[c][oy][ox] = r == 0 ? a_rgb[c] * v[ox] : fmaf(a_rgb[c], v[ox], rgb[c][oy][ox]);
                }
                // (the stored activation carries the next layer's style when that layer wants it so; the ToRGB sum took the plain one)
                if (p.out != nullptr) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{v[0] * s2, v[1] * s2, v[2] * s2, v[3] * s2}), out_rsrc, out_voff, r * c_step + oy * row_step, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RGB) {
            // The sums of the four lane rows (channels 4 g + r, g = 0 .. 3) in two steps, each one swap and one add per two registers:
            // v_permlane32_swap of the sums of output rows (0, 2) / (1, 3) leaves rows 0 / 1 of both in the lower 32 lanes and rows
            // 2 / 3 in the upper; v_permlane16_swap of those two results leaves lane row g with the complete sums of OUTPUT row g:
            // 48 -> 24 -> 12 registers, and every lane row holds a different quarter of the tile's sums.
            float q[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ox = 0; ox < 4; ++ox) {
                    const float h02 = swap_add<32>(rgb[c][0][ox], rgb[c][2][ox]), h13 = swap_add<32>(rgb[c][1][ox], rgb[c][3][ox]);
                    q[c][ox] = swap_add<16>(h02, h13);
                }
            // Partial image of the block's 32 channels: [Cout / 32][B][3][OH][OW]. Lane row g of a wave holds (R, G, B) of output
            // row g of its tile's pixels for the wave's 16 channels; the other wave of the SIMD holds the other 16 channels of the
            // same pixels. Both epilogues of a tile run between the same two barriers, so neither wave can read the other's sums
            // here: each leaves its own in its role's buffer (three 16-byte units per lane), and the role-0 wave adds and stores them
            // behind the next barrier (finish_rgb). The buffers are written again at the next tile boundary, n >= 4 barriers later
            // (winograd43_supported): one buffer per role is enough, no second set by tile parity.
            f32x4* const xchg = reinterpret_cast<f32x4*>(rgb_xchg + cot * kRgbXchgFloats) + (pg * 12 + g) * 16 + n16;
#pragma unroll
            for (int c = 0; c < 3; ++c) xchg[c * 4 * 16] = f32x4{q[c][0], q[c][1], q[c][2], q[c][3]};
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (in LDS before this wave's next barrier)
            rgb_off = (((size_t)t.m_tile * p.B + t.b0) * 3) * p.OH * p.OW + (size_t)t.y0 * p.OW + t.x0;
        }
        lane_setup();
    };
    // (RGB, role 0, behind the barrier that follows a tile's two epilogues) the partial image of that tile: the sums of channel
    // tile 1 + those of channel tile 0, in this order (what the role-1 wave added in its registers before the epilogues shared an
    // interval: the images stay bit for bit). Twelve 16-byte stores from the lanes g == 0; one colour at a time (24 live registers).
    auto finish_rgb = [&]() {
        const int lane = fresh_lane();
        const int n16 = lane & 15;
        if (lane < 16) {
            const f32x4* const x0 = reinterpret_cast<const f32x4*>(rgb_xchg) + (pg * 12) * 16 + n16;
            const f32x4* const x1 = x0 + kRgbXchgFloats / 4;
            float* const y_base = p.rgb_y + rgb_off + (size_t)(4 * (pg * kTR + n16 / kTC)) * p.OW + 4 * (n16 % kTC);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int oy = 0; oy < 4; ++oy)
                    *reinterpret_cast<f32x4*>(y_base + ((size_t)c * p.OH + oy) * p.OW) = x1[(c * 4 + oy) * 16] + x0[(c * 4 + oy) * 16];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // ---- ring prologue: the first two chunks of the stream, all pieces at once ----
    for (int c = 0; c < kNBUF - 1; ++c) {
        stage_begin();
        if (cur_valid) {
#pragma unroll
            for (int r = 0; r < kPiecesPerWave; ++r) stage_piece(r);
        }
    }

    // ---- the stream: k-step G of the block multiplies chunk G (chunk G % n of tile G / n), ring slot G % 3 ----
    // The two waves of a SIMD run half a k-step apart: in the interval between two barriers the role-0 wave loads and
    // transforms chunk G and then multiplies it, the role-1 wave first multiplies chunk G - 1 out of its registers and then
    // loads and transforms chunk G. While one of them waits for LDS or issues vector instructions the other keeps the
    // matrix pipe busy.
    // Tile boundaries. BOTH epilogues of a tile run in the first interval of the NEXT tile (interval B), while the ring keeps
    // fetching: the role-1 wave multiplies the tile's last chunk there, which it has in registers, and runs its epilogue behind
    // it; the role-0 wave, whose last multiply ended the interval before, has DEFERRED its epilogue to the top of interval B, in
    // front of the next tile's first load + transform + multiply (its accumulators are dead until that multiply's C = 0, V / A
    // until the load). So the two epilogues run beside each other and beside a multiply, not one after the other with the partner
    // parked at the barrier. The block's last tile has no interval B: both waves run its epilogue behind the stream's last
    // barrier, again side by side. What this order relies on:
    //  * the constants of tile t (set t & 1) are overwritten by those of tile t + 2, which are issued with that tile's first
    //    chunk in interval n - 2 of tile t + 1; both epilogues of tile t end in interval 0 of tile t + 1: n - 2 >= 2 > 0
    //    (winograd43_supported demands n >= 4);
    //  * (RGB) the sums both waves leave in rgb_xchg in interval B are added and stored by the role-0 wave at the top of
    //    interval B + 1 (finish_rgb), or behind one trailing barrier that both roles execute for the block's last tile.
    // Shape of the loops: tiles outside, their chunks inside, the epilogue UNCONDITIONALLY behind the inner loop, one nest per
    // role: accumulators that flow through a conditional (an epilogue under `if` inside one loop) cost 244 spilled
    // registers here; do-while because the guard path of a `for` (all accumulators zero) meets the real path in front of the
    // epilogue and costs accumulator copies. For the same reason the role-0 nest is rotated by one k-step (the first tile's first
    // k-step is peeled): the next tile's first multiply follows the epilogue unconditionally -- behind the block's last tile it
    // multiplies stale operands into dead accumulators, 36 MFMAs per block -- and only the barrier and the load around it are
    // conditional, as in the role-1 nest.
    int slot = 0, G = 0;
    // Opens interval G: chunk G must have landed. vmcnt counts in issue order, so the wait may leave in flight whatever this
    // wave issued BEHIND chunk G's pieces: always the five pieces of chunk G + 1, and `stores` stores of an epilogue:
    //  * kStoresPerEpilogue at the open of interval B + 1, both roles, in the launches that store activations (p.out: every
    //    layer but the 1024^2 one, which only feeds ToRGB and issues none -- there the count is the plain five). The epilogue's
    //    stores go out in interval B; role 0: [chunk B + 1: interval B - 1] < stores < [chunk B + 2: this multiply];
    //    role 1: [chunk B + 1] < [chunk B + 2: the multiply in front of the epilogue] < stores. Either way 16 + 5 are younger
    //    than chunk B + 1;
    //  * kRgbStores at the open of interval B + 2, role 0, RGB: finish_rgb stores at the top of interval B + 1,
    //    [chunk B + 2: interval B] < 12 stores < [chunk B + 3: interval B + 1's multiply]; the activation stores of interval B
    //    are older than chunk B + 2 there and are waited for (issued more than an interval earlier);
    //  * 0 everywhere else (role 1 at B + 2 waits for its activation stores of interval B, which are younger than chunk B + 2:
    //    stricter than needed, as it has always been, and more than an interval old).
    auto open_interval = [&](int stores) {
        if (G + 1 >= total)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (stores == kStoresPerEpilogue)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPiecesPerWave + kStoresPerEpilogue) : "memory");
        else if (stores == kRgbStores)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPiecesPerWave + kRgbStores) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kPiecesPerWave) : "memory");
        if (!(GANCE_W43_ABLATE & 16)) __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        stage_begin();  // chunk G + 2 -> the slot k-step G - 1 read (every wave is past the barrier: nobody reads it any more)
        __builtin_amdgcn_sched_barrier(0);
    };
    auto close_interval = [&]() {
        __builtin_amdgcn_sched_barrier(0);
        slot = slot == kNBUF - 1 ? 0 : slot + 1;
        ++G;
    };
    const int act_stores = p.out != nullptr ? kStoresPerEpilogue : 0;  // (wave-uniform)
    if (role == 0) {
        lane_setup();  // (again, per nest: per-lane values shared by the two nests are live to the common tail and cost a spilled register)
        open_interval(0);  // interval 0 of the block's first tile
        load_transform(slot);
        __builtin_amdgcn_sched_barrier(0);
        multiply(std::true_type{});
        close_interval();
        int tile = 0;
        // what a tile boundary leaves to the two intervals behind it: the stores their opens may leave in flight (carried as state,
        // not derived from q: hipcc then peels those two trips of the inner loop, and the peeled copies spill accumulators)
        int stores = 0, stores_next = 0;
        do {
            int q = 1;
            do {  // intervals 1 .. n - 1 of the tile
                open_interval(stores);
                if constexpr (RGB) {
                    if (stores_next != 0) finish_rgb();  // (interval B + 1, in front of this interval's five pieces)
                }
                stores = stores_next;
                stores_next = 0;
                asm volatile("" : "+s"(stores), "+s"(stores_next));  // (opaque: values that settle after two trips make hipcc peel two trips)
                load_transform(slot);
                __builtin_amdgcn_sched_barrier(0);
                multiply(std::false_type{});
                close_interval();
            } while (++q < n);
            // interval 0 of the next tile, if there is one: this tile's epilogue first
            const bool more = tile + 1 < my_tiles;
            if (more)
                open_interval(0);
            else
                cur_valid = false;
            epilogue(tile);
            stores = act_stores;
            stores_next = RGB ? kRgbStores : 0;
            if (more) {
                load_transform(slot);
            } else {  // (operands of a multiply nobody reads: left undefined, so that the old ones are not kept across the epilogue)
#pragma unroll
                for (int k = 0; k < 36; ++k) asm volatile("" : "=v"(V[k]), "=v"(A[k]));
            }
            __builtin_amdgcn_sched_barrier(0);
            multiply(std::true_type{});
            if (more) close_interval();
        } while (++tile < my_tiles);
    } else {
        lane_setup();
        open_interval(0);  // interval 0: nothing to multiply yet; this interval's DMA pieces go out in one burst
        if (cur_valid) {
#pragma unroll
            for (int r = 0; r < kPiecesPerWave; ++r) stage_piece(r);
        }
        load_transform(slot);
        close_interval();
        int tile = 0;
        do {
            open_interval(tile > 0 ? act_stores : 0);
            multiply(std::true_type{});  // chunk 0 of the tile
            __builtin_amdgcn_sched_barrier(0);
            load_transform(slot);
            close_interval();
            int q = 2;
            do {
                open_interval(0);
                multiply(std::false_type{});
                __builtin_amdgcn_sched_barrier(0);
                load_transform(slot);
                close_interval();
            } while (++q < n);
            // the tile's last chunk: multiplied in the first interval of the next tile (if there is one), then the epilogue,
            // then that interval's own load + transform
            const bool more = tile + 1 < my_tiles;
            if (more)
                open_interval(0);
            else
                cur_valid = false;
            multiply(std::false_type{});
            __builtin_amdgcn_sched_barrier(0);
            epilogue(tile);
            if (more) {
                load_transform(slot);
                close_interval();
            }
        } while (++tile < my_tiles);
    }
    if constexpr (RGB) {  // the sums of the block's last tile: in LDS, from both roles, behind one more barrier
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (role == 0) finish_rgb();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing of the ring may still be landing when the block's LDS is given back
}

// (plain functions around the templated body: as a kernel TEMPLATE the host pass of hipcc drops the instantiation, see winograd64_conv.hip)
__global__ __launch_bounds__(512, 1) void winograd43_kernel(const ConvArgs p) { winograd43_body<false, 64>(p); }
__global__ __launch_bounds__(512, 1) void winograd43_rgb_kernel(const ConvArgs p) { winograd43_body<true, 64>(p); }
__global__ __launch_bounds__(512, 1) void winograd43_w32_kernel(const ConvArgs p) { winograd43_body<false, 32>(p); }
__global__ __launch_bounds__(512, 1) void winograd43_w32_rgb_kernel(const ConvArgs p) { winograd43_body<true, 32>(p); }

bool winograd43_supported(int cin, int cout, int H, int W) {
    // (>= 4 chunks per tile: a tile's constant set and the ToRGB buffers are written again n - 2 / n intervals behind the interval
    // that holds the previous tile's two epilogues -- see the stream loop). Pixel tiles of 16 x 64, or 32 x 32 on the 32-pixel-wide layer.
    return cin % kKC == 0 && cin / kKC >= 4 && cout % kBM == 0 && ((W % 64 == 0 && H % 16 == 0) || (W == 32 && H % 32 == 0));
}

size_t winograd43_weight_floats(int cin, int cout) { return (size_t)(cout / kBM) * (cin / kKC) * kWFloats; }

bool winograd43_rgb_supported(int cout) { return winograd64_rgb_supported(cout); }  // (shares launch_winograd64_rgb_coef's table: Cout = 32 or a multiple of 64)
int winograd43_rgb_partials(int cout) { return cout / kBM; }

// w_in: the layer's runtime-scaled weights [tap = ky*3+kx][ci][co]; w_out: [m tile of 32][chunk of 4][channel tile][ci][co % 16][36],
// position j * 6 + i = (G g G^T)[i][j], i along y
void winograd43_transform_weights(const float* w_in, int cin, int cout, float* w_out) {
    const double G[6][3] = {{1. / 4, 0., 0.},          {-1. / 6, -1. / 6, -1. / 6}, {-1. / 6, 1. / 6, -1. / 6},
                            {1. / 24, 1. / 12, 1. / 6}, {1. / 24, -1. / 12, 1. / 6}, {0., 0., 1.}};
    const int chunks = cin / kKC;
    std::fill(w_out, w_out + winograd43_weight_floats(cin, cout), 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci) {
            double gk[3][3], tmp[6][3], u[6][6];
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) gk[ky][kx] = w_in[((size_t)(ky * 3 + kx) * cin + ci) * cout + co];
            for (int i = 0; i < 6; ++i)
                for (int kx = 0; kx < 3; ++kx) tmp[i][kx] = G[i][0] * gk[0][kx] + G[i][1] * gk[1][kx] + G[i][2] * gk[2][kx];
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) u[i][j] = tmp[i][0] * G[j][0] + tmp[i][1] * G[j][1] + tmp[i][2] * G[j][2];
            const int mtile = co / kBM, m = co % kBM, ch = ci / kKC, kc = ci % kKC;
            float* dst = w_out + ((size_t)mtile * chunks + ch) * kWFloats + ((m / 16) * 4 + kc) * kUnit + (m % 16) * 36;
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) dst[j * 6 + i] = (float)u[i][j];
        }
}

hipError_t launch_winograd43_conv(const ConvArgs& args, hipStream_t stream) {
    const bool rgb = args.epilogue == kEpilogueFullRgbPart;
    if (!winograd43_supported(args.Cin, args.Cout, args.H, args.W)) return hipErrorInvalidValue;
    if (rgb ? (!winograd43_rgb_supported(args.Cout) || args.rgb_coef == nullptr || args.rgb_y == nullptr) : (args.epilogue != kEpilogueFull || args.out == nullptr))
        return hipErrorInvalidValue;
    // (the epilogue's stores address a tile's 16 channels x 16 rows with 32-bit byte offsets from the tile's origin)
    if (args.out != nullptr && (args.out_c_stride <= 0 || args.out_row_stride <= 0 || 16 * args.out_c_stride + 16 * (long long)args.out_row_stride + 64 >= (1ll << 29)))
        return hipErrorInvalidValue;
    const bool narrow = args.W % 64 != 0;  // the 32 x 32 pixel geometry
    void (*const kernel)(const ConvArgs) = narrow ? (rgb ? winograd43_w32_rgb_kernel : winograd43_w32_kernel) : (rgb ? winograd43_rgb_kernel : winograd43_kernel);
    const int tw = narrow ? 32 : 64, th = 1024 / tw;
    const size_t lds_bytes = sizeof(float) * ((size_t)kNBUF * (narrow ? Geo43<32>::kSlot : Geo43<64>::kSlot) + 2 * kConstFloats + (rgb ? 2 * kRgbXchgFloats : 0));
    // (154.5 KB / 157.5 KB with both ToRGB buffers, + 16 bytes of tickets, of the CU's 160 KB)
    static_assert(sizeof(float) * (kNBUF * std::max(Geo43<32>::kSlot, Geo43<64>::kSlot) + 2 * kConstFloats + 2 * kRgbXchgFloats) + 64 <= 160 * 1024,
                  "ring + tile constants + ToRGB buffers must fit the LDS of a CU");
    static PerDeviceInt resident[4];  // per device: the dynamic-LDS opt-in and the launch size = one block per CU, a multiple of 8 (XCDs)
    int resident_blocks = 0;
    hipError_t e = resident[(narrow ? 2 : 0) + (rgb ? 1 : 0)].get(
        [&](int device, int* value) {
            hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (err != hipSuccess) return err;
            int cus = 0;
            if ((err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return err;
            *value = std::max(8, cus / 8 * 8);
            return hipSuccess;
        },
        &resident_blocks);
    if (e != hipSuccess) return e;
    ConvArgs a = args;
    a.tiles_x = a.W / tw;
    a.tiles_y = a.H / th;
    a.m_tiles = a.Cout / kBM;
    a.total_chunks = a.Cin / kKC;
    a.total_tiles = a.m_tiles * a.tiles_x * a.tiles_y * a.B;
    const auto log2_exact = [](int v) { return v > 0 && (v & (v - 1)) == 0 ? __builtin_ctz((unsigned)v) : -1; };
    const int shm = log2_exact(a.m_tiles), shx = log2_exact(a.tiles_x), shy = log2_exact(a.tiles_y);
    a.tile_shifts = shm >= 0 && shx >= 0 && shy >= 0 ? shm | shx << 8 | shy << 16 : -1;  // (-1: the kernel divides)
    if ((a.tiles_x * a.tiles_y * a.B) % 4 != 0) a.xcd_blocking = 0;  // (the 4 x 8 blocking walks pixel tiles four at a time)
    // blocks per CU (ConvArgs::grid_rounds), as long as a block's stream stays long beside its ring prologue (about two k-steps):
    // at least 64 k-steps per block, else fewer, larger blocks (one frame per call: one block per CU as before)
    int rounds = std::max(1, a.grid_rounds);
    const int min_tiles = std::max(1, 64 / a.total_chunks);
    while (rounds > 1 && a.total_tiles < resident_blocks * rounds * min_tiles) --rounds;
    hipLaunchKernelGGL(kernel, dim3(std::min(a.total_tiles, resident_blocks * rounds)), dim3(512), lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace gance
