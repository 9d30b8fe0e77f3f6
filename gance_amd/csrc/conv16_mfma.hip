// Direct-form modulated 3x3 convolution for layers with 16 output channels (the 1024^2 layers of a config-e generator:
// Conv0_up 32 -> 16 and Conv1 16 -> 16), on v_mfma_f32_16x16x4_f32: M = 16 is the whole Cout, so one wave holds every
// output channel of its 16 pixels and the last layer's ToRGB (16 -> 3) is a sum inside the wave.
//
// Same formulation, argument struct, weight image and tap tables as conv_mfma.hip (whose 32x32x2 template needs BM to be a
// multiple of 32):   out[b,co,p] = d[b,co] * sum_{tap,ci} w[tap,ci,co] * (s[b,ci] * x[b,ci,p+tap])
// with the style multiplied into the input patch as it is staged and the demodulation in the epilogue. The weights are
// conv_mfma.hip's direct image [chunk of 16][tap slot 0..8][16 ci][16 co], slot t of a transposed conv = filter tap
// kUpTapWeight[t] (engine.hip).
//
// One block = 4 waves = a tile of TH x TW output pixels (UP: positions of the (H+1) x (W+1) grid, all four parity classes)
// of one sample. Per chunk of 16 input channels the block stages the tile's haloed patch (times the style) and the chunk's
// weights in LDS, then every wave walks its TH * TW / 64 groups of 16 consecutive pixels: one A fragment (weights) per
// (tap, 4 channels) serves all of them, one ds_read_b32 per MFMA fetches the B fragment. Two or more blocks per CU overlap
// one block's staging with another's MFMAs; nothing is pipelined inside a block (the layer is bound by the matrix pipe:
// DESIGN.md section 3).
//
// MFMA layout (16x16x4 f32): A[m][k] sits in lane 16 k + m, B[k][n] in lane 16 k + n, D[m][n] in lane 16 (m / 4) + n,
// register m % 4: a lane holds four channels of one pixel.

#include <hip/hip_runtime.h>

#include "kernels.h"

namespace gance {

typedef float f32x4_16 __attribute__((ext_vector_type(4)));

namespace {

// transposed conv: 9 (class, dy, dx) entries in the order of conv_mfma.hip's tap tables
// EE (0,0) (0,-1) (-1,0) (-1,-1) | EO (0,0) (-1,0) | OE (0,0) (0,-1) | OO (0,0)
__host__ __device__ constexpr int up16_cls(int t) { return t < 4 ? 0 : (t < 6 ? 1 : (t < 8 ? 2 : 3)); }
__host__ __device__ constexpr int up16_dy(int t) { return (t == 2 || t == 3 || t == 5) ? -1 : 0; }
__host__ __device__ constexpr int up16_dx(int t) { return (t == 1 || t == 3 || t == 7) ? -1 : 0; }

template <int TH, int TW, bool UP>
struct Conv16Tile {
    static constexpr int kKC = 16;                 // input channels per LDS stage
    static constexpr int kRowGroups = TW / 16;     // 16-pixel groups per tile row
    static constexpr int kGroups = TH * kRowGroups;
    static constexpr int kGW = kGroups / 4;        // groups per wave
    static constexpr int kCls = UP ? 4 : 1;
    // the patch: padded input rows y0 .. y0 + kPH - 1, padded columns x0 .. x0 + kPW - 1 (padded = image + (1, 4))
    static constexpr int kPH = UP ? TH + 1 : TH + 2;
    static constexpr int kPW = UP ? TW + 4 : TW + 8;
    // plane stride = 16 mod 64: the four k planes of a B fragment fall on disjoint quarters of the LDS banks
    static constexpr int kPlane = (kPH * kPW + 47) / 64 * 64 + 16;
    static constexpr int kWFloats = 9 * kKC * 16;
    static_assert(TW % 16 == 0 && kGroups % 4 == 0 && kPW % 4 == 0 && kPlane >= kPH * kPW, "tile geometry");
};

template <int TH, int TW, bool UP>
__global__ __launch_bounds__(256, UP ? 2 : 4) void modconv16_kernel(const ConvArgs p) {
    using T = Conv16Tile<TH, TW, UP>;
    constexpr int GW = T::kGW, PW = T::kPW, PH = T::kPH, PLANE = T::kPlane, NCLS = T::kCls;
    __shared__ __attribute__((aligned(16))) float patch[T::kKC * PLANE];
    __shared__ __attribute__((aligned(16))) float wl[T::kWFloats];

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int l15 = lane & 15;
    const int lq = lane >> 4;  // the k row of an operand fragment / the channel quarter of an accumulator

    int id = blockIdx.x;
    const int tile_x = id % p.tiles_x;
    id /= p.tiles_x;
    const int tile_y = id % p.tiles_y;
    const int b = min(id / p.tiles_y, p.B - 1);
    const int y0 = tile_y * TH, x0 = tile_x * TW;
    const int Hp = p.H + 2, Wp = p.W + 8;
    const float* const xb = p.x + (size_t)b * p.x_b_stride;
    const float* const sb = p.s + (size_t)b * p.s_stride;

    f32x4_16 acc[NCLS][GW];
#pragma unroll
    for (int c = 0; c < NCLS; ++c)
#pragma unroll
        for (int g = 0; g < GW; ++g) acc[c][g] = f32x4_16{0.f, 0.f, 0.f, 0.f};

    // patch offset of each group's pixel (its (0, 0) tap sits at + (1, 4) of the padded tile origin)
    int boff[GW];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int G = wave * GW + g;
        boff[g] = lq * PLANE + (G / T::kRowGroups + 1) * PW + (G % T::kRowGroups) * 16 + l15 + 4;
    }

    const int chunks = p.Cin / T::kKC;
    for (int chunk = 0; chunk < chunks; ++chunk) {
        if (chunk > 0) __syncthreads();  // the previous chunk's fragments have been read
        const int ci0 = chunk * T::kKC;
        // the patch [16 ci][PH][PW] times the style, as float4s; rows and columns past the padded tensor (edge tiles of the
        // position grid) repeat its last ones: only masked outputs read them
        // (every load of the chunk is issued before the first LDS write: one memory round trip per chunk, not one per float4)
        constexpr int kPatchF4 = T::kKC * PH * (PW / 4), kPatchTrips = (kPatchF4 + 255) / 256, kWTrips = (T::kWFloats / 4 + 255) / 256;
        float4 pv[kPatchTrips], wv[kWTrips];
        float psv[kPatchTrips];
        const float4* const wsrc = reinterpret_cast<const float4*>(p.w + (size_t)chunk * T::kWFloats);
#pragma unroll
        for (int i = 0; i < kPatchTrips; ++i) {
            const int f = min(tid + 256 * i, kPatchF4 - 1);  // (tail threads repeat the last float4 and do not write it)
            const int q = f % (PW / 4);
            const int py = (f / (PW / 4)) % PH;
            const int c = f / ((PW / 4) * PH);
            const int gy = min(y0 + py, Hp - 1), gx = min(x0 + 4 * q, Wp - 4);
            pv[i] = *reinterpret_cast<const float4*>(xb + ((size_t)(ci0 + c) * Hp + gy) * Wp + gx);
            psv[i] = sb[ci0 + c];
        }
#pragma unroll
        for (int i = 0; i < kWTrips; ++i) wv[i] = wsrc[min(tid + 256 * i, T::kWFloats / 4 - 1)];
#pragma unroll
        for (int i = 0; i < kPatchTrips; ++i) {
            const int f = tid + 256 * i;
            if (f < kPatchF4) {
                const int q = f % (PW / 4);
                const int py = (f / (PW / 4)) % PH;
                const int c = f / ((PW / 4) * PH);
                const float sv = psv[i];
                *reinterpret_cast<float4*>(patch + c * PLANE + py * PW + 4 * q) = make_float4(pv[i].x * sv, pv[i].y * sv, pv[i].z * sv, pv[i].w * sv);
            }
        }
#pragma unroll
        for (int i = 0; i < kWTrips; ++i)
            if (tid + 256 * i < T::kWFloats / 4) reinterpret_cast<float4*>(wl)[tid + 256 * i] = wv[i];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // stride 1: tap t = ky * 3 + kx reads (y + ky - 1, x + kx - 1); transposed: slot t reads (y' + dy, x' + dx)
            const int shift = UP ? up16_dy(t) * PW + up16_dx(t) : (t / 3 - 1) * PW + (t % 3 - 1);
            constexpr int kNoCls = 0;
            const int cls = UP ? up16_cls(t) : kNoCls;
#pragma unroll
            for (int kq = 0; kq < T::kKC / 4; ++kq) {
                const float a = wl[t * (T::kKC * 16) + kq * 64 + lane];
#pragma unroll
                for (int g = 0; g < GW; ++g) {
                    const float bv = patch[boff[g] + kq * 4 * PLANE + shift];
                    acc[cls][g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, acc[cls][g], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: a lane holds channels 4 lq + r (r = 0..3) of its pixel ----
    float dv[4], bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dv[r] = p.d[(size_t)b * p.d_stride + 4 * lq + r];
        bias[r] = p.bias[4 * lq + r];
    }
    if (!UP && p.epilogue == kEpilogueRgb) {
        // last layer: activation -> ToRGB -> + upsampled skip image + bias -> fp32 image (if asked for) and uint8 NHWC
        const int R = p.OW, Rh = R >> 1;
        float coef[4][3];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sv = p.rgb_s[(size_t)b * p.s_stride + 4 * lq + r];
#pragma unroll
            for (int k = 0; k < 3; ++k) coef[r][k] = sv * p.rgb_w[(4 * lq + r) * 3 + k];
        }
        // the noise values and the lane's tap of the upsampled skip image of every group, fetched together ahead of the arithmetic:
        // upsample_2d per axis is (odd o: .75, .25) of sources (o >> 1, + 1), (even: .25, .75) of ((o >> 1) - 1, o >> 1), zero outside;
        // each lane quarter takes one of its pixel's four taps, the quarters join in the channel sum's exchange
        float nzv[GW], skip[GW][3];
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            const int G = wave * GW + g;
            const int oy = y0 + G / T::kRowGroups, ox = x0 + (G % T::kRowGroups) * 16 + l15;
            const bool ok = oy < p.OH && ox < p.OW;
            nzv[g] = (p.noise != nullptr && ok) ? p.noise[(size_t)b * p.noise_b_stride + (size_t)oy * p.OW + ox] : 0.f;
            const int row = ((oy & 1) ? (oy >> 1) : (oy >> 1) - 1) + (lq & 1);
            const int col = ((ox & 1) ? (ox >> 1) : (ox >> 1) - 1) + (lq >> 1);
            const float wrow = ((oy & 1) != 0) == ((lq & 1) == 0) ? 0.75f : 0.25f;
            const float wcol = ((ox & 1) != 0) == ((lq >> 1) == 0) ? 0.75f : 0.25f;
            const bool tap_ok = p.rgb_y_prev != nullptr && ok && row >= 0 && row < Rh && col >= 0 && col < Rh;
            const float* const yp = p.rgb_y_prev + (size_t)b * 3 * Rh * Rh + (size_t)max(row, 0) * Rh + max(col, 0);
#pragma unroll
            for (int k = 0; k < 3; ++k) skip[g][k] = tap_ok ? wrow * wcol * yp[(size_t)k * Rh * Rh] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < GW; ++g) {
            const int G = wave * GW + g;
            const int oy = y0 + G / T::kRowGroups, ox = x0 + (G % T::kRowGroups) * 16 + l15;
            const bool ok = oy < p.OH && ox < p.OW;
            const size_t pix = (size_t)oy * R + ox;
            const float nz = nzv[g] * p.noise_strength;
            float rgb[3] = {skip[g][0], skip[g][1], skip[g][2]};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[0][g][r] * dv[r];
                v += nz + bias[r];
                v = fmaxf(v, 0.2f * v) * 1.4142135623730951f;  // lrelu(0.2) * sqrt(2)
#pragma unroll
                for (int k = 0; k < 3; ++k) rgb[k] = fmaf(v, coef[r][k], rgb[k]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                rgb[k] += __shfl_xor(rgb[k], 16);
                rgb[k] += __shfl_xor(rgb[k], 32);
            }
            unsigned packed = 0;  // this pixel's three bytes (the same in all four lanes of the pixel)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float y = rgb[k] + p.rgb_bias[k];
                if (p.rgb_y != nullptr && lq == 0 && ok) p.rgb_y[((size_t)b * 3 + k) * R * R + pix] = y;
                // tf.saturate_cast(x * 127.5 + 128): two roundings (the barrier keeps them apart)
                float q = y * 127.5f;
                asm volatile("" : "+v"(q));
                q += 128.0f;
                q = fminf(fmaxf(q, 0.f), 255.f);
                packed |= (unsigned)(int)q << (8 * k);
            }
            // 16 pixels x 3 bytes = 12 dwords, contiguous in the NHWC frame: lane t < 12 assembles dword t from the packed
            // pixels floor(4t/3) and floor(4t/3) + 1 (R is a multiple of the tile width: a group is whole or absent)
            const int first = (4 * l15) / 3, skew = (4 * l15) % 3;
            const unsigned lo = __shfl(packed, first), hi = __shfl(packed, min(first + 1, 15));
            const unsigned word = skew == 0 ? (lo | (hi << 24)) : (skew == 1 ? ((lo >> 8) | (hi << 16)) : ((lo >> 16) | (hi << 8)));
            const bool group_ok = oy < p.OH && (ox - l15) + 15 < p.OW;
            if (p.rgb_u8 != nullptr && lane < 12 && group_ok)
                reinterpret_cast<unsigned*>(p.rgb_u8 + ((size_t)b * R * R + (pix - l15)) * 3)[lane] = word;
        }
        return;
    }
    const bool full = !UP && p.epilogue == kEpilogueFull;
    float* const out_b = p.out + (size_t)b * p.out_b_stride + (size_t)(4 * lq) * p.out_c_stride;
    float nzf[GW];
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int G = wave * GW + g;
        const int oy = y0 + G / T::kRowGroups, ox = x0 + (G % T::kRowGroups) * 16 + l15;
        nzf[g] = (full && p.noise != nullptr && oy < p.OH && ox < p.OW) ? p.noise[(size_t)b * p.noise_b_stride + (size_t)oy * p.OW + ox] : 0.f;
    }
#pragma unroll
    for (int g = 0; g < GW; ++g) {
        const int G = wave * GW + g;
        const int oy = y0 + G / T::kRowGroups, ox = x0 + (G % T::kRowGroups) * 16 + l15;
        const size_t at = (size_t)(oy + p.out_y_off) * p.out_row_stride + ox + p.out_x_off;
        const float nz = nzf[g] * p.noise_strength;
#pragma unroll
        for (int c = 0; c < NCLS; ++c) {
            // class c = (py, px): valid positions shrink by one where the parity is odd
            if (!(oy < p.OH - (UP ? (c >> 1) : 0) && ox < p.OW - (UP ? (c & 1) : 0))) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[c][g][r] * dv[r];
                if (full) {
                    v += nz + bias[r];
                    v = fmaxf(v, 0.2f * v) * 1.4142135623730951f;
                }
                out_b[(size_t)c * p.cls_stride + (size_t)r * p.out_c_stride + at] = v;
            }
        }
    }
}

}  // namespace

hipError_t launch_modconv16(int tile_id, const ConvArgs& a, int total_blocks, hipStream_t stream) {
    const ConvTileInfo& t = kConvTiles[tile_id];
    // one channel tile, no split-K, whole 16-channel chunks; the fused ToRGB only on a stride-1 layer whose width the tiles cover exactly
    if (t.BM != 16 || a.Cout != 16 || a.Cin % 16 != 0 || a.m_tiles != 1 || a.nsplit != 1 || total_blocks != a.tiles_x * a.tiles_y * a.B)
        return hipErrorInvalidValue;
    if (a.epilogue == kEpilogueRgb && (t.up || a.OW % t.TW != 0 || a.OH % t.TH != 0)) return hipErrorInvalidValue;
    if (a.epilogue != kEpilogueRgb && a.epilogue != kEpilogueFull && a.epilogue != kEpilogueRaw) return hipErrorInvalidValue;
    if (t.up)
        hipLaunchKernelGGL((modconv16_kernel<8, 32, true>), dim3(total_blocks), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL((modconv16_kernel<4, 64, false>), dim3(total_blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace gance
