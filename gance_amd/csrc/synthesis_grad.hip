// Differentiable synthesis: the plain-form forward and backward kernels behind torch.ops.gance.modconv3x3,
// noise_bias_lrelu and torgb_skip (gance_amd/torch_ops.py, gance_amd/stylegan2/differentiable.py).
// A second path through the generator's arithmetic beside the engine's: activations are stored as the published network
// defines them (not pre-multiplied by the next style), every layer has one form whatever the batch, and every kernel is
// fp32 NCHW on the caller's stream, without host synchronisation and without floating-point atomics: every sum has one
// order, so two runs give the same bits.
//
// The two contractions of a modulated 3x3 conv are ONE kernel (contract_kernel), on v_mfma_f32_16x16x4_f32:
//
//     out[b, m, oy, ox] = post[b, m] * sum_{tap = (ty, tx), k} W(tap, k, m) * pre[b, k] * IN[b, k, oy * os + ty - pad, ox * os + tx - pad]
//
// where IN is the stored input, zero outside it, or (zero_insert) the input with a zero between every two values:
//
//     forward, stride 1    IN = x        pre = style  post = demod  W(tap, k, m) = w[tap][k][m]       os 1  pad 1
//     forward, up          IN = x, zero-inserted      pre = style  post = demod  w[tap][k][m]         os 1  pad 2   -> (2H+1)^2, then the FIR
//     backward data        IN = grad_y   pre = demod  post = none   W(tap, k, m) = w[8 - tap][m][k]   os 1  pad 1
//     backward data, up    IN = FIR^T(grad_y) (2H+1)^2  pre = demod  post = none  w[8 - tap][m][k]    os 2  pad 0
//
// The transposed stride-2 conv of the published upsample_conv_2d is a stride-1 conv of the zero-inserted input with the
// filter as stored (conv_transpose of the flipped filter un-flips it); three quarters of its products are zeros, which is
// the price of one kernel for every layer. The backward-data result is left WITHOUT the style: grad_style[b, i] =
// sum_pos x * g needs it that way (a style may be zero), and the same pass that takes that sum writes grad_x = g * style.
//
// MFMA layout (16x16x4 f32): A[m][k] sits in lane 16 k + m, B[k][n] in lane 16 k + n, D[m][n] in lane 16 (m / 4) + n,
// register m % 4. A block is 4 waves = 64 consecutive pixels (row-major over the output) x 16 MT output channels of one
// sample; per chunk of 16 contracted channels it stages the chunk's weights [tap][k][m] in LDS (the transposition of the
// backward form happens there) and every lane fetches its own B values from global memory, zero where the tap falls outside.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_sgrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMinSide = 4, kMaxSide = 1024, kMaxChannels = 512, kMaxBatch = 65535;
constexpr int kMaxSegments = 64;         // partial sums per plane of a position sum
constexpr int kSegmentPositions = 4096;  // positions per partial sum (until kMaxSegments is reached)

struct ContractArgs {
    const float* in;    // [B][K][IH][IW]
    const float* w;     // [9][w_cin][w_cout], runtime-scaled
    const float* pre;   // [B][K]
    const float* post;  // [B][M] or nullptr
    float* out;         // [B][M][OH][OW]
    int K, M;           // contracted and produced channels
    int w_cin, w_cout;
    int transposed;     // 0: W(tap, k, m) = w[tap][k][m]; 1: W(tap, k, m) = w[8 - tap][m][k]
    int IH, IW, OH, OW;
    int out_stride, pad, zero_insert;
};

template <int MT>
__global__ __launch_bounds__(kThreads) void contract_kernel(const ContractArgs p) {
    // row stride = 16 mod 64 (or 16 itself): the four k rows of an A fragment fall on disjoint quarters of the LDS banks
    constexpr int ROW = MT == 1 ? 16 : 16 * MT + 16;
    __shared__ float wl[9 * 16 * ROW];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.z, m0 = blockIdx.y * 16 * MT;
    const int pixels = p.OH * p.OW;
    const int pix = blockIdx.x * 64 + wave * 16 + l15;
    const bool pix_ok = pix < pixels;
    const int oy = pix / p.OW, ox = pix - oy * p.OW;

    // the lane's input offset of every tap (-1: the tap reads a zero)
    int off[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        int iy = oy * p.out_stride + t / 3 - p.pad, ix = ox * p.out_stride + t % 3 - p.pad;
        bool ok = pix_ok && iy >= 0 && ix >= 0;
        if (p.zero_insert) {
            ok = ok && (iy & 1) == 0 && (ix & 1) == 0;
            iy >>= 1;
            ix >>= 1;
        }
        ok = ok && iy < p.IH && ix < p.IW;
        off[t] = ok ? iy * p.IW + ix : -1;
    }

    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const size_t in_plane = (size_t)p.IH * p.IW;
    for (int k0 = 0; k0 < p.K; k0 += 16) {
        if (k0 > 0) __syncthreads();  // the previous chunk's fragments have been read
        for (int e = tid; e < 9 * 16 * 16 * MT; e += kThreads) {
            const int m = e % (16 * MT), k = (e / (16 * MT)) % 16, t = e / (16 * MT * 16);
            const size_t src = p.transposed ? ((size_t)(8 - t) * p.w_cin + (m0 + m)) * p.w_cout + (k0 + k)
                                            : ((size_t)t * p.w_cin + (k0 + k)) * p.w_cout + (m0 + m);
            wl[(t * 16 + k) * ROW + m] = p.w[src];
        }
        __syncthreads();
        // a chunk's 144 products are summed on their own and then added to the total: blocked summation, whose rounding error
        // grows with the chunk count plus the chunk length instead of with their product (K up to 4608)
        f32x4 part[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) part[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            const int k = k0 + kq * 4 + lq;
            const float sv = p.pre[(size_t)b * p.K + k];
            const float* const plane = p.in + ((size_t)b * p.K + k) * in_plane;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float bv = off[t] >= 0 ? plane[off[t]] * sv : 0.f;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float a = wl[(t * 16 + kq * 4 + lq) * ROW + mt * 16 + l15];
                    part[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, part[mt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] += part[mt];
    }

    // a lane holds channels 4 lq + r (r = 0 .. 3) of each 16-channel tile, for its pixel
    if (!pix_ok) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + mt * 16 + 4 * lq + r;
            const float scale = p.post != nullptr ? p.post[(size_t)b * p.M + m] : 1.f;
            p.out[((size_t)b * p.M + m) * pixels + pix] = acc[mt][r] * scale;
        }
}

// the [1,3,3,1] FIR of upsample_conv_2d (gain 4, pads 1 and 1: [1,3,3,1] / 4 per axis): t [planes][T][T], T = S + 1 -> y [planes][S][S],
// y[oy][ox] = sum_{a,c} f[a] f[c] t[oy + a - 1][ox + c - 1], zero outside t
__global__ __launch_bounds__(kThreads) void fir_kernel(const float* __restrict__ t, float* __restrict__ y, int S, size_t total) {
    const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int T = S + 1;
    const int ox = (int)(at % S), oy = (int)((at / S) % S);
    const float* const plane = t + (at / ((size_t)S * S)) * ((size_t)T * T);
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int ty = oy + a - 1;
        if (ty < 0 || ty >= T) continue;
        float row = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int tx = ox + c - 1;
            if (tx >= 0 && tx < T) row += f[c] * plane[(size_t)ty * T + tx];
        }
        sum += f[a] * row;
    }
    y[at] = sum;
}

// its transpose: gy [planes][S][S] -> gt [planes][T][T], gt[ty][tx] = sum_{a,c} f[a] f[c] gy[ty - a + 1][tx - c + 1]
__global__ __launch_bounds__(kThreads) void fir_transpose_kernel(const float* __restrict__ gy, float* __restrict__ gt, int S, size_t total) {
    const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int T = S + 1;
    const int tx = (int)(at % T), ty = (int)((at / T) % T);
    const float* const plane = gy + (at / ((size_t)T * T)) * ((size_t)S * S);
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int oy = ty - a + 1;
        if (oy < 0 || oy >= S) continue;
        float row = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ox = tx - c + 1;
            if (ox >= 0 && ox < S) row += f[c] * plane[(size_t)oy * S + ox];
        }
        sum += f[a] * row;
    }
    gt[at] = sum;
}

// Position sums, in a fixed order: partial[plane][seg] = sum over the segment's positions of a * b (each thread its strided
// positions in rising order, then a tree over the block); with `scaled` (which may be `a` itself) it also receives
// a * scale[plane] (grad_x = g * style, in the pass that reads g anyway). plane_finish_kernel adds a plane's partials in rising order.
__global__ __launch_bounds__(kThreads) void plane_dot_kernel(const float* a, const float* __restrict__ b, const float* __restrict__ scale,
                                                             float* scaled, int positions, int segment, float* __restrict__ partial) {
    __shared__ float sums[kThreads];
    const int plane = blockIdx.x, seg = blockIdx.y;
    const size_t base = (size_t)plane * positions;
    const int first = seg * segment, last = min(first + segment, positions);
    const float sv = scaled != nullptr ? scale[plane] : 1.f;
    float sum = 0.f;
    for (int at = first + threadIdx.x; at < last; at += kThreads) {
        const float av = a[base + at];
        sum += av * b[base + at];
        if (scaled != nullptr) scaled[base + at] = av * sv;
    }
    sums[threadIdx.x] = sum;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) sums[threadIdx.x] += sums[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)plane * gridDim.y + seg] = sums[0];
}

__global__ __launch_bounds__(kThreads) void plane_finish_kernel(const float* __restrict__ partial, int segments, const float* __restrict__ divisor,
                                                                int planes, float* __restrict__ out) {
    const int plane = blockIdx.x * kThreads + threadIdx.x;
    if (plane >= planes) return;
    float sum = 0.f;
    for (int seg = 0; seg < segments; ++seg) sum += partial[(size_t)plane * segments + seg];
    out[plane] = divisor != nullptr ? sum / divisor[plane] : sum;
}

// act = lrelu_0.2(x + noise * strength + bias[c]) * sqrt(2); noise [noise_batch = 1 or B][1][H][W]
__global__ __launch_bounds__(kThreads) void noise_bias_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ noise, int noise_batch,
                                                                    const float* __restrict__ strength, const float* __restrict__ bias,
                                                                    int channels, int positions, size_t total, float* __restrict__ out) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const size_t pos = at % positions, plane = at / positions;
    const int c = (int)(plane % channels);
    const size_t b = plane / channels;
    const float v = x[at] + noise[(noise_batch > 1 ? b : 0) * positions + pos] * strength[0] + bias[c];
    out[at] = (v > 0.f ? v : 0.2f * v) * 1.4142135623730951f;
}

// leaky ReLU keeps the sign: the slope of a position is read off the saved output
__global__ __launch_bounds__(kThreads) void noise_bias_lrelu_backward_kernel(const float* __restrict__ grad_out, const float* __restrict__ out,
                                                                             size_t total, float* __restrict__ grad_x) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    grad_x[at] = grad_out[at] * ((out[at] > 0.f ? 1.f : 0.2f) * 1.4142135623730951f);
}

// noise_bias_lrelu_backward_kernel with the noise gradient in the same pass: grad_noise[n][pos] = strength * sum_{b of plane n} sum_c grad_x[b][c][pos]
// (a shared plane, noise_batch 1, sums over the batch too). A block is PX consecutive positions x G = kThreads / PX channel
// groups: thread (px, g) adds the channels g, g + G, ... of each sample in rising order, thread (px, 0) adds the G partial sums
// in rising order. PX is chosen by the shape alone (64, or 16 below 4096 positions, where 512 channels would otherwise sit
// in 16 ... 256 threads), so the order is a function of the shape and two runs give the same bits.
template <int PX>
__global__ __launch_bounds__(kThreads) void noise_bias_lrelu_backward_noise_kernel(const float* __restrict__ grad_out, const float* __restrict__ out,
                                                                                   const float* __restrict__ strength, int noise_batch, int batch,
                                                                                   int channels, int positions, float* __restrict__ grad_x,
                                                                                   float* __restrict__ grad_noise) {
    constexpr int G = kThreads / PX;
    __shared__ float part[kThreads];
    const int px = threadIdx.x % PX, g = threadIdx.x / PX;
    const int pos = blockIdx.x * PX + px;
    const int plane = blockIdx.y;
    const int b_first = noise_batch > 1 ? plane : 0, b_last = noise_batch > 1 ? plane + 1 : batch;
    float sum = 0.f;
    if (pos < positions)
        for (int b = b_first; b < b_last; ++b)
            for (int c = g; c < channels; c += G) {
                const size_t at = ((size_t)b * channels + c) * positions + pos;
                const float gx = grad_out[at] * ((out[at] > 0.f ? 1.f : 0.2f) * 1.4142135623730951f);
                grad_x[at] = gx;
                sum += gx;
            }
    part[g * PX + px] = sum;
    __syncthreads();
    if (g == 0 && pos < positions) {
        float total = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) total += part[k * PX + px];
        grad_noise[(size_t)plane * positions + pos] = total * strength[0];
    }
}

// y = upsample_2d(y_prev) + sum_i w[i][c] style[b][i] x[b][i] + bias[c]. upsample_2d per axis: output o reads the zero-inserted
// image z (z[2 j] = y_prev[j]) at o + a - 2 with [1,3,3,1] / 4 (gain 2 per axis, pads 2 and 1)
__global__ __launch_bounds__(kThreads) void torgb_skip_kernel(const float* __restrict__ x, const float* __restrict__ style, const float* __restrict__ w,
                                                              const float* __restrict__ bias, const float* __restrict__ y_prev, int cin, int side,
                                                              float* __restrict__ y) {
    __shared__ float coef[kMaxChannels * 3];
    const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    const int b = blockIdx.y;
    for (int e = threadIdx.x; e < cin * 3; e += kThreads) coef[e] = w[e] * style[(size_t)b * cin + e / 3];
    __syncthreads();
    const int positions = side * side;
    const int pos = blockIdx.x * kThreads + threadIdx.x;
    if (pos >= positions) return;
    float sum[3] = {0.f, 0.f, 0.f};
    const float* const xb = x + (size_t)b * cin * positions + pos;
    for (int i = 0; i < cin; ++i) {
        const float xv = xb[(size_t)i * positions];
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = fmaf(coef[i * 3 + c], xv, sum[c]);
    }
    float up[3] = {0.f, 0.f, 0.f};
    if (y_prev != nullptr) {
        const int half = side >> 1, oy = pos / side, ox = pos - oy * side;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int zy = oy + a - 2;
            if (zy < 0 || (zy & 1) != 0 || (zy >> 1) >= half) continue;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int zx = ox + d - 2;
                if (zx < 0 || (zx & 1) != 0 || (zx >> 1) >= half) continue;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    up[c] += f[a] * f[d] * y_prev[(((size_t)b * 3 + c) * half + (zy >> 1)) * half + (zx >> 1)];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) y[((size_t)b * 3 + c) * positions + pos] = up[c] + sum[c] + bias[c];
}

// g[b][i][pos] = sum_c w[i][c] grad_y[b][c][pos]: the ToRGB's backward data before the style (plane_dot_kernel applies it)
__global__ __launch_bounds__(kThreads) void torgb_backward_data_kernel(const float* __restrict__ grad_y, const float* __restrict__ w, int cin,
                                                                       int positions, float* __restrict__ g) {
    __shared__ float wl[kMaxChannels * 3];
    const int b = blockIdx.y;
    for (int e = threadIdx.x; e < cin * 3; e += kThreads) wl[e] = w[e];
    __syncthreads();
    const int pos = blockIdx.x * kThreads + threadIdx.x;
    if (pos >= positions) return;
    float gv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) gv[c] = grad_y[((size_t)b * 3 + c) * positions + pos];
    float* const gb = g + (size_t)b * cin * positions + pos;
    for (int i = 0; i < cin; ++i) gb[(size_t)i * positions] = fmaf(wl[i * 3 + 2], gv[2], fmaf(wl[i * 3 + 1], gv[1], wl[i * 3] * gv[0]));
}

// the transpose of upsample_2d: grad_y [planes][side][side] -> grad_y_prev [planes][side / 2][side / 2]; source j feeds the
// outputs 2 j + 2 - a with f[a]
__global__ __launch_bounds__(kThreads) void upsample_transpose_kernel(const float* __restrict__ grad_y, int side, size_t total,
                                                                      float* __restrict__ grad_y_prev) {
    const float f[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    const int half = side >> 1;
    const int sx = (int)(at % half), sy = (int)((at / half) % half);
    const float* const plane = grad_y + (at / ((size_t)half * half)) * ((size_t)side * side);
    float sum = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int oy = 2 * sy + 2 - a;
        if (oy < 0 || oy >= side) continue;
        float row = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int ox = 2 * sx + 2 - d;
            if (ox >= 0 && ox < side) row += f[d] * plane[(size_t)oy * side + ox];
        }
        sum += f[a] * row;
    }
    grad_y_prev[at] = sum;
}

// ---- host side ----

static int invalid(const char* function, const std::string& message) {
    return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT, std::string(function) + ": " + message);
}

static bool misaligned(const void* pointer) { return (uintptr_t)pointer % alignof(float) != 0; }

// the checks every entry point shares; `channels` lists the channel counts (each a multiple of 16 in [16, 512])
static int check_shape(const char* function, int32_t batch, std::initializer_list<int32_t> channels, int32_t height, int32_t width) {
    if (batch < 1 || batch > kMaxBatch) return invalid(function, "batch must be in [1, " + std::to_string(kMaxBatch) + "], got " + std::to_string(batch));
    for (const int32_t count : channels)
        if (count < 16 || count > kMaxChannels || count % 16 != 0)
            return invalid(function, "channel counts must be multiples of 16 in [16, " + std::to_string(kMaxChannels) + "], got " + std::to_string(count));
    if (height != width) return invalid(function, "inputs must be square, got " + std::to_string(height) + " x " + std::to_string(width));
    if (height < kMinSide || height > kMaxSide)
        return invalid(function, "side must be in [" + std::to_string(kMinSide) + ", " + std::to_string(kMaxSide) + "], got " + std::to_string(height));
    // one thread per element of the largest tensor of a call (an up layer's (2 side + 1)^2 intermediate) in one grid
    for (const int32_t count : channels)
        if ((int64_t)batch * count * (2 * height + 1) * (2 * height + 1) > 0x7FFFFFFF)
            return invalid(function, "batch of " + std::to_string(batch) + " is more than one call's grid at this size");
    return GANCE_OK;
}

static int check_pointers(const char* function, std::initializer_list<const void*> required, std::initializer_list<const void*> optional = {}) {
    for (const void* pointer : required)
        if (pointer == nullptr) return invalid(function, "NULL pointer");
    for (const void* pointer : required)
        if (misaligned(pointer)) return invalid(function, "misaligned pointer (float32 data must be 4-byte aligned)");
    for (const void* pointer : optional)
        if (misaligned(pointer)) return invalid(function, "misaligned pointer (float32 data must be 4-byte aligned)");
    return GANCE_OK;
}

static int segments_of(int positions) { return std::min(kMaxSegments, (positions + kSegmentPositions - 1) / kSegmentPositions); }

static uint64_t round16(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

// workspace of a modulated conv: [the position sums' partials][up: the (2 side + 1)^2 intermediate of Cout channels]
static uint64_t modconv_partial_bytes(int32_t batch, int32_t cin, int32_t cout) {
    return round16((uint64_t)batch * std::max(cin, cout) * kMaxSegments * sizeof(float));
}
static uint64_t modconv_workspace(int32_t batch, int32_t cin, int32_t cout, int32_t side, int32_t up) {
    const uint64_t grid = 2 * (uint64_t)side + 1;
    return modconv_partial_bytes(batch, cin, cout) + (up ? round16((uint64_t)batch * cout * grid * grid * sizeof(float)) : 0);
}

static int no_device() {
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return gance::set_last_error(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    return GANCE_OK;
}

static int hip_failure(const char* function, const char* what, hipError_t status) {
    return gance::set_last_error(GANCE_ERR_HIP, std::string(function) + ": " + what + ": " + hipGetErrorString(status));
}

static int launched(const char* function) {
    const hipError_t status = hipGetLastError();
    return status == hipSuccess ? GANCE_OK : hip_failure(function, "launch", status);
}

static unsigned blocks_for(size_t total) { return (unsigned)((total + kThreads - 1) / kThreads); }

static void launch_contract(const ContractArgs& a, int batch, hipStream_t stream) {
    const unsigned pixel_blocks = (unsigned)((a.OH * a.OW + 63) / 64);
    if (a.M % 64 == 0)
        contract_kernel<4><<<dim3(pixel_blocks, a.M / 64, batch), kThreads, 0, stream>>>(a);
    else if (a.M % 32 == 0)
        contract_kernel<2><<<dim3(pixel_blocks, a.M / 32, batch), kThreads, 0, stream>>>(a);
    else
        contract_kernel<1><<<dim3(pixel_blocks, a.M / 16, batch), kThreads, 0, stream>>>(a);
}

// out[plane] = sum_pos a * b (/ divisor[plane]); with `scaled`, scaled = a * scale[plane] as well (in place when scaled == a)
static void launch_position_sums(const float* a, const float* b, const float* scale, float* scaled, const float* divisor, int planes,
                                 int positions, float* partial, float* out, hipStream_t stream) {
    const int segments = segments_of(positions);
    const int segment = (positions + segments - 1) / segments;
    plane_dot_kernel<<<dim3(planes, segments), kThreads, 0, stream>>>(a, b, scale, scaled, positions, segment, partial);
    plane_finish_kernel<<<blocks_for(planes), kThreads, 0, stream>>>(partial, segments, divisor, planes, out);
}

}  // namespace gance_sgrad

extern "C" {

int gance_modconv3x3_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t side, int32_t up, uint64_t* workspace_bytes) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_modconv3x3_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_shape(kName, batch, {cin, cout}, side, side)) return status;
    if (up && side * 2 > kMaxSide) return invalid(kName, "an up layer's input side must be at most " + std::to_string(kMaxSide / 2) + ", got " + std::to_string(side));
    *workspace_bytes = modconv_workspace(batch, cin, cout, side, up);
    return GANCE_OK;
}

int gance_modconv3x3_forward(const float* d_x, const float* d_style, const float* d_demod, const float* d_weight, int32_t batch, int32_t cin,
                             int32_t cout, int32_t height, int32_t width, int32_t up, float* d_y, void* d_workspace, uint64_t workspace_bytes,
                             void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_modconv3x3_forward";
    if (const int status = check_pointers(kName, {d_x, d_style, d_demod, d_weight, d_y, d_workspace})) return status;
    if (const int status = check_shape(kName, batch, {cin, cout}, height, width)) return status;
    if (up && height * 2 > kMaxSide) return invalid(kName, "an up layer's input side must be at most " + std::to_string(kMaxSide / 2) + ", got " + std::to_string(height));
    const uint64_t needed = modconv_workspace(batch, cin, cout, height, up);
    if (workspace_bytes < needed)
        return invalid(kName, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) + " needed (gance_modconv3x3_workspace_bytes)");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int side = height;
    ContractArgs a{};
    a.in = d_x, a.w = d_weight, a.pre = d_style, a.post = d_demod;
    a.K = cin, a.M = cout, a.w_cin = cin, a.w_cout = cout, a.transposed = 0;
    a.IH = a.IW = side, a.out_stride = 1;
    if (!up) {
        a.out = d_y, a.OH = a.OW = side, a.pad = 1, a.zero_insert = 0;
        launch_contract(a, batch, stream);
    } else {
        float* const grid = (float*)((char*)d_workspace + modconv_partial_bytes(batch, cin, cout));
        a.out = grid, a.OH = a.OW = 2 * side + 1, a.pad = 2, a.zero_insert = 1;
        launch_contract(a, batch, stream);
        const size_t total = (size_t)batch * cout * (2 * side) * (2 * side);
        fir_kernel<<<blocks_for(total), kThreads, 0, stream>>>(grid, d_y, 2 * side, total);
    }
    return launched(kName);
}

int gance_modconv3x3_backward(const float* d_grad_y, const float* d_x, const float* d_y, const float* d_style, const float* d_demod,
                              const float* d_weight, int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t up,
                              float* d_grad_x, float* d_grad_style, float* d_grad_demod, void* d_workspace, uint64_t workspace_bytes,
                              void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_modconv3x3_backward";
    if (const int status = check_pointers(kName, {d_grad_y, d_x, d_y, d_style, d_demod, d_weight, d_grad_x, d_grad_style, d_grad_demod, d_workspace}))
        return status;
    if (const int status = check_shape(kName, batch, {cin, cout}, height, width)) return status;
    if (up && height * 2 > kMaxSide) return invalid(kName, "an up layer's input side must be at most " + std::to_string(kMaxSide / 2) + ", got " + std::to_string(height));
    const uint64_t needed = modconv_workspace(batch, cin, cout, height, up);
    if (workspace_bytes < needed)
        return invalid(kName, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) + " needed (gance_modconv3x3_workspace_bytes)");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int side = height, out_side = up ? 2 * side : side;
    float* const partial = (float*)d_workspace;

    // grad_demod[b][o] = sum_pos grad_y * y / demod   (y = demod * the contraction)
    launch_position_sums(d_grad_y, d_y, nullptr, nullptr, d_demod, batch * cout, out_side * out_side, partial, d_grad_demod, stream);

    // g = the backward-data contraction, without the style, into grad_x
    ContractArgs a{};
    a.w = d_weight, a.pre = d_demod, a.post = nullptr, a.out = d_grad_x;
    a.K = cout, a.M = cin, a.w_cin = cin, a.w_cout = cout, a.transposed = 1;
    a.OH = a.OW = side, a.zero_insert = 0;
    if (!up) {
        a.in = d_grad_y, a.IH = a.IW = side, a.out_stride = 1, a.pad = 1;
    } else {
        float* const grid = (float*)((char*)d_workspace + modconv_partial_bytes(batch, cin, cout));
        const size_t total = (size_t)batch * cout * (2 * side + 1) * (2 * side + 1);
        fir_transpose_kernel<<<blocks_for(total), kThreads, 0, stream>>>(d_grad_y, grid, 2 * side, total);
        a.in = grid, a.IH = a.IW = 2 * side + 1, a.out_stride = 2, a.pad = 0;
    }
    launch_contract(a, batch, stream);

    // grad_style[b][i] = sum_pos x * g, then grad_x = g * style
    launch_position_sums(d_grad_x, d_x, d_style, d_grad_x, nullptr, batch * cin, side * side, partial, d_grad_style, stream);
    return launched(kName);
}

int gance_noise_bias_lrelu_forward(const float* d_x, const float* d_noise, int32_t noise_batch, const float* d_strength, const float* d_bias,
                                   int32_t batch, int32_t channels, int32_t height, int32_t width, float* d_out, void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_noise_bias_lrelu_forward";
    if (const int status = check_pointers(kName, {d_x, d_noise, d_strength, d_bias, d_out})) return status;
    if (const int status = check_shape(kName, batch, {channels}, height, width)) return status;
    if (noise_batch != 1 && noise_batch != batch)
        return invalid(kName, "noise must hold 1 or " + std::to_string(batch) + " planes, got " + std::to_string(noise_batch));
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    const size_t total = (size_t)batch * channels * height * width;
    noise_bias_lrelu_kernel<<<blocks_for(total), kThreads, 0, (hipStream_t)stream_ptr>>>(d_x, d_noise, noise_batch, d_strength, d_bias, channels,
                                                                                        height * width, total, d_out);
    return launched(kName);
}

int gance_noise_bias_lrelu_backward(const float* d_grad_out, const float* d_out, int32_t batch, int32_t channels, int32_t height, int32_t width,
                                    float* d_grad_x, float* d_grad_noise, float* d_grad_strength, float* d_grad_bias, void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_noise_bias_lrelu_backward";
    if (const int status = check_pointers(kName, {d_grad_out, d_out, d_grad_x})) return status;
    if (const int status = check_shape(kName, batch, {channels}, height, width)) return status;
    if (d_grad_noise != nullptr || d_grad_strength != nullptr || d_grad_bias != nullptr)
        return invalid(kName, "gradients for noise, strength and bias are not implemented: pass NULL");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    const size_t total = (size_t)batch * channels * height * width;
    noise_bias_lrelu_backward_kernel<<<blocks_for(total), kThreads, 0, (hipStream_t)stream_ptr>>>(d_grad_out, d_out, total, d_grad_x);
    return launched(kName);
}

int gance_noise_bias_lrelu_backward_noise(const float* d_grad_out, const float* d_out, const float* d_strength, int32_t noise_batch, int32_t batch,
                                          int32_t channels, int32_t height, int32_t width, float* d_grad_x, float* d_grad_noise, void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_noise_bias_lrelu_backward_noise";
    if (const int status = check_pointers(kName, {d_grad_out, d_out, d_strength, d_grad_x, d_grad_noise})) return status;
    if (const int status = check_shape(kName, batch, {channels}, height, width)) return status;
    if (noise_batch != 1 && noise_batch != batch)
        return invalid(kName, "noise must hold 1 or " + std::to_string(batch) + " planes, got " + std::to_string(noise_batch));
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_out));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    const int positions = height * width;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (positions >= 4096)
        noise_bias_lrelu_backward_noise_kernel<64><<<dim3((positions + 63) / 64, noise_batch), kThreads, 0, stream>>>(
            d_grad_out, d_out, d_strength, noise_batch, batch, channels, positions, d_grad_x, d_grad_noise);
    else
        noise_bias_lrelu_backward_noise_kernel<16><<<dim3((positions + 15) / 16, noise_batch), kThreads, 0, stream>>>(
            d_grad_out, d_out, d_strength, noise_batch, batch, channels, positions, d_grad_x, d_grad_noise);
    return launched(kName);
}

int gance_torgb_skip_workspace_bytes(int32_t batch, int32_t cin, int32_t side, uint64_t* workspace_bytes) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_torgb_skip_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_shape(kName, batch, {cin}, side, side)) return status;
    *workspace_bytes = modconv_partial_bytes(batch, cin, cin);
    return GANCE_OK;
}

int gance_torgb_skip_forward(const float* d_x, const float* d_style, const float* d_weight, const float* d_bias, const float* d_y_prev,
                             int32_t batch, int32_t cin, int32_t height, int32_t width, float* d_y, void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_torgb_skip_forward";
    if (const int status = check_pointers(kName, {d_x, d_style, d_weight, d_bias, d_y}, {d_y_prev})) return status;
    if (const int status = check_shape(kName, batch, {cin}, height, width)) return status;
    if (d_y_prev != nullptr && height % 2 != 0) return invalid(kName, "with a skip image the side must be even, got " + std::to_string(height));
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    torgb_skip_kernel<<<dim3(blocks_for((size_t)height * width), batch), kThreads, 0, (hipStream_t)stream_ptr>>>(d_x, d_style, d_weight, d_bias, d_y_prev,
                                                                                                               cin, height, d_y);
    return launched(kName);
}

int gance_torgb_skip_backward(const float* d_grad_y, const float* d_x, const float* d_style, const float* d_weight, int32_t batch, int32_t cin,
                              int32_t height, int32_t width, float* d_grad_x, float* d_grad_style, float* d_grad_y_prev, void* d_workspace,
                              uint64_t workspace_bytes, void* stream_ptr) {
    using namespace gance_sgrad;
    static const char* const kName = "gance_torgb_skip_backward";
    if (const int status = check_pointers(kName, {d_grad_y, d_x, d_style, d_weight, d_grad_x, d_grad_style, d_workspace}, {d_grad_y_prev})) return status;
    if (const int status = check_shape(kName, batch, {cin}, height, width)) return status;
    if (d_grad_y_prev != nullptr && height % 2 != 0) return invalid(kName, "with a skip image the side must be even, got " + std::to_string(height));
    const uint64_t needed = modconv_partial_bytes(batch, cin, cin);
    if (workspace_bytes < needed)
        return invalid(kName, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) + " needed (gance_torgb_skip_workspace_bytes)");
    if (const int status = no_device()) return status;
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess) return hip_failure(kName, "hipSetDevice", guard.status());
    hipStream_t stream = (hipStream_t)stream_ptr;
    const int positions = height * width;
    torgb_backward_data_kernel<<<dim3(blocks_for((size_t)positions), batch), kThreads, 0, stream>>>(d_grad_y, d_weight, cin, positions, d_grad_x);
    launch_position_sums(d_grad_x, d_x, d_style, d_grad_x, nullptr, batch * cin, positions, (float*)d_workspace, d_grad_style, stream);
    if (d_grad_y_prev != nullptr) {
        const size_t total = (size_t)batch * 3 * (height / 2) * (width / 2);
        upsample_transpose_kernel<<<blocks_for(total), kThreads, 0, stream>>>(d_grad_y, height, total, d_grad_y_prev);
    }
    return launched(kName);
}

}  // extern "C"
