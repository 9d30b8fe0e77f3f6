// The plain 3x3 convolution behind torch.ops.gance.conv3x3 (gance_amd/torch_ops.py, gance_amd/stylegan2/lpips.py; DESIGN.md
// section 9 item 16): zero padding 1, stride 1, cross-correlation, no style, no demodulation, no weight gradient
//
//     y[b, o, oy, ox] = sum_{ty, tx, i} w[ty][tx][i][o] * x[b, i, oy + ty - 1, ox + tx - 1]
//
// fp32 NCHW on the caller's stream, without host synchronisation and without floating-point atomics; every sum has one order,
// a function of (cin, cout, side) alone, so two runs give the same bits and a sample's bits do not depend on its batch.
// The input gradient is the same convolution of grad_y with wt[ty][tx][o][i] = w[2 - ty][2 - tx][i][o], which the caller
// builds once: there is one kernel family, not a forward one and a backward one.
//
// conv3x3_kernel<MT, SPLIT>, on v_mfma_f32_16x16x4_f32 (A[m][k] in lane 16 k + m, B[k][n] in lane 16 k + n, D[m][n] in lane
// 16 (m / 4) + n, register m % 4; m an output channel, k a contracted channel, n a pixel of one row):
//   * a block is 4 waves = 8 rows x 16 columns of output pixels x 16 MT output channels of one sample; wave w owns rows 2 w and
//     2 w + 1, so it carries 2 MT independent accumulators;
//   * per chunk of 16 contracted channels the block stages the 10 x 18 input patch (the tile and one ring, zeros where the ring
//     or the tile leaves the image, so the K loop has no bounds tests) and the chunk's weights [tap][k][m] in LDS. A staged
//     input value serves up to nine taps and every channel tile; a fragment row read for (row r, tap row ty) is the one of
//     (row r + 1, tap row ty - 1), so a wave reads 4 patch rows x 3 shifts per k step, not 2 x 9;
//   * bank rules: a ds_read_b32 is served in 32-lane halves over 32 banks, a half holds two k planes of 16 consecutive words:
//     the plane strides (kPlane for the patch, ROW for the weights) are 16 mod 32, so the two planes fall on disjoint halves
//     of the banks whatever the shift. Patch rows (18 words) are unaligned: they are staged and read a word at a time;
//   * the next chunk is fetched into registers (12 + 9 MT loads per lane, below the 63 a wave may have in flight) before the
//     current chunk's MFMAs are issued and written to LDS after them: the fetch runs under the matrix work, and two blocks
//     fit a CU (59 KB of LDS each at MT = 4), so one block's barriers are covered by the other's MFMAs;
//   * blocked summation: a chunk's 144 products are summed on their own, then added to the running total (K reaches 4608);
//   * SPLIT: the chunks are divided over `splits` blocks, each writes its partial sums to the workspace, and
//     conv3x3_finish_kernel adds them in rising order. The small layers fill the machine this way (no atomics).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <string>

#include "../../include/gance_hip.h"
#include "kernels.h"

namespace gance_conv3x3 {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMinSide = 4, kMaxSide = 1024, kMaxChannels = 512, kMaxBatch = 65535;
constexpr int kTileRows = 8, kTileCols = 16;
constexpr int kPatchRows = kTileRows + 2, kPatchCols = kTileCols + 2;
constexpr int kPlane = 208;  // words per staged input channel: 10 x 18 = 180, padded to 16 mod 32
constexpr int kPatchLoads = (16 * kPatchRows * kPatchCols + kThreads - 1) / kThreads;  // 12 (the last one a quarter full)

struct Args {
    const float* in;  // [B][K][side][side]
    const float* w;   // [9][K][M]
    float* out;       // [B][M][side][side], or with SPLIT the partials [splits][B][M][side][side]
    int K, M, side;
    int splits;
};

template <int MT, bool SPLIT>
__global__ __launch_bounds__(kThreads, 2) void conv3x3_kernel(const Args p) {
    constexpr int ROW = MT == 1 ? 16 : 16 * MT + 16;    // 16 mod 32
    constexpr int WLOADS = 9 * 16 * 16 * MT / kThreads;  // 9 MT
    constexpr int WROWS = kThreads / (16 * MT);          // rows of [tap][k] one pass of the block covers
    __shared__ float xs[16 * kPlane];
    __shared__ float ws[9 * 16 * ROW];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int side = p.side;
    const int tiles_x = (side + kTileCols - 1) / kTileCols;
    const int oy0 = (blockIdx.x / tiles_x) * kTileRows, ox0 = (blockIdx.x % tiles_x) * kTileCols;
    const int m0 = blockIdx.y * 16 * MT;
    const int b = SPLIT ? blockIdx.z / p.splits : blockIdx.z;
    const int split = SPLIT ? blockIdx.z % p.splits : 0;
    const int chunks = p.K / 16;
    const int chunk_first = SPLIT ? split * chunks / p.splits : 0;
    const int chunk_last = SPLIT ? (split + 1) * chunks / p.splits : chunks;

    // what this lane stages of a chunk: patch words (source offset inside the chunk's 16 planes, -1 a zero) and weight words
    const size_t plane = (size_t)side * side;
    int x_src[kPatchLoads], x_dst[kPatchLoads];
#pragma unroll
    for (int j = 0; j < kPatchLoads; ++j) {
        const int e = tid + j * kThreads;
        const int k = e / (kPatchRows * kPatchCols), rest = e % (kPatchRows * kPatchCols);
        const int r = rest / kPatchCols, c = rest % kPatchCols;
        const int iy = oy0 + r - 1, ix = ox0 + c - 1;
        const bool inside = k < 16 && iy >= 0 && iy < side && ix >= 0 && ix < side;
        x_src[j] = inside ? (int)(k * plane) + iy * side + ix : -1;
        x_dst[j] = k < 16 ? k * kPlane + r * kPatchCols + c : -1;
    }
    const int w_m = tid % (16 * MT), w_row = tid / (16 * MT);
    const bool w_ok = m0 + w_m < p.M;  // the last channel tile of a block may lie past cout: it is staged as zeros
    const float* const w_lane = p.w + (size_t)w_row * p.M + min(m0 + w_m, p.M - 1);
    const float* const in_sample = p.in + (size_t)b * p.K * plane;

    float x_reg[kPatchLoads], w_reg[WLOADS];
    auto fetch = [&](int chunk) {
        const float* const in_chunk = in_sample + (size_t)chunk * 16 * plane;
#pragma unroll
        for (int j = 0; j < kPatchLoads; ++j) x_reg[j] = in_chunk[max(x_src[j], 0)];
        const float* const w_chunk = w_lane + (size_t)chunk * 16 * p.M;
#pragma unroll
        for (int j = 0; j < WLOADS; ++j) {
            const int row = j * WROWS;  // + w_row: tap row / 16, channel row % 16; WROWS divides 16
            w_reg[j] = w_chunk[((size_t)(row / 16) * p.K + row % 16) * p.M];
        }
    };

    f32x4 acc[2][MT];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[r][mt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* const x_frag = xs + lq * kPlane + 2 * wave * kPatchCols + l15;
    const float* const w_frag = ws + lq * ROW + l15;

    fetch(chunk_first);
    for (int chunk = chunk_first; chunk < chunk_last; ++chunk) {
#pragma unroll
        for (int j = 0; j < kPatchLoads; ++j)
            if (x_dst[j] >= 0) xs[x_dst[j]] = x_src[j] >= 0 ? x_reg[j] : 0.f;
#pragma unroll
        for (int j = 0; j < WLOADS; ++j) ws[(w_row + j * WROWS) * ROW + w_m] = w_ok ? w_reg[j] : 0.f;
        __syncthreads();
        if (chunk + 1 < chunk_last) fetch(chunk + 1);  // in flight under this chunk's MFMAs

        f32x4 part[2][MT];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) part[r][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) {
            float bv[4][3];
#pragma unroll
            for (int pr = 0; pr < 4; ++pr)
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) bv[pr][tx] = x_frag[kq * 4 * kPlane + pr * kPatchCols + tx];
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int tx = 0; tx < 3; ++tx)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const float a = w_frag[((ty * 3 + tx) * 16 + kq * 4) * ROW + mt * 16];
                        part[0][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[ty][tx], part[0][mt], 0, 0, 0);
                        part[1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[ty + 1][tx], part[1][mt], 0, 0, 0);
                    }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[r][mt] += part[r][mt];
        __syncthreads();  // the chunk's fragments have been read
    }

    // a lane holds channels 4 lq + i (i = 0 .. 3) of each 16-channel tile, for column l15 of its two rows
    float* const out = p.out + ((size_t)split * gridDim.z / p.splits + b) * p.M * plane;
    const int ox = ox0 + l15;
    if (ox >= side) return;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + 2 * wave + r;
        if (oy >= side) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + mt * 16 + 4 * lq + i;
                if (m < p.M) out[(size_t)m * plane + (size_t)oy * side + ox] = acc[r][mt][i];
            }
    }
}

// y = the partials [splits][total] added in rising order
__global__ __launch_bounds__(kThreads) void conv3x3_finish_kernel(const float* __restrict__ partial, int splits, size_t total, float* __restrict__ y) {
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= total) return;
    float sum = partial[at];
    for (int s = 1; s < splits; ++s) sum += partial[(size_t)s * total + at];
    y[at] = sum;
}

// ---- host side ----

static int invalid(const char* function, const std::string& message) {
    return gance::set_last_error(GANCE_ERR_INVALID_ARGUMENT, std::string(function) + ": " + message);
}

static bool misaligned(const void* pointer) { return (uintptr_t)pointer % alignof(float) != 0; }

static int check_shape(const char* function, int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width) {
    if (batch < 1 || batch > kMaxBatch) return invalid(function, "batch must be in [1, " + std::to_string(kMaxBatch) + "], got " + std::to_string(batch));
    for (const int32_t count : {cin, cout})
        if (count < 16 || count > kMaxChannels || count % 16 != 0)
            return invalid(function, "channel counts must be multiples of 16 in [16, " + std::to_string(kMaxChannels) + "], got " + std::to_string(count));
    if (height != width) return invalid(function, "inputs must be square, got " + std::to_string(height) + " x " + std::to_string(width));
    if (height < kMinSide || height > kMaxSide)
        return invalid(function, "side must be in [" + std::to_string(kMinSide) + ", " + std::to_string(kMaxSide) + "], got " + std::to_string(height));
    // one thread per element of the larger tensor in one grid (the finishing pass), and int offsets inside a sample
    if ((int64_t)batch * std::max(cin, cout) * height * height > 0x7FFFFFFF)
        return invalid(function, "batch of " + std::to_string(batch) + " is more than one call's grid at this size");
    return GANCE_OK;
}

// The form of a shape, a function of (cin, cout, side) and never of the batch: 8 * t + log2(splits), t = 0, 1, 2 for channel
// tiles of 16, 32 and 64 per block. Splits: the 8 x 16 pixel tiles of one sample times the channel tiles fill 256 CUs from
// side 128 up at VGG's widths; below, the contracted chunks are divided, by 2 up to side 64, 4 up to 32, 16 up to 16, and
// never into runs of fewer than two chunks.
struct Form {
    int mt, splits;
    int id() const { return 8 * (mt == 4 ? 2 : mt == 2 ? 1 : 0) + (splits == 16 ? 4 : splits == 8 ? 3 : splits == 4 ? 2 : splits == 2 ? 1 : 0); }
};

static Form form_of(int32_t cin, int32_t cout, int32_t side) {
    Form form;
    form.mt = cout >= 64 ? 4 : cout >= 32 ? 2 : 1;
    const int wanted = side <= 16 ? 16 : side <= 32 ? 4 : side <= 64 ? 2 : 1;
    form.splits = 1;
    while (form.splits * 2 <= wanted && form.splits * 2 * 2 <= cin / 16) form.splits *= 2;
    return form;
}

static uint64_t round16(uint64_t bytes) { return (bytes + 15) / 16 * 16; }

// the partial sums of a split form; 16 bytes otherwise, so that the workspace is a pointer every form may check alike
static uint64_t workspace_of(int32_t batch, int32_t cin, int32_t cout, int32_t side) {
    const Form form = form_of(cin, cout, side);
    if (form.splits == 1) return 16;
    return round16((uint64_t)form.splits * batch * cout * side * side * sizeof(float));
}

template <int MT>
static void launch(const Args& a, int batch, hipStream_t stream) {
    const unsigned tiles = (unsigned)(((a.side + kTileCols - 1) / kTileCols) * ((a.side + kTileRows - 1) / kTileRows));
    const unsigned channel_blocks = (unsigned)((a.M + 16 * MT - 1) / (16 * MT));
    if (a.splits == 1)
        conv3x3_kernel<MT, false><<<dim3(tiles, channel_blocks, batch), kThreads, 0, stream>>>(a);
    else
        conv3x3_kernel<MT, true><<<dim3(tiles, channel_blocks, batch * a.splits), kThreads, 0, stream>>>(a);
}

}  // namespace gance_conv3x3

extern "C" {

int gance_conv3x3_form(int32_t cin, int32_t cout, int32_t side, int32_t* form) {
    using namespace gance_conv3x3;
    static const char* const kName = "gance_conv3x3_form";
    if (form == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_shape(kName, 1, cin, cout, side, side)) return status;
    *form = form_of(cin, cout, side).id();
    return GANCE_OK;
}

int gance_conv3x3_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t side, uint64_t* workspace_bytes) {
    using namespace gance_conv3x3;
    static const char* const kName = "gance_conv3x3_workspace_bytes";
    if (workspace_bytes == nullptr) return invalid(kName, "NULL pointer");
    if (const int status = check_shape(kName, batch, cin, cout, side, side)) return status;
    *workspace_bytes = workspace_of(batch, cin, cout, side);
    return GANCE_OK;
}

int gance_conv3x3_forward(const float* d_x, const float* d_weight, int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width,
                          float* d_y, void* d_workspace, uint64_t workspace_bytes, void* stream_ptr) {
    using namespace gance_conv3x3;
    static const char* const kName = "gance_conv3x3_forward";
    for (const void* pointer : {(const void*)d_x, (const void*)d_weight, (const void*)d_y, (const void*)d_workspace})
        if (pointer == nullptr) return invalid(kName, "NULL pointer");
    for (const void* pointer : {(const void*)d_x, (const void*)d_weight, (const void*)d_y, (const void*)d_workspace})
        if (misaligned(pointer)) return invalid(kName, "misaligned pointer (float32 data must be 4-byte aligned)");
    if (const int status = check_shape(kName, batch, cin, cout, height, width)) return status;
    const uint64_t needed = workspace_of(batch, cin, cout, height);
    if (workspace_bytes < needed)
        return invalid(kName, "workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(needed) + " needed (gance_conv3x3_workspace_bytes)");
    int device_count = 0;
    if (hipGetDeviceCount(&device_count) != hipSuccess || device_count == 0)
        return gance::set_last_error(GANCE_ERR_NO_DEVICE, "no HIP device visible; libgance_hip has no CPU path");
    gance::DeviceGuard guard(gance::device_of_pointer(d_x));  // launch where the data lives
    if (guard.status() != hipSuccess)
        return gance::set_last_error(GANCE_ERR_HIP, std::string(kName) + ": hipSetDevice: " + hipGetErrorString(guard.status()));
    hipStream_t stream = (hipStream_t)stream_ptr;
    const Form form = form_of(cin, cout, height);
    Args a{};
    a.in = d_x, a.w = d_weight, a.K = cin, a.M = cout, a.side = height, a.splits = form.splits;
    a.out = form.splits == 1 ? d_y : (float*)d_workspace;
    if (form.mt == 4)
        launch<4>(a, batch, stream);
    else if (form.mt == 2)
        launch<2>(a, batch, stream);
    else
        launch<1>(a, batch, stream);
    if (form.splits > 1) {
        const size_t total = (size_t)batch * cout * height * height;
        conv3x3_finish_kernel<<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, stream>>>((const float*)d_workspace, form.splits, total, d_y);
    }
    const hipError_t status = hipGetLastError();
    return status == hipSuccess ? GANCE_OK : gance::set_last_error(GANCE_ERR_HIP, std::string(kName) + ": launch: " + hipGetErrorString(status));
}

}  // extern "C"
