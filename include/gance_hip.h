/*
 * gance_hip.h -- C ABI of libgance_hip.so, the MI355X (gfx950) implementation of GANce's hot path
 *                audio -> latent -> StyleGAN2 frame synthesis.
 *
 * Plain pointers and sizes only; no torch / numpy types. Device pointers are HIP device pointers
 * (e.g. torch.Tensor.data_ptr() of a cuda tensor); `stream` is a hipStream_t passed as void*
 * (NULL = the null stream). All functions return GANCE_OK (0) or a negative-free status code
 * below; gance_last_error() returns a thread-local description of the last failure.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the GANce tree).
 */
#ifndef GANCE_HIP_H
#define GANCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANCE_ABI_VERSION 6

enum gance_status {
    GANCE_OK = 0,
    GANCE_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, bad size, batch > max_batch ...            */
    GANCE_ERR_BAD_WEIGHTS = 2,      /* weight blob length does not match the configuration      */
    GANCE_ERR_HIP = 3,              /* a HIP runtime call failed (see gance_last_error)         */
    GANCE_ERR_OUT_OF_MEMORY = 4,    /* hipMalloc failed                                         */
    GANCE_ERR_NO_DEVICE = 5         /* no gfx950 device visible: there is NO CPU fallback       */
};

const char* gance_last_error(void);
int gance_abi_version(void);

/* ------------------------------------------------------------------------------------------ */
/* Latent -> frame: StyleGAN2 generator engine (the skip generator of config-f and config-e)  */
/* ------------------------------------------------------------------------------------------ */

typedef struct gance_engine gance_engine; /* opaque; owns weights + workspace in HBM */

/* The channel table is nf(stage) = clip(fmap_base >> stage, 1, 512): fmap_base = 16 << 10 (config-f) unless `flags` carries
 * GANCE_FLAG_FMAP_BASE_8K (config-e: half the channels from 64x64 up, 16 at 1024x1024). Up to 32x32 both are one network. */
typedef struct gance_engine_config {
    int32_t resolution; /* output side, power of two in [8, 1024]; 1024 = FFHQ config-f / config-e */
    int32_t max_batch;  /* workspace is sized for this many frames per call (>= 1)             */
    int32_t device;     /* HIP device ordinal                                                  */
    int32_t flags;      /* GANCE_FLAG_*                                                        */
} gance_engine_config;

#define GANCE_FLAG_PROFILE_STEPS 1 /* record a hipEvent pair around every kernel launch        */
/* The Conv1 layers from 32x32 up run in Winograd form whenever a launch has at least one tile per CU: F(4x4,3x3) (1/4 of
 * the multiply-adds) where the launch fills the chip with its 16 x 64 pixel tiles, else F(2x2,3x3) (4/9), else the direct
 * form; results differ between the forms by fp32 rounding only (~1e-6 of the activation range). DIRECT_CONV keeps every
 * layer in direct form; FORCE_WINOGRAD alone puts every layer that supports it on the F(2x2,3x3) kernels whatever the
 * batch, FORCE_WINOGRAD | WINOGRAD43 on the F(4x4,3x3) kernel where that supports the layer (parity tests of each form). With
 * either, a 32-channel last layer (1024^2, or 512^2 with FMAP_BASE_8K) runs in that form with the ToRGB channel sum in its
 * epilogue, the launch the default selects there once it fills the chip, not the direct-form launch that absorbs the whole ToRGB. */
#define GANCE_FLAG_DIRECT_CONV 2
#define GANCE_FLAG_FORCE_WINOGRAD 4
/* Conv0_up of the layers whose input is >= 64 wide runs as ONE kernel (transposed conv + FIR + noise + bias +
 * leaky ReLU, the (2H+1)^2 intermediate stays on chip) whenever the launch gives every CU a block without
 * cutting the image into row segments shorter than 4 steps. SPLIT_UPFIR keeps the two-pass form
 * (transposed conv, then FIR pass); FORCE_FUSED_UPFIR drops the block-count condition (parity tests). */
#define GANCE_FLAG_SPLIT_UPFIR 8
#define GANCE_FLAG_FORCE_FUSED_UPFIR 16
/* The per-call scratch (activations etc.: ~0.8 GB per frame of batch capacity at 1024^2) is shared by every
 * engine of one (device, resolution, max_batch): N resident networks cost N x 135 MB of weights + ONE workspace.
 * Calls that share it are ordered by an event, on whatever streams they run. PRIVATE_WORKSPACE gives an engine
 * its own (calls of different engines may then overlap on different streams). */
#define GANCE_FLAG_PRIVATE_WORKSPACE 32
/* The network is config-e (fmap_base = 8 << 10): gance_engine_create expects the blob of that channel table
 * (gance_weight_blob_floats_flags) and gance_engine_describe_plan plans its layers. Engines with and without it never share
 * a workspace. */
#define GANCE_FLAG_FMAP_BASE_8K 128
#define GANCE_FLAG_WINOGRAD43 64 /* with FORCE_WINOGRAD: Conv1 layers from 32x32 up in Winograd F(4x4,3x3) form wherever the kernel supports the layer */

/*
 * Load a network. Replaces load_network_network + wrap_loaded_network
 * (gance/network_interface/network_functions.py:93-111,114-192): the reference unpickles a TF1
 * Network and opens a session; here the caller hands the raw variables as one float32 blob in
 * the order documented in gance_amd/stylegan2/spec.py::variable_shapes (TF variable order:
 * mapping dense 0..7 {weight,bias}, dlatent_avg, const, per conv layer {weight HWIO, mod_weight,
 * mod_bias, noise_strength, bias}, per ToRGB {weight, mod_weight, mod_bias, bias}, noise buffers).
 * The engine applies the equalised-LR runtime coefficients and re-lays the weights out for its
 * kernels. `host_weights` is host memory and is not retained.
 */
int gance_engine_create(const gance_engine_config* config, const float* host_weights,
                        uint64_t num_floats, gance_engine** out_engine);

/* Replaces the worker's stop_function (network_functions.py:303-321): frees HBM. NULL is a no-op. */
void gance_engine_destroy(gance_engine* engine);

/* network.input_shape[1] (network_functions.py:191): length of a z / w vector (512). */
int32_t gance_engine_vector_length(const gance_engine* engine);
/* Number of dlatent rows W the matrix path expects (18 at 1024, 14 at 256). */
int32_t gance_engine_num_layers(const gance_engine* engine);
int32_t gance_engine_resolution(const gance_engine* engine);
int32_t gance_engine_max_batch(const gance_engine* engine);
/* Number of floats gance_engine_create expects for `resolution` (0 if unsupported). */
uint64_t gance_weight_blob_floats(int32_t resolution);
/* ... for an engine created with `flags`: only GANCE_FLAG_FMAP_BASE_8K changes the count (without it: the function above). */
uint64_t gance_weight_blob_floats_flags(int32_t resolution, int32_t flags);

/*
 * Matrix path. Replaces create_image_matrix (network_functions.py:160-169):
 *   G.components.synthesis.run(dlatents[1,W,512], randomize_noise=False,
 *                              output_transform=convert_images_to_uint8(nchw_to_nhwc=True))
 * batched: d_dlatents is [batch][W][512] float32 on the device. d_out_u8 receives
 * [batch][R][R][3] uint8 (RGB, NHWC) and may be NULL; d_out_f32 (optional, may be NULL) receives
 * the pre-quantisation image [batch][3][R][R] float32 for tolerance checks.
 */
int gance_synthesize_w(gance_engine* engine, const float* d_dlatents, int32_t batch,
                       uint8_t* d_out_u8, float* d_out_f32, void* stream);

/*
 * Vector path. Replaces create_image_vector (network_functions.py:144-158):
 *   G.run(z[1,512], None, truncation_psi=1.2, output_transform=...)
 * = normalise z, 8-layer mapping, broadcast to W rows, w' = avg + psi*(w - avg) on every row,
 * synthesis. d_z is [batch][512] float32 on the device. Stored noise buffers are used.
 */
int gance_synthesize_z(gance_engine* engine, const float* d_z, int32_t batch,
                       float truncation_psi, uint8_t* d_out_u8, float* d_out_f32, void* stream);

/*
 * Host-buffer forms of the two calls above for the reference's one-frame-at-a-time boundary
 * (ImageFunction.__call__, network_functions.py:51-63): H2D copy, synthesis, D2H copy,
 * synchronous. h_out_u8 is [batch][R][R][3]; h_out_f32 may be NULL.
 */
int gance_synthesize_w_host(gance_engine* engine, const float* h_dlatents, int32_t batch,
                            uint8_t* h_out_u8, float* h_out_f32);
int gance_synthesize_z_host(gance_engine* engine, const float* h_z, int32_t batch,
                            float truncation_psi, uint8_t* h_out_u8, float* h_out_f32);

/*
 * Profiling / debugging (no reference counterpart).
 * With GANCE_FLAG_PROFILE_STEPS every launch of the last synthesize call is bracketed by
 * hipEvents on the call's stream. gance_engine_step_count returns the number of launches,
 * gance_engine_step_info fills name (<=63 chars + NUL), elapsed milliseconds and the
 * algorithmic FLOPs and bytes of launch `index` of the LAST call (synchronises the stream).
 */
/* Change the profiling mode between calls: `flags` replaces the GANCE_FLAG_PROFILE_STEPS bit of the
 * engine's configuration; with a non-NULL `only_step` just the launches whose name contains that
 * string are bracketed (two events per call instead of ~100: what bench.py's timed region uses
 * for the dominant kernel) and their records accumulate over calls (up to 4096) until the next
 * gance_engine_set_profiling. */
int gance_engine_set_profiling(gance_engine* engine, int32_t flags, const char* only_step);
int32_t gance_engine_step_count(const gance_engine* engine);
int gance_engine_step_info(gance_engine* engine, int32_t index, char* name64, float* ms,
                           double* flops, double* bytes);
/* Host only, no device and no weights: the launch names, one per line and in launch order, of a gance_synthesize_w call of
 * `batch` frames on an engine created from `config` (and the GANCE_TUNE_* environment of this process) on a device of `num_cus`
 * compute units -- the very strings gance_engine_step_info reports for such a call. `out` receives them NUL-terminated;
 * GANCE_ERR_INVALID_ARGUMENT for a bad configuration or batch, or a `capacity` that is too small. */
int gance_engine_describe_plan(const gance_engine_config* config, int32_t num_cus, int32_t batch, char* out, uint64_t capacity);
/*
 * randomize_noise of the generator. The reference's vector path (create_image_vector, network_functions.py:152-157)
 * leaves `randomize_noise` at the upstream default True: every call draws fresh N(0, 1) noise, one plane per layer AND
 * PER SAMPLE (upstream: tf.random_normal([N, 1, H, W])), instead of the stored noise buffers; its matrix path passes
 * randomize_noise=False (:121-125). gance_engine_randomize_noise draws planes for `count` samples (0: max_batch) of every
 * layer whose noise_strength is non-zero (none in a random-init network) into buffers of the engine's own, asynchronously
 * on `stream` (with a NULL stream it returns after completion: the host-buffer entries run on a stream of their own).
 * Sample b of the following calls (batch <= count, else GANCE_ERR_INVALID_ARGUMENT) reads the plane with the id
 * d_sample_ids[b] (device memory, int64) or, with d_sample_ids NULL, first_sample + b; a plane is a function of
 * (seed, layer, id) only, so with id = frame number a frame's noise does not depend on how frames were batched or
 * sharded. The draws stay until the next call of either function; gance_engine_restore_noise goes back to the stored
 * buffers (which are never overwritten).
 */
int gance_engine_randomize_noise(gance_engine* engine, uint64_t seed, int32_t count, uint64_t first_sample,
                                 const int64_t* d_sample_ids, void* stream);
int gance_engine_restore_noise(gance_engine* engine, void* stream);
/* Debug: the noise plane sample `sample` of conv layer `conv_layer` currently reads ([res][res] floats, count = res * res), to host memory. */
int gance_engine_debug_read_noise(gance_engine* engine, int32_t conv_layer, int32_t sample, float* h_out, uint64_t count);

/*
 * Debug: run only the first `num_steps` conv layers of the next synthesize_w calls (<=0 = all)
 * and copy the current activation tensor [batch][C][res][res] to the host.
 */
int gance_engine_debug_stop_after(gance_engine* engine, int32_t num_conv_layers);
int gance_engine_debug_read_activation(gance_engine* engine, int32_t batch, float* h_out,
                                       uint64_t max_floats, int32_t* out_channels,
                                       int32_t* out_side);
/*
 * Debug: the fp32 skip image [batch][3][side][side] that the last ToRGB of the engine's last call left in the workspace, to
 * host memory: after a call stopped by gance_engine_debug_stop_after, the image of the resolution it stopped in (stopped after
 * an up layer: of the resolution before it, whose Conv1 then ran exactly as in a whole call). GANCE_ERR_INVALID_ARGUMENT when
 * no ToRGB of that call stored an fp32 image (a bytes-only call of the largest resolutions; a call replayed from a graph),
 * when `batch` is not that call's, or when the image exceeds `max_floats`.
 */
int gance_engine_debug_read_skip_image(gance_engine* engine, int32_t batch, float* h_out, uint64_t max_floats, int32_t* out_side);
/*
 * Debug: the part of a call in front of the first convolution, stage by stage, host memory in and out (each returns after
 * completion). All four return GANCE_ERR_INVALID_ARGUMENT, and write nothing, for a NULL argument, a batch outside
 * [1, max_batch], a layer out of range or a result larger than `max_floats`.
 * gance_engine_debug_mapping: the output [batch][512] of the first `num_dense_layers` (1 ... 8) dense layers of the mapping
 * network for z [batch][512], through the launch loop gance_synthesize_z runs.
 * gance_engine_debug_dlatents: the dlatents [batch][num_layers][512] that gance_synthesize_z would hand to synthesis.
 * gance_engine_debug_read_style / _read_demod: the style vector [batch][cin] of conv layer `index` (kind 0) or of ToRGB
 * `index` (kind 1, 0 = 4x4), and the demodulation vector [batch][cout] of conv layer `conv_layer`, as the engine's last
 * synthesize_w / synthesize_z call of `batch` samples left them (a call stopped by gance_engine_debug_stop_after will do:
 * both are computed before the first layer). Refused when another engine of the shared workspace made the last call.
 */
int gance_engine_debug_mapping(gance_engine* engine, const float* h_z, int32_t batch, int32_t num_dense_layers, float* h_out,
                               uint64_t max_floats);
int gance_engine_debug_dlatents(gance_engine* engine, const float* h_z, int32_t batch, float truncation_psi, float* h_out,
                                uint64_t max_floats);
int gance_engine_debug_read_style(gance_engine* engine, int32_t kind, int32_t index, int32_t batch, float* h_out, uint64_t max_floats);
int gance_engine_debug_read_demod(gance_engine* engine, int32_t conv_layer, int32_t batch, float* h_out, uint64_t max_floats);
/*
 * Debug: the state the workspace keeps between calls. Every convolution kernel reads out-of-image taps as zeros without a
 * bounds test: the borders of each layer's activation planes [res+2][res+8] (interior: rows 1 ... res, columns 4 ... res+3)
 * and of an up layer's parity planes [H+3][W+8] (class (py, px) owns rows 1 ... H+1-py, columns 4 ... W+4-px) are zeroed
 * once, when the workspace is created, and no kernel may write them. Both entries first wait for the workspace's last call
 * (whichever engine of the shared workspace made it, on whatever stream) and return after completion.
 * gance_engine_debug_border_residue: six words per conv layer into h_out (count = 6 * conv layers, else
 * GANCE_ERR_INVALID_ARGUMENT): border words of the layer's activation buffer with !(v == 0.0f) (-0 passes, NaN counts), border
 * words scanned, planes scanned; then the same three for its parity planes (zeros for a stride-1 layer). The scan covers the
 * buffers' whole capacity (max_batch samples, every split unit, the four classes, every channel), not the last call's batch.
 * gance_engine_debug_poison_scratch: fills every cell that is NOT border of every activation and parity plane, and every
 * other scratch buffer of the workspace (split-K slabs, GEMM operands and products, skip images, ToRGB coefficients and
 * partial images, styles, demodulation, dlatents, mapping buffers, z; the byte staging with a byte pattern), with `value`, and
 * forgets whose styles and whose skip image the workspace holds: a call after it must return what it would have returned
 * before, since a call reads no scratch it did not write itself. With include_borders != 0 the borders are filled too,
 * which breaks the workspace for good: refused with GANCE_ERR_INVALID_ARGUMENT unless the engine was created with
 * GANCE_FLAG_PRIVATE_WORKSPACE; it exists to show that the scan sees every border word.
 */
int gance_engine_debug_border_residue(gance_engine* engine, uint64_t* h_out, uint64_t count);
int gance_engine_debug_poison_scratch(gance_engine* engine, float value, int32_t include_borders);

/* ------------------------------------------------------------------------------------------ */
/* Audio -> latent: spectrogram, fft-roll, alpha blend with projected latents                  */
/* ------------------------------------------------------------------------------------------ */

typedef struct gance_blend gance_blend; /* opaque; operator tables + workspace in HBM */

typedef struct gance_blend_config {
    int32_t num_frames;            /* N output frames; audio holds N * vector_length samples      */
    int32_t vector_length;         /* L = 512                                                     */
    int32_t num_projection_frames; /* F projected latents; N % F == 0 (divisor.py:19-24)          */
    int32_t latent_depth;          /* rows per latent matrix (18)                                 */
    int32_t blend_depth;           /* rows that receive the blend (--blend-depth, <= 18)          */
    int32_t fft_roll_enabled;      /* --fft-roll-enabled                                          */
    int32_t num_networks;          /* K = len(network_indices)                                    */
    int32_t has_amplitude_range;   /* 0 = no min-max scaling                                      */
    double alpha;                  /* --alpha                                                     */
    double amplitude_lo;           /* --fft-amplitude-range                                       */
    double amplitude_hi;
    /* savgol_filter applied to the rolling RMS before it is quantised to network indices:
     * 0, 0 = (3, 2), what alpha_blend_projection_file passes (visualization_inputs.py:244-252);
     * noise-blend leaves reduce_vector_rms_rolling_average at its defaults (7, 3)
     * (visualization_inputs.py:146-151, vector_reduction.py:102-108). */
    int32_t index_savgol_window_length;
    int32_t index_savgol_polyorder;
} gance_blend_config;

/*
 * Replaces the table-free Python of alpha_blend_projection_file
 * (gance/data_into_network_visualization/visualization_inputs.py:169-270) and everything it calls:
 * compute_spectrogram_smooth_scale (gance/apply_spectrogram.py:85-118), reduce_vector_rms_rolling_average
 * + quantize_results_layers (gance/vector_sources/vector_reduction.py:102-124,161-194),
 * rotate_vectors_over_time / smooth_each_vector / duplicate_to_vector_count / promote_to_matrix_duplicate
 * (gance/vector_sources/vector_sources_common.py:408-428,169-188,298-365).
 * Raises (returns GANCE_ERR_INVALID_ARGUMENT) where the reference raises ValueError: N % F != 0.
 */
int gance_blend_create(const gance_blend_config* config, int32_t device, gance_blend** out_blend);
void gance_blend_destroy(gance_blend* blend);

/*
 * d_audio: float32 [>= N*L] time-series audio (read_wavs_scale_for_video's output,
 * gance/vector_sources/music.py:60-169). d_latent_row0: float32 [F][L], row 0 of every projected
 * final latent (the only row the reference uses, visualization_inputs.py:220-231).
 * d_dlatents (may be NULL): float32 [N][latent_depth][L], the per-frame matrices `combined` is
 * split into by _frame_inputs (network_visualization.py:233-251), cast to the float32 the
 * network is fed. d_network_indices (may be NULL): int32 [N]. With debug_stages != 0 every
 * intermediate is kept for gance_blend_read_stage. Asynchronous on `stream`.
 */
int gance_blend_run(gance_blend* blend, const float* d_audio, uint64_t num_samples,
                    const float* d_latent_row0, float* d_dlatents, int32_t* d_network_indices,
                    int32_t debug_stages, void* stream);

enum gance_blend_stage {
    GANCE_STAGE_DB = 0,            /* float64 [N][255]  compute_spectrogram, transposed          */
    GANCE_STAGE_SCALED = 1,        /* float64 [N][L]    after resample + minmax                  */
    GANCE_STAGE_SMOOTHED_TIME = 2, /* float64 [N][L]    after smooth_across_vectors(7,3)         */
    GANCE_STAGE_SMOOTHED = 3,      /* float64 [N][L]    compute_spectrogram_smooth_scale         */
    GANCE_STAGE_ROLLED = 4,        /* float64 [N][L]    after rotate_vectors_over_time           */
    GANCE_STAGE_FINAL = 5,         /* float64 [N][L]    a_vectors.data                           */
    GANCE_STAGE_BLEND_ROW = 6,     /* float64 [N][L]    combined.data[0]                         */
    GANCE_STAGE_RAW_RMS = 7,       /* float32 [N]                                                */
    GANCE_STAGE_ROLL_VALUES = 8,   /* int32   [N]       quantised roll per frame                 */
    GANCE_STAGE_ROLL_CUMULATIVE = 9, /* int32 [N]       cumsum(roll) mod L                       */
    GANCE_STAGE_NETWORK_INDICES = 10, /* int32 [N]                                               */
    GANCE_STAGE_ROLLING_AVERAGE = 11, /* float64 [N]    roll chain                               */
    GANCE_STAGE_ROLLING_SMOOTHED = 12, /* float64 [N]   roll chain                               */
    GANCE_STAGE_INDEX_SMOOTHED = 13,   /* float64 [N]   network-index chain                      */
    GANCE_STAGE_MINMAX = 14            /* float64 [3]   global max |X|, min and max of the resampled dB  */
};
/* Synchronises the device and copies one stage of the LAST run to host memory. */
int gance_blend_read_stage(gance_blend* blend, int32_t stage, void* h_out, uint64_t num_bytes);

/* ---- stand-alone forms of the audio -> latent stages -------------------------------------------
 * The reference exposes every stage of the chain as its own function; gance_blend_run fuses them, these
 * entry points run one stage on a caller-shaped array (all pointers device pointers, float64 where the
 * reference computes in float64). Each returns after `stream` has drained unless noted.
 *
 * gance_vec_savgol_f64            smooth_across_vectors (axis 0) / smooth_each_vector (axis 1)
 *                                 (gance/vector_sources/vector_sources_common.py:136-188): scipy.signal.savgol_filter,
 *                                 mode "interp", along one axis of [num_vectors][vector_length]; any polyorder < window_length
 * gance_vec_fourier_resample_f64  scale_vectors_to_length_resample (:211-230): scipy.signal.resample per vector
 * gance_vec_spectrogram_f64       compute_spectrogram (gance/apply_spectrogram.py:49-82): periodic-Hann windows of
 *                                 num_frequency_bins - 2 samples, hop num_frequency_bins, 20 log10(|X| / max |X|);
 *                                 d_out is [(bins - 2) / 2][frames] like the reference's array; num_frequency_bins <= 2732
 *                                 (the window, cosine and sine tables of one frame share 64 KiB of LDS)
 * gance_vec_spectrogram2_f64      the same with the reference's `truncate` argument (:75-78): truncate = 0 keeps all
 *                                 num_frequency_bins - 2 bins of the two-sided spectrum (the maximum is then taken over all
 *                                 of them, the Nyquist bin included); d_out is [bins - 2][frames]
 * gance_vec_minmax_scale_f64      sklearn minmax_scale of the whole array, in place (apply_spectrogram.py:43)
 * gance_vec_remap_f64             remap_values_into_range (:44-61): interp1d through two points (asynchronous)
 * gance_vec_rms_rolling_average   reduce_vector_rms_rolling_average (gance/vector_sources/vector_reduction.py:102-124):
 *                                 librosa RMS (hop 512) -> pandas rolling mean, NaN head = series mean -> savgol;
 *                                 num_values = 1 + (num_samples - vector_length) / 512 entries per output
 * gance_vec_rms_rolling_max       reduce_vector_rms_rolling_max (:38-58): the same RMS, then scipy.ndimage.maximum_filter1d
 *                                 of size num_values / 80 (mode "reflect") when that is > 0, else a copy (asynchronous)
 * gance_vec_quantize_f64          quantize_results_layers (:161-194): remap [min, max] -> [0, K - 1], np.rint (asynchronous)
 * gance_debug_fourier_resample_matrix  host only: the [in_length][out_length] operator the resample kernel applies
 * gance_debug_savgol_table        host only: the Savitzky-Golay operator every stage applies, window_length interior taps
 *                                 then (window_length / 2) edge rows of window_length weights each; `count` must be
 *                                 window_length + (window_length / 2) * window_length; the argument checks of gance_vec_savgol_f64 */
int gance_vec_savgol_f64(const double* d_in, int32_t num_vectors, int32_t vector_length, int32_t axis, int32_t window_length,
                         int32_t polyorder, double* d_out, void* stream);
int gance_vec_fourier_resample_f64(const double* d_in, int32_t num_vectors, int32_t in_length, int32_t out_length, double* d_out,
                                   void* stream);
int gance_vec_spectrogram_f64(const float* d_audio, uint64_t num_samples, int32_t num_frequency_bins, double* d_out, void* stream);
int gance_vec_spectrogram2_f64(const float* d_audio, uint64_t num_samples, int32_t num_frequency_bins, int32_t truncate, double* d_out,
                               void* stream);
int gance_vec_minmax_scale_f64(double* d_data, uint64_t count, double lo, double hi, void* stream);
int gance_vec_remap_f64(const double* d_in, uint64_t count, double in_lo, double in_hi, double out_lo, double out_hi, double* d_out,
                        void* stream);
int gance_vec_rms_rolling_average(const float* d_audio, uint64_t num_samples, int32_t vector_length, int32_t rolling_window,
                                  int32_t savgol_window_length, int32_t savgol_polyorder, float* d_rms, double* d_rolling,
                                  double* d_smoothed, int32_t num_values, void* stream);
int gance_vec_rms_rolling_max(const float* d_audio, uint64_t num_samples, int32_t vector_length, float* d_rms, float* d_out,
                              int32_t num_values, void* stream);
int gance_vec_quantize_f64(const double* d_in, int32_t count, int32_t num_indices, int64_t* d_out, void* stream);
int gance_debug_fourier_resample_matrix(int32_t in_length, int32_t out_length, double* h_out);
int gance_debug_savgol_table(int32_t window_length, int32_t polyorder, double* h_out, uint64_t count);

/* ------------------------------------------------------------------------------------------ */
/* Post-synthesis resize (next row f-2)                                                        */
/* ------------------------------------------------------------------------------------------ */

/*
 * Replaces resize_source's cv2.resize(image, (side, side), interpolation=cv2.INTER_CUBIC)
 * (gance/image_sources/video_common.py:399-429) for square uint8 RGB frames resident in HBM:
 * d_in [batch][src_side][src_side][3] -> d_out [batch][dst_side][dst_side][3]. Float bicubic,
 * a = -0.75, replicated border, round half up (OpenCV's 11-bit fixed point is not reproduced:
 * parity unpinned). Asynchronous on `stream`.
 */
int gance_resize_bicubic_u8(const uint8_t* d_in, int32_t batch, int32_t src_side, uint8_t* d_out,
                            int32_t dst_side, void* stream);

/* ---- smoothed-noise vector source (noise-blend) ------------------------------------------------
 * Replaces gaussian_data (gance/vector_sources/primatives.py:49-74) after its MT19937 draw, and the
 * minmax_scale(noise, (-4, 4)) of alpha_blend_vectors_max_rms_power_audio
 * (gance/data_into_network_visualization/visualization_inputs.py:135-142).
 * d_randn  [num_vectors][vector_length] float32 standard-normal draws (device; the caller's
 *          np.random.RandomState(1234).randn(...).astype(float32), primatives.py:66-68)
 * sigma_across / sigma_within   scipy.ndimage.gaussian_filter sigmas over vectors / inside a
 *          vector (mode "wrap", truncate 4.0); 0 skips the axis, as scipy does
 * feature_range  NULL, or {lo, hi}: min-max scale the RMS-normalised field to [lo, hi]
 * d_out    [num_vectors][vector_length] float32 (device, != d_randn)
 * Runs on `stream` of the current device and returns after the stream has drained. */
int gance_gaussian_noise(const float* d_randn, int32_t num_vectors, int32_t vector_length, double sigma_across,
                         double sigma_within, const double* feature_range, float* d_out, void* stream);

/* ---- eye-tracking overlay gate (pixel work only; the landmark detector stays external) ---------
 * gance_phash_crops_u8 replaces imagehash.phash(Image.fromarray(frame).crop(box)) of
 * compute_eye_tracking_overlay (gance/overlay/overlay_eye_tracking.py:100-108): PIL convert("L"),
 * PIL resize((32, 32), LANCZOS), scipy.fftpack.dct on both axes, top-left 8x8 > median.
 * d_frames [num_frames][side][side][3] uint8 (device); h_crops [num_crops][5] int32 (host):
 * frame index, x, y, width, height (a BoundingBox, overlay_common.py:19-27), inside the frame;
 * h_hashes [num_crops] uint64 (host): bit 63 = coefficient (0,0), row-major, i.e. the integer
 * whose hex string is str(imagehash.ImageHash). The phash distance is popcount(a ^ b).
 * Returns after `stream` has drained. */
int gance_phash_crops_u8(const uint8_t* d_frames, int32_t num_frames, int32_t side, const int32_t* h_crops,
                         int32_t num_crops, uint64_t* h_hashes, void* stream);

/* gance_overlay_boxes_u8 replaces write_boxes_onto_image (gance/overlay/overlay_common.py:104-172):
 * out = background, and foreground inside the padded rectangle _draw_mask draws around each
 * bounding box (x_pad = 0.098 side, y_pad = 0.058 side around the box's vertical centre, PIL
 * polygon with outline: inclusive integer bounds, corners truncated toward zero).
 * All three frame arrays are [num_frames][side][side][3] uint8 on the device; out may alias
 * background. h_boxes [num_boxes][5] int32 (host): frame index, x, y, width, height.
 * Returns after `stream` has drained. */
int gance_overlay_boxes_u8(const uint8_t* d_foreground, const uint8_t* d_background, uint8_t* d_out, int32_t num_frames,
                           int32_t side, const int32_t* h_boxes, int32_t num_boxes, void* stream);

/* ---- audio time-stretch ---------------------------------------------------------------------
 * Replaces resampy.resample(wav, sr_orig, sr_new) (resampy 0.2.2, filter "kaiser_best") of
 * _scale_wav_to_sample_rate (gance/vector_sources/music.py:212-230) inside read_wavs_scale_for_video
 * (:60-169), restated operation for operation: the 32 769-entry Kaiser-windowed-sinc half window
 * (64 zero crossings x 512 entries, beta 14.769656459379492, roll-off 0.9475937167399596), linear
 * interpolation between table entries, the running-sum time register, left wing then right wing, and the
 * accumulation in the signal's own dtype (one rounding to float32 per tap for a float32 signal). A ratio of
 * exactly 1 still filters. num_out must equal (uint64_t)(num_in * sr_new / sr_orig), resampy's length rule
 * (test/test_vector_source_music.py:13-24). Pinned by test/test_dynamic_model_switching.py:15-39 (claps.wav,
 * RMS of the first vector = 0.00298562). Device pointers; returns after `stream` has drained. */
int gance_resample_audio_f32(const float* d_in, uint64_t num_in, double sr_orig, double sr_new, float* d_out,
                             uint64_t num_out, void* stream);
int gance_resample_audio_f64(const double* d_in, uint64_t num_in, double sr_orig, double sr_new, double* d_out,
                             uint64_t num_out, void* stream);
/* host only: the filter table the resampler interpolates (count must be 32769) */
int gance_debug_resample_filter(double* h_out, uint64_t count);

/* ---- Motion-JPEG frame encoder -----------------------------------------------------------------
 * Replaces the video encode of write_source_to_disk_forward (gance/image_sources/video_common.py:301-376:
 * ffmpeg / x264 crf 18, yuv422p, high_quality=True) whose file add_wavs_to_video (:67-79) then muxes: frames are encoded in HBM as baseline JFIF
 * files (4:2:2, the Annex K tables scaled by `quality` as libjpeg's jpeg_set_quality does, standard
 * Huffman tables, one restart interval per MCU row: DRI = side / 16), arithmetic as libjpeg's islow
 * path, so libjpeg decodes them to exactly the pixels of its own encode at that quality.
 * gance_jpeg_encode_bounds: host only; the workspace and output capacity one call of (batch, side)
 * needs. Both are worst-case sizes (a block is at most 1660 bits before 0xFF stuffing): the encoder
 * cannot truncate. batch >= 1, side a multiple of 16 in [16, 8192].
 * gance_jpeg_encode_u8: d_frames [batch][side][side][3] uint8 (device, 16-byte aligned); quality 1..100;
 * d_workspace (device, 16-byte aligned) of workspace_bytes; d_out (device) receives the batch's files
 * back to back, frame b at [d_offsets[b], d_offsets[b + 1]); d_offsets [batch + 1] int64 (device).
 * Asynchronous on `stream`; the bytes are the same whatever the batch a frame is encoded in.
 * Returns GANCE_ERR_INVALID_ARGUMENT before touching a device for a bad side, quality, or a workspace or
 * capacity below the bounds. */
int gance_jpeg_encode_bounds(int32_t batch, int32_t side, uint64_t* workspace_bytes, uint64_t* out_capacity);
int gance_jpeg_encode_u8(const uint8_t* d_frames, int32_t batch, int32_t side, int32_t quality, void* d_workspace,
                         uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream);

/* Frames [batch][height][width][3] of any 4:2:2-compatible size (the debug video is a row of square panels:
 * horizontal_concat_images at gance/projection_file_blend.py:302-334, written with high_quality=False at :335-341
 * "because this video can be shaped very weird"). width and height are multiples of 16 in [16, 8192], DRI = width / 16;
 * everything else as gance_jpeg_encode_bounds / gance_jpeg_encode_u8, which are these with width = height = side and
 * produce the same bytes as before. */
int gance_jpeg_encode_rect_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity);
int gance_jpeg_encode_rect_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, int32_t quality,
                              void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                              int64_t* d_offsets, void* stream);

/* The same files with per-frame optimised Huffman tables (libjpeg's optimize_coding, PIL's optimize=True): each frame's four
 * DHT segments are jchuff.c's jpeg_gen_optimal_table of that frame's own symbol counts (htest_one_block: DC categories with
 * the predictors reset per restart interval, AC run/size pairs over the zigzag order, luma into tables 0, Cb and Cr into
 * tables 1), limited to 16 bits as Annex K.3 does. Quantised coefficients, and so the decoded pixels, are those of
 * gance_jpeg_encode_rect_u8; only the DHT segments and the entropy-coded bytes differ, and the header length differs per
 * frame. A frame whose merge gives a code of more than 32 bits (libjpeg's JERR_HUFF_CLEN_OVERFLOW) is coded with the four
 * Annex K tables. Arguments and checks as gance_jpeg_encode_rect_*; the output capacity is the same, the workspace larger
 * by about 8.5 KiB per frame. Deterministic (the counts are integer sums); a frame's bytes do not depend on its batch. */
int gance_jpeg_encode_rect_optimized_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes,
                                            uint64_t* out_capacity);
int gance_jpeg_encode_rect_optimized_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, int32_t quality,
                                        void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                        int64_t* d_offsets, void* stream);
/* The table build of the above on given counts: d_counts [n][256] int32 (device; negative counts as 0) -> d_bits [n][16]
 * uint8 (codes per length 1..16), d_values [n][256] uint8 (the symbols in code order, the rest 0) and d_status [n] int32:
 * 0 a table, 1 a code of more than 32 bits before the limiting (the encoder then uses the Annex K tables), 2 no symbol
 * counted; bits and values are 0 unless the status is 0. Asynchronous on `stream`. */
int gance_jpeg_optimal_tables(const int32_t* d_counts, int32_t n, uint8_t* d_bits, uint8_t* d_values, int32_t* d_status,
                              void* stream);

/* ---- PNG still encoder -------------------------------------------------------------------------
 * Replaces PIL's Image.save(format="PNG") of write_image (gance/image_sources/still_image_common.py:19-28) and of
 * synthesize_images.py:188-191: frames are encoded in HBM as standard PNG files (signature, IHDR with 8-bit depth,
 * colour type 2, no interlace, IDAT chunks, IEND). Each row takes the filter (None, Sub, Up, Average, Paeth) with the
 * smallest sum of |int8(filtered byte)|, ties to the lowest number; the filtered stream is deflated in independent
 * segments of 32768 bytes, each one dynamic-Huffman block over literals and end-of-block (no match search) closed by
 * an empty stored block, or one stored block whenever that is not larger; one IDAT chunk per segment and one for the
 * Adler-32. A frame of one flat colour therefore costs about 1 bit per byte (gance_png_encode_lz_u8 below does not).
 * gance_png_encode_bounds: host only; the workspace and output capacity one call needs. The capacity is exact for
 * the worst case (every segment stored): batch * (63 + 17 * segments + height * (3 * width + 1)).
 * batch >= 1, width and height in [1, 8192].
 * gance_png_encode_u8: d_frames [batch][height][width][3] uint8 RGB (device); d_workspace (device, 16-byte aligned)
 * of workspace_bytes; d_out (device) receives the files back to back, frame b at [d_offsets[b], d_offsets[b + 1]);
 * d_offsets [batch + 1] int64 (device). Asynchronous on `stream`; a frame's bytes are the same whatever the batch it
 * is encoded in. Returns GANCE_ERR_INVALID_ARGUMENT before touching a device for a NULL pointer, a size out of range,
 * or a workspace or capacity below the bounds. */
int gance_png_encode_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity);
int gance_png_encode_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, void* d_workspace,
                        uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream);

/* The same encoder with an LZ77 match search, for frames with flat or repeating areas (plot panels, masks, smooth
 * output). Filter, container, segments, Adler-32 and CRCs are those of gance_png_encode_u8; each segment takes the
 * smallest of (a) one stored block, (b) the literal-only dynamic block plus the empty stored block, (c) one dynamic block
 * of literals, length / distance pairs (RFC 1951: lengths 3 .. 258, overlapping copies allowed) and end-of-block plus the
 * same empty stored block; on equal sizes the earlier. (a) and (b) are gance_png_encode_u8's bytes of that segment, so a
 * file is never larger than its file of the same frame, and noisy texture comes out byte for byte the same. A match never
 * reaches before its own segment's first byte: every segment inflates alone. The parse is greedy with a single-entry
 * hash table (zlib level 1's design point); see DESIGN.md section 9 item 14 for measured sizes and rates.
 * gance_png_encode_lz_bounds: the capacity is gance_png_encode_bounds' (the stored form stays the worst case); the
 * workspace is larger by 4 * 32768 bytes per segment (one 4-byte token per filtered byte), about five times the other's.
 * gance_png_encode_lz_u8: the contract and the refusals of gance_png_encode_u8. */
int gance_png_encode_lz_bounds(int32_t batch, int32_t width, int32_t height, uint64_t* workspace_bytes, uint64_t* out_capacity);
int gance_png_encode_lz_u8(const uint8_t* d_frames, int32_t batch, int32_t width, int32_t height, void* d_workspace,
                           uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, int64_t* d_offsets, void* stream);

/* ---- Motion-JPEG frame decoder -----------------------------------------------------------------
 * The other half of the encoder above, and what frames_in_video (gance/image_sources/video_common.py:229-298) gets from
 * cv2.VideoCapture: baseline sequential JFIF files (SOF0, 8 bit, three components sampled 2x1 / 1x1 / 1x1, one
 * interleaved scan, any 8-bit DQT, any DHT or none (then the Annex K tables, the "AVI1" form), any DRI or none, width
 * and height in [1, 8192]) decoded in HBM to uint8 [batch][height][width][3] RGB, equal pixel for pixel to libjpeg's
 * default decode (jidctint.c jpeg_idct_islow with samples saturated to 0..255, jdsample.c h2v1_fancy_upsample, jdcolor.c
 * ycc_rgb_convert; a frame of width 3 or 4 has a chroma width of 2, where libjpeg replicates the chroma samples instead).
 * Restart segments decode in parallel; a file without DRI is one segment (correct, slow).
 * gance_jpeg_parse_header: host only; `file` [file_bytes] is one JFIF file (host memory), `info` receives its
 * description: sizes, restart interval (0 = none), where the entropy-coded data starts (scan_offset) and how many bytes
 * follow it to the end of the file (scan_bytes: the EOI is found on the device), and per component (Y, Cb, Cr) the
 * quantisation table (natural order) and the DC / AC Huffman tables (code counts per length 1..16, then the symbols).
 * Returns GANCE_ERR_INVALID_ARGUMENT with the reason in gance_last_error for a file that is cut short or not of the
 * form above (progressive or another SOFn, 4:2:0, 4:4:4, grey, 12-bit samples, a 16-bit DQT, more than one scan) or whose
 * Huffman tables are not valid (more than 256 codes, an over-subscribed code, a DC category above 11).
 * gance_jpeg_decode_bounds: host only; the workspace one decode call of `batch` frames of width x height whose files
 * total `total_bytes` needs.
 * gance_jpeg_decode_u8: d_data (device) holds the batch's files, frame b at [h_offsets[b], h_offsets[b + 1]) (h_offsets
 * [batch + 1] and infos [batch] on the host, infos[b] as parsed from frame b: all of one width and height); d_workspace
 * (device, 16-byte aligned); d_out (device) [batch][height][width][3]; d_status [batch] int32 (device) receives
 * GANCE_JPEG_OK or the first reason frame b could not be decoded: its pixels are then unspecified, every other frame's
 * are unaffected. No read leaves a frame's own byte range. Asynchronous on `stream` (the tables travel through a pinned
 * buffer the library owns); a frame's pixels are a pure function of its bytes, the same whatever the batch.
 * Returns GANCE_ERR_INVALID_ARGUMENT before touching a device for a NULL pointer, frames of different sizes, a
 * description parse_header would not produce for the frame's range, or a workspace below the bounds. */
enum { GANCE_JPEG_OK = 0, GANCE_JPEG_TRUNCATED = 1, GANCE_JPEG_INVALID_CODE = 2, GANCE_JPEG_MARKER_MISMATCH = 3 };
typedef struct gance_jpeg_info {
    int32_t width, height;
    int32_t restart_interval;    /* MCUs (16 x 8 pixels) per restart segment, 0 = no restart markers */
    int32_t has_huffman_tables;  /* 0: the file has no DHT and the Annex K tables were filled in */
    uint64_t scan_offset, scan_bytes;
    uint8_t quant[3][64];
    uint8_t huff_bits[3][2][16]; /* [component][0 = DC, 1 = AC] */
    uint8_t huff_values[3][2][256];
} gance_jpeg_info;
int gance_jpeg_parse_header(const uint8_t* file, uint64_t file_bytes, gance_jpeg_info* info);
int gance_jpeg_decode_bounds(int32_t batch, int32_t width, int32_t height, uint64_t total_bytes, uint64_t* workspace_bytes);
int gance_jpeg_decode_u8(const uint8_t* d_data, const int64_t* h_offsets, const gance_jpeg_info* infos, int32_t batch,
                         void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, int32_t* d_status, void* stream);

/* The same decoder for the four baseline layouts a video from elsewhere comes in; the three entries above are these with
 * the layout held to 4:2:2, and keep their refusals word for word. One interleaved scan of all components:
 *   layout                   components (H x V)    MCU       blocks per MCU, in order
 *   GANCE_JPEG_LAYOUT_422    2x1, 1x1, 1x1         16 x 8    Y left, Y right, Cb, Cr
 *   GANCE_JPEG_LAYOUT_420    2x2, 1x1, 1x1         16 x 16   Y00, Y01, Y10, Y11 (raster order inside the MCU), Cb, Cr
 *   GANCE_JPEG_LAYOUT_444    1x1, 1x1, 1x1         8 x 8     Y, Cb, Cr
 *   GANCE_JPEG_LAYOUT_GREY   one, any factors      8 x 8     Y (decoded to RGB with three equal channels)
 * The restart interval counts MCUs of the file's own layout. Upsampling is libjpeg's default: h2v1_fancy_upsample (4:2:2)
 * and h2v2_fancy_upsample (4:2:0) over the component's true size ceil(W / 2) [x ceil(H / 2)], and plain replication for
 * both when that width is at most 2 (W <= 4), as jdsample.c chooses; none for 4:4:4.
 * gance_jpeg_parse_header_layouts: as gance_jpeg_parse_header; info->layout receives the layout. For grey only
 * component 0's tables are meaningful, the rest are zero. Still refused, with a reason that names it: other sampling
 * factors (4:4:0, 4:1:1, ...), two or four components, progressive and the other SOFn, 12-bit samples, a 16-bit DQT,
 * more than one scan.
 * gance_jpeg_decode_layouts_bounds / gance_jpeg_decode_layouts_u8: as gance_jpeg_decode_bounds / gance_jpeg_decode_u8;
 * all frames of a call share width, height and layout (GANCE_ERR_INVALID_ARGUMENT, "one layout", before a device is
 * touched, otherwise). The workspace of 4:2:2 is that of gance_jpeg_decode_bounds. */
enum { GANCE_JPEG_LAYOUT_422 = 0, GANCE_JPEG_LAYOUT_420 = 1, GANCE_JPEG_LAYOUT_444 = 2, GANCE_JPEG_LAYOUT_GREY = 3 };
typedef struct gance_jpeg_frame_info {
    gance_jpeg_info info;
    int32_t layout; /* GANCE_JPEG_LAYOUT_* */
    int32_t reserved;
} gance_jpeg_frame_info;
int gance_jpeg_parse_header_layouts(const uint8_t* file, uint64_t file_bytes, gance_jpeg_frame_info* info);
int gance_jpeg_decode_layouts_bounds(int32_t batch, int32_t width, int32_t height, int32_t layout, uint64_t total_bytes,
                                     uint64_t* workspace_bytes);
int gance_jpeg_decode_layouts_u8(const uint8_t* d_data, const int64_t* h_offsets, const gance_jpeg_frame_info* infos, int32_t batch,
                                 void* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, int32_t* d_status, void* stream);

/* ---- debug-video panels ------------------------------------------------------------------------
 * Replaces the per-frame matplotlib drawing of the debug video: fig.canvas.draw() per frame in
 * render_current_matplotlib_frame (gance/data_into_network_visualization/visualization_common.py) under
 * _write_data_to_axes (network_visualization.py:254-400), visualize_overlay_computation
 * (gance/overlay/overlay_visualization.py:128-234) and visualize_result_layers (visualize_vector_reduction.py:85-179),
 * and the horizontal_concat_images of gance/projection_file_blend.py:302-334.
 * A debug frame is a row of square panels; both entries write ONE panel [side][side][3] of `batch` consecutive
 * frames: panel row r of frame b starts at d_out + b * out_frame_stride + r * out_row_stride (bytes; d_out and both
 * strides 16-byte aligned; side a multiple of 16 in [16, 4096]). Asynchronous on `stream`, no host synchronisation;
 * the bytes written are a pure function of the arguments (the same however the frames are split into calls).
 * Both return GANCE_ERR_INVALID_ARGUMENT before touching a device for a NULL pointer, a bad side or stride, a source
 * index outside `src_count`, or a table that fails the rules below. */
#define GANCE_DEBUG_MAX_AXES 8
#define GANCE_DEBUG_MAX_MARKS 24
enum { GANCE_DEBUG_MARK_POINTS = 0, GANCE_DEBUG_MARK_POLYLINE = 1, GANCE_DEBUG_MARK_CURSOR = 2, GANCE_DEBUG_MARK_BAR = 3 };
enum { GANCE_DEBUG_F32 = 0, GANCE_DEBUG_F64 = 1, GANCE_DEBUG_I32 = 2 };
/* pixel rectangle inside the panel and the data limits mapped onto it; rectangles of one call must not overlap */
typedef struct gance_debug_axis {
    int32_t x, y, width, height;
    double x_min, x_max, y_min, y_max; /* finite, min != max */
} gance_debug_axis;
/* One mark. Sample i of a series is at x = x_start + i and reads data[(frame.number / frame_divisor) * frame_stride + i]
 * (skipped when that index is outside [0, limit) or the value is not finite). POINTS: a filled square per sample
 * (ax.scatter). POLYLINE: the samples joined (ax.plot; dash_on / dash_off in pixel columns, 0 = solid). CURSOR: a
 * vertical line over the axis height at x = frame.cursor (axvline / vlines; no series). BAR: a horizontal bar from
 * x = 0 to x = sample 0 over the middle half of the axis (barh). Drawn iff (frame.flags & flag_mask) == flag_value. */
typedef struct gance_debug_mark {
    int32_t kind, axis, dtype, count;
    const void* data; /* device, aligned to its element */
    int64_t limit, frame_stride;
    int32_t frame_divisor, size; /* size: side of the square stamped per sample / line step, 1 .. 64 pixels */
    int32_t dash_on, dash_off;
    int32_t flag_mask, flag_value;
    uint8_t rgba[4]; /* alpha 0 .. 255 */
    int32_t reserved;
    double x_start;
} gance_debug_mark;
typedef struct gance_debug_frame {
    int64_t number; /* frame number (>= 0) the series rows are derived from */
    double cursor;  /* x of CURSOR marks */
    int32_t flags, reserved;
} gance_debug_frame;
/* image panels: frame b shows d_src[(first_number + b) / divisor - src_base] of [src_count][side][side][3] (device,
 * 16-byte aligned): divisor 1 for the stream's own frames, frame_multiplier for reader.final_images / target_images */
int gance_debug_place_panels_u8(const uint8_t* d_src, int32_t src_count, int32_t side, int64_t first_number, int32_t divisor,
                                int64_t src_base, int32_t batch, uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride,
                                void* stream);
/* plot panels: d_chrome [side][side][3] (device: the window's static template) copied to every frame, then `marks`
 * (host, <= GANCE_DEBUG_MAX_MARKS) composited in table order on `axes` (host, <= GANCE_DEBUG_MAX_AXES) with the per-frame
 * values of d_frames [batch] (device). The rasterisation rule is in DESIGN.md section 9 and gance_amd/csrc/debug_panels.hip. */
int gance_debug_draw_panels_u8(const uint8_t* d_chrome, int32_t side, const gance_debug_axis* axes, int32_t num_axes,
                               const gance_debug_mark* marks, int32_t num_marks, const gance_debug_frame* d_frames, int32_t batch,
                               uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride, void* stream);
/* The 3-D view of the synthesis inputs (plot_vectors_3d / draw_y_point of gance/data_into_network_visualization/vectors_3d.py,
 * network_visualization.py:133-142, 269-285): every element of every input vector of the run as a point (x = sample
 * number, y = vector number, z = value) coloured by its value, and a marker that moves along y. The rasterisation rule is
 * in DESIGN.md section 9 item 8 and gance_amd/csrc/scatter3d.hip. The view is orthographic: u_k = (p_k - lo_k) /
 * (hi_k - lo_k) - 0.5, then the dot products with `right` (to the right on the panel), `up` and `toward` (towards the
 * viewer: nearer points hide farther ones). All limits finite with min != max; no view vector all zero. */
typedef struct gance_debug_view3d {
    int32_t x, y, width, height; /* pixel rectangle inside the panel the projected unit cube is fitted to */
    double x_min, x_max, y_min, y_max, z_min, z_max;
    double c_min, c_max; /* the values mapped onto LUT entries 0 .. 255 */
    double right[3], up[3], toward[3];
    int32_t point_size, marker_size; /* side of the square stamped per point / for the marker, 1 .. 64 pixels */
    uint8_t marker_rgb[3];
    uint8_t reserved0;
    int32_t reserved1;
    double marker_x, marker_z; /* the marker of a frame sits at (marker_x, frame.cursor, marker_z) */
} gance_debug_view3d;
/* the template of a run: d_chrome [side][side][3] (device) with the cloud on top, into d_template [side][side][3] (both
 * 16-byte aligned). Point (n, i) reads d_values[n * vector_stride + i] (device, GANCE_DEBUG_F32 or GANCE_DEBUG_F64,
 * vector_stride >= vector_length in elements: 18 L reads row 0 of [N][18][L]); a value that is not finite is not drawn.
 * At every pixel the point with the largest (depth level, n * vector_length + i) shows, as d_lut[c] ([256][3], device).
 * d_keys: a workspace of side * side 64-bit words (device), zeroed here. num_vectors * vector_length in [1, 2^40).
 * Asynchronous on `stream`, no host synchronisation; the bytes are a pure function of the arguments. */
int gance_debug_scatter3d_u8(const uint8_t* d_chrome, int32_t side, const gance_debug_view3d* view, const void* d_values, int32_t dtype,
                             int64_t num_vectors, int64_t vector_length, int64_t vector_stride, const uint8_t* d_lut, uint64_t* d_keys,
                             uint8_t* d_template, void* stream);
/* one panel of `batch` consecutive frames (d_out and the strides as above): d_template copied to every frame with the
 * marker at y = d_frames[b].cursor stamped on top in marker_rgb, opaque, clipped to the rectangle (not drawn where the
 * cursor is not finite) */
int gance_debug_draw_scatter3d_u8(const uint8_t* d_template, int32_t side, const gance_debug_view3d* view, const gance_debug_frame* d_frames,
                                  int32_t batch, uint8_t* d_out, int64_t out_frame_stride, int64_t out_row_stride, void* stream);
/* Per-frame text on one panel of `batch` consecutive frames (d_out and the strides as above), written ON TOP of what is
 * there: call it after gance_debug_draw_panels_u8. The string of frame b is the bytes d_text[b * text_stride ...] (device)
 * up to the first NUL, or all text_stride bytes; a byte outside 32 .. 126 is drawn as '?'. Glyph i of the 5 x 7 font
 * (gance_amd/csrc/debug_font.h) covers the columns x + i * 6 * scale ... + 5 * scale - 1 and the rows y ... y + 7 * scale - 1;
 * a pixel whose glyph bit is set becomes `rgb` (0x00BBGGRR: red in the low byte), opaque; no other pixel is written.
 * Pixels are clipped to the panel and to the columns [x, x + max_width). side a multiple of 16 in [16, 4096], text_stride
 * in [1, 256], scale in [1, 64], max_width >= 1, x and y in [0, side), batch >= 1, d_out and both strides 16-byte aligned,
 * out_row_stride >= 3 * side and out_frame_stride >= a whole panel ((side - 1) rows + 3 * side). Asynchronous on `stream`, no host
 * synchronisation; the bytes are a pure function of the arguments. */
int gance_debug_draw_text_u8(const uint8_t* d_text, int32_t text_stride, int32_t x, int32_t y, int32_t max_width, int32_t scale,
                             uint32_t rgb, int32_t side, int32_t batch, uint8_t* d_out, int64_t out_frame_stride,
                             int64_t out_row_stride, void* stream);
/* the font's table: 95 glyphs x 5 column bytes, bit 0 = top row (host only, no GPU needed); count must be 475 */
int gance_debug_font_columns(uint8_t* h_out, uint64_t count);

/* ------------------------------------------------------------------------------------------ */
/* Differentiable synthesis: forward and backward of the generator's three layer operations   */
/* ------------------------------------------------------------------------------------------ */
/*
 * The plain-form path behind torch.ops.gance.modconv3x3 / noise_bias_lrelu / torgb_skip and
 * gance_amd/stylegan2/differentiable.py: the image's gradient with respect to the dlatents,
 * which the engine's forward-only kernel forms cannot give. Every tensor is float32, C-contiguous, NCHW, on the device;
 * every call is asynchronous on `stream` without host synchronisation, uses no floating-point atomics and sums in one
 * fixed order: the bits are a pure function of the arguments. Refused with GANCE_ERR_INVALID_ARGUMENT before a device is
 * touched: a NULL pointer (except where noted), a pointer that is not 4-byte aligned, a channel count that is not a multiple
 * of 16 in [16, 512], height != width, a side outside [4, 1024] (an up layer's input side outside [4, 512]), a batch
 * outside [1, 65535] or so large that batch * channels * (2 side + 1)^2 passes 2^31 - 1, a workspace below the bound.
 *
 * Modulated 3x3 conv (modulated_conv2d_layer of the published network with the style and the demodulation as inputs):
 *   y[b,o] = demod[b,o] * sum_{i,tap} weight[tap,i,o] * style[b,i] * x[b,i]     zero padding 1; weight [3][3][cin][cout] runtime-scaled
 * with up != 0 the stride-2 transposed conv and the [1,3,3,1] FIR of upsample_conv_2d: x [batch][cin][side][side] ->
 * y [batch][cout][2 side][2 side]. The backward gives grad_x (shape of x), grad_style [batch][cin] and grad_demod
 * [batch][cout] (demod > 0); there is no weight gradient. d_y is the forward's output. Both contractions run on
 * v_mfma_f32_16x16x4_f32. The workspace (16-byte multiples, any 4-byte aligned address) serves either direction.
 */
int gance_modconv3x3_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t side, int32_t up, uint64_t* workspace_bytes);
int gance_modconv3x3_forward(const float* d_x, const float* d_style, const float* d_demod, const float* d_weight, int32_t batch, int32_t cin,
                             int32_t cout, int32_t height, int32_t width, int32_t up, float* d_y, void* d_workspace, uint64_t workspace_bytes,
                             void* stream);
int gance_modconv3x3_backward(const float* d_grad_y, const float* d_x, const float* d_y, const float* d_style, const float* d_demod,
                              const float* d_weight, int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t up,
                              float* d_grad_x, float* d_grad_style, float* d_grad_demod, void* d_workspace, uint64_t workspace_bytes,
                              void* stream);
/*
 * out = lrelu_0.2(x + noise * strength + bias[c]) * sqrt(2): x, out [batch][channels][side][side], d_noise
 * [noise_batch = 1 or batch][1][side][side], d_strength one float on the device, d_bias [channels]. The backward reads the
 * slope off the sign of the saved output (leaky ReLU keeps the sign) and gives grad_x; d_grad_noise, d_grad_strength and
 * d_grad_bias are reserved and must be NULL (the noise gradient has an entry point of its own, below).
 */
int gance_noise_bias_lrelu_forward(const float* d_x, const float* d_noise, int32_t noise_batch, const float* d_strength, const float* d_bias,
                                   int32_t batch, int32_t channels, int32_t height, int32_t width, float* d_out, void* stream);
int gance_noise_bias_lrelu_backward(const float* d_grad_out, const float* d_out, int32_t batch, int32_t channels, int32_t height, int32_t width,
                                    float* d_grad_x, float* d_grad_noise, float* d_grad_strength, float* d_grad_bias, void* stream);
/*
 * The same backward with the noise gradient, in one pass over grad_out and out: d_grad_x as above (the same bits), and
 * d_grad_noise [noise_batch][1][side][side], grad_noise[n][p] = strength * sum_c grad_x[b][c][p] over the samples b that
 * read plane n (noise_batch 1: every sample, in rising order). The order of the sum is a function of the shape alone.
 */
int gance_noise_bias_lrelu_backward_noise(const float* d_grad_out, const float* d_out, const float* d_strength, int32_t noise_batch, int32_t batch,
                                          int32_t channels, int32_t height, int32_t width, float* d_grad_x, float* d_grad_noise, void* stream);
/*
 * ToRGB of the skip architecture: y = upsample_2d(y_prev) + sum_i weight[i,c] * style[b,i] * x[b,i] + bias[c], no
 * demodulation: x [batch][cin][side][side], weight [cin][3], y [batch][3][side][side], d_y_prev [batch][3][side / 2][side / 2]
 * or NULL (the 4x4 layer; with it the side must be even). The backward gives grad_x, grad_style [batch][cin] and, unless
 * d_grad_y_prev is NULL, the transpose of the zero-insert + FIR upsample applied to grad_y.
 */
int gance_torgb_skip_workspace_bytes(int32_t batch, int32_t cin, int32_t side, uint64_t* workspace_bytes);
int gance_torgb_skip_forward(const float* d_x, const float* d_style, const float* d_weight, const float* d_bias, const float* d_y_prev,
                             int32_t batch, int32_t cin, int32_t height, int32_t width, float* d_y, void* stream);
int gance_torgb_skip_backward(const float* d_grad_y, const float* d_x, const float* d_style, const float* d_weight, int32_t batch, int32_t cin,
                              int32_t height, int32_t width, float* d_grad_x, float* d_grad_style, float* d_grad_y_prev, void* d_workspace,
                              uint64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Projection: the losses of gance_amd/stylegan2/projector.py   */
/* ------------------------------------------------------------------------------------------ */
/*
 * Float32, C-contiguous, on the device, asynchronous on `stream`, no atomics and one fixed summation order, as above.
 * Refused with GANCE_ERR_INVALID_ARGUMENT before a device is touched: a NULL or misaligned pointer, a batch outside
 * [1, 65535], a side that is not a power of two in the stated range, a workspace below the bound.
 *
 * Noise regulariser of StyleGAN2's projector, per sample over planes d_noise [batch][1][side][side], side a power of two in
 * [4, 1024]:  reg = 0;  repeat { reg += mean(v * roll(v, 1, W))^2 + mean(v * roll(v, 1, H))^2;  stop if side <= 8;
 * v = 2x2 mean of v }  (the roll wraps). levels = max(1, log2(side) - 2). The forward writes d_reg [batch] and the two means
 * of every level, d_means [batch][levels][2], and leaves the pyramid in the workspace; the backward takes d_means and the
 * same workspace, unchanged since the forward, and gives d_grad_noise [batch][1][side][side] from d_grad_reg [batch].
 */
int gance_noise_regularizer_workspace_bytes(int32_t batch, int32_t side, uint64_t* workspace_bytes);
int gance_noise_regularizer_forward(const float* d_noise, int32_t batch, int32_t side, float* d_reg, float* d_means, void* d_workspace,
                                    uint64_t workspace_bytes, void* stream);
int gance_noise_regularizer_backward(const float* d_grad_reg, const float* d_noise, const float* d_means, const void* d_workspace,
                                     uint64_t workspace_bytes, int32_t batch, int32_t side, float* d_grad_noise, void* stream);
/*
 * Pyramid distance (weight-free; NOT the LPIPS of the published projector): d_image [batch][3][R][R] in -1 ... 1, R a power of
 * two in [8, 1024]; d_target [batch][3][T][T] in 0 ... 255, T = min(R, 256), f = R / T.  p = f x f area mean of
 * (image + 1) * 127.5;  d_0 = (p - target) / 255;  d_l = 2x2 mean of d_(l-1) while the side of d_(l-1) is above 8;
 * dist[b] = sum_l mean over channels and pixels of d_l^2. The forward leaves the d_l in the workspace; the backward takes the
 * same workspace, unchanged since, and gives d_grad_image [batch][3][R][R] from d_grad_dist [batch].
 */
int gance_pyramid_distance_workspace_bytes(int32_t batch, int32_t resolution, uint64_t* workspace_bytes);
int gance_pyramid_distance_forward(const float* d_image, const float* d_target, int32_t batch, int32_t resolution, float* d_dist,
                                   void* d_workspace, uint64_t workspace_bytes, void* stream);
int gance_pyramid_distance_backward(const float* d_grad_dist, const void* d_workspace, uint64_t workspace_bytes, int32_t batch,
                                    int32_t resolution, float* d_grad_image, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* LPIPS on VGG16: what gance_amd/stylegan2/lpips.py adds to gance_modconv3x3 */
/* ------------------------------------------------------------------------------------------ */
/*
 * Float32, C-contiguous, NCHW, square, on the device, asynchronous on `stream`, no atomics and one fixed summation order, as
 * above. Refused with GANCE_ERR_INVALID_ARGUMENT before a device is touched: a NULL or misaligned pointer, a batch outside
 * [1, 65535], a channel count that is not a multiple of 16 in [16, 512], a side outside [4, 1024], an odd side with `pool`, a
 * resolution that is not a multiple of the side, a workspace below the bound.
 *
 * Input: d_image [batch][3][R][R] -> d_out [batch][16][S][S], R = resolution a multiple of S = side: channel c < 3 is
 * ((the R / S x R / S area mean) - d_shift[c]) / d_scale[c], channels 3 ... 15 are zero (conv1_1 runs with 16 input channels).
 * The backward reads d_grad [batch][16][S][S] and gives d_grad_image = grad[:, :3] / (scale_c * (R / S)^2) over each cell.
 */
int gance_lpips_input_forward(const float* d_image, const float* d_shift, const float* d_scale, int32_t batch, int32_t resolution, int32_t side,
                              float* d_out, void* stream);
int gance_lpips_input_backward(const float* d_grad, const float* d_scale, int32_t batch, int32_t resolution, int32_t side, float* d_grad_image,
                               void* stream);
/*
 * y = max(x + bias[c], 0) over [batch][channels][side][side]; with pool != 0 also d_p [batch][channels][side / 2][side / 2], the
 * maximum of each 2x2 window of y, in the same pass (without pool d_p is not read and may be NULL). The backward gives
 * grad_x = (y > 0) * (grad_y + grad_p routed to the window's selected element): the largest y of the window, the first in
 * row-major order among equals. Without pool d_grad_p is not read and may be NULL.
 */
int gance_bias_relu_forward(const float* d_x, const float* d_bias, int32_t batch, int32_t channels, int32_t side, int32_t pool, float* d_y,
                            float* d_p, void* stream);
int gance_bias_relu_backward(const float* d_grad_y, const float* d_grad_p, const float* d_y, int32_t batch, int32_t channels, int32_t side,
                             int32_t pool, float* d_grad_x, void* stream);
/*
 * The LPIPS head of one tap: per pixel n = |f|_2 over the channels, u = f / (n + 1e-10);
 * dist[b] = mean over the pixels of sum_c lin[c] * (u_c - target_c)^2, with d_target [batch][channels][side][side] already
 * normalised (gance_lpips_normalize) and d_lin [channels]. The workspace (8-byte aligned) holds one fp64 partial per block. The
 * backward recomputes n and gives d_grad_f from d_grad_dist [batch]; at an all-zero pixel the derivative of n is taken as 0.
 * gance_lpips_normalize writes u.
 */
int gance_lpips_layer_workspace_bytes(int32_t batch, int32_t side, uint64_t* workspace_bytes);
int gance_lpips_layer_forward(const float* d_f, const float* d_target, const float* d_lin, int32_t batch, int32_t channels, int32_t side,
                              float* d_dist, void* d_workspace, uint64_t workspace_bytes, void* stream);
int gance_lpips_layer_backward(const float* d_grad_dist, const float* d_f, const float* d_target, const float* d_lin, int32_t batch,
                               int32_t channels, int32_t side, float* d_grad_f, void* stream);
int gance_lpips_normalize(const float* d_f, int32_t batch, int32_t channels, int32_t side, float* d_out, void* stream);

/*
 * The plain 3x3 convolution of gance::conv3x3 (csrc/conv3x3.hip), which VGG16Lpips runs on with
 * convolution="conv3x3": y[b][o][oy][ox] = sum_{ty, tx, i} w[ty][tx][i][o] * x[b][i][oy + ty - 1][ox + tx - 1], zero padding 1,
 * stride 1 (cross-correlation: gance_modconv3x3_forward with up = 0, unit style and unit demodulation). d_x [batch][cin][S][S],
 * d_weight [3][3][cin][cout], d_y [batch][cout][S][S]; exact fp32 on v_mfma_f32_16x16x4_f32, a chunk of 16 contracted channels
 * summed on its own and then added to the total. No style, no demodulation, no weight gradient. The input gradient is the
 * same entry point applied to grad_y and wt[ty][tx][o][i] = w[2 - ty][2 - tx][i][o].
 *
 * Refused as above: a NULL or misaligned pointer, channel counts that are not multiples of 16 in [16, 512], a side outside
 * [4, 1024], height != width, a batch outside [1, 65535], a workspace below gance_conv3x3_workspace_bytes (never 0).
 *
 * gance_conv3x3_form (host only, no device): the kernel form launched for a shape, a function of (cin, cout, side) and never of
 * the batch, so a sample's bits do not depend on the batch it arrives in. form = 8 * t + s:
 *   t = 0, 1, 2: a block computes 8 x 16 pixels x 16, 32, 64 output channels (cout 16; 32 or 48; 64 and above);
 *   s = log2(splits): the chunks of contracted channels are divided over 2^s blocks whose partial sums go to the workspace and
 *   are added in rising order by a second launch. splits is the largest power of two that is at most 16 for a side up to 16,
 *   4 up to 32, 2 up to 64 and 1 above, and at most cin / 32 (no run of fewer than two chunks).
 */
int gance_conv3x3_form(int32_t cin, int32_t cout, int32_t side, int32_t* form);
int gance_conv3x3_workspace_bytes(int32_t batch, int32_t cin, int32_t cout, int32_t side, uint64_t* workspace_bytes);
int gance_conv3x3_forward(const float* d_x, const float* d_weight, int32_t batch, int32_t cin, int32_t cout, int32_t height, int32_t width,
                          float* d_y, void* d_workspace, uint64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANCE_HIP_H */
