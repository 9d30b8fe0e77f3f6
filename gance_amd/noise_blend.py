"""
noise-blend end to end: WAV(s) + network(s) -> frames, the vector-input twin of
projection-file-blend (music_into_networks.py:285-401 in the reference).

Same stages as the reference command: read the WAVs stretched to one 512-sample vector per output
frame (FPS mode), blend the spectrogram with the smoothed-noise field
(`alpha_blend_vectors_max_rms_power_audio`), feed every blended vector to the network the
rolling RMS picks, through the z entry (mapping + truncation psi 1.2 + synthesis), and scale to
`output_side_length`. Everything after the WAV read stays in HBM; with `torch.distributed`
initialised the frames are sharded across ranks exactly as in projection_file_blend.py.

`noise_blend_api` is the command: it streams the run (`noise_blend_frame_chunks`, the frame stream of
projection_file_blend.py fed with z vectors) into a memory-mapped `.npy` or a Motion-JPEG AVI with the song, and with
`debug_path` writes the reference's debug video beside it (music_into_networks.py:380-398: the hero frame next to the
synthesis-inputs plot), composed and encoded in HBM. `noise_blend_frames` is the one-shot form: every frame of a short
run as one host array.
"""

import os
from pathlib import Path
from typing import Callable, Dict, Iterator, List, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from gance_amd import projection_file_blend
from gance_amd.data_into_network_visualization import visualization_inputs
from gance_amd.data_into_network_visualization.visualization_common import DataLabel, ResultLayers
from gance_amd.debug_video.compose import DebugSources, DebugVideo, panel_layout
from gance_amd.network_interface.network_functions import MultiNetwork
from gance_amd.projection_file_blend import DEFAULT_STREAM_BATCH, shard_synthesize_gather
from gance_amd.vector_sources import music

# the labels alpha_blend_vectors_max_rms_power_audio gives its index layers (visualization_inputs.py:146-164 in the reference)
INDEX_LABEL = "Savgol Smoothing Filter (window={}, polyorder={})".format(*visualization_inputs.NOISE_INDEX_SAVGOL)


def noise_blend_frames(  # pylint: disable=too-many-arguments
    wav: List[str],
    network_paths: List[Path],
    frames_to_visualize: Optional[int],
    output_fps: float,
    output_side_length: int,
    alpha: float,
    fft_roll_enabled: bool,
    fft_amplitude_range: Tuple[int, int],
) -> Optional[np.ndarray]:
    """
    The synthesis pipeline of the reference's `noise_blend` command with its parameter names.
    :return: frames [N][S][S][3] uint8 on rank 0; None on other ranks when running distributed.
    """
    rank = dist.get_rank() if dist.is_initialized() else 0
    device = torch.device("cuda", torch.cuda.current_device())
    networks = MultiNetwork(network_paths=network_paths, load=True)
    try:
        vector_length = networks.expected_vector_length
        vectors = indices = None
        num_frames = 0
        if rank == 0:
            audio = music.read_wavs_scale_for_video(
                wavs=[Path(path) for path in wav], vector_length=vector_length, frames_per_second=output_fps
            ).wav_data
            blend = visualization_inputs.alpha_blend_vectors_max_rms_power_audio_device(
                alpha, fft_roll_enabled, fft_amplitude_range, audio, vector_length, len(networks.network_indices),
                device=device.index,
            )
            vectors, indices = blend.vectors, blend.network_indices
            blend.blend.close()
            if frames_to_visualize is not None:
                vectors, indices = vectors[:frames_to_visualize], indices[:frames_to_visualize]
            num_frames = int(vectors.shape[0])
        return shard_synthesize_gather(vectors, indices, num_frames, networks, output_side_length, device)
    finally:
        networks.unload()


def noise_debug_sources(  # pylint: disable=too-many-arguments
    spectrogram: np.ndarray,
    noise: torch.Tensor,
    vectors: torch.Tensor,
    indices: np.ndarray,
    index_smoothed: np.ndarray,
    frames_to_visualize: Optional[int],
    alpha: float,
    device: torch.device,
) -> DebugSources:
    """
    What the debug video of this command plots, as `vector_synthesis(enable_2d=True)` gets it from the reference's
    VisualizationInput (visualization_inputs.py:153-166): input A the spectrogram [N, L] float64 (host; uploaded here),
    input B the noise field [N, L] float32, one row per OUTPUT frame, combined the z vectors [N, L] themselves (both in
    HBM already); limits are each series' global min / max, over the whole song whatever `frames_to_visualize` cuts.
    No final images: this command has no projection file.
    """
    count = int(vectors.shape[0]) if frames_to_visualize is None else min(int(vectors.shape[0]), frames_to_visualize)
    return DebugSources(
        a_vectors=torch.from_numpy(np.ascontiguousarray(spectrogram[:count])).to(device),
        b_vectors=noise,
        limits={
            "a": (float(spectrogram.min()), float(spectrogram.max())),
            "b": (float(noise.min()), float(noise.max())),
            "combined": (float(vectors.min()), float(vectors.max())),
        },
        labels={"a": "Audio Spectrogram", "b": "Gaussian Smoothed Noise", "combined": f"Combined w/ Alpha Blending, a={alpha}"},
        network_indices=ResultLayers(
            result=DataLabel(np.asarray(indices[:count]).astype(int), f"{INDEX_LABEL} Scaled, Quantized"),
            layers=[DataLabel(index_smoothed[:count], INDEX_LABEL)],
        ),
    )


def _prepare_noise_inputs(  # pylint: disable=too-many-arguments,too-many-locals
    wav: List[str],
    networks: MultiNetwork,
    frames_to_visualize: Optional[int],
    output_fps: float,
    alpha: float,
    fft_roll_enabled: bool,
    fft_amplitude_range: Tuple[int, int],
    device: torch.device,
    want_debug: bool,
) -> projection_file_blend._BlendInputs:  # pylint: disable=protected-access
    """
    Rank 0: WAV -> per-frame z vectors [N, L] and network indices in HBM, the preparation of `noise_blend_frames`.
    :param want_debug: also keep what the debug video shows (visualization_inputs.py:153-166 in the reference): the blend
    stage `final` (input A), the noise field, one row per output frame (input B), and the index layer, as DebugSources
    without final images; the z vectors themselves are the combined series.
    """
    vector_length = networks.expected_vector_length
    audio = music.read_wavs_scale_for_video(
        wavs=[Path(path) for path in wav], vector_length=vector_length, frames_per_second=output_fps
    ).wav_data
    blend = visualization_inputs.alpha_blend_vectors_max_rms_power_audio_device(
        alpha, fft_roll_enabled, fft_amplitude_range, audio, vector_length, len(networks.network_indices),
        device=device.index, keep_stages=want_debug,
    )
    vectors, indices = blend.vectors, blend.network_indices
    debug = None
    if want_debug:
        try:  # (one read-back before the stream starts: the stages live in the blend's workspace, which is freed below)
            spectrogram = blend.blend.read_stage("final")
            index_smoothed = blend.blend.read_stage("index_smoothed")
        except Exception:
            blend.blend.close()
            raise
        debug = noise_debug_sources(spectrogram, blend.noise, vectors, indices.cpu().numpy(), index_smoothed, frames_to_visualize, alpha, device)
    blend.blend.close()
    if frames_to_visualize is not None:
        vectors, indices = vectors[:frames_to_visualize], indices[:frames_to_visualize]
    return projection_file_blend._BlendInputs(vectors, indices, int(vectors.shape[0]), None, None, 1, debug)  # pylint: disable=protected-access


def noise_blend_frame_chunks(  # pylint: disable=too-many-arguments
    wav: List[str],
    network_paths: List[Path],
    frames_to_visualize: Optional[int],
    output_fps: float,
    output_side_length: int,
    alpha: float,
    fft_roll_enabled: bool,
    fft_amplitude_range: Tuple[int, int],
    frames_per_call: int = DEFAULT_STREAM_BATCH,
    networks: Optional[MultiNetwork] = None,
    timings: Optional[Dict[str, object]] = None,
    drain: str = "rank0",
    on_total: Optional[Callable[[int], None]] = None,
    jpeg_quality: Optional[int] = None,
    *,
    debug: Optional[DebugVideo] = None,
    noise_seed: Optional[int] = None,
    jpeg_huffman: str = "standard",
) -> Iterator[Tuple[int, int, np.ndarray]]:
    """
    The frame stream of the command: a generator of (first_frame_index, total_frames, frames [n, S, S, 3] uint8, or
    EncodedFrames with `jpeg_quality`) in frame order. It IS the stream of
    projection_file_blend.projection_file_blend_frame_chunks, fed with z vectors [N, L] instead of latent matrices: the
    same chunks, windows by network, rings, encode and debug composer, the same keywords with the same meaning, and the
    same life time of a yielded chunk (a view of a ring slot: consume or copy it before advancing the generator twice
    more). Nothing ever holds more than the stream's chunks. Collective under `torch.distributed`.
    :param debug: a DebugVideo: rank 0 also composes the debug frames (hero frame, synthesis inputs: two square panels) of
    every chunk in HBM and hands them to `debug.on_encoded`; `timings["debug_frames_held_max"]` is one chunk (nothing of
    this video waits for a window).
    :param noise_seed: None (default): fresh noise planes per engine call, as upstream's randomize_noise=True draws them.
    An int s: frame k of the run reads the planes of (s, layer, k), k its GLOBAL frame number, however the run is cut into
    calls, windows, networks and ranks -- the frames of a trained network are then a function of the arguments alone (at
    random init every noise strength is zero and the planes are never read).
    :raises ValueError: as the projection stream, for the same mistakes, before anything is loaded.
    """
    projection_file_blend._check_stream_arguments(drain, None, jpeg_quality, output_side_length, debug, jpeg_huffman)  # pylint: disable=protected-access

    def prepare(resident: MultiNetwork, device: torch.device):
        return _prepare_noise_inputs(
            wav, resident, frames_to_visualize, output_fps, alpha, fft_roll_enabled, fft_amplitude_range, device, want_debug=debug is not None
        )

    yield from projection_file_blend._frame_stream(  # pylint: disable=protected-access
        prepare, network_paths, output_side_length, frames_per_call, None, networks, timings, drain, on_total, jpeg_quality, debug,
        noise_seed=noise_seed, jpeg_huffman=jpeg_huffman,
    )


def noise_blend_api(  # pylint: disable=too-many-arguments,too-many-locals
    wav: List[str],
    output_path: Optional[str],
    network_paths: List[Path],
    frames_to_visualize: Optional[int],
    output_fps: float,
    output_side_length: int,
    debug_path: Optional[str],
    debug_window: Optional[int],
    debug_side_length: Optional[int],
    alpha: float,
    fft_roll_enabled: bool,
    fft_amplitude_range: Tuple[int, int],
    drain: Optional[str] = None,
    *,
    output_format: str = "npy",
    jpeg_quality: int = 90,
    noise_seed: Optional[int] = None,
    jpeg_huffman: str = "standard",
) -> None:
    """
    Same parameter list as the reference command (music_into_networks.py:285-401). Frames are written to `output_path`
    chunk by chunk: `output_format="npy"` (the default) a memory-mapped `.npy` uint8 array [N][S][S][3] (`.npy` appended
    if it is missing; under drain="per-rank" every rank writes its own pieces), "avi" a Motion-JPEG OpenDML AVI with the
    WAVs as its audio stream, encoded in HBM at `jpeg_quality` (raw frames never reach the host). With `debug_path` the
    debug video is written there as a second AVI with the song: per frame the hero frame scaled to `debug_side_length`
    beside the synthesis-inputs plot (windows of `debug_window` frames, a fifth of the run if None). The AVI and the debug
    video force drain="rank0". `drain`, `output_format`, `jpeg_quality`, `jpeg_huffman` mean what they mean in
    projection_file_blend_api; `noise_seed`: see noise_blend_frame_chunks.
    :raises ValueError: before any device is touched, with the messages of projection_file_blend_api: an unknown
    output_format or jpeg_huffman; "avi" with a side that is not a multiple of 16, a jpeg_quality outside 1..100 or a frame rate AVI cannot
    hold; `debug_path` without a `debug_side_length` that is a multiple of 16 in [16, 4096].
    """
    encode = projection_file_blend.check_output_arguments(output_format, output_side_length, jpeg_quality, output_fps, jpeg_huffman)
    drain = drain or os.environ.get("GANCE_STREAM_DRAIN", "rank0")
    debug_side = projection_file_blend.check_debug_arguments(debug_path, debug_side_length, debug_window, False, jpeg_quality, output_fps)
    if encode or debug_path is not None:
        drain = "rank0"
    debug_panels = panel_layout(final_images=False, overlay=False, mask=False).panel_count

    def chunks_of(on_total, quality, debug):
        return noise_blend_frame_chunks(
            wav, network_paths, frames_to_visualize, output_fps, output_side_length, alpha, fft_roll_enabled, fft_amplitude_range,
            drain=drain, on_total=on_total, jpeg_quality=quality, debug=debug, noise_seed=noise_seed, jpeg_huffman=jpeg_huffman,
        )

    projection_file_blend.write_frame_stream(
        chunks_of, wav, output_path, output_fps, output_side_length, debug_path, debug_side, debug_window, debug_panels, drain, encode,
        int(jpeg_quality), jpeg_huffman,
    )
