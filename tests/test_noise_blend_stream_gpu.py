"""
GPU tests of the noise-blend command as a product: `noise_blend_frame_chunks` (the projection command's frame stream fed
with z vectors) against the one-shot `noise_blend_frames`, the noise-seed rule (frame k reads the planes of (seed, layer,
k), k its global number, however the run is cut), the Motion-JPEG AVI with the song, and the two-panel debug video.
Random-init and stress networks of gance_amd/stylegan2/spec.py at 32^2 / 64^2 and a synthetic WAV.

The kernel form of an engine call is a function of its batch (1 LSB on a few pixels between calls of 8 and of 16 frames,
see tests/test_blend_api_gpu.py and tests/test_debug_video_gpu.py), so wherever two runs are compared bit for bit both
issue their ENGINE calls with the same number of frames (`engine_calls_of`): chunking, windows, rings, encoder pieces and
the noise ids still run at the different frames per call the cases name.
"""

import io
import struct
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import pytest
import torch
from PIL import Image
from scipy.io import wavfile

import debug_video_ref as ref
from gance_amd import network_file, noise_blend, projection_file_blend, synthetic, torch_ops  # noqa: F401
from gance_amd.data_into_network_visualization import visualization_inputs
from gance_amd.debug_video import compose
from gance_amd.network_interface.network_functions import LoadedNetwork
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.vector_sources import music

pytestmark = pytest.mark.gpu

L, FPS = 512, 30.0
BLEND = dict(alpha=0.25, fft_roll_enabled=True, fft_amplitude_range=(-5, 5))


def write_wav(tmp_path: Path, num_frames: int, seed: int = 61) -> str:
    """A float32 WAV at L * fps Hz: FPS mode then gives one vector per output frame, `num_frames` of them."""
    path = tmp_path / "audio.wav"
    wavfile.write(str(path), int(L * FPS), synthetic.synthetic_audio(num_frames, L, seed=seed, frames_per_second=FPS))
    return str(path)


def write_networks(tmp_path: Path, count: int, side: int, stress: bool = False) -> List[Path]:
    paths = []
    for seed in range(count):
        paths.append(tmp_path / f"net_{seed}.pkl")
        if stress:  # (non-zero noise strengths: the planes are read)
            network_file.save_network(paths[-1], side, sg2_spec.make_stress_variables(side, seed=40 + seed))
        else:
            network_file.write_random_network(paths[-1], side, seed=30 + seed)
    return paths


def engine_calls_of(monkeypatch, frames: int) -> List[np.ndarray]:
    """Every engine call of the stream and of the one-shot form takes `frames` frames; returns the list the calls' ids land in."""
    original = projection_file_blend.synthesize_device_frames_network_major
    seen: List[np.ndarray] = []

    def pinned(dlatents, network_indices, networks, output_side_length=None, batch=None, out=None, **noise):  # pylint: disable=unused-argument
        return original(dlatents, network_indices, networks, output_side_length, frames, out=out, **noise)

    real_seeded = projection_file_blend._seeded_noise  # pylint: disable=protected-access

    def recording(engine, seed, ids, device, stream):
        seen.append(np.array(ids))
        return real_seeded(engine, seed, ids, device, stream)

    monkeypatch.setattr(projection_file_blend, "synthesize_device_frames_network_major", pinned)
    monkeypatch.setattr(projection_file_blend, "_seeded_noise", recording)
    return seen


def collect(chunks, frames_per_call: int, world_size: int = 1) -> np.ndarray:
    """The concatenated chunks of a stream (copied: a chunk is a view of a ring slot), with the stream's own bounds checked."""
    out: Optional[np.ndarray] = None
    expected_first = 0
    for first, total, frames in chunks:
        assert first == expected_first and 0 < len(frames) <= world_size * frames_per_call  # in order, never more than a chunk
        if out is None:
            out = np.zeros((total, *frames.shape[1:]), dtype=np.uint8)
        out[first : first + len(frames)] = frames
        expected_first += len(frames)
    assert out is not None and expected_first == len(out)
    return out


# ---- 1. the stream against the one-shot function ------------------------------------------------------------------------
@pytest.mark.parametrize("out_side", [64, 48])  # 48: the 64^2 frames go through the bicubic resize
@pytest.mark.parametrize("frames_to_visualize", [20, None])
@pytest.mark.parametrize("num_networks", [1, 3])
def test_stream_equals_the_one_shot_function(tmp_path: Path, monkeypatch, num_networks: int, frames_to_visualize, out_side: int) -> None:
    """Fails on the parent commit: noise_blend has no frame stream."""
    num_frames = 40
    engine_calls_of(monkeypatch, 8)
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, num_networks, 64)
    arguments = ([wav], network_paths, frames_to_visualize, FPS, out_side, BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"])
    want = noise_blend.noise_blend_frames(*arguments)
    assert want.shape == (frames_to_visualize or num_frames, out_side, out_side, 3)
    for frames_per_call in (8, 16):
        timings: Dict[str, object] = {}
        got = collect(noise_blend.noise_blend_frame_chunks(*arguments, frames_per_call=frames_per_call, timings=timings), frames_per_call)
        print(f"{num_networks} networks, {frames_per_call} per call, {frames_to_visualize}, side {out_side}: {int((got != want).sum())} bytes differ")
        assert np.array_equal(got, want)
        assert timings["frames"] == len(want) and timings["bytes_to_host"] == want.size


# ---- 2. the noise-seed rule ---------------------------------------------------------------------------------------------
def blended_vectors(wav: str, num_networks: int):
    """The z vectors and network indices the command prepares for this WAV (host copies)."""
    audio = music.read_wavs_scale_for_video(wavs=[Path(wav)], vector_length=L, frames_per_second=FPS).wav_data
    blend = visualization_inputs.alpha_blend_vectors_max_rms_power_audio_device(
        BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"], audio, L, num_networks, device=torch.cuda.current_device()
    )
    try:
        return blend.vectors.cpu().numpy(), blend.network_indices.cpu().numpy()
    finally:
        blend.blend.close()


def seeded_frames(wav: str, network_paths: List[Path], frames_to_visualize, frames_per_call: int, seed: Optional[int]) -> np.ndarray:
    return collect(
        noise_blend.noise_blend_frame_chunks(
            [wav], network_paths, frames_to_visualize, FPS, 32, BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"],
            frames_per_call=frames_per_call, noise_seed=seed,
        ),
        frames_per_call,
    )


def test_noise_seed_rule_with_one_network(tmp_path: Path, monkeypatch) -> None:
    """Engine calls of 4 frames in every run; the stream cuts the 32 frames into 8 chunks of 4 or 2 of 16."""
    num_frames, seed = 32, 20261017
    seen = engine_calls_of(monkeypatch, 4)
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 1, 32, stress=True)
    by_four = seeded_frames(wav, network_paths, None, 4, seed)
    ids_by_four = [ids.tolist() for ids in seen]
    del seen[:]
    by_sixteen = seeded_frames(wav, network_paths, None, 16, seed)
    assert ids_by_four == [ids.tolist() for ids in seen] == [list(range(start, start + 4)) for start in range(0, num_frames, 4)]  # GLOBAL numbers
    print("4 against 16 per call:", int((by_four != by_sixteen).sum()), "bytes differ")
    assert np.array_equal(by_four, by_sixteen)
    z, _indices = blended_vectors(wav, 1)
    network = LoadedNetwork(network_paths[0], max_batch=4)
    try:
        want = network.create_images_vector(z, noise_seed=seed)
        other = network.create_images_vector(z, noise_seed=seed + 1)
    finally:
        network.stop()
    print("against create_images_vector:", int((by_four != want).sum()), "bytes differ;", int((want != other).sum()), "between two seeds")
    assert (want != other).any(axis=(1, 2, 3)).all(), "the network's noise strengths are not zero: another seed must change every frame"
    assert np.array_equal(by_four, want)
    # without a seed: fresh planes per engine call, as before
    assert not np.array_equal(seeded_frames(wav, network_paths, None, 16, None), seeded_frames(wav, network_paths, None, 16, None))


def test_noise_seed_rule_with_two_networks(tmp_path: Path, monkeypatch) -> None:
    """
    Two stress networks switched by the RMS index. (i) Engine calls of ONE frame, windows of 2 pieces: the run is cut into
    windows, pieces and networks differently at 4 and at 16 frames per call, and every call has the same kernel forms.
    (ii) Engine calls of TWO frames over a run in which both networks have an even number of frames (so that no call is a
    single frame): calls that pair frames across a switch of the index are not contiguous and take the id tensor.
    """
    num_frames, seed = 46, 77
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 2, 32, stress=True)
    z, indices = blended_vectors(wav, 2)
    assert len(z) == num_frames
    print("network indices:", indices.tolist())
    assert set(indices.tolist()) == {0, 1}, "the index sequence must use both networks"
    # the longest run in which both networks have an even count of frames
    visualized = next(n for n in range(num_frames, 1, -1) if set(indices[:n].tolist()) == {0, 1} and all(int((indices[:n] == k).sum()) % 2 == 0 for k in (0, 1)))
    assert visualized >= 24
    members = [np.nonzero(indices[:visualized] == k)[0] for k in (0, 1)]
    pairs = [own[start : start + 2] for own in members for start in range(0, len(own), 2)]
    assert any(pair[1] != pair[0] + 1 for pair in pairs), "at least one engine call must be non-contiguous"

    def reference(count: int, max_batch: int) -> np.ndarray:
        """Frame k from its own network's create_images_vector over ALL z vectors: the planes of (seed, k)."""
        want = None
        for k, path in enumerate(network_paths):
            network = LoadedNetwork(path, max_batch=max_batch)
            try:
                images = network.create_images_vector(z[:count], noise_seed=seed)
            finally:
                network.stop()
            want = np.zeros_like(images) if want is None else want
            want[indices[:count] == k] = images[indices[:count] == k]
        return want

    # (i)
    with monkeypatch.context() as patch:
        seen = engine_calls_of(patch, 1)
        patch.setattr(projection_file_blend, "STREAM_WINDOW_PIECES_PER_NETWORK", 1)
        by_four = seeded_frames(wav, network_paths, None, 4, seed)
        calls_by_four = len(seen)
        by_sixteen = seeded_frames(wav, network_paths, None, 16, seed)
        assert calls_by_four == num_frames and len(seen) == 2 * num_frames
    print("(i) 4 against 16 per call:", int((by_four != by_sixteen).sum()), "bytes differ")
    assert np.array_equal(by_four, by_sixteen)
    want = reference(num_frames, 1)
    print("(i) against create_images_vector:", int((by_four != want).sum()), "bytes differ")
    assert np.array_equal(by_four, want)

    # (ii) (windows of 16 pieces: the whole run is one window at 4 frames per call too, so every network's frames pair up)
    seen = engine_calls_of(monkeypatch, 2)
    monkeypatch.setattr(projection_file_blend, "STREAM_WINDOW_PIECES_PER_NETWORK", 8)
    by_four = seeded_frames(wav, network_paths, visualized, 4, seed)
    scattered = [ids for ids in seen if len(ids) == 2 and ids[1] != ids[0] + 1]
    assert all(len(ids) == 2 for ids in seen) and scattered, "the d_sample_ids branch must run"
    print(f"(ii) {visualized} frames, {len(seen)} engine calls, {len(scattered)} of them non-contiguous, e.g. {scattered[0].tolist()}")
    by_sixteen = seeded_frames(wav, network_paths, visualized, 16, seed)
    print("(ii) 4 against 16 per call:", int((by_four != by_sixteen).sum()), "bytes differ")
    assert np.array_equal(by_four, by_sixteen)
    want = reference(visualized, 2)
    print("(ii) against create_images_vector:", int((by_four != want).sum()), "bytes differ")
    assert np.array_equal(by_four, want)


# ---- 3. the AVI ------------------------------------------------------------------------------------------------------------
def avi_streams(path: Path):
    """(JPEG files in order, audio bytes, (width, height) of avih, (scale, rate, length) of the video strh) of an OpenDML AVI."""
    blob = path.read_bytes()
    at = blob.index(b"indx")
    streams = {}
    while at >= 0:
        data_at = at + 8
        count, chunk_id = struct.unpack_from("<I4s", blob, data_at + 4)
        chunks = []
        for i in range(count):
            ix_at = struct.unpack_from("<Q", blob, data_at + 24 + 16 * i)[0]
            entries, base = struct.unpack_from("<I", blob, ix_at + 12)[0], struct.unpack_from("<Q", blob, ix_at + 20)[0]
            for j in range(entries):
                offset, size = struct.unpack_from("<II", blob, ix_at + 32 + 8 * j)
                chunks.append(blob[base + offset : base + offset + size])
        streams[chunk_id] = chunks
        at = blob.find(b"indx", data_at, blob.index(b"movi"))
    size = struct.unpack_from("<II", blob, blob.index(b"avih") + 8 + 32)
    strh = blob.index(b"strh") + 8
    assert blob[strh : strh + 4] == b"vids"
    scale, rate, _start, length = struct.unpack_from("<IIII", blob, strh + 20)
    return streams[b"00dc"], b"".join(streams.get(b"01wb", [])), size, (scale, rate, length)


def api_arguments(wav: str, network_paths: List[Path], output_path, side: int, debug_path=None, debug_window=None, debug_side=None, frames_to_visualize=None):
    """Positional arguments of noise_blend_api in the reference's order."""
    return [
        [wav], output_path, network_paths, frames_to_visualize, FPS, side, debug_path, debug_window, debug_side, BLEND["alpha"],
        BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"],
    ]


def test_avi_holds_the_encoders_bytes_and_the_song(tmp_path: Path) -> None:
    num_frames, side, quality = 36, 48, 85
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 2, 64)
    raw_path, avi_path = tmp_path / "frames", tmp_path / "video.avi"
    noise_blend.noise_blend_api(*api_arguments(wav, network_paths, str(raw_path), side))
    frames = np.load(str(raw_path) + ".npy")
    assert frames.shape == (num_frames, side, side, 3) and frames.dtype == np.uint8
    noise_blend.noise_blend_api(*api_arguments(wav, network_paths, str(avi_path), side), output_format="avi", jpeg_quality=quality)
    files, audio, size, (scale, rate, length) = avi_streams(avi_path)
    assert len(files) == num_frames == length and size == (side, side)
    assert rate / scale == FPS
    assert audio == wavfile.read(wav)[1].tobytes()  # the WAV's samples
    data, offsets = torch.ops.gance.jpeg_encode(torch.from_numpy(frames).cuda(), quality)
    host_offsets, blob = offsets.cpu().numpy(), data.cpu().numpy().tobytes()
    for index, written in enumerate(files):
        assert written == blob[host_offsets[index] : host_offsets[index + 1]], index  # (the encoder's bytes do not depend on the batch)
        decoded = Image.open(io.BytesIO(written))
        assert decoded.size == (side, side) and decoded.mode == "RGB"
    # the per-rank drain of the raw form writes the same file
    per_rank_path = tmp_path / "per_rank.npy"
    noise_blend.noise_blend_api(*api_arguments(wav, network_paths, str(per_rank_path), side), drain="per-rank")
    assert np.array_equal(np.load(per_rank_path), frames)


# ---- 4. the debug video ----------------------------------------------------------------------------------------------------
def debug_run(wav: str, network_paths: List[Path], side: int, debug_side: int, window, frames_per_call: int):
    """(composed debug frames [N, S, 2 S, 3], the frames the same run yields) through DebugVideo.on_composed."""
    composed: Dict[int, np.ndarray] = {}
    encoded: List[int] = []

    def on_composed(first: int, frames: torch.Tensor) -> None:
        for i, frame in enumerate(frames.cpu().numpy()):
            composed[first + i] = frame

    def on_encoded(first: int, chunk) -> None:
        assert chunk.side == debug_side and chunk.width == 2 * debug_side
        encoded.extend(range(first, first + len(chunk)))

    debug = compose.DebugVideo(debug_side, window, on_encoded, on_composed, jpeg_quality=80)
    timings: Dict[str, object] = {}
    output = collect(
        noise_blend.noise_blend_frame_chunks(
            [wav], network_paths, None, FPS, side, BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"],
            frames_per_call=frames_per_call, debug=debug, timings=timings,
        ),
        frames_per_call,
    )
    assert sorted(composed) == encoded == list(range(len(output)))  # every frame, in frame order
    assert timings["debug_frames_held_max"] <= frames_per_call  # (no overlay panel: nothing of this video waits for a window)
    return np.stack([composed[i] for i in range(len(output))]), output


def test_debug_video_panels(tmp_path: Path, monkeypatch) -> None:
    num_frames, side, debug_side, window = 40, 64, 96, 12
    engine_calls_of(monkeypatch, 8)
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 2, 64)
    raw, output = debug_run(wav, network_paths, side, debug_side, window, 8)
    assert raw.shape == (num_frames, debug_side, 2 * debug_side, 3)  # the frame width is 2 S
    # the left panel: the hero frame scaled to the debug side
    assert np.array_equal(raw[:, :, :debug_side], torch.ops.gance.resize_bicubic(torch.from_numpy(output).cuda(), debug_side).cpu().numpy())

    # the right panel: the restated rule on the panel's own chrome and tables, bound to the series the command plots
    audio = music.read_wavs_scale_for_video(wavs=[Path(wav)], vector_length=L, frames_per_second=FPS).wav_data
    blend = visualization_inputs.alpha_blend_vectors_max_rms_power_audio_device(
        BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"], audio, L, 2, device=torch.cuda.current_device(), keep_stages=True
    )
    try:
        spectrogram, index_smoothed = blend.blend.read_stage("final"), blend.blend.read_stage("index_smoothed")
        sources = noise_blend.noise_debug_sources(
            spectrogram, blend.noise, blend.vectors, blend.network_indices.cpu().numpy(), index_smoothed, None, BLEND["alpha"], torch.device("cuda")
        )
        panel = compose.synthesis_panel_of(debug_side, window, 1, sources, blend.vectors)
        series = {"a": spectrogram, "b": blend.noise.cpu().numpy(), "combined": blend.vectors.cpu().numpy(), **panel.host_series()}
    finally:
        blend.blend.close()
    assert series["b"].shape == series["combined"].shape == (num_frames, L) and series["a"].dtype == np.float64
    assert panel.combined_stride == L and panel.frame_multiplier == 1 and panel.width == window
    for window_index in range(-(-num_frames // window)):
        table = panel.window(window_index)
        axes = [dict(x=a.x, y=a.y, width=a.width, height=a.height, x_limits=a.x_limits, y_limits=a.y_limits) for a in table.axes]
        marks = []
        for spec in table.marks:
            mark = dict(
                kind=spec.kind, axis=spec.axis, count=spec.count, frame_stride=spec.frame_stride, frame_divisor=spec.frame_divisor, size=spec.size,
                rgba=(*spec.colour, spec.alpha), dash=spec.dash, flag_mask=spec.flag_mask, flag_value=spec.flag_value, x_start=spec.x_start,
            )
            if spec.series is not None:
                mark["data"] = np.asarray(series[spec.series]).reshape(-1)[spec.offset :]
            marks.append(mark)
        numbers = range(table.first_frame, table.first_frame + table.num_frames)
        frames = [dict(number=n, cursor=panel.cursor(n), flags=0) for n in numbers]
        want = ref.draw(table.chrome(debug_side), axes, marks, frames)
        got = raw[table.first_frame : table.first_frame + table.num_frames, :, debug_side:]
        print(f"window {window_index}: {int((got != want).any(axis=-1).sum())} pixels differ")
        assert np.array_equal(got, want), window_index
    plot = raw[:, :, debug_side:]
    assert not np.array_equal(plot[0], plot[1]) and (plot[0] != plot[window]).any()  # the cursor moves, the windows change

    # 8 and 16 frames per call over windows of 12: window and chunk borders fall differently
    by_sixteen, output_by_sixteen = debug_run(wav, network_paths, side, debug_side, window, 16)
    print("8 against 16 per call:", int((raw != by_sixteen).sum()), "bytes differ")
    assert np.array_equal(output, output_by_sixteen) and np.array_equal(raw, by_sixteen)


def test_debug_video_file(tmp_path: Path) -> None:
    num_frames, side, debug_side = 24, 64, 64
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 1, 64)
    plain, with_debug, debug_path = tmp_path / "plain", tmp_path / "with_debug", tmp_path / "debug.avi"
    noise_blend.noise_blend_api(*api_arguments(wav, network_paths, str(plain), side))
    noise_blend.noise_blend_api(*api_arguments(wav, network_paths, str(with_debug), side, str(debug_path), None, debug_side), jpeg_quality=85)
    assert Path(str(plain) + ".npy").read_bytes() == Path(str(with_debug) + ".npy").read_bytes()  # the debug video changes no frame
    files, audio, size, (scale, rate, length) = avi_streams(debug_path)
    assert size == (2 * debug_side, debug_side) and len(files) == num_frames == length and rate / scale == FPS
    assert audio == wavfile.read(wav)[1].tobytes()  # written with the song
    # the file holds the encoder's bytes of the composed frames of the same run (the API's frames per call, its window)
    raw, output = debug_run(wav, network_paths, side, debug_side, None, projection_file_blend.DEFAULT_STREAM_BATCH)
    assert np.array_equal(output, np.load(str(plain) + ".npy")) and np.array_equal(raw[:, :, :debug_side], output)  # 64 -> 64: no resize
    data, offsets = torch.ops.gance.jpeg_encode_rect(torch.from_numpy(raw).cuda(), 85)
    host_offsets, blob = offsets.cpu().numpy(), data.cpu().numpy().tobytes()
    for index, written in enumerate(files):
        assert written == blob[host_offsets[index] : host_offsets[index + 1]], index
        assert Image.open(io.BytesIO(written)).size == (2 * debug_side, debug_side)


# ---- 5. once through RCCL ----------------------------------------------------------------------------------------------
def test_noise_stream_once_through_rccl_with_one_rank(tmp_path: Path, monkeypatch) -> None:
    """
    The one-rank rehearsal of tests/test_full_size_stream_gpu.py for this command: process group "nccl" of one rank,
    GANCE_FORCE_COLLECTIVES=1 -> the z vectors [N, L] and the indices go through `scatter_for_stream`, every chunk through
    an asynchronous gather, the noise ids are the rank's `stream_order`. Frames must equal the short-cut path's, both drains.
    """
    import datetime  # pylint: disable=import-outside-toplevel

    import torch.distributed as dist  # pylint: disable=import-outside-toplevel

    from gance_amd import frame_sharding  # pylint: disable=import-outside-toplevel

    num_frames, seed = 24, 5
    engine_calls_of(monkeypatch, 4)
    wav, network_paths = write_wav(tmp_path, num_frames), write_networks(tmp_path, 1, 32, stress=True)
    short_cut = seeded_frames(wav, network_paths, None, 8, seed)
    assert not dist.is_initialized()
    store = dist.FileStore(str(tmp_path / "rccl_store"), 1)
    monkeypatch.setenv("GANCE_FORCE_COLLECTIVES", "1")
    device = torch.device("cuda", torch.cuda.current_device())
    dist.init_process_group("nccl", store=store, rank=0, world_size=1, device_id=device, timeout=datetime.timedelta(seconds=120))
    calls = {"gather": 0, "scatter": 0}
    real_gather, real_scatter = dist.gather, dist.scatter

    def counting_gather(tensor, *args, **kwargs):
        calls["gather"] += 1
        return real_gather(tensor, *args, **kwargs)

    def counting_scatter(tensor, *args, **kwargs):
        assert tensor.is_cuda
        calls["scatter"] += 1
        return real_scatter(tensor, *args, **kwargs)

    monkeypatch.setattr(dist, "gather", counting_gather)
    monkeypatch.setattr(dist, "scatter", counting_scatter)
    try:
        assert frame_sharding.collectives_forced()
        through_rccl = seeded_frames(wav, network_paths, None, 8, seed)
        assert calls == {"gather": 3, "scatter": 2}, calls  # one gather per chunk; z vectors + indices scattered
        per_rank = collect(
            noise_blend.noise_blend_frame_chunks(
                [wav], network_paths, None, FPS, 32, BLEND["alpha"], BLEND["fft_roll_enabled"], BLEND["fft_amplitude_range"],
                frames_per_call=8, noise_seed=seed, drain="per-rank",
            ),
            8,
        )
        assert calls["gather"] == 3  # (no gather with the per-rank drain)
    finally:
        frame_sharding._CONTROL_GROUP[0] = None  # pylint: disable=protected-access
        dist.destroy_process_group()
    assert np.array_equal(through_rccl, short_cut) and np.array_equal(per_rank, short_cut)
