"""
GPU tests of the JPEG encoder's "optimized" Huffman mode (torch.ops.gance.jpeg_encode_optimized, jpeg_optimal_huffman,
`jpeg_huffman="optimized"`): against the `jpeg_encode_rect` file of the same frame only the DHT segments and the
entropy-coded bytes may differ, the tables are libjpeg's optimal ones for the frame's own symbols
(tests/jpeg_huffman_ref.py, held against PIL in tests/test_jpeg_huffman.py), and the files are smaller.
"""

from pathlib import Path
from typing import List, Tuple

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import jpeg_huffman_ref as ref
from gance_amd import network_file, projection_file_blend, synthetic, torch_ops  # noqa: F401
from gance_amd.projection import projection_file_reader as pfr
from gance_amd.video import mjpeg_avi, video_common
from jpeg_decode_ref import ANNEX_K, decode_coefficients, gradients, noise, parse_header, pil_decode

pytestmark = pytest.mark.gpu

QUALITIES = (1, 50, 90, 100)


def split(data: torch.Tensor, offsets: torch.Tensor) -> List[bytes]:
    host = offsets.cpu().numpy()
    blob = data[: int(host[-1])].cpu().numpy().tobytes()
    return [blob[host[i] : host[i + 1]] for i in range(len(host) - 1)]


def half_noise(width: int, height: int, seed: int) -> np.ndarray:
    return (128 + (noise(width, height, seed).astype(np.int64) - 128) // 2).astype(np.uint8)


def mixed_batch(width: int, height: int) -> np.ndarray:
    """Noise, flat, gradients, half-amplitude noise: four frames with four different sets of tables."""
    return np.stack([noise(width, height, 11), ref.flat(width, height), gradients(width, height), half_noise(width, height, 12)])


def encode_both(frames: np.ndarray, quality: int) -> Tuple[List[bytes], List[bytes], np.ndarray]:
    """(standard files, optimised files, the optimised batch through torch.ops.gance.jpeg_decode)."""
    d_frames = torch.from_numpy(frames).cuda()
    standard = split(*torch.ops.gance.jpeg_encode_rect(d_frames, quality))
    data, offsets = torch.ops.gance.jpeg_encode_optimized(d_frames, quality)
    return standard, split(data, offsets), torch.ops.gance.jpeg_decode(data, offsets).cpu().numpy()


def assert_same_pixels_and_smaller(standard: List[bytes], optimized: List[bytes], decoded: np.ndarray, what: str) -> None:
    for index, (old, new) in enumerate(zip(standard, optimized)):
        want = pil_decode(new)
        assert np.array_equal(want, pil_decode(old)), (what, index)
        assert np.array_equal(decoded[index], want), (what, index)
        print(f"{what} frame {index}: {len(old)} -> {len(new)} bytes")
        assert len(new) < len(old), (what, index, len(new), len(old))


def assert_only_tables_and_scan_differ(old: bytes, new: bytes, what) -> None:
    (old_begin, old_end), (new_begin, new_end) = ref.dht_range(old), ref.dht_range(new)
    old_header, new_header = parse_header(old), parse_header(new)
    assert new[:new_begin] == old[:old_begin], what  # SOI, APP0, DQT x 2, SOF0
    assert new[new_end : new_header.scan_offset] == old[old_end : old_header.scan_offset], what  # DRI, SOS
    assert new[new_begin : new_begin + 2] == b"\xff\xc4" and new[new_end : new_end + 2] == b"\xff\xdd", what
    assert new[-2:] == b"\xff\xd9", what


@pytest.mark.parametrize("width_height", [(16, 16), (48, 32), (32, 48), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames(width_height) -> None:
    width, height = width_height
    frames = mixed_batch(width, height)
    for quality in QUALITIES:
        standard, optimized, decoded = encode_both(frames, quality)
        tables = []
        for index, (old, new) in enumerate(zip(standard, optimized)):
            what = (width, height, quality, index)
            assert_only_tables_and_scan_differ(old, new, what)
            header = parse_header(new)
            coefficients = decode_coefficients(new, header)
            assert np.array_equal(coefficients, decode_coefficients(old, parse_header(old))), what
            got = ref.dht_of(new)
            assert list(got) == list(ref.TABLE_ORDER), what  # DC0, AC0, DC1, AC1
            assert got == ref.tables_of_counts(ref.symbol_counts(coefficients, header.restart_interval)), what
            tables.append(got)
        # tables per frame, not per batch (at quality 1 two of the small frames can come down to the same symbols)
        assert any(tables[index] != tables[0] for index in range(1, 4)), (width, height, quality)
        assert_same_pixels_and_smaller(standard, optimized, decoded, f"{width}x{height} q{quality}")


def test_length_limit_in_a_real_frame() -> None:
    frames = ref.decaying_noise(384)[None]
    standard, optimized, decoded = encode_both(frames, 100)
    header = parse_header(optimized[0])
    counts = ref.symbol_counts(decode_coefficients(optimized[0], header), header.restart_interval)
    assert max(ref.merged_code_sizes(counts[1])) > 16  # the Annex K.3 step does real work on this frame
    assert ref.dht_of(optimized[0]) == ref.tables_of_counts(counts)
    assert np.array_equal(pil_decode(optimized[0]), pil_decode(standard[0]))
    assert np.array_equal(decoded[0], pil_decode(standard[0]))


@pytest.mark.parametrize("width_height", [(256, 256), (1040, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_larger_frames(width_height) -> None:
    width, height = width_height
    frames = mixed_batch(width, height)
    for quality in (50, 100):
        standard, optimized, decoded = encode_both(frames, quality)
        assert_same_pixels_and_smaller(standard, optimized, decoded, f"{width}x{height} q{quality}")


def test_bytes_do_not_depend_on_the_batch() -> None:
    makers = (noise, half_noise, ref.texture, lambda w, h, s: ((gradients(w, h).astype(np.int64) + 3 * s) % 256).astype(np.uint8))
    frames = np.stack([makers[index % 4](48, 48, 100 + index) for index in range(64)])
    assert len({frame.tobytes() for frame in frames}) == 64
    d_frames = torch.from_numpy(frames).cuda()
    in_batch = split(*torch.ops.gance.jpeg_encode_optimized(d_frames, 90))
    assert len(set(in_batch)) == 64
    alone = split(*torch.ops.gance.jpeg_encode_optimized(d_frames[63:64], 90))
    first_of_five = split(*torch.ops.gance.jpeg_encode_optimized(torch.flip(d_frames, (0,))[:5].contiguous(), 90))
    assert alone[0] == in_batch[63] and first_of_five[0] == in_batch[63]
    assert in_batch == split(*torch.ops.gance.jpeg_encode_optimized(d_frames, 90))  # and not on the run


def test_jpeg_optimal_huffman() -> None:
    rng = np.random.RandomState(21)
    single = [0] * 256
    single[0x31] = 7
    vectors = [ref.fibonacci_counts(depth) for depth in (17, 24, 32, 33)] + [[1000] * 256, single, [0] * 256]
    for symbols in (2, 3, 12, 40, 162, 256):  # random sparse counts: ties, large ranges, every table size
        for high in (2, 50, 1_000_000):
            counts = np.zeros(256, np.int64)
            counts[rng.choice(256, symbols, replace=False)] = rng.randint(1, high + 1, symbols)
            vectors.append(counts.tolist())
    counts = torch.tensor(vectors, dtype=torch.int32).cuda()
    bits, values, status = (tensor.cpu().numpy() for tensor in torch.ops.gance.jpeg_optimal_huffman(counts))
    assert bits.shape == (len(vectors), 16) and values.shape == (len(vectors), 256) and status.shape == (len(vectors),)
    for index, vector in enumerate(vectors):
        if not any(vector):
            assert status[index] == 2, index
            continue
        want = ref.optimal_table(vector)
        if want is None:
            assert status[index] == 1 and index == 3, index
            continue
        assert status[index] == 0, index
        assert bits[index].tolist() == want[0], index
        assert values[index, : len(want[1])].tolist() == want[1], index
        assert not values[index, len(want[1]) :].any(), index
    assert not bits[status != 0].any() and not values[status != 0].any()
    with pytest.raises(ValueError):
        torch.ops.gance.jpeg_optimal_huffman(counts[:, :255])


# ---- through a product ---------------------------------------------------------------------------------------------------
def blend_inputs(tmp_path: Path, num_projection: int, side: int = 64) -> dict:
    """tests/test_mjpeg_decode_gpu.py::blend_inputs restated: WAV + projection file + two random networks on disk."""
    L, fps_in, fps_out = 512, 15.0, 30.0
    num_frames = int(num_projection * fps_out / fps_in)
    audio = synthetic.synthetic_audio(num_frames, L, seed=61, frames_per_second=fps_out)
    wav_path = tmp_path / "audio.wav"
    wavfile.write(str(wav_path), int(L * fps_out), audio)
    latents = synthetic.synthetic_final_latents(num_projection, L, seed=62)
    projection_path = tmp_path / "projection.npz"
    pfr.write_projection_npz(projection_path, latents.reshape(18, num_projection, L).transpose(1, 0, 2), projection_fps=fps_in)
    network_paths = []
    for seed in range(2):
        path = tmp_path / f"net_{seed}.pkl"
        network_file.write_random_network(path, side, seed=seed)
        network_paths.append(path)
    return dict(
        wav=[str(wav_path)], network_paths=network_paths, frames_to_visualize=None, output_fps=fps_out, alpha=0.25,
        fft_roll_enabled=True, fft_amplitude_range=(-5, 5), projection_file_path=str(projection_path), blend_depth=12,
    )


def test_through_projection_file_blend(tmp_path: Path) -> None:
    inputs = blend_inputs(tmp_path, num_projection=6)
    paths = {}
    for mode in ("standard", "optimized"):
        paths[mode] = (tmp_path / f"{mode}.avi", tmp_path / f"{mode}_debug.avi")
        projection_file_blend.projection_file_blend_api(
            **inputs, output_path=str(paths[mode][0]), output_format="avi", jpeg_quality=85, output_side_length=64,
            debug_path=str(paths[mode][1]), debug_window=None, debug_side_length=64, complexity_change_rolling_sum_window=None,
            complexity_change_threshold=None, phash_distance=None, bbox_distance=None, track_length=None, jpeg_huffman=mode,
        )
    annex_k = {key: (list(table[0]), list(table[1])) for key, table in ANNEX_K.items()}
    for which in (0, 1):  # the video, its debug video
        standard, optimized = (video_common.frames_in_video(paths[mode][which]) for mode in ("standard", "optimized"))
        assert optimized.total_frame_count == standard.total_frame_count == 12
        for old, new in zip(standard.frames, optimized.frames):
            assert np.array_equal(np.asarray(old), np.asarray(new))
        sizes = [paths[mode][which].stat().st_size for mode in ("standard", "optimized")]
        print(f"{'debug video' if which else 'video'}: {sizes[0]} -> {sizes[1]} bytes")
        assert sizes[1] < sizes[0]
        for mode in ("standard", "optimized"):
            with mjpeg_avi.MjpegAviReader(paths[mode][which]) as reader:
                files = reader.read_frame_bytes(0, reader.frame_count)
            own_tables = [ref.dht_of(data) != annex_k for data in files]
            assert all(own_tables) if mode == "optimized" else not any(own_tables)
