"""
Development tooling: write a small, REAL HDF5 projection file WITH latent histories, with h5py, in the layout the
reference's writer produces (gance/projection/projector_file_writer.py:749-755 the `latents_histories` group with one
sub-group `latents_histories_<frame>` per projected frame, :871-877 one dataset `latents_histories_<frame>_step_<step>`
of shape (1, 18, 512) float32 per projection step; datasets gzip-9 + shuffle like every other, :814-834).

h5py is not installed in the interpreter the product runs on; run this with one that has it:

    python3.9 tests/dev/make_projection_history_fixture.py

Writes tests/golden/projection_histories.hdf5 (three projected frames with 11, 3 and 3 steps: step_10 has to sort after
step_2, and step 5 exists in frame 0 only) and tests/golden/projection_histories_expected.npz (the arrays that were
written). The last step of every history equals the frame's final latents; the images are 16 x 16 and blocky.
"""

from pathlib import Path

import h5py
import numpy as np

GOLDEN_DIR = Path(__file__).resolve().parent.parent / "golden"
COMPRESSION_LEVEL = 9
STEPS = (11, 3, 3)
NETWORK_MD5_HASH = "00112233445566778899aabbccddeeff"


def create_dataset(group, name: str, data: np.ndarray) -> None:
    group.create_dataset(
        f"/{group.name}/{name}", shape=data.shape, dtype=data.dtype, data=data, compression="gzip", compression_opts=COMPRESSION_LEVEL,
        shuffle=True,
    )


def blocky(rng: np.random.RandomState) -> np.ndarray:
    """16 x 16 x 3 uint8 of 4 x 4 blocks."""
    return np.repeat(np.repeat(rng.randint(0, 256, size=(4, 4, 3)).astype(np.uint8), 4, axis=0), 4, axis=1)


def attributes(frames: int, complete: bool) -> dict:
    return {
        "version_number": 2,
        "complete": complete,
        "original_target_path": "/videos/history clip.mp4",
        "original_width_height": (1920, 1080),
        "projection_width_height": (16, 16),
        "target_md5_hash": "0123456789abcdef0123456789abcdef",
        "original_network_path": "/networks/network-snapshot-000064.pkl",
        "network_md5_hash": NETWORK_MD5_HASH,
        "steps_in_projection": max(STEPS),
        "noises_shapes": np.nan,
        "latents_histories_enabled": True,
        "noises_histories_enabled": False,
        "images_histories_enabled": False,
        "original_fps": 30.0,
        "projection_fps": 7.5,
        "original_frame_count": 4 * frames,
        "projection_frame_count": frames,
    }


def main() -> None:
    rng = np.random.RandomState(417)
    frames = len(STEPS)
    # (values on a grid of 1 / 32: exact in float32, and the file stays small)
    finals = [np.round(rng.randn(512) * 32.0).astype(np.float32) / 32.0 for _ in range(frames)]
    starts = [np.round(rng.randn(512) * 96.0).astype(np.float32) / 32.0 for _ in range(frames)]
    histories = []
    for final, start, steps in zip(finals, starts, STEPS):
        weights = ((steps - 1 - np.arange(steps)) / (steps - 1)) ** 2  # 1 at step 0, 0 at the last step
        rows = [np.round((final + (start - final) * weight) * 32.0).astype(np.float32) / 32.0 for weight in weights]
        assert np.array_equal(rows[-1], final)
        histories.append(np.stack([np.tile(row[None, :], (18, 1)) for row in rows]))  # [steps, 18, 512]
    targets = [blocky(rng) for _ in range(frames)]
    final_images = [blocky(rng) for _ in range(frames)]
    path = GOLDEN_DIR / "projection_histories.hdf5"
    with h5py.File(name=str(path), mode="w") as f:
        f.attrs.update(attributes(frames, complete=False))
        groups = {name: f.create_group(name) for name in ("target_images", "final_latents", "final_images", "latents_histories")}
        for name in ("images_histories", "noises_histories"):
            f.create_group(name)
        for index in range(frames):
            create_dataset(groups["target_images"], f"target_images_{index}", targets[index])
            history_group = groups["latents_histories"].create_group(f"latents_histories_{index}")
            for step in range(STEPS[index]):
                create_dataset(history_group, f"latents_histories_{index}_step_{step}", histories[index][step][None])
            create_dataset(groups["final_latents"], f"final_latents_{index}", np.tile(finals[index][None, None, :], (1, 18, 1)))
            create_dataset(groups["final_images"], f"final_images_{index}", final_images[index])
            f.flush()
        f.attrs.update(attributes(frames, complete=True))
    expected = {f"history_{index}": histories[index] for index in range(frames)}
    expected.update(
        final_latents=np.stack([np.tile(final[None, :], (18, 1)) for final in finals]), target_images=np.stack(targets),
        final_images=np.stack(final_images),
    )
    np.savez_compressed(GOLDEN_DIR / "projection_histories_expected.npz", **expected)
    print(f"wrote {path.name} ({path.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
