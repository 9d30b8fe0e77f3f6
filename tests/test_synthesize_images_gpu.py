"""
GPU tests of the still products (gance_amd/synthesize_images.py): the files `synthesis_file_into_networks` and
`images_from_network` write, against the engine's own images and a one-vector-at-a-time replay of the reference's loop.
"""

import hashlib
import json
from pathlib import Path
from typing import Dict, List, Tuple

import numpy as np
import pytest

from gance_amd import network_file, synthesize_images
from gance_amd.hash_file import hash_file
from gance_amd.image_sources.still_image_common import read_image, write_image
from gance_amd.network_interface.network_functions import MultiNetwork
from gance_amd.stylegan2 import spec as sg2_spec
from gance_amd.synthesis_file import read_vector_in_file, write_synthesis_file
from gance_amd.vector_sources.primatives import gaussian_data

pytestmark = pytest.mark.gpu

SAMPLE = Path(__file__).resolve().parent / "golden" / "sample_synthesis_file.json"
RESOLUTION = 32
NOISE_SEED = 99  # the perturbed network's noise strengths are not zero: a seed makes its images repeatable
VERSION_2_KEYS = {"vector", "network_path", "network_hash", "image_path", "image_hash", "version"}


@pytest.fixture(scope="module")
def networks(tmp_path_factory) -> Tuple[Path, List[Path]]:
    """A directory with two random-init networks of different seeds, the second with every bias and noise term live."""
    directory = tmp_path_factory.mktemp("networks")
    paths = [directory / "a_plain.pkl", directory / "b_perturbed.pkl"]  # sorted: the plain one is index 0
    network_file.save_network(paths[0], RESOLUTION, sg2_spec.make_random_variables(RESOLUTION, seed=1))
    network_file.save_network(paths[1], RESOLUTION, sg2_spec.make_random_variables(RESOLUTION, seed=2, perturb=True))
    return directory, sorted(paths)


def check_pair(image_path: Path, network_path: Path, vector: np.ndarray, want_image: np.ndarray) -> None:
    """One .png / .json pair: the pixels, the two hashes, the key set and the stored vector."""
    assert np.array_equal(read_image(image_path), want_image), image_path.name
    with open(image_path.with_suffix(".json")) as file:
        described = json.load(file)
    assert set(described) == VERSION_2_KEYS and described["version"] == 2
    assert described["image_hash"] == hash_file(image_path) == hashlib.md5(image_path.read_bytes()).hexdigest()
    assert described["network_hash"] == hash_file(network_path)
    assert (described["image_path"], described["network_path"]) == (str(image_path), str(network_path))
    assert np.array_equal(read_vector_in_file(image_path.with_suffix(".json")), np.asarray(vector, dtype=np.float64))


def test_synthesis_file_into_networks(networks, tmp_path: Path) -> None:
    networks_directory, network_paths = networks
    rs = np.random.RandomState(5)
    sources = tmp_path / "sources"
    sources.mkdir()
    written = {"first": rs.randn(512).astype(np.float32), "second": rs.randn(512).astype(np.float32)}
    for name, vector in written.items():
        write_synthesis_file(sources / f"{name}.json", vector, Path("n.pkl"), "nh", Path("i.png"), "ih")
    output = tmp_path / "out"
    synthesize_images.synthesis_file_into_networks(
        networks_dir=str(networks_directory), network=None, synthesis_files_dir=str(sources), synthesis_file=[str(SAMPLE)],
        output_directory=str(output), noise_seed=NOISE_SEED,
    )
    vectors: Dict[Path, np.ndarray] = {sources / f"{name}.json": vector for name, vector in written.items()}
    vectors[SAMPLE] = read_vector_in_file(SAMPLE)
    assert sorted(path.name for path in output.iterdir()) == sorted(path.stem for path in vectors)
    with MultiNetwork(network_paths=network_paths) as multi_network:
        for source, vector in vectors.items():
            directory = output / source.stem
            names = {f"network_{path.name}_{hash_file(source)}{suffix}" for path in network_paths for suffix in (".png", ".json")}
            assert {path.name for path in directory.iterdir()} == names
            for index, network_path in enumerate(network_paths):
                want = multi_network.indexed_create_image_vector(index, vector, noise_seed=NOISE_SEED)
                check_pair(directory / f"network_{network_path.name}_{hash_file(source)}.png", network_path, vector, want)
        # the plain network's noise strengths are zero: its images are those of the call without a seed
        plain = multi_network.indexed_create_image_vector(0, vectors[SAMPLE])
        assert np.array_equal(read_image(output / SAMPLE.stem / f"network_{network_paths[0].name}_{hash_file(SAMPLE)}.png"), plain)


class GreenFinder:  # pylint: disable=too-few-public-methods
    """Stands in for the detector: one location when the green channel's mean is above a threshold. Gives up, instead of
    letting a pass run on, if it is asked more often than the test can need."""

    def __init__(self, threshold: float) -> None:
        self.threshold = threshold
        self.calls = 0

    def face_locations(self, image: np.ndarray) -> List[Tuple[int, int, int, int]]:
        self.calls += 1
        assert self.calls < 400, "the finder's threshold splits no network's images"
        return [(0, 0, 1, 1)] if float(image[..., 1].mean()) > self.threshold else []


def files_of(directory: Path) -> Dict[str, bytes]:
    return {str(path.relative_to(directory)): path.read_bytes() for path in sorted(directory.rglob("*")) if path.is_file()}


def test_images_from_network(networks, tmp_path: Path) -> None:
    networks_directory, network_paths = networks
    seed, num_faces, no_faces = 4321, 3, 2
    with MultiNetwork(network_paths=network_paths) as multi_network:
        probe_state = np.random.RandomState(17)
        probe = [gaussian_data(512, 1, random_state=probe_state) for _ in range(8)]
        greens = [
            float(multi_network.indexed_create_image_vector(index, vector, noise_seed=NOISE_SEED)[..., 1].mean())
            for index in range(len(network_paths)) for vector in probe
        ]
        threshold = float(np.median(greens))
        print("probe green means", np.round(greens, 2), "median", threshold)
        # the reference's loop, one vector at a time: what the batched runs must reproduce
        finder = GreenFinder(threshold)
        random_state = np.random.RandomState(seed)
        expected: Dict[str, Tuple[Path, np.ndarray, np.ndarray]] = {}
        drawn = 0
        for index, network_path in enumerate(network_paths):
            prefix = f"{network_path.stem}/{network_path.stem}_{hash_file(network_path)}"
            for kind, contains_face, wanted in [("face", True, num_faces), ("no_face", False, no_faces)]:
                count = 0
                while count < wanted:
                    vector = gaussian_data(vector_length=512, num_vectors=1, random_state=random_state)
                    drawn += 1
                    image = multi_network.indexed_create_image_vector(index, vector, noise_seed=NOISE_SEED)
                    if any(finder.face_locations(image)) == contains_face:
                        expected[f"{prefix}_{kind}_{count}.png"] = (network_path, vector, image)
                        count += 1
    print("candidates drawn", drawn, "for", len(expected), "images")
    outputs = []
    for frames_per_call in (1, 4):
        output = tmp_path / f"per_call_{frames_per_call}"
        synthesize_images.images_from_network(
            str(networks_directory), str(output), num_faces, no_faces, random_seed=seed, face_finder=GreenFinder(threshold),
            frames_per_call=frames_per_call, noise_seed=NOISE_SEED,
        )
        files = files_of(output)
        assert sorted(files) == sorted([name for name in expected] + [name[:-4] + ".json" for name in expected])
        for name, (network_path, vector, image) in expected.items():
            check_pair(output / name, network_path, vector, image)
        # the .json files name their own directory: compare the runs with that prefix taken out
        outputs.append({name: content.replace(str(output).encode(), b"") for name, content in files.items()})
    assert outputs[0] == outputs[1]

    with pytest.raises(NotImplementedError):
        synthesize_images.images_from_network(str(networks_directory), str(tmp_path / "none"), 1, 0)
    with pytest.raises(NotImplementedError):
        synthesize_images.images_from_network(str(networks_directory), str(tmp_path / "none"), 0, 1)
    unfiltered = tmp_path / "any"
    synthesize_images.images_from_network(str(networks_directory), str(unfiltered), 0, 0, random_seed=seed, num_images=5, frames_per_call=4)
    for network_path in network_paths:
        names = sorted(path.name for path in (unfiltered / network_path.stem).iterdir())
        stem = f"{network_path.stem}_{hash_file(network_path)}_any_"
        assert names == sorted(f"{stem}{i}{suffix}" for i in range(5) for suffix in (".png", ".json"))
    # the unfiltered images go through the same stream: the first network's are its first five vectors
    random_state = np.random.RandomState(seed)
    first = network_paths[0]
    for i in range(5):
        vector = gaussian_data(vector_length=512, num_vectors=1, random_state=random_state)
        stored = read_vector_in_file(unfiltered / first.stem / f"{first.stem}_{hash_file(first)}_any_{i}.json")
        assert np.array_equal(stored, vector.astype(np.float64))


def test_write_image_and_read_image(tmp_path: Path) -> None:
    import torch  # pylint: disable=import-outside-toplevel

    image = np.random.RandomState(2).randint(0, 256, (37, 53, 3)).astype(np.uint8)
    write_image(image, tmp_path / "host.png")
    write_image(torch.from_numpy(image).cuda(), tmp_path / "device.png")
    assert (tmp_path / "host.png").read_bytes() == (tmp_path / "device.png").read_bytes()
    assert np.array_equal(read_image(tmp_path / "host.png"), image)
    assert read_image(tmp_path / "host.png", mode="L").shape == (37, 53)
