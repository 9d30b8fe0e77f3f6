"""
Given some networks, synthesize stills with them (synthesize_images.py of the reference): the two commands as API
functions, the click CLI left out as for the other products.

* `synthesis_file_into_networks`: re-render the vectors of stored synthesis files through every network;
* `images_from_network`: random-z stills per network, filtered by a face / no-face test.

Both write a `.png` and, beside it, the JSON synthesis file that describes how it was made. The work is batched: up to
`max_batch` vectors are uploaded at once, their frames stay in HBM and are encoded there in one call
(image_sources/still_image_common.py), and only compressed bytes cross to the host, plus, in the filtered passes, the
frames the detector looks at. Each frame is still the image of `indexed_create_image_vector` for its vector, bit for
bit (LoadedNetwork.create_images_vector_device): the files, and a detector's verdicts, do not depend on the batching.
"""

from collections import deque
from pathlib import Path
from typing import Any, Deque, List, Optional

import numpy as np
import torch

from gance_amd.hash_file import hash_file
from gance_amd.image_sources.still_image_common import PNG, check_compression, write_images_device
from gance_amd.logger_common import LOGGER
from gance_amd.network_interface.network_functions import NETWORK_SUFFIX, MultiNetwork
from gance_amd.synthesis_file import SYNTHESIS_FILE_SUFFIX, read_vector_in_file, write_synthesis_file
from gance_amd.vector_sources.primatives import DEFAULT_RANDOM_SEED, gaussian_data
from gance_amd.vector_sources.vector_types import SingleVector

# candidates synthesised per engine call of `images_from_network`; the engine's max_batch caps it
DEFAULT_FRAMES_PER_CALL = 16


def all_paths(dir_of_paths: Optional[str], given_paths: Optional[List[str]], suffix: str) -> List[Path]:
    """
    Boil the two ways of naming files down to one list (synthesize_images.py:39-58): the files with `suffix` in a
    directory, then the paths given directly.
    """
    output_paths: List[Path] = []
    if dir_of_paths is not None:
        output_paths += list(Path(dir_of_paths).glob(f"*{suffix}"))
    if given_paths is not None:
        output_paths += [Path(path) for path in given_paths]
    return output_paths


def synthesis_file_into_networks(  # pylint: disable=too-many-locals
    networks_dir: Optional[str],
    network: Optional[List[str]],
    synthesis_files_dir: Optional[str],
    synthesis_file: Optional[List[str]],
    output_directory: str,
    noise_seed: Optional[int] = None,
    png_compression: str = "huffman",
) -> None:
    """
    For each input synthesis file, read the vector; write each vector to each network
    (synthesize_images.py:109-202). Images and their synthesis files go to one directory per input file, named after its
    stem, as `network_{network file name}_{md5 of the input synthesis file}.png` / `.json`. Networks outside, vectors
    inside; the vectors of one network are synthesised and encoded in batches of up to `max_batch`.
    :param noise_seed: not in the reference, whose images draw fresh noise each (None): with a seed every image is
        `indexed_create_image_vector(index, vector, noise_seed=noise_seed)`, repeatable.
    :param png_compression: not in the reference: still_image_common.COMPRESSIONS; "matches" writes smaller or equal files
        of the same pixels, and the JSON's image_hash is that file's.
    :raises ValueError: an unknown png_compression, before anything is read or written.
    """
    check_compression(png_compression)
    network_paths = all_paths(dir_of_paths=networks_dir, given_paths=network, suffix=NETWORK_SUFFIX)
    synthesis_file_paths = all_paths(dir_of_paths=synthesis_files_dir, given_paths=synthesis_file, suffix=SYNTHESIS_FILE_SUFFIX)
    if not network_paths or not synthesis_file_paths:
        LOGGER.info(f"No input! Found networks: {network_paths} Found Syn files: {synthesis_file_paths}")
        return None
    LOGGER.info(f"Found {len(network_paths)} networks and {len(synthesis_file_paths)} synthesis files.")

    top_level_output_directory = Path(output_directory)
    top_level_output_directory.mkdir(exist_ok=True)
    output_directories = [top_level_output_directory.joinpath(path.with_suffix("").name) for path in synthesis_file_paths]
    for directory in output_directories:
        directory.mkdir(exist_ok=True)
    synthesis_file_hashes = [hash_file(path) for path in synthesis_file_paths]
    vectors = [read_vector_in_file(path) for path in synthesis_file_paths]

    with MultiNetwork(network_paths=network_paths) as multi_network:
        if multi_network is None:
            LOGGER.error("Couldn't load network")
            return None
        for index, network_path in enumerate(network_paths):
            network_hash = hash_file(network_path)
            image_paths = [
                directory.joinpath(f"network_{network_path.name}_{synthesis_file_hash}.{PNG}")
                for synthesis_file_hash, directory in zip(synthesis_file_hashes, output_directories)
            ]
            for start in range(0, len(vectors), multi_network.max_batch):
                batch_paths = image_paths[start : start + multi_network.max_batch]
                batch_vectors = vectors[start : start + multi_network.max_batch]
                frames = multi_network.indexed_create_images_vector_device(index, np.stack(batch_vectors), noise_seed=noise_seed)
                image_hashes = write_images_device(frames, batch_paths, compression=png_compression)
                for image_path, image_hash, vector in zip(batch_paths, image_hashes, batch_vectors):
                    write_synthesis_file(
                        destination_path=image_path.with_suffix(SYNTHESIS_FILE_SUFFIX),
                        network_path=network_path,
                        network_hash=network_hash,
                        image_path=image_path,
                        image_hash=image_hash,
                        vector=vector,
                    )
    return None


class _Candidates:
    """
    The reference's vector sequence, batched: one `gaussian_data(vector_length, 1, random_state)` draw per candidate
    (synthesize_images.py:237-241) from the one RandomState that runs on across passes and networks. Vectors are drawn
    `frames_per_call` at a time; those drawn but not yet judged when a pass has its count wait in the queue for the next
    pass (of this or the next network), so the judged vectors are always a prefix of the stream with none skipped.
    """

    def __init__(self, vector_length: int, random_state: "np.random.RandomState", frames_per_call: int) -> None:
        self._vector_length = vector_length
        self._random_state = random_state
        self._frames_per_call = frames_per_call
        self._queue: Deque[SingleVector] = deque()

    def take(self, wanted: Optional[int] = None) -> List[SingleVector]:
        """The next frames_per_call vectors of the stream, or the next `wanted` if that is fewer."""
        count = self._frames_per_call if wanted is None else max(1, min(wanted, self._frames_per_call))
        while len(self._queue) < count:
            self._queue.append(SingleVector(gaussian_data(vector_length=self._vector_length, num_vectors=1, random_state=self._random_state)))
        return [self._queue.popleft() for _ in range(count)]

    def give_back(self, vectors: List[SingleVector]) -> None:
        """Unjudged vectors, in order, to the front of the queue."""
        self._queue.extendleft(reversed(vectors))


def _write_pass(  # pylint: disable=too-many-arguments,too-many-locals
    multi_network: MultiNetwork,
    index: int,
    candidates: _Candidates,
    wanted: int,
    kind: str,
    contains_face: Optional[bool],
    face_finder: Any,
    output_directory: Path,
    network_name: str,
    network_path: Path,
    network_hash: str,
    noise_seed: Optional[int],
    png_compression: str,
) -> None:
    """
    One pass of one network (create_images + write_images, synthesize_images.py:215-295): candidates in stream order,
    judged in that order, until `wanted` are accepted; accepted frames of a batch are encoded together.
    `contains_face` None accepts every candidate.
    """
    written = 0
    while written < wanted:
        vectors = candidates.take(wanted - written if contains_face is None else None)  # a filtered pass cannot know how many it needs
        frames = multi_network.indexed_create_images_vector_device(index, np.stack(vectors), noise_seed=noise_seed)
        accepted: List[int] = []
        judged = len(vectors)
        if contains_face is None:
            accepted = list(range(len(vectors)))
        else:
            host_frames = frames.cpu().numpy()
            for position in range(len(vectors)):
                if any(face_finder.face_locations(host_frames[position])) == contains_face:
                    accepted.append(position)
                    if written + len(accepted) == wanted:
                        judged = position + 1  # the reference stops drawing here: the rest is for the next pass
                        break
        candidates.give_back(vectors[judged:])
        if not accepted:
            continue
        image_paths = [
            output_directory.joinpath(f"{network_name}_{network_hash}_{kind}_{written + offset}.{PNG}") for offset in range(len(accepted))
        ]
        picked = frames if len(accepted) == len(vectors) else frames[torch.tensor(accepted, device=frames.device)]
        image_hashes = write_images_device(picked, image_paths, compression=png_compression)
        for image_path, image_hash, position in zip(image_paths, image_hashes, accepted):
            write_synthesis_file(
                destination_path=image_path.with_suffix(SYNTHESIS_FILE_SUFFIX),
                network_path=network_path,
                network_hash=network_hash,
                image_path=image_path,
                image_hash=image_hash,
                vector=vectors[position],
            )
            LOGGER.info(f"Wrote image {image_path}")
        written += len(accepted)


def images_from_network(  # pylint: disable=too-many-arguments,too-many-locals
    networks_directory: str,
    output_directory: str,
    num_faces: int,
    no_faces: int,
    random_seed: int = DEFAULT_RANDOM_SEED,
    face_finder: Any = None,
    num_images: int = 0,
    frames_per_call: int = DEFAULT_FRAMES_PER_CALL,
    noise_seed: Optional[int] = None,
    png_compression: str = "huffman",
) -> None:
    """
    Load each network of a directory and synthesize stills with it (synthesize_images.py:327-394): per network a
    directory named after it with `{network_name}_{network_hash}_{face|no_face}_{i}.png`, `num_faces` images in which
    `face_finder.face_locations(image)` finds something, then `no_faces` in which it finds nothing, each with its `.json`.
    The vectors are the reference's: one `gaussian_data` draw per candidate from one RandomState(random_seed) that runs
    on across the passes and the networks, whatever `frames_per_call` is.
    :param face_finder: any object with `face_locations(image) -> sequence` (the detector is external, as in the overlay).
    :param num_images: not in the reference: after the two filtered passes, this many unfiltered images per network, named
        `..._any_{i}.png`; they go on in the same vector stream.
    :param frames_per_call: candidates synthesised per engine call (at most the engine's max_batch).
    :param noise_seed: not in the reference, whose images draw fresh noise each (None): with a seed every candidate is
        `indexed_create_image_vector(index, vector, noise_seed=noise_seed)`, so a run can be repeated.
    :param png_compression: not in the reference: still_image_common.COMPRESSIONS; "matches" writes smaller or equal files
        of the same pixels, and the JSON's image_hash is that file's.
    :raises NotImplementedError: num_faces or no_faces non-zero without a face_finder.
    :raises ValueError: an unknown png_compression, before anything is read or written.
    """
    check_compression(png_compression)
    if face_finder is None and (num_faces or no_faces):
        raise NotImplementedError("num_faces / no_faces need a face_finder (an object with face_locations(image)); num_images needs none")
    # sorted: the reference takes the directory's own order, and the vector stream runs on from network to network
    network_paths = sorted(Path(networks_directory).glob(f"*{NETWORK_SUFFIX}"))
    top_level_output_directory = Path(output_directory)
    top_level_output_directory.mkdir(exist_ok=True)
    if not network_paths:
        LOGGER.info(f"Couldn't find any {NETWORK_SUFFIX} files in {networks_directory}. Exiting.")
        return None
    LOGGER.info(f"Found {len(network_paths)} networks.")

    with MultiNetwork(network_paths=network_paths) as multi_network:
        if multi_network is None:
            LOGGER.error("Couldn't load network")
            return None
        candidates = _Candidates(
            vector_length=multi_network.expected_vector_length,
            random_state=np.random.RandomState(random_seed),  # pylint: disable=no-member
            frames_per_call=max(1, min(int(frames_per_call), multi_network.max_batch)),
        )
        for index, network_path in enumerate(network_paths):
            LOGGER.info(f"Writing images for {network_path}")
            network_hash = hash_file(network_path)
            network_name = network_path.with_suffix("").name
            current_output_directory = top_level_output_directory.joinpath(network_name)
            current_output_directory.mkdir(exist_ok=True)
            for kind, contains_face, wanted in [("face", True, num_faces), ("no_face", False, no_faces), ("any", None, num_images)]:
                _write_pass(
                    multi_network=multi_network,
                    index=index,
                    candidates=candidates,
                    wanted=wanted,
                    kind=kind,
                    contains_face=contains_face,
                    face_finder=face_finder,
                    output_directory=current_output_directory,
                    network_name=network_name,
                    network_path=network_path,
                    network_hash=network_hash,
                    noise_seed=noise_seed,
                    png_compression=png_compression,
                )
    return None
