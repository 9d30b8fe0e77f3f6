"""
"Synthesis files": JSON files that describe a vector that was fed into a network, the network that was used and the
resulting image (gance/synthesis_file.py). Same names, signatures and file contents; the reference's dataclasses_json
round trip is plain `json` here.
"""

import json
from enum import IntEnum
from pathlib import Path
from typing import Union

import numpy as np

from gance_amd.vector_sources.vector_types import SingleMatrix, SingleVector

SYNTHESIS_FILE_SUFFIX = ".json"  # synthesis_file.py:17


class Version(IntEnum):
    """Synthesis file versions (synthesis_file.py:20-29)."""

    version_0 = 0
    version_1 = 1

    # Renamed fields with 'model' in them to use 'network' instead.
    version_2 = 2


def write_synthesis_file(  # pylint: disable=too-many-arguments
    destination_path: Path,
    vector: Union[SingleVector, SingleMatrix],
    network_path: Path,
    network_hash: str,
    image_path: Path,
    image_hash: str,
) -> None:
    """
    Write a version-2 synthesis file (synthesis_file.py:61-91): the keys of SynthesisFileDict in its field order.
    :param destination_path: Path to write the file to.
    :param vector: The vector (L,) or matrix (W, L) that was input to the network to produce the image.
    :param network_path: Path to the network used in the synthesis; context for a future reader.
    :param network_hash: Hash of the network file.
    :param image_path: Original path of this file's pair, the image.
    :param image_hash: Hash of the image file.
    """
    with open(str(destination_path), "w") as file:
        json.dump(
            {
                "vector": np.asarray(vector).tolist(),
                "network_path": str(network_path),
                "network_hash": network_hash,
                "image_path": str(image_path),
                "image_hash": image_hash,
                "version": int(Version.version_2),
            },
            file,
        )


def read_vector_in_file(path_to_json: Path) -> SingleVector:
    """
    The vector (only the vector) of a synthesis file of any version (synthesis_file.py:94-121). Files below version 2
    name the network `model_path` / `model_hash`; version 0 (or no `version` key) stored the vector in the network's
    input form [1, L], whose row 0 is the vector.
    :raises KeyError: a file below version 2 without the `model_*` keys, or any file without `vector`.
    """
    with open(str(path_to_json), "r") as file:
        raw_dict = json.load(file)
    if "version" not in raw_dict or raw_dict["version"] is None or raw_dict["version"] < Version.version_2:
        raw_dict["network_path"] = raw_dict.pop("model_path")
        raw_dict["network_hash"] = raw_dict.pop("model_hash")
    version = Version(raw_dict["version"]) if raw_dict.get("version") is not None else Version.version_0
    vector = np.array(raw_dict["vector"])
    if version == Version.version_0:
        vector = vector[0]
    return SingleVector(vector)
