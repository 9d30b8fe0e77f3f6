"""
CPU tests of the synthesis-file and file-hash modules: the reference's known answer for its own sample file, round
trips, the version-2 key set, and the older versions.
"""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from gance_amd import synthesis_file
from gance_amd.hash_file import hash_file

SAMPLE = Path(__file__).resolve().parent / "golden" / "sample_synthesis_file.json"


def test_read_vector_of_the_reference_sample_file() -> None:
    """The reference's own hand-verified known answer (its test/test_synthesis_file.py) on its version-0 sample file."""
    vector = synthesis_file.read_vector_in_file(SAMPLE)
    assert vector.shape == (512,)
    assert hashlib.md5(vector.tobytes()).hexdigest() == "ec0b12c590fc748668aadd260664284a"


@pytest.mark.parametrize("shape", [(512,), (18, 512)])
def test_write_then_read_round_trip(tmp_path: Path, shape) -> None:
    data = np.random.RandomState(3).randn(*shape).astype(np.float32)
    path = tmp_path / f"file{synthesis_file.SYNTHESIS_FILE_SUFFIX}"
    synthesis_file.write_synthesis_file(path, data, Path("/networks/a.pkl"), "nethash", Path("/images/a.png"), "imghash")
    back = synthesis_file.read_vector_in_file(path)
    assert back.shape == shape and np.array_equal(back.astype(np.float32), data)
    with open(path) as file:
        written = json.load(file)
    assert set(written) == {"vector", "network_path", "network_hash", "image_path", "image_hash", "version"}
    assert written["version"] == 2 == synthesis_file.Version.version_2
    assert (written["network_path"], written["network_hash"]) == ("/networks/a.pkl", "nethash")
    assert (written["image_path"], written["image_hash"]) == ("/images/a.png", "imghash")


def test_older_versions_read_back(tmp_path: Path) -> None:
    vector = [float(i) / 7 for i in range(512)]
    common = {"image_path": "i.png", "image_hash": "h"}
    files = {
        "v0_no_key": ({"model_path": "m.pkl", "model_hash": "h", "vector": [vector], **common}, vector),
        "v0": ({"model_path": "m.pkl", "model_hash": "h", "vector": [vector], "version": 0, **common}, vector),
        "v1": ({"model_path": "m.pkl", "model_hash": "h", "vector": vector, "version": 1, **common}, vector),
        "v2": ({"network_path": "m.pkl", "network_hash": "h", "vector": vector, "version": 2, **common}, vector),
        "v2_matrix": ({"network_path": "m.pkl", "network_hash": "h", "vector": [vector, vector], "version": 2, **common}, [vector, vector]),
    }
    for name, (content, expected) in files.items():
        path = tmp_path / f"{name}.json"
        path.write_text(json.dumps(content))
        assert np.array_equal(synthesis_file.read_vector_in_file(path), np.array(expected)), name
    (tmp_path / "v1_new_keys.json").write_text(json.dumps({"network_path": "m", "network_hash": "h", "vector": vector, "version": 1, **common}))
    with pytest.raises(KeyError):  # a version-1 file has the model_* keys
        synthesis_file.read_vector_in_file(tmp_path / "v1_new_keys.json")


@pytest.mark.parametrize("size", [0, 8192, 8193])
def test_hash_file_is_the_md5_of_the_contents(tmp_path: Path, size: int) -> None:
    content = np.random.RandomState(size).randint(0, 256, size).astype(np.uint8).tobytes()
    path = tmp_path / "blob"
    path.write_bytes(content)
    assert hash_file(path) == hashlib.md5(content).hexdigest()
