"""
Hash a file on disk (gance/hash_file.py).
"""

import hashlib
from pathlib import Path


def hash_file(path_to_file: Path) -> str:
    """
    Hex digest of the MD5 of a file's contents (hash_file.py:9-24), read in pieces so that a network file of hundreds
    of MB is never in memory at once.
    """
    file_hash = hashlib.md5()
    with open(str(path_to_file), "rb") as file:
        for chunk in iter(lambda: file.read(1 << 20), b""):
            file_hash.update(chunk)
    return file_hash.hexdigest()
