"""
The calls of tests/test_workspace_state_gpu.py (what one workspace is put through, whatever form each call takes) and the launch
names those calls must have on 256 CUs, put together from the three case tables of the isolated checks: tests/isolated_small_cases.py
(config-f layers 0 ... 10, and 11 ... 16 from two frames up), tests/isolated_image_cases.py (config-f image launches) and
tests/isolated_config_e_cases.py (config-e layers 7 ... 16 and image launches; layers 0 ... 6 are named as in config-f).
tests/test_workspace_state_cases.py holds `name_misses` against the call planner on the CPU, so that "the workspace stayed clean
after every production form" is a statement about the planner's forms and not about whatever happened to run.

The geometry of the zero borders is restated here, apart from the library: an activation plane [res + 2][res + 8] has its interior
at rows 1 ... res, columns 4 ... res + 3; a parity plane [H + 3][W + 8] of class (py, px) owns rows 1 ... H + 1 - py, columns
4 ... W + 4 - px. Everything else is border.
"""

import random
from typing import Dict, List, NamedTuple, Tuple

import isolated_config_e_cases as e_cases
import isolated_image_cases as image_cases
import isolated_small_cases as small_cases

NUM_CUS = small_cases.NUM_CUS
POISON = float(2 ** 20)  # finite (a padded K's zero weights still contribute exactly 0) and far above any activation
ORDER_SEED = 20


class Network(NamedTuple):
    config: str  # "f" or "e"
    resolution: int
    max_batch: int
    batches: Tuple[int, ...]
    history_batches: Tuple[int, ...]  # the batches whose results are held to pristine engines' (the 1024^2 networks: fewer, for time)


NETWORKS: Dict[str, Network] = {
    "f-128": Network("f", 128, 64, tuple(batch for batch, _ in small_cases.CASES), tuple(batch for batch, _ in small_cases.CASES)),
    "e-256": Network("e", 256, 64, tuple(batch for batch, _ in e_cases.CASES), tuple(batch for batch, _ in e_cases.CASES)),
    "f-1024": Network("f", 1024, 9, small_cases.LARGE_LAYER_BATCHES, (1, 3, 9)),
    "e-1024": Network("e", 1024, 17, e_cases.LARGE_LAYER_BATCHES, (1, 3, 17)),
}

# every forced form of the 128^2 config-f network, all on one shared workspace
FORCED_RESOLUTION, FORCED_MAX_BATCH, FORCED_BATCHES = 128, 64, (1, 5, 64)
FORCED_FORMS: List[Tuple[str, str]] = [(conv_form, up_form) for conv_form in ("direct", "winograd", "winograd43") for up_form in ("auto", "split", "fused")] + [
    ("auto", "split"), ("auto", "fused"),
]


def call_order(batches) -> List[int]:
    """The batches once in a seeded shuffled order, then once descending: every form both follows and precedes forms of other batches."""
    shuffled = list(batches)
    random.Random(ORDER_SEED).shuffle(shuffled)
    return shuffled + sorted(batches, reverse=True)


def act_border_words(res: int) -> int:
    """Border words of one activation plane [res + 2][res + 8]."""
    return (res + 2) * (res + 8) - res * res


def parity_border_words(h: int, py: int, px: int) -> int:
    """Border words of one parity plane [h + 3][h + 8] of class (py, px)."""
    return (h + 3) * (h + 8) - (h + 1 - py) * (h + 1 - px)


def name_misses(config: str, resolution: int, batch: int, names) -> List[str]:
    """What is wrong with the launch names of a default-form call of `batch` frames on 256 CUs, by the three case tables."""
    names = list(names)
    misses = []
    launches = small_cases.conv_launches(names)
    num_convs = 2 * (resolution.bit_length() - 1) - 3
    if sorted(launches) != list(range(num_convs)):
        misses.append(f"conv launches of layers {sorted(launches)}, expected 0 ... {num_convs - 1}")
    for idx, name in sorted(launches.items()):
        if config == "e" and idx >= e_cases.FIRST_LAYER:
            want = e_cases.expected_name(idx, batch)
        elif idx <= small_cases.LAST_SMALL_LAYER:
            want = small_cases.expected_name(idx, batch)
        elif batch >= 2:
            want = small_cases.LARGE_NOISE_FORMS["auto"][idx]
        else:
            continue  # (config-f layers 11 ... 16 at one frame: no table names them)
        if name != want:
            misses.append(f"layer {idx} at {batch} frames: {name}, the table has {want}")
    images = image_cases.image_launches(names)
    forms = e_cases.IMAGE_FORMS if config == "e" else image_cases.FORMS
    for r in sorted(forms):
        if r > resolution:
            continue
        want, _ = e_cases.expected_form(r, batch) if config == "e" else image_cases.expected_form(r, batch)
        if r not in images:
            misses.append(f"{r}^2 image at {batch} frames: no conv launch in front of it")
            continue
        _, conv = images[r]
        if (want is None and "+" in conv.split("_")[0]) or (want is not None and conv != want):
            misses.append(f"{r}^2 image at {batch} frames: {conv}, the table has {want or 'a plain conv'}")
    return misses
