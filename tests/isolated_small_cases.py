"""
The case table of the isolated 4^2 ... 128^2 layer checks, shared by tests/test_isolated_small_layers_gpu.py (which runs the cases on
the device) and tests/test_isolated_coverage.py (which holds the table against the call planner on the CPU).

On 256 CUs with the default flags and no GANCE_TUNE_* knob, conv layers 0 ... 10 (layer_idx) of a call of 1 ... 64 frames run in 25
distinct (layer, form) launches; FORMS lists them with the smallest batch that selects each (a form holds from its batch up to the
next entry's). CASES visits every batch at which a form first appears and checks there only the layers whose form is new, plus the
whole chain at one frame and at 64 (the batch bench.py and the stream issue: the forms of 18 frames, every launch at full occupancy).

NOISE_CASES is the table of tests/test_isolated_noise_gpu.py, which runs the layers with a noise plane per sample
(gance_engine_randomize_noise: sample b reads noise + b * noise_b_stride). It is derived from FORMS: every (layer, form) once, at the
LARGEST batch that still selects it, so that as many samples as possible have b > 0. LARGE_NOISE_CASES are the calls that test makes
of the 256^2 ... 1024^2 layers.
"""

from typing import Dict, List, Tuple

NUM_CUS = 256  # the CU count FORMS was read at (MI355X)
LAST_SMALL_LAYER = 10  # layer_idx of the 128^2 Conv1: the isolated checks of tests/test_isolated_layers_gpu.py start above it

# layer_idx -> [(smallest batch that selects the form, conv launch name)]
FORMS: Dict[int, List[Tuple[int, str]]] = {
    0: [(1, "conv0_4x4_512->512")],
    1: [(1, "convT1_8x8_512->512"), (8, "convTG1_8x8_512->512")],
    2: [(1, "conv2_8x8_512->512"), (16, "convVG2_8x8_512->512")],
    3: [(1, "convT3_16x16_512->512"), (2, "convTG3_16x16_512->512")],
    4: [(1, "conv4_16x16_512->512"), (4, "convVG4_16x16_512->512")],
    5: [(1, "convT5_32x32_512->512"), (6, "convTF5_32x32_512->512/16"), (18, "convTF5_32x32_512->512/s3")],
    6: [(1, "convVG6_32x32_512->512"), (16, "convV6+rgb_32x32_512->512")],
    7: [(1, "convTG7_64x64_512->512"), (8, "convTF7_64x64_512->512/16"), (9, "convTF7_64x64_512->512/s3"), (16, "convTFp7_64x64_512->512/s3")],
    8: [(1, "convVG8_64x64_512->512"), (4, "convV8+rgb_64x64_512->512")],
    9: [(1, "convTG9_128x128_512->256"), (3, "convTF9_128x128_512->256/s3"), (4, "convTFp9_128x128_512->256/s3")],
    10: [(1, "convVG10_128x128_256->256"), (2, "convV10+rgb_128x128_256->256")],
}

# (frames per call, layer_idx checked there)
CASES: List[Tuple[int, List[int]]] = [
    (1, list(range(11))),
    (2, [3, 10]),
    (3, [9]),
    (4, [4, 8, 9]),
    (6, [5]),
    (8, [1, 7]),
    (9, [7]),
    (16, [2, 6, 7]),
    (18, [5]),
    (64, list(range(11))),
]

MAX_BATCH = CASES[-1][0]  # the largest call FORMS describes


def last_batch(layer_idx: int, form: int) -> int:
    """The largest batch that selects the form-th entry of FORMS[layer_idx]: one below the next entry's first, MAX_BATCH for the last."""
    forms = FORMS[layer_idx]
    return forms[form + 1][0] - 1 if form + 1 < len(forms) else MAX_BATCH


def _noise_cases() -> List[Tuple[int, List[int]]]:
    by_batch: Dict[int, List[int]] = {}
    for idx in sorted(FORMS):
        for form in range(len(FORMS[idx])):
            by_batch.setdefault(last_batch(idx, form), []).append(idx)
    return sorted(by_batch.items())


# (frames per call, layer_idx checked there with a noise plane per sample): each form at the last batch of its range
NOISE_CASES: List[Tuple[int, List[int]]] = _noise_cases()

# (conv_form, frames per call) of the per-sample-noise checks of layers 11 ... 16 (1024^2 network), which have one form each over
# 2 ... 64 frames: 9 frames (one row segment at 1024^2: the geometry of 64-frame calls), and the direct form (the conv_mfma.hip
# tiles; the debug tap on conv16+torgb runs the unfused launch). A case of 3 frames (4 row segments) passed and was left out for its
# time (tests/test_isolated_noise_gpu.py).
LARGE_NOISE_CASES: List[Tuple[str, int]] = [("auto", 9), ("direct", 2)]

# conv_form -> {layer_idx: conv launch name} of layers 11 ... 16 in a 1024^2 call of 2 ... 64 frames on 256 CUs
LARGE_NOISE_FORMS: Dict[str, Dict[int, str]] = {
    "auto": {
        11: "convTFp11_256x256_256->128/s3", 12: "convV12+rgb_256x256_128->128",
        13: "convTFp13_512x512_128->64/s3", 14: "convV14+rgb_512x512_64->64",
        15: "convTFp15_1024x1024_64->32/s3", 16: "convV16+rgb_1024x1024_32->32",
    },
    "direct": {
        11: "convTF11_256x256_256->128/s3", 12: "conv12_256x256_128->128",
        13: "convTF13_512x512_128->64/s3", 14: "conv14_512x512_64->64",
        15: "convTF15_1024x1024_64->32/s3", 16: "conv16+torgb_1024x1024_32->32",
    },
}

# the batches tests/test_isolated_layers_gpu.py runs the 256^2 ... 1024^2 layers at on 256 CUs (16 / 8 / 4 / 2 / 1 row segments)
LARGE_LAYER_BATCHES = (1, 2, 3, 5, 9)


def layers_at(batch: int) -> List[int]:
    """The layers the table checks at `batch` frames per call."""
    return dict(CASES)[batch]


def expected_name(layer_idx: int, batch: int) -> str:
    """The conv launch name of the layer in a call of `batch` frames on 256 CUs: the last form selected at or below that batch."""
    return [name for first, name in FORMS[layer_idx] if first <= batch][-1]


def conv_launches(names) -> Dict[int, str]:
    """{layer_idx: conv launch name} of a call's launch names (describe_plan's, or the profiled steps')."""
    launches = {}
    for name in names:
        if name.startswith("conv"):
            kind = name.split("_")[0].split("+")[0]
            launches[int("".join(ch for ch in kind if ch.isdigit()))] = name
    return launches
