"""
The case table of the isolated checks of config-e generators (fmap_base = 8 << 10), shared by tests/test_isolated_config_e_gpu.py
(which runs the cases on the device) and tests/test_isolated_coverage.py (which holds the table against the call planner on the
CPU). The style is that of tests/isolated_small_cases.py and tests/isolated_image_cases.py.

Conv layers 0 ... 6 (layer_idx; 4^2 ... 32^2, 512 -> 512) of a config-e call have the launch names of a config-f call at every batch
(held by tests/test_isolated_coverage.py), so the config-f checks of tests/test_isolated_small_layers_gpu.py stand for them. From
layer 7 up the channel counts halve a resolution earlier than in config-f, and on 256 CUs with the default flags and no GANCE_TUNE_*
knob layers 7 ... 16 of a call of 1 ... 64 frames run in 27 distinct (layer, form) launches. FORMS lists them with the batch RANGES
that select each, not with first batches: layers 9, 11 and 13 leave "/s3" for "/16x" at exactly 17 frames and return at 18.

CASES visits every batch at which a form of layers 7 ... 12 first appears and checks there the layers whose form is new, and all of
layers 7 ... 12 at one frame and at 64. The network of those checks is the 256^2 one (the smallest that holds layers 7 ... 12), which
plans these layers exactly like the 1024^2 one at every batch of CASES and NOISE_CASES (held by tests/test_isolated_coverage.py; no
(layer, batch) differs, so none has to be checked on the 1024^2 network with the stop-after tap instead). Layers 13 ... 16 are
reached by the batches of ISOLATED in tests/test_config_e_gpu.py (LARGE_LAYER_BATCHES), on the 1024^2 network.

NOISE_CASES, for the checks with a noise plane per sample: every (layer, form) of layers 7 ... 12 once, at the LAST batch of its
(last) range, so that as many samples as possible have b > 0; 17 and 5 are their own last batch. Forms that exist only at one
frame (convVG10, conv12) are run all the same, against the stored plane as the "other" one. Layers 13 ... 16 run with a plane per
sample in the "loud" rows of ISOLATED in tests/test_config_e_gpu.py (2, 3 and 17 frames: their activations at the last batch, 64
frames, are gigabytes to read back).

IMAGE_FORMS / IMAGE_CASES: the image branch at 64^2 ... 512^2. A config-e call produces nine (resolution, form) image launches
there: the stand-alone torgb_<r>x<r> after a plain conv (convVG, conv + finish), and the channel sum in the epilogue of the
F(2x2,3x3) launch ("convW<n>+rgb": Cout / 64 partial images) or of the F(4x4,3x3) launch ("convV<n>+rgb": Cout / 32 partial images).
"""

from typing import Dict, List, Optional, Tuple

from isolated_image_cases import conv1_index, image_launches  # noqa: F401  pylint: disable=unused-import
from isolated_small_cases import conv_launches  # noqa: F401  pylint: disable=unused-import

NUM_CUS = 256  # the CU count FORMS was read at (MI355X)
FIRST_LAYER, LAST_LAYER = 7, 16  # layer_idx of the 64^2 Conv0_up (the first whose channels differ from config-f) and of the 1024^2 Conv1
LAST_SMALL_LAYER = 12  # layer_idx of the 256^2 Conv1: the last layer of the 256^2 network
MAX_BATCH = 64  # the largest call FORMS describes

Ranges = List[Tuple[int, int]]  # [(first batch, last batch)], inclusive

# layer_idx -> [(batch ranges that select the form, conv launch name)]
FORMS: Dict[int, List[Tuple[Ranges, str]]] = {
    7: [([(1, 15)], "convTG7_64x64_512->256"), ([(16, 17)], "convTFp7_64x64_512->256/16x"), ([(18, 64)], "convTFp7_64x64_512->256/s3")],
    8: [
        ([(1, 4)], "convVG8_64x64_256->256"), ([(5, 5)], "conv8_64x64_256->256"), ([(6, 7)], "convW8+rgb_64x64_256->256"),
        ([(8, 64)], "convV8+rgb_64x64_256->256"),
    ],
    9: [
        ([(1, 4)], "convTG9_128x128_256->128"), ([(5, 5)], "convTF9_128x128_256->128/s3"),
        ([(6, 16), (18, 64)], "convTFp9_128x128_256->128/s3"), ([(17, 17)], "convTFp9_128x128_256->128/16x"),
    ],
    10: [
        ([(1, 1)], "convVG10_128x128_128->128"), ([(2, 2)], "conv10_128x128_128->128"), ([(3, 3)], "convW10+rgb_128x128_128->128"),
        ([(4, 64)], "convV10+rgb_128x128_128->128"),
    ],
    11: [
        ([(1, 2)], "convT11_256x256_128->64"), ([(3, 16), (18, 64)], "convTFp11_256x256_128->64/s3"),
        ([(17, 17)], "convTFp11_256x256_128->64/16x"),
    ],
    12: [([(1, 1)], "conv12_256x256_64->64"), ([(2, 64)], "convV12+rgb_256x256_64->64")],
    13: [
        ([(1, 1)], "convT13_512x512_64->32"), ([(2, 16), (18, 64)], "convTFp13_512x512_64->32/s3"),
        ([(17, 17)], "convTFp13_512x512_64->32/16x"),
    ],
    14: [([(1, 64)], "convV14+rgb_512x512_32->32")],
    15: [([(1, 1)], "convT15_1024x1024_32->16"), ([(2, 64)], "convTF15_1024x1024_32->16/16")],
    16: [([(1, 64)], "conv16+torgb_1024x1024_16->16")],
}

SMALL_LAYERS = list(range(FIRST_LAYER, LAST_SMALL_LAYER + 1))  # checked on the 256^2 network
LARGE_LAYERS = list(range(LAST_SMALL_LAYER + 1, LAST_LAYER + 1))  # checked on the 1024^2 network (tests/test_config_e_gpu.py)

# (frames per call, layer_idx checked there): every form of layers 7 ... 12 at the first batch of its range
CASES: List[Tuple[int, List[int]]] = [
    (1, SMALL_LAYERS),
    (2, [10, 12]),
    (3, [10, 11]),
    (4, [10]),
    (5, [8, 9]),
    (6, [8, 9]),
    (8, [8]),
    (16, [7]),
    (17, [9, 11]),
    (18, [7]),
    (64, SMALL_LAYERS),
]

# the batches at which tests/test_config_e_gpu.py::test_layers_512_and_1024_in_isolation runs layers 13 ... 16 with conv_form and
# up_form "auto" on 256 CUs (the 32 -> 16 up layer is one fused launch from 2 frames there); at 17 frames only layers 13 and 14
LARGE_LAYER_BATCHES = (1, 2, 3, 17)
LARGE_CASES: List[Tuple[int, List[int]]] = [(1, LARGE_LAYERS), (2, LARGE_LAYERS), (3, LARGE_LAYERS), (17, [13, 14])]


def first_batch(layer_idx: int, form: int) -> int:
    """The smallest batch that selects the form-th entry of FORMS[layer_idx]."""
    return FORMS[layer_idx][form][0][0][0]


def last_batch(layer_idx: int, form: int) -> int:
    """The largest batch that selects the form-th entry of FORMS[layer_idx]: the end of its last range."""
    return FORMS[layer_idx][form][0][-1][1]


def _noise_cases() -> List[Tuple[int, List[int]]]:
    by_batch: Dict[int, List[int]] = {}
    for idx in SMALL_LAYERS:
        for form in range(len(FORMS[idx])):
            by_batch.setdefault(last_batch(idx, form), []).append(idx)
    return sorted(by_batch.items())


# (frames per call, layer_idx checked there with a noise plane per sample): each form of layers 7 ... 12 at its last batch
NOISE_CASES: List[Tuple[int, List[int]]] = _noise_cases()


def layers_at(batch: int) -> List[int]:
    """The layers CASES checks at `batch` frames per call."""
    return dict(CASES)[batch]


def expected_name(layer_idx: int, batch: int) -> str:
    """The conv launch name of the layer in a config-e call of `batch` frames on 256 CUs."""
    names = [name for ranges, name in FORMS[layer_idx] if any(first <= batch <= last for first, last in ranges)]
    assert len(names) == 1, (layer_idx, batch, names)
    return names[0]


# resolution -> [(batch ranges, the conv launch that does the channel sum or None, partial images)]; None: the stand-alone
# torgb_<r>x<r> sums the channels itself, after a plain conv launch
IMAGE_FORMS: Dict[int, List[Tuple[Ranges, Optional[str], int]]] = {
    64: [([(1, 5)], None, 0), ([(6, 7)], "convW8+rgb_64x64_256->256", 4), ([(8, 64)], "convV8+rgb_64x64_256->256", 8)],
    128: [([(1, 2)], None, 0), ([(3, 3)], "convW10+rgb_128x128_128->128", 2), ([(4, 64)], "convV10+rgb_128x128_128->128", 4)],
    256: [([(1, 1)], None, 0), ([(2, 64)], "convV12+rgb_256x256_64->64", 2)],
    512: [([(1, 64)], "convV14+rgb_512x512_32->32", 1)],
}

# (network resolution, frames per call, resolutions checked there): every image form at the first batch of its range; 3 and 7
# frames: the last sample of an odd call, inside partial images laid out [m][B][3][R][R] (7: "convW8+rgb", 3: "convW10+rgb"); 64
# frames: the last sample of a full call. The bytes are checked at the 256^2 network's last resolution, in every case on it.
IMAGE_CASES: List[Tuple[int, int, List[int]]] = [
    (256, 1, [64, 128, 256]),
    (256, 2, [256]),
    (256, 3, [128, 256]),
    (256, 4, [128]),
    (256, 6, [64]),
    (256, 7, [64, 128, 256]),
    (256, 8, [64]),
    (256, 64, [64, 128, 256]),
    (1024, 1, [512]),
    (1024, 3, [512]),
]


def expected_form(resolution: int, batch: int) -> Tuple[Optional[str], int]:
    """(the conv launch that does the channel sum or None, partial images) of a config-e call of `batch` frames on 256 CUs."""
    forms = [(name, partials) for ranges, name, partials in IMAGE_FORMS[resolution] if any(first <= batch <= last for first, last in ranges)]
    assert len(forms) == 1, (resolution, batch, forms)
    return forms[0]


def form_of(torgb: str, conv: str) -> Tuple[str, str]:
    """What tells one image form of a resolution from another: (ToRGB launch name, the conv kind up to its layer number if it does
    the channel sum: "convW+rgb" / "convV+rgb" / "conv+torgb", else "")."""
    kind = conv.split("_")[0]
    return torgb, ("".join(ch for ch in kind.split("+")[0] if not ch.isdigit()) + "+" + kind.split("+")[1]) if "+" in kind else ""
