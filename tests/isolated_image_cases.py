"""
The case table of the isolated image-branch checks (ToRGB + upsample of the skip image + bias, and the bytes), shared by
tests/test_isolated_image_gpu.py (which runs the cases on the device) and tests/test_isolated_coverage.py (which holds the table
against the call planner on the CPU).

On 256 CUs with the default flags and no GANCE_TUNE_* knob a call of 1 ... 64 frames produces twelve (resolution, form) image
launches: at every resolution up to 128^2 the small kernel (torgb_small_kernel: the channel sum split 8 ways through LDS; 4^2 has
no skip image), and from some batch up at 32^2 ... 128^2, always at 256^2 ... 1024^2, the channel sum in the epilogue of the
F(4x4,3x3) conv launch ("convV<n>+rgb": Cout / 32 partial images, which torgb_kernel adds; one partial image is finished in place
in the skip buffer). The 1024^2 and 128^2 networks agree on the first six resolutions. With conv_form="direct" there are two more
forms: torgb_kernel doing the channel sum itself (256^2, 512^2), and the whole ToRGB in the last conv ("conv16+torgb").
"""

from typing import Dict, List, Optional, Tuple

NUM_CUS = 256  # the CU count FORMS was read at (MI355X)

# resolution -> [(smallest batch that selects the form, the conv launch that does the channel sum or None, partial images)];
# None: the ToRGB pass sums the channels itself (a form holds from its batch up to the next entry's)
FORMS: Dict[int, List[Tuple[int, Optional[str], int]]] = {
    4: [(1, None, 0)],
    8: [(1, None, 0)],
    16: [(1, None, 0)],
    32: [(1, None, 0), (16, "convV6+rgb_32x32_512->512", 16)],
    64: [(1, None, 0), (4, "convV8+rgb_64x64_512->512", 16)],
    128: [(1, None, 0), (2, "convV10+rgb_128x128_256->256", 8)],
    256: [(1, "convV12+rgb_256x256_128->128", 4)],
    512: [(1, "convV14+rgb_512x512_64->64", 2)],
    1024: [(1, "convV16+rgb_1024x1024_32->32", 1)],
}

# conv_form="direct", every batch: no partial images; the last conv absorbs its whole ToRGB (and there is no ToRGB pass)
DIRECT_FORMS: Dict[int, Optional[str]] = {256: None, 512: None, 1024: "conv16+torgb_1024x1024_32->32"}

# (network resolution, conv_form, frames per call, resolutions checked there). 64 frames: the last sample of a full call, the
# partial images indexed with the call's batch; 3 frames: odd, the last sample inside partial images laid out [m][B][3][R][R]
CASES: List[Tuple[int, str, int, List[int]]] = [
    (128, "auto", 1, [4, 8, 16, 32, 64, 128]),
    (128, "auto", 2, [128]),
    (128, "auto", 4, [64]),
    (128, "auto", 16, [32]),
    (128, "auto", 64, [4, 8, 16, 32, 64, 128]),
    (1024, "auto", 1, [256, 512, 1024]),
    (1024, "auto", 3, [256, 512, 1024]),
    (1024, "direct", 2, [256, 512, 1024]),
]


def conv1_index(resolution: int) -> int:
    """layer_idx of the conv in front of the resolution's ToRGB (the 4x4 conv, or Conv1)."""
    return max(0, 2 * (resolution.bit_length() - 1) - 4)


def expected_form(resolution: int, batch: int, conv_form: str = "auto") -> Tuple[Optional[str], int]:
    """(the conv launch that does the channel sum or None, partial images) of a call of `batch` frames on 256 CUs."""
    if conv_form == "direct":  # (up to 128^2: the small kernel after a plain conv)
        return DIRECT_FORMS.get(resolution), 0
    return [(name, partials) for first, name, partials in FORMS[resolution] if first <= batch][-1]


def image_launches(names) -> Dict[int, Tuple[str, str]]:
    """{resolution: (its ToRGB launch name or "", the conv launch name in front of it)} of a call's launch names
    (describe_plan's, or the profiled steps')."""
    names = list(names)
    launches = {}
    for name in names:
        if name.startswith("conv"):
            kind, size = name.split("_")[0:2]
            resolution = int(size.split("x")[0])
            if int("".join(ch for ch in kind.split("+")[0] if ch.isdigit())) == conv1_index(resolution):
                torgb = f"torgb_{resolution}x{resolution}"
                launches[resolution] = (torgb if torgb in names else "", name)
    return launches


def form_of(torgb: str, conv: str) -> Tuple[str, str]:
    """What tells one image form of a resolution from another: (ToRGB launch name, "+rgb" / "+torgb" / "" of the conv)."""
    kind = conv.split("_")[0]
    return torgb, ("+" + kind.split("+")[1]) if "+" in kind else ""
