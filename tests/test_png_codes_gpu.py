"""
GPU tests that read the deflate blocks of both PNG encoders back (torch.ops.gance.png_encode, csrc/png.hip;
torch.ops.gance.png_encode_lz, csrc/png_lz.hip) with the reader of tests/deflate_ref.py, which tests/test_deflate_ref.py
holds against zlib, and hold every segment to the rules, with no tolerance: the block structure, the three codes
(complete, within their limits, a length exactly where a symbol occurs, never a longer code for a more frequent symbol),
their cost (the Huffman optimum where the unrestricted code fits the limit, the restated limiting rule's where it does
not), the run-length coded header of the match-search mode, its matches, and the choices between the forms of a segment.
The inputs are SHAPES x CONTENTS of png_lz_ref.py and its limit inputs, which reach the 15-bit and the 7-bit limit
(tests/test_png_codes.py proves that without a GPU; here it is asserted again on what was read back).
"""

from functools import lru_cache
from typing import Dict, List, NamedTuple, Sequence, Tuple

import deflate_ref as ref
import numpy as np
import pytest
import torch
from png_lz_ref import CONTENTS, SEGMENT, SHAPES, content, limit_inputs, segment_payloads
from png_ref import filtered_rows, parse_png

from gance_amd import hip_lib, torch_ops  # noqa: F401  pylint: disable=unused-import

pytestmark = pytest.mark.gpu

LIMIT_INPUTS: Dict[str, np.ndarray] = dict(limit_inputs())
CASES: List[Tuple[str, Tuple[int, int]]] = [(kind, shape) for shape in SHAPES for kind in CONTENTS]
CASES += [(name, image.shape[:2]) for name, image in LIMIT_INPUTS.items()]
CASE_IDS = [f"{kind}-{shape[0]}x{shape[1]}" for kind, shape in CASES]


class Segment(NamedTuple):
    """One segment of one file, read back."""

    payload: bytes
    blocks: List[ref.Block]
    size: int  # bytes of the filtered stream it codes
    last: bool

    @property
    def coded(self) -> bool:
        return self.blocks[0].btype == 2

    @property
    def has_match(self) -> bool:
        return any(len(token) == 2 for token in self.blocks[0].tokens)


class ReadBack(NamedTuple):
    stream: bytes  # the reference's filtered stream
    default: List[Segment]  # png_encode's segments
    search: List[Segment]  # png_encode_lz's


def image_of(kind: str, shape: Tuple[int, int]) -> np.ndarray:
    return LIMIT_INPUTS[kind] if kind in LIMIT_INPUTS else content(kind, *shape)


def segments_of(op, image: np.ndarray, stream: bytes) -> List[Segment]:  # type: ignore[no-untyped-def]
    data, offsets = op(torch.from_numpy(image[None]).cuda())
    file_bytes = data[: int(offsets[1])].cpu().numpy().tobytes()
    payloads = segment_payloads(parse_png(file_bytes), file_bytes)
    assert len(payloads) == -(-len(stream) // SEGMENT)
    segments = []
    for index, payload in enumerate(payloads):
        want = stream[index * SEGMENT : (index + 1) * SEGMENT]
        read = ref.read_deflate(payload)
        assert read.produced == want and read.end_bit == 8 * len(payload), index
        segments.append(Segment(payload, read.blocks, len(want), index == len(payloads) - 1))
    return segments


@lru_cache(maxsize=None)
def read_back(kind: str, shape: Tuple[int, int]) -> ReadBack:
    """Both ops' files of one input, encoded and read once for the tests that share them."""
    image = image_of(kind, shape)
    stream = filtered_rows(image)[0].tobytes()
    return ReadBack(stream, segments_of(torch.ops.gance.png_encode, image, stream), segments_of(torch.ops.gance.png_encode_lz, image, stream))


# ---- the checks of one segment ----------------------------------------------------------------------------------------
def check_structure(segment: Segment) -> None:
    """One stored block of the segment's length, or a dynamic block and an empty stored block that ends on a byte boundary."""
    first = segment.blocks[0]
    if first.btype == 0:
        assert len(segment.blocks) == 1 and first.stored_len == segment.size and first.final == int(segment.last)
        assert first.start_bit == 0 and len(segment.payload) == 5 + segment.size
        return
    assert [block.btype for block in segment.blocks] == [2, 0]
    tail = segment.blocks[1]
    assert first.final == 0 and first.start_bit == 0 and tail.final == int(segment.last)
    assert tail.start_bit == first.end_bit and tail.stored_len == 0 and tail.end_bit == tail.token_bit == 8 * len(segment.payload)
    assert len(segment.payload) == -(-(first.end_bit + 3) // 8) + 4  # nothing but the padding between the two


def check_code(name: str, lengths: Sequence[int], histogram: Sequence[int], limit: int) -> None:
    """A complete code within `limit`: a length exactly where a symbol occurs, never a longer code for a more frequent symbol,
    and the cost of the Huffman code where that fits the limit, of the restated limiting rule where it does not."""
    lengths = list(lengths) + [0] * (len(histogram) - len(lengths))
    assert [length > 0 for length in lengths] == [count > 0 for count in histogram], name
    assert ref.kraft(lengths, limit) == 1 << limit and max(lengths) <= limit, name
    shortest_of_the_rarer = limit
    for count in sorted({count for count in histogram if count}):  # ascending: no code longer than any of a rarer symbol
        group = [length for other, length in zip(histogram, lengths) if other == count]
        assert max(group) <= shortest_of_the_rarer, (name, count)
        shortest_of_the_rarer = min(group)
    depth, optimum = ref.huffman_depth_and_cost(histogram)
    paid = sum(count * length for count, length in zip(histogram, lengths))
    want = optimum if depth <= limit else ref.cost(histogram, ref.limited_lengths(histogram, limit))
    assert paid == want, (name, depth, paid, want)


def header_bits_of(block: ref.Block) -> int:
    return 17 + 3 * block.hclen + sum(block.cl_lengths[symbol] + ref.CL_EXTRA.get(symbol, 0) for symbol, _ in block.cl_symbols)


def check_codes(block: ref.Block, with_matches: bool) -> None:
    """The three codes of a dynamic block, its header and its bit counts."""
    assert block.ll_histogram[ref.END_OF_BLOCK] == 1 and block.ll_lengths[ref.END_OF_BLOCK] > 0
    check_code("literal/length", block.ll_lengths, block.ll_histogram, ref.LIT_LIMIT)
    used_distances = [symbol for symbol, count in enumerate(block.d_histogram) if count]
    if with_matches:
        assert used_distances and block.hlit == max(257, 1 + max(symbol for symbol, count in enumerate(block.ll_histogram) if count))
        assert block.hdist == 1 + used_distances[-1]
        if len(used_distances) == 1:  # one code of one bit
            assert block.d_lengths == [0] * used_distances[0] + [1]
        else:
            check_code("distance", block.d_lengths, block.d_histogram, ref.DIST_LIMIT)
        assert block.cl_symbols == ref.run_length_symbols(block.ll_lengths + block.d_lengths)
        at = 0
        for token in block.tokens:
            if len(token) == 2:
                assert 3 <= token[0] <= 258 and 1 <= token[1] <= at, (token, at)  # never before the segment's first byte
            at += 1 if len(token) == 1 else token[0]
    else:
        assert not used_distances and (block.hlit, block.hdist, block.d_lengths) == (257, 1, [1])
        assert block.cl_symbols == [(length, 0) for length in block.ll_lengths + [1]]  # no 16, 17 or 18
    check_code("code-length", block.cl_lengths, ref.cl_histogram(block.cl_symbols), ref.CL_LIMIT)
    sent = [block.cl_lengths[symbol] > 0 for symbol in ref.CL_ORDER]
    assert block.hclen == max(4, 19 - sent[::-1].index(True))  # the lengths sent end at the last used symbol of the order
    assert block.token_bit - block.start_bit == header_bits_of(block)
    assert block.end_bit - block.token_bit == ref.data_bits(block)


def literal_only_bits(piece: bytes) -> Tuple[int, int]:
    """(header bits, data bits) of the default encoder's coded form of a segment, by the restatements."""
    histogram = np.bincount(np.frombuffer(piece, dtype=np.uint8), minlength=257).tolist()
    histogram[ref.END_OF_BLOCK] = 1
    lengths = ref.limited_lengths(histogram, ref.LIT_LIMIT)
    sent = [lengths.get(symbol, 0) for symbol in range(257)] + [1]
    header = [sent.count(length) for length in range(19)]
    cl_lengths = ref.limited_lengths(header, ref.CL_LIMIT)
    hclen = max(4, 19 - [symbol in cl_lengths for symbol in ref.CL_ORDER][::-1].index(True))
    return 17 + 3 * hclen + ref.cost(header, cl_lengths), ref.cost(histogram, lengths)


def check_default_choice(segment: Segment, piece: bytes) -> None:
    """Coded exactly when ceil((header bits + data bits + 3) / 8) + 4 <= 5 + n."""
    header_bits, data_bits = literal_only_bits(piece)
    if segment.coded:
        block = segment.blocks[0]
        assert (block.token_bit - block.start_bit, block.end_bit - block.token_bit) == (header_bits, data_bits)
    assert segment.coded == (-(-(header_bits + data_bits + 3) // 8) + 4 <= 5 + len(piece)), (header_bits, data_bits, len(piece))


@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_every_segment_keeps_the_rules(kind: str, shape: Tuple[int, int]) -> None:
    stream, default, search = read_back(kind, shape)
    for index, (plain, with_search) in enumerate(zip(default, search)):
        piece = stream[index * SEGMENT : (index + 1) * SEGMENT]
        check_structure(plain)
        check_structure(with_search)
        assert not plain.has_match
        if plain.coded:
            check_codes(plain.blocks[0], with_matches=False)
        check_default_choice(plain, piece)
        # the match search: never larger; with a match strictly smaller (the earlier form on equal sizes), else the same bytes
        if with_search.has_match:
            check_codes(with_search.blocks[0], with_matches=True)
            assert len(with_search.payload) < len(plain.payload), index
        else:
            assert with_search.payload == plain.payload, index


# ---- the inputs reach the limits, on what was read back ----------------------------------------------------------------
def depth_of(histogram: Sequence[int]) -> int:
    return ref.huffman_depth_and_cost(histogram)[0]


def test_both_ops_repair_a_literal_code_deeper_than_15() -> None:
    fibonacci = read_back("fibonacci", LIMIT_INPUTS["fibonacci"].shape[:2])
    scene256 = read_back("scene256", (256, 256))
    for name, segments in [("png_encode", fibonacci.default), ("png_encode_lz", fibonacci.search)]:
        assert len(segments) == 1 and segments[0].coded
        block = segments[0].blocks[0]
        print(f"{name} fibonacci: depth {depth_of(block.ll_histogram)}, longest code {max(block.ll_lengths)}, {len(segments[0].payload)} bytes")
        assert depth_of(block.ll_histogram) >= 17 and max(block.ll_lengths) == 15
    for name, segments in [("png_encode", scene256.default), ("png_encode_lz", scene256.search)]:
        assert len(segments) == 7 and all(segment.coded for segment in segments)
        depths = [depth_of(segment.blocks[0].ll_histogram) for segment in segments]
        print(f"{name} scene(256, 2): depths {depths}")
        assert depths[1] == 16 and max(segments[1].blocks[0].ll_lengths) == 15


def test_both_ops_repair_a_code_length_code_deeper_than_7() -> None:
    dyadic = read_back("dyadic", LIMIT_INPUTS["dyadic"].shape[:2])
    for name, segments in [("png_encode", dyadic.default), ("png_encode_lz", dyadic.search)]:
        assert len(segments) == 2 and segments[0].coded
        block = segments[0].blocks[0]
        depth = depth_of(ref.cl_histogram(block.cl_symbols))
        print(f"{name} dyadic: code-length depth {depth}, longest code {max(block.cl_lengths)}, literal depth {depth_of(block.ll_histogram)}")
        assert depth >= 8 and max(block.cl_lengths) == 7


def test_match_search_wins_under_a_deep_literal_code() -> None:
    """The Fibonacci rows over flat rows: the default encoder repairs a code 17 bits deep, the match search codes the
    segment with matches and many distance symbols, and smaller. (No input was found whose block WITH matches is deeper
    than 15; tools/png_lz_codes_check.hip drives that case on the host.)"""
    flat = read_back("fibonacci_flat", LIMIT_INPUTS["fibonacci_flat"].shape[:2])
    (plain,), (with_search,) = flat.default, flat.search
    assert plain.coded and depth_of(plain.blocks[0].ll_histogram) == 17 and max(plain.blocks[0].ll_lengths) == 15
    block = with_search.blocks[0]
    matches = [token for token in block.tokens if len(token) == 2]
    print(f"fibonacci_flat: {len(with_search.payload)} bytes against {len(plain.payload)}, {len(matches)} matches, "
          f"literal/length depth {depth_of(block.ll_histogram)}, longest code {max(block.ll_lengths)}")  # fmt: skip
    assert with_search.has_match and len(with_search.payload) < len(plain.payload)
    # the 14 448 zeros are copies at distance 1, but for the run's first bytes and the segment's last (a row of slack)
    assert sum(1 for count in block.d_histogram if count) >= 3 and sum(token[0] for token in matches if token[1] == 1) >= 48 * 301 - 301


def test_the_cases_reach_every_form() -> None:
    """Over all the inputs: stored and coded segments of the default encoder; all three forms of the match search; one, two
    and more used distance symbols; headers with 16, 17 and 18."""
    forms, distances, repeats = set(), set(), set()
    for kind, shape in CASES:
        _, default, search = read_back(kind, shape)
        forms |= {("default", segment.coded) for segment in default}
        for segment in search:
            forms.add(("search", segment.coded, segment.has_match))
            if segment.has_match:
                distances.add(min(3, sum(1 for count in segment.blocks[0].d_histogram if count)))
                repeats |= {symbol for symbol, _ in segment.blocks[0].cl_symbols if symbol >= 16}
    assert forms == {("default", False), ("default", True), ("search", False, False), ("search", True, False), ("search", True, True)}
    assert distances == {1, 2, 3} and repeats == {16, 17, 18}
