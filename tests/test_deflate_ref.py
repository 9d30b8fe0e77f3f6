"""
CPU tests of the raw-deflate reader of tests/deflate_ref.py against zlib, which is the reference here: on zlib's own
streams of the PNG tests' filtered bytes (dynamic, fixed and stored blocks, with and without matches) the reader gives
the input back, every coded block's histograms account for exactly the bits between its first token and its end, and
zlib's codes are complete. That is what entitles the reader to judge the GPU encoders' files (tests/test_png_codes_gpu.py).
"""

import zlib
from typing import Dict, List, Tuple

import deflate_ref as ref
import numpy as np
import pytest
from png_lz_ref import CONTENTS, SEGMENT, content, panel
from png_ref import filtered_rows, scene

# name -> (level, strategy)
MODES: Dict[str, Tuple[int, int]] = {
    "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
    "rle": (6, zlib.Z_RLE), "fixed": (6, zlib.Z_FIXED), "level0": (0, zlib.Z_DEFAULT_STRATEGY),
}


def streams() -> List[Tuple[str, bytes]]:
    images = [(kind, content(kind, 64, 64)) for kind in CONTENTS]
    images += [("scene128", scene(128, 1)), ("panel128", panel(128)), ("ramp4x300", content("ramp", 4, 300)), ("one_pixel", content("scene", 1, 1))]
    return [(name, filtered_rows(image)[0].tobytes()) for name, image in images]


STREAMS = streams()


def check_block(block: ref.Block) -> None:
    if block.btype == 0:
        assert block.end_bit - block.token_bit == 8 * block.stored_len and block.token_bit % 8 == 0
        return
    assert ref.data_bits(block) == block.end_bit - block.token_bit
    assert sum(block.ll_histogram) == len(block.tokens) + 1 and block.ll_histogram[256] == 1
    assert sum(block.d_histogram) == sum(1 for token in block.tokens if len(token) == 2)
    if block.btype == 2:
        # zlib's three codes are complete: it gives two symbols a code even where one or none is used
        assert ref.kraft(block.ll_lengths, 15) == 1 << 15
        assert ref.kraft(block.d_lengths, 15) == 1 << 15
        assert ref.kraft(block.cl_lengths, 7) == 1 << 7
        assert len(block.ll_lengths) == block.hlit and len(block.d_lengths) == block.hdist
        header_bits = 17 + 3 * block.hclen + sum(block.cl_lengths[symbol] + ref.CL_EXTRA.get(symbol, 0) for symbol, _ in block.cl_symbols)
        assert block.token_bit - block.start_bit == header_bits


@pytest.mark.parametrize("mode", list(MODES))
def test_reader_gives_zlibs_streams_back_and_accounts_for_every_bit(mode: str) -> None:
    level, strategy = MODES[mode]
    kinds = set()
    for name, stream in STREAMS:
        for start in range(0, len(stream), SEGMENT):
            piece = stream[start : start + SEGMENT]
            for flush in (zlib.Z_SYNC_FLUSH, zlib.Z_FINISH):
                compressor = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
                packed = compressor.compress(piece) + compressor.flush(flush)
                read = ref.read_deflate(packed)
                assert read.produced == piece, (name, start)
                assert read.end_bit == 8 * len(packed) if flush == zlib.Z_SYNC_FLUSH else -(-read.end_bit // 8) == len(packed)
                assert [block.final for block in read.blocks] == [0] * (len(read.blocks) - 1) + [1 if flush == zlib.Z_FINISH else 0]
                position = 0
                for block in read.blocks:
                    assert block.start_bit == position
                    check_block(block)
                    position = block.end_bit
                    kinds.add(block.btype)
                    if any(len(token) == 2 for token in block.tokens):
                        kinds.add("matches")
                tokens = [token for block in read.blocks for token in block.tokens]
                assert sum(1 if len(token) == 1 else token[0] for token in tokens) == len(piece) - sum(b.stored_len or 0 for b in read.blocks)
    want = {
        "level1": {0, 2, "matches"}, "level6": {0, 2, "matches"}, "huffman_only": {0, 2}, "rle": {0, 2, "matches"}, "fixed": {0, 1, "matches"},
        "level0": {0},
    }[mode]
    assert want <= kinds, kinds  # the block types the mode is there for did occur
    if mode == "huffman_only":
        assert "matches" not in kinds


def test_reader_refuses_what_the_format_forbids() -> None:
    packed = zlib.compress(STREAMS[0][1], 6)[2:-4]
    assert ref.read_deflate(packed).produced == STREAMS[0][1]
    with pytest.raises(ValueError):
        ref.read_deflate(packed[: len(packed) // 2])  # cut short
    with pytest.raises(ValueError):
        ref.read_deflate(b"\x07")  # BTYPE 3
    with pytest.raises(ValueError):
        ref.read_deflate(b"\x01\x01\x00\x00\x00\x55")  # NLEN is not LEN's complement
    # fixed block: a match of length 3 at distance 1 with nothing before it
    with pytest.raises(ValueError, match="before the stream"):
        ref.read_deflate(bytes([0b00000011, 0b00000010, 0, 0]))


def test_restatements_on_small_histograms() -> None:
    """Known answers: 1 1 2 3 5 has the depths 4 4 3 2 1; limits bite as package-merge says; runs as RFC 1951 3.2.7 reads."""
    histogram = [5, 3, 2, 1, 1]
    assert ref.huffman_depths(histogram) == {0: 1, 1: 2, 2: 3, 3: 4, 4: 4}
    assert ref.huffman_depth_and_cost(histogram) == (4, 5 + 6 + 6 + 4 + 4)
    assert ref.package_merge_cost(histogram, 4) == 25 and ref.package_merge_cost(histogram, 15) == 25
    assert ref.package_merge_cost(histogram, 3) == 5 * 2 + 3 * 2 + 2 * 2 + 3 + 3 == 26
    assert ref.limited_lengths(histogram, 3) == {0: 1, 1: 3, 2: 3, 3: 3, 4: 3}  # 26 bits as well
    assert ref.cost(histogram, ref.limited_lengths(histogram, 3)) == 26
    # 1 1 2 4 8 16 at a limit of 4: depths 5 5 4 3 2 1; 4 4 4 3 2 1 is one place over; the 3 is lengthened
    assert ref.limited_lengths([16, 8, 4, 2, 1, 1], 4) == {0: 1, 1: 2, 2: 4, 3: 4, 4: 4, 5: 4}
    assert ref.package_merge_cost([16, 8, 4, 2, 1, 1], 4) == 16 + 16 + 16 + 8 + 4 + 4
    assert ref.limited_lengths(histogram, 4) == ref.huffman_depths(histogram)
    rs = np.random.RandomState(5)
    for _ in range(40):
        histogram = list((rs.randint(0, 2, 40) * rs.geometric(0.02, 40)))
        histogram[7] += 1
        histogram[9] += 1
        depth, best = ref.huffman_depth_and_cost(histogram)
        for limit in (6, 7, 9, 15):
            lengths = ref.limited_lengths(histogram, limit)
            assert ref.kraft(list(lengths.values()), limit) == 1 << limit and max(lengths.values()) <= limit
            assert best <= ref.package_merge_cost(histogram, limit) <= ref.cost(histogram, lengths)
            if depth <= limit:
                assert ref.cost(histogram, lengths) == best == ref.package_merge_cost(histogram, limit)
    lengths = [0] * 139 + [5] + [7] * 8 + [0, 0] + [3] * 4 + [0] * 10
    assert ref.run_length_symbols(lengths) == [(18, 127), (0, 0), (5, 0), (7, 0), (16, 3), (7, 0), (0, 0), (0, 0), (3, 0), (16, 0), (17, 7)]
