"""
A raw-deflate (RFC 1951) reader that reports what it read, and restatements of the code-building rules of the two PNG
encoders (gance_amd/csrc/png.hip, png_lz.hip), for the tests that read the encoders' blocks back. Pure Python, written
from RFC 1951 and from the rules as the headers of csrc/png_common.h and csrc/png_lz_codes.h state them, not from the
kernels. tests/test_deflate_ref.py holds the reader against zlib's own streams. Not collected by pytest.

The reader takes one raw deflate stream, or a piece of one that ends on a byte boundary behind a block (a segment's payload
as png_lz_ref.segment_payloads cuts them: a Z_SYNC_FLUSH point), and decodes it with per-block lookup tables.
"""

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)  # RFC 1951 3.2.7
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DISTANCE_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
                 16385, 24577)  # fmt: skip
DISTANCE_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_EXTRA = {16: 2, 17: 3, 18: 7}
END_OF_BLOCK = 256
LIT_LIMIT, DIST_LIMIT, CL_LIMIT = 15, 15, 7

Token = Tuple[int, ...]  # (byte,) or (length, distance)


@dataclass
class Block:
    """One block of a stream. Bit positions count from the stream's first bit."""

    final: int
    btype: int  # 0 stored, 1 fixed, 2 dynamic
    start_bit: int  # of BFINAL
    token_bit: int  # of the first token's code; stored: of the first data byte
    end_bit: int  # behind the end-of-block code; stored: behind the last data byte
    stored_len: Optional[int] = None
    hlit: Optional[int] = None  # the counts themselves: 257 .. 286, 1 .. 30, 4 .. 19
    hdist: Optional[int] = None
    hclen: Optional[int] = None
    cl_lengths: List[int] = field(default_factory=list)  # [19] by symbol; dynamic blocks only
    cl_symbols: List[Tuple[int, int]] = field(default_factory=list)  # (code-length symbol, its extra value or 0) as sent
    ll_lengths: List[int] = field(default_factory=list)  # [hlit] (fixed: 288)
    d_lengths: List[int] = field(default_factory=list)  # [hdist] (fixed: 30)
    tokens: List[Token] = field(default_factory=list)
    ll_histogram: List[int] = field(default_factory=list)  # [286], end-of-block counted
    d_histogram: List[int] = field(default_factory=list)  # [30]


@dataclass
class Stream:
    produced: bytes
    blocks: List[Block]
    end_bit: int  # behind the last block


def _decode_table(lengths: Sequence[int]) -> Tuple[List[int], int]:
    """(table, bits): table[the next `bits` bits, LSB first] = symbol << 4 | code length, -1 where no code begins so."""
    bits = max(max(lengths), 1)
    count = [0] * (bits + 2)
    for length in lengths:
        count[length] += 1
    count[0] = 0
    if sum(count[length] << (bits - length) for length in range(1, bits + 1)) > 1 << bits:
        raise ValueError("over-subscribed code")
    next_code, code = [0] * (bits + 2), 0
    for length in range(1, bits + 1):  # RFC 1951 3.2.2
        code = (code + count[length - 1]) << 1
        next_code[length] = code
    table = [-1] * (1 << bits)
    for symbol, length in enumerate(lengths):
        if length == 0:
            continue
        code = next_code[length]
        next_code[length] += 1
        reverse = int(format(code, f"0{length}b")[::-1], 2)
        fill = 1 << (bits - length)
        table[reverse :: 1 << length] = [symbol << 4 | length] * fill
    return table, bits


def read_deflate(data: bytes) -> Stream:
    """
    Decode `data` block by block up to the block with BFINAL, or to the end of `data` where that is a byte boundary
    behind a block. :raises ValueError: anything RFC 1951 forbids, a distance before the stream's first byte, data cut short.
    """
    padded = bytes(data) + b"\0\0\0\0"
    total_bits = 8 * len(data)
    position = 0
    out = bytearray()
    blocks: List[Block] = []

    def take(count: int) -> int:
        nonlocal position
        at = position >> 3
        value = (int.from_bytes(padded[at : at + 4], "little") >> (position & 7)) & ((1 << count) - 1)
        position += count
        if position > total_bits:
            raise ValueError("stream cut short")
        return value

    def symbol_of(table: List[int], bits: int) -> int:
        nonlocal position
        at = position >> 3
        entry = table[(int.from_bytes(padded[at : at + 4], "little") >> (position & 7)) & ((1 << bits) - 1)]
        if entry < 0:
            raise ValueError(f"no code at bit {position}")
        position += entry & 15
        if position > total_bits:
            raise ValueError("stream cut short")
        return entry >> 4

    while True:
        start = position
        final, btype = take(1), take(2)
        if btype == 3:
            raise ValueError("BTYPE 3")
        if btype == 0:
            position = (position + 7) & ~7
            length, complement = take(16), take(16)
            if length != complement ^ 0xFFFF:
                raise ValueError("LEN / NLEN")
            block = Block(final, 0, start, position, position + 8 * length, stored_len=length)
            if block.end_bit > total_bits:
                raise ValueError("stream cut short")
            out += data[position >> 3 : (position >> 3) + length]
            position = block.end_bit
        else:
            block = Block(final, btype, start, 0, 0)
            if btype == 1:
                block.ll_lengths = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                block.d_lengths = [5] * 30
                distance_table_lengths = [5] * 32
            else:
                block.hlit, block.hdist, block.hclen = take(5) + 257, take(5) + 1, take(4) + 4
                if block.hlit > 286 or block.hdist > 30:
                    raise ValueError("HLIT / HDIST")
                block.cl_lengths = [0] * 19
                for index in range(block.hclen):
                    block.cl_lengths[CL_ORDER[index]] = take(3)
                cl_table, cl_bits = _decode_table(block.cl_lengths)
                lengths: List[int] = []
                while len(lengths) < block.hlit + block.hdist:
                    symbol = symbol_of(cl_table, cl_bits)
                    extra = take(CL_EXTRA[symbol]) if symbol >= 16 else 0
                    block.cl_symbols.append((symbol, extra))
                    if symbol < 16:
                        lengths.append(symbol)
                    elif symbol == 16:
                        if not lengths:
                            raise ValueError("repeat of nothing")
                        lengths += [lengths[-1]] * (3 + extra)
                    else:
                        lengths += [0] * ((3 if symbol == 17 else 11) + extra)
                if len(lengths) != block.hlit + block.hdist:
                    raise ValueError("a run passes the last code length")
                block.ll_lengths, block.d_lengths = lengths[: block.hlit], lengths[block.hlit :]
                distance_table_lengths = block.d_lengths
                if block.ll_lengths[END_OF_BLOCK] == 0:
                    raise ValueError("no end-of-block code")
            ll_table, ll_bits = _decode_table(block.ll_lengths)
            d_table, d_bits = _decode_table(distance_table_lengths)
            block.token_bit = position
            block.ll_histogram, block.d_histogram = [0] * 286, [0] * 30
            block_begin = len(out)
            while True:
                symbol = symbol_of(ll_table, ll_bits)
                if symbol < 256:
                    out.append(symbol)
                    continue
                if symbol == END_OF_BLOCK:
                    break
                if symbol > 285:
                    raise ValueError("length symbol 286 / 287")
                length = LENGTH_BASE[symbol - 257] + take(LENGTH_EXTRA[symbol - 257])
                distance_symbol = symbol_of(d_table, d_bits)
                if distance_symbol > 29:
                    raise ValueError("distance symbol 30 / 31")
                distance = DISTANCE_BASE[distance_symbol] + take(DISTANCE_EXTRA[distance_symbol])
                if distance > len(out):
                    raise ValueError(f"distance {distance} at byte {len(out)}: before the stream")
                block.tokens.append((len(out), length, distance))  # with its place; the literals between come in below
                if distance >= length:
                    out += out[len(out) - distance : len(out) - distance + length]
                else:
                    for _ in range(length):
                        out.append(out[-distance])
            block.end_bit = position
            # tokens in stream order: the literals between the matches noted above
            matches, block.tokens = block.tokens, []
            at = block_begin
            for where, length, distance in matches:
                block.tokens += [(byte,) for byte in out[at:where]]
                block.tokens.append((length, distance))
                at = where + length
            block.tokens += [(byte,) for byte in out[at:]]
            for token in block.tokens:
                if len(token) == 1:
                    block.ll_histogram[token[0]] += 1
                else:
                    block.ll_histogram[length_symbol(token[0])] += 1
                    block.d_histogram[distance_symbol_of(token[1])] += 1
            block.ll_histogram[END_OF_BLOCK] = 1
        blocks.append(block)
        if final or position == total_bits:
            break
    return Stream(bytes(out), blocks, position)


def length_symbol(length: int) -> int:
    """The literal/length symbol 257 .. 285 of a match length 3 .. 258 (RFC 1951 3.2.5)."""
    if length == 258:
        return 285
    return 257 + max(index for index in range(28) if LENGTH_BASE[index] <= length)


def distance_symbol_of(distance: int) -> int:
    return max(index for index in range(30) if DISTANCE_BASE[index] <= distance)


def ll_extra_bits(symbol: int) -> int:
    return LENGTH_EXTRA[symbol - 257] if symbol > 256 else 0


def data_bits(block: Block) -> int:
    """Σ histogram × (code length + extra bits) of a coded block, end-of-block included: what its tokens must take."""
    ll = sum(count * (block.ll_lengths[symbol] + ll_extra_bits(symbol)) for symbol, count in enumerate(block.ll_histogram) if count)
    return ll + sum(count * (block.d_lengths[symbol] + DISTANCE_EXTRA[symbol]) for symbol, count in enumerate(block.d_histogram) if count)


def kraft(lengths: Sequence[int], limit: int) -> int:
    """Σ 2^(limit − length) over the used symbols: 2^limit for a complete code."""
    return sum(1 << (limit - length) for length in lengths if length)


# ---- restatements of the code-building rules --------------------------------------------------------------------------
def huffman_depths(histogram: Sequence[int]) -> Dict[int, int]:
    """
    symbol -> depth in the unrestricted Huffman tree of the used symbols, by the two-queue construction over the symbols
    in ascending (count, symbol) order; of equal weights a leaf is taken before a merged node, which gives the tree of
    least depth among the optimal ones. Two used symbols or more.
    """
    leaves = sorted((count, symbol) for symbol, count in enumerate(histogram) if count > 0)
    if len(leaves) < 2:
        raise ValueError("two used symbols or more")
    weight = [count for count, _ in leaves]
    parent: List[int] = [-1] * len(leaves)
    merged: List[int] = []  # node numbers, in the order made: their weights ascend
    next_leaf, next_merged = 0, 0

    def smallest() -> int:
        nonlocal next_leaf, next_merged
        if next_leaf < len(leaves) and (next_merged >= len(merged) or weight[next_leaf] <= weight[merged[next_merged]]):
            next_leaf += 1
            return next_leaf - 1
        next_merged += 1
        return merged[next_merged - 1]

    for _ in range(len(leaves) - 1):
        first, second = smallest(), smallest()
        weight.append(weight[first] + weight[second])
        parent.append(-1)
        parent[first] = parent[second] = len(weight) - 1
        merged.append(len(weight) - 1)
    depth = [0] * len(weight)
    for node in range(len(weight) - 2, -1, -1):  # a parent has a larger number than its children
        depth[node] = depth[parent[node]] + 1
    return {symbol: depth[index] for index, (_, symbol) in enumerate(leaves)}


def cost(histogram: Sequence[int], lengths: Dict[int, int]) -> int:
    return sum(count * lengths[symbol] for symbol, count in enumerate(histogram) if count)


def huffman_depth_and_cost(histogram: Sequence[int]) -> Tuple[int, int]:
    """(deepest code, Σ count × depth) of the unrestricted Huffman code. The cost does not depend on how ties are broken."""
    depths = huffman_depths(histogram)
    return max(depths.values()), cost(histogram, depths)


def package_merge_cost(histogram: Sequence[int], limit: int) -> int:
    """Σ count × length of an optimal code with no length over `limit` (Larmore and Hirschberg's package-merge)."""
    leaves = sorted(count for count in histogram if count > 0)
    if len(leaves) < 2 or len(leaves) > 1 << limit:
        raise ValueError("2 .. 2^limit used symbols")
    # an item is (weight, the number of leaves of each rank it holds); the cheapest 2 n - 2 of the last level's items
    # give the lengths: a leaf's length is the number of chosen items that hold it. Only the count per rank is needed.
    items = [(weight, (rank,)) for rank, weight in enumerate(leaves)]
    level = list(items)
    for _ in range(limit - 1):
        packages = [(level[i][0] + level[i + 1][0], level[i][1] + level[i + 1][1]) for i in range(0, len(level) - 1, 2)]
        level = sorted(items + packages, key=lambda item: item[0])
    lengths = [0] * len(leaves)
    for _, ranks in level[: 2 * len(leaves) - 2]:
        for rank in ranks:
            lengths[rank] += 1
    assert sum(1 << (limit - length) for length in lengths) == 1 << limit and max(lengths) <= limit
    return sum(weight * length for weight, length in zip(leaves, lengths))


def limited_lengths(histogram: Sequence[int], limit: int) -> Dict[int, int]:
    """
    The project's length-limited code of the used symbols (two or more), as the headers state the rule: the Huffman
    depths; every code longer than `limit` moved to `limit`; then, until the Kraft sum is one again, the deepest code
    shorter than `limit` is lengthened by one bit and one code of `limit` bits becomes its brother; at last the lengths
    are handed out afresh, the shortest to the most frequent symbols, by descending (count, symbol).
    """
    depths = huffman_depths(histogram)
    per_length = [0] * (limit + 1)
    for depth in depths.values():
        per_length[min(depth, limit)] += 1
    excess = sum(number << (limit - length) for length, number in enumerate(per_length) if length) - (1 << limit)
    for _ in range(excess):  # each move takes 2^-limit off the sum
        length = max(candidate for candidate in range(1, limit) if per_length[candidate])
        per_length[length] -= 1
        per_length[length + 1] += 2
        per_length[limit] -= 1
    order = sorted(depths, key=lambda symbol: (-histogram[symbol], -symbol))
    handed = [length for length in range(1, limit + 1) for _ in range(per_length[length])]
    return dict(zip(order, handed))


def run_length_symbols(lengths: Sequence[int]) -> List[Tuple[int, int]]:
    """
    The (code-length symbol, extra value) sequence the match-search encoder sends for `lengths` (the literal/length
    lengths with the distance lengths behind them, runs crossing over): a run of equal lengths at a time. Zeros: 18 for
    138 at a time while 11 or more are left, 17 for 3 .. 10, fewer as themselves. Other lengths: the length once, 16 for
    6 at a time while 3 or more are left, fewer as themselves.
    """
    out: List[Tuple[int, int]] = []
    at = 0
    while at < len(lengths):
        value, run = lengths[at], 1
        while at + run < len(lengths) and lengths[at + run] == value:
            run += 1
        at += run
        if value == 0:
            while run >= 11:
                out.append((18, min(run, 138) - 11))
                run -= min(run, 138)
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((value, 0))
            run -= 1
            while run >= 3:
                out.append((16, min(run, 6) - 3))
                run -= min(run, 6)
        out += [(value, 0)] * run
    return out


def cl_histogram(symbols: Sequence[Tuple[int, int]]) -> List[int]:
    histogram = [0] * 19
    for symbol, _ in symbols:
        histogram[symbol] += 1
    return histogram
