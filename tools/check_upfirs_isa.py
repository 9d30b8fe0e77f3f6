"""Compile upfir_split.hip to ISA (no GPU needed) and check what the split-operand up kernels depend on but no parity test can see.

Per kernel (upfirs_fused{,_noise,_pre,_pre_noise}_kernel):
  * no scratch (a spill would be a vector-memory access inside the row loop, and would shift the hand count below);
  * the K loop's MFMAs all there: 1044 = 2 chunk parities x 522, a chunk being rows 0 ... 7 of the row loop (row 0: the three dy = -1 taps,
    rows 1 ... 7: all nine taps; 18 + 7 x 54 products of six terms) = 396, and its last row = 126: the six dy = 0 taps (36), the dy = -1 taps
    of position row y' = H (18, last step only) and the halo tile (9 taps x 6 terms = 54, one class per wave, all nine compiled in; + 18
    for its row y' = H);
  * the hand-counted wait `s_waitcnt vmcnt(24)` (the inline asm in run_chunk's row kTRows - 2): once per chunk parity. Nothing else orders
    the next chunk's weight LDS-DMA (weights_dma: seven `buffer_load_dwordx4 ... lds` per wave, the seventh behind a forward branch) before
    read_a3 reads its fragments, and vmcnt counts in issue order: on EVERY path from the last weight DMA to that wait exactly 24 more
    vector-memory instructions must issue. Fewer and the DMA may still be in flight when the wait passes (a stale-weight race that depends on
    timing); more and the wait drains loads it did not need to. The path must not cross a loop head (a label some later branch jumps back to).
The compiler's own `s_waitcnt vmcnt(24)` (eight more per kernel) are not the inline one: only a wait between ;;#ASMSTART / ;;#ASMEND counts.
The epilogue's noise DMA is an `... lds` load too; it lies after the K loop, outside every checked path.

`python tools/check_upfirs_isa.py [file.s]` checks an existing assembly file instead of compiling (to try a hand edit of the ISA).
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

KERNELS = ("upfirs_fused_kernel", "upfirs_fused_noise_kernel", "upfirs_fused_pre_kernel", "upfirs_fused_pre_noise_kernel")
MFMAS = 1044
WAIT_COUNT = 24
WEIGHT_DMAS = 7  # per chunk parity: ceil(27 fragment units / 4 waves)

VMEM = re.compile(r"^\s*(buffer_|global_|flat_|scratch_)")
LDS_DMA = re.compile(r"^\s*buffer_load_dwordx4\b.*\blds\b")
LABEL = re.compile(r"^(\.LBB\w+):")
BRANCH = re.compile(r"^\s*(s_branch|s_cbranch_\w+)\s+(\.LBB\w+)")


def inline_waits(lines: list) -> list:
    """Indices of `s_waitcnt vmcnt(24)` lines written by inline asm (the line before is ;;#ASMSTART)."""
    return [i for i, line in enumerate(lines) if line.strip() == f"s_waitcnt vmcnt({WAIT_COUNT})" and i > 0 and lines[i - 1].strip() == ";;#ASMSTART"]


def path_counts(lines: list, first: int, last: int, labels: dict) -> set:
    """Vector-memory instructions issued after line `first` and before line `last`, over every path that reaches `last`
    (forward branches only; a backward branch or one that leaves the range raises / drops the path)."""
    counts = set()
    stack = [(first + 1, 0)]
    while stack:
        i, n = stack.pop()
        while i < last:
            line = lines[i]
            if VMEM.match(line):
                n += 1
            branch = BRANCH.match(line)
            if branch:
                target = labels[branch.group(2)]
                if target <= i:
                    raise AssertionError(f"backward branch at line {i} between the weight DMA and the wait")
                if target <= last:
                    if branch.group(1) == "s_branch":
                        i = target
                        continue
                    stack.append((target, n))
                elif branch.group(1) == "s_branch":
                    break  # (leaves the range: this path does not reach the wait)
            if line.strip().startswith(("s_endpgm", "s_setpc")):
                break
            i += 1
        else:
            counts.add(n)
    return counts


def check_kernel(text: str, name: str) -> list:
    """Problems found in kernel `name` (empty: all checks hold); prints one summary line."""
    start = text.index(f"_ZN5gance{len(name)}{name}ENS_9UpFirArgsE:")
    end = text.index(".Lfunc_end", start)
    meta = text[end:end + 6000]
    lines = text[start:end].split("\n")
    problems = []
    scratch = int(re.search(r"; ScratchSize: (\d+)", meta).group(1))
    mfmas = sum(1 for line in lines if re.match(r"^\s+v_mfma_f32_16x16x32_bf16", line))
    if scratch != 0:
        problems.append(f"scratch {scratch} B")
    if mfmas != MFMAS:
        problems.append(f"{mfmas} MFMAs, want {MFMAS}")
    labels = {m.group(1): i for i, line in enumerate(lines) for m in [LABEL.match(line)] if m}
    loop_heads = {labels[m.group(2)] for i, line in enumerate(lines) for m in [BRANCH.match(line)] if m and labels[m.group(2)] <= i}
    waits = inline_waits(lines)
    if len(waits) != 2:
        problems.append(f"{len(waits)} inline vmcnt({WAIT_COUNT}) waits, want 2 (one per chunk parity)")
    found = []
    previous = 0
    for w in waits:
        dmas = [i for i in range(previous, w) if LDS_DMA.match(lines[i])]
        previous = w
        if len(dmas) != WEIGHT_DMAS:
            problems.append(f"{len(dmas)} weight LDS-DMAs before the wait at line {w}, want {WEIGHT_DMAS}")
            continue
        if any(dmas[0] < head <= w for head in loop_heads):
            problems.append(f"a loop head lies between the weight DMA at line {dmas[0]} and the wait at line {w}")
            continue
        try:
            counts = path_counts(lines, dmas[-1], w, labels)
        except AssertionError as error:
            problems.append(str(error))
            continue
        found.append(sorted(counts))
        if counts != {WAIT_COUNT}:
            problems.append(f"vector-memory instructions between the last weight DMA and the wait at line {w}: {sorted(counts)} over its paths, want {WAIT_COUNT}")
    print(f"{name:32s} scratch {scratch} B  MFMAs {mfmas}  inline waits {len(waits)}  vector-memory ops from the last weight DMA to each: {found}"
          + ("" if not problems else "  FAIL: " + "; ".join(problems)))
    return problems


def main() -> int:
    if len(sys.argv) > 1:
        text = Path(sys.argv[1]).read_text()
    else:
        src = Path(__file__).resolve().parent.parent / "gance_amd" / "csrc" / "upfir_split.hip"
        with tempfile.NamedTemporaryFile(suffix=".s") as out:
            subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "--cuda-device-only", "-S", str(src), "-o", out.name],
                           check=True, cwd=src.parent, stderr=subprocess.DEVNULL)
            text = Path(out.name).read_text()
    bad = False
    for name in KERNELS:
        bad |= bool(check_kernel(text, name))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
