"""
Per-layer kernel time and achieved TFLOP/s of the thirteen forward and thirteen backward gance::conv3x3 launches of one
`VGG16Lpips(convolution="conv3x3")` call, from the kernel trace of

    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d DIR -o lpips_conv3x3 --output-format csv -- \
        python tools/gpu_lpips_rate.py --measure distance --batch 1 --legs hip-conv3x3

    python tools/lpips_conv3x3_layers.py DIR/.../lpips_conv3x3_kernel_trace.csv [--stats ..._kernel_stats.csv]

The trace holds one pass over the target (13 launches) and then N forward + backward calls of 26 launches each, in the order
conv1_1 ... conv5_3, conv5_3 ... conv1_1; a launch is a conv3x3_kernel dispatch plus the conv3x3_finish_kernel that follows a
split form. The first two calls (the warm-up) are dropped; each of the 26 positions is reported by its median. FLOPs are
2 * 9 * cin * cout * side^2 of the layer's shape (conv1_1 counted with its 16 padded input channels, as it runs), and the
peak is 157.3 TFLOP/s (fp32 matrix cores). Writes profiles/lpips_conv3x3_layers.json and, with --stats, the per-kernel totals
profiles/lpips_conv3x3_kernel_stats.csv (microseconds). Needs no GPU.
"""

import argparse
import csv
import json
import statistics
import sys
from pathlib import Path
from typing import List

REPO_ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO_ROOT))
from gance_amd import hip_lib  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import lpips  # noqa: E402  pylint: disable=wrong-import-position

PEAK_TFLOPS = 157.3
SIDE = lpips.DEFAULT_SIDE
WARM_UP_CALLS = 2


def layer_shapes() -> List[dict]:
    """The 26 launches of one call in launch order."""
    forward, side = [], SIDE
    for index, (name, cin, cout) in enumerate(lpips.CONV_LAYERS):
        forward.append({"layer": name, "cin": max(cin, 16), "cout": cout, "side": side})
        if index in lpips.POOL_LAYERS:
            side //= 2
    backward = [{"layer": shape["layer"], "cin": shape["cout"], "cout": shape["cin"], "side": shape["side"]} for shape in reversed(forward)]
    return [dict(shape, direction="forward") for shape in forward] + [dict(shape, direction="backward") for shape in backward]


def launches(trace: Path) -> List[float]:
    """Microseconds of every conv3x3 launch (the finishing pass of a split form added to its main kernel), in start order."""
    with open(trace, newline="") as file:
        rows = [row for row in csv.DictReader(file) if "gance_conv3x3::" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    out: List[float] = []
    for row in rows:
        duration = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0
        if "conv3x3_finish_kernel" in row["Kernel_Name"]:
            out[-1] += duration
        else:
            out.append(duration)
    return out


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("trace", type=Path)
    parser.add_argument("--stats", type=Path, help="rocprofv3's ..._kernel_stats.csv of the same run")
    parser.add_argument("--out", type=Path, default=REPO_ROOT / "profiles" / "lpips_conv3x3_layers.json")
    parser.add_argument("--stats-out", type=Path, default=REPO_ROOT / "profiles" / "lpips_conv3x3_kernel_stats.csv")
    args = parser.parse_args()
    shapes = layer_shapes()
    times = launches(args.trace)
    per_call, target_pass = len(shapes), len(lpips.CONV_LAYERS)
    calls, rest = divmod(len(times) - target_pass, per_call)
    if rest != 0 or calls <= WARM_UP_CALLS:
        raise SystemExit(f"{len(times)} conv3x3 launches are not one target pass of {target_pass} and more than {WARM_UP_CALLS} calls of {per_call}")
    rows = []
    for position, shape in enumerate(shapes):
        samples = [times[target_pass + call * per_call + position] for call in range(WARM_UP_CALLS, calls)]
        microseconds = statistics.median(samples)
        flops = 2.0 * 9 * shape["cin"] * shape["cout"] * shape["side"] ** 2
        tflops = flops / microseconds / 1e6
        rows.append(dict(shape, form=hip_lib.conv3x3_form(shape["cin"], shape["cout"], shape["side"]), gflop=round(flops / 1e9, 3),
                         kernel_us=round(microseconds, 1), tflops=round(tflops, 1), of_peak=round(tflops / PEAK_TFLOPS, 3)))  # fmt: skip
    total_us = sum(row["kernel_us"] for row in rows)
    total_gflop = sum(row["gflop"] for row in rows)
    result = {
        "what": "gance::conv3x3 launches of one VGG16Lpips(convolution='conv3x3') forward + backward at side 256, one frame: median kernel time "
        f"over {calls - WARM_UP_CALLS} calls of one rocprofv3 --kernel-trace run (finishing pass of a split form included)",
        "peak_tflops": PEAK_TFLOPS,
        "launches": rows,
        "total": {"kernel_us": round(total_us, 1), "gflop": round(total_gflop, 2), "tflops": round(total_gflop / total_us * 1e3, 1)},
    }
    args.out.write_text(json.dumps(result, indent=1) + "\n")
    print("| launch | cin -> cout | side | form | GFLOP | kernel µs | TFLOP/s | of 157.3 |")
    print("|---|---|---|---|---|---|---|---|")
    for row in rows:
        print(f"| {row['layer']} {row['direction']} | {row['cin']} -> {row['cout']} | {row['side']} | {row['form']} | {row['gflop']} | {row['kernel_us']} | {row['tflops']} | {row['of_peak']:.1%} |")
    print(f"| all 26 | | | | {result['total']['gflop']} | {result['total']['kernel_us']} | {result['total']['tflops']} | {result['total']['tflops'] / PEAK_TFLOPS:.1%} |")
    if args.stats is not None:
        with open(args.stats, newline="") as file:
            stats = list(csv.DictReader(file))
        with open(args.stats_out, "w", newline="") as file:
            writer = csv.writer(file, lineterminator="\n")
            writer.writerow(["Name", "Calls", "TotalDurationUs", "AverageUs", "Percentage"])
            for row in stats:
                writer.writerow([row["Name"], row["Calls"], round(int(row["TotalDurationNs"]) / 1000), round(float(row["AverageNs"]) / 1000, 1), row["Percentage"]])


if __name__ == "__main__":
    main()
