"""
Which kernel form every conv layer runs in, by batch size: the engine's own decisions (engine.hip: plan_call, which asks
conv_form_of / up_runs_fused / plan_layer once per layer), read back from the launch names of real calls at every batch
size 1 ... max_batch.
    python tools/gpu_form_table.py [resolution] [max_batch] > profiles/form_table.txt
Legend: conv<N> direct form, convW F(2x2,3x3), convV F(4x4,3x3), +rgb ToRGB channel sum in the epilogue, +torgb fused ToRGB +
uint8; convT two-pass up layer (+ fir pass), convTF / convTFp one fused up kernel (p: input pre-scaled by its style; /16: the
16-channel two-blocks-per-CU geometry); (xK): split-K factor K of a direct-form launch is not in the name -- see `finish` rows.

--conv-form / --up-form (comma-separated lists: one engine per combination, one after the other) and --batches choose what
runs; the table printed is that of the last combination. --trace FILE also writes, per combination and batch size, every step
name of the call and a sha256 of the returned uint8 frames (weights from make_random_variables(perturb=True), so that noise
and bias terms are live): two libraries (GANCE_HIP_LIBRARY) that plan and compute the same give identical files.
--fmap-base 8192 traces a config-e generator (profiles/launch_plan_config_e_256cus.txt, held by tests/test_config_e_plan.py).
--compact TRACE... needs no GPU: it prints the traces' names from `styles` on (a gance_synthesize_w call; the nine launches
of the mapping network in front are the same in every call) in the run-length form of profiles/launch_plan_256cus.txt, which
tests/test_engine_plan.py holds gance_engine_describe_plan to.
"""
import argparse
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

parser = argparse.ArgumentParser(description=__doc__.split("\n\n", maxsplit=1)[0])
parser.add_argument("resolution", nargs="?", type=int, default=1024)
parser.add_argument("max_batch", nargs="?", type=int, default=64)
parser.add_argument("--conv-form", default="auto", help="auto, direct, winograd, winograd43; or a comma-separated list")
parser.add_argument("--up-form", default="auto", help="auto, split, fused; or a comma-separated list")
parser.add_argument("--batches", default=None, help="comma-separated frames per call (default: 1 ... max_batch)")
parser.add_argument("--fmap-base", type=int, default=16 << 10, help="16384: a config-f generator (default); 8192: a config-e one")
parser.add_argument("--trace", default=None, help="append step names and frame hashes of every call to this file")
parser.add_argument("--compact", nargs="+", default=None, help="trace files to print in run-length form (no GPU)")
options = parser.parse_args()


def runs_of(values: dict) -> list:
    """[(first batch, last batch, value)]: the runs of consecutive batch sizes with the same value."""
    runs = []
    for batch, value in sorted(values.items()):
        if runs and runs[-1][2] == value and runs[-1][1] == batch - 1:
            runs[-1][1] = batch
        else:
            runs.append([batch, batch, value])
    return [tuple(run) for run in runs]


def compact(paths: list) -> None:
    names, sequences, sections = {}, {}, []
    for path in paths:
        for line in Path(path).read_text().splitlines():
            if line.startswith("config "):
                sections.append((line[len("config "):], {}))
            elif line.startswith("B "):
                _, batch, _, *steps = line.split()
                steps = tuple(names.setdefault(step, len(names) + 1) for step in steps[steps.index("styles"):])
                sections[-1][1][int(batch)] = sequences.setdefault(steps, f"S{len(sequences) + 1}")
    print("# launch names of a gance_synthesize_w call by configuration and frames per call, 256 CUs; from tools/gpu_form_table.py --trace / --compact")
    print("# N<k> name: a launch name; S<n>: a distinct sequence of them, by k, in launch order;")
    print("# [resolution max_batch conv_form up_form knob]: a configuration (knob: GANCE_TUNE_<knob>, - for none); B a-b: S<n>: the sequence of a to b frames per call")
    for name, number in names.items():
        print(f"N{number} {name}")
    for steps, tag in sequences.items():
        print(f"{tag}: " + " ".join(str(step) for step in steps))
    for header, by_batch in sections:
        print(f"[{header}]")
        for first, last, tag in runs_of(by_batch):
            print(f"B {first}" + (f"-{last}" if last > first else "") + f": {tag}")


if options.compact:
    compact(options.compact)
    sys.exit(0)

from gance_amd import hip_lib  # noqa: E402
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402

resolution, max_batch = options.resolution, options.max_batch
batches = [int(b) for b in options.batches.split(",")] if options.batches else list(range(1, max_batch + 1))
variables = sg2_spec.make_random_variables(resolution, seed=0, perturb=options.trace is not None, fmap_base=options.fmap_base)
knobs = ",".join(f"{k[len('GANCE_TUNE_'):]}={v}" for k, v in sorted(os.environ.items()) if k.startswith("GANCE_TUNE_")) or "-"
for conv_form in options.conv_form.split(","):
    for up_form in options.up_form.split(","):
        engine = hip_lib.Engine(variables, resolution, max_batch=max_batch, profile=True, conv_form=conv_form, up_form=up_form)
        rng = np.random.RandomState(0)
        table = {}  # layer tag -> list of form per batch
        order = []
        trace = [f"config {resolution} {max_batch} {conv_form} {up_form} {knobs}"]
        for batch in batches:
            frames = engine.synthesize_z(rng.randn(batch, 512).astype(np.float32))
            trace.append(f"B {batch} {hashlib.sha256(frames.tobytes()).hexdigest()} " + " ".join(step.name for step in engine.steps()))
            seen = {}
            for step in engine.steps():
                if not step.name.startswith("conv"):
                    continue
                kind, _, rest = step.name.partition("_")
                digits = "".join(ch for ch in kind if ch.isdigit())
                tag = f"{int(digits):2d} {rest.split('/')[0]}"  # (the name's "/16" / "/16x" suffix goes into the form)
                form = kind.replace(digits, "", 1) + ("/" + step.name.rsplit("/", 1)[1] if "/" in step.name else "")  # (/16, /16x, /s3)
                seen[tag] = form
                if tag not in table:
                    table[tag] = {}
                    order.append(tag)
            finishes = {s.name.split("_")[0].replace("finish", "") for s in engine.steps() if s.name.startswith("finish")}
            for tag, form in seen.items():
                layer = tag.split()[0]
                table[tag][batch] = form + (" +finish (split-K)" if layer in finishes else "")
        engine.close()
        if options.trace:
            with open(options.trace, "a", encoding="utf-8") as out:
                out.write("\n".join(trace) + "\n")
print(f"kernel form of every conv layer of the {resolution}x{resolution} generator by frames per engine call (1 ... {max_batch}); from tools/gpu_form_table.py")
for tag in order:
    print(f"  {tag:32s} " + " | ".join(f"B {first}" + (f"-{last}" if last > first else "") + f": {form}" for first, last, form in runs_of(table[tag])))
