"""
Rate of a config-e generator (fmap_base = 8 << 10) at 1024^2 on one GPU, beside the config-f one in the same process
(`python tools/gpu_config_e_rate.py [--out profiles/config_e_rate_1024.json]`):

1. frames/s of both random-init networks (seed 0: the networks bench.py times) at 1, 4, 16 and 64 frames per call, z vectors
   resident in HBM -> mapping -> truncation -> synthesis -> uint8 frames in HBM (Engine.synthesize_z_device), device events over
   >= 0.5 s of calls per leg. Every leg is warmed up first; then three rounds, config-e and config-f alternated inside each
   round, and the medians over the rounds (every round's figures are kept).
2. the two launches of the 16-channel layers at 64 frames per call, bracketed by HIP events (profiling on, three calls, median):
   the 32 -> 16 up layer and the frame-emitting 16 -> 16 conv, with the bytes and flops the engine books for them and the
   resulting fractions of the 6.3 TB/s copy rate and the 155 TFLOP/s fp32-MFMA rate (the measured rates of the microarchitecture guide).
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from gance_amd import hip_lib  # noqa: E402  pylint: disable=wrong-import-position
from gance_amd.stylegan2 import spec as sg2_spec  # noqa: E402  pylint: disable=wrong-import-position

RESOLUTION, MAX_BATCH, PSI = 1024, 64, 1.2
BATCHES = (1, 4, 16, 64)
ROUNDS, LEG_MS = 3, 500.0
COPY_RATE_BYTES, FP32_MFMA_RATE_FLOPS = 6.3e12, 155e12
LAUNCHES = ("convTF15_1024x1024_32->16/16", "conv16+torgb_1024x1024_16->16")


def leg(engine, z: torch.Tensor, out: torch.Tensor, batch: int, min_ms: float) -> float:
    """frames/s of calls of `batch` frames over at least `min_ms` of device time."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream().cuda_stream
    calls_per_span = max(1, 64 // batch)
    calls, elapsed_ms = 0, 0.0
    while elapsed_ms < min_ms:
        start.record()
        for _ in range(calls_per_span):
            engine.synthesize_z_device(z.data_ptr(), batch, PSI, out.data_ptr(), 0, stream)
        end.record()
        torch.cuda.synchronize()
        calls += calls_per_span
        elapsed_ms += start.elapsed_time(end)
    return calls * batch / (elapsed_ms / 1e3)


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n", maxsplit=1)[0])
    parser.add_argument("--out", default=None, help="write the JSON here as well as to stdout")
    options = parser.parse_args()
    device = torch.device("cuda", 0)
    z = torch.from_numpy(np.random.RandomState(0).randn(MAX_BATCH, 512).astype(np.float32)).to(device)
    out = torch.empty((MAX_BATCH, RESOLUTION, RESOLUTION, 3), dtype=torch.uint8, device=device)
    engines = {
        name: hip_lib.Engine(sg2_spec.make_random_variables(RESOLUTION, seed=0, fmap_base=fmap_base), RESOLUTION, max_batch=MAX_BATCH, device=0)
        for name, fmap_base in (("config_e", 8 << 10), ("config_f", 16 << 10))
    }
    result: dict = {"resolution": RESOLUTION, "device": torch.cuda.get_device_name(0), "compute_units": torch.cuda.get_device_properties(0).multi_processor_count}
    try:
        for batch in BATCHES:  # warm-up of every leg
            for engine in engines.values():
                leg(engine, z, out, batch, 50.0)
        rounds = {name: {batch: [] for batch in BATCHES} for name in engines}
        for _ in range(ROUNDS):
            for batch in BATCHES:
                for name, engine in engines.items():
                    rounds[name][batch].append(leg(engine, z, out, batch, LEG_MS))
        result["frames_per_s"] = {name: {str(batch): statistics.median(values) for batch, values in by_batch.items()} for name, by_batch in rounds.items()}
        result["frames_per_s_rounds"] = {name: {str(batch): values for batch, values in by_batch.items()} for name, by_batch in rounds.items()}

        engine = engines["config_e"]
        engine.set_profiling(True)
        stream = torch.cuda.current_stream().cuda_stream
        samples: dict = {name: [] for name in LAUNCHES}
        booked: dict = {}
        call_ms = []
        for _ in range(3):
            engine.synthesize_z_device(z.data_ptr(), MAX_BATCH, PSI, out.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            steps = engine.steps()
            call_ms.append(sum(step.ms for step in steps))
            for step in steps:
                if step.name in samples:
                    samples[step.name].append(step.ms)
                    booked[step.name] = (step.flops, step.bytes)
        engine.set_profiling(False)
        launches = {}
        for name in LAUNCHES:
            ms = statistics.median(samples[name])
            flops, nbytes = booked[name]
            launches[name] = {
                "frames_per_call": MAX_BATCH, "ms": ms, "us_per_frame": ms * 1e3 / MAX_BATCH, "flops": flops, "bytes": nbytes,
                "tflops": flops / ms / 1e9, "tbytes_per_s": nbytes / ms / 1e9,
                "fraction_of_155_tflops": flops / (ms / 1e3) / FP32_MFMA_RATE_FLOPS,
                "fraction_of_6p3_tbytes_per_s": nbytes / (ms / 1e3) / COPY_RATE_BYTES,
            }
        result["launches_at_64_frames_per_call"] = launches
        result["profiled_call_ms_sum_of_launches"] = statistics.median(call_ms)
    finally:
        for engine in engines.values():
            engine.close()
    text = json.dumps(result, indent=1)
    print(text)
    if options.out:
        Path(options.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
