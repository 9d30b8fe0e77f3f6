"""
bench.py's host-side bookkeeping (no GPU): how a launch of the engine's step table maps to a kernel and to the flops
the matrix cores execute, and that the committed traffic record answers for the launches that can be dominant. On the GPU:
what a plain run and a --full run print.
"""
import importlib.util
import json
from pathlib import Path

import pytest

REPO_ROOT = Path(__file__).resolve().parent.parent


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", REPO_ROOT / "bench.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_step_names_map_to_kernels_and_executed_flops() -> None:
    bench = _bench_module()
    assert bench.kernel_of_step("convTF15_1024x1024_64->32") == "upfir_fused_kernel"
    assert bench.kernel_of_step("convTFp15_1024x1024_64->32") == "upfir_fused_pre_kernel"
    assert bench.kernel_of_step("convTFp15_1024x1024_64->32/16") == "upfir16_fused_pre_kernel"
    assert bench.kernel_of_step("convTFp15_1024x1024_64->32/16x") == "upfir16x_fused_pre_kernel"
    assert bench.kernel_of_step("convTFp7_64x64_512->512/16x") == "upfir16x_fused_w32_pre_kernel"
    assert bench.kernel_of_step("convTFp7_64x64_512->512/16") == "upfir16_fused_w32_pre_kernel"
    assert bench.kernel_of_step("convTF5_32x32_512->512/16") == "upfir16_fused_w16_kernel"
    assert bench.kernel_of_step("convTG3_16x16_512->512") == "tile_gemm_kernel"
    assert bench.kernel_of_step("convVG4_16x16_512->512") == "tile_gemm_kernel"
    assert bench.executed_fraction("convVG4_16x16_512->512") == 0.25
    assert abs(bench.executed_fraction("convTFp15_1024x1024_64->32/16x") - 15 / 18) < 1e-12
    assert bench.kernel_of_step("convW16+rgb_1024x1024_32->32") == "winograd64_c32_rgb_kernel"
    assert bench.kernel_of_step("convW8+rgb_64x64_512->512") == "winograd64_rgb_kernel"
    assert bench.kernel_of_step("convW14_512x512_64->64") == "winograd64_kernel"
    assert bench.kernel_of_step("conv16+torgb_1024x1024_32->32") == "modconv_mfma_kernel"
    # Winograd F(2x2, 3x3): 16 multiplies per 2x2 tile and input channel instead of 36
    assert abs(bench.executed_fraction("convW8+rgb_64x64_512->512") - 16.0 / 36.0) < 1e-12
    assert bench.executed_fraction("convTF9_128x128_512->256") == 1.0
    # Winograd F(4x4, 3x3): 36 multiplies per 4x4 tile and input channel instead of 144
    assert bench.kernel_of_step("convV8+rgb_64x64_512->512") == "winograd43_rgb_kernel" and bench.executed_fraction("convV8+rgb_64x64_512->512") == 0.25
    assert bench.executed_fraction("conv4_16x16_512->512") == 1.0
    # the split-operand form of the fused up kernel: six bf16 part products per fp32 product, priced against the bf16 matrix peak
    name = "convTFp15_1024x1024_64->32/s3"
    assert bench.kernel_of_step(name) == "upfirs_fused_pre_kernel" and bench.kernel_of_step("convTF9_128x128_512->256/s3") == "upfirs_fused_kernel"
    assert bench.executed_fraction(name) == 6.0 and bench.matrix_peak(name) == bench.BF16_MFMA_PEAK_TFLOPS
    assert bench.matrix_peak("convTFp15_1024x1024_64->32/16x") == bench.FP32_MFMA_PEAK_TFLOPS
    # even at the fp32 pipe's whole algorithmic rate (157.3 TFLOP/s of direct-form flops) the split form is well under its own roof
    assert 6.0 * bench.FP32_MFMA_PEAK_TFLOPS / bench.BF16_MFMA_PEAK_TFLOPS < 0.4


def test_traffic_record_covers_the_dominant_launches_of_the_default_workload() -> None:
    """
    profiles/traffic_latest.json is written by tools/make_traffic_record.py from the round's --pmc passes: it must hold the
    two launches that trade the "dominant kernel" place (the fused up kernel and the Winograd conv at 1024x1024), bench.py
    must find them by step name (both names of the fused up kernel), and the recorded HBM traffic must stay near the
    algorithmic bytes (tensors read once, written once) -- a kernel that re-reads shows up here first.
    """
    bench = _bench_module()
    record = json.loads((REPO_ROOT / "profiles" / "traffic_latest.json").read_text())
    workload = record["workload"]
    assert any(key.startswith("convTF15_1024x1024") for key in record["launches"])
    assert any(key.startswith(("convV16+rgb_1024x1024", "convW16+rgb_1024x1024")) for key in record["launches"])
    for key in record["launches"]:
        steps = [key + "_64->32"] + ([key.replace("convTF", "convTFp", 1) + "_64->32"] if key.startswith("convTF") else [])
        for step in steps:
            measured, note = bench.measured_traffic(step, workload["resolution"], workload["frames_per_step_per_gpu"])
            assert measured is not None and measured > 0 and "profiles/" in note
    for key, entry in record["launches"].items():
        ratio = entry["hbm_bytes_per_launch"] / entry["algorithmic_bytes_per_launch"]
        # the 512^2 / 1024^2 launches -- where HBM traffic is a third of the roof -- move little more than the algorithmic bytes;
        # the deep-K F(4x4,3x3) launches re-stream their transformed weights (36/9 x the 3x3 ones) once per pixel tile and every
        # patch once per 32-channel tile: x5.7 at 64^2, 1.7 TB/s, far from binding
        # (the 16 -> 32 up layer in one launch since round 4: 2 048 blocks of 16 channels re-stream the layer's 9.4 MB of weights once per
        # group of samples and every sample's whole input once per channel tile: x8.2 of its 177 MB, 1.5 TB/s for 0.96 ms)
        assert 1.0 <= ratio < (1.5 if key.endswith(("512x512", "1024x1024")) else 10.0), (key, ratio)  # (x1.38 at 1024^2: 18 x 72 patches per 16 x 64 tile, two partial images)
        # (the split-operand up launches keep the bf16 matrix cores busy 0.27 ... 0.46 of the launch: six 16-cycle products per fp32 product,
        # the rest is the wave's own staging and FIR)
        assert 0.2 < entry["mfma_busy_fraction"] < 1.0
    # another workload: no figure rather than a wrong one
    assert bench.measured_traffic("convV16+rgb_1024x1024_32->32", 512, workload["frames_per_step_per_gpu"])[0] is None


def test_metric_labels_of_the_sharded_product_stream_measurements() -> None:
    """`bench.sharded`: the N-GPU forms of the configs[2] / [3] / [4] labels name the GPU count and drop the one-GPU wording."""
    bench = _bench_module()
    assert bench.sharded(bench.METRIC_CONFIG_3, 1) == bench.METRIC_CONFIG_3
    for label in (bench.METRIC_CONFIG_2, bench.METRIC_CONFIG_3, bench.METRIC_CONFIG_4, bench.METRIC_CONFIG_4_OVERLAY):
        text = bench.sharded(label, 8)
        assert text.endswith("frame-sharded over 8 GPUs") and "ONE GPU" not in text and "on one GPU" not in text
    assert "2160" in bench.sharded(bench.METRIC_CONFIG_3, 8)


def test_dump_outputs_writes_float_arrays_of_the_step_within_the_budget(tmp_path) -> None:
    """`--dump-outputs`: float32 / float64 .npy files only, the same files for the same frames, the values where the index says."""
    import numpy as np  # pylint: disable=import-outside-toplevel
    import torch  # pylint: disable=import-outside-toplevel

    bench = _bench_module()
    frames = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(3, 16, 16, 3)).astype(np.uint8))
    record = bench.dump_outputs(tmp_path / "a", frames)
    bench.dump_outputs(tmp_path / "b", frames)
    assert record["frames_shape"] == [3, 16, 16, 3] and sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(record["files"])
    for name in record["files"]:
        first, second = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert first.dtype in (np.float32, np.float64) and np.array_equal(first, second)
    flat = frames.numpy().reshape(-1)
    index = np.load(tmp_path / "a" / "frames_sample_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "frames_sample.npy"), flat[index].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "frame_last.npy"), frames.numpy()[-1].astype(np.float32))
    # the default workload (64 frames of 1024 x 1024 x 3): two float32 frames + the sample and its float64 positions
    assert 2 * 1024 * 1024 * 3 * 4 + bench.DUMP_SAMPLE_SIZE * (4 + 8) <= 64 * 2**20


def _bench_line(*arguments: str) -> dict:
    import subprocess  # pylint: disable=import-outside-toplevel
    import sys  # pylint: disable=import-outside-toplevel

    result = subprocess.run(
        [sys.executable, str(REPO_ROOT / "bench.py"), *arguments], capture_output=True, text=True, cwd=REPO_ROOT, timeout=300, check=False
    )
    assert result.returncode == 0, result.stderr[-2000:]
    return json.loads(result.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_full_adds_the_launch_table() -> None:
    """
    A plain run is set-up, warm-up, the timed steps and the line: no cpu_baseline, no extras, no all-conv figures. Its dtype
    comes from the launch names of the last warm-up step; a --full run takes them from its extra, untimed step.
    """
    plain = _bench_line("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "16")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["higher_is_better"] is True and plain["unit"] == "frames/s" and plain["ms_per_step"] > 0
    assert abs(plain["value"] - 16 * 1e3 / plain["ms_per_step"]) < 1e-3 * plain["value"]
    assert "cpu_baseline" not in plain and "extras" not in plain
    assert "all_conv_launches" not in plain["roofline"] and "whole_path_frac" not in plain["roofline"]
    assert plain["roofline"]["launches_averaged"] >= 2
    full = _bench_line("--gpus", "1", "--steps", "1", "--warmup", "1", "--batch", "16", "--full", "--no-cpu-baseline", "--no-extras")
    assert full["dtype"] == plain["dtype"]
    assert full["roofline"]["all_conv_launches"]["winograd_launches"] > 0 and full["roofline"]["whole_path_frac"] > 0
