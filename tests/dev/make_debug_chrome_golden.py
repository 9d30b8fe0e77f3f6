"""
Writes tests/golden/debug_chrome.npz: the chrome templates that tests/test_debug_video.py::test_chrome_matches_golden
compares against, drawn by gance_amd/debug_video (our own code; nothing else is involved).

    python tests/dev/make_debug_chrome_golden.py
"""

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from gance_amd.debug_video import chrome  # noqa: E402  pylint: disable=wrong-import-position


def golden_axes(side: int):
    """Fixed labels and limits: a titled axis with legend, grid and threshold over a small untitled one."""
    rectangles = chrome.stacked_rectangles(side, ((0, 3), (3, 4)), 4)
    return [
        chrome.AxisSpec(
            *rectangles[0][:4], (0.0, 23.0), (-5.0, 17.5), "Overlay Discriminator (Image Hashing)", rectangles[0][4],
            legend=(("Bounding Boxes", chrome.RED), ("Complete Image", chrome.BLUE)), grid=True, hlines=((10.0, chrome.PURPLE),),
        ),
        chrome.AxisSpec(*rectangles[1][:4], (0.0, 2.0), (0.0, 1.0), "network Index", rectangles[1][4]),
    ]


def main() -> None:
    out = Path(__file__).resolve().parents[1] / "golden" / "debug_chrome.npz"
    np.savez_compressed(out, **{f"side_{side}": chrome.render_chrome(side, golden_axes(side)) for side in (96, 400)})
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
