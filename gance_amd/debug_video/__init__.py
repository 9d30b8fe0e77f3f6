"""
The debug video of projection-file-blend without matplotlib: a bitmap font and numpy chrome templates on the host
(font.py, chrome.py), mark tables per window (panels.py), and the composer that places, draws and holds the frames in
HBM (compose.py; HIP kernels of gance_amd/csrc/debug_panels.hip).
"""
