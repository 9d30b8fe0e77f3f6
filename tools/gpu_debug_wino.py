"""Dev check: a Winograd conv form against the direct form, same engine inputs (fp32 image and uint8 frames).

    python tools/gpu_debug_wino.py [winograd|winograd43|auto]     (conv_form of hip_lib.Engine; default winograd43)
"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np

from gance_amd import hip_lib
from gance_amd.stylegan2 import spec

form = sys.argv[1] if len(sys.argv) > 1 else "winograd43"
variables = spec.make_random_variables(1024, seed=0, perturb=True)
z = np.random.RandomState(1).randn(4, 512).astype(np.float32)
frames = {}
for conv_form in ("direct", form):
    engine = hip_lib.Engine(variables, 1024, max_batch=4, device=0, conv_form=conv_form)
    u8, f32 = engine.synthesize_z(z, want_float=True)
    frames[conv_form] = (np.array(u8), np.array(f32))
    engine.close()
(ua, a), (ub, b) = frames["direct"], frames[form]
print("image range", a.min(), a.max(), f"max abs diff direct vs {form}", np.abs(a - b).max(), "rms", np.sqrt(np.mean((a - b) ** 2)))
print("u8 differing", int((ua != ub).sum()), "of", ua.size, "max", int(np.abs(ua.astype(int) - ub.astype(int)).max()))
