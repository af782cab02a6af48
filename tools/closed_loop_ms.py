"""usage (GPU box): python tools/closed_loop_ms.py [--device-register] [--device-reference] [--reref N]   -- the closed-loop point of
bench.py --extras alone: ms per cycle / tracking / mapping.  --device-register: the registration as one kernel launch
(esvo_track_solve, on_device).  --reref N: re-reference to the fused map every N ticks (default: never; 1 is what a tracking
node does, the mapper publishes its cloud after every tick).  --device-reference: the re-reference takes the cloud from the
device-resident map (esvo_map_cloud_build + esvo_track_set_reference_from_cloud) instead of downloading and re-uploading it.
--json FILE: the figures appended to FILE as one JSON line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from esvo_amd import closed_loop as cl  # noqa: E402

device_register = "--device-register" in sys.argv[1:]
device_reference = "--device-reference" in sys.argv[1:]
reref = int(sys.argv[sys.argv.index("--reref") + 1]) if "--reref" in sys.argv[1:] else 10**9
r = cl.run(n_ticks=15, reref=reref, device_register=device_register, device_reference=device_reference)
med = lambda v: float(np.median(np.asarray(v[3:])))  # noqa: E731
print(("device-register " if device_register else "") + ("device-reference " if device_reference else "") + ("reref %d " % reref if reref < 10**9 else "") + "cycle %.3f ms  tracking %.3f ms  mapping %.3f ms  end error %.2f mm of %.1f mm  max rot err %.3f deg  points/cycle %d" % (
    med(r["cycle_ms"]), med(r["track_ms"]), med(r["map_ms"]), r["pos_err"][-1] * 1e3, r["gt_len"][-1] * 1e3, max(r["rot_err_deg"]),
    int(np.median(r["points"]))))
if "--json" in sys.argv[1:]:
    import json
    with open(sys.argv[sys.argv.index("--json") + 1], "a") as f:
        f.write(json.dumps({"bench": "closed_loop_ms", "reref": reref if reref < 10**9 else None, "device_reference": device_reference,
                            "device_register": device_register, "cycle_ms": round(med(r["cycle_ms"]), 4),
                            "tracking_ms": round(med(r["track_ms"]), 4), "tracking_ms_worst": round(max(r["track_ms"][3:]), 4),
                            "mapping_ms": round(med(r["map_ms"]), 4), "end_error_mm": round(r["pos_err"][-1] * 1e3, 3),
                            "map_cells": r["map_cells"]}) + "\n")
print("tracking ms per cycle:", " ".join("%.2f" % v for v in r["track_ms"]))
