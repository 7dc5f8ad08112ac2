#!/usr/bin/env python3
"""One round of the guard set of DESIGN.md 3.2 item 23 with bench.py's own functions, under the library DIRAL_LIB names:
the one-slot kernels that share the new text with the metric's instantiation (the policy epilogue, a sticky policy's keyed
quads, float64 outputs) and the slot loops.  One JSON line; the caller alternates the parent's library and this one.
   DIRAL_LIB=... python profiles/valu_diet/guard.py [--slots]      (--slots: the K-slot lines too)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402

import bench  # noqa: E402

dev = torch.device("cuda:0")
out = {"rollout_sps_fused_us": bench.rollout_sps_fused(dev)["ms_per_slot"] * 1e3}
_, r = bench.run_workload("c2", dev, 0, 1, 300, 10, 0, "f32", "my_step", True, 0.9, False)
out["c2_sticky_0.9_kernel_us"] = r["kernel_ms"] * 1e3
_, r = bench.run_workload("c2", dev, 0, 1, 300, 10, 0, "f64", "my_step", True, 0.0, False)
out["c2_f64_kernel_us"] = r["kernel_ms"] * 1e3
if "--slots" in sys.argv:
    out["rollout_sps_kslots_us"] = bench.rollout_sps_kslots(dev)["ms_per_slot"] * 1e3
print(json.dumps(out))
