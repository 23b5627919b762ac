"""Record the result bits of the step and pack kernels: every case of tests/step_bits_support.py on cuda:0 -> SHA-256 digests as JSON
(tests/golden/step_bits.json is such a file; tests/test_step_bits_gpu.py compares with it).  IDMVTON_HIP_LIB selects the library: the
recording is made once, from a build of the commit whose bits are to be kept.

    IDMVTON_HIP_LIB=<that build>/libidmvton_hip.so python tools/gpu_step_bits.py --source "<the commit>" --out step_bits.json
    python tools/gpu_step_bits.py --check tests/golden/step_bits.json       compare the in-tree library with a recording (exit status 1 on a difference)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--source", default="", help="the commit the selected library was built from (stored in the file)")
ap.add_argument("--check", default=None)
args = ap.parse_args()

import idm_vton_amd  # noqa: E402,F401
from tests.step_bits_support import CASES, digests, run  # noqa: E402

got = {name: digests(run(name, "cuda")) for name in CASES}
print("library:", os.environ.get("IDMVTON_HIP_LIB", "(in-tree)"), "--", len(got), "cases")
if args.out:
    with open(args.out, "w") as f:
        json.dump({"source": args.source, "cases": got}, f, indent=0, sort_keys=True)
        f.write("\n")
if args.check:
    with open(args.check) as f:
        want = json.load(f)["cases"]
    bad = [name for name in CASES if got[name] != want.get(name)]
    print("differ:", bad if bad else "none")
    sys.exit(1 if bad else 0)
