"""tree_pins.json: SHA-256 digests of what the walks of nbd.tree and the two tree simulators compute on the MI355X for
the cases of tests/test_tree_pins_gpu.py. The inputs, the cases and the digest are that module's; this script only
records them.

Run once on the GPU, against a library built from the commit the bits are to be pinned to: the C-ABI is what carries the
bits, so a build of that commit's csrc/, named by NBD_LIB_OVERRIDE, is driven by this tree's Python.

    NBD_LIB_OVERRIDE=/path/to/that/libnbd_hip.so python tests/golden/make_tree_pins.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "nbody-deep-sim_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_tree_pins_gpu as pins  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else pins.FIXTURE
    digests = {pins.key(*case): pins.walk_digests(*case) for case in pins.CASES}
    digests["leapfrog"] = pins.leapfrog_digests()
    digests["block"] = pins.block_digests()
    with open(out, "w") as f:
        json.dump({"digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    from nbd import _lib
    print(out, len(digests), "cases, library", _lib.LIB_PATH)
