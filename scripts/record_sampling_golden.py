"""Record tests/golden/sampling_draws.json: the ids (and, through the filtered entry point,
the ``stats``) that the device sampler draws for the cases of tests/test_sampling_golden.py.

The fixture pins the sampler across changes of its source, so it is recorded with the
kernel library of the commit to compare against and never with the tree under test:

    NSA_KERNEL_LIB=<that commit's libnsa_kernels.so> python scripts/record_sampling_golden.py [--out PATH]

Every case is checked (its rows reach the intended kernel path, a kept set of several ids
shows several drawn ids) before anything is written.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_sampling_golden as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=G.GOLDEN)
    a = ap.parse_args()
    from nanosandbox_amd.ops import _lib
    print(f"kernel library: {_lib.LIB_PATH}", flush=True)
    cases = {}
    for name in G.CASE_IDS:
        cases[name] = G.draw(name)
        paths = G.check_case(name, cases[name]["ids"])
        distinct = {i for form in cases[name]["ids"] for ids in form for i in ids}
        print(f"{name}: {paths[0][0]}, {len(distinct)} distinct ids", flush=True)
    doc = {"rows": G.ROWS, "salt": G.SALT, "temperature": G.TEMPERATURE, "positions": list(G.POSITIONS),
           "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
