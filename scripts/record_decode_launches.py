"""Record tests/golden/decode_launches.json: per case of tests/test_decode_launches_gpu.py the
kernel-library calls of an eager run and the tokens, graph keys, replays, statistics and recorded
log-probability bits of a run on captured graphs.

The fixture pins the decode runtime across changes of its Python, so it is recorded on an MI355X with
the ``nanosandbox_amd/runtime/decode.py`` of the commit to compare against and never with the tree
under test (the test module uses the public API only, so the same file observes both):

    python scripts/record_decode_launches.py [--out PATH]

Record twice, in two processes: the two files must be byte-identical.  A case whose tokens are not is
named in the test module's ``UNPINNED_TOKENS`` and recorded without them.  Every case is checked (it
ran on the decoder that was looked at, it launched something) before anything is written.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_decode_launches_gpu as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=G.GOLDEN)
    a = ap.parse_args()
    from nanosandbox_amd.runtime import decode
    print(f"decode runtime: {decode.__file__}", flush=True)
    model = G.build_model()
    cases = {}
    for name in G.CASES:
        seen = cases[name] = G.observe(model, name)
        assert seen["launches"] and seen["replays"] > 0 and seen["graphs"], name
        print(f"{name}: {len(seen['launches'])} launches, {seen['replays']} replays, graphs {seen['graphs']}",
              flush=True)
        if name in G.UNPINNED_TOKENS:
            del seen["tokens"]
            seen.pop("lp", None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"model": G.ARGS, "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
