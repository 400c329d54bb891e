"""Did a change touch the device code?  Compiles csrc/kernels/*.hip files from a git revision
and from the working tree to gfx950 assembly (device side only, the flags of
nanosandbox_amd/build.py) and compares the two texts per file.  Needs hipcc, no GPU.

    python scripts/device_asm_diff.py [REV] csrc/kernels/decode.hip csrc/kernels/decode_q8.hip

Per file: ``identical``; ``reordered`` (the same functions with the same bodies, emitted in
another order); or ``DIFFERENT`` with the names of the functions whose bodies differ or that only
one side has.  Exit status 1 if any file is DIFFERENT.  REV defaults to HEAD~1.
"""
import argparse
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanosandbox_amd import build  # noqa: E402

KERNELS = os.path.join("csrc", "kernels")
# hipcc names one symbol per file after a hash of the source's path: the same id on both sides
CUID = "-cuid=device_asm_diff"
BEGIN = re.compile(r"; -- Begin function (\S+)")
END = "; -- End function"
# local labels carry the function's index in the file, which moves when the order does
LABEL = re.compile(r"\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+")


def device_asm(tree, name, out):
    src = os.path.join(tree, KERNELS, name)
    flags = build.kernel_flags(src, include_dir=os.path.join(tree, KERNELS))
    build._run([build._hipcc(), *flags, CUID, "--cuda-device-only", "-S", src, "-o", out])
    return open(out).read()


def functions(asm):
    """{name: body} of an assembly listing, local labels without the function's index."""
    out, name, body = {}, None, []
    for line in asm.splitlines():
        m = BEGIN.search(line)
        if m:
            name, body = m.group(1), []
        if name is not None:
            body.append(LABEL.sub(r".\1", line))
            if END in line:
                out[name], name = "\n".join(body), None
    return out


def compare(old, new):
    """('identical' | 'reordered' | 'DIFFERENT', names of the functions that differ)."""
    if old == new:
        return "identical", []
    fo, fn = functions(old), functions(new)
    differ = sorted(n for n in fo.keys() | fn.keys() if fo.get(n) != fn.get(n))
    if differ:
        return "DIFFERENT", [n + ("" if n in fo and n in fn else " (old only)" if n in fo else " (new only)")
                             for n in differ]
    if list(fo) != list(fn):
        return "reordered", []
    return "DIFFERENT", ["(outside the functions)"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev_and_files", nargs="+", metavar="[REV] FILE", help="git revision (default HEAD~1), then "
                    "csrc/kernels/*.hip files")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args(argv)
    rev, files = "HEAD~1", a.rev_and_files
    if not files[0].endswith(".hip"):
        rev, files = files[0], files[1:]
    names = [os.path.basename(f) for f in files]
    if not names:
        ap.error("no csrc/kernels/*.hip file given")
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        os.makedirs(old_tree)
        tar = os.path.join(tmp, "old.tar")
        subprocess.run(["git", "-C", ROOT, "archive", "-o", tar, rev, KERNELS.replace(os.sep, "/")], check=True)
        with tarfile.open(tar) as t:
            t.extractall(old_tree)
        jobs = [(tree, n, os.path.join(tmp, f"{side}_{n}.s")) for n in names
                for side, tree in (("old", old_tree), ("new", ROOT))]
        with ThreadPoolExecutor(max_workers=max(1, a.jobs)) as ex:
            asm = list(ex.map(lambda j: device_asm(*j), jobs))
    bad = 0
    for i, n in enumerate(names):
        verdict, differ = compare(asm[2 * i], asm[2 * i + 1])
        print(f"{n}: {verdict} ({rev} {len(asm[2 * i].splitlines())} lines, working tree "
              f"{len(asm[2 * i + 1].splitlines())})")
        for d in differ:
            print(f"  {d}")
        bad += verdict == "DIFFERENT"
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
