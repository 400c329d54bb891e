"""scripts/device_asm_diff.py: the three verdicts of its text comparison on small hand-written
listings (the compilation itself needs hipcc and is what the script is run for), and that it
compiles with the flags of nanosandbox_amd/build.py."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("device_asm_diff", os.path.join(ROOT, "scripts", "device_asm_diff.py"))
dad = importlib.util.module_from_spec(spec)
spec.loader.exec_module(dad)


def _fn(name, index, op="v_add_f32_e32 v0, v0, v1"):
    return (f"\t.globl\t{name} ; -- Begin function {name}\n{name}:\n\ts_cbranch_scc1 .LBB{index}_2\n\t{op}\n"
            f".LBB{index}_2:\n\ts_endpgm\n.Lfunc_end{index}:\n\t.size\t{name}, .Lfunc_end{index}-{name}\n"
            "                                        ; -- End function\n")


HEAD = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n'


def test_identical_and_reordered():
    a = HEAD + _fn("ka", 0) + _fn("kb", 1)
    assert dad.compare(a, a) == ("identical", [])
    # the same two bodies in the other order: only the index in the local labels moves
    assert dad.compare(a, HEAD + _fn("kb", 0) + _fn("ka", 1)) == ("reordered", [])


def test_different_names_the_functions():
    a = HEAD + _fn("ka", 0) + _fn("kb", 1)
    assert dad.compare(a, HEAD + _fn("ka", 0) + _fn("kb", 1, op="v_mul_f32_e32 v0, v0, v1")) == ("DIFFERENT", ["kb"])
    assert dad.compare(a, HEAD + _fn("ka", 0)) == ("DIFFERENT", ["kb (old only)"])
    assert dad.compare(HEAD + _fn("ka", 0), a) == ("DIFFERENT", ["kb (new only)"])
    # a change outside every function is not passed over
    assert dad.compare(a, a + "\t.p2align 4\n")[0] == "DIFFERENT"


def test_flags_are_the_builds():
    from nanosandbox_amd import build

    src = os.path.join(build.CSRC, "kernels", "flash_attn.hip")
    flags = build.kernel_flags(src)
    assert "-O3" in flags and f"--offload-arch={build.ARCH}" in flags
    assert all(f in flags for f in build.FILE_FLAGS["flash_attn.hip"])
    assert not any(f in build.kernel_flags(src, file_flags={}) for f in build.FILE_FLAGS["flash_attn.hip"])
