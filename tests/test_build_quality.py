"""Build-quality guard (no GPU needed): the hot kernels must compile without scratch (register-spill) traffic
and without a copy of their parameter blocks to scratch.

A wave of these kernels stalls for an L2 round trip on every scratch reload; builds that differed only in
where hipcc's register allocator spilled differed by up to 7 us per call, and a parameter block copied to
scratch at kernel entry (what hipcc does without the flag in clima_amd/build.py) doubles the run time
("What bounds these kernels").  The check reads the gfx950 assembly hipcc writes for
clima_amd/csrc/kernels.hip with the build's own flags (tests/build_inspect.py; tools/scratch_report.py prints the same
counts from the same place).
"""
import os
import re

import pytest

import build_inspect
from clima_amd import build as B

# kernels of the production paths: fused grid, stand-alone opacity tile, group-of-lanes opacity,
# wave-per-column two-stream, batched IR, prep, integration
HOT = re.compile(r"k_fused|k_opacity8|k_opacity_coop|k_twostream_w|k_twostream_h|k_twostream_ir_batch|k_prep|k_integrate_one|k_green_")


@pytest.fixture(scope="module")
def assembly():
    if not build_inspect.have_hipcc():
        pytest.skip("no hipcc")
    return build_inspect.scratch_counts()


# The 16- and 32-lane group-of-lanes kernels are compiled for one wave per SIMD more than their registers allow
# without spilling (round 3, measured: 610 -> 541 us at 16 g-points, 4.67 -> 2.92 ms at 32): a few dozen scratch accesses
# outside the sort network are the price, and are bounded here.
BOUNDED = re.compile(r"k_opacity_coopILi(16|32)E")
BOUND = 64
# Round 4: the kernels that hold the assembly form of the mixing step (rorr_xys_asm.inc names 192 registers; the
# compiler keeps what lives across it in the other 64).  What is left is a handful of loop-invariant values spilled
# once before the species loop and reloaded after it -- none on the path of a mixing step (measured: 84.1 -> 81.8 us
# per config-2 call against the build without the block, 84.5 with 20 of them still inside the loop).
ASM_STEP = re.compile(r"k_fusedILi0E|k_opacity8ILi0E")
ASM_STEP_BOUND = 16


def test_hot_kernels_have_no_scratch_traffic(assembly):
    hot = {k: v for k, v in assembly.items() if HOT.search(k)}
    assert len(hot) >= 30, sorted(hot)             # every instantiation of the fused grid and the stand-alone kernels
    bad = {k: v for k, v in hot.items() if v and not BOUNDED.search(k) and not ASM_STEP.search(k)}
    assert not bad, "scratch instructions in: %s (python tools/scratch_report.py)" % bad
    over = {k: v for k, v in hot.items() if BOUNDED.search(k) and v > BOUND}
    assert not over, "more than %d scratch instructions in: %s" % (BOUND, over)
    over = {k: v for k, v in hot.items() if ASM_STEP.search(k) and v > ASM_STEP_BOUND}
    assert not over, "more than %d scratch instructions in: %s" % (ASM_STEP_BOUND, over)


def test_build_flags_keep_parameter_blocks_in_the_kernarg_segment():
    assert any("instcombine-max-copied-from-constant-users" in f for f in B.FLAGS)


def _environment_table():
    """The names in the first column of INTEGRATION.md's table of environment variables."""
    text = open(os.path.join(os.path.dirname(B.CSRC), "..", "INTEGRATION.md")).read()
    rows = text[text.index("Environment variables."):].split("\n| name |", 1)[1].split("\n\n", 1)[0].splitlines()[2:]
    return {re.match(r"\| `(\w+)` \|", row).group(1) for row in rows}


def test_every_environment_variable_the_library_reads_is_documented():
    """The string literals passed to getenv( under clima_amd/csrc, with the CLIMA_* names the Python package reads, are
    exactly the rows of INTEGRATION.md's table; the kernels' file and what it includes read no environment at all."""
    read = set()
    for name in sorted(os.listdir(B.CSRC)):
        if not name.endswith((".hip", ".inc", ".h")):
            continue
        src = open(os.path.join(B.CSRC, name)).read()
        found = re.findall(r'getenv\(\s*"(\w+)"', src)
        assert len(found) == src.count("getenv"), "%s: a getenv whose argument is no string literal (or a comment's)" % name
        if name == "kernels.hip" or name.endswith(".inc"):
            assert "getenv" not in src, "%s reads the environment" % name
        read |= set(found)
    assert len(read) >= 10, read
    pkg = os.path.dirname(B.CSRC)
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            read |= set(re.findall(r'environ(?:\.get\(|\[)\s*"(CLIMA_\w+)"', open(os.path.join(pkg, name)).read()))
    assert read == _environment_table(), sorted(read ^ _environment_table())
