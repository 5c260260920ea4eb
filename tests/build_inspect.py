"""What the tests and tools/scratch_report.py read off the build without a GPU, each stated once: the gfx950 assembly of
clima_amd/csrc/kernels.hip under the build's own flags (clima_amd/build.py FLAGS) with its scratch instructions per
kernel, and the argument counts of the prototypes in include/clima_radtran_hip.h.  The assembly is compiled once per
process (about 80 s) and cached."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

from clima_amd import build as B

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def have_hipcc():
    return bool(os.path.exists(B.HIPCC) or shutil.which(B.HIPCC))


@functools.lru_cache(maxsize=None)
def kernel_scratch(extra_flags=()):
    """{mangled kernel name: (lines of its body, [(line number in the body, the line) of every line that names a
    scratch_ instruction])}.  extra_flags: a tuple of further compiler flags (-D...)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kernels.s")
        flags = [f for f in B.FLAGS if f not in ("-fPIC", "-shared")]
        subprocess.check_call([B.HIPCC] + flags + list(extra_flags) + ["-S", "--cuda-device-only", "-w", os.path.join(B.CSRC, "kernels.hip"), "-o", out])
        kernels, name, n, hits = {}, None, 0, []
        for line in open(out):
            m = re.match(r"^(_ZN5clima\w+):", line)
            if m:
                name, n, hits = m.group(1), 0, []
            elif name is not None:
                n += 1
                if "scratch_" in line:
                    hits.append((n, line.strip()))
                elif line.startswith(".Lfunc_end"):
                    kernels[name] = (n, hits)
                    name = None
    return kernels


def scratch_counts():
    """scratch instructions per kernel of kernels.hip"""
    return {k: len(hits) for k, (_, hits) in kernel_scratch().items()}


@functools.lru_cache(maxsize=None)
def header_text():
    """include/clima_radtran_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clima_radtran_hip.h")).read(), flags=re.S)


def header_arg_counts():
    """{name: argument count} of every prototype of the header"""
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bvoid\s+([a-z_0-9]+)\s*\(([^)]*)\)", header_text())}
