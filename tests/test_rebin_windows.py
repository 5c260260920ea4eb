"""The crossing windows of the window-form rebin are stated in clima_amd/csrc/radtran_dev.h (RB_WIN_* / RB_TIGHT_*: what
the kernels evaluate and what the host checks a handle's weights against) and once more in tools/gen_rorr_asm.py, which
has to run on its own and from which the committed rorr_xys_asm.inc was generated.  No GPU needed."""
import ast
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _header_arrays():
    text = open(os.path.join(ROOT, "clima_amd", "csrc", "radtran_dev.h")).read()
    found = re.findall(r"constexpr int (RB_\w+)\[8\] = \{([^}]*)\};", text)
    return {name: [int(x) for x in body.split(",")] for name, body in found}


def _generator_lists():
    tree = ast.parse(open(os.path.join(ROOT, "tools", "gen_rorr_asm.py")).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in ("RB_LO", "RB_HI"):
            out[node.targets[0].id] = ast.literal_eval(node.value)
    return out


def test_header_states_four_window_tables():
    h = _header_arrays()
    assert sorted(h) == ["RB_TIGHT_HI", "RB_TIGHT_LO", "RB_WIN_HI", "RB_WIN_LO"]
    for name, v in h.items():
        assert len(v) == 8 and v[0] == 0 and v[1:] == sorted(v[1:]) and 0 < v[1] and v[-1] < 64, (name, v)
    for k in range(1, 8):   # a window is a range, and the tight one lies inside the wide one
        assert h["RB_WIN_LO"][k] <= h["RB_TIGHT_LO"][k] <= h["RB_TIGHT_HI"][k] <= h["RB_WIN_HI"][k], k


def test_generator_windows_are_the_headers_tight_pair():
    h, g = _header_arrays(), _generator_lists()
    assert sorted(g) == ["RB_HI", "RB_LO"]
    assert g["RB_LO"] == h["RB_TIGHT_LO"]
    assert g["RB_HI"] == h["RB_TIGHT_HI"]


def test_kernels_read_the_headers_tables():
    """kernels.hip keeps no table of its own: rb_lo / rb_hi index the header's arrays."""
    text = open(os.path.join(ROOT, "clima_amd", "csrc", "kernels.hip")).read()
    for fn, tight, wide in (("rb_lo", "RB_TIGHT_LO", "RB_WIN_LO"), ("rb_hi", "RB_TIGHT_HI", "RB_WIN_HI")):
        m = re.search(r"constexpr int %s\(int k\) \{ return TIGHT \? (\w+)\[k\] : (\w+)\[k\]; \}" % fn, text)
        assert m and m.groups() == (tight, wide), fn
