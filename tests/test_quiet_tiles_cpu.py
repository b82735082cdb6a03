"""
CPU: the quiet tiles of the one-kernel step (classic_fused.hpp, quiet_tiles.hpp) rely on a whitelist.
The words of one launch may decide the next only if nothing but the step itself and read-only calls came in between, so
every C entry point that takes a solver and is not on the list below must invalidate them (QuietTiles::invalidate)
before anything else.  A new entry point fails here until it does so or is added to the list.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pyclaw_amd", "csrc", "pclaw.hip")
HDR = os.path.join(ROOT, "pyclaw_amd", "csrc", "quiet_tiles.hpp")

# the step itself carries the words on (internally: only its one-kernel form of the whole block), the rest only read
CARRY = {"pcl_step_hyperbolic", "pcl_bc_step"}
READ_ONLY = {"pcl_destroy", "pcl_get_q", "pcl_get_strip", "pcl_get_cells", "pcl_sync", "pcl_timer_start",
             "pcl_timer_stop", "pcl_kernel_timing", "pcl_step_count", "pcl_kernel_timing_read", "pcl_step_form_stats",
             "pcl_tile_skip_stats"}


def entry_points():
    src = open(SRC).read()
    out = {}
    for m in re.finditer(r"^(?:int|void) (pcl_\w+)\(pcl_solver \*s\b[^{;]*\{\n", src, re.M):
        out[m.group(1)] = src[m.end():m.end() + 400].split("\n")[0]
    return out


def test_every_other_entry_point_invalidates_first():
    eps = entry_points()
    assert len(eps) >= 40 and CARRY <= set(eps) and READ_ONLY <= set(eps)
    for name, first_line in eps.items():
        if name in CARRY or name in READ_ONLY:
            continue
        assert first_line.strip().startswith("if (s) s->qt.invalidate();"), (name, first_line)


def code(path):
    """the file without its comments"""
    return re.sub(r"//[^\n]*", "", open(path).read())


def test_step_entry_points_drop_then_restore():
    src, hdr = code(SRC), code(HDR)
    # (a) the step entry points take the flag and clear it before they touch the quiet-tile state in any other way
    for name in CARRY:
        body = src[src.index("int %s(pcl_solver *s" % name):]
        body = body[:body.index("\n}\n")]
        uses = [m.group(0) for m in re.finditer(r"\bqt\b[^;]*;", body)]
        assert uses and re.match(r"qt\.take_valid\(\)", uses[0]), (name, uses[:1])
        assert sum("take_valid" in u for u in uses) == 1, (name, uses)
    # the solver holds one QuietTiles and nothing else of the kind
    assert len(re.findall(r"\bQuietTiles\s+\w+\s*;", src)) == 1 and "QuietTiles qt;" in src
    # (b) the flag becomes true at one place in the two files, launched(), and is not a public member
    true_sites = re.findall(r"\bvalid\s*=\s*true\b", src + hdr)
    assert len(true_sites) == 1
    launched = hdr[hdr.index("void launched("):]
    assert re.search(r"\bvalid\s*=\s*true\b", launched[:launched.index("\n    }\n")])
    decl = re.search(r"^\s*bool\b[^;()]*\bvalid\b[^;()]*;", hdr, re.M)
    assert decl and "private:" in hdr[:decl.start()] and "public:" not in hdr[hdr.index("private:"):]
    assert re.search(r"\bclass QuietTiles\b", hdr)
    # (c) nothing in pclaw.hip assigns to it, or names it at all
    assert not re.search(r"\bvalid\s*(?:[-+|&^]?=)(?!=)", src)
    assert not re.search(r"(?:\.|->)\s*valid\b", src)
