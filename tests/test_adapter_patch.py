"""adapters/libviso_hip.patch must fit the reference tree, leave it untouched when VISO_USE_HIP is not defined, and
with the macro swap exactly the hot-path functions for adapters/viso_hip_adapter.inc.  The reference
itself cannot be compiled here (no OpenCV / Boost), so this is a source-level check of the two preprocessor views of the
patched files.  The reference is not part of this repository: its src/viso.cpp and src/viso.h are stood in for by
tests/golden/reference_layout.json (made by tests/golden/make_reference_layout.py from a checkout of the reference),
which gives their line counts, the lines of their conditional directives and the lines of the definitions and call
sites named below.  The patch is applied to a placeholder file of that shape, one numbered placeholder per reference
line, so that every surviving reference line can be told by its number."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "adapters", "libviso_hip.patch")
ADAPTER = os.path.join(ROOT, "adapters", "viso_hip_adapter.inc")
LAYOUT = os.path.join(ROOT, "tests", "golden", "reference_layout.json")

REPLACED = ("tr2mat", "match_circle", "match_desc", "ransac_minimize_reproj", "minimize_reproj")   # anchors def_<name>


def view(text, defined):
    """The file as the preprocessor passes it on, for the VISO_USE_HIP conditionals only (every other directive is kept
    as text; nesting is tracked so that an #endif of another conditional inside a guarded function is not mistaken)."""
    out, stack = [], []          # stack entries: None = foreign conditional, True/False = ours (keep / drop)
    for ln in text.splitlines(keepends=True):
        s = ln.strip()
        ours = re.match(r"#\s*(ifdef|ifndef)\s+VISO_USE_HIP\b", s)
        if ours:
            stack.append((ours.group(1) == "ifdef") == defined)
            continue
        if re.match(r"#\s*if", s):
            stack.append(None)
        elif re.match(r"#\s*endif", s):
            top = stack.pop()
            if top is not None:
                continue
        if all(t is not False for t in stack):
            out.append(ln)
    assert not stack
    return "".join(out)


def parse_patch(text):
    """{file: [(old_start, old_count, new_start, new_count, [hunk lines])]} of a unified diff."""
    files, hunks, lines = {}, None, text.splitlines()
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("--- a/"):
            assert lines[i + 1].startswith("+++ b/")
            hunks = files.setdefault(lines[i + 1][len("+++ b/"):], [])
            i += 2
            continue
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", ln)
        if m:
            hunks.append((int(m[1]), int(m[2] or 1), int(m[3]), int(m[4] or 1), []))
        else:
            hunks[-1][4].append(ln)
        i += 1
    return files


def _kind(line):
    s = line.strip()
    return "if" if re.match(r"#\s*if", s) else "endif" if re.match(r"#\s*endif", s) else None


def placeholder_file(info):
    """One line per reference line: its conditional directives keep their kind, every line carries its number."""
    ifs, endifs = set(info["if"]), set(info["endif"])
    return [("#if " if n in ifs else "#endif " if n in endifs else "") + f"/*@ref {n}*/"
            for n in range(1, info["lines"] + 1)]


def apply_hunks(old, hunks):
    """The patched file.  The hunks' positions must agree with the reference's length, and every context line must
    fall on a reference line of the same kind (directive or not)."""
    new, pos = [], 0
    for a, b, c, d, body in hunks:
        start = a - 1 if b else a
        assert pos <= start <= len(old)
        new += old[pos:start]
        pos = start
        assert len(new) == (c - 1 if d else c)
        for ln in body:
            tag, txt = (ln[:1] or " "), ln[1:]
            assert tag in " +", "the patch removes no reference line"
            if tag == " ":
                assert pos < len(old) and _kind(txt) == _kind(old[pos]), (a, ln)
                new.append(old[pos])
                pos += 1
            else:
                new.append(txt)
        assert pos == start + b and len(new) == (c - 1 if d else c) + d
    return new + old[pos:]


@pytest.fixture(scope="module")
def layout():
    with open(LAYOUT) as f:
        lay = json.load(f)
    assert not any(info["mentions_VISO_USE_HIP"] for info in lay["files"].values())
    return lay


@pytest.fixture(scope="module")
def patched(layout):
    """{file: (reference placeholder lines, patched lines)} for src/viso.cpp and src/viso.h."""
    files = parse_patch(open(PATCH).read())
    out = {}
    for rel, info in layout["files"].items():
        old = placeholder_file(info)
        out[rel] = (old, apply_hunks(old, files[rel]))
    return out


def _text(lines):
    return "".join(ln + "\n" for ln in lines)


def _ref_positions(lines):
    """reference line number -> index in `lines`, for the reference lines that survived."""
    out = {}
    for i, ln in enumerate(lines):
        m = re.search(r"/\*@ref (\d+)\*/", ln)
        if m:
            out[int(m[1])] = i
    return out


def test_without_the_macro_the_tree_is_the_reference(patched):
    for rel in ("src/viso.cpp", "src/viso.h"):
        old, new = patched[rel]
        assert view(_text(new), defined=False) == _text(old), rel
    # every other source file is untouched (src/CMakeLists.txt only gains the VISO_USE_HIP option)
    assert sorted(parse_patch(open(PATCH).read())) == ["src/CMakeLists.txt", "src/viso.cpp", "src/viso.h"]


def test_with_the_macro_the_hot_path_comes_from_the_adapter(layout, patched):
    anchor = {k: v["lines"] for k, v in layout["anchors"].items()}
    assert all(v["file"] == "src/viso.cpp" for v in layout["anchors"].values())
    lines = view(_text(patched["src/viso.cpp"][1]), defined=True).splitlines()
    kept = _ref_positions(lines)
    for name in REPLACED:
        assert len(anchor["def_" + name]) == 1, name
        assert not [n for n in anchor["def_" + name] if n in kept], f"the reference's {name} is still compiled"
    # collect_matches: the (.., Mat &x) overload is gone, the other two stay
    cm, cm_x = anchor["def_collect_matches"], anchor["def_collect_matches_x"]
    assert len(cm) == 3 and len(cm_x) == 1 and cm_x[0] in cm
    assert cm_x[0] not in kept and all(n in kept for n in cm if n != cm_x[0])
    # the adapter: once, behind both triangulate_rectified templates (an explicit specialisation needs its primary
    # template), in front of sequence_odometry (its first use), where MatchParams and kp2mat are visible
    inc = [i for i, ln in enumerate(lines) if ln.strip() == '#include "viso_hip_adapter.inc"']
    assert len(inc) == 1
    pos = lambda name: [kept[n] for n in anchor[name]]
    assert len(anchor["def_triangulate_rectified"]) == 2
    assert max(pos("def_triangulate_rectified")) < inc[0] < pos("def_sequence_odometry")[0]
    assert pos("def_struct_MatchParams")[0] < inc[0] and pos("def_kp2mat")[0] < inc[0]
    # the call sites are the reference's own, unchanged (5-argument match_desc needs the adapter's default argument)
    assert len(anchor["call_match_desc_match11"]) == 1 and anchor["call_match_desc_match11"][0] in kept
    assert not any("match_desc(kp1,kp1_prev,d1,d1_prev,match11);" in ln for ln in lines)   # no added call site
    # RANSAC stream key = the frame's FILE NUMBER (what viso_kitti / kitti_shard key on), read off the generator
    assert sum("param.frame_index = images.index() - 1;" in ln for ln in lines) == 1
    h = view(_text(patched["src/viso.h"][1]), defined=True)
    assert "unsigned long long ransac_seed = 0, frame_index = 0;" in h
    assert "int index() const { return m_index; }" in h
    cmake = parse_patch(open(PATCH).read())["src/CMakeLists.txt"]
    assert any("VISO_USE_HIP" in ln for h_ in cmake for ln in h_[4] if ln.startswith("+"))


def test_adapter_defines_each_replacement_once():
    a = open(ADAPTER).read()
    for sig in (r"^void match_desc\(const KeyPoints& kp1, const KeyPoints& kp2, const Descriptors& d1, const Descriptors& d2,\n\s+Matches& match, const MatchParams& sp = MatchParams\(\)\)",
                r"^bool minimize_reproj\(const Mat& X, const Mat& observe, vector<double>& tr, const struct param& param,",
                r"^bool ransac_minimize_reproj\(const Mat& X, const Mat& observe, vector<double>& best_tr,",
                r"^void match_circle\(const Matches& lr, const Matches& lrp, const Matches& m11, const Matches& m22,",
                r"^void tr2mat\(vector<double> tr, Mat& Tr\)",
                r"^void collect_matches\(const KeyPoints& kp1, const KeyPoints& kp2, const Matches& match, Mat& x\)",
                r"^template <> Mat triangulate_rectified<double>\(const Mat& x, const struct param& param\)"):
        assert len(re.findall(sig, a, flags=re.M)) == 1, sig
    assert "static uint64_t call" not in a and "param.frame_index" in a and '#include "viso.h"' not in a
