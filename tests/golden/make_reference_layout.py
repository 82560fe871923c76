"""Generates tests/golden/reference_layout.json: where things are in the reference's src/viso.cpp and src/viso.h, so that
tests/test_adapter_patch.py can check adapters/libviso_hip.patch without a checkout of the reference.  Recorded per
file: its sha256 and line count, the line numbers of its conditional directives (#if* / #endif: the only lines that
matter to the VISO_USE_HIP views), and the line numbers of the named anchors below.  No source text is stored.

    python tests/golden/make_reference_layout.py <checkout of alexkreimer/libviso>
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

ANCHORS = {   # name -> (file, regex on the line); every match is recorded
    # the reference's definitions that the adapter replaces (first line of each definition)
    "def_tr2mat": ("src/viso.cpp", r"^tr2mat\(vector<double> tr,Mat& Tr\)"),
    "def_match_circle": ("src/viso.cpp", r"^match_circle\(const Matches& match_lr, const Matches& match_lr_prev,"),
    "def_match_desc": ("src/viso.cpp", r"^match_desc\(const KeyPoints& kp1, const KeyPoints& kp2,"),
    "def_ransac_minimize_reproj": ("src/viso.cpp", r"^ransac_minimize_reproj\(const Mat& X, /\* 3d points \*/"),
    "def_minimize_reproj": ("src/viso.cpp", r"^minimize_reproj\(const Mat& X, const Mat& observe, vector<double>& tr,"),
    # the three collect_matches overloads, and the one among them whose next line ends in `Mat &x)`
    "def_collect_matches": ("src/viso.cpp", r"^collect_matches\(const KeyPoints& kp1, const KeyPoints &kp2,"),
    "def_collect_matches_x": ("src/viso.cpp", r"^collect_matches\(const KeyPoints& kp1, const KeyPoints &kp2,(?=.*\n.*Mat &x\))"),
    # what the adapter's #include must come after / before
    "def_triangulate_rectified": ("src/viso.cpp", r"^triangulate_rectified\(const Mat& x,"),
    "def_sequence_odometry": ("src/viso.cpp", r"^sequence_odometry\(const Mat& P1"),
    "def_struct_MatchParams": ("src/viso.cpp", r"^struct MatchParams"),
    "def_kp2mat": ("src/viso.cpp", r"^kp2mat\(const KeyPoints& kp\)"),
    # the call site that needs the adapter's default argument
    "call_match_desc_match11": ("src/viso.cpp", r".*match_desc\(kp1,kp1_prev,d1,d1_prev,match11\);"),
}
FILES = ("src/viso.cpp", "src/viso.h")


def layout(ref):
    out = {"files": {}, "anchors": {}}
    text = {}
    for rel in FILES:
        raw = open(os.path.join(ref, rel), "rb").read()
        text[rel] = raw.decode("utf-8", errors="surrogateescape")
        lines = text[rel].splitlines()
        out["files"][rel] = {
            "sha256": hashlib.sha256(raw).hexdigest(), "lines": len(lines),
            "if": [i + 1 for i, ln in enumerate(lines) if re.match(r"#\s*if", ln.strip())],
            "endif": [i + 1 for i, ln in enumerate(lines) if re.match(r"#\s*endif", ln.strip())],
            "mentions_VISO_USE_HIP": "VISO_USE_HIP" in text[rel],
        }
    for name, (rel, rx) in ANCHORS.items():
        starts = [m.start() for m in re.finditer(rx, text[rel], flags=re.M)]
        out["anchors"][name] = {"file": rel, "lines": [text[rel].count("\n", 0, s) + 1 for s in starts]}
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with open(os.path.join(HERE, "reference_layout.json"), "w") as f:
        json.dump(layout(sys.argv[1]), f, indent=1)
        f.write("\n")
