"""The kernels' cross-lane vocabulary lives in ONE header, libviso_amd/csrc/wave.h: the lane-move builtins and the inline-asm
one-liners are spelled there and nowhere else, and the per-file copies it replaced (one set per matcher kernel file, each under
the file's own prefix) do not come back with the next kernel file that starts as a copy of another.  Reads the sources as
text: no compiler, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libviso_amd", "csrc")

BUILTINS = ["__builtin_amdgcn_update_dpp", "__builtin_amdgcn_ds_swizzle", "__builtin_amdgcn_ds_bpermute"]
MNEMONICS = ["v_add_f32_e64", "v_min_f32_e32", "v_max_f32_e32", "v_med3_u32"]
REMOVED = ["dpp_mov", "mu_dpp", "mp_dpp", "mb_dpp", "st_dpp", "ms_dpp", "mu_bcast", "mu_l1_bits", "mp_l1_bits", "mb_l1_bits",
           "ms_l1_bits", "mu_fmin", "mu_fmax", "mu_ybucket", "mp_ybucket", "ms_ybucket", "st_bucket", "st_scan_incl"]


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    paths.append(os.path.join(ROOT, "tools", "experiments", "match_strip.hip"))
    assert os.path.join(CSRC, "wave.h") in paths and len(paths) > 30
    out = {}
    for p in paths:
        with open(p) as f:
            out[os.path.relpath(p, ROOT)] = f.read()
    return out


def _files_with(word, whole_word=False):
    rx = re.compile(r"(?<![A-Za-z0-9_])" + re.escape(word) + r"(?![A-Za-z0-9_])" if whole_word else re.escape(word))
    return sorted(name for name, text in _sources().items() if rx.search(text))


WAVE_H = os.path.join("libviso_amd", "csrc", "wave.h")


def test_lane_builtins_only_in_wave_h():
    for b in BUILTINS:
        assert _files_with(b) == [WAVE_H], b


def test_asm_one_liners_only_in_wave_h():
    for m in MNEMONICS:
        assert _files_with(m) == [WAVE_H], m
    # row8_of's clamp has one user and stays beside it
    assert _files_with("v_med3_i32") == [os.path.join("libviso_amd", "csrc", "match_dev.h")]


def test_no_per_file_copy_is_back():
    for name in REMOVED:
        assert _files_with(name, whole_word=True) == [], name


def test_wave_h_is_a_dependency_of_every_object():
    with open(os.path.join(CSRC, "Makefile")) as f:
        hdrs = [ln for ln in f.read().splitlines() if re.match(r"HDRS\s*=", ln)]
    assert len(hdrs) == 1 and "wave.h" in hdrs[0].split("=", 1)[1].split()
