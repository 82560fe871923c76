"""The test-only harness of the device helper headers (tests/dev_harness/helpers.hip): build it with the library's own compiler
flags, load it once per session, and call its wrappers on numpy arrays.  The helpers are tested as compiled in the harness's own
translation unit; VISO_DEV_HARNESS_CSRC names another directory to take the four headers from (a copy with one helper changed:
how the tests are shown to bite)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np

import libviso_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "dev_harness", "helpers.hip")
CSRC = os.environ.get("VISO_DEV_HARNESS_CSRC") or libviso_amd.CSRC
HIPCC = "/opt/rocm/bin/hipcc"

# every wrapper of the elementwise form dh_<name>(a, b, c, out, n, p), and the others by their own signatures
ELEMENTWISE = (
    ["wave_dpp_0x%s" % c for c in ("B1", "4E", "141", "140", "128")]
    + ["wave_dpp_bc_0x%s" % c for c in ("00", "55", "AA", "FF", "101", "130", "138")]
    + ["viso_dpp_0x%s_0x%s" % cm for cm in (("111", "f"), ("112", "f"), ("114", "f"), ("118", "f"), ("142", "a"), ("143", "c"),
                                             ("B1", "f"), ("4E", "f"), ("141", "f"), ("140", "f"), ("130", "f"), ("138", "f"))]
    + ["dpp_f64_0x%s_0x%s" % cm for cm in (("111", "f"), ("112", "f"), ("114", "f"), ("118", "f"), ("142", "a"), ("143", "c"))]
    + ["wave_shr1", "wave_shl1", "wave_swizzle_0x101F", "wave_swizzle_0x401F", "swz_bcast8", "bperm", "rdlane", "readlane_f32", "uni",
       "wave_min63", "wave_max63", "wave_max63_u64", "wave_scan", "wave_sum63", "wave_min_u32", "wave_max_u32", "wave_max_u64",
       "row_min_u32", "group_sum_4", "group_sum_8", "wave_fext_min", "wave_fext_max", "wave_fsum63", "wave_sum_to_lane63",
       "block_sum_7_4", "block_sum_27_4", "block_sum_50_4", "abs_add_abs", "add_abs_abs", "fmin_raw", "fmax_raw", "med3_u32",
       "row8_of", "row8_of_uniform", "row8_pair_of_biased", "pack_block_sums", "mbcnt", "l1", "buckets", "sampson", "epipolar_band",
       "map_hash", "voxel_key", "voxel_runs", "lu_solve6", "sample3", "splitmix64", "mulhi64", "up6"])
OTHERS = ["store_row8", "bitonic", "list_position", "voxel_probe", "write_cov6", "host_voxel_key", "host_sample3", "host_splitmix64",
          "host_mulhi64"]
WRAPPERS = ELEMENTWISE + OTHERS


def library_cxxflags():
    """CXXFLAGS of libviso_amd/csrc/Makefile, with its ARCH filled in: read, not restated."""
    text = open(os.path.join(libviso_amd.CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_command(out):
    return [HIPCC] + library_cxxflags() + ["-shared", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", out]


_tmp = None
_so = None
_lib = None


def build():
    """Compile the harness for gfx950 into a temporary directory (kept for the session); returns the shared library's path."""
    global _tmp, _so
    if _so is None:
        _tmp = tempfile.TemporaryDirectory(prefix="viso_dev_harness_")
        so = os.path.join(_tmp.name, "libviso_dev_harness.so")
        r = subprocess.run(compile_command(so), capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the device helper harness does not compile:\n" + r.stderr[-4000:])
        _so = so
    return _so


def load():
    """ctypes handle of the harness, built on first use.  torch first, as libviso_amd.load() does: one HIP runtime per process."""
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = C.CDLL(build())
        for name in WRAPPERS:
            getattr(_lib, "dh_" + name).restype = None if name.startswith("host_") else C.c_int
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _in(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype)


def check(err, name):
    assert err == 0, "dh_%s: HIP error %d" % (name, err)


def call(name, out, a, b=None, c=None, p=0):
    """dh_<name>(a, b, c, out, n, p): `out` [n, ...] is written in place and returned; n a multiple of 256.  The arrays must have the
    wrapper's element types already (nothing is converted)."""
    assert name in ELEMENTWISE, name
    assert out.flags.c_contiguous and all(x is None or x.flags.c_contiguous for x in (a, b, c))
    n = out.shape[0]
    assert n % 256 == 0 and all(x is None or x.shape[0] == n for x in (a, b, c))
    check(getattr(load(), "dh_" + name)(_ptr(a), _ptr(b), _ptr(c), _ptr(out), C.c_int(n), C.c_int(p)), name)
    return out


def store_row8(buf, va, vb, s, mode):
    va, vb = _in(va, np.int32), _in(vb, np.int32)
    assert buf.dtype == np.uint8 and buf.size == (2 * (len(va) // 64) + 1) * 128 and len(va) == len(vb)
    check(load().dh_store_row8(_ptr(buf), _ptr(va), _ptr(vb), C.c_int(len(va)), C.c_int(s), C.c_int(mode)), "store_row8")
    return buf


def bitonic(io, npad, threads):
    """io [blocks, npad + guard] u64, sorted in place: the first npad keys of every row by a workgroup of `threads`."""
    assert io.dtype == np.uint64 and io.flags.c_contiguous
    check(load().dh_bitonic(_ptr(io), C.c_int(npad), C.c_int(io.shape[1] - npad), C.c_int(io.shape[0]), C.c_int(threads)), "bitonic")
    return io


def list_position(take):
    take = _in(take, np.int32)
    at, ret, total = np.zeros(len(take), np.uint64), np.zeros(len(take), np.int32), C.c_ulonglong(0)
    check(load().dh_list_position(_ptr(take), _ptr(at), _ptr(ret), C.byref(total), C.c_int(len(take))), "list_position")
    return at, ret, total.value


def voxel_probe(table, keys, find=False):
    """Every key through voxel_probe (the table is updated in place), or voxel_find: (slot, claimed or None, returned)."""
    keys = _in(keys, np.uint64)
    assert table.dtype == np.uint64 and table.flags.c_contiguous
    slot, ret = np.zeros(len(keys), np.uint32), np.zeros(len(keys), np.int32)
    claimed = None if find else np.zeros(len(keys), np.int32)
    check(load().dh_voxel_probe(_ptr(table), C.c_int(len(table)), _ptr(keys), C.c_int(len(keys)), _ptr(slot), _ptr(claimed), _ptr(ret)),
          "voxel_probe")
    return slot, claimed, ret


def write_cov6(Li, sigma2):
    Li, sigma2 = _in(Li, np.float64), _in(sigma2, np.float64)
    cov = np.zeros_like(Li)
    check(load().dh_write_cov6(_ptr(Li), _ptr(sigma2), _ptr(cov), C.c_int(len(sigma2))), "write_cov6")
    return cov


def host_voxel_key(k, d):
    k, d = _in(k, np.int32), _in(d, np.uint32)
    out = np.zeros((len(d), 5), np.int64)
    load().dh_host_voxel_key(_ptr(k), _ptr(d), _ptr(out), C.c_int(len(d)))
    return out


def host_sample3(a, N):
    a, N = _in(a, np.uint64), _in(N, np.int32)
    out = np.zeros((len(N), 3), np.int32)
    load().dh_host_sample3(_ptr(a), _ptr(N), _ptr(out), C.c_int(len(N)))
    return out


def host_splitmix64(a):
    a = _in(a, np.uint64)
    out = np.zeros((len(a), 2), np.uint64)
    load().dh_host_splitmix64(_ptr(a), _ptr(out), C.c_int(len(a)))
    return out


def host_mulhi64(a, b):
    a, b = _in(a, np.uint64), _in(b, np.uint64)
    out = np.zeros(len(a), np.uint64)
    load().dh_host_mulhi64(_ptr(a), _ptr(b), _ptr(out), C.c_int(len(a)))
    return out
