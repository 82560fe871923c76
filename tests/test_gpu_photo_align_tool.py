"""python -m libviso_amd.fuse_map --surface --align --gray DIR --align-photo WEIGHT on a small synthetic directory: five views of
the textured wall of tests/photo_align_cases.py, ray cast exactly, with a pose file that carries a steady drift.  On one plane the
alignment on the distance alone leaves the motion inside the plane free; with the photometric row the last frame's in-plane error is
smaller.  Without --align-photo the tool's files are those of the same loop through the calls that existed before the option."""
import math
import os

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath
from libviso_amd.abi import TSDF_ALIGNMENT_DTYPE, Param

import align_cases as AC
import align_ref as AR
import photo_align_cases as PC

pytestmark = pytest.mark.gpu

N_VIEWS = 5
DRIFT = [0.0015, -0.0020, 0.0010, 0.012, -0.008, 0.015]   # a frame: 0.15 degrees and 0.02 m (tests/test_gpu_align_tool.py's)


def _scene(tmp_path):
    prm = AC.param()
    truth = [AC.view(0.004 * i, -0.006 * i, 0.002 * i, 0.03 * i, -0.01 * i, 0.10 * i) for i in range(N_VIEWS)]
    drifted, D = [], np.eye(4)
    for T in truth:
        drifted.append(T @ D)
        D = D @ hostmath.tr2mat(DRIFT)
    d, im = tmp_path / "disp", tmp_path / "image_0"
    d.mkdir()
    im.mkdir()
    frames = [PC.raycast(T, "wall") for T in truth]
    for i, (m, g) in enumerate(frames):
        fuse_map.write_disparity_png(str(d / ("%06d.png" % i)), m)
        fuse_map.write_png8(str(im / ("%06d.png" % i)), g)
    poses, calib = str(tmp_path / "poses.txt"), str(tmp_path / "calib.txt")
    fuse_map.write_poses(poses, drifted)
    P0 = [prm.f, 0.0, prm.cu, 0.0, 0.0, prm.f, prm.cv, 0.0, 0.0, 0.0, 1.0, 0.0]
    P1 = list(P0)
    P1[3] = -prm.f * prm.base
    with open(calib, "w") as f:
        for name, P in (("P0", P0), ("P1", P1)):
            f.write(name + ": " + " ".join("%.17g" % v for v in P) + "\n")
    return str(d), str(im), poses, calib, frames, truth


def _in_plane(T, truth):
    """(metres, degrees) of T against truth inside the wall z = 6: the translation along x and y, the rotation about z."""
    R = truth[:3, :3].T @ T[:3, :3]
    return float(np.linalg.norm((T[:3, 3] - truth[:3, 3])[:2])), abs(math.degrees(math.atan2(R[1, 0], R[0, 0])))


def test_the_photometric_row_holds_the_wall_and_the_plain_mode_is_unchanged(viso, tmp_path, capsys):
    d, im, poses, calib, frames, truth = _scene(tmp_path)
    common = ["--surface", "--voxel", "0.1", "--capacity-log2", "18", "--gray", im, "--align", "--align-voxel-gate", "2"]
    out0, out1 = str(tmp_path / "plain.ply"), str(tmp_path / "photo.ply")
    al0, al1 = str(tmp_path / "plain.txt"), str(tmp_path / "photo.txt")
    assert fuse_map.main([d, poses, calib, out0] + common + ["--aligned-poses", al0]) == 0
    capsys.readouterr()
    assert fuse_map.main([d, poses, calib, out1] + common + ["--aligned-poses", al1, "--align-photo", "0.03125"]) == 0
    text = capsys.readouterr().out
    assert "4 maps aligned before they were fused (status: count 1: 4)" in text, text
    T = fuse_map.read_poses(poses)
    f, cu, cv, base = fuse_map.read_calib(calib)
    prm = Param.default(base=base, f=f, cu=cu, cv=cv)

    def by_hand(photo):
        tsdf = libviso_amd.TsdfMap(None, gray=True, voxel=0.1, capacity_log2=18)
        used = []
        for i, (m, g) in enumerate(frames):
            pose = T[i]
            if used:
                pose = used[-1] @ np.linalg.inv(T[i - 1]) @ T[i]
                extra = dict(image=g, photo_weight=0.03125) if photo else {}
                rec = tsdf.align(m, prm, pose, min_weight=1, gate_voxels=2.0, **extra)
                assert photo or rec.dtype == TSDF_ALIGNMENT_DTYPE
                if rec["status"] >= 1:
                    pose = rec["pose"].copy()
            used.append(pose)
            tsdf.fuse(m, prm, pose=pose, image=g)
        c = tsdf.surface(1)
        ply = libviso_amd.surface_ply_bytes(c, 0.1, tsdf.vertex_gray(c))
        tsdf.close()
        return used, ply

    # without --align-photo: the loop through the plain align, byte for byte
    for photo, al, out in ((False, al0, out0), (True, al1, out1)):
        used, ply = by_hand(photo)
        text = str(tmp_path / "by_hand.txt")
        fuse_map.write_poses(text, used)
        assert open(al).read() == open(text).read() and len(open(al).read().splitlines()) == N_VIEWS, photo
        assert open(out, "rb").read() == ply, photo
    # the last frame inside the wall
    plain, photo = fuse_map.read_poses(al0)[-1], fuse_map.read_poses(al1)[-1]
    e0, e1, e_file = _in_plane(plain, truth[-1]), _in_plane(photo, truth[-1]), _in_plane(T[-1], truth[-1])
    err = AR.pose_error(photo, truth[-1])
    print(f"last frame inside the wall: {e1[0]:.5f} m {e1[1]:.4f} degrees with --align-photo, {e0[0]:.5f} m {e0[1]:.4f} degrees with --align "
          f"alone, {e_file[0]:.5f} m {e_file[1]:.4f} degrees in the file; all six: {err[0]:.4f} degrees {err[1]:.5f} m")
    assert e1[0] < e0[0] and e1[1] < e0[1] and e1[0] < e_file[0] and e1[1] < e_file[1]


def test_align_photo_needs_align_and_gray(capsys):
    for args in (["--surface", "--align-photo", "0.03"], ["--surface", "--align", "--align-photo", "0.03"],
                 ["--surface", "--gray", "images", "--align-photo", "0.03"]):
        with pytest.raises(SystemExit) as ex:
            fuse_map.main(["maps", "poses.txt", "calib.txt", "out.ply"] + args)
        assert ex.value.code == 2
