"""python -m libviso_amd.fuse_map --surface --align on a small synthetic directory: five views of the three-plane scene of
tests/align_cases.py, ray cast exactly, with a pose file that carries a steady drift.  The poses the tool writes equal those of the
same loop through TsdfMap.align and TsdfMap.fuse, as the file's text; the final frame's pose is nearer the scene's truth with
--align than without it; and without --align the PLY is what the restatement (tests/tsdf_ref.py) gives for the drifted poses, as
before the option existed."""
import os

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath
from libviso_amd.abi import Param

import align_cases as AC
import align_ref as AR
import tsdf_ref as R

pytestmark = pytest.mark.gpu

N_VIEWS = 5
DRIFT = [0.0015, -0.0020, 0.0010, 0.012, -0.008, 0.015]   # a frame: 0.15 degrees and 0.02 m


def _scene(tmp_path):
    prm = AC.param()
    truth = [AC.view(0.004 * i, -0.006 * i, 0.002 * i, 0.03 * i, -0.01 * i, 0.10 * i) for i in range(N_VIEWS)]
    drifted, D = [], np.eye(4)
    for T in truth:
        drifted.append(T @ D)
        D = D @ hostmath.tr2mat(DRIFT)
    d = tmp_path / "disp"
    d.mkdir()
    maps = [AC.raycast(T) for T in truth]
    for i, m in enumerate(maps):
        fuse_map.write_disparity_png(str(d / ("%06d.png" % i)), m)
    poses, calib = str(tmp_path / "poses.txt"), str(tmp_path / "calib.txt")
    fuse_map.write_poses(poses, drifted)
    P0 = [prm.f, 0.0, prm.cu, 0.0, 0.0, prm.f, prm.cv, 0.0, 0.0, 0.0, 1.0, 0.0]
    P1 = list(P0)
    P1[3] = -prm.f * prm.base
    with open(calib, "w") as f:
        for name, P in (("P0", P0), ("P1", P1)):
            f.write(name + ": " + " ".join("%.17g" % v for v in P) + "\n")
    return str(d), poses, calib, maps, truth


def test_align_mode_tracks_then_fuses_and_plain_surface_is_unchanged(viso, tmp_path, capsys):
    d, poses, calib, maps, truth = _scene(tmp_path)
    common = ["--surface", "--voxel", "0.1", "--capacity-log2", "18"]
    out0, out1, aligned = str(tmp_path / "plain.ply"), str(tmp_path / "aligned.ply"), str(tmp_path / "aligned.txt")
    assert fuse_map.main([d, poses, calib, out0] + common) == 0
    assert fuse_map.main([d, poses, calib, out1] + common + ["--align", "--aligned-poses", aligned, "--align-voxel-gate", "2"]) == 0
    text = capsys.readouterr().out
    assert "4 maps aligned before they were fused (status: count 1: 4)" in text, text
    # what the tool reads back from its own input
    T = fuse_map.read_poses(poses)
    f, cu, cv, base = fuse_map.read_calib(calib)
    prm = Param.default(base=base, f=f, cu=cu, cv=cv)
    back = [fuse_map.read_disparity_png(os.path.join(d, n)) for n in fuse_map.list_maps(d)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(back, maps))
    # without --align: the restatement of the fuse at the file's poses
    want, st = R.fuse(list(zip(maps, T)), prm, 0.1, 3, 16, 18)
    assert st["n_dropped"] == 0 and st["n_out_of_range"] == 0
    assert open(out0, "rb").read() == R.ply_bytes(R.crossings(want), 0.1)
    assert open(out1, "rb").read() != open(out0, "rb").read()
    # the same loop by hand
    tsdf = libviso_amd.TsdfMap(None, voxel=0.1, capacity_log2=18)
    used = []
    for i, m in enumerate(maps):
        pose = T[i]
        if used:
            pose = used[-1] @ np.linalg.inv(T[i - 1]) @ T[i]
            rec = tsdf.align(m, prm, pose, min_weight=1, gate_voxels=2.0)
            assert rec["status"] == 1
            pose = rec["pose"].copy()
        used.append(pose)
        tsdf.fuse(m, prm, pose=pose)
    by_hand = str(tmp_path / "by_hand.txt")
    fuse_map.write_poses(by_hand, used)
    assert open(aligned).read() == open(by_hand).read() and len(open(aligned).read().splitlines()) == N_VIEWS
    assert open(out1, "rb").read() == libviso_amd.surface_ply_bytes(tsdf.surface(1), 0.1)
    tsdf.close()
    # the last frame against the truth
    got = fuse_map.read_poses(aligned)
    assert np.array_equal(got[0], T[0]) and np.array_equal(got[-1][:3], used[-1][:3])
    with_align, without = AR.pose_error(got[-1], truth[-1]), AR.pose_error(T[-1], truth[-1])
    print(f"last frame: {with_align[0]:.4f} degrees {with_align[1]:.5f} m with --align, {without[0]:.4f} degrees {without[1]:.5f} m without")
    assert with_align[0] < without[0] and with_align[1] < without[1]


def test_align_needs_a_tsdf_map(capsys):
    for args in (["--align"], ["--surface", "--aligned-poses", "x.txt"]):
        with pytest.raises(SystemExit) as ex:
            fuse_map.main(["maps", "poses.txt", "calib.txt", "out.ply"] + args)
        assert ex.value.code == 2
