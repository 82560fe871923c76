"""python -m libviso_amd.fuse_map --travel-field on a directory of maps in the runners' format: the cost of the file is the
restatement's (tests/travel_ref.py) on the same map, box, goal and clearance, and the stored way back from the last camera to the
first keeps the path rule.

Input condition, asserted on the restatement: the last camera's voxel is reached, and the surface is in the way of some cells (the
clearance takes free cells away)."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map

import travel_ref as T
from test_gpu_evict import WIN
from test_gpu_evict_tool import _tool, _tree
from test_travel_cpu import check_path

pytestmark = pytest.mark.gpu

FRAMES, HALF, CLEARANCE = (9, 12), 5.1, 0.3


def test_travel_file_equals_the_restatement(viso, tmp_path):
    frames, prm, inputs = _tree(tmp_path)
    w = WIN["tsdf"]
    out, field = str(tmp_path / "out.ply"), str(tmp_path / "travel.npz")
    text = _tool(inputs + [out, "--surface", "--voxel", str(w["voxel"]), "--min-disp", str(w["min_disp16"] / 16), "--capacity-log2", "14",
                           "--min-weight", "1", "--frames", str(FRAMES[0]), str(FRAMES[1]), "--travel-field", field, "--travel-clearance",
                           str(CLEARANCE), "--field-half-side", str(HALF)])
    assert "travel field of 52 x 52 x 52 voxels" in text and "clipped" not in text and "the way back has" in text
    tsdf = libviso_amd.TsdfMap(None, voxel=w["voxel"], min_disp16=w["min_disp16"], capacity_log2=14)
    for m, _, pose in frames[FRAMES[0]:FRAMES[1]]:
        tsdf.fuse(m, prm, pose=pose)
    entries = tsdf.entries()
    tsdf.close()
    box, clipped = fuse_map.field_box(frames[FRAMES[1] - 1][2][:3, 3], HALF, w["voxel"])
    here, goal = (np.floor(frames[i][2][:3, 3] / w["voxel"]).astype(np.int64) for i in (FRAMES[1] - 1, FRAMES[0]))
    clearance_sq = libviso_amd.travel_clearance_sq(CLEARANCE, w["voxel"])
    assert not clipped and clearance_sq == 3                           # 1.5 voxels: 2.25, up to 3
    cost, sq, st, used, reached = T.travel(entries, 1, box, 0, clearance_sq, [goal])
    lo = np.asarray(box[0])
    free = T.free_of(sq, st, 0, clearance_sq)
    assert used == 1 and cost[tuple(here - lo)] != T.NONE and 100 < (~free).sum() < free.size and (~free & (sq > 0) & ((st & 3) != 2)).any()
    with np.load(field) as f:
        assert sorted(f.files) == ["box", "cost", "path", "voxel"]
        got, got_box, way, voxel = f["cost"], f["box"], f["path"], f["voxel"]
    assert got.dtype == np.uint32 and got.shape == (52, 52, 52) and np.array_equal(got, cost)
    assert got_box.dtype == np.int32 and np.array_equal(got_box, np.stack(box)) and float(voxel) == w["voxel"]
    assert f"{reached} reached" in text and f"the way back has {len(way)} voxels" in text
    assert way.dtype == np.int32 and np.array_equal(way[0], here) and np.array_equal(way[-1], goal)
    check_path(way - lo, cost, free, tuple(here - lo))
    assert np.array_equal(way - lo, T.path(cost, here - lo))
