"""python -m libviso_amd.fuse_map --distance-field on a directory of maps in the runners' format: the arrays of the file are those
of TsdfMap.distance_field on the same map and box."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map

from test_gpu_evict import WIN
from test_gpu_evict_tool import _tool, _tree

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ("--surface", "--mesh"))
def test_field_file_equals_the_direct_call(viso, tmp_path, mode):
    frames, prm, inputs = _tree(tmp_path)
    w = WIN["tsdf"]
    out, field = str(tmp_path / "out.ply"), str(tmp_path / "field.npz")
    text = _tool(inputs + [out, mode, "--voxel", str(w["voxel"]), "--min-disp", str(w["min_disp16"] / 16), "--capacity-log2", "14",
                           "--min-weight", "2", "--distance-field", field, "--field-half-side", "5.1"])
    assert "distance field of 52 x 52 x 52 voxels" in text and "clipped" not in text
    tsdf = libviso_amd.TsdfMap(None, voxel=w["voxel"], min_disp16=w["min_disp16"], capacity_log2=14)
    for m, _, pose in frames:
        tsdf.fuse(m, prm, pose=pose)
    box, clipped = fuse_map.field_box(frames[-1][2][:3, 3], 5.1, w["voxel"])
    want = tsdf.distance_field(box, min_weight=2)
    other = tsdf.distance_field(box, min_weight=1)
    tsdf.close()
    assert not clipped and want.n_sites > 100 and f"{want.n_sites} surface voxels" in text
    with np.load(field) as f:
        assert sorted(f.files) == ["lo", "sq", "state", "voxel"]
        sq, state, lo, voxel = f["sq"], f["state"], f["lo"], f["voxel"]
    assert sq.dtype == np.uint32 and state.dtype == np.uint8 and sq.shape == (52, 52, 52)
    assert sq.tobytes() == want.sq.tobytes() and state.tobytes() == want.state.tobytes()
    assert np.array_equal(lo, want.box[0]) and lo.dtype == np.int32 and float(voxel) == w["voxel"]
    assert state.tobytes() != other.state.tobytes()          # --min-weight reached the call
