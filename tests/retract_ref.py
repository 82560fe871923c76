"""The retract of fused frames from a TSDF map (include/viso_hip.h, "TSDF retract") restated in numpy on sorted entry arrays.  No
device and no library.

The updates of the retracted frames are those of the fuse's restatements: carve_ref.updates, which with the default options is
tsdf_ref's and gray_ref's fuse byte for byte (tests/test_tsdf_carve_cpu.py holds them to each other), and the entry arrays are
theirs.  What is restated here is rules 2 to 6: the subtraction per key in the table's modular arithmetic, the updates that find no
voxel, the weights taken below zero, the check of every voxel behind the take, the freeing, the counters and the report; and that a
refused call hands back what it was given."""
import numpy as np

import carve_ref
import gray_ref
import tsdf_ref
from map_ref import keys_of

REPORT = ("n_points", "n_updates", "n_missing", "n_underflow", "n_inconsistent", "n_freed")


def fuse(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, gray=False, **opts):
    """carve_ref.fuse: (every voxel of the map sorted by key, the counters).  frames: (map, pose), with gray (map, image, pose)."""
    return carve_ref.fuse(frames, param, voxel, trunc, min_disp16, capacity_log2, 1, gray, **opts)


def retract(entries, stats, frames, param, voxel=0.2, trunc=3, min_disp16=16, gray=False, **opts):
    """The map (entries: every voxel, sorted by key; stats: its five counters) with `frames` retracted, all in one call, with the
    options `opts` as the map's current ones.  Returns (entries, stats, report, ok): ok False is the refusal, and entries and stats
    are then the arguments themselves.  report["n_underflow"] is the number of voxels that underflow; the device's value is only
    zero or not zero with it."""
    dtype = gray_ref.ENTRY if gray else tsdf_ref.ENTRY
    assert entries.dtype == dtype and stats["n_dropped"] == 0
    have = keys_of(entries["k"].astype(np.int64))
    assert (np.diff(have) > 0).all()
    K, Q, W, G, n_points, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0, 0
    for m, image, pose in carve_ref._frames(frames, gray):
        k, q, w, g, n, o = carve_ref.updates(m, image, param, pose, voxel, trunc, min_disp16, **opts)
        K.append(k); Q.append(q); W.append(w); G.append(g); n_points += n; n_oor += o
    keys, q, w, g = (np.concatenate(v) for v in (K, Q, W, G))
    # rule 2: every update looks its voxel up; one that finds none changes nothing
    at = np.minimum(np.searchsorted(have, keys), max(len(have) - 1, 0))
    found = have[at] == keys if len(have) else np.zeros(len(keys), bool)
    at, q, w, g = at[found], q[found], w[found], g[found]
    dw, ds, dg = (np.zeros(len(have), np.int64) for _ in range(3))
    np.add.at(dw, at, w)
    np.add.at(ds, at, w * q)
    np.add.at(dg, at, w * g)
    assert (dw < 2 ** 32).all()
    weight = entries["weight"].astype(np.int64)
    underflow = dw > weight
    new_w = (weight - dw) % (1 << 32)                                           # modulo 2^32
    new_s = entries["sum"] - ds                                                 # int64: modulo 2^64 (no sum of a test comes near)
    new_g = (entries["gray"] if gray else np.zeros(len(have), np.uint64)) - dg.astype(np.uint64)   # uint64: modulo 2^64
    # rule 3: the check of every voxel of the table behind the take
    lim = trunc * 1024
    zero = new_w == 0
    rest = (new_s != 0) | (new_g != 0)
    beyond = (np.abs(new_s) > lim * new_w) | (new_g > np.uint64(255) * new_w.astype(np.uint64))
    report = dict(n_points=n_points, n_updates=len(keys), n_missing=int((~found).sum()), n_underflow=int(underflow.sum()),
                  n_inconsistent=int((zero & rest).sum() + (~zero & beyond).sum()), n_freed=int((zero & ~rest).sum()))
    if report["n_missing"] or report["n_underflow"] or report["n_inconsistent"]:
        return entries, stats, report, False
    out = entries[~zero].copy()
    out["weight"], out["sum"] = new_w[~zero], new_s[~zero]
    if gray:
        out["gray"] = new_g[~zero]
    st = dict(stats, n_points=stats["n_points"] - n_points, n_updates=stats["n_updates"] - len(keys),
              n_out_of_range=stats["n_out_of_range"] - n_oor, n_occupied=stats["n_occupied"] - report["n_freed"])
    assert min(st.values()) >= 0
    return out, st, report, True


def same_report(got, want):
    """A device report against the restatement's: equal, but for n_underflow, of which only zero or not zero is defined."""
    return all(got[k] == want[k] for k in REPORT if k != "n_underflow") and (got["n_underflow"] != 0) == (want["n_underflow"] != 0)
