"""numpy restatement of the opt-in rectification (include/viso_hip.h, viso_rectify_map / viso_batch_set_rectify): the map
builder in the header's form, the host quantisation and the integer remap of rectify_remap_kernel."""
import numpy as np


def rectify_map(K, D, R, P, out_shape):
    """The plumb-bob map of one camera, straight from the header's formula (float64, then float32)."""
    K, R, P = (np.asarray(a, np.float64).reshape(3, -1) for a in (K, R, P))
    k1, k2, p1, p2, k3 = np.asarray(D, np.float64)
    rows, cols = out_shape
    iR = np.linalg.inv(P[:, :3] @ R)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    X = iR[0, 0] * x + iR[0, 1] * y + iR[0, 2]
    Y = iR[1, 0] * x + iR[1, 1] * y + iR[1, 2]
    W = iR[2, 0] * x + iR[2, 1] * y + iR[2, 2]
    xp, yp = X / W, Y / W
    r2 = xp * xp + yp * yp
    kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xp * kr + 2 * p1 * xp * yp + p2 * (r2 + 2 * xp * xp)
    yd = yp * kr + p1 * (r2 + 2 * yp * yp) + 2 * p2 * xp * yp
    return (K[0, 0] * xd + K[0, 2]).astype(np.float32), (K[1, 1] * yd + K[1, 2]).astype(np.float32)


def quantise(mapx, mapy):
    """(ix, iy, fx, fy, outside): X = lrintf(map * 32) (ties to even), ix = X >> 5, fx = X & 31; outside = not finite or
    |map| >= 32768 (int64 arrays; ix .. fy are 0 where outside)."""
    mx, my = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    with np.errstate(invalid="ignore"):
        outside = ~(np.isfinite(mx) & np.isfinite(my) & (np.abs(mx) < 32768) & (np.abs(my) < 32768))
    X = np.where(outside, 0, np.rint(np.where(outside, 0, mx) * np.float32(32))).astype(np.int64)
    Y = np.where(outside, 0, np.rint(np.where(outside, 0, my) * np.float32(32))).astype(np.int64)
    return X >> 5, Y >> 5, X & 31, Y & 31, outside


def remap(raw, mapx, mapy, border=0):
    """The integer bilinear remap of one raw image (rows x cols uint8) through one map: uint8 of the map's shape."""
    raw = np.asarray(raw, np.uint8)
    rows, cols = raw.shape
    ix, iy, fx, fy, outside = quantise(mapx, mapy)

    def tap(a, b):
        x, y = ix + a, iy + b
        ok = (x >= 0) & (x < cols) & (y >= 0) & (y < rows) & ~outside
        return np.where(ok, raw[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)].astype(np.int64), border)

    s = ((32 - fx) * (32 - fy) * tap(0, 0) + fx * (32 - fy) * tap(1, 0) + (32 - fx) * fy * tap(0, 1) + fx * fy * tap(1, 1) + 512) >> 10
    assert s.max(initial=0) <= 255
    return s.astype(np.uint8)


def maps_of(calib):
    """[(mapx, mapy)] per camera of a synth.raw_stereo_calib dict, built by this restatement."""
    return [rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], calib["out_shape"]) for s in (0, 1)]


def rectify_sequence(images, maps, border=0):
    """[nf][2][raw_rows][raw_cols] -> [nf][2][out_rows][out_cols] with maps [(mapx, mapy)] per side."""
    nf = images.shape[0]
    out = np.empty((nf, 2) + maps[0][0].shape, np.uint8)
    for t in range(nf):
        for s in (0, 1):
            out[t, s] = remap(images[t, s], maps[s][0], maps[s][1], border)
    return out


def write_cam_to_cam(path, calib, drop=None, extra_value=None):
    """A KITTI raw calib_cam_to_cam.txt for a synth.raw_stereo_calib dict (camera 00 = left, 01 = right; %.17g: the parser
    reads back the same doubles).  drop: a key to leave out; extra_value: a key that gets one number too many."""
    def row(v):
        return " ".join("%.17g" % x for x in np.asarray(v, np.float64).reshape(-1))
    rr, rc = calib["raw_shape"]
    orows, ocols = calib["out_shape"]
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for c in (0, 1):
        i = "%02d" % c
        for key, v in (("S_" + i, [rc, rr]), ("K_" + i, calib["K"][c]), ("D_" + i, calib["D"][c]), ("R_" + i, np.eye(3)),
                       ("T_" + i, [0.0, 0.0, 0.0]), ("S_rect_" + i, [ocols, orows]), ("R_rect_" + i, calib["R"][c]),
                       ("P_rect_" + i, calib["P"][c])):
            if key == drop:
                continue
            vals = list(np.asarray(v, np.float64).reshape(-1)) + ([1.0] if key == extra_value else [])
            lines.append(key + ": " + row(vals))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path
