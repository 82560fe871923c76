"""python -m libviso_amd.fuse_map DISPARITY_DIR POSES.txt CALIB.txt OUT.ply [--voxel V --min-count N --min-disp PX --frames B E]
                                 [--surface | --mesh [--trunc T --min-weight N] [--render DIR [--render-depth M]] [--gray IMAGE_DIR]
                                                     [--normals] [--shaded DIR]
                                                     [--align [--aligned-poses FILE --align-voxel-gate G --align-photo WEIGHT]]
                                                     [--carve VOXELS [--carve-near METRES]] [--depth-weights SHIFT[,MAX]]
                                                     [--distance-field FILE.npz [--field-half-side METRES]]
                                                     [--travel-field FILE.npz [--travel-clearance METRES] [--field-half-side METRES]]
                                                     [--repose NEW_POSES.txt]]
                                 [--window METRES [--archive FILE.npy]]

Fuses the maps a KITTI runner wrote with --disparity DIR and the poses of its pose file into one voxel map on the device
(libviso_amd.VoxelMap; include/viso_hip.h, "voxel map") and writes the occupied voxels as a binary PLY point cloud: x, y, z the
float32 centroid of each voxel, count the number of points fused into it.

  DISPARITY_DIR  16-bit grayscale PNGs named by image index (value / 16 = disparity in 1/16 px, 0 = invalid)
  POSES.txt      KITTI pose file: 12 numbers a line, the first three rows of the pose; line i belongs to the i-th map
  CALIB.txt      the sequence's calib.txt (lines P0: and P1:)
  --frames B E   only maps B .. E-1 of the directory (positions in name order), with their poses
  --surface      fuse into a TSDF map instead (libviso_amd.TsdfMap; include/viso_hip.h, "TSDF map") and write the points where the
                 averaged signed distance changes sign between neighbouring voxels: x, y, z the float32 crossing point, weight the
                 smaller of the two voxels' weights.  --trunc T: the truncation band in voxels (3); --min-weight N: only voxels
                 with at least this many updates (1).  --capacity-log2 then defaults to 26.
  --mesh         fuse into a TSDF map as --surface does, with its options, and write the surface as a triangle mesh by marching
                 tetrahedra (include/viso_hip.h, "TSDF mesh"): per vertex x, y, z and weight as above, per face three vertex
                 indices, the normals towards the cameras.  Not together with --surface.
  --render DIR   with --surface or --mesh: after fusing, also render the model at every pose that was fused, at the size of the
                 input maps, by ray casting (include/viso_hip.h, "TSDF render"; --min-weight applies), and write DIR/<name of the
                 input map> in the format of the input maps (a pixel rendered beyond 255.9 px, which the format cannot hold, is
                 written as invalid).  --render-depth M: how far a ray is followed, in metres (40).
  --gray IMAGE_DIR  with --surface or --mesh: fuse the left camera images with the maps (a gray TSDF map; include/viso_hip.h, "TSDF
                 intensity").  IMAGE_DIR holds 8-bit grayscale PNGs with the maps' names and sizes (KITTI's image_0).  The PLY's
                 vertices then carry the surface's intensity as red = green = blue after weight, and --render also writes
                 DIR/gray/<name> as 8-bit PNGs, the intensity of every rendered pixel (0 where the map is invalid).
  --normals      with --surface or --mesh: the PLY's vertices also carry the surface's unit normal, towards the cameras, as float nx,
                 ny, nz after x, y, z (include/viso_hip.h, "TSDF normals"; --min-weight applies); (0, 0, 0) where there is none, as
                 along the rim of the data.
  --shaded DIR   with --render: also write DIR/<name> as 8-bit PNGs, every rendered view shaded by the normals of its pixels under
                 a light at the camera (libviso_amd.shade_normals; 0 where the map is invalid or the pixel has no normal).
  --align        with --surface or --mesh: track, then fuse (include/viso_hip.h, "TSDF align").  The first map is fused at its pose;
                 every later map i is first aligned against the model fused so far, from the guess aligned(i-1) pose(i-1)^-1 pose(i)
                 (the file's motion applied to the previous map's aligned pose), and fused at the aligned pose when the alignment
                 ends with status >= 1, otherwise at that guess.  --align-voxel-gate G: the gate in voxels (1.0, at most --trunc);
                 --min-weight applies to the voxels the alignment reads.  --aligned-poses FILE: the poses the maps were fused at, in
                 the format of POSES.txt.  The statuses are counted in the tool's output.
  --align-photo WEIGHT  with --align and --gray: every used pixel also pulls the model's intensity to its own (include/viso_hip.h,
                 "TSDF photometric align"), which holds the motions that a flat scene leaves free.  WEIGHT: pixels of disparity per
                 gray level (the library's default is 0.03125).  Without it --align is the alignment on the distance alone.
  --carve VOXELS  with --surface or --mesh: every pixel's ray also updates the VOXELS voxels in front of its truncation band
                 (include/viso_hip.h, "TSDF fuse options"), so a surface that later maps look through (a stereo outlier, a car that
                 has driven away) leaves the model.  --carve-near METRES: free-space samples nearer to the camera than this are left
                 out (0).  Every carved voxel is at least one more update a pixel.
  --depth-weights SHIFT[,MAX]  with --surface or --mesh: an update weighs min(max(disp16^2 >> SHIFT, 1), MAX) and not 1 (MAX: 255),
                 so a near measurement pulls the average harder than a far one; --min-weight and the PLY's weight then are sums of
                 such weights.  Without --carve and --depth-weights the output is byte for byte what it was.
  --distance-field FILE.npz  with --surface or --mesh: after fusing, also write the distance field of the surface (include/viso_hip.h,
                 "TSDF distance field"; --min-weight applies) over the box of voxels that a cube of half side --field-half-side METRES
                 (20) around the last fused camera position touches, clipped to 512 voxels an axis around that position: sq (uint32
                 [n0][n1][n2], the squared distance to the nearest surface voxel of the box in voxels; 4294967295: none), state
                 (uint8: 0 unknown, 1 in front, 2 behind, +4 on the surface), lo (the box's first voxel) and voxel, as a numpy .npz.
  --travel-field FILE.npz  with --surface or --mesh: after fusing, also write the travel field (include/viso_hip.h, "TSDF travel
                 field"; --min-weight applies) over the box of --distance-field (--field-half-side METRES, 20) around the last fused
                 camera position, towards the first fused camera position as the goal, for a body that keeps --travel-clearance
                 METRES (0) from the surface.  Unknown voxels count as free, the optimistic field: the cameras themselves stand in
                 space that no map updated.  cost (uint32 [n0][n1][n2], thirds of a voxel along the cheapest <3,4,5> chamfer way;
                 4294967295: not free or no way), box (int32 [2][3]: lo, hi), voxel and, when the last camera position is reached,
                 path (int32 [m][3], the voxels of the way back from it to the goal), as a numpy .npz.
  --repose NEW_POSES.txt  with --surface or --mesh: the poses were corrected after the maps were fused (include/viso_hip.h, "TSDF
                 retract").  Every map is first fused at its pose in POSES.txt; then every map whose pose differs in NEW_POSES.txt
                 (as many lines) is retracted at the old pose and fused at the new one (TsdfMap.move), and OUT.ply, the renders
                 and the fields are written from the result: byte-identical to a run with NEW_POSES.txt as POSES.txt.  The number of
                 moved maps is printed.  Not together with --window (evicted voxels cannot be retracted) or --align.
  --window METRES  keep the map on the device to a cube of this half side around the camera (include/viso_hip.h, "Map eviction"):
                 before map i is fused (and, with --align, aligned), every voxel outside the box of voxels that the cube around the
                 translation of pose i touches leaves the table, on the device, and is appended to an archive on the host.  So a
                 table far smaller than the scene (--capacity-log2) follows the camera over any distance.  Without --surface or
                 --mesh, OUT.ply is written from the archive merged with the live voxels and is byte-identical to the run without
                 --window.  With --surface or --mesh, OUT.ply and the renders are of the live window at the end, and the model that
                 --align tracks against is the window: tracking in bounded memory.
  --archive FILE.npy  with --window: the evicted voxels, merged by key and sorted, as a numpy array of the map's entry dtype
                 (libviso_amd.merge_entries of it and of a map's entries is the unbounded map).

Both runners write byte-identical directories and pose files for every rank count and chunk size, so the PLY is identical too."""
import argparse
import os
import struct
import sys
import zlib

import numpy as np

DISP_INVALID = -16
FIELD_MAX_AXIS = 512  # the longest box of a distance field, in voxels
DISP_PNG_MAX = 4095   # the largest map value a 16-bit file holds (x 16)
RENDER_VIEWS = 16     # views of one --render call


def _read_png_gray(path, want_depth):
    """The bytes of a non-interlaced grayscale PNG of want_depth (8 or 16) bits as uint8 [rows][cols * want_depth / 8]; all five
    row filters.  ValueError for anything else."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, ihdr = 8, [], None
    while pos + 12 <= len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError(f"{path}: truncated chunk")
        if zlib.crc32(kind + body) != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if ihdr is None:
        raise ValueError(f"{path}: no IHDR chunk")
    cols, rows, depth, color, comp, filt, inter = ihdr
    if (depth, color, comp, filt, inter) != (want_depth, 0, 0, 0, 0) or rows < 1 or cols < 1:
        raise ValueError(f"{path}: only non-interlaced {want_depth}-bit grayscale PNGs are read")
    bpp = want_depth // 8
    stride = bpp * cols
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != rows * (stride + 1):
        raise ValueError(f"{path}: {raw.size} bytes of image data, expected {rows * (stride + 1)}")
    raw = raw.reshape(rows, stride + 1)
    out = np.zeros((rows, stride), np.uint8)
    zero = np.zeros(stride, np.int32)
    for y in range(rows):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else zero
        if ft == 0:
            rec = line
        elif ft == 2:
            rec = line + up
        elif ft in (1, 3, 4):   # the filters that look left: byte by byte, per channel of bpp bytes
            rec = np.zeros(stride, np.int32)
            for i in range(stride):
                a = int(rec[i - bpp]) if i >= bpp else 0
                b = int(up[i])
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = int(up[i - bpp]) if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                rec[i] = (int(line[i]) + pred) & 255
        else:
            raise ValueError(f"{path}: unknown row filter {ft}")
        out[y] = (rec & 255).astype(np.uint8)
    return out


def read_png16(path):
    """A non-interlaced 16-bit grayscale PNG as uint16 [rows][cols]; all five row filters.  ValueError for anything else."""
    return _read_png_gray(path, 16).view(">u2").astype(np.uint16)


def read_png8(path):
    """A non-interlaced 8-bit grayscale PNG (a camera image, KITTI's image_0) as uint8 [rows][cols]; all five row filters.
    ValueError for anything else."""
    return _read_png_gray(path, 8)


def read_disparity_png(path):
    """The runners' map as int16 in 1/16 px: value / 16, DISP_INVALID where the file has 0."""
    v = read_png16(path)
    d = (v // 16).astype(np.int16)
    d[v == 0] = DISP_INVALID
    return d


def _write_png_gray(path, rows, cols, depth, line_bytes):
    """line_bytes: uint8 [rows][cols * depth / 8], the big-endian samples of a grayscale PNG of `depth` bits (row filter 0)."""
    raw = np.zeros((rows, 1 + line_bytes.shape[1]), np.uint8)
    raw[:, 1:] = line_bytes

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, depth, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def write_png16(path, v):
    """uint16 [rows][cols] as a non-interlaced 16-bit grayscale PNG (row filter 0), which read_png16 reads back to the same array."""
    v = np.ascontiguousarray(v, np.uint16)
    if v.ndim != 2 or v.size == 0:
        raise ValueError("write_png16: a 2-D array with at least one pixel")
    rows, cols = v.shape
    _write_png_gray(path, rows, cols, 16, v.astype(">u2").view(np.uint8).reshape(rows, 2 * cols))


def write_png8(path, v):
    """uint8 [rows][cols] as a non-interlaced 8-bit grayscale PNG (row filter 0), which read_png8 reads back to the same array."""
    v = np.asarray(v)
    if v.dtype != np.uint8 or v.ndim != 2 or v.size == 0:
        raise ValueError("write_png8: a 2-D uint8 array with at least one pixel")
    _write_png_gray(path, v.shape[0], v.shape[1], 8, np.ascontiguousarray(v))


def write_disparity_png(path, d16):
    """An int16 map in 1/16 px in the runners' format: value = disparity x 256, 0 where the map is invalid.  A valid value is
    1 .. 4095 (the file's 16 bits end below 256 px), so no valid pixel is written as 0 and read_disparity_png reads the file back
    to the same array."""
    d16 = np.asarray(d16)
    if d16.dtype != np.int16 or ((d16 != DISP_INVALID) & ((d16 < 1) | (d16 > DISP_PNG_MAX))).any():
        raise ValueError(f"write_disparity_png: an int16 map whose valid values are 1 .. {DISP_PNG_MAX}")
    write_png16(path, np.where(d16 == DISP_INVALID, 0, d16.astype(np.int32) * 16).astype(np.uint16))


def read_poses(path):
    """[n][4][4] float64 from a KITTI pose file (12 numbers a line)."""
    out = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            if not line.strip():
                continue
            v = [float(t) for t in line.split()]
            if len(v) != 12:
                raise ValueError(f"{path}:{ln}: expected 12 numbers, found {len(v)}")
            T = np.eye(4)
            T[:3] = np.array(v).reshape(3, 4)
            out.append(T)
    return np.array(out).reshape(-1, 4, 4)


def write_poses(path, poses):
    """A KITTI pose file: the first three rows of every pose, 12 numbers a line, each written so that it reads back to the same
    double."""
    with open(path, "w") as f:
        for T in np.asarray(poses, np.float64).reshape(-1, 4, 4):
            f.write(" ".join("%.17g" % v for v in T[:3].reshape(-1)) + "\n")


def read_calib(path):
    """(f, cu, cv, base) from calib.txt's P0 and P1, as the runners take them."""
    P = {}
    with open(path) as f:
        for line in f:
            name, _, rest = line.partition(":")
            v = rest.split()
            if name.strip() in ("P0", "P1") and len(v) == 12:
                P[name.strip()] = np.array([float(t) for t in v]).reshape(3, 4)
    if "P0" not in P or "P1" not in P:
        raise ValueError(f"{path}: no P0: and P1: lines of 12 numbers")
    P1, P2 = P["P0"], P["P1"]
    return float(P1[0, 0]), float(P1[0, 2]), float(P1[1, 2]), float(abs(P2[0, 3] / P2[0, 0]))


def list_maps(directory):
    return sorted(n for n in os.listdir(directory) if n.lower().endswith(".png"))


def field_box(centre, half_side, voxel):
    """((lo, hi), clipped): libviso_amd.voxel_box of the cube around centre, every axis longer than FIELD_MAX_AXIS voxels cut to
    that many around the voxel that holds the centre."""
    import libviso_amd
    lo, hi = (v.astype(np.int64) for v in libviso_amd.voxel_box(centre, half_side, voxel))
    long = hi - lo > FIELD_MAX_AXIS
    mid = np.floor(np.asarray(centre, np.float64) / voxel).astype(np.int64)
    lo = np.where(long, np.maximum(mid - FIELD_MAX_AXIS // 2, -(1 << 31)), lo)
    hi = np.where(long, np.minimum(lo + FIELD_MAX_AXIS, (1 << 31) - 1), hi)
    return (lo, hi), bool(long.any())


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m libviso_amd.fuse_map", description=__doc__.split("\n\n")[1])
    ap.add_argument("disparity_dir"); ap.add_argument("poses"); ap.add_argument("calib"); ap.add_argument("out")
    ap.add_argument("--voxel", type=float, default=0.2, help="edge of a voxel in metres (0.2)")
    ap.add_argument("--min-count", type=int, default=1, help="only voxels with at least this many points (1)")
    ap.add_argument("--min-disp", type=float, default=1.0, help="smallest disparity used, in pixels (1.0)")
    ap.add_argument("--frames", type=int, nargs=2, metavar=("B", "E"), help="only maps B .. E-1 of the directory")
    ap.add_argument("--capacity-log2", type=int, default=None, help="log2 of the table's slots (24; 26 with --surface or --mesh)")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--surface", action="store_true", help="write the surface crossings of a TSDF map in place of the centroids")
    mode.add_argument("--mesh", action="store_true", help="write the triangle mesh of a TSDF map in place of the centroids")
    ap.add_argument("--trunc", type=int, default=3, help="with --surface or --mesh: the truncation band in voxels (3)")
    ap.add_argument("--min-weight", type=int, default=1, help="with --surface or --mesh: only voxels with at least this many updates (1)")
    ap.add_argument("--render", metavar="DIR", help="with --surface or --mesh: also write the model rendered at every fused pose into DIR")
    ap.add_argument("--render-depth", type=float, default=40.0, metavar="M", help="with --render: how far a ray is followed, metres (40)")
    ap.add_argument("--gray", metavar="IMAGE_DIR", help="with --surface or --mesh: fuse the 8-bit left images of the maps' names with them")
    ap.add_argument("--normals", action="store_true", help="with --surface or --mesh: write the vertices' normals into the PLY")
    ap.add_argument("--shaded", metavar="DIR", help="with --render: also write every rendered view shaded by its normals into DIR")
    ap.add_argument("--align", action="store_true", help="with --surface or --mesh: align every map against the model before it is fused")
    ap.add_argument("--aligned-poses", metavar="FILE", help="with --align: write the poses the maps were fused at")
    ap.add_argument("--align-voxel-gate", type=float, default=1.0, metavar="G", help="with --align: the gate in voxels (1.0)")
    ap.add_argument("--align-photo", type=float, default=None, metavar="WEIGHT", help="with --align and --gray: add the photometric row, "
                    "at this many pixels of disparity per gray level")
    ap.add_argument("--carve", type=int, default=None, metavar="VOXELS", help="with --surface or --mesh: also update this many voxels in front "
                    "of the truncation band of every ray")
    ap.add_argument("--carve-near", type=float, default=None, metavar="METRES", help="with --carve: leave out free-space samples nearer than this (0)")
    ap.add_argument("--depth-weights", default=None, metavar="SHIFT[,MAX]", help="with --surface or --mesh: an update weighs "
                    "min(max(disp16^2 >> SHIFT, 1), MAX), MAX 255")
    ap.add_argument("--distance-field", metavar="FILE.npz", help="with --surface or --mesh: also write the distance field of the surface "
                    "around the last fused camera position")
    ap.add_argument("--field-half-side", type=float, default=None, metavar="METRES", help="with --distance-field or --travel-field: the half side "
                    "of the box (20)")
    ap.add_argument("--travel-field", metavar="FILE.npz", help="with --surface or --mesh: also write the travel field around the last fused "
                    "camera position, the first fused camera position the goal")
    ap.add_argument("--travel-clearance", type=float, default=None, metavar="METRES", help="with --travel-field: how far the body keeps from the surface (0)")
    ap.add_argument("--window", type=float, default=None, metavar="METRES", help="keep the map to a cube of this half side around the camera; "
                    "what leaves it goes to an archive on the host (OUT.ply: the whole map without --surface or --mesh, else the live window)")
    ap.add_argument("--archive", metavar="FILE.npy", help="with --window: write the merged evicted voxels as a numpy array of entries")
    ap.add_argument("--repose", metavar="NEW_POSES.txt", help="with --surface or --mesh: once every map is fused at POSES, move every frame "
                    "whose pose differs in this file to its pose there (retract and fuse again), then write the output")
    a = ap.parse_args(argv)
    if a.repose and not (a.surface or a.mesh):
        ap.error("--repose needs --surface or --mesh (only a TSDF map lets go of a fused frame)")
    if a.repose and a.window is not None:
        ap.error("--repose does not go with --window (voxels that were evicted cannot be retracted)")
    if a.repose and a.align:
        ap.error("--repose does not go with --align (the frames are not fused at POSES then)")
    if a.archive and a.window is None:
        ap.error("--archive needs --window")
    fuse_options = {}
    if a.carve is not None or a.depth_weights is not None:
        if not (a.surface or a.mesh):
            ap.error("--carve and --depth-weights need --surface or --mesh (they are fuse options of a TSDF map)")
        if a.carve is not None:
            fuse_options["carve_voxels"] = a.carve
        if a.depth_weights is not None:
            try:
                shift, _, wmax = a.depth_weights.partition(",")
                fuse_options.update(weight_shift=int(shift), weight_max=int(wmax) if wmax else 255)
            except ValueError:
                ap.error("--depth-weights needs SHIFT or SHIFT,MAX, both integers")
    if a.carve_near is not None:
        if a.carve is None:
            ap.error("--carve-near needs --carve")
        fuse_options["carve_near"] = a.carve_near
    if a.window is not None and not (np.isfinite(a.window) and a.window >= 0):
        ap.error("--window needs a half side >= 0 in metres")
    if a.align and not (a.surface or a.mesh):
        ap.error("--align needs --surface or --mesh (only a TSDF map is aligned against)")
    if a.aligned_poses and not a.align:
        ap.error("--aligned-poses needs --align")
    if a.align_photo is not None and not (a.align and a.gray):
        ap.error("--align-photo needs --align and --gray (the photometric row reads a gray TSDF map and the maps' images)")
    if a.render and not (a.surface or a.mesh):
        ap.error("--render needs --surface or --mesh (only a TSDF map is rendered)")
    if a.normals and not (a.surface or a.mesh):
        ap.error("--normals needs --surface or --mesh (only a TSDF map has normals)")
    if a.shaded and not a.render:
        ap.error("--shaded needs --render DIR (the shaded images are of the rendered views)")
    if a.distance_field and not (a.surface or a.mesh):
        ap.error("--distance-field needs --surface or --mesh (only a TSDF map has a surface to be far from)")
    if a.travel_field and not (a.surface or a.mesh):
        ap.error("--travel-field needs --surface or --mesh (only a TSDF map has a surface to keep clear of)")
    if a.travel_clearance is not None and not a.travel_field:
        ap.error("--travel-clearance needs --travel-field")
    if a.travel_clearance is not None and not (np.isfinite(a.travel_clearance) and a.travel_clearance >= 0):
        ap.error("--travel-clearance needs a clearance >= 0 in metres")
    if a.field_half_side is not None and not (a.distance_field or a.travel_field):
        ap.error("--field-half-side needs --distance-field or --travel-field")
    if a.field_half_side is not None and not (np.isfinite(a.field_half_side) and a.field_half_side >= 0):
        ap.error("--field-half-side needs a half side >= 0 in metres")
    if a.gray and not (a.surface or a.mesh):
        ap.error("--gray needs --surface or --mesh (only a TSDF map carries intensity)")
    import libviso_amd
    from libviso_amd.abi import Param
    names, poses = list_maps(a.disparity_dir), read_poses(a.poses)
    if len(names) != len(poses):
        sys.exit(f"fuse_map: {len(names)} maps in {a.disparity_dir} but {len(poses)} poses in {a.poses}")
    b, e = a.frames if a.frames else (0, len(names))
    if not 0 <= b <= e <= len(names):
        sys.exit(f"fuse_map: --frames {b} {e} is outside the {len(names)} maps")
    new_poses = read_poses(a.repose) if a.repose else None
    if new_poses is not None and len(new_poses) != len(poses):
        sys.exit(f"fuse_map: {len(poses)} poses in {a.poses} but {len(new_poses)} in {a.repose}")
    f, cu, cv, base = read_calib(a.calib)
    prm = Param.default(base=base, f=f, cu=cu, cv=cv)
    archive = []   # --window: what left the map, in the order it left

    def evict_to_window(vmap, i):
        if a.window is not None:
            archive.append(vmap.evict(libviso_amd.voxel_box(poses[i][:3, 3], a.window, a.voxel)))

    def write_archive(dtype):
        if a.window is None:
            return ""
        n = sum(len(x) for x in archive)
        if a.archive:
            np.save(a.archive, libviso_amd.merge_entries(np.zeros(0, dtype), *archive))
        return f"; window of {a.window} m: {n} voxels evicted" + (f" -> {a.archive}" if a.archive else "")
    if a.surface or a.mesh:
        gray = bool(a.gray)
        tsdf = libviso_amd.TsdfMap(None, gray=gray, voxel=a.voxel, trunc_voxels=a.trunc, min_disp16=max(1, int(round(a.min_disp * 16))),
                                   capacity_log2=26 if a.capacity_log2 is None else a.capacity_log2, **fuse_options)
        try:
            shape = None
            used, statuses = [], {}   # --align: the poses the maps were fused at, and how the alignments ended
            for i in range(b, e):
                m = read_disparity_png(os.path.join(a.disparity_dir, names[i]))
                shape = shape or m.shape
                if a.render and m.shape != shape:
                    sys.exit(f"fuse_map: --render needs maps of one size, but {names[i]} is {m.shape[1]} x {m.shape[0]}")
                if gray:
                    image = read_png8(os.path.join(a.gray, names[i]))
                    if image.shape != m.shape:
                        sys.exit(f"fuse_map: {names[i]} is {image.shape[1]} x {image.shape[0]} in {a.gray} but its map is {m.shape[1]} x {m.shape[0]}")
                evict_to_window(tsdf, i)
                pose = poses[i]
                if a.align and used:
                    pose = used[-1] @ np.linalg.inv(poses[i - 1]) @ poses[i]
                    photo = {} if a.align_photo is None else dict(image=image, photo_weight=a.align_photo)
                    rec = tsdf.align(m, prm, pose, min_weight=a.min_weight, gate_voxels=a.align_voxel_gate, **photo)
                    statuses[int(rec["status"])] = statuses.get(int(rec["status"]), 0) + 1
                    if rec["status"] >= 1:
                        pose = rec["pose"].copy()
                used.append(pose)
                if gray:
                    tsdf.fuse(m, prm, pose=pose, image=image)
                else:
                    tsdf.fuse(m, prm, pose=pose)
            if new_poses is not None:
                moved = [i for i in range(b, e) if not np.array_equal(poses[i], new_poses[i])]
                for i in moved:   # the frame as it was fused, from its files again
                    m = read_disparity_png(os.path.join(a.disparity_dir, names[i]))
                    tsdf.move(m, prm, poses[i], new_poses[i], image=read_png8(os.path.join(a.gray, names[i])) if gray else None)
                print(f"fuse_map: {len(moved)} of {e - b} maps moved to their poses in {a.repose}")
                poses = new_poses   # --render and the fields see the model from where the frames are now
            st = tsdf.stats()
            note = write_archive(tsdf._evict_dtype())
            if a.align:
                if a.aligned_poses:
                    write_poses(a.aligned_poses, used)
                print(f"fuse_map: {max(0, e - b - 1)} maps aligned before they were fused (status: count " +
                      ", ".join(f"{k}: {v}" for k, v in sorted(statuses.items())) + ")" + (f" -> {a.aligned_poses}" if a.aligned_poses else ""))
                poses = np.array(list(poses[:b]) + used + list(poses[e:])).reshape(-1, 4, 4)   # --render sees the model from where it was fused
            if a.render and e > b:
                os.makedirs(os.path.join(a.render, "gray") if gray else a.render, exist_ok=True)
                if a.shaded:
                    os.makedirs(a.shaded, exist_ok=True)
                n_near = 0
                for i0 in range(b, e, RENDER_VIEWS):   # several views a call
                    i1 = min(e, i0 + RENDER_VIEWS)
                    views = (tsdf.normals if a.shaded else tsdf).render(prm, shape, poses[i0:i1], max_depth=a.render_depth,
                                                                        min_weight=a.min_weight, gray=gray)
                    if a.shaded:
                        views, lit = views[:-1] if gray else views[0], libviso_amd.shade_normals(views[-1])
                    views, shades = views if gray else (views, None)
                    near = views > DISP_PNG_MAX   # nearer than the files can say
                    n_near += int(near.sum())
                    views[near] = DISP_INVALID
                    for i in range(i0, i1):
                        write_disparity_png(os.path.join(a.render, names[i]), views[i - i0])
                        if gray:
                            write_png8(os.path.join(a.render, "gray", names[i]), np.where(near[i - i0], 0, shades[i - i0]).astype(np.uint8))
                        if a.shaded:
                            write_png8(os.path.join(a.shaded, names[i]), np.where(near[i - i0], 0, lit[i - i0]).astype(np.uint8))
                print(f"fuse_map: {e - b} views rendered to {a.render_depth} m ({n_near} pixels beyond 255.9 px left out) -> {a.render}")
            if a.distance_field and e > b:
                half = 20.0 if a.field_half_side is None else a.field_half_side
                box, clipped = field_box(poses[e - 1][:3, 3], half, a.voxel)
                field = tsdf.distance_field(box, min_weight=a.min_weight)
                np.savez(a.distance_field, sq=field.sq, state=field.state, lo=field.box[0], voxel=np.float64(a.voxel))
                print(f"fuse_map: distance field of {' x '.join(str(v) for v in field.sq.shape)} voxels, {field.n_sites} surface voxels" +
                      (f" (the box of {half} m clipped to {FIELD_MAX_AXIS} voxels an axis)" if clipped else "") + f" -> {a.distance_field}")
            if a.travel_field and e > b:
                half = 20.0 if a.field_half_side is None else a.field_half_side
                box, clipped = field_box(poses[e - 1][:3, 3], half, a.voxel)
                here, goal = (np.floor(poses[i][:3, 3] / a.voxel).astype(np.int64) for i in (e - 1, b))
                travel = tsdf.travel_field(box, [goal], clearance=a.travel_clearance or 0.0, min_weight=a.min_weight, unknown_is_site=False)
                way = travel.path(here)
                arrays = dict(cost=travel.cost, box=np.stack(travel.box), voxel=np.float64(a.voxel))
                if way is not None:
                    arrays["path"] = way
                np.savez(a.travel_field, **arrays)
                print(f"fuse_map: travel field of {' x '.join(str(v) for v in travel.cost.shape)} voxels, {travel.n_reached} reached in "
                      f"{travel.rounds} rounds, " + ("the goal is not free" if not travel.n_goals_used else "no way back" if way is None else
                                                    f"the way back has {len(way)} voxels, {float(travel.cost[tuple(here - box[0])]) / 3 * a.voxel:.2f} m") +
                      (f" (the box of {half} m clipped to {FIELD_MAX_AXIS} voxels an axis)" if clipped else "") + f" -> {a.travel_field}")
            shade = None   # the intensity of the PLY's vertices
            if a.mesh:
                vertices, triangles = tsdf.mesh(a.min_weight)
                shade = tsdf.vertex_gray(vertices) if gray else None
                normals = tsdf.normals.vertices(vertices, a.min_weight) if a.normals else None
            else:
                crossings = tsdf.surface(a.min_weight)
                shade = tsdf.vertex_gray(crossings) if gray else None
                normals = tsdf.normals.vertices(crossings, a.min_weight) if a.normals else None
        finally:
            tsdf.close()
        if a.mesh:
            if normals is not None:
                libviso_amd.write_mesh_normals_ply(a.out, vertices, triangles, normals, shade)
            else:
                libviso_amd.write_mesh_ply(a.out, vertices, triangles, shade)
            print(f"fuse_map: {e - b} maps, {st['n_points']} points, {st['n_updates']} updates ({st['n_out_of_range']} samples out of range), "
                  f"{st['n_occupied']} voxels, {len(vertices)} vertices and {len(triangles)} triangles at weight >= {a.min_weight} -> {a.out}{note}")
            return 0
        if normals is not None:
            libviso_amd.write_surface_normals_ply(a.out, crossings, a.voxel, normals, shade)
        else:
            libviso_amd.write_surface_ply(a.out, crossings, a.voxel, shade)
        print(f"fuse_map: {e - b} maps, {st['n_points']} points, {st['n_updates']} updates ({st['n_out_of_range']} samples out of range), "
              f"{st['n_occupied']} voxels, {len(crossings)} crossings at weight >= {a.min_weight} -> {a.out}{note}")
        return 0
    vmap = libviso_amd.VoxelMap(None, voxel=a.voxel, min_disp16=max(1, int(round(a.min_disp * 16))),
                                capacity_log2=24 if a.capacity_log2 is None else a.capacity_log2)
    try:
        for i in range(b, e):
            evict_to_window(vmap, i)
            vmap.fuse(read_disparity_png(os.path.join(a.disparity_dir, names[i])), prm, pose=poses[i])
        st = vmap.stats()
        if a.window is None:
            entries = vmap.entries(a.min_count)
        else:   # the whole map: what left merged with what is live
            entries = libviso_amd.merge_entries(*archive, vmap.entries())
            st["n_occupied"] = len(entries)
            entries = entries[entries["count"] >= a.min_count]
    finally:
        vmap.close()
    note = write_archive(entries.dtype)
    libviso_amd.write_map_ply(a.out, entries, a.voxel)
    print(f"fuse_map: {e - b} maps, {st['n_points']} points ({st['n_out_of_range']} out of range), {st['n_occupied']} voxels, "
          f"{len(entries)} with count >= {a.min_count} -> {a.out}{note}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
