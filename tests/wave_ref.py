"""numpy lane models of the cross-lane helpers of libviso_amd/csrc/wave.h (wave64): dpp() moves an array of 64 lane values as one
DPP instruction does, and every reduction, scan and exchange of the header is restated from it, step by step, in the header's
order.  tests/test_dev_harness_cpu.py pins dpp() against source-lane tables written out by hand and the restatements against
numpy's own reductions; tests/test_gpu_dev_helpers.py compares the device with them bit for bit."""
import numpy as np

WAVE = 64
WAVE_STEPS = ((0x111, 0xF), (0x112, 0xF), (0x114, 0xF), (0x118, 0xF), (0x142, 0xA), (0x143, 0xC))   # VISO_WAVE_STEPS


def dpp_source(ctrl):
    """The lane each of the 64 lanes reads under DPP control `ctrl`; -1: the lane has no source."""
    src = np.full(WAVE, -1, np.int64)
    for lane in range(WAVE):
        row, r = lane & ~15, lane & 15
        if 0x00 <= ctrl <= 0xFF:                       # quad_perm
            s = (lane & ~3) | ((ctrl >> (2 * (lane & 3))) & 3)
        elif 0x101 <= ctrl <= 0x10F:                   # row_shl:n  (lane <- lane + n of its row)
            s = lane + (ctrl & 15) if r + (ctrl & 15) < 16 else -1
        elif 0x111 <= ctrl <= 0x11F:                   # row_shr:n  (lane <- lane - n of its row)
            s = lane - (ctrl & 15) if r >= (ctrl & 15) else -1
        elif 0x121 <= ctrl <= 0x12F:                   # row_ror:n
            s = row | ((r - (ctrl & 15)) & 15)
        elif ctrl == 0x130:                            # wave_shl:1
            s = lane + 1 if lane < 63 else -1
        elif ctrl == 0x138:                            # wave_shr:1
            s = lane - 1
        elif ctrl == 0x140:                            # row_mirror
            s = row | (15 - r)
        elif ctrl == 0x141:                            # row_half_mirror
            s = (lane & ~7) | (7 - (lane & 7))
        elif ctrl == 0x142:                            # row_bcast:15: lane 15 of a row to the next row
            s = row - 1
        elif ctrl == 0x143:                            # row_bcast:31: lane 31 to rows 2 and 3
            s = 31 if lane >= 32 else -1
        else:
            raise ValueError("DPP control 0x%x is not modelled" % ctrl)
        src[lane] = s
    return src


def dpp(v, ctrl, row_mask=0xF, old=0, bound_ctrl=False):
    """update_dpp(old, v, ctrl, row_mask, 0xf, bound_ctrl) over 64 lanes: a lane of a row inside row_mask takes its source lane's
    value, or, without a source, `old` (0 under bound_ctrl); the lanes of a row outside row_mask keep `old`."""
    v = np.asarray(v)
    assert v.shape == (WAVE,)
    out = np.empty_like(v)
    out[:] = old
    src = dpp_source(ctrl)
    for lane in range(WAVE):
        if not (row_mask >> (lane >> 4)) & 1:
            continue
        if src[lane] >= 0:
            out[lane] = v[src[lane]]
        elif bound_ctrl:
            out[lane] = 0
    return out


def swizzle(v, pat):
    """ds_swizzle in bitmask mode: lane' = ((lane & and) | or) ^ xor inside each half of 32 lanes."""
    v = np.asarray(v)
    a, o, x = pat & 31, (pat >> 5) & 31, (pat >> 10) & 31
    lane = np.arange(WAVE)
    return v[(lane & 32) | ((((lane & 31) & a) | o) ^ x)]


def _steps(v, op, ident):
    with np.errstate(over="ignore", invalid="ignore"):
        for ctrl, mask in WAVE_STEPS:
            v = op(v, dpp(v, ctrl, mask, ident))
    return v


def wave_min63(v):
    v = np.asarray(v)
    return _steps(v, np.minimum, ~np.zeros((), v.dtype))   # unsigned: all ones


def wave_max63(v):
    return _steps(np.asarray(v), np.maximum, 0)


def wave_scan(v):
    """viso_wave_scan / viso_wave_sum63 (integers, wrapping) and viso_wave_fsum63 / wave_sum_to_lane63 (floats, this order)."""
    return _steps(np.asarray(v), np.add, 0)


def wave_max_keep(v):
    """wave_max_u32's steps: a lane without a source keeps its own value (old = v)."""
    v = np.asarray(v)
    for ctrl, mask in WAVE_STEPS:
        v = np.maximum(v, np.where(_has_source(ctrl, mask), dpp(v, ctrl, mask, 0), v))
    return v


def _has_source(ctrl, mask):
    return (dpp_source(ctrl) >= 0) & (((mask >> (np.arange(WAVE) >> 4)) & 1) == 1)


def row_min(v):
    v = np.asarray(v)
    for ctrl in (0xB1, 0x4E, 0x141, 0x140):
        v = np.minimum(v, dpp(v, ctrl, 0xF, ~np.zeros((), v.dtype)))
    return v


def wave_min_all(v):
    """wave_min_u32: rows by exchanges, then the two row broadcasts; the value of lane 63 to every lane."""
    v = row_min(v)
    v = np.minimum(v, dpp(v, 0x142, 0xA, ~np.zeros((), v.dtype)))
    v = np.minimum(v, dpp(v, 0x143, 0xC, ~np.zeros((), v.dtype)))
    return np.full(WAVE, v[63], v.dtype)


def wave_max_u64(v):
    v = np.asarray(v, np.uint64)
    hi, lo = (v >> np.uint64(32)).astype(np.uint32), (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    mh = wave_max_keep(hi)[63]
    ml = wave_max_keep(np.where(hi == mh, lo, np.uint32(0)))[63]
    return np.full(WAVE, (np.uint64(mh) << np.uint64(32)) | np.uint64(ml), np.uint64)


def group_sum(v, lanes):
    v = np.asarray(v)
    with np.errstate(over="ignore"):
        v = v + dpp(v, 0xB1)
        v = v + dpp(v, 0x4E)
        if lanes == 8:
            v = v + dpp(v, 0x141)
    return v


def _fext2(a, b, is_max):
    """fminf / fmaxf: a NaN operand is ignored; NaN only when both are."""
    return np.fmax(a, b) if is_max else np.fmin(a, b)


def wave_fext(v, is_max):
    """viso_wave_fext: the exchanges inside the rows, then the four rows' values.  The value only: where +0 and -0 tie, fminf /
    fmaxf promise no sign."""
    v = np.asarray(v, np.float32)
    for ctrl in (0xB1, 0x4E, 0x141, 0x140):
        v = _fext2(v, dpp(v, ctrl, 0xF, np.float32(0)), is_max)
    a, b, c, d = v[0], v[16], v[32], v[48]
    return np.full(WAVE, _fext2(_fext2(a, b, is_max), _fext2(c, d, is_max), is_max), np.float32)


def block_sum(acc, waves):
    """block_sum<NS, WAVES>: acc [waves * 64, NS] -> tot [NS]; every wave by the six steps, then the waves in order."""
    acc = np.asarray(acc)
    tot = np.empty(acc.shape[1], acc.dtype)
    for k in range(acc.shape[1]):
        red = [wave_scan(acc[w * WAVE:(w + 1) * WAVE, k])[63] for w in range(waves)]
        s = red[0]
        for w in range(1, waves):
            s = s + red[w]
        tot[k] = s
    return tot


def pack_block_sums(v):
    """match_dev.h pack_block_sums: the four 16-lane sums, clamped to int16, biased by 32768, as two dwords."""
    v = np.asarray(v, np.int64).reshape(4, 16).sum(axis=1)
    v = ((v + 2 ** 31) % 2 ** 32) - 2 ** 31                    # the device adds in int32
    s = (np.clip(v, -32768, 32767) + 32768).astype(np.uint32)
    return np.uint32(s[0] | (s[1] << 16)), np.uint32(s[2] | (s[3] << 16))


def row8(v, s):
    """The plane byte of element v at shift s: clip(v + (128 << s), 0, (256 << s) - 1) >> s."""
    v = np.asarray(v, np.int64)
    return (np.clip(v + (128 << s), 0, (256 << s) - 1) >> s).astype(np.uint32)


def bitonic_cw(header_text):
    """The comparators per wave and stage of bitonic_sort_lds, read from match_dev.h: its `const int cw = A ? B : C;` as a
    function of (half, threads)."""
    import re
    cond, yes, no = re.search(r"const int cw = (.+?) \? (.+?) : (.+?);", header_text).groups()
    expr = "(%s) if (%s) else (%s)" % (yes.replace("/", "//"), cond, no)
    return lambda half, threads: eval(expr, {"min": min, "max": max}, {"half": half, "THREADS": threads, "NW": threads // 64})


def bitonic_stages(threads, npad, cw_of):
    """The loops of bitonic_sort_lds<threads>(keys, npad), restated: per stage (k, j) the key indices (i, l = i + j) of every
    comparator that runs, and whether it sorts upwards; cw_of(half, threads): the header's comparators per wave and stage."""
    nw = threads // 64
    half = npad >> 1
    cw = cw_of(half, threads)
    k, lk = 2, 1
    while k <= npad:
        j, lj = k >> 1, lk - 1
        while j > 0:
            t = np.concatenate([w * cw + np.arange(cw) for w in range(nw) if w * cw < half])   # (m = lane, lane + 64, .. < cw)
            i = ((t >> lj) << (lj + 1)) + (t & (j - 1))
            yield i, i + j, (i & k) == 0
            j >>= 1
            lj -= 1
        k <<= 1
        lk += 1


def bitonic_sort_model(keys, threads, cw_of):
    """The network applied to keys (a power of two of them): what the restated loops leave."""
    keys = np.array(keys)
    for i, l, up in bitonic_stages(threads, len(keys), cw_of):
        a, b = keys[i], keys[l]
        swap = (a > b) == up
        keys[i], keys[l] = np.where(swap, b, a), np.where(swap, a, b)
    return keys


def splitmix64(s):
    """viso_splitmix64 on Python integers: (the output, the advanced state)."""
    M = (1 << 64) - 1
    s = (s + 0x9E3779B97F4A7C15) & M
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31), s


def map_hash(k):
    M = (1 << 64) - 1
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & M
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & M
    k ^= k >> 31
    return k & 0xFFFFFFFF
