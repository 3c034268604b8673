"""Host mirror of the point-cloud rasteriser (csrc/render.hip, pdgn_render_sheet): the same projection order, depth
quantisation and key in numpy, the per-pixel minimum with np.minimum.at.  Test infrastructure: the product never imports it.

Layout (include/pdgn_hip.h): u, v, d = fma(m2, z, fma(m1, y, fma(m0, x, m3))) per view row; pixel (floor(u), floor(v)) inside
the cloud's own cell; q = min(uint32(clamp(d, 0, 1) * 2^24), 2^24 - 1); key = q << 8 | (255 - (q >> 17)); every pixel of the
disc dx^2 + dy^2 <= r^2 that lies inside the cell takes the minimum; untouched pixels are 0, the others the key's low byte."""
import numpy as np

EMPTY = np.uint32(0xFFFFFFFF)
BACKGROUND = 0


def _fma(a, b, c, dtype):
    """a * b + c with one rounding to `dtype`: the product of two fp32 values is exact in fp64 (fp32 mode: the fp64 sum is
    rounded once more, which differs from the fused result only on double-rounding ties; exact inputs have none)."""
    r = np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
    return r.astype(dtype)


def project(pts, view, dtype=np.float32):
    """pts (..., 3), view (3, 4) -> u, v, d in `dtype`, the kernel's order of operations."""
    pts = np.asarray(pts, dtype=dtype)
    m = np.asarray(view, dtype=dtype)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    return tuple(_fma(m[r, 2], z, _fma(m[r, 1], y, _fma(m[r, 0], x, m[r, 3], dtype), dtype), dtype) for r in range(3))


def point_keys(pts, view, dtype=np.float32):
    """-> (iu, iv, key, valid): the pixel inside the cell (int64, may lie outside it) and the uint32 key of every point."""
    u, v, d = project(pts, view, dtype)
    valid = np.isfinite(u) & np.isfinite(v) & ~np.isnan(d)
    iu = np.floor(np.where(valid, u, 0)).astype(np.int64)
    iv = np.floor(np.where(valid, v, 0)).astype(np.int64)
    dc = np.clip(np.where(valid, d, 0), 0, 1).astype(dtype)
    q = np.minimum((dc * dtype(16777216.0)).astype(np.int64), 0xFFFFFF).astype(np.uint32)
    key = (q << np.uint32(8)) | (np.uint32(255) - (q >> np.uint32(17)))
    return iu, iv, key, valid


def sheet_keys(clouds, view, cell, radius, dtype=np.float32):
    """clouds: list of (B, N_c, 3) arrays -> (B * cell, len(clouds) * cell) uint32 keys."""
    B = clouds[0].shape[0]
    keys = np.full((B * cell, len(clouds) * cell), EMPTY, dtype=np.uint32)
    for c, pts in enumerate(clouds):
        iu, iv, key, valid = point_keys(pts, view, dtype)
        row0 = (np.arange(B, dtype=np.int64) * cell).reshape(B, 1)
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                if dx * dx + dy * dy > radius * radius:
                    continue
                px, py = iu + dx, iv + dy
                ok = valid & (px >= 0) & (px < cell) & (py >= 0) & (py < cell)
                np.minimum.at(keys, ((row0 + py)[ok], (c * cell + px)[ok]), key[ok])
    return keys


def resolve(keys):
    return np.where(keys == EMPTY, BACKGROUND, keys & np.uint32(0xFF)).astype(np.uint8)


def render(clouds, view, cell, radius, dtype=np.float32):
    return resolve(sheet_keys(clouds, view, cell, radius, dtype))


# ---------------------------------------------------------------------------- the lattice inputs of the bit-equality tests
# Coordinates are multiples of 2^-8 in [-1, 1] and the view's entries multiples of 2^-6 below 128: every product is a multiple
# of 2^-14 below 2^7 and every partial sum a multiple of 2^-14 below 2^9, i.e. at most 23 significant bits -- each fp32
# operation of the projection is exact, fused or not, and so is d * 2^24.
LATTICE_CELL = 128
LATTICE_VIEWS = {
    # axis-aligned: a pixel column is one x, so points that differ in z alone pile up on one pixel; +-1 maps 16 pixels outside
    "axis": np.array([[80.0, 0.0, 0.0, 64.0], [0.0, -80.0, 0.0, 64.0], [0.0, 0.0, -0.4375, 0.5]], dtype=np.float32),
    # tilted: a dyadic three-quarter view, wide enough that part of the cube leaves the cell
    "tilted": np.array([[60.5, 0.0, -42.25, 64.0], [17.75, -66.5, 25.5, 64.0], [-0.25, -0.203125, -0.359375, 0.5]], dtype=np.float32),
}


def lattice_clouds(B, N, seed):
    """Two cloud lists (B, N, 3) and (B, N // 2, 3) on the 2^-8 lattice of [-1, 1]^3; in every cloud of the first list 64
    points share one (x, y) and differ in z."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (N, N // 2):
        k = rng.integers(-256, 257, size=(B, n, 3))
        out.append(k)
    out[0][:, :64, 0:2] = out[0][:, :1, 0:2]
    out[0][:, :64, 0:2] = np.clip(out[0][:, :64, 0:2], -128, 128)                 # keep the pile inside the cell
    return [(k.astype(np.float64) / 256.0).astype(np.float32) for k in out]


def read_png(data):
    """A 20-line reader for what write_png writes (8-bit grey, filter type 0): bytes -> (H, W) uint8, checking the signature,
    every chunk's CRC and the chunk order."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, chunks = 8, []
    while at < len(data):
        (n,) = struct.unpack(">I", data[at:at + 4])
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == (zlib.crc32(tag + body) & 0xFFFFFFFF), "crc of %r" % tag
        chunks.append((tag, body))
        at += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and at == len(data)
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any(), "filter type 0 on every scanline"
    return raw[:, 1:].copy()
