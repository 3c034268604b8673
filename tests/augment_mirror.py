"""Host mirror of the discriminator augmentation (csrc/augment.hip, pdgn_amd.augment): the same pure function of
(seed, t, global row, tag) in numpy.  Test infrastructure: the product never imports it.

Counter layout (include/pdgn_hip.h, pdgn_augment_rows_fwd): key = (seed lo, seed hi); counter = (group, global row, t lo,
tag | t hi24 << 8) with t = clock - 1; tag = 16 + 3 * network + role (real, fake, gen).  Group 0: enable words of flip, rotation,
scale, translation; group 1: jitter's enable word, v of the angle, v of the log-scale; group 2: v of the translation; group 4 + n:
point n's jitter (Box-Muller pairs (0,1) -> x, y; (2,3) -> z, unused).  v = ((w >> 8) - 2^23) 2^-23."""
import numpy as np

import feed_mirror as fm

TAG_BASE = 16
ROLES = ("real", "fake", "gen")
FEEDER_TAGS = (0, 1, 2, fm.TAG_Z1, fm.TAG_Z2, fm.TAG_ORDER)
GROUP_ENABLE, GROUP_SHAPE, GROUP_SHIFT, GROUP_POINT0 = 0, 1, 2, 4


def tag(network, role):
    return TAG_BASE + 3 * network + ROLES.index(role)


def threshold(p):
    return int(round(p * (1 << 24)))


def table(p=0.5, rot_max_deg=180.0, scale_max=1.25, flip=True, trans_max=0.1, jitter_sigma=0.0, up_axis=1, flip_axis=0):
    """pdgn_aug_table's fields as the kernels read them (ranges rounded to fp32; a zero range disables its component)."""
    thr = threshold(p)
    return {"thr_flip": thr if flip else 0, "thr_rot": thr if rot_max_deg > 0 else 0, "thr_scale": thr if scale_max > 1 else 0,
            "thr_trans": thr if trans_max > 0 else 0, "thr_jitter": thr if jitter_sigma > 0 else 0, "flip_axis": flip_axis,
            "up_axis": up_axis, "rot_max": float(np.float32(np.radians(rot_max_deg))), "log_scale_max": float(np.float32(np.log(scale_max))),
            "trans_max": float(np.float32(trans_max)), "sigma": float(np.float32(jitter_sigma))}


def words(seed, t, rows, tag_, group):
    """The four words of `group` for every global row of `rows` -> (len(rows), 4) uint32."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    c3 = tag_ | (((t >> 32) & 0xFFFFFF) << 8)
    return fm.philox4x32_10((np.uint64(group), rows, t & 0xFFFFFFFF, c3), fm._key(seed))


def unit(w, dtype=np.float64):
    """((w >> 8) - 2^23) 2^-23 in [-1, 1)."""
    return ((w >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(dtype) * dtype(2.0 ** -23)


def decisions(tab, seed, t, rows, tag_):
    """(len(rows), 5) bool: flip, rotation, scale, translation, jitter enabled."""
    e, d = words(seed, t, rows, tag_, GROUP_ENABLE), words(seed, t, rows, tag_, GROUP_SHAPE)
    hi = lambda w: (w >> np.uint32(8)).astype(np.int64)
    return np.stack([hi(e[:, 0]) < tab["thr_flip"], hi(e[:, 1]) < tab["thr_rot"], hi(e[:, 2]) < tab["thr_scale"],
                     hi(e[:, 3]) < tab["thr_trans"], hi(d[:, 0]) < tab["thr_jitter"]], axis=1)


def affine(tab, seed, t, rows, tag_, dtype=np.float64):
    """(len(rows), 12): per row the matrix s R F row-major, then the translation, evaluated in `dtype` (fp64: the reference of the
    tests; fp32: the formula as the kernel spells it, every operation rounded on its own)."""
    f = dtype
    on = decisions(tab, seed, t, rows, tag_)
    d, w = words(seed, t, rows, tag_, GROUP_SHAPE), words(seed, t, rows, tag_, GROUP_SHIFT)
    theta = f(tab["rot_max"]) * unit(d[:, 1], f)
    c = np.where(on[:, 1], np.cos(theta), f(1)).astype(f)
    s = np.where(on[:, 1], np.sin(theta), f(0)).astype(f)
    sc = np.where(on[:, 2], np.exp(f(tab["log_scale_max"]) * unit(d[:, 2], f)), f(1)).astype(f)
    u, fa = tab["up_axis"], tab["flip_axis"]
    ia = (u + 1) % 3
    out = np.zeros((len(on), 12), dtype=f)
    for i in range(3):
        for j in range(3):
            r = (np.ones_like(c) if i == u and j == u else np.zeros_like(c) if i == u or j == u else c if i == j
                 else -s if i == ia else s)
            if j == fa:
                r = np.where(on[:, 0], -r, r)
            out[:, 3 * i + j] = sc * r
        out[:, 9 + i] = np.where(on[:, 3], f(tab["trans_max"]) * unit(w[:, i], f), f(0))
    return out


def jitter(tab, seed, t, rows, tag_, N, dtype=np.float64):
    """(len(rows), N, 3): the normals added to each point (zero rows where jitter is disabled)."""
    on = decisions(tab, seed, t, rows, tag_)[:, 4]
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    groups = (GROUP_POINT0 + np.arange(N, dtype=np.uint64)).reshape(1, -1)
    c3 = tag_ | (((t >> 32) & 0xFFFFFF) << 8)
    w = fm.philox4x32_10((groups, rows, t & 0xFFFFFFFF, c3), fm._key(seed))          # (rows, N, 4)
    z = fm.normals_from_words(w, tab["sigma"], dtype)[..., :3]
    return np.where(on[:, None, None], z, dtype(0))


def rows_fp32(aff, x):
    """The kernel's arithmetic in numpy fp32: aff (B,12) fp32, x (B,3,N) fp32 -> (B*N,3), ((a0 x0 + a1 x1) + a2 x2) + t."""
    aff, x = np.asarray(aff, dtype=np.float32), np.asarray(x, dtype=np.float32)
    B, _, N = x.shape
    out = np.empty((B, N, 3), dtype=np.float32)
    for i in range(3):
        a = aff[:, 3 * i:3 * i + 3, None]
        out[:, :, i] = ((a[:, 0] * x[:, 0] + a[:, 1] * x[:, 1]) + a[:, 2] * x[:, 2]) + aff[:, 9 + i, None]
    return out.reshape(B * N, 3)


def grad_fp32(aff, d_rows, B, N):
    """dx (B,3,N) = A^T d_rows in the kernel's order: (a0j d0 + a1j d1) + a2j d2."""
    aff, d = np.asarray(aff, dtype=np.float32), np.asarray(d_rows, dtype=np.float32).reshape(B, N, 3)
    out = np.empty((B, 3, N), dtype=np.float32)
    for j in range(3):
        out[:, j] = (aff[:, j, None] * d[:, :, 0] + aff[:, 3 + j, None] * d[:, :, 1]) + aff[:, 6 + j, None] * d[:, :, 2]
    return out
