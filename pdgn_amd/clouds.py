"""Ragged point clouds as training data: shapes that store DIFFERENT numbers of points (part-annotation sets, scans, the output of any
surface sampler with a density target), resident on the device as one (T,3) array and an offset table, so that every visit of a shape
is a fresh draw made inside the one feed launch (data.RaggedFeeder -> csrc/feed.hip: pdgn_feed_batch_ragged).

`CloudSet` holds a set of shapes as the two arrays the kernels take, normalised cloud by cloud with data.normalize_clouds itself;
`CloudSet.sample` draws the reference clouds of the test phase and the reports (pdgn_sample_ragged).  `open_ragged_root` reads a
directory <synsetid>/<split>/* of .npy and text clouds, or the .npz that `python -m pdgn_amd.clouds pack DIR OUT.npz` makes of one;
`pack --layout part` reads the part-annotation layout (synsetoffset2category.txt, <synsetid>/points/*.pts) with the reference's 90 / 10
split (datasets_4point.py:48-52).  Per-point attributes (normals, labels: further columns of a text file) are dropped.
"""
import os
import sys

import numpy as np

NORMALIZE = (None, "shape_unit", "shape_bbox")
SPLITS = ("train", "val", "test")
TEXT_SUFFIXES = (".pts", ".xyz", ".txt")
MAX_POINTS = 0x7FFFFFFF                                          # pdgn_feed_batch_ragged: T <= 2^31 - 1 (include/pdgn_hip.h)


def _namer(names):
    return (lambda s: "cloud %d" % s) if names is None else (lambda s: "cloud %d (%s)" % (s, names[s]))


class CloudSet:
    """S shapes as the device arrays of pdgn_feed_batch_ragged / pdgn_sample_ragged (include/pdgn_hip.h): points (T,3) fp32, all shapes'
    points back to back; off (S+1) int64, off[0] = 0, strictly increasing, off[S] = T; shift (S,3) / scale (S) fp32: the normalisation
    that was applied ((raw - shift) / scale, data.normalize_clouds cloud by cloud).  Built by `from_clouds` / `from_arrays`, which
    guarantee what the kernels expect: every shape owns a point, every coordinate is finite, the table ascends from 0 to T."""

    def __init__(self, points, off, shift, scale, normalize=None, off_host=None):
        self.points, self.off, self.shift, self.scale = points, off, shift, scale
        self.normalize = normalize
        self._off_host = np.asarray(off.cpu().numpy() if off_host is None else off_host, dtype=np.int64)   # (the table once on the host: no sync per look)
        self.S, self.T = int(self._off_host.shape[0]) - 1, int(points.shape[0])

    # ------------------------------------------------------------------ construction (host)
    @classmethod
    def from_clouds(cls, clouds, normalize=None, names=None):
        """clouds: a list of (M_s,3) arrays.  Refused before anything is built: an empty list, a cloud with no points, a non-finite
        coordinate, any shape other than (M,3)."""
        clouds = list(clouds)
        if not clouds:
            raise ValueError("CloudSet: no clouds")
        name = _namer(names)
        off = [0]
        for s, c in enumerate(clouds):
            shape = tuple(np.shape(c))
            if len(shape) != 2 or shape[1] != 3:
                raise ValueError("%s: a cloud is (M,3), got %s" % (name(s), shape))
            if shape[0] < 1:
                raise ValueError("%s: no points" % name(s))
            off.append(off[-1] + shape[0])
        points = np.concatenate([np.asarray(c, dtype=np.float32) for c in clouds], 0)
        return cls.from_arrays(points, np.asarray(off, dtype=np.int64), normalize, names)

    @classmethod
    def from_arrays(cls, points, off, normalize=None, names=None):
        """From the concatenated form (what `pack` stores): points (T,3), off (S+1); the same checks, on a host copy of off."""
        import torch
        from .data import normalize_clouds
        if normalize not in NORMALIZE:
            raise ValueError("CloudSet: normalize %r -- ragged clouds take None, 'shape_unit' or 'shape_bbox'" % (normalize,))
        name = _namer(names)
        if isinstance(points, torch.Tensor):
            points = points.detach().cpu().numpy()
        if isinstance(off, torch.Tensor):
            off = off.detach().cpu().numpy()
        points = np.asarray(points)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("CloudSet: points are (T,3), got %s" % (points.shape,))
        points = np.ascontiguousarray(points, dtype=np.float32)
        off = np.asarray(off).reshape(-1)
        if off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
            raise ValueError("CloudSet: off is an integer table of S + 1 >= 2 entries (no clouds?)")
        off = off.astype(np.int64)
        S, T = off.shape[0] - 1, points.shape[0]
        if off[0] != 0 or off[-1] != T:
            raise ValueError("CloudSet: off must ascend from 0 to the number of points %d, got %d .. %d" % (T, off[0], off[-1]))
        if np.any(np.diff(off) < 1):
            raise ValueError("%s: no points" % name(int(np.argmax(np.diff(off) < 1))))
        if T > MAX_POINTS:
            raise ValueError("CloudSet: %d points, one device set holds at most 2^31 - 1" % T)
        finite = np.isfinite(points).all(axis=1)
        if not finite.all():
            at = int(np.argmin(finite))
            s = int(np.searchsorted(off, at, side="right")) - 1
            raise ValueError("%s: point %d is not finite" % (name(s), at - int(off[s])))
        host = torch.from_numpy(points)
        shift, scale = torch.zeros(S, 3), torch.ones(S)
        if normalize is not None:                                # data.normalize_clouds itself, cloud by cloud: its result bit for bit
            out = torch.empty_like(host)
            for s in range(S):
                a, b = int(off[s]), int(off[s + 1])
                norm, sh, sc = normalize_clouds(host[a:b][None], normalize)
                if not bool(torch.isfinite(norm).all()):
                    raise ValueError("%s: %d points without extent, %r cannot normalise it (--min_points drops short clouds)"
                                     % (name(s), b - a, normalize))
                out[a:b], shift[s], scale[s] = norm[0], sh[0, 0], sc[0, 0, 0]
            host = out
        return cls(host, torch.from_numpy(off), shift, scale, normalize, off_host=off)

    # ------------------------------------------------------------------ placement and views
    def to(self, device):
        return CloudSet(self.points.to(device).contiguous(), self.off.to(device).contiguous(), self.shift.to(device), self.scale.to(device),
                        self.normalize, off_host=self._off_host)

    def counts(self):
        """(S) int64 numpy: the points every shape stores."""
        return np.diff(self._off_host)

    def cloud(self, s):
        """(M_s,3): a view of shape s."""
        s = int(s)
        if not 0 <= s < self.S:
            raise IndexError("cloud %d of %d" % (s, self.S))
        return self.points[int(self._off_host[s]):int(self._off_host[s + 1])]

    def stats(self, n=None):
        """{"shapes", "points", "min", "median", "max"} of the counts and, for a given n, "n" and "shorter": how many shapes store fewer
        than n points (their rows show every stored point floor(n / M) or ceil(n / M) times)."""
        c = self.counts()
        out = {"shapes": self.S, "points": self.T, "min": int(c.min()), "median": float(np.median(c)), "max": int(c.max())}
        if n is not None:
            out["n"], out["shorter"] = int(n), int((c < int(n)).sum())
        return out

    # ------------------------------------------------------------------ reference draws
    def sample(self, n, seed, draw=0):
        """(S,n,3): out[s, j] = point pi_s(j mod M_s) of shape s (pdgn_sample_ragged): n distinct points where the shape stores that
        many, all of it with evenly spread duplicates where not; a pure function of (seed, draw), its streams apart from every
        training draw of the same seed."""
        import torch
        from . import _lib
        _lib.require(self.points, "the cloud set's points", torch.float32, 2)
        _lib.require(self.off, "the cloud set's offsets", torch.int64, 1)
        out = torch.empty(self.S, int(n), 3, dtype=torch.float32, device=self.points.device)
        _lib.check(_lib.lib().pdgn_sample_ragged(self.S, int(n), _lib.ptr(self.points), _lib.ptr(self.off), self.T,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(out),
                                                 _lib.stream_of(self.points)), "pdgn_sample_ragged")
        return out


# ---------------------------------------------------------------------------- directories and packed files
def load_text_cloud(path):
    """(M,3) fp32 of a text cloud (.pts / .xyz / .txt): one point per line, whitespace- or comma-separated, the first three columns;
    further columns (normals, labels) are ignored, as are empty lines and lines that start with '#'."""
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            tok = line.replace(",", " ").split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) < 3:
                raise ValueError("%s:%d: a point has three coordinates" % (path, ln))
            try:
                rows.append((float(tok[0]), float(tok[1]), float(tok[2])))
            except ValueError:
                raise ValueError("%s:%d: not three numbers: %r" % (path, ln, line.strip())) from None
    return np.asarray(rows, dtype=np.float64).reshape(-1, 3).astype(np.float32)


def load_cloud(path):
    """One stored cloud, by its suffix: .npy (M,3), or a text file (`load_text_cloud`)."""
    if str(path).endswith(".npy"):
        pc = np.load(path)
        if pc.ndim != 2 or pc.shape[1] != 3:
            raise ValueError("%s: a cloud is (M,3), got %s" % (path, pc.shape))
        return np.ascontiguousarray(pc, dtype=np.float32)
    return load_text_cloud(path)


def _is_cloud_file(name):
    return name.endswith(".npy") or name.endswith(TEXT_SUFFIXES)


def read_cloud_root(root, synsetids=None):
    """A directory <synsetid>/<split>/* holding any mix of .npy and .pts / .xyz / .txt clouds -> {synsetid: {split: [(M,3) fp32, ...]}},
    the files of a split in sorted name order; raw coordinates.  synsetids: these categories only."""
    out = {}
    for sid in sorted(os.listdir(root)):
        if not os.path.isdir(os.path.join(root, sid)) or (synsetids is not None and sid not in synsetids):
            continue
        for split in SPLITS:
            folder = os.path.join(root, sid, split)
            if not os.path.isdir(folder):
                continue
            clouds = [load_cloud(os.path.join(folder, n)) for n in sorted(os.listdir(folder)) if _is_cloud_file(n)]
            if clouds:
                out.setdefault(sid, {})[split] = clouds
    if not out and synsetids is None:                            # (none of the categories asked for: the caller's to say)
        raise ValueError("%s: no <synsetid>/<split>/* clouds (.npy, .pts, .xyz, .txt) found" % (root,))
    return out


def read_part_root(root, synsetids=None):
    """The part-annotation layout: synsetoffset2category.txt (`name synsetid` per line) and <synsetid>/points/*.pts -> the mapping of
    `read_cloud_root` with the reference's split (datasets_4point.py:48-52): names sorted, the first int(0.9 * count) files `train`, the
    rest `test`, and `val` the same clouds as `test`.  The labels beside the points are not read."""
    catfile = os.path.join(root, "synsetoffset2category.txt")
    if not os.path.exists(catfile):
        raise ValueError("%s: no synsetoffset2category.txt (the part-annotation layout)" % (root,))
    with open(catfile) as f:
        sids = [line.split()[1] for line in f if len(line.split()) >= 2]
    out = {}
    for sid in sorted(set(sids)):
        folder = os.path.join(root, sid, "points")
        if (synsetids is not None and sid not in synsetids) or not os.path.isdir(folder):
            continue
        names = sorted(os.listdir(folder))
        cut = int(len(names) * 0.9)
        for split, part in (("train", names[:cut]), ("test", names[cut:])):
            clouds = [load_cloud(os.path.join(folder, n)) for n in part if _is_cloud_file(n)]
            if clouds:
                out.setdefault(sid, {})[split] = clouds
        if "test" in out.get(sid, {}):
            out[sid]["val"] = out[sid]["test"]
    if not out and synsetids is None:
        raise ValueError("%s: no <synsetid>/points/*.pts clouds found" % (root,))
    return out


def pack(root, out_path, layout="splits"):
    """Write the directory's clouds as one .npz with the keys "<synsetid>/<split>/points" ((T,3) fp32, raw) and "<synsetid>/<split>/off"
    ((S+1) int64).  layout: "splits" (<synsetid>/<split>/*) or "part" (`read_part_root`)."""
    if layout not in ("splits", "part"):
        raise ValueError("pack: layout 'splits' or 'part', got %r" % (layout,))
    arrays = {}
    for sid, splits in (read_part_root(root) if layout == "part" else read_cloud_root(root)).items():
        for split, clouds in splits.items():
            arrays["%s/%s/points" % (sid, split)] = np.concatenate(clouds, 0)
            arrays["%s/%s/off" % (sid, split)] = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    np.savez(out_path, **arrays)
    return sorted(arrays)


def load_packed(path, synsetids=None):
    """The mapping `read_cloud_root` returns, from a file `pack` wrote."""
    out = {}
    with np.load(path) as f:
        for key in f.files:
            sid, split, what = key.split("/")
            if what == "points" and (synsetids is None or sid in synsetids):
                points, off = f[key], f["%s/%s/off" % (sid, split)].astype(np.int64)
                out.setdefault(sid, {})[split] = [points[off[s]:off[s + 1]] for s in range(off.shape[0] - 1)]
    return out


def is_ragged_root(path):
    """Whether a --data_root is a packed ragged set: an .npz with "<synsetid>/<split>/points" keys.  (A directory does not say what it
    is -- <synsetid>/<split>/*.npy is also the layout of equal-sized clouds -- and is read as ragged only where the caller asks.)"""
    path = str(path)
    if path.endswith(".npz") and os.path.isfile(path):
        with np.load(path) as f:
            return any(k.count("/") == 2 and k.endswith("/points") for k in f.files)
    return False


def open_ragged_root(path, synsetids=None):
    """{synsetid: {split: [(M,3) fp32 arrays]}} of a directory <synsetid>/<split>/* or of the .npz `pack` made of one."""
    if os.path.isdir(path):
        return read_cloud_root(str(path), synsetids)
    return load_packed(path, synsetids)


def split_cloudset(root, split, normalize=None, min_points=1):
    """One CloudSet of a split over every category of an opened root (`open_ragged_root`, or the path of one), categories in sorted
    order.  min_points: shapes that store fewer points are dropped; the set's `dropped` says how many were."""
    if isinstance(root, (str, os.PathLike)):
        root = open_ragged_root(root)
    clouds = [c for sid in sorted(root) if split in root[sid] for c in root[sid][split]]
    if not clouds:
        raise ValueError("the ragged data has no %r split" % split)
    kept = [c for c in clouds if c.shape[0] >= int(min_points)]
    if not kept:
        raise ValueError("no cloud of the %r split stores %d points or more" % (split, int(min_points)))
    cs = CloudSet.from_clouds(kept, normalize)
    cs.dropped = len(clouds) - len(kept)
    return cs


USAGE = "usage: python -m pdgn_amd.clouds pack [--layout splits|part] DIR OUT.npz"


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if not argv or argv[0] != "pack":
        raise SystemExit(USAGE)
    rest, layout, paths = argv[1:], "splits", []
    while rest:
        word = rest.pop(0)
        if word == "--layout" and rest and rest[0] in ("splits", "part"):
            layout = rest.pop(0)
        elif word.startswith("--"):
            raise SystemExit(USAGE)
        else:
            paths.append(word)
    if len(paths) != 2:
        raise SystemExit(USAGE)
    keys = pack(paths[0], paths[1], layout)
    print("packed %d arrays into %s" % (len(keys), paths[1]))


if __name__ == "__main__":
    main()
