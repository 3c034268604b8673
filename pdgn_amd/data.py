"""ShapeNetCore ingestion and normalisation modes of the reference (datasets_4point.py:266-380,
models/PDGNet_v2.py:415-430), batched on whatever device the clouds live on.

The reference normalises cloud by cloud in a Python loop at load time; here the five `scale_mode`s are
tensor expressions over a (S, N, 3) stack.  `ShapeNetCore` reads the same HDF5 layout
(`f[synsetid][split] -> (S, N, 3)`) -- from a path when `h5py` is installed, or from any mapping with that
shape (which is also how the tests drive it: this image has no h5py).

`BatchFeeder` is the training-side feed: the whole split stays on the device and ONE launch (csrc/feed.hip,
pdgn_feed_batch) writes a batch -- shuffled clouds, the three sub-samplings, the transposes and both noise draws --
into the buffers the training step reads (`subsample="fps"`: a second launch, csrc/fps.hip's pdgn_feed_fps_pyramid, replaces the
three independent with-replacement sub-samplings by nested farthest-point subsets of the finest cloud).  Clouds stored denser than they are trained on (the 15 000 points per shape of
ShapeNetCore.v2.PC15k) go through pdgn_feed_batch_resample: a fresh `num_point` subset of every cloud each time it is visited.  `MeshFeeder` is the same feed for shapes stored
as triangle meshes (pdgn_amd.meshes.MeshSet; pdgn_feed_batch_mesh): every visit of a shape is a fresh i.i.d. sample of its surface.
`RaggedFeeder` is the same feed for shapes that store different numbers of points (pdgn_amd.clouds.CloudSet; pdgn_feed_batch_ragged).
"""
import os
import random

import numpy as np
import torch

SCALE_MODES = (None, "global_unit", "shape_unit", "shape_bbox", "shape_half", "shape_34")

# ShapeNetCore.v2 synset ids of the 55 categories the reference knows (datasets_4point.py:238-262)
_SYNSETS = """02691156 airplane|02747177 can|02773838 bag|02801938 basket|02808440 bathtub|02818832 bed|02828884 bench|
02843684 birdhouse|02871439 bookshelf|02876657 bottle|02880940 bowl|02924116 bus|02933112 cabinet|02942699 camera|
02946921 tin_can|02954340 cap|02958343 car|02992529 cellphone|03001627 chair|03046257 clock|03085013 keyboard|
03207941 dishwasher|03211117 monitor|03261776 earphone|03325088 faucet|03337140 file|03467517 guitar|03513137 helmet|
03593526 jar|03624134 knife|03636649 lamp|03642806 laptop|03691459 speaker|03710193 mailbox|03759954 microphone|
03761084 microwave|03790512 motorcycle|03797390 mug|03928116 piano|03938244 pillow|03948459 pistol|03991062 pot|
04004475 printer|04074963 remote_control|04090263 rifle|04099429 rocket|04225987 skateboard|04256520 sofa|
04330267 stove|04379243 table|04401088 telephone|04460130 tower|04468005 train|04530566 vessel|04554684 washer"""
synsetid_to_cate = dict(item.split() for item in _SYNSETS.replace("\n", "").split("|"))
cate_to_synsetid = {v: k for k, v in synsetid_to_cate.items()}


def dataset_statistics(all_points):
    """get_statistics (:289-316): per-axis mean over every point, one std over every coordinate."""
    B, N, _ = all_points.shape
    return {"mean": all_points.reshape(B * N, -1).mean(dim=0), "std": all_points.reshape(-1).std(dim=0)}


def normalize_clouds(pcs, mode, global_std=None):
    """(S, N, 3) -> (normalised clouds, shift (S,1,3), scale (S,1,1)) for a `scale_mode` of :326-348
    (`shape_unit` / `shape_bbox` are also the two modes of PDGNet_v2.normalize_point_clouds :415-430)."""
    if mode not in SCALE_MODES:
        raise ValueError("unknown scale_mode %r" % (mode,))
    S = pcs.shape[0]
    if mode is None:
        shift = torch.zeros(S, 1, 3, dtype=pcs.dtype, device=pcs.device)
        scale = torch.ones(S, 1, 1, dtype=pcs.dtype, device=pcs.device)
    elif mode == "shape_bbox":
        pc_max, pc_min = pcs.max(dim=1, keepdim=True)[0], pcs.min(dim=1, keepdim=True)[0]
        shift = (pc_min + pc_max) / 2
        scale = (pc_max - pc_min).max(dim=2, keepdim=True)[0] / 2
    else:
        shift = pcs.mean(dim=1, keepdim=True)
        if mode == "global_unit":
            if global_std is None:
                raise ValueError("global_unit needs the data set's std (dataset_statistics)")
            scale = torch.as_tensor(global_std, dtype=pcs.dtype, device=pcs.device).reshape(1, 1, 1).expand(S, 1, 1)
        else:
            scale = pcs.reshape(S, -1).std(dim=1).view(S, 1, 1)
            if mode == "shape_half":
                scale = scale / 0.5
            elif mode == "shape_34":
                scale = scale / 0.75
    return (pcs - shift) / scale, shift, scale


def normalize_point_clouds(pcs, mode):
    """PDGNet_v2.normalize_point_clouds (:415-430) for a whole (S,N,3) stack (mode None: unchanged)."""
    if mode is None:
        return pcs
    if mode not in ("shape_unit", "shape_bbox"):
        raise ValueError("the test phase normalises with shape_unit or shape_bbox, got %r" % (mode,))
    return normalize_clouds(pcs, mode)[0]


def multires_sample(pcs, sizes=(256, 512, 1024), generator=None):
    """The three sub-resolutions of __getitem__ (:372-379): indices drawn WITH replacement, one draw per cloud."""
    S, N, _ = pcs.shape
    out = []
    for r in sizes:
        sel = torch.randint(0, N, (S, r), generator=generator, device=pcs.device if generator is None else generator.device)
        out.append(torch.gather(pcs, 1, sel.to(pcs.device).unsqueeze(2).expand(S, r, 3)))
    return out


def _open(source):
    if not isinstance(source, (str, bytes, os.PathLike)):
        return source, None
    try:
        import h5py
    except ImportError as e:                                    # pragma: no cover - h5py absent in this image
        raise ImportError("reading %r needs h5py; pass a {synsetid: {split: array}} mapping instead" % (source,)) from e
    f = h5py.File(source, "r")
    return f, f


class ShapeNetCore(torch.utils.data.Dataset):
    """datasets_4point.ShapeNetCore (:266-380): same constructor arguments, same per-item tuple
    (256 / 512 / 1024 resampled points, the full cloud, the category name), same deterministic shuffle."""

    GRAVITATIONAL_AXIS = 1

    def __init__(self, cates_list, split, scale_mode, path, transform=None, tail=None):
        """tail = N: keep the LAST N points of every stored cloud, all three splits alike, cut before any statistic or
        normalisation (the held-out points of clouds a BatchFeeder trains on the head of); None: the clouds as stored."""
        super().__init__()
        cates = [cates_list] if isinstance(cates_list, str) else list(cates_list)
        assert split in ("train", "val", "test")
        assert scale_mode in SCALE_MODES
        if "all" in cates:
            cates = list(cate_to_synsetid.keys())
        self.cate_synsetids = sorted(cate_to_synsetid[s] for s in cates)
        self.split, self.scale_mode, self.transform, self.path = split, scale_mode, transform, path
        f, closer = _open(path)
        try:
            def read(sid, sp):
                pcs = torch.as_tensor(np.asarray(f[sid][sp]))
                return pcs if tail is None else pcs[:, max(pcs.shape[1] - int(tail), 0):]

            every = [read(sid, sp) for sid in self.cate_synsetids for sp in ("train", "val", "test")]
            self.stats = dataset_statistics(torch.cat(every, dim=0))
            self.pointclouds = []
            for sid in self.cate_synsetids:
                pcs = read(sid, split)
                norm, shift, scale = normalize_clouds(pcs, scale_mode, self.stats["std"])
                for j in range(pcs.shape[0]):
                    self.pointclouds.append({"pointcloud": norm[j], "cate": synsetid_to_cate[sid], "id": j,
                                             "shift": shift[j], "scale": scale[j]})
        finally:
            if closer is not None:
                closer.close()
        self.pointclouds.sort(key=lambda d: d["id"])
        random.Random(2020).shuffle(self.pointclouds)           # the reference's deterministic shuffle (:362-363)

    def __len__(self):
        return len(self.pointclouds)

    def __getitem__(self, idx):
        data = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.pointclouds[idx].items()}
        if self.transform is not None:
            data = self.transform(data)
        pc = data["pointcloud"]
        subs = [pc[np.random.choice(pc.shape[0], r), :].float() for r in (256, 512, 1024)]
        return subs[0], subs[1], subs[2], pc, data["cate"]

    def stack(self, device=None):
        """All clouds of the split as one (S,N,3) tensor in data-set order (the test phase's `ref_pcs`, :293-298)."""
        pcs = torch.stack([d["pointcloud"] for d in self.pointclouds], 0)
        return pcs.to(device) if device is not None else pcs


# ---------------------------------------------------------------------------- the training feed (csrc/feed.hip)
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_TAG_ORDER = 5                                                  # stream tags 0..4 belong to pdgn_feed_batch (include/pdgn_hip.h)


def _philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy arrays of 32-bit words held in uint64 -> four arrays of words."""
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def epoch_order(seed, epoch, S):
    """The permutation of [0, S) an epoch visits the clouds in (the DataLoader's shuffle=True, models/PDGNet_v2.py:78):
    a stable argsort of S Philox words, key (seed lo, seed hi), counter (group, epoch lo, epoch hi, tag 5).  A pure function of
    its arguments, computed on the host: resuming at an epoch boundary needs no saved generator state."""
    seed, epoch, S = int(seed), int(epoch), int(S)
    g = np.arange((S + 3) // 4, dtype=np.uint64)
    full = lambda v: np.full_like(g, v)
    words = _philox4x32_10(g, full(epoch & 0xFFFFFFFF), full((epoch >> 32) & 0xFFFFFFFF), full(_TAG_ORDER),
                           seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.argsort(np.stack(words, axis=1).reshape(-1)[:S], kind="stable").astype(np.int32)


def batches_per_epoch(S, B, world=1):
    """Full batches only, as the reference does (models/PDGNet_v2.py:79, :169); the global batch is B * world."""
    return int(S) // (int(B) * int(world))


class _Feeder:
    """What the device feeds share: the (rank, world) schedule over `epoch_order`, the pinned upload of an epoch's order, the checks of the
    buffers a batch is written into and the optional farthest-point launch behind the feed launch.  A subclass validates its own source,
    calls `_setup` and implements `_launch(first, t, row0, reals, z1, z2)`: the feed launch itself."""

    NOISE_DIM = 128
    SUBSAMPLE = ("random", "fps")
    FPS_MAX_N = 8192                                             # PDGN_FPS_MAX_N (include/pdgn_hip.h)

    def _check_subsample(self, subsample):
        if subsample not in self.SUBSAMPLE:
            raise ValueError("subsample %r: one of %s" % (subsample, ", ".join(self.SUBSAMPLE)))
        self.subsample = subsample

    def _setup(self, device, S, batch_size, sizes, seed, rank, world, sigma, what="clouds"):
        """self.N and self.subsample are set; everything else the schedule needs is set here."""
        from . import _lib
        sizes = tuple(int(r) for r in sizes)
        if len(sizes) == 4 and sizes[3] == self.N:
            sizes = sizes[:3]
        if len(sizes) != 3 or min(sizes) < 1:
            raise ValueError("sizes: the three sub-resolutions (optionally followed by N), got %r" % (sizes,))
        if self.subsample == "fps":
            if not sizes[0] <= sizes[1] <= sizes[2] <= self.N:
                raise ValueError('subsample="fps": the sizes must ascend and not exceed num_point = %d (each level is a prefix of '
                                 "the next), got %r" % (self.N, sizes))
            if self.N > self.FPS_MAX_N:
                raise ValueError('subsample="fps": num_point %d, the farthest-point kernel holds at most %d points' % (self.N, self.FPS_MAX_N))
        self.device, self.sizes = device, sizes
        self.S = int(S)
        self.B, self.seed, self.rank, self.world, self.sigma = int(batch_size), int(seed), int(rank), int(world), float(sigma)
        if self.B < 1 or self.world < 1 or not 0 <= self.rank < self.world:
            raise ValueError("batch_size >= 1 and 0 <= rank < world, got %d, %d, %d" % (self.B, self.rank, self.world))
        self.batches_per_epoch = batches_per_epoch(self.S, self.B, self.world)
        if self.batches_per_epoch < 1:
            raise ValueError("%d %s do not make one batch of %d x %d" % (self.S, what, self.B, self.world))
        self._order = torch.empty(self.S, dtype=torch.int32, device=device)
        self._order_host = torch.empty(self.S, dtype=torch.int32).pin_memory()
        self._order_epoch = None
        self._fps = _lib.lib().pdgn_feed_fps_pyramid if self.subsample == "fps" else None
        self._check = None

    def shapes(self):
        """Shapes of (p1, p2, p3, p4, z)."""
        return [(self.B, 3, r) for r in self.sizes + (self.N,)] + [(self.B, self.NOISE_DIM)]

    def buffers(self):
        """Fresh (reals, z1, z2) of the right shapes on the feeder's device."""
        sh = self.shapes()
        new = lambda s: torch.empty(s, dtype=torch.float32, device=self.device)
        return [new(s) for s in sh[:4]], new(sh[4]), new(sh[4])

    def _upload_order(self, epoch):
        # the previous epoch's upload may not have run yet, and it reads the pinned staging buffer when it runs
        if self._order_epoch is not None:
            self._order_copied.synchronize()
        self._order_host.copy_(torch.from_numpy(epoch_order(self.seed, epoch, self.S)))
        self._order.copy_(self._order_host, non_blocking=True)
        self._order_copied = torch.cuda.Event()
        self._order_copied.record(torch.cuda.current_stream(self.device))
        self._order_epoch = epoch

    def fill(self, epoch, i, reals, z1, z2):
        """Batch i (0-based) of `epoch` (1-based) into the given tensors, on the current stream: one launch (subsample="fps": two)."""
        from . import _lib
        key = (tuple(t.data_ptr() for t in reals), z1.data_ptr(), z2.data_ptr())
        if key != self._check:                                   # (the same static buffers every iteration: checked once)
            if len(reals) != 4:
                raise ValueError("reals: four tensors (B,3,r1) (B,3,r2) (B,3,r3) (B,3,N)")
            for t, name, shape in zip(list(reals) + [z1, z2], ("p1", "p2", "p3", "p4", "z1", "z2"), self.shapes() + [self.shapes()[4]]):
                _lib.require(t, name, torch.float32, len(shape))
                if tuple(t.shape) != shape:
                    raise ValueError("%s must be %s, got %s" % (name, shape, tuple(t.shape)))
                if t.device != self.device:
                    raise _lib.PdgnHipError("%s is on %s, the %s on %s" % (name, t.device, self._WHAT, self.device))
            self._check = key
        if not 0 <= i < self.batches_per_epoch or epoch < 1:
            raise IndexError("batch %d of epoch %d: an epoch has %d batches, epochs count from 1" % (i, epoch, self.batches_per_epoch))
        if epoch != self._order_epoch:
            self._upload_order(epoch)
        t = (epoch - 1) * self.batches_per_epoch + i
        self._launch((i * self.world + self.rank) * self.B, t, self.rank * self.B, reals, z1, z2)
        if self._fps is not None:                                # the same (seed, iteration, global row) as the feed launch: its own tag
            _lib.check(self._fps(self.B, self.N, self.sizes[0], self.sizes[1], self.sizes[2], _lib.ptr(reals[3]),
                                 self.seed & 0xFFFFFFFFFFFFFFFF, t, self.rank * self.B,
                                 _lib.ptr(reals[0]), _lib.ptr(reals[1]), _lib.ptr(reals[2]), None, _lib.stream_of(reals[3])),
                       "pdgn_feed_fps_pyramid")


class BatchFeeder(_Feeder):
    """A device-resident split and the launch that turns it into training batches.

    clouds: (S, M, 3) fp32 device tensor (`ShapeNetCore.stack(device)`; `from_dataset` does that and refuses a data set with a
    per-item `transform`, for which the device path has no hook).  sizes: the three sub-resolutions (a fourth entry must
    equal N).  num_point: N, the points of the finest output (default M: the stored clouds themselves); pool: P, the leading
    points of a cloud that may be drawn (default M).  With N < M or a pool every row of the finest output is a fresh draw of N
    distinct points of its cloud's pool per iteration and the sub-resolutions draw from the pool (pdgn_feed_batch_resample);
    with neither, the launch is pdgn_feed_batch.  Batch i of `epoch` on `rank` of `world` takes the clouds order[(i * world + rank) * B ...] of
    `epoch_order(seed, epoch, S)`; global rows rank * B + b and the global iteration (epoch - 1) * batches_per_epoch + i index
    the random streams, so that `world` ranks at batch B draw what one rank draws at batch B * world.
    subsample: "random" (the default: the reference's three independent with-replacement draws, made by the feed launch) or "fps":
    after the feed launch, unchanged, pdgn_feed_fps_pyramid on the same stream overwrites p1..p3 with the leading r1 / r2 / r3
    points of a farthest-point order of the row's p4 (start index drawn per row and iteration) -- nested, evenly spread, without
    duplicates where p4 has none; p4, z1, z2 are what "random" writes.  "fps" needs ascending sizes <= N and N <= FPS_MAX_N."""

    _WHAT = "clouds"

    def __init__(self, clouds, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=None, pool=None, subsample="random"):
        from . import _lib
        self._check_subsample(subsample)
        if not isinstance(clouds, torch.Tensor):
            if getattr(clouds, "transform", None) is not None:
                raise ValueError("BatchFeeder: the data set has a per-item transform; the device feed has no per-item Python hook")
            raise TypeError("BatchFeeder takes the (S,N,3) device tensor of a split (ShapeNetCore.stack(device), or "
                            "BatchFeeder.from_dataset)")
        _lib.require(clouds, "clouds", torch.float32, 3)
        if clouds.shape[2] != 3:
            raise ValueError("clouds must be (S,N,3), got %s" % (tuple(clouds.shape),))
        self.M = int(clouds.shape[1])
        self.N = self.M if num_point is None else int(num_point)
        self.P = self.M if pool is None else int(pool)
        if not 1 <= self.N <= self.M:
            raise ValueError("num_point %d: the clouds have %d points" % (self.N, self.M))
        if not self.N <= self.P <= self.M:
            raise ValueError("pool %d: at least num_point = %d and at most the %d stored points" % (self.P, self.N, self.M))
        self._resample = self.N != self.M or pool is not None
        self.clouds = clouds
        self._setup(clouds.device, clouds.shape[0], batch_size, sizes, seed, rank, world, sigma)
        self._fn = _lib.lib().pdgn_feed_batch_resample if self._resample else _lib.lib().pdgn_feed_batch

    @classmethod
    def from_dataset(cls, dataset, device, batch_size, sizes=(256, 512, 1024), seed=0, **kw):
        if getattr(dataset, "transform", None) is not None:
            raise ValueError("BatchFeeder: the data set has a per-item transform; the device feed has no per-item Python hook")
        return cls(dataset.stack(device).float().contiguous(), batch_size, sizes, seed, **kw)

    def _launch(self, first, t, row0, reals, z1, z2):
        from . import _lib
        dims = (self.B, self.S, self.M, self.P, self.N) if self._resample else (self.B, self.S, self.N)
        _lib.check(self._fn(*dims, self.sizes[0], self.sizes[1], self.sizes[2], _lib.ptr(self.clouds),
                            _lib.ptr(self._order), first, self.seed & 0xFFFFFFFFFFFFFFFF, t, row0, self.sigma,
                            _lib.ptr(reals[0]), _lib.ptr(reals[1]), _lib.ptr(reals[2]), _lib.ptr(reals[3]), _lib.ptr(z1), _lib.ptr(z2),
                            _lib.stream_of(self.clouds)), "pdgn_feed_batch_resample" if self._resample else "pdgn_feed_batch")


class MeshFeeder(_Feeder):
    """BatchFeeder for shapes stored as triangle meshes (pdgn_amd.meshes.MeshSet on the device): every visit of a shape is a fresh
    i.i.d. sample of its surface, all four resolutions drawn independently inside ONE launch (csrc/feed.hip: pdgn_feed_batch_mesh);
    the schedule, the random streams' indexing by global row and global iteration and the noise are BatchFeeder's.
    subsample="fps": pdgn_feed_fps_pyramid behind the mesh launch overwrites p1..p3 with nested farthest-point subsets of the row's p4."""

    _WHAT = "meshes"

    def __init__(self, meshset, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=2048, subsample="random"):
        from . import _lib
        from .meshes import MeshSet
        self._check_subsample(subsample)
        if not isinstance(meshset, MeshSet):
            raise TypeError("MeshFeeder takes a pdgn_amd.meshes.MeshSet on the device (MeshSet.from_meshes(...).to(device))")
        _lib.require(meshset.verts, "the mesh set's vertices", torch.float32, 2)
        self.N = int(num_point)
        if self.N < 1:
            raise ValueError("num_point %d: at least one" % self.N)
        self.meshes = meshset
        self._setup(meshset.verts.device, meshset.S, batch_size, sizes, seed, rank, world, sigma, what="shapes")
        self._fn = _lib.lib().pdgn_feed_batch_mesh

    def _launch(self, first, t, row0, reals, z1, z2, face_rec=None):
        from . import _lib
        m = self.meshes
        _lib.check(self._fn(self.B, self.S, m.V, m.F, self.N, self.sizes[0], self.sizes[1], self.sizes[2], _lib.ptr(m.verts), _lib.ptr(m.faces),
                            _lib.ptr(m.face_off), _lib.ptr(m.alias), _lib.ptr(self._order), first, self.seed & 0xFFFFFFFFFFFFFFFF, t, row0,
                            self.sigma, _lib.ptr(reals[0]), _lib.ptr(reals[1]), _lib.ptr(reals[2]), _lib.ptr(reals[3]), _lib.ptr(z1),
                            _lib.ptr(z2), _lib.ptr(face_rec), _lib.stream_of(m.verts)), "pdgn_feed_batch_mesh")


class RaggedFeeder(_Feeder):
    """BatchFeeder for shapes that store different numbers of points (pdgn_amd.clouds.CloudSet on the device): ONE launch (csrc/feed.hip:
    pdgn_feed_batch_ragged) writes the batch -- the finest output of a row is a fresh draw of num_point distinct points of its shape where
    the shape stores that many, and the whole shape with evenly spread duplicates where it stores fewer; the sub-resolutions draw with
    replacement from the whole shape; the schedule, the random streams' indexing by global row and global iteration and the noise are
    BatchFeeder's.  subsample="fps": pdgn_feed_fps_pyramid behind the launch overwrites p1..p3 with nested farthest-point subsets of the
    row's p4."""

    _WHAT = "clouds"

    def __init__(self, cloudset, batch_size, sizes, seed, rank=0, world=1, sigma=0.2, num_point=2048, subsample="random"):
        from . import _lib
        from .clouds import CloudSet
        self._check_subsample(subsample)
        if not isinstance(cloudset, CloudSet):
            raise TypeError("RaggedFeeder takes a pdgn_amd.clouds.CloudSet on the device (CloudSet.from_clouds(...).to(device))")
        _lib.require(cloudset.points, "the cloud set's points", torch.float32, 2)
        _lib.require(cloudset.off, "the cloud set's offsets", torch.int64, 1)
        if cloudset.off.device != cloudset.points.device:
            raise _lib.PdgnHipError("the cloud set's offsets are on %s, its points on %s" % (cloudset.off.device, cloudset.points.device))
        self.N = int(num_point)
        if self.N < 1:
            raise ValueError("num_point %d: at least one" % self.N)
        self.clouds = cloudset
        self._setup(cloudset.points.device, cloudset.S, batch_size, sizes, seed, rank, world, sigma, what="shapes")
        self._fn = _lib.lib().pdgn_feed_batch_ragged

    def _launch(self, first, t, row0, reals, z1, z2):
        from . import _lib
        c = self.clouds
        _lib.check(self._fn(self.B, self.S, self.N, self.sizes[0], self.sizes[1], self.sizes[2], _lib.ptr(c.points), _lib.ptr(c.off), c.T,
                            _lib.ptr(self._order), first, self.seed & 0xFFFFFFFFFFFFFFFF, t, row0, self.sigma,
                            _lib.ptr(reals[0]), _lib.ptr(reals[1]), _lib.ptr(reals[2]), _lib.ptr(reals[3]), _lib.ptr(z1), _lib.ptr(z2),
                            _lib.stream_of(c.points)), "pdgn_feed_batch_ragged")
