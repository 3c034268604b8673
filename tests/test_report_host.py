"""Snapshot reports, host side (pdgn_amd/report.py): the PNG writer, the rasteriser's numpy mirror (tests/render_mirror.py) on
hand-made and lattice inputs, the new command-line flags, and the reduction stage of the cheap metrics against the reference's
own outputs (tests/golden/eval_metrics.npz)."""
import struct
import zlib

import numpy as np
import pytest
import torch

import render_mirror as rm


def test_write_png_round_trips_through_a_small_reader(tmp_path):
    from pdgn_amd.report import write_png
    rng = np.random.default_rng(0)
    for shape in ((1, 1), (5, 7), (128, 640)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        path = write_png(str(tmp_path / "a.png"), img)
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        assert data[12:16] == b"IHDR" and struct.unpack(">II", data[16:24]) == (shape[1], shape[0])
        assert data[-12:] == struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND") & 0xFFFFFFFF)
        assert np.array_equal(rm.read_png(data), img)                          # (checks every chunk's CRC)
    write_png(str(tmp_path / "t.png"), torch.from_numpy(img))                  # a tensor is taken as well
    assert np.array_equal(rm.read_png(open(tmp_path / "t.png", "rb").read()), img)
    for bad in (img.astype(np.int32), img[None], np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(str(tmp_path / "bad.png"), bad)


def test_mirror_nearer_point_wins_a_pixel():
    """Two points on one pixel: the nearer one (smaller d) decides its grey value, whatever their order.  This exercises the
    numpy mirror alone (it says nothing about csrc/render.hip and passes without it): it pins, by hand, the expected image that
    tests/test_gpu_report.py holds the kernel to."""
    view = np.array([[8, 0, 0, 8], [0, -8, 0, 8], [0, 0, -0.5, 0.5]], dtype=np.float32)      # 16 x 16 cell, z towards the viewer
    near, far = [0.25, 0.25, 0.5], [0.25, 0.25, -0.5]
    for pts in ([near, far], [far, near]):
        img = rm.render([np.array([pts], dtype=np.float32)], view, 16, 0)
        assert img.shape == (16, 16) and np.count_nonzero(img) == 1
        q = int(0.25 * 2 ** 24)
        assert img[6, 10] == 255 - (q >> 17) == 223                           # u = 10, v = 6; d(near) = 0.25, d(far) = 0.75
    alone = rm.render([np.array([[far]], dtype=np.float32)], view, 16, 0)
    assert alone[6, 10] == 255 - (int(0.75 * 2 ** 24) >> 17) == 159
    # radius 1: a plus of five pixels; a point at the cell's edge is clipped to the cell, never written to the neighbour
    two = rm.render([np.array([[[0.99, 0.0, 0.0]]], dtype=np.float32)] * 2, view, 16, 1)
    assert two.shape == (16, 32) and np.count_nonzero(two[:, :16]) == 4 and np.array_equal(two[:, :16], two[:, 16:])
    assert two[8, 15] and two[8, 14] and two[7, 15] and two[9, 15] and not two[8, 16 - 16]
    out = rm.render([np.array([[[3.0, 0.0, 0.0], [np.nan, 0.0, 0.0]]], dtype=np.float32)], view, 16, 1)
    assert not out.any()


@pytest.mark.parametrize("name", sorted(rm.LATTICE_VIEWS))
@pytest.mark.parametrize("B,N", [(1, 256), (3, 2048)])
def test_mirror_is_exact_on_the_lattice_inputs(name, B, N):
    """The inputs of the GPU bit-equality test: the fp32 evaluation and an fp64 one give the same pixels and keys, so the
    expected image does not depend on how a product and a sum are rounded (fused or not).  Mirror only, like the test above:
    it guards the GPU test's expectation, not the kernel."""
    view = rm.LATTICE_VIEWS[name]
    assert np.array_equal(view * 64, np.round(view * 64))
    clouds = rm.lattice_clouds(B, N, seed=11)
    for pts in clouds:
        assert np.array_equal(pts * 256, np.round(pts * 256)) and np.abs(pts).max() <= 1
        a, b = rm.point_keys(pts, view, np.float32), rm.point_keys(pts, view, np.float64)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        u32, u64 = rm.project(pts, view, np.float32), rm.project(pts, view, np.float64)
        assert all(np.array_equal(p.astype(np.float64), q) for p, q in zip(u32, u64))
    k32, k64 = rm.sheet_keys(clouds, view, rm.LATTICE_CELL, 1, np.float32), rm.sheet_keys(clouds, view, rm.LATTICE_CELL, 1, np.float64)
    assert np.array_equal(k32, k64)
    # the cases the GPU test is meant to cover are present: points outside their cell, many points on one pixel
    iu, iv, _, _ = rm.point_keys(clouds[0], view, np.float32)
    outside = (iu < 0) | (iu >= rm.LATTICE_CELL) | (iv < 0) | (iv >= rm.LATTICE_CELL)
    assert outside.any() and not outside.all()
    _, counts = np.unique(np.stack([iu[0], iv[0]], 1), axis=0, return_counts=True)
    assert counts.max() >= (64 if name == "axis" else 2)


def test_default_view_frames_the_unit_sphere():
    from pdgn_amd.report import default_view
    for cell in (64, 128):
        view = default_view(cell)
        assert view.dtype == np.float32 and view.shape == (3, 4)
        rng = np.random.default_rng(1)
        p = rng.standard_normal((4096, 3))
        p = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
        u, v, d = rm.project(p, view, np.float64)
        assert u.min() >= 0 and u.max() < cell and v.min() >= 0 and v.max() < cell and d.min() >= 0 and d.max() <= 1
        # y is up (image rows grow downwards) and the depth falls towards the viewer
        assert rm.project(np.array([0, 1, 0], np.float32), view)[1] < cell / 2 < rm.project(np.array([0, -1, 0], np.float32), view)[1]
        rot = view[:, :3].astype(np.float64) / np.array([[0.48 * cell], [-0.48 * cell], [-0.5]])
        assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-6) and np.linalg.det(rot) > 0


def test_report_flags_default_to_off_and_parsing_is_unchanged_without_them():
    from pdgn_amd import train
    base = ["--model_dir", "m", "--choice", "chair", "--batch_size", "4"]
    args = train.parse_args(base)
    assert (args.report_every, args.report_rows, args.report_full) == (0, 8, False)
    rest = {k: v for k, v in vars(args).items() if not k.startswith("report_")}
    assert rest == {"phase": "train", "workers": 4, "gpu": 0, "batch_size": 4, "num_point": 2048, "num_k": 20, "learning_rate": 0.0001,
                    "max_epoch": 300, "noise_dim": 128, "optimizer": "adam", "debug": True,
                    "data_root": "/opt/data/private/shapenet/shapenet.hdf5", "log_info": "log_info.txt", "model_dir": "m",
                    "checkpoint_dir": "checkpoint", "snapshot": 20, "choice": "chair", "network": "PDGNet_v2", "savename": None,
                    "pretrain_model_G": None, "pretrain_model_D": None, "softmax": "True", "dataset": "shapenet15k",
                    "normalize": "shape_bbox", "seed": 9999, "save_dir": "./results", "device": "cuda"}
    on = train.parse_args(base + ["--report_every", "5", "--report_rows", "3", "--report_full"])
    assert (on.report_every, on.report_rows, on.report_full) == (5, 3, True)
    assert {k: v for k, v in vars(on).items() if not k.startswith("report_")} == rest
    for bad in (["--report_every", "-1"], ["--report_rows", "0"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)


def test_report_cli_parser():
    from pdgn_amd import report
    args = report.build_parser().parse_args(["out.npy", "-o", "sheet.png"])
    assert (args.clouds, args.output, args.rows, args.cell, args.radius) == ("out.npy", "sheet.png", 8, 128, 1)


def test_metric_reduction_reproduces_the_reference(golden):
    """The reduction stage of quick_metrics (evaluation.reduce_metrics) on the reference's own matrices; the tolerance of
    tests/test_evaluation_host.py for the same values."""
    from pdgn_amd import evaluation as ev
    from pdgn_amd.report import QUICK_KEYS
    g = golden("eval_metrics.npz")
    t = lambda k: torch.from_numpy(g[k])
    r = ev.reduce_metrics(t("all_dist"), t("Mxx"), t("Mxy"), t("Myy"), "CD")
    assert set(r) == set(QUICK_KEYS) - {"jsd"}
    for mine, theirs in (("lgan_mmd-CD", "lgan_mmd"), ("lgan_cov-CD", "lgan_cov"), ("lgan_mmd_smp-CD", "lgan_mmd_smp"),
                         ("1-NN-CD-acc", "knn_acc"), ("1-NN-CD-acc_t", "knn_acc_t"), ("1-NN-CD-acc_f", "knn_acc_f")):
        np.testing.assert_allclose(r[mine].numpy(), g[theirs], rtol=1e-6, atol=0)


def test_render_sheet_refuses_host_tensors():
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.report import render_sheet
    with pytest.raises(PdgnHipError):
        render_sheet(torch.zeros(1, 8, 3))


def test_log_line_of_a_run_without_reports_is_what_it_was():
    """--report_every 0 leaves the output files as they were: the args line of log_info.txt does not list the report flags."""
    from pdgn_amd import train
    base = ["--model_dir", "m", "--choice", "chair"]
    off = str(train.logged_args(train.parse_args(base)))
    assert "report_" not in off and off.startswith("Namespace(phase='train', workers=4,") and off.endswith("device='cuda')")
    on = str(train.logged_args(train.parse_args(base + ["--report_every", "20"])))
    assert on == off[:-1] + ", report_every=20, report_rows=8, report_full=False)"


def test_generator_forward_hints_round_trip():
    """What SnapshotReporter puts back after its forwards (PointGenerator.forward_hints / restore_forward_hints)."""
    from pdgn_amd.generator import PointGenerator
    G = PointGenerator(base_points=16)
    decs = G._deconvs()
    assert G.forward_hints() == [{}, {}, {}, {}]
    marker = object()
    for i, d in enumerate(decs[:3]):
        d._rows_hint = 100 + i
    decs[0]._pre = marker
    hints = G.forward_hints()
    assert hints == [{"_rows_hint": 100, "_pre": marker}, {"_rows_hint": 101}, {"_rows_hint": 102}, {}]
    for d in decs:
        d._rows_hint, d._pre = 7, None                                          # what forwards in between leave behind
    G.restore_forward_hints(hints)
    assert G.forward_hints() == hints and "_rows_hint" not in decs[3].__dict__ and "_pre" not in decs[1].__dict__
