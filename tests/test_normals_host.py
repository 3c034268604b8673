"""Surface normals on the host: the numpy mirror of csrc/normals.hip (tests/normals_mirror.py) against float64
eigh, its exact cases, the poison rules and the sign modes; the PLY writer; render_sheet's `normals` argument; the command lines."""
import argparse
import re

import numpy as np
import pytest
import torch

import normals_mirror as nm

F = np.float32
BASE = ["--model_dir", "m"]
# Measured on the five seeded clouds below, k = 8 and 16 (the figures each run prints): the largest angle x gap is 7.8e-6 degrees, the
# largest eigenvalue error 2.41e-7 lambda2 (three other seeds: 9.0e-6 and 2.41e-7).  Each bound is ten times its measured maximum: the
# margin covers other seeds, not other arithmetic.
ANGLE_GAP_BOUND = 7.8e-5
EIG_BOUND = 2.41e-6


@pytest.fixture(scope="module")
def clouds():
    return nm.accuracy_clouds(0)


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("name", ["sphere512", "cube512", "noisy512", "sphere64", "blob256"])
def test_the_mirror_agrees_with_float64_eigh_on_every_point(clouds, name, k):
    """angle to the fp64 normal [degrees] x (lambda1 - lambda0) / lambda2 over ALL points (where the two smallest eigenvalues meet the
    normal is not defined, and the product stays small there anyway), and |eig - eig64| / lambda2."""
    x = clouds[name]
    angle_gap, eig_err = nm.against_eigh(x, nm.knn_indices(x, k))
    print("%s k=%d: angle x gap %.3g degrees (bound %.3g), eigenvalues %.3g lambda2 (bound %.3g)" % (name, k, angle_gap, ANGLE_GAP_BOUND, eig_err, EIG_BOUND))
    assert angle_gap <= ANGLE_GAP_BOUND and eig_err <= EIG_BOUND


def test_the_outputs_no_longer_change_after_four_sweeps(clouds):
    x = clouds["noisy512"]
    a, _ = nm.covariance(x, nm.knn_indices(x, 16).astype(np.int64))
    four, five, six = (nm.select(*nm.jacobi(a, s)) for s in (4, 5, 6))
    assert nm.SWEEPS == 5
    for got in (four, six):
        assert nm.same_bits(got[0], five[0]) and nm.same_bits(got[1], five[1])


def planar_grid():
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 2) / 8.0
    return np.concatenate([g, np.full((64, 1), 0.25)], axis=1).astype(F)


def test_a_planar_grid_has_exact_normals_and_an_exact_zero():
    """z = 0.25 everywhere, k = 9: the mean's z is 2.25 * fl(1/9) = 0.25 after rounding, so the z row and column of the covariance are
    exact zeros, no rotation touches them, and V's third column stays (0, 0, 1)."""
    x = planar_grid()
    normal, eig = nm.estimate_cloud(x, nm.knn_indices(x, 9))
    assert np.array_equal(normal, np.tile(np.array([[0, 0, 1]], F), (64, 1)))
    assert np.array_equal(eig[:, 0], np.zeros(64, F)) and (eig[:, 1] > 0).all() and (eig[:, 1] <= eig[:, 2]).all()


def test_one_point_and_equal_points_give_the_first_axis_and_zeros():
    """No off-diagonal element is ever non-zero: V stays the identity, and of three equal eigenvalues the lowest column comes first.  The
    equal points sit on dyadic coordinates with k a power of two, where the mean is exact (elsewhere the mean of k copies of x may differ from
    x in the last bit and leave eigenvalues of the order of 1e-16 |x|^2)."""
    p = np.array([[0.3, 0.1, -2.0]], F)
    normal, eig = nm.estimate_cloud(p, np.zeros((1, 1), np.int32))
    assert np.array_equal(normal, [[1, 0, 0]]) and np.array_equal(eig, np.zeros((1, 3), F))
    x = np.tile(np.array([[0.375, -1.5, 0.0625]], F), (10, 1))
    for k in (1, 4, 8):
        normal, eig = nm.estimate_cloud(x, nm.knn_indices(x, k))
        assert np.array_equal(normal, np.tile(np.array([[1, 0, 0]], F), (10, 1))) and np.array_equal(eig, np.zeros((10, 3), F))
        assert not np.signbit(eig).any()


def test_poison_reaches_exactly_the_points_the_rules_name(clouds):
    x = clouds["sphere64"].copy()
    idx = nm.knn_indices(x, 8)
    clean_n, clean_e = nm.estimate_cloud(x, idx)
    assert np.isfinite(clean_n).all() and np.isfinite(clean_e).all()
    # an index outside [0, n): that point alone, whatever the other seven are
    bad = idx.copy()
    bad[5, 3], bad[9, 0], bad[11, 7] = 64, -1, 2 ** 31 - 1
    n1, e1 = nm.estimate_cloud(x, bad)
    hit = np.zeros(64, bool)
    hit[[5, 9, 11]] = True
    assert np.isnan(n1[hit]).all() and np.isnan(e1[hit]).all()
    assert nm.same_bits(n1[~hit], clean_n[~hit]) and nm.same_bits(e1[~hit], clean_e[~hit])
    # a NaN (or infinite) coordinate: every point that has it among its neighbours, and no other
    for value in (np.nan, np.inf):
        y = x.copy()
        y[20, 1] = value
        n2, e2 = nm.estimate_cloud(y, idx)
        hit = (idx == 20).any(axis=1)
        assert 1 < hit.sum() < 64
        assert np.isnan(n2[hit]).all() and np.isnan(e2[hit]).all()
        assert nm.same_bits(n2[~hit], clean_n[~hit]) and nm.same_bits(e2[~hit], clean_e[~hit])


def test_the_four_orient_modes(clouds):
    x = clouds["sphere512"]
    idx = nm.knn_indices(x, 16)
    plain, eig = nm.estimate_cloud(x, idx)
    lead = np.take_along_axis(plain, np.abs(plain).argmax(axis=1)[:, None], axis=1)[:, 0]
    assert (lead > 0).all()                                         # orient 0: the largest component is positive
    o = np.array([0.3, -0.2, 0.9], F)
    along, _ = nm.estimate_cloud(x, idx, 1, o)
    assert (nm.dot3(along, np.broadcast_to(o, x.shape)) >= 0).all()
    centre = np.array([0.0, 0.0, 0.0], F)
    away, eig_away = nm.estimate_cloud(x, idx, 3, centre)
    towards, _ = nm.estimate_cloud(x, idx, 2, centre)
    assert (nm.dot3(away, x) > 0.9).all()                           # a unit sphere about the origin: the outward normal is x itself
    assert nm.same_bits(towards, -away) and nm.same_bits(eig_away, eig)
    for other in (along, away, towards):                            # a mode changes signs and nothing else
        assert np.array_equal(np.abs(other), np.abs(plain))
    off = np.array([0.0, 0.0, 5.0], F)                              # a position outside the sphere: every normal turns to it
    assert (nm.dot3(nm.estimate_cloud(x, idx, 2, off)[0], off - x) >= 0).all()


# ---------------------------------------------------------------------------- the lit shade
def test_the_lit_shade_spans_48_to_255_and_is_two_sided():
    light = np.array([0.0, 0.0, 1.0], F)
    n = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 0.6, 0.8], [np.nan, 0, 1], [0, 0, 2]], F)
    assert nm.lit_shade(n, light).tolist() == [255, 255, 48, 48 + int(F(207.0) * F(0.8)), 48, 255]


def test_the_lit_mirror_without_normals_is_the_depth_mirror():
    import render_mirror as rm
    clouds = rm.lattice_clouds(2, 128, 3)
    view = rm.LATTICE_VIEWS["tilted"]
    assert np.array_equal(nm.render_lit(clouds, [None, None], view, view[2, :3], 128, 1), rm.render(clouds, view, 128, 1))
    lit = nm.render_lit(clouds, [np.zeros_like(clouds[0]), None], view, view[2, :3], 128, 1)        # zero normals: the darkest shade
    assert set(np.unique(lit[:, :128])) == {0, 48} and np.array_equal(lit[:, 128:], rm.render(clouds, view, 128, 1)[:, 128:])


# ---------------------------------------------------------------------------- PLY
def _read_ply(data):
    head, payload = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    (count,) = [int(l.split()[2]) for l in lines if l.startswith("element vertex")]
    props = [l.split() for l in lines if l.startswith("property")]
    assert all(p[1] == "float" for p in props) and not any(l.startswith("element face") for l in lines)
    return count, [p[2] for p in props], payload


@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_round_trip_keeps_every_bit(tmp_path, with_normals):
    from pdgn_amd.export import write_ply
    rng = np.random.default_rng(4)
    xyz = rng.standard_normal((37, 3)).astype(F)
    xyz[3, 1], xyz[4, 0] = np.nan, -0.0
    normals = rng.standard_normal((37, 3)).astype(F) if with_normals else None
    path = write_ply(str(tmp_path / "c.ply"), xyz if with_normals else torch.from_numpy(xyz), normals)
    count, names, payload = _read_ply(open(path, "rb").read())
    assert count == 37 and names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else [])
    got = np.frombuffer(payload, dtype="<f4").reshape(37, len(names))
    want = np.concatenate([xyz, normals], axis=1) if with_normals else xyz
    assert got.tobytes() == want.astype("<f4").tobytes()
    for bad in (np.zeros((0, 3), F), np.zeros((4, 2), F), np.zeros((4, 3), np.int32)):
        with pytest.raises(ValueError):
            write_ply(str(tmp_path / "bad.ply"), bad)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "bad.ply"), xyz, xyz[:5])


def test_export_parser():
    from pdgn_amd import export
    args = export.build_parser().parse_args(["out.npy", "-o", "d", "--first", "2", "--count", "3", "--normals", "12", "--orient", "none"])
    assert (args.clouds, args.output, args.first, args.count, args.normals, args.orient) == ("out.npy", "d", 2, 3, 12, "none")
    assert export.build_parser().parse_args(["out.npy", "-o", "d"]).orient == "outward"
    with pytest.raises(SystemExit):
        export.build_parser().parse_args(["out.npy", "-o", "d", "--orient", "inward"])
    assert "heuristic" in export.main.__doc__ and "convex" in export.main.__doc__


def test_export_without_normals_needs_no_device(tmp_path):
    from pdgn_amd import export
    pcs = np.random.default_rng(1).standard_normal((5, 3, 16)).astype(F)         # the reference's (S, 3, N) layout
    np.save(tmp_path / "out.npy", pcs)
    export.main([str(tmp_path / "out.npy"), "-o", str(tmp_path / "plys"), "--first", "1", "--count", "2"])
    assert sorted(p.name for p in (tmp_path / "plys").iterdir()) == ["cloud_1.ply", "cloud_2.ply"]
    count, names, payload = _read_ply((tmp_path / "plys" / "cloud_2.ply").read_bytes())
    assert count == 16 and names == ["x", "y", "z"]
    assert np.array_equal(np.frombuffer(payload, dtype="<f4").reshape(16, 3), pcs[2].T)


# ---------------------------------------------------------------------------- arguments
def test_render_sheet_checks_the_form_of_normals_before_the_device():
    """What is wrong with `normals` or `light` by its form alone is refused before the clouds are looked at -- here they are host
    tensors, which render_sheet refuses next (no CPU path)."""
    from pdgn_amd._lib import PdgnHipError
    from pdgn_amd.report import render_sheet
    x = torch.zeros(2, 16, 3)
    for bad in ("shade", ["estimate"], ["estimate", None, None], torch.zeros(2, 16, 3), 7, ["estimate", "flat"]):
        with pytest.raises(ValueError):
            render_sheet([x, x], normals=bad)
    with pytest.raises(TypeError):
        render_sheet([x, x], normals=[np.zeros((2, 16, 3), F), None])
    with pytest.raises(ValueError):
        render_sheet([x, x], normals="estimate", normals_k=0)
    for light in ((0, 0, 0), (1, 2), (np.nan, 0, 1)):
        with pytest.raises(ValueError):
            render_sheet([x, x], normals="estimate", light=light)
    for fine in ("estimate", ["estimate", None], [None, None], [torch.zeros(2, 16, 3), None]):
        with pytest.raises(PdgnHipError):                           # the form is fine: the host tensors are what is refused
            render_sheet([x, x], normals=fine, light=(0, 0, 2))
    with pytest.raises(PdgnHipError):
        render_sheet([x, x])


def test_estimate_normals_and_surface_stats_refuse_host_tensors():
    from pdgn_amd import evaluation, pointops
    from pdgn_amd._lib import PdgnHipError
    with pytest.raises(PdgnHipError):
        pointops.estimate_normals(torch.zeros(1, 8, 3))
    with pytest.raises(PdgnHipError):
        evaluation.surface_stats(torch.zeros(1, 8, 3))
    assert "differentiable" in pointops.estimate_normals.__doc__


def test_the_parsers_take_the_flags_and_the_default_namespace_is_what_it_was(capsys):
    from pdgn_amd import report, train
    args = train.parse_args(BASE)
    assert not args.report_lit and not args.report_surface
    assert not any(k in ("report_lit", "report_surface") for k in vars(args))
    got = train.parse_args(BASE + ["--report_every", "5", "--report_lit", "--report_surface"])
    assert got.report_lit is True and got.report_surface is True
    for bad in (["--report_lit"], ["--report_surface"], ["--report_lit", "--report_surface"], ["--report_spacing"]):
        with pytest.raises(SystemExit):
            train.parse_args(BASE + bad)
        assert "needs --report_every" in capsys.readouterr().err, bad
    for dest in ("report_lit", "report_surface"):
        action = [a for a in train.build_parser()._actions if a.dest == dest]
        assert len(action) == 1 and action[0].default is argparse.SUPPRESS, dest
    assert "--report_lit" in train.__doc__ and "--report_surface" in train.__doc__
    args = report.build_parser().parse_args(["out.npy", "-o", "s.png", "--lit"])
    assert args.lit is True and report.build_parser().parse_args(["out.npy"]).lit is False


def test_the_header_declares_both_entry_points_and_the_limits():
    from pdgn_amd import _lib
    vp, i, f = _lib.ctypes.c_void_p, _lib.ctypes.c_int, _lib.ctypes.c_float
    assert _lib.SIGNATURES["pdgn_estimate_normals"] == (i, (i, i, i, vp, vp, i, f, f, f, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_render_sheet_lit"] == (i, (i, i, vp, vp, vp, i, vp, vp, i, i, vp, vp, vp))
    text = open(_lib.HEADER).read()
    assert int(re.search(r"#define PDGN_NORMALS_MAX_K (\d+)", text).group(1)) == nm.MAX_K == 64
    assert int(re.search(r"#define PDGN_NORMALS_SWEEPS (\d+)", text).group(1)) == nm.SWEEPS == 5
    assert int(re.search(r"#define PDGN_NORMALS_STAGE_MAX_N (\d+)", text).group(1)) == 4096      # tests/test_gpu_normals.py straddles it
