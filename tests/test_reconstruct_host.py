"""Surface reconstruction without a device: what the rules of csrc/reconstruct.hip, as tests/reconstruct_mirror.py
states them, achieve -- closed, oriented, manifold meshes of a sphere and of tori, two components for nested spheres, a rim for half a
sphere -- that culling changes no bit, the output order, the edge cases (f = 0, no valid node, dead points, one cell), mesh_report itself,
the PLY and OBJ writers, the export parser's refusals and the header."""
import re
import struct

import numpy as np
import pytest
import torch

import normals_mirror as nm
import orient_mirror as om
import reconstruct_mirror as rm
from pdgn_amd import reconstruct                                    # (host side only here: mesh_report, to_meshset, the refusals)

F = np.float32
TORUS_VOLUME = 2 * np.pi ** 2 * 1.0 * 0.4 ** 2                     # 3.158
# measured on the mirror (seeds 0 .. 7 of om.torus(2048, .), R = 40, radius_factor 5): the volume is 3.229 .. 3.233, +2.2 % to +2.4 % (IMLS
# pushes convex parts outwards); twice the larger figure is the bound, and never more than 10 %
TORUS_DEVIATION = 0.024
# the sphere's vertices: |v| - 1 is 0.0224 .. 0.0256 on the mirror (512 points, R = 32, radius_factor 3)
SPHERE_EXCESS = 0.0256


def _report(verts, faces):
    return reconstruct.mesh_report(verts, faces)


def _closed(rep):
    return rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["oriented"]


@pytest.fixture(scope="module")
def sphere():
    x, g = rm.fibonacci_sphere(512)
    return (x, g) + rm.reconstruct_cloud(x, g, 32, radius_factor=3.0)


@pytest.fixture(scope="module")
def tori():
    out = {}
    for seed in (0, 1):
        x, truth = om.torus(2048, seed)
        out[seed] = (x, truth.astype(F)) + rm.reconstruct_cloud(x, truth.astype(F), 40, radius_factor=5.0)
    return out


def test_the_sphere_is_closed_oriented_and_just_outside_the_unit_sphere(sphere):
    x, g, verts, faces, stats, grid, field = sphere
    rep = _report(verts, faces)
    radius = np.linalg.norm(verts.astype(np.float64), axis=1)
    print(rep, stats, radius.min(), radius.max())
    assert _closed(rep) and rep["components"] == 1 and rep["euler"] == 2 and rep["volume"] > 0
    assert stats[0] == verts.shape[0] == rep["vertices"] and stats[1] == faces.shape[0] and stats[2] == 0
    assert (radius > 1.0).all() and radius.max() - 1.0 <= 2 * SPHERE_EXCESS
    assert abs(rep["area"] / (4 * np.pi) - 1) < 0.1


def test_the_tori_are_closed_with_euler_characteristic_zero_and_the_right_volume(tori):
    for seed, (x, g, verts, faces, stats, grid, field) in tori.items():
        rep = _report(verts, faces)
        print(seed, rep, stats)
        assert _closed(rep) and rep["components"] == 1 and rep["euler"] == 0, seed
        assert stats[2] == 0 and abs(rep["volume"] / TORUS_VOLUME - 1) <= min(2 * TORUS_DEVIATION, 0.10), seed


@pytest.mark.parametrize("seed", rm.EXPORT_SEEDS)
def test_the_chain_of_mirrors_closes_the_tori_the_export_test_runs_on_the_device(seed):
    """normals_mirror at k = 16, orient_mirror, reconstruct_mirror at R = 40, radius_factor 5: what `python -m pdgn_amd.export --mesh 40`
    computes on the device, on the host."""
    x, truth = om.torus(2048, seed)
    idx = nm.knn_indices(x, 16)
    o, parent, ostats = om.orient_cloud(x, nm.estimate_cloud(x, idx)[0], idx)
    assert ostats[0] == 1 and ((o.astype(np.float64) * truth).sum(axis=1) > 0).all()
    verts, faces, stats, grid, field = rm.reconstruct_cloud(x, o, 40, radius_factor=5.0)
    rep = _report(verts, faces)
    print(seed, rep, stats)
    assert _closed(rep) and rep["components"] == 1 and rep["euler"] == 0 and stats[2] == 0
    assert abs(rep["volume"] / TORUS_VOLUME - 1) <= min(2 * TORUS_DEVIATION, 0.10)


def test_nested_spheres_are_two_components_and_inward_normals_give_a_negative_volume():
    outer, go = rm.fibonacci_sphere(512)
    inner, gi = rm.fibonacci_sphere(256, 0.45)
    x, g = np.concatenate([outer, inner]), np.concatenate([go, -gi])
    verts, faces, stats, grid, field = rm.reconstruct_cloud(x, g, 36, radius=0.3)
    rep = _report(verts, faces)
    assert _closed(rep) and rep["components"] == 2 and rep["euler"] == 4
    near = np.linalg.norm(verts.astype(np.float64), axis=1) < 0.7
    inner_faces = faces[near[faces[:, 0]]]
    assert near[inner_faces].all() and 0 < inner_faces.shape[0] < faces.shape[0]
    shell, ball = _report(verts, inner_faces), _report(verts, faces[~near[faces[:, 0]]])
    print(shell, ball)
    assert shell["volume"] < 0 < ball["volume"] and _closed(shell) and _closed(ball)
    assert abs(rep["volume"] - (ball["volume"] + shell["volume"])) < 1e-9


def test_half_a_sphere_has_a_rim_and_no_quad_touches_an_invalid_node():
    x, g = rm.fibonacci_sphere(1024)
    keep = x[:, 2] > 0
    verts, faces, stats, (origin, voxel, inv), field = rm.reconstruct_cloud(x[keep], g[keep], 32, radius_factor=3.0)
    rep = _report(verts, faces)
    print(rep, stats)
    assert rep["boundary_edges"] > 0 and rep["nonmanifold_edges"] == 0 and rep["components"] == 1 and rep["euler"] == 1
    assert stats[2] > 0 and stats[3] > 0                            # open edges are counted, and there are invalid nodes
    # every vertex comes from a cell whose eight corners are valid
    cell = np.floor((verts.astype(np.float64) - origin.astype(np.float64)) / float(voxel) + 1e-6).astype(int)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                assert not np.isnan(field[cell[:, 0] + a, cell[:, 1] + b, cell[:, 2] + c]).any()


def test_culling_changes_no_bit_and_an_explicit_mask_may_drop_only_what_cannot_reach(sphere, tori):
    for x, g, verts, faces, stats, (origin, voxel, inv), field in (sphere, tori[0]):
        R = field.shape[0]
        plain = rm.field_cloud(x, g, origin, voxel, inv, R, cull=False)
        assert rm.bits_equal(plain.reshape(R, R, R), field)         # (reconstruct_cloud culls)
        skip = rm.brick_skips(x, origin, voxel, inv, R)
        assert 0.5 < skip.mean() < 1.0
        thinned = skip & (np.random.default_rng(2).random(skip.shape) < 0.5)               # any subset of what may be dropped
        assert rm.bits_equal(rm.field_cloud(x, g, origin, voxel, inv, R, skip=thinned), plain)
    # the test is sharp where it has to be: dropping ONE point at ONE brick that it can reach changes the field there and nowhere else
    x, g, verts, faces, stats, (origin, voxel, inv), field = sphere
    skip = rm.brick_skips(x, origin, voxel, inv, 32)
    assert skip.shape == (512, 8, 8, 8)
    reached = np.zeros(skip.shape, dtype=bool)                      # (point, brick) pairs with t > 0 at some node of the brick
    P = rm.node_positions(origin, voxel, 32).reshape(32, 32, 32, 3)
    for j in (0, 200, 511):
        d = (P - x[j]).astype(F)
        t = (F(1.0) - (nm.dot3(d, d).astype(F) * inv).astype(F)).astype(F)
        reached[j] = (t > 0).reshape(8, 4, 8, 4, 8, 4).any(axis=(1, 3, 5))
        assert reached[j].any() and not (reached[j] & skip[j]).any()
        bi, bj, bk = np.argwhere(reached[j])[0]
        wrong = skip.copy()
        wrong[j, bi, bj, bk] = True
        other = rm.field_cloud(x, g, origin, voxel, inv, 32, skip=wrong).reshape(32, 32, 32)
        differs = other.view(np.uint32) != field.view(np.uint32)
        assert differs.any() and not differs.reshape(8, 4, 8, 4, 8, 4).any(axis=(1, 3, 5))[~(np.arange(512).reshape(8, 8, 8) == (bi * 8 + bj) * 8 + bk)].any()


def test_shuffled_points_change_the_field_in_the_last_bits_only(sphere):
    x, g, verts, faces, stats, (origin, voxel, inv), field = sphere
    perm = np.random.default_rng(1).permutation(x.shape[0])
    other = rm.field_cloud(x[perm], g[perm], origin, voxel, inv, 32, cull=True).reshape(32, 32, 32)
    assert np.array_equal(np.isnan(other), np.isnan(field))
    ok = ~np.isnan(field)
    assert np.abs(other[ok].astype(np.float64) - field[ok]).max() < 1e-5


def test_vertices_come_by_ascending_cell_and_faces_by_ascending_key(tori):
    x, g, verts, faces, stats, (origin, voxel, inv), field = tori[1]
    R = field.shape[0]
    C = R - 1
    active = rm.active_cells(field)
    cells = np.stack(np.nonzero(active), axis=1)                    # ascending cell id
    assert cells.shape[0] == verts.shape[0]
    local = (verts.astype(np.float64) - origin.astype(np.float64)) / float(voxel) - cells
    assert (local > -1e-4).all() and (local < 1 + 1e-4).all()       # vertex r lies in the r-th active cell
    # a quad's four cells share exactly one grid edge: its low node and axis give the key
    quads = np.concatenate([faces[0::2], faces[1::2][:, 2:]], axis=1)
    assert (faces[0::2, 0] == faces[1::2, 0]).all() and (faces[0::2, 2] == faces[1::2, 1]).all()
    qc = cells[quads]                                               # (Q,4,3)
    lo, hi = qc.min(axis=1), qc.max(axis=1)
    axis = np.argmin(hi - lo, axis=1)
    assert ((hi - lo).sum(axis=1) == 2).all()
    node = hi.copy()
    node[np.arange(node.shape[0]), axis] = lo[np.arange(node.shape[0]), axis]
    key = 3 * ((node[:, 0] * R + node[:, 1]) * R + node[:, 2]) + axis
    assert (np.diff(key) > 0).all()


def test_nodes_exactly_on_a_plane_of_points_count_as_outside():
    """Points on z = 0 with normals +z on a grid with nodes at z = 0: there f = 0 exactly (every d . g is 0), which is outside; the crossing
    is between the nodes below (f < 0) and those on the plane, at t = 1, so the vertices lie on z = 0 exactly."""
    ii, jj = np.meshgrid(np.arange(-8, 9), np.arange(-8, 9), indexing="ij")
    x = np.stack([ii.ravel() * 0.125, jj.ravel() * 0.125, np.zeros(ii.size)], axis=1).astype(F)
    g = np.tile(np.array([[0, 0, 1]], F), (x.shape[0], 1))
    origin, voxel, inv, R = np.array([-1, -1, -1], F), F(0.25), F(1.0 / 0.3 ** 2), 9
    f = rm.field_cloud(x, g, origin, voxel, inv, R).reshape(R, R, R)
    on_plane = f[:, :, 4]
    assert (on_plane == 0).all() and (f[:, :, 3] < 0).all() and (f[:, :, 5] > 0).all() and np.isnan(f[:, :, 0]).all()
    verts, faces, stats = rm.surface_nets_cloud(f, origin, voxel)
    assert verts.shape[0] == 64 and (verts[:, 2] == 0).all() and stats[1] == 2 * 49 and stats[2] == 81 - 49
    assert rm.bits_equal(verts[0], np.array([-0.875, -0.875, 0.0], F))     # the cell's centre in x and y, the plane in z
    rep = _report(verts, faces)
    assert rep["volume"] == 0 and rep["boundary_edges"] == 28 and rep["euler"] == 1
    normal = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    assert (normal[:, 2] > 0).all()                                 # counter-clockwise seen from outside (+z)


def test_h_too_small_for_any_node_gives_nothing():
    x, g = rm.fibonacci_sphere(64)
    origin, voxel, inv = rm.grid_for(x, 9, 1e-4)
    f = rm.field_cloud(x, g, origin, voxel, inv, 9)
    assert (f.view(np.uint32) == rm.NAN_BITS).all()
    verts, faces, vert_off, face_off, stats = rm.surface_nets(np.stack([f.reshape(9, 9, 9)] * 2), [origin] * 2, [voxel] * 2)
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and faces.dtype == np.int32
    assert (vert_off == 0).all() and (face_off == 0).all() and stats.tolist() == [[0, 0, 0, 729]] * 2


def test_dead_points_change_nothing(sphere):
    x, g, verts, faces, stats, (origin, voxel, inv), field = sphere
    x2 = np.concatenate([x[:100], np.zeros((3, 3), F), x[100:]])
    g2 = np.concatenate([g[:100], np.ones((3, 3), F), g[100:]])
    x2[100, 0], g2[101, 1], x2[102, 2] = np.inf, np.nan, np.nan
    for cull in (False, True):
        assert rm.bits_equal(rm.field_cloud(x2, g2, origin, voxel, inv, 32, cull=cull).reshape(32, 32, 32), field)
    o2, v2, i2 = rm.grid_for(x2, 32, 0.3)
    o1, v1, i1 = rm.grid_for(x, 32, 0.3)
    assert rm.bits_equal(o2, o1) and v2 == v1 and i2 == i1          # the box ignores them too


def test_a_single_cell():
    f = np.array([[[-1, 1], [1, 1]], [[1, 1], [1, 1]]], F)
    verts, faces, stats = rm.surface_nets_cloud(f, np.zeros(3, F), F(1.0))
    assert stats == (1, 0, 3, 0) and faces.shape == (0, 3)
    third = F(0.5) / F(3.0)
    assert rm.bits_equal(verts, np.full((1, 3), third, F))
    f[1, 1, 1] = np.nan                                             # a corner without data: no active cell, the three edges stay open
    assert rm.surface_nets_cloud(f, np.zeros(3, F), F(1.0))[2] == (0, 0, 3, 1)


def test_mesh_report_on_known_meshes():
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
    rep = _report(tet_v, tet_f)
    assert _closed(rep) and rep["euler"] == 2 and rep["components"] == 1 and abs(rep["volume"] - 1 / 6) < 1e-12
    assert abs(rep["area"] - (1.5 + np.sqrt(3) / 2)) < 1e-6
    assert _report(tet_v, tet_f[:, ::-1])["volume"] < 0
    flipped = tet_f.copy()
    flipped[0] = flipped[0, ::-1]
    assert not _report(tet_v, flipped)["oriented"]
    assert _report(tet_v, tet_f[:3])["boundary_edges"] == 3
    fan = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int32)    # three triangles on one edge
    assert _report(np.concatenate([tet_v, [[0, 0, -1]]]).astype(F), fan)["nonmanifold_edges"] == 1
    two = _report(np.concatenate([tet_v, tet_v + 5]), np.concatenate([tet_f, tet_f + 4]))
    assert two["components"] == 2 and two["euler"] == 4
    with pytest.raises(ValueError):
        _report(tet_v, tet_f + 1)
    empty = _report(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    assert empty["faces"] == 0 and empty["components"] == 0 and empty["oriented"]


# ---------------------------------------------------------------------------- writers, parser, header
def _todays_write_ply(path, xyz, normals=None):
    """The cloud writer as it stood before faces were added, kept here to compare bytes against."""
    rows = np.asarray(xyz).astype("<f4")
    if normals is not None:
        rows = np.concatenate([rows, np.asarray(normals).astype("<f4")], axis=1)
    header = ["ply", "format binary_little_endian 1.0", "comment pdgn_amd.export", "element vertex %d" % rows.shape[0]]
    header += ["property float %s" % name for name in ("x", "y", "z", "nx", "ny", "nz")[:rows.shape[1]]]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii") + np.ascontiguousarray(rows).tobytes())


def test_write_ply_with_faces_reads_back_and_without_is_byte_equal(tmp_path, sphere):
    from pdgn_amd import export
    x, g, verts, faces, stats, grid, field = sphere
    export.write_ply(tmp_path / "m.ply", verts, faces=faces)
    raw = open(tmp_path / "m.ply", "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "comment pdgn_amd.export"]
    assert lines[3:] == ["element vertex %d" % verts.shape[0], "property float x", "property float y", "property float z",
                         "element face %d" % faces.shape[0], "property list uchar int vertex_indices"]
    V, Fc = verts.shape[0], faces.shape[0]
    assert len(body) == 12 * V + 13 * Fc
    assert rm.bits_equal(np.array(struct.unpack("<%df" % (3 * V), body[:12 * V]), dtype=F).reshape(V, 3), verts)
    rec = [struct.unpack_from("<B3i", body, 12 * V + 13 * i) for i in range(Fc)]
    assert all(r[0] == 3 for r in rec) and np.array_equal(np.array([r[1:] for r in rec], np.int32), faces)
    export.write_ply(tmp_path / "t.ply", torch.from_numpy(verts), torch.from_numpy(g[:V] if V <= g.shape[0] else np.zeros_like(verts)),
                     faces=torch.from_numpy(faces))
    assert open(tmp_path / "t.ply", "rb").read().count(b"property float") == 6
    for normals in (None, g):
        export.write_ply(tmp_path / "a.ply", x, normals)
        _todays_write_ply(tmp_path / "b.ply", x, normals)
        assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    for bad in (faces.astype(F), faces[:, :2], faces + V, -faces - 1):
        with pytest.raises(ValueError):
            export.write_ply(tmp_path / "bad.ply", verts, faces=bad)
    assert not (tmp_path / "bad.ply").exists()


def test_write_obj_round_trips_through_load_obj(tmp_path, sphere):
    from pdgn_amd import export
    from pdgn_amd.meshes import load_obj
    x, g, verts, faces, stats, grid, field = sphere
    export.write_obj(tmp_path / "m.obj", verts, faces)
    v, f = load_obj(str(tmp_path / "m.obj"))
    assert rm.bits_equal(v, verts) and np.array_equal(f, faces) and f.dtype == np.int32
    with pytest.raises(ValueError):
        export.write_obj(tmp_path / "bad.obj", verts, faces + verts.shape[0])
    with pytest.raises(ValueError):
        export.write_obj(tmp_path / "bad.obj", verts.astype(np.int32), faces)


def test_to_meshset_takes_global_indices(sphere):
    x, g, verts, faces, stats, grid, field = sphere
    V, Fc = verts.shape[0], faces.shape[0]
    ms = reconstruct.to_meshset(np.concatenate([verts, verts + 3]), np.concatenate([faces, faces]), [0, V, 2 * V], [0, Fc, 2 * Fc])
    assert ms.S == 2 and ms.V == 2 * V and ms.F == 2 * Fc
    assert np.array_equal(ms.faces.numpy()[Fc:], faces + V) and ms.faces.dtype == torch.int32


def test_the_export_parser_takes_mesh_and_refuses_what_it_cannot_do(tmp_path, capsys):
    from pdgn_amd import export
    args = export.build_parser().parse_args(["out.npy", "-o", "d", "--mesh", "64", "--mesh_radius_factor", "4", "--mesh_format", "obj"])
    assert args.mesh == 64 and args.mesh_radius_factor == 4.0 and args.mesh_format == "obj" and args.mesh_radius is None
    plain = export.build_parser().parse_args(["out.npy", "-o", "d"])
    assert plain.mesh is None and plain.orient == "outward" and plain.normals is None and plain.mesh_format == "ply"
    cloud = tmp_path / "c.npy"
    np.save(cloud, np.zeros((1, 64, 3), F))
    out = str(tmp_path / "out")
    for bad, said in ((["--mesh", "32", "--orient", "none"], "oriented normals"), (["--mesh", "1"], "between 2 and 256"),
                      (["--mesh", "257"], "between 2 and 256"), (["--mesh", "32", "--mesh_radius", "0.1", "--mesh_radius_factor", "3"], "exclude"),
                      (["--mesh", "32", "--mesh_radius", "-1"], "positive"), (["--mesh_radius", "0.1"], "go with --mesh"),
                      (["--mesh_format", "obj"], "go with --mesh"), (["--mesh", "32", "--mesh_format", "stl"], "invalid choice")):
        with pytest.raises(SystemExit):
            export.main([str(cloud), "-o", out] + bad)
        assert said in capsys.readouterr().err, bad
    big = tmp_path / "big.npy"
    np.save(big, np.zeros((1, export.CONSISTENT_MAX_POINTS + 1, 3), F))
    with pytest.raises(SystemExit):                                 # --mesh implies --orient consistent, and with it the 4096-point limit
        export.main([str(big), "-o", out, "--mesh", "32"])
    assert "at most 4096 points" in capsys.readouterr().err and not (tmp_path / "out").exists()
    assert "--mesh 64" in export.__doc__


def test_the_wrappers_refuse_host_tensors_and_bad_arguments():
    from pdgn_amd._lib import PdgnHipError
    x = torch.zeros(1, 8, 3)
    for call in (lambda: reconstruct.imls_field(x, x), lambda: reconstruct.reconstruct(x), lambda: reconstruct.grid_for(x, 8, 0.1),
                 lambda: reconstruct.surface_nets(torch.zeros(1, 4, 4, 4), torch.zeros(1, 3), torch.ones(1))):
        with pytest.raises(PdgnHipError):
            call()
    with pytest.raises(TypeError):
        reconstruct.imls_field(np.zeros((1, 8, 3), F), x)
    assert reconstruct.MIN_RESOLUTION == rm.MIN_R == 2 and reconstruct.MAX_RESOLUTION == rm.MAX_R == 256
    for fn in (reconstruct.imls_field, reconstruct.surface_nets, reconstruct.reconstruct, reconstruct.grid_for, reconstruct.mesh_report):
        assert fn.__doc__


def test_the_header_declares_the_entry_points_and_the_limits():
    from pdgn_amd import _lib
    vp, i, ll = _lib.ctypes.c_void_p, _lib.ctypes.c_int, _lib.ctypes.c_longlong
    assert _lib.SIGNATURES["pdgn_imls_grid"] == (i, (i, i, i, vp, vp, vp, vp, i, vp, vp))
    assert "pdgn_imls_set_cull" not in _lib.SIGNATURES and _lib.SIGNATURES["pdgn_imls_chunk"] == (i, ())
    assert _lib.SIGNATURES["pdgn_surface_nets_count"] == (i, (i, i, vp, vp, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_surface_nets_emit"] == (i, (i, i) + (vp,) * 9 + (ll,) * 4 + (vp, vp, vp))
    text = open(_lib.HEADER).read()
    assert int(re.search(r"#define PDGN_RECON_MIN_R (\d+)", text).group(1)) == rm.MIN_R
    assert int(re.search(r"#define PDGN_RECON_MAX_R (\d+)", text).group(1)) == rm.MAX_R
    assert _lib.ABI_VERSION >= 45
    # the library and the mirror state the same rules
    import os
    src = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "pdgn_amd", "csrc", "reconstruct.hip")).read()
    for phrase in ("NORMATIVE ORDER", "t = 1 - d2 * inv", "0x7FC00000", "(-1,-1), (0,-1), (0,0), (-1,0)", "3 (node id) + A"):
        assert phrase in src and phrase in rm.__doc__, phrase
