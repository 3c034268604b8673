"""Consistent normal orientation without a device: what the rules of csrc/orient.hip, as tests/orient_mirror.py
states them, achieve on shapes with concavities and several components; that the tree they grow is a minimum spanning forest; that the
outputs differ from the inputs in sign bits alone and do not depend on how the lists are written; poison; the wrappers' and the export
parser's refusals."""
import re

import numpy as np
import pytest
import torch

import normals_mirror as nm
import orient_mirror as om

F = np.float32


def _estimate(x, k):
    idx = nm.knn_indices(x, k)
    return idx, nm.estimate_cloud(x, idx)[0]


def _sphere(n, rng):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _nested_spheres():
    rng = np.random.default_rng(0)
    outer, inner = _sphere(512, rng), _sphere(256, rng)
    return np.ascontiguousarray(np.concatenate([outer, 0.4 * inner]), dtype=F), np.concatenate([outer, inner])


@pytest.fixture(scope="module")
def cases():
    """name -> (x, g, idx, analytic outward normal or None): every cloud the tests below share, estimated and listed once."""
    out = {}
    for n, k in ((512, 8), (1024, 10), (2048, 16)):
        for seed in (0, 1, 2):
            x, truth = om.torus(n, seed)
            idx, g = _estimate(x, k)
            out["torus%d_%d" % (n, seed)] = (x, g, idx, truth)
    x, truth = _nested_spheres()
    idx, g = _estimate(x, 8)
    out["nested"] = (x, g, idx, truth)
    clouds = nm.accuracy_clouds(0)
    cube = clouds["cube512"]
    face = np.abs(cube).argmax(axis=1)                              # (a point on an edge: either face's normal; the estimate is near one of them)
    truth = np.zeros((512, 3))
    truth[np.arange(512), face] = np.sign(cube[np.arange(512), face])
    idx, g = _estimate(cube, 12)
    out["cube512"] = (cube, g, idx, truth)
    noisy = clouds["noisy512"]
    idx, g = _estimate(noisy, 16)
    out["noisy512"] = (noisy, g, idx, noisy.astype(np.float64) / np.linalg.norm(noisy.astype(np.float64), axis=1, keepdims=True))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def results(cases):
    return {name: om.orient_cloud(x, g, idx) for name, (x, g, idx, _) in cases.items()}


def _wrong(o, truth):
    return int(((o.astype(np.float64) * truth).sum(axis=1) <= 0).sum())


def test_every_normal_of_the_tori_is_right_where_the_centroid_heuristic_fails_on_a_fifth(cases, results):
    for name, (x, g, idx, truth) in cases.items():
        if not name.startswith("torus"):
            continue
        o, parent, stats = results[name]
        heuristic = nm.sign(g, x, 3, x.astype(np.float64).mean(axis=0))
        bad = _wrong(heuristic, truth)
        print(name, "heuristic wrong", bad, "propagation wrong", _wrong(o, truth), "stats", stats)
        assert bad >= 0.2 * x.shape[0], name                        # the input tells the two methods apart
        assert _wrong(o, truth) == 0, name
        assert stats[0] == 1 and stats[3] == 0, name


def test_nested_spheres_cube_and_noisy_sphere_are_all_right(cases, results):
    for name in ("nested", "cube512", "noisy512"):
        o, parent, stats = results[name]
        print(name, "wrong", _wrong(o, cases[name][3]), "stats", stats)
        assert _wrong(o, cases[name][3]) == 0, name
    assert results["nested"][2][0] == 2 and (results["nested"][1] == -1).sum() == 2
    assert results["cube512"][2][0] == 1 and results["noisy512"][2][0] == 1


def _kruskal(n, eu, ev, ew):
    """An independent minimum spanning forest: edges by ascending weight bits, union-find -> the sorted weights of the edges taken."""
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    taken = []
    for e in np.argsort(ew, kind="stable"):
        a, b = find(int(eu[e])), find(int(ev[e]))
        if a != b:
            root[a] = b
            taken.append(int(ew[e]))
    return sorted(taken), len({find(i) for i in range(n)})


def _tree_weights(g, parent):
    child = np.nonzero(parent >= 0)[0]
    with np.errstate(all="ignore"):
        w = (F(1.0) - np.abs(nm.dot3(g[child], g[parent[child]]))).astype(F)
        w = np.where(w > 0, w, F(0.0)).astype(F)
    return sorted(int(b) for b in np.ascontiguousarray(w).view(np.uint32))


@pytest.mark.parametrize("name", ["torus512_0", "torus1024_1", "nested", "cube512", "noisy512"])
def test_the_tree_is_a_minimum_spanning_forest(cases, results, name):
    x, g, idx, _ = cases[name]
    o, parent, stats = results[name]
    n = x.shape[0]
    eu, ev, ew = om.edges(x, g, idx)
    want, comps = _kruskal(n, eu, ev, ew)
    assert _tree_weights(g, parent) == want                         # bit for bit: the multiset is unique even under ties
    assert stats[0] == comps == (parent == -1).sum()
    assert stats[2] == sum(b > om.HALF_BITS for b in want)
    # every tree edge is an edge of the graph
    have = set(zip(eu.tolist(), ev.tolist())) | set(zip(ev.tolist(), eu.tolist()))
    assert all((c, int(parent[c])) in have for c in np.nonzero(parent >= 0)[0].tolist())


def _check_forest(parent, live, eu, ev):
    n = parent.shape[0]
    assert ((parent == -2) == ~live).all()                          # spans exactly the live points
    assert (parent[live] >= -1).all() and (parent < n).all()
    done = parent == -1
    for i in np.nonzero(live)[0].tolist():                          # acyclic: every walk upwards ends at a root
        path = []
        while not done[i]:
            path.append(i)
            assert len(path) <= n, "cycle"
            i = int(parent[i])
            assert i >= 0 and live[i]
        done[path] = True
    # one root per connected component of the live graph
    root = list(range(n))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for a, b in zip(eu.tolist(), ev.tolist()):
        root[find(a)] = find(b)
    comp_of_roots = [find(i) for i in np.nonzero(parent == -1)[0].tolist()]
    assert len(set(comp_of_roots)) == len(comp_of_roots) == len({find(i) for i in np.nonzero(live)[0].tolist()})


def test_the_forest_is_acyclic_spans_the_live_points_and_has_one_root_per_component(cases, results):
    for name, (x, g, idx, _) in cases.items():
        eu, ev, _ = om.edges(x, g, idx)
        _check_forest(results[name][1], om.live_points(x, g), eu, ev)


def test_the_outputs_differ_from_the_inputs_in_the_sign_bit_only(cases, results):
    for name, (x, g, idx, _) in cases.items():
        o, parent, stats = results[name]
        diff = o.view(np.uint32) ^ g.view(np.uint32)
        assert np.isin(diff, (0, 0x80000000)).all()
        assert (diff[:, 0] == diff[:, 1]).all() and (diff[:, 1] == diff[:, 2]).all()      # a normal is negated whole
        assert stats[1] == (diff[:, 0] != 0).sum()


def test_slot_order_and_repeats_change_no_bit(cases, results):
    rng = np.random.default_rng(5)
    for name in ("torus512_0", "nested", "cube512"):
        x, g, idx, _ = cases[name]
        want = results[name]
        shuffled = rng.permuted(idx, axis=1)
        assert not np.array_equal(shuffled, idx)
        repeated = np.concatenate([shuffled, idx[:, :3], idx[:, -1:]], axis=1)
        for lists in (shuffled, repeated):
            o, parent, stats = om.orient_cloud(x, g, lists)
            assert nm.same_bits(o, want[0]) and np.array_equal(parent, want[1]) and stats == want[2]


def test_poison_behaves_as_the_rules_say(cases):
    x, g, idx, truth = cases["torus512_0"]
    x, g, idx = x.copy(), g.copy(), idx.copy()
    n = x.shape[0]
    g[7, 1] = np.nan                                                # a NaN normal
    x[11, 0] = np.inf                                               # an infinite coordinate
    idx[20, 3], idx[21, 0], idx[22, 5] = n, -1, 2 ** 31 - 1         # out of range: never dereferenced
    idx[30, :] = 30                                                 # self slots alone: point 30 is reached only through others' lists
    o, parent, stats = om.orient_cloud(x, g, idx)
    assert parent[7] == -2 and parent[11] == -2 and stats[3] == 2
    assert nm.same_bits(o[[7, 11]], g[[7, 11]])                     # dead points keep their bits
    live = om.live_points(x, g)
    assert not (np.isin(parent, (7, 11))).any()                     # and are nobody's parent
    eu, ev, _ = om.edges(x, g, idx)
    assert not np.isin(np.concatenate([eu, ev]), (7, 11)).any() and (eu != ev).all() and eu.max() < n and ev.max() < n
    _check_forest(parent, live, eu, ev)
    assert parent[30] >= 0                                          # joined through a neighbour's list: the graph is symmetrised
    assert _wrong(o[live], truth[live]) == 0
    # a cloud of dead points alone, and one whose lists hold nothing usable
    o, parent, stats = om.orient_cloud(np.full((4, 3), np.nan, F), np.ones((4, 3), F), np.zeros((4, 2), np.int32))
    assert (parent == -2).all() and stats == (0, 0, 0, 4) and (o == 1).all()
    gz = np.array([[0, 0, 1], [0, 0, -1], [1, 0, -0.0], [0, 1, 0.0]], F)
    o, parent, stats = om.orient_cloud(np.zeros((4, 3), F), gz, np.full((4, 1), 9, np.int32))
    assert (parent == -1).all() and stats == (4, 1, 0, 0)           # four roots, each by the g.z rule: -0.0 is not below zero
    assert nm.same_bits(o, gz * np.array([[1], [-1], [1], [1]], F))


def test_ties_go_to_the_lower_index_and_roots_to_the_highest_point():
    # a 4 x 4 lattice in the plane z = 0 with normals +-(0, 0, 1): every weight is 0, every point is as high as any other
    ii, jj = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    x = np.stack([ii.ravel(), jj.ravel(), np.zeros(16)], axis=1).astype(F)
    g = np.zeros((16, 3), F)
    g[:, 2] = np.where(np.arange(16) % 3 == 0, -1.0, 1.0)
    idx = nm.knn_indices(x, 5)
    o, parent, stats = om.orient_cloud(x, g, idx)
    assert parent[0] == -1 and stats == (1, 6, 0, 0) and (o[:, 2] == 1).all()
    # Prim with ties to the lower index: points join in index order wherever the lattice allows it, each from its lowest tree neighbour
    assert parent[1] == 0 and parent[4] == 0 and parent[5] == 0 and parent[15] == 7   # (5 is in 0's list; 7 is the lowest point in 15's)
    x[9, 2] = 0.5                                                   # now one point is the highest
    o, parent, stats = om.orient_cloud(x, g, idx)
    assert parent[9] == -1 and (parent == -1).sum() == 1


# ---------------------------------------------------------------------------- wrappers, parser, header
def test_the_wrappers_refuse_host_tensors_and_bad_arguments():
    from pdgn_amd import pointops
    from pdgn_amd._lib import PdgnHipError
    x = torch.zeros(1, 8, 3)
    with pytest.raises(PdgnHipError):
        pointops.orient_normals(x, x)
    with pytest.raises(TypeError):
        pointops.orient_normals(np.zeros((1, 8, 3), F), x)
    with pytest.raises(PdgnHipError):
        pointops.estimate_normals(x, orient="consistent")
    assert "differentiable" in pointops.orient_normals.__doc__ and "consistent" in pointops.estimate_normals.__doc__
    assert pointops.ORIENT_MAX_N == om.MAX_N and pointops.ORIENT_MAX_K == om.MAX_K


def test_the_export_parser_takes_consistent_and_keeps_its_default(tmp_path, capsys):
    from pdgn_amd import export
    args = export.build_parser().parse_args(["out.npy", "-o", "d", "--normals", "16", "--orient", "consistent"])
    assert args.orient == "consistent" and args.normals == 16
    assert export.build_parser().parse_args(["out.npy", "-o", "d"]).orient == "outward"
    with pytest.raises(SystemExit):
        export.build_parser().parse_args(["out.npy", "-o", "d", "--orient", "inward"])
    assert "spanning" in export.main.__doc__
    # clouds beyond the kernel's limit are refused before anything touches a device
    big = tmp_path / "big.npy"
    np.save(big, np.zeros((1, export.CONSISTENT_MAX_POINTS + 1, 3), F))
    with pytest.raises(SystemExit):
        export.main([str(big), "-o", str(tmp_path / "out"), "--normals", "8", "--orient", "consistent"])
    assert "at most 4096 points" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
    with pytest.raises(SystemExit):
        export.main([str(big), "-o", str(tmp_path / "out"), "--normals", "65", "--orient", "consistent"])


def test_the_header_declares_the_entry_points_and_the_limits():
    from pdgn_amd import _lib
    vp, i, ll = _lib.ctypes.c_void_p, _lib.ctypes.c_int, _lib.ctypes.c_longlong
    assert _lib.SIGNATURES["pdgn_orient_normals"] == (i, (i, i, i, vp, vp, vp, vp, vp, vp, vp, vp))
    assert _lib.SIGNATURES["pdgn_orient_workspace_ints"] == (ll, (i, i, i))
    text = open(_lib.HEADER).read()
    assert int(re.search(r"#define PDGN_ORIENT_MAX_N (\d+)", text).group(1)) == om.MAX_N == 4096
    assert om.MAX_K == nm.MAX_K and om.HALF_BITS == 0x3F000000
