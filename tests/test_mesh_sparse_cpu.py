"""Brick-sparse TSDF volumes on the CPU: the host build of mvster_amd/csrc/tsdf_sparse_math.h against the
host build of tsdf_math.h, the dense path the existing tests pin -- for any set of bricks, for the set ``allocate`` gives, and in
a virtual grid the dense path refuses -- and the argument checks of the new functions and entry points."""
import numpy as np
import pytest

from tests import mesh_cases as M
from tests import mesh_sparse_cases as S


@pytest.fixture(scope="module")
def hosts():
    return S.load_sparse_hostmath(), M.load_tsdf_hostmath()


def dense_mesh(hd, v, weight=None, min_weight=None):
    ve, co, tr, owners = M.extract_host(hd, v["tsdf"], v["weight"] if weight is None else weight, v["rgb"], v["has_color"], v["origin"],
                                        v["voxel"], v["dims"], v["min_weight"] if min_weight is None else min_weight)
    return ve, co, tr, S.dense_keys(owners)


# ---- any S -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", S.ANY_S_VOLUMES)
def test_any_brick_set_is_the_dense_mesh_of_the_masked_volume(hosts, name):
    hs, hd = hosts
    v = M.volume_cases()[name]
    for seed, (which, bricks) in enumerate(sorted(S.brick_sets(v["dims"], 17).items())):
        got = S.extract_sparse_host(hs, S.cut_into_bricks(v, bricks), bricks, v["origin"], v["voxel"], v["dims"], v["min_weight"])
        masked = S.masked_outside(v, bricks)
        want = dense_mesh(hd, masked)
        print("%s / %s: %d bricks, %d vertices, %d triangles" % (name, which, len(bricks), len(got[0]), len(got[2])))
        S.assert_canonically_equal(got, want, (name, which))
        assert got[2].size == 0 or (got[2].min() >= 0 and got[2].max() < len(got[0]))
        if which == "full":
            S.assert_canonically_equal(got, dense_mesh(hd, v), (name, "full against the unmasked volume"))
            assert len(got[2]) == len(M.host_mesh(name)[2])
        if which == "empty":
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3].shape == (0,)
    # the order of the definition: keys ascend inside a brick by local node then d; bricks ascend
    bricks = S.brick_sets(v["dims"], 17)["full"]
    keys = S.extract_sparse_host(hs, S.cut_into_bricks(v, bricks), bricks, v["origin"], v["voxel"], v["dims"], v["min_weight"])[3]
    nx, ny, nz = v["dims"]
    node, d = keys // 8, keys % 8
    i, j, k = node % nx, (node // nx) % ny, node // (nx * ny)
    nb = S.brick_dims(v["dims"])
    brick = i // 8 + nb[0] * (j // 8 + nb[1] * (k // 8))
    local = i % 8 + 8 * (j % 8 + 8 * (k % 8))
    order = (brick * 512 + local) * 8 + d
    assert (np.diff(order) > 0).all()


# ---- allocation --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,s", S.REFINED)
def test_allocation_covers_what_is_needed(name, s):
    c = S.refined(name, s)
    allocated, needed = S.host_sparse(name, s)["bricks"], S.needed_bricks(c)
    nb = S.brick_dims(c["dims"])
    print("%s x%d: %d bricks in the grid, %d needed, %d allocated" % (name, s, nb[0] * nb[1] * nb[2], len(needed), len(allocated)))
    assert (np.diff(allocated) > 0).all() and allocated.min() >= 0 and allocated.max() < nb[0] * nb[1] * nb[2]
    assert np.isin(needed, allocated).all(), np.setdiff1d(needed, allocated)
    if (name, s) in S.TIGHT:
        assert len(allocated) <= 2 * len(needed)


def test_allocation_leaves_most_of_a_wide_grid_empty(hosts):
    """The plane in a 129^3 grid (17^3 = 4913 bricks): its slabs are 8 nodes deep and about 54 x 41 nodes wide, so with the
    widening at most 4 x 9 x 8 = 288 bricks can be touched -- 6% of the grid; fewer than a quarter is asked"""
    c = S.plane_129()
    allocated = S.allocate_host(hosts[0], *(c[k] for k in ("depths", "masks", "Ks", "Es", "origin", "voxel", "dims", "trunc")))
    needed = S.needed_bricks(c)
    print("plane in 129^3: %d bricks in the grid, %d needed, %d allocated" % (17 ** 3, len(needed), len(allocated)))
    assert np.isin(needed, allocated).all() and len(needed) > 0
    assert len(allocated) < 17 ** 3 / 4


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,s", S.REFINED)
def test_end_to_end_equals_dense(hosts, name, s):
    hs, hd = hosts
    c = S.refined(name, s)
    sparse = S.host_sparse(name, s)
    bricks, vol = sparse["bricks"], sparse["volume"]
    dense = dict(zip(("tsdf", "weight", "rgb", "has_color"), S.host_dense(name, s)))
    want_bricks = S.cut_into_bricks(dict(c, **dense), bricks)
    for key in ("tsdf", "weight", "rgb", "has_color"):                          # every allocated node, and the empty words beyond the grid
        M.assert_bytes(vol[key], want_bricks[key], (name, s, key))
    for mw in (1, 2):
        got = sparse["mesh"] if mw == 1 else S.extract_sparse_host(hs, vol, bricks, c["origin"], c["voxel"], c["dims"], mw)
        ve, co, tr, owners = M.extract_host(hd, dense["tsdf"], dense["weight"], dense["rgb"], dense["has_color"], c["origin"], c["voxel"],
                                            c["dims"], mw)
        print("%s x%d, min_weight %d: %d vertices, %d triangles" % (name, s, mw, len(ve), len(tr)))
        S.assert_canonically_equal(got, (ve, co, tr, S.dense_keys(owners)), (name, s, mw))
        assert len(tr) > 0 or mw == 2                                           # (one view: no node is seen twice)


def test_beyond_the_dense_limit(hosts):
    hs, hd = hosts
    c = S.plane_huge()
    assert hd.hm_tsdf_grid_ok(*c["dims"]) == 0 and hs.hm_sparse_grid_bricks(*c["dims"]) == 256 * 256 * 128
    r = S.host_huge()
    vertices, colors, triangles, keys = r["mesh"]
    print("2048 x 2048 x 1024: %d bricks allocated, %d vertices, %d triangles" % (len(r["bricks"]), len(vertices), len(triangles)))
    assert len(triangles) > 0 and len(r["bricks"]) < 1000
    err = np.abs(vertices[:, 2].astype(np.float64) - M.PLANE_DEPTH)
    print("worst |z - d0| = %.3e, rounding term %.3e" % (err.max(), S.rounding_term(c)))
    assert err.max() <= S.rounding_term(c)
    assert (colors == np.asarray(M.PLANE_COLOUR, np.uint8)).all()
    p = vertices.astype(np.float64)[triangles]
    assert (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])[:, 2] < 0).all()      # toward the camera: free space
    assert keys.min() > 1 << 34 and len(np.unique(keys)) == len(keys)
    # the same surface as in the small grid: as many triangles as the plane case refined by 1 gives around the same nodes
    small = S.host_sparse("plane", 1)["mesh"]
    assert len(small[2]) > 0


# ---- argument checks -----------------------------------------------------------------------------------------------------------------------

def _maps():
    c = M.map_cases()["plane"]
    return [c[k] for k in ("depths", "masks", "images", "Ks", "Es", "origin", "voxel", "dims", "trunc")]


def test_sparse_function_argument_checks():
    from mvster_amd import mesh
    d, m, im, Ks, Es, o, vx, dims, t = _maps()
    for bad_dims, match in (((1, 8, 8), "2 .. 2\\^20"), (((1 << 20) + 1, 8, 8), "2 .. 2\\^20"), ((1 << 20, 1 << 20, 8), "2\\^27 bricks"),
                            ((8, 8), "three integers"), ((8.5, 8, 8), "three integers")):
        with pytest.raises(RuntimeError, match=match):
            mesh.integrate_tsdf_sparse(d, m, im, Ks, Es, o, vx, bad_dims, t, device="cuda:0")
        with pytest.raises(RuntimeError, match=match):
            mesh.allocate_bricks(d, m, Ks, Es, o, vx, bad_dims, t, device="cuda:0")
    nb = mesh.brick_dims(dims)
    n = nb[0] * nb[1] * nb[2]
    for bad, match in (([3, 1], "ascending"), ([1, 1], "duplicates"), ([0, n], "must lie in"), ([-1, 0], "must lie in"),
                       ([0.5], "integer brick numbers"), ([[0, 1]], "1-d")):
        with pytest.raises(RuntimeError, match=match):
            mesh.integrate_tsdf_sparse(d, m, im, Ks, Es, o, vx, dims, t, bricks=np.asarray(bad), device="cuda:0")
    with pytest.raises(RuntimeError, match="MI355X only"):
        mesh.integrate_tsdf_sparse(d, m, im, Ks, Es, o, vx, dims, t)
    with pytest.raises(RuntimeError, match="MI355X only"):
        mesh.allocate_bricks(d, m, Ks, Es, o, vx, dims, t, device="cpu")
    with pytest.raises(RuntimeError, match="voxel_size"):
        mesh.allocate_bricks(d, m, Ks, Es, o, 0.0, dims, t, device="cuda:0")
    with pytest.raises(RuntimeError, match="masks must have the shape"):
        mesh.allocate_bricks(d, m[:, :-1], Ks, Es, o, vx, dims, t, device="cuda:0")
    skewed = np.array(Ks[0], np.float64)
    skewed[1, 0] = 0.01
    with pytest.raises(RuntimeError, match="upper triangular"):
        mesh.allocate_bricks(d, m, [skewed], Es, o, vx, dims, t, device="cuda:0")
    with pytest.raises(RuntimeError, match="upper triangular"):
        mesh.integrate_tsdf_sparse(d, m, im, [skewed], Es, o, vx, dims, t, device="cuda:0")
    sheared = np.eye(4)
    sheared[0, 1] = 1e-2                                                         # moves a node 2.5 away by 0.075 > 0.05 / 4
    with pytest.raises(RuntimeError, match="orthonormal only to"):
        mesh.allocate_bricks(d, m, Ks, [sheared], o, vx, dims, t, device="cuda:0")
    for fn in (mesh.extract_mesh_sparse, mesh.densify):
        with pytest.raises(RuntimeError, match="SparseTSDFVolume"):
            fn(object())
    with pytest.raises(RuntimeError, match="min_weight"):
        mesh.extract_mesh_sparse(object(), 0)
    with pytest.raises(RuntimeError, match="keys must be True or False"):
        mesh.extract_mesh_sparse(object(), 1, keys=1)
    assert mesh.sparse_bytes(10, 1000) == 10 * mesh.BRICK_BYTES + 1000 * mesh.DIRECTORY_BYTES


def test_mesh_scene_sparse_and_spec_argument_checks():
    from mvster_amd import fusion, mesh
    d, m, im, Ks, Es, o, vx, dims, t = _maps()
    with pytest.raises(RuntimeError, match="sparse must be True or False"):
        mesh.mesh_scene(d, m, im, Ks, Es, vx, sparse=1, device="cuda:0")
    # the dense cap does not apply to a sparse grid; its own limits do, before any device call
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="2\\^31 - 1 nodes"):
        mesh.grid_for_bounds("t", lo, hi, 5e-4, 2e-3, memory_budget=1 << 50)       # 2009^3 nodes
    origin, gd = mesh.grid_for_bounds("t", lo, hi, 5e-4, 2e-3, memory_budget=1 << 50, sparse=True)
    assert all(2005 <= n <= 2012 for n in gd) and origin == (-2e-3, -2e-3, -2e-3)
    with pytest.raises(RuntimeError, match="sparse grid would hold"):
        mesh.grid_for_bounds("t", lo, hi, 1e-7, 4e-7, sparse=True)              # above 2^20 nodes per axis
    with pytest.raises(RuntimeError, match="sparse grid would hold"):
        mesh.grid_for_bounds("t", lo, hi, 1e-4, 4e-4, sparse=True)              # 1252^3 bricks: above 2^27
    with pytest.raises(RuntimeError, match="sparse grid would hold"):
        mesh.grid_for_bounds("t", lo, hi, 5e-4, 2e-3, memory_budget=1 << 20, sparse=True)      # the directory alone (79 MB)
    with pytest.raises(RuntimeError, match="sparse grid would hold"):
        mesh.mesh_scene(d, m, im, Ks, Es, 5e-4, bounds=(lo, hi), memory_budget=1 << 20, sparse=True, device="cuda:0")
    # the spec: a fourth field beside the tuple
    spec = mesh.TSDFMesh(0.5, sparse=True)
    assert spec.sparse is True and mesh.TSDFMesh(0.5).sparse is False and spec == (0.5, None, 2) and fusion.TSDFMesh is mesh.TSDFMesh
    assert mesh.TSDFMesh(0.5, None, 1, True).sparse is True and spec._replace(min_weight=1).sparse is True
    assert "sparse=True" in repr(spec)
    assert mesh.check_mesh_spec("x", spec) == (0.5, 2.0, 2)
    with pytest.raises(RuntimeError, match="mesh.sparse must be True or False"):
        mesh.check_mesh_spec("x", mesh.TSDFMesh(0.5, sparse="yes"))


def test_sparse_entry_points_validate_before_any_hip_call():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    assert lib.mvster_tsdf_sparse_bricks(2048, 2048, 1024) == 1 << 23 and lib.mvster_tsdf_sparse_bricks(9, 8, 2) == 2
    assert lib.mvster_tsdf_sparse_bricks(1 << 20, 1 << 10, 2) == 1 << 24
    for dims in ((1, 8, 8), ((1 << 20) + 1, 8, 8), (1 << 20, 1 << 20, 2)):
        assert lib.mvster_tsdf_sparse_bricks(*dims) == _lib.ERR_SHAPE
    p = 1 << 32                                                                  # a stand-in address nothing may dereference
    g = (0, 0, 0, 1.0, 16, 16, 16)
    assert lib.mvster_tsdf_sparse_mark(p, None, p, 1, 4, 4, *g, 1.0, p, None) == _lib.ERR_NULL
    for V, H, W, voxel, dims, trunc in ((0, 4, 4, 1.0, (16, 16, 16), 1.0), (1, 0, 4, 1.0, (16, 16, 16), 1.0), (1, 4, 4, 0.0, (16, 16, 16), 1.0),
                                        (1, 4, 4, 1.0, (1, 16, 16), 1.0), (1, 4, 4, 1.0, (1 << 20, 1 << 20, 16), 1.0),
                                        (1, 4, 4, 1.0, (16, 16, 16), 0.0), (1, 4, 4, float("nan"), (16, 16, 16), 1.0),
                                        (1, 4, 4, 1.0, (16, 16, 16), float("inf"))):
        assert lib.mvster_tsdf_sparse_mark(p, p, p, V, H, W, 0, 0, 0, voxel, *dims, trunc, p, None) == _lib.ERR_SHAPE
        assert lib.mvster_tsdf_sparse_integrate(p, p, p, p, V, H, W, 0, 0, 0, voxel, *dims, trunc, p, 1, p, p, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_tsdf_sparse_compact_count(None, 8, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_tsdf_sparse_compact_count(p, 0, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_tsdf_sparse_compact_count(p, (1 << 27) + 1, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_tsdf_sparse_compact_emit(p, 8, None, 1, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_tsdf_sparse_compact_emit(p, 8, p, 9, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_tsdf_sparse_compact_emit(p, 8, p, 1, p, None, None) == _lib.ERR_NULL
    assert lib.mvster_tsdf_sparse_integrate(p, p, None, p, 1, 4, 4, *g, 1.0, p, 1, p, p, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_tsdf_sparse_integrate(p, p, p, p, 1, 4, 4, *g, 1.0, p, 9, p, p, p, p, None) == _lib.ERR_SHAPE       # 8 bricks in the grid
    assert lib.mvster_tsdf_sparse_integrate(p, p, p, p, 1, 4, 4, *g, 1.0, p, -1, p, p, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_tsdf_sparse_integrate(p, p, p, p, 1, 4, 4, *g, 1.0, None, 0, None, None, None, None, None) == 0     # nothing to do
    assert lib.mvster_tsdf_sparse_integrate(p, p, p, p, 1, 4, 4, *g, 1.0, p, 1, p, None, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_mesh_sparse_count(p, p, None, p, 1, 16, 16, 16, 1, p, p, p, p, p, p, None) == _lib.ERR_NULL
    for Nb, dims, mw in ((0, (16, 16, 16), 1), (9, (16, 16, 16), 1), (1, (16, 1, 16), 1), (1, (16, 16, 16), 0)):
        assert lib.mvster_mesh_sparse_count(p, p, p, p, Nb, *dims, mw, p, p, p, p, p, p, None) == _lib.ERR_SHAPE
    ev = lambda Nv, vertices=p, voffsets=p, Nb=1: lib.mvster_mesh_sparse_emit_vertices(p, p, p, p, p, p, Nb, 0, 0, 0, 1.0, 16, 16, 16, p, p,
                                                                                         voffsets, Nv, vertices, p, None, None)
    assert ev(1, voffsets=None) == _lib.ERR_NULL and ev(1 << 31) == _lib.ERR_SHAPE and ev(-1) == _lib.ERR_SHAPE and ev(1, Nb=9) == _lib.ERR_SHAPE
    assert ev(0, vertices=None) == 0 and ev(1, vertices=None) == _lib.ERR_NULL
    et = lambda Nv, Nt, triangles=p, toffsets=p, mw=1: lib.mvster_mesh_sparse_emit_triangles(p, p, p, p, 1, 16, 16, 16, mw, p, p, p, toffsets,
                                                                                               Nv, Nt, triangles, None)
    assert et(1, 1, toffsets=None) == _lib.ERR_NULL and et(1 << 31, 1) == _lib.ERR_SHAPE and et(1, -1) == _lib.ERR_SHAPE
    assert et(1, 1, mw=0) == _lib.ERR_SHAPE and et(0, 0, triangles=None) == 0 and et(1, 1, triangles=None) == _lib.ERR_NULL
