"""TSDF integration and marching tetrahedra without a GPU: the host build of
mvster_amd/csrc/tsdf_math.h against the NumPy restatement byte for byte, the properties of the surface the definition promises
(a closed oriented 2-manifold, the interpolation bound, order, welding), the PLY files and the argument checks."""
import inspect

import numpy as np
import pytest

from tests import mesh_cases as M


@pytest.fixture(scope="module")
def host():
    return M.load_tsdf_hostmath()


# ---- the host build equals the restatement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.map_cases()))
def test_integration_host_build_equals_numpy(host, name):
    c = M.map_cases()[name]
    want = M.integrate_numpy(*(c[k] for k in ("depths", "masks", "images", "Ks", "Es", "origin", "voxel", "dims", "trunc")))
    v = M.host_volume(name)
    for got, w, what in zip((v["tsdf"], v["weight"], v["rgb"], v["has_color"]), want, ("tsdf", "weight", "rgb", "has_color")):
        M.assert_bytes(got, w, (name, what))
    assert v["weight"].max() >= 1 and (v["weight"] == 0).any(), "the case must hold counted and uncounted nodes"


def test_bad_depths_are_skipped(host):
    """NaN, +-inf, 0, negative and masked samples, nodes behind a camera and outside every image count for nothing: the volume
    equals the one of the same maps with every such sample masked, and the camera that looks away changes nothing"""
    c = M.map_cases()["bad_depths"]
    v = M.host_volume("bad_depths")
    d = c["depths"]
    clean_mask = c["masks"] & np.isfinite(d) & (d > 0)
    assert (clean_mask != c["masks"]).mean() > 0.1
    clean = M.integrate_host(host, np.where(clean_mask, d, 1.0), clean_mask, c["images"], c["Ks"], c["Es"], c["origin"], c["voxel"],
                             c["dims"], c["trunc"])
    three = M.integrate_host(host, d[:3], c["masks"][:3], c["images"][:3], c["Ks"][:3], c["Es"][:3], c["origin"], c["voxel"],
                             c["dims"], c["trunc"])
    for a, b, e in zip((v["tsdf"], v["weight"], v["rgb"], v["has_color"]), clean, three):
        M.assert_bytes(a, b)
        M.assert_bytes(a, e)
    assert np.isfinite(v["tsdf"]).all() and np.abs(v["tsdf"]).max() <= 1
    only_third = M.integrate_host(host, d[2:3], c["masks"][2:3], c["images"][2:3], c["Ks"][2:3], c["Es"][2:3], c["origin"], c["voxel"],
                                  c["dims"], c["trunc"])
    xs = M.node_coords(c["origin"], c["voxel"], c["dims"])[0]
    eye_x = -(c["Es"][2][:3, :3].T @ c["Es"][2][:3, 3])[0]
    assert (only_third[1][:, :, xs <= eye_x] == 0).all() and only_third[1].max() == 1       # behind the camera: never counted


@pytest.mark.parametrize("name", sorted(M.all_volumes()))
def test_extraction_host_build_equals_numpy(host, name):
    v = M.all_volumes()[name]
    want = M.extract_numpy(v["tsdf"], v["weight"], v["rgb"], v["has_color"], v["origin"], v["voxel"], v["dims"], v["min_weight"])
    got = M.host_mesh(name)
    for g, w, what in zip(got, want, ("vertices", "colors", "triangles", "owners")):
        M.assert_bytes(g, w, (name, what))
    if name != "no_sign_change":
        assert len(got[0]) > 0 and len(got[2]) > 0, name


def test_grid_limits(host):
    assert host.hm_tsdf_grid_ok(2, 2, 2) and host.hm_tsdf_grid_ok(1 << 10, 1 << 10, (1 << 11) - 1)
    assert host.hm_tsdf_grid_ok(2, 2, (1 << 29) - 1) and not host.hm_tsdf_grid_ok(2, 2, 1 << 29)
    for bad in ((1, 2, 2), (2, 1, 2), (2, 2, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 40, 1 << 40, 2), (0, 5, 5), (-3, 5, 5)):
        assert not host.hm_tsdf_grid_ok(*bad), bad


# ---- order, welding, use ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(M.all_volumes()))
def test_order_welding_and_use(name):
    v = M.all_volumes()[name]
    vertices, colors, triangles, owners = M.host_mesh(name)
    nx, ny, nz = v["dims"]
    key = owners[:, 0] * 8 + owners[:, 1]
    assert (np.diff(key) > 0).all(), "vertices by owner node, then d; no (owner, d) twice"
    assert ((owners[:, 1] >= 1) & (owners[:, 1] <= 7)).all()
    if len(triangles):
        assert triangles.min() >= 0 and triangles.max() < len(vertices)
        assert len(np.unique(triangles)) == len(vertices), "every vertex is used by a triangle"
    else:
        assert len(vertices) == 0
    # a triangle's corners lie on edges of one cell, and the cells come in index order
    i, j, k = owners[:, 0] % nx, owners[:, 0] // nx % ny, owners[:, 0] // (nx * ny)
    low = np.stack([i, j, k], 1)[triangles]                                      # [Nt,3 corners,3 axes]
    d = owners[:, 1][triangles]
    high = low + np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], 2)
    cell = low.min(1)                   # every triangle of the case table has a corner on an edge owned by v0, the cell's node
    assert (high.max(1) - cell <= 1).all()
    cell_index = cell[:, 0] + nx * (cell[:, 1] + ny * cell[:, 2])
    assert (np.diff(cell_index) >= 0).all(), "triangles by cell index"
    known = v["weight"].reshape(nz, ny, nx) >= v["min_weight"]
    for ci, cj, ck in np.unique(cell, axis=0):
        assert known[ck:ck + 2, cj:cj + 2, ci:ci + 2].all(), "a triangle in a cell with an unknown corner"


def test_triangles_come_in_cell_order():
    """The sphere: the cell of a triangle (from the restatement's loop) never decreases, and within a cell the tetrahedra"""
    v = M.all_volumes()["sphere_inside"]
    _, _, triangles, owners = M.host_mesh("sphere_inside")
    nx, ny, _ = v["dims"]
    inside = v["tsdf"] < 0
    cells = []
    for k, j, i in zip(*np.nonzero(np.ones_like(inside))):
        if i + 1 >= nx or j + 1 >= ny or k + 1 >= inside.shape[0]:
            continue
        for q, (corners, det) in enumerate(M.TETS):
            ins = [bool(inside[k + ((c >> 2) & 1), j + ((c >> 1) & 1), i + (c & 1)]) for c in corners]
            cells += [(i + nx * (j + ny * k), q)] * len(M.tet_triangles(ins, det))
    assert len(cells) == len(triangles) and cells == sorted(cells)


# ---- the sphere: a closed oriented 2-manifold within the interpolation bound -------------------------------------------------------------

def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def assert_closed_oriented(vertices, triangles, centre):
    e = directed_edges(triangles)
    code = e[:, 0] * (len(vertices) + 1) + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    back = e[:, 1] * (len(vertices) + 1) + e[:, 0]
    assert np.array_equal(np.sort(code), np.sort(back)), "a directed edge without its reverse"
    V, E, F = len(vertices), len(code) // 2, len(triangles)
    assert V - E + F == 2, (V, E, F)
    p = vertices.astype(np.float64)[triangles]
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    volume = (p[:, 0] * np.cross(p[:, 1], p[:, 2])).sum() / 6
    assert volume > 0
    out = (normals * (p.mean(1) - centre)).sum(1)
    assert (out > 0).all(), "a triangle faces the centre (or has no area): %d of %d" % ((out <= 0).sum(), len(out))
    return volume


def rounding_term(v):
    """float32 rounding: a coordinate of magnitude <= m is stored within m 2^-24, so a position within sqrt(3) m 2^-24; a sample
    |tsdf| <= 1 is stored within 2^-24, that is trunc 2^-24 in distance, which moves the interpolant by at most as much; the
    float64 steps in between are 2^-29 times finer and covered by doubling"""
    m = max(abs(o) + v["voxel"] * n for o, n in zip(v["origin"], v["dims"]))
    return 2 * (np.sqrt(3) * m + v["trunc"]) * 2.0 ** -24


def test_sphere_inside_is_closed_oriented_and_within_the_bound():
    v = M.all_volumes()["sphere_inside"]
    vertices, _, triangles, _ = M.host_mesh("sphere_inside")
    volume = assert_closed_oriented(vertices, triangles, v["centre"])
    r = v["radius"]
    assert 0.9 * 4 / 3 * np.pi * r ** 3 < volume < 4 / 3 * np.pi * r ** 3                  # inscribed, and not by much
    L = np.sqrt(3) * v["voxel"]
    bound = L * L / (8 * (r - L)) + rounding_term(v)
    err = np.abs(np.linalg.norm(vertices.astype(np.float64) - v["centre"], axis=1) - r)
    print("sphere: %d vertices, %d triangles, worst | |p - c| - r | = %.3e, bound %.3e" % (len(vertices), len(triangles), err.max(), bound))
    assert err.max() <= bound


def test_integrated_sphere_is_oriented_and_near_the_sphere():
    """Through integrate_tsdf's definition (six views that see the sphere and nothing behind it, projective distances,
    min_weight 1).  A ray that misses the sphere has no depth, so free space beside the silhouettes is never counted and stays
    unknown: the surface is open there.  And the projective distance of a node just behind a grazing ray's hit is slightly
    negative although the node is outside, which leaves small inward-facing flaps outside the sphere at the silhouettes -- the
    known artefact of projective TSDFs, not hidden here.  What holds: the surface is oriented (no directed edge twice); the
    triangles that face the centre are few and all lie outside the sphere; a vertex lies on an edge whose ends a view counted
    within the truncation, so it is within trunc + sqrt(3) voxel of the sphere"""
    v = M.all_volumes()["sphere_views"]
    vertices, colors, triangles, _ = M.host_mesh("sphere_views")
    e = directed_edges(triangles)
    code = e[:, 0] * (len(vertices) + 1) + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    p = vertices.astype(np.float64)[triangles]
    out = (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * (p.mean(1) - v["centre"])).sum(1)
    inward = out <= 0
    print("integrated sphere: %d triangles, %d face the centre" % (len(triangles), inward.sum()))
    assert len(triangles) > 1500 and inward.mean() < 0.05
    assert (np.linalg.norm(p[inward].mean(1) - v["centre"], axis=1) > v["radius"]).all()
    err = np.abs(np.linalg.norm(vertices.astype(np.float64) - v["centre"], axis=1) - v["radius"])
    print("integrated sphere: worst distance to the sphere %.3e (voxel %.3e)" % (err.max(), v["voxel"]))
    assert err.max() <= v["trunc"] + np.sqrt(3) * v["voxel"]
    assert colors.std() > 10                                                     # colours come from the seeded images


def test_cut_sphere_and_holes_are_open():
    for name in ("sphere_cut", "holes"):
        vertices, _, triangles, _ = M.host_mesh(name)
        e = directed_edges(triangles)
        code = e[:, 0] * (len(vertices) + 1) + e[:, 1]
        back = e[:, 1] * (len(vertices) + 1) + e[:, 0]
        assert len(np.unique(code)) == len(code), name                           # still oriented: no directed edge twice
        border = ~np.isin(code, back)
        assert border.any(), name                                                # and open
    full = M.host_mesh("sphere_inside")[2]
    assert 0 < len(M.host_mesh("holes")[2]) < len(full)


def test_exact_zero_counts_as_outside_and_keeps_degenerate_triangles():
    v = M.all_volumes()["exact_zero_plane"]
    vertices, _, triangles, owners = M.host_mesh("exact_zero_plane")
    nx, ny, _ = v["dims"]
    assert (owners[:, 0] // (nx * ny) == 2).all(), "only edges from layer 2 (inside) to layer 3 (exactly 0: outside) cross"
    zs = M.node_coords(v["origin"], v["voxel"], v["dims"])[2]
    assert (vertices[:, 2] == np.float32(zs[3])).all()                          # t = 1: every vertex is a node of layer 3
    p = vertices.astype(np.float64)[triangles]
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area == 0).any() and (area > 0).any()
    assert len(np.unique(vertices, axis=0)) < len(vertices)                     # coinciding vertices stay separate vertices


def test_no_sign_change_gives_nothing():
    vertices, colors, triangles, _ = M.host_mesh("no_sign_change")
    assert vertices.shape == (0, 3) and colors.shape == (0, 3) and triangles.shape == (0, 3)


@pytest.mark.parametrize("name", ["plane", "plane_65"])
def test_plane_is_flat_and_takes_the_image_colour(name):
    v = M.all_volumes()[name]
    vertices, colors, triangles, _ = M.host_mesh(name)
    assert len(triangles) > 0
    err = np.abs(vertices[:, 2].astype(np.float64) - M.PLANE_DEPTH)
    print("%s: worst |z - d0| = %.3e, rounding term %.3e" % (name, err.max(), rounding_term(v)))
    assert err.max() <= rounding_term(v)
    assert (colors == np.asarray(M.PLANE_COLOUR, np.uint8)).all()
    p = vertices.astype(np.float64)[triangles]
    normals = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert (normals[:, 2] < 0).all()                                             # toward the camera at the origin: free space


# ---- files ------------------------------------------------------------------------------------------------------------------------------

def test_mesh_ply_round_trip(tmp_path):
    from mvster_amd import mesh
    vertices, colors, triangles, _ = M.host_mesh("sphere_cut")
    f = str(tmp_path / "m.ply")
    mesh.write_mesh_ply(f, vertices, triangles, colors)
    head = open(f, "rb").read(400).split(b"end_header\n")[0].decode("ascii")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(vertices))
    assert "element face %d\nproperty list uchar int vertex_indices\n" % len(triangles) in head
    v, t, c = mesh.read_mesh_ply(f)
    M.assert_bytes(v, vertices)
    M.assert_bytes(t, triangles)
    M.assert_bytes(c, colors)
    mesh.write_mesh_ply(f, vertices, triangles)
    v, t, c = mesh.read_mesh_ply(f)
    M.assert_bytes(v, vertices)
    M.assert_bytes(t, triangles)
    assert c is None
    mesh.write_mesh_ply(f, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint8))
    v, t, c = mesh.read_mesh_ply(f)
    assert v.shape == (0, 3) and t.shape == (0, 3) and c.shape == (0, 3)
    with pytest.raises(RuntimeError, match="outside"):
        mesh.write_mesh_ply(f, vertices[:5], triangles)


# ---- argument checks: on the host, before any device call ---------------------------------------------------------------------------

def _maps():
    c = M.map_cases()["plane"]
    return [c[k] for k in ("depths", "masks", "images", "Ks", "Es")], c


def test_integrate_tsdf_argument_checks():
    from mvster_amd import mesh
    (d, m, im, Ks, Es), c = _maps()
    good = dict(origin=c["origin"], voxel_size=c["voxel"], dims=c["dims"], trunc=c["trunc"])
    for change, match in ((dict(dims=(1, 4, 4)), "at least 2 nodes"), (dict(dims=(2048, 1024, 1024)), "2\\^31 - 1 nodes"),
                          (dict(dims=(4, 4)), "three integers"), (dict(dims=(4.5, 4, 4)), "three integers"),
                          (dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"),
                          (dict(trunc=-1.0), "trunc"), (dict(origin=(0, 0)), "origin"), (dict(origin=(0, float("inf"), 0)), "origin")):
        with pytest.raises(RuntimeError, match=match):
            mesh.integrate_tsdf(d, m, im, Ks, Es, **dict(good, **change))
    with pytest.raises(RuntimeError, match="masks"):
        mesh.integrate_tsdf(d, m[:, :-1], im, Ks, Es, **good)
    with pytest.raises(RuntimeError, match="images"):
        mesh.integrate_tsdf(d, m, im[..., :2], Ks, Es, **good)
    with pytest.raises(RuntimeError, match="uint8"):
        mesh.integrate_tsdf(d, m, im.astype(np.float32), Ks, Es, **good)
    with pytest.raises(RuntimeError, match="intrinsics"):
        mesh.integrate_tsdf(d, m, im, Ks + Ks, Es, **good)
    with pytest.raises(RuntimeError, match="third row"):
        mesh.integrate_tsdf(d, m, im, [np.asarray(Ks[0]) * 2], Es, **good)
    with pytest.raises(RuntimeError, match=r"\[4,4\]"):
        mesh.integrate_tsdf(d, m, im, Ks, [np.eye(3)], **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # everything is in order: only the GPU is missing
        mesh.integrate_tsdf(d, m, im, Ks, Es, **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.integrate_tsdf(d, m, im, Ks, Es, device="cpu", **good)


def test_mesh_scene_and_extract_mesh_argument_checks():
    import torch
    from mvster_amd import mesh
    (d, m, im, Ks, Es), c = _maps()
    with pytest.raises(RuntimeError, match="trunc must be >= 2"):
        mesh.mesh_scene(d, m, im, Ks, Es, 0.05, trunc=0.09, bounds=((0, 0, 2), (1, 1, 3)))
    with pytest.raises(RuntimeError, match="min_weight"):
        mesh.mesh_scene(d, m, im, Ks, Es, 0.05, min_weight=0, bounds=((0, 0, 2), (1, 1, 3)))
    with pytest.raises(RuntimeError, match="lo <= hi"):
        mesh.mesh_scene(d, m, im, Ks, Es, 0.05, bounds=((0, 0, 3), (1, 1, 2)))
    with pytest.raises(RuntimeError, match=r"bounds must be \(lo, hi\)"):
        mesh.mesh_scene(d, m, im, Ks, Es, 0.05, bounds=5)
    with pytest.raises(RuntimeError) as e:
        mesh.mesh_scene(d, m, im, Ks, Es, 0.001, bounds=((0, 0, 2), (1, 1, 3)), memory_budget=1 << 20)
    msg = str(e.value)
    assert "nodes" in msg and "bytes" in msg and "voxel_size of" in msg
    fit = float(msg.split("voxel_size of ")[1].split()[0])
    origin, dims = mesh.grid_for_bounds("t", (0, 0, 2), (1, 1, 3), fit, 4 * 0.001, 1 << 20)     # the size it names does fit
    assert dims[0] * dims[1] * dims[2] * mesh.NODE_BYTES <= 1 << 20
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.mesh_scene(d, m, im, Ks, Es, 0.05, bounds=((0, 0, 2), (1, 1, 3)))
    origin, dims = mesh.grid_for_bounds("t", (0.0, 0.0, 2.0), (1.0, 0.5, 3.0), 0.05, 0.2)
    assert origin == (-0.2, -0.2, 1.8) and dims == (29, 19, 29)
    for lo, hi, n in zip(origin, (1.0, 0.5, 3.0), dims):
        assert lo + 0.05 * (n - 1) >= hi + 0.2 - 1e-12
    with pytest.raises(RuntimeError, match="TSDFVolume"):
        mesh.extract_mesh(dict())
    z = torch.zeros(3, 3, 3)
    vol = mesh.TSDFVolume(z, z.int(), torch.zeros(3, 3, 3, 3, dtype=torch.uint8), z.to(torch.uint8), (0, 0, 0), 0.1, (3, 3, 3), 0.4)
    with pytest.raises(RuntimeError, match="min_weight"):
        mesh.extract_mesh(vol, min_weight=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.extract_mesh(vol)
    with pytest.raises(RuntimeError, match="volume.weight"):
        mesh.extract_mesh(mesh.TSDFVolume(z, z, vol.rgb, vol.has_color, (0, 0, 0), 0.1, (3, 3, 3), 0.4))


def test_mesh_spec_checks_and_defaults():
    from mvster_amd import fusion, mesh, scan
    assert fusion.TSDFMesh is mesh.TSDFMesh and mesh.TSDFMesh(0.01) == (0.01, None, 2)
    assert mesh.check_mesh_spec("x", None) is None
    assert mesh.check_mesh_spec("x", mesh.TSDFMesh(0.5)) == (0.5, 2.0, 2)
    for bad, match in ((0.01, "TSDFMesh"), (mesh.TSDFMesh(-1.0), "voxel_size"), (mesh.TSDFMesh(0.1, 0.15), "trunc must be >= 2"),
                       (mesh.TSDFMesh(0.1, None, 0), "min_weight"), (mesh.TSDFMesh(0.1, None, 1.5), "min_weight")):
        for call in (lambda b: fusion.fuse_scene(None, None, None, None, None, None, 0.9, 3, mesh=b),
                     lambda b: fusion.filter_depth("a", "b", "c", "d.ply", mesh=b, meshfilename="m.ply"),
                     lambda b: scan.reconstruct_scan(None, None, None, None, None, None, mesh=b)):
            with pytest.raises(RuntimeError, match=match):
                call(bad)
    with pytest.raises(RuntimeError, match="go together"):
        fusion.filter_depth("a", "b", "c", "d.ply", meshfilename="m.ply")
    with pytest.raises(RuntimeError, match="meshfilename needs mesh"):
        scan.reconstruct_scan(None, None, None, None, None, None, meshfilename="m.ply")
    # mesh=None is the default everywhere: the keyword paths are untouched
    for fn, names in ((fusion.fuse_scene, ("mesh",)), (fusion.filter_depth, ("mesh", "meshfilename")),
                      (scan.reconstruct_scan, ("mesh", "meshfilename"))):
        sig = inspect.signature(fn)
        for n in names:
            assert sig.parameters[n].default is None, (fn.__name__, n)


def test_abi_entry_points_validate_before_any_hip_call():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    assert lib.mvster_mesh_blocks(8) == 1 and lib.mvster_mesh_blocks(257) == 2 and lib.mvster_mesh_blocks((1 << 31) - 1) == 1 << 23
    assert lib.mvster_mesh_blocks(7) == _lib.ERR_SHAPE and lib.mvster_mesh_blocks(1 << 31) == _lib.ERR_SHAPE
    p = 1 << 32                                                                  # a stand-in address nothing may dereference
    assert lib.mvster_tsdf_integrate(None, p, p, p, 1, 4, 4, 0, 0, 0, 1.0, 2, 2, 2, 1.0, p, p, p, p, None) == _lib.ERR_NULL
    for V, H, W, voxel, dims, trunc in ((0, 4, 4, 1.0, (2, 2, 2), 1.0), (1, 0, 4, 1.0, (2, 2, 2), 1.0), (1, 4, 4, 0.0, (2, 2, 2), 1.0),
                                        (1, 4, 4, 1.0, (1, 2, 2), 1.0), (1, 4, 4, 1.0, (2048, 1024, 1024), 1.0),
                                        (1, 4, 4, 1.0, (2, 2, 2), 0.0), (1, 4, 4, float("nan"), (2, 2, 2), 1.0)):
        assert lib.mvster_tsdf_integrate(p, p, p, p, V, H, W, 0, 0, 0, voxel, *dims, trunc, p, p, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_count(p, None, 2, 2, 2, 1, p, p, p, p, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_mesh_count(p, p, 2, 1, 2, 1, p, p, p, p, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_emit_vertices(p, p, p, 0, 0, 0, 1.0, 2, 2, 2, p, p, None, 1, p, p, None) == _lib.ERR_NULL
    assert lib.mvster_mesh_emit_vertices(p, p, p, 0, 0, 0, 1.0, 2, 2, 2, p, p, p, 1 << 31, p, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_emit_vertices(p, p, p, 0, 0, 0, 1.0, 2, 2, 2, p, p, p, 0, None, None, None) == 0     # nothing to do
    assert lib.mvster_mesh_emit_vertices(p, p, p, 0, 0, 0, 1.0, 2, 2, 2, p, p, p, 1, None, p, None) == _lib.ERR_NULL
    assert lib.mvster_mesh_emit_triangles(p, p, 2, 2, 2, 1, p, p, p, None, 1, 1, p, None) == _lib.ERR_NULL
    assert lib.mvster_mesh_emit_triangles(p, p, 2, 2, 2, 1, p, p, p, p, 1 << 31, 1, p, None) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_emit_triangles(p, p, 2, 2, 2, 1, p, p, p, p, 0, 0, None, None) == 0
