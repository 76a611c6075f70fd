"""Mesh cleaning without a GPU: the host build of mvster_amd/csrc/mesh_math.h against the NumPy restatement
byte for byte, the facts the cases were chosen for, the PLY files with normals, and every argument check."""
import inspect

import numpy as np
import pytest

from tests import mesh_cases as M
from tests import mesh_clean_cases as K


@pytest.fixture(scope="module")
def host():
    return K.load_mesh_clean_hostmath()


@pytest.mark.parametrize("name", sorted(K.all_meshes()))
def test_host_build_equals_numpy(host, name):
    v, c, t = K.all_meshes()[name]
    for s, setting in enumerate(K.SETTINGS):
        K.assert_clean_equal(K.host_clean(name, s), K.clean_numpy(v, c, t, normals=True, **setting), (name, setting))
    got, want = K.components_host(host, None, t, len(v)), K.components_numpy(None, t, len(v))
    for k in K.COMPONENT_KEYS:
        M.assert_bytes(got[k], want[k], (name, k))
    n, valid = K.normals_host(host, v, t) if np.isfinite(v).all() else (None, None)
    if n is not None:
        wn, wv = K.normals_numpy(v, t)
        M.assert_bytes(n, wn, (name, "normals"))
        M.assert_bytes(valid, wv, (name, "valid"))


def test_rows_are_put_in_order_at_any_length(host):
    rng = np.random.RandomState(3)
    for L in (0, 1, 2, 15, 16, 17, 18, 100, 3000):
        for hi in (3, 1 << 30):
            row = rng.randint(0, hi, size=L).astype(np.int32)
            want = np.sort(row)
            host.hm_mesh_sort_row(row.ctypes.data, L)
            assert np.array_equal(row, want), (L, hi)


def _clean(name, **kw):
    v, c, t = K.extracted(name)
    return K.clean_host(K.load_mesh_clean_hostmath(), v, c, t, **kw)


def test_exact_zero_plane_welds_to_one_sheet():
    v, c, t = K.extracted("exact_zero_plane")
    assert (len(v), len(t)) == (99, 160)
    r = _clean("exact_zero_plane")
    assert (len(r["vertices"]), len(r["triangles"])) == (30, 40)
    assert r["stats"] == dict(welded=69, degenerate=120, components=1, components_kept=1, triangles_removed=120, vertices_removed=69)
    assert len(np.unique(v, axis=0)) == 30
    # a kept vertex keeps its own bytes, and the indices point at them
    M.assert_bytes(r["vertices"], v[r["vertex_index"]])
    M.assert_bytes(r["colors"], c[r["vertex_index"]])
    M.assert_bytes(r["vertices"][r["triangles"]], v[t[r["triangle_index"]]])
    assert (np.diff(r["vertex_index"]) > 0).all() and (np.diff(r["triangle_index"]) > 0).all()


def test_exact_zero_random():
    v, c, t = K.extracted("exact_zero_random")
    assert (len(v), len(t)) == (95, 82)
    r = _clean("exact_zero_random")
    assert (len(r["vertices"]), len(r["triangles"])) == (79, 58) and r["stats"]["components"] == 11


def test_node_sphere_stays_closed():
    v, c, t = K.extracted("node_sphere")
    assert int((K.node_sphere_volume()["tsdf"] == 0).sum()) == 30
    assert (len(v), len(t)) == (1298, 2592) and K.closed_and_oriented(t)
    r = _clean("node_sphere")
    assert (len(r["vertices"]), len(r["triangles"])) == (1184, 2364)
    assert K.closed_and_oriented(r["triangles"]) and K.euler(1184, r["triangles"]) == 2
    assert r["stats"]["components"] == 1


def test_two_spheres_are_two_components():
    v, c, t = K.extracted("two_spheres")
    assert (len(v), len(t)) == (1216, 2424)
    r = _clean("two_spheres")
    assert (len(r["vertices"]), len(r["triangles"])) == (1198, 2388)
    comp = K.components_host(K.load_mesh_clean_hostmath(), r["vertices"], r["triangles"], len(r["vertices"]))
    assert comp["n_triangles"].tolist() == [1620, 768]
    for k in range(2):
        assert K.closed_and_oriented(r["triangles"][comp["tri_component"] == k])
    first = r["triangles"][comp["tri_component"] == 0]
    for kw in (dict(min_triangles=769), dict(largest_only=True)):
        one = _clean("two_spheres", **kw)
        assert one["stats"]["components"] == 2 and one["stats"]["components_kept"] == 1
        M.assert_bytes(one["vertices"][one["triangles"]], r["vertices"][first])
    assert len(_clean("two_spheres", min_triangles=768)["triangles"]) == 2388
    assert len(_clean("two_spheres", min_triangles=1621)["triangles"]) == 0


def test_sphere_views_falls_into_pieces():
    r = _clean("sphere_views")
    comp = K.components_host(K.load_mesh_clean_hostmath(), r["vertices"], r["triangles"], len(r["vertices"]))
    sizes = np.sort(comp["n_triangles"])[::-1]
    assert len(sizes) == 27 and sizes[:5].tolist() == [718, 364, 362, 352, 300] and sizes[5:].max() <= 14
    assert len(_clean("sphere_views", min_triangles=15)["triangles"]) == 2096


def test_largest_only_tie_goes_to_the_smaller_root():
    v, c, t = K.hand_meshes()["two_tetrahedra"]
    r = K.clean_host(K.load_mesh_clean_hostmath(), v, c, t, largest_only=True)
    assert r["vertex_index"].tolist() == [0, 1, 2, 3] and r["triangle_index"].tolist() == [4, 5, 6, 7]


def test_sphere_inside_normals_are_radial_and_follow_the_winding(host):
    v, c, t = K.extracted("sphere_inside")
    n, valid = K.normals_host(host, v, t)
    assert valid.all()
    vol = M.volume_cases()["sphere_inside"]
    radial = v.astype(np.float64) - vol["centre"]
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cos = (n.astype(np.float64) * radial).sum(1)
    print("sphere_inside: least cosine of a vertex normal with the radial direction %.4f" % cos.min())
    assert cos.min() >= 0.98
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    back, bvalid = K.normals_host(host, v, t[:, ::-1].copy())
    M.assert_bytes(back, -n)
    M.assert_bytes(bvalid, valid)


def test_exact_zero_plane_normals_need_the_cleaning(host):
    v, c, t = K.extracted("exact_zero_plane")
    n, valid = K.normals_host(host, v, t)
    assert int((valid == 0).sum()) == 19 and not n[valid == 0].any()
    r = _clean("exact_zero_plane", normals=True)
    assert len(r["normals"]) == 30 and r["normals_valid"].all()


def test_mesh_ply_round_trip_with_normals(tmp_path):
    from mvster_amd import mesh
    r = _clean("exact_zero_plane", normals=True)
    f = str(tmp_path / "n.ply")
    mesh.write_mesh_ply(f, r["vertices"], r["triangles"], r["colors"], r["normals"])
    head = open(f, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    props = [l.split()[-1] for l in head if l.startswith("property") and "list" not in l]
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    got = mesh.read_mesh_ply(f, with_normals=True)
    assert len(got) == 4
    for g, w in zip(got, (r["vertices"], r["triangles"], r["colors"], r["normals"])):
        M.assert_bytes(g, w)
    plain = mesh.read_mesh_ply(f)                                               # the default reads such a file too, as a 3-tuple
    assert len(plain) == 3
    for g, w in zip(plain, (r["vertices"], r["triangles"], r["colors"])):
        M.assert_bytes(g, w)
    mesh.write_mesh_ply(f, r["vertices"], r["triangles"], normals=r["normals"])    # normals without colours
    v, t, c, n = mesh.read_mesh_ply(f, with_normals=True)
    assert c is None
    M.assert_bytes(n, r["normals"])
    mesh.write_mesh_ply(f, r["vertices"], r["triangles"], r["colors"])             # a file without normals
    assert mesh.read_mesh_ply(f, with_normals=True)[3] is None
    with pytest.raises(RuntimeError, match="normals must be"):
        mesh.write_mesh_ply(f, r["vertices"], r["triangles"], normals=r["normals"][:-1])
    res = dict(mesh_vertices=r["vertices"], mesh_triangles=r["triangles"], mesh_colors=r["colors"], mesh_normals=r["normals"])
    mesh.write_result_mesh(f, res)
    M.assert_bytes(mesh.read_mesh_ply(f, with_normals=True)[3], r["normals"])
    del res["mesh_normals"]
    mesh.write_result_mesh(f, res)
    assert mesh.read_mesh_ply(f, with_normals=True)[3] is None


def test_clean_spec_checks_and_defaults():
    from mvster_amd import fusion, mesh, scan
    assert fusion.MeshClean is mesh.MeshClean and mesh.MeshClean() == (True, 0, False, False)
    assert mesh.check_clean_spec("x", None) is None and mesh.check_clean_spec("x", None, None) is None
    assert mesh.check_clean_spec("x", mesh.MeshClean(False, 15), mesh.TSDFMesh(0.1)) == (False, 15, False, False)
    spec = mesh.TSDFMesh(0.1)
    calls = (lambda b, m: fusion.fuse_scene(None, None, None, None, None, None, 0.9, 3, mesh=m, mesh_clean=b),
             lambda b, m: fusion.filter_depth("a", "b", "c", "d.ply", mesh=m, meshfilename=None if m is None else "m.ply", mesh_clean=b),
             lambda b, m: scan.reconstruct_scan(None, None, None, None, None, None, mesh=m, mesh_clean=b))
    for bad, match in (((True, 0, False, False), "MeshClean"), (mesh.MeshClean(1), "weld"), (mesh.MeshClean(True, -1), "min_triangles"),
                       (mesh.MeshClean(True, 1.5), "min_triangles"), (mesh.MeshClean(True, True), "min_triangles"),
                       (mesh.MeshClean(True, 0, None), "largest_only"), (mesh.MeshClean(True, 0, False, "yes"), "normals")):
        for call in calls:
            with pytest.raises(RuntimeError, match=match):
                call(bad, spec)
        with pytest.raises(RuntimeError, match=match):
            mesh.mesh_scene(None, None, None, None, None, 0.1, mesh_clean=bad)
    for call in calls:                                                          # a MeshClean without a mesh to clean
        with pytest.raises(RuntimeError, match="mesh_clean needs mesh="):
            call(mesh.MeshClean(), None)
    for fn in (fusion.fuse_scene, fusion.filter_depth, scan.reconstruct_scan, mesh.mesh_scene):
        assert inspect.signature(fn).parameters["mesh_clean"].default is None, fn.__name__


def test_clean_mesh_argument_checks():
    import torch
    from mvster_amd import mesh
    v, t = torch.zeros(5, 3), torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32)
    c = torch.zeros(5, 3, dtype=torch.uint8)
    for kw, match in ((dict(min_triangles=-1), "min_triangles"), (dict(min_triangles=2.0), "min_triangles"), (dict(weld=1), "weld"),
                      (dict(largest_only=0), "largest_only"), (dict(normals="x"), "normals"), (dict(table_slots=63), "table_slots"),
                      (dict(table_slots=96), "table_slots"), (dict(table_slots=1 << 31), "table_slots"), (dict(table_slots=64.0), "table_slots")):
        with pytest.raises(RuntimeError, match=match):
            mesh.clean_mesh(v, t, c, **kw)
    with pytest.raises(RuntimeError, match="table_slots"):                      # a power of two, but below 2 * Nv
        mesh.clean_mesh(torch.zeros(40, 3), t, table_slots=64)
    assert mesh.clean_slots(0) == 64 and mesh.clean_slots(32) == 64 and mesh.clean_slots(33) == 128 and mesh.clean_slots(1 << 29) == 1 << 30
    for bad in (torch.tensor([[0, 1, 5]], dtype=torch.int32), torch.tensor([[0, -1, 2]], dtype=torch.int32)):
        for call in (lambda: mesh.clean_mesh(v, bad), lambda: mesh.vertex_normals(v, bad), lambda: mesh.mesh_components(bad, 5)):
            with pytest.raises(RuntimeError, match="outside 0 .. 4"):
                call()
    with pytest.raises(RuntimeError, match=r"vertices must be a float32 tensor \[Nv,3\]"):
        mesh.clean_mesh(v.double(), t)
    with pytest.raises(RuntimeError, match=r"triangles must be an int32 tensor \[Nt,3\]"):
        mesh.clean_mesh(v, t.long())
    with pytest.raises(RuntimeError, match="colors must be"):
        mesh.clean_mesh(v, t, c[:4])
    with pytest.raises(RuntimeError, match="n_vertices"):
        mesh.mesh_components(t, -1)
    for call in (lambda: mesh.clean_mesh(v, t, c), lambda: mesh.vertex_normals(v, t), lambda: mesh.mesh_components(t, 5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):              # everything is in order: only the GPU is missing
            call()


def test_abi_entry_points_validate_before_any_hip_call():
    import __graft_entry__ as ge
    ge.build()
    from mvster_amd import _lib
    lib = _lib.load()
    import ctypes
    a, b = ctypes.c_long(-1), ctypes.c_long(-1)
    assert lib.mvster_mesh_clean_work(10, 7, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (80 + 14 + 3, 3 * 2 + 8)
    assert lib.mvster_mesh_clean_work(257, 300, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (8 * 257 + 600 + 6, 3 * 3 + 8)
    assert lib.mvster_mesh_clean_work(-1, 0, ctypes.byref(a), ctypes.byref(b)) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_clean_work(0, (1 << 29) + 1, ctypes.byref(a), ctypes.byref(b)) == _lib.ERR_SHAPE
    assert lib.mvster_mesh_clean_work(1, 1, None, ctypes.byref(b)) == _lib.ERR_NULL
    assert lib.mvster_mesh_normals_blocks(0) == 0 and lib.mvster_mesh_normals_blocks(257) == 2 and lib.mvster_mesh_normals_blocks(-1) == _lib.ERR_SHAPE
    p = 1 << 32                                                                  # a stand-in address nothing may dereference
    plan = lambda **kw: lib.mvster_mesh_clean_plan(*[dict(dict(vertices=p, triangles=p, Nv=10, Nt=7, weld=1, min_triangles=0,
                                                               largest_only=0, table=p, slots=64, canon=p, labels=p, tl=p, tc=p, roots=p,
                                                               cv=p, ct=p, rows=7, wi=p, wl=p, stream=None), **kw)[k] for k in
                                                     ("vertices", "triangles", "Nv", "Nt", "weld", "min_triangles", "largest_only", "table",
                                                      "slots", "canon", "labels", "tl", "tc", "roots", "cv", "ct", "rows", "wi", "wl", "stream")])
    for k in ("vertices", "triangles", "table", "canon", "labels", "tl", "tc", "roots", "cv", "ct", "wi", "wl"):
        assert plan(**{k: None}) == _lib.ERR_NULL, k
    for kw in (dict(Nv=-1), dict(Nt=(1 << 29) + 1), dict(weld=2), dict(min_triangles=-1), dict(largest_only=-1), dict(slots=32),
               dict(slots=96), dict(Nv=33), dict(slots=1 << 31), dict(rows=-1)):
        assert plan(**kw) == _lib.ERR_SHAPE, kw
    assert plan(Nv=0) == 0 and plan(Nt=0) == 0                                  # an empty mesh: nothing to do
    emit = lambda **kw: lib.mvster_mesh_clean_emit(*[dict(dict(vertices=p, colors=p, triangles=p, Nv=10, Nt=7, canon=p, wi=p, nvo=4,
                                                               nto=3, ov=p, oc=p, ot=p, vi=p, ti=p, stream=None), **kw)[k] for k in
                                                     ("vertices", "colors", "triangles", "Nv", "Nt", "canon", "wi", "nvo", "nto", "ov",
                                                      "oc", "ot", "vi", "ti", "stream")])
    for k in ("vertices", "triangles", "canon", "wi", "ov", "oc", "ot", "vi", "ti"):
        assert emit(**{k: None}) == _lib.ERR_NULL, k
    for kw in (dict(nvo=11), dict(nto=8), dict(nvo=-1), dict(Nv=-1)):
        assert emit(**kw) == _lib.ERR_SHAPE, kw
    assert emit(nvo=0, nto=0, ov=None, ot=None) == 0
    normals = lambda **kw: lib.mvster_mesh_vertex_normals(*[dict(dict(vertices=p, triangles=p, Nv=10, Nt=7, counts=p, starts=p, rows=p,
                                                                      normals=p, valid=p, stream=None), **kw)[k] for k in
                                                            ("vertices", "triangles", "Nv", "Nt", "counts", "starts", "rows", "normals", "valid",
                                                             "stream")])
    for k in ("vertices", "triangles", "counts", "starts", "rows", "normals", "valid"):
        assert normals(**{k: None}) == _lib.ERR_NULL, k
    assert normals(Nv=-1) == _lib.ERR_SHAPE and normals(Nt=(1 << 29) + 1) == _lib.ERR_SHAPE and normals(Nv=0) == 0
