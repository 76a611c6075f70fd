"""Mesh cleaning on the GPU against the host build of mvster_amd/csrc/mesh_math.h, byte for byte: every mesh
of tests/mesh_cases.py and the hand-built meshes of tests/mesh_clean_cases.py, every case twice with the second run compared byte
for byte against the first, outputs pre-filled with a sentinel, and one synthetic scan through ``reconstruct_scan``."""
import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, fusion, mesh, scan
from tests import mesh_cases as M
from tests import mesh_clean_cases as K
from tests import scan_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILLS = (0xA5, 0x3C)


def on_gpu(name):
    v, c, t = K.all_meshes()[name]
    return torch.from_numpy(v).to(DEV), torch.from_numpy(c).to(DEV), torch.from_numpy(t).to(DEV)


def host_arrays(r):
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in r.items()}


@pytest.mark.parametrize("name", sorted(K.all_meshes()))
def test_clean_mesh_equals_the_host_build(name):
    v, c, t = on_gpu(name)
    for s, setting in enumerate(K.SETTINGS):
        want = K.host_clean(name, s)
        runs = [host_arrays(mesh.clean_mesh(v, t, c, normals=True, fill=f, **setting)) for f in FILLS]
        K.assert_clean_equal(runs[0], want, (name, setting))
        K.assert_clean_equal(runs[1], runs[0], (name, setting, "second run"))
    got = host_arrays(mesh.clean_mesh(v, t, None, normals=False))              # without colours, without normals
    assert got["colors"] is None and "normals" not in got
    K.assert_clean_equal(dict(got, colors=K.host_clean(name, 0)["colors"]), {k: x for k, x in K.host_clean(name, 0).items() if
                                                                            k not in ("normals", "normals_valid")}, (name, "plain"))


@pytest.mark.parametrize("name", sorted(K.all_meshes()))
def test_components_and_normals_equal_the_host_build(name):
    v, c, t = on_gpu(name)
    hv, hc, ht = K.all_meshes()[name]
    h = K.load_mesh_clean_hostmath()
    want = K.components_host(h, None, ht, len(hv))
    runs = [host_arrays(mesh.mesh_components(t, len(hv))) for _ in range(2)]
    for k in K.COMPONENT_KEYS:
        M.assert_bytes(runs[0][k], want[k], (name, k))
        M.assert_bytes(runs[1][k], runs[0][k], (name, k, "second run"))
    wn, wv = K.normals_host(h, hv, ht)
    for f in FILLS:
        got = mesh.vertex_normals(v, t, fill=f)
        M.assert_bytes(got["normals"].cpu().numpy(), wn, (name, "normals", f))
        M.assert_bytes(got["valid"].cpu().numpy(), wv, (name, "valid", f))


def test_cases_are_what_they_are_for():
    """The hand-built meshes do reach the sizes they were built for"""
    hm = K.hand_meshes()
    v, c, t = hm["fan_3000"]
    assert np.bincount(t.reshape(-1)).max() == 3000
    assert K.host_clean("separate_2000", 0)["stats"]["components"] == 2000 and K.host_clean("separate_6000", 0)["stats"]["components"] == 6000
    assert ("random_%dx%d" % (K.SCAN_TILE + 1, K.SCAN_TILE + 1)) in hm
    r = K.host_clean("coincident_600", 0)
    assert r["stats"]["welded"] == 599 and r["vertex_index"][0] == 0
    assert K.host_clean("strip_5000", 0)["stats"]["components"] == 1
    assert K.host_clean("two_tetrahedra", 3)["triangle_index"].tolist() == [4, 5, 6, 7]
    assert K.host_clean("not_finite", 0)["stats"]["degenerate"] > 0 and K.host_clean("repeated_indices", 0)["stats"]["degenerate"] == 4
    assert K.host_clean("unused_vertices", 0)["stats"]["vertices_removed"] == 7


def test_scans_past_their_first_pass():
    """More than 16 384 workgroups of 256: the scans of the roots, of the kept vertices and triangles and of the normals' rows all
    take a second pass, and the offsets behind it are the host build's"""
    hv, hc, ht = K.tile_crossing_mesh()
    h = K.load_mesh_clean_hostmath()
    v, c, t = torch.from_numpy(hv).to(DEV), torch.from_numpy(hc).to(DEV), torch.from_numpy(ht).to(DEV)
    want = K.clean_host(h, hv, hc, ht, normals=True)
    assert len(want["vertices"]) > K.SCAN_TILE * 256 and want["stats"]["components"] == 3 * K.TILE_CROSSING_TRIANGLES // 4
    runs = [host_arrays(mesh.clean_mesh(v, t, c, normals=True, fill=f)) for f in FILLS]
    K.assert_clean_equal(runs[0], want, "tile crossing")
    K.assert_clean_equal(runs[1], runs[0], "tile crossing, second run")
    del runs
    pairs = K.clean_host(h, hv, hc, ht, min_triangles=2)
    assert pairs["stats"]["components_kept"] == K.TILE_CROSSING_TRIANGLES // 4 and len(pairs["triangles"]) == K.TILE_CROSSING_TRIANGLES // 2
    K.assert_clean_equal(host_arrays(mesh.clean_mesh(v, t, c, min_triangles=2, fill=FILLS[0])), pairs, "tile crossing, pairs")
    comp = mesh.mesh_components(t, len(hv))
    assert len(comp["roots"]) == want["stats"]["components"]
    first = ht.reshape(-1, 4, 3)                                                # triangles 4k and 4k+1 are one component
    roots = np.sort(np.concatenate([np.minimum(first[:, 0].min(1), first[:, 1].min(1)), first[:, 2].min(1), first[:, 3].min(1)]))
    M.assert_bytes(comp["roots"].cpu().numpy(), roots.astype(np.int32), "roots")


def test_empty_inputs_give_empty_meshes():
    for nv, nt in ((0, 0), (5, 0)):
        v, t = torch.zeros(nv, 3, device=DEV), torch.zeros(nt, 3, device=DEV, dtype=torch.int32)
        c = torch.zeros(nv, 3, device=DEV, dtype=torch.uint8)
        r = mesh.clean_mesh(v, t, c, normals=True)
        for k, shape, dtype in (("vertices", (0, 3), torch.float32), ("colors", (0, 3), torch.uint8), ("triangles", (0, 3), torch.int32),
                                ("vertex_index", (0,), torch.int64), ("triangle_index", (0,), torch.int64),
                                ("normals", (0, 3), torch.float32), ("normals_valid", (0,), torch.uint8)):
            assert tuple(r[k].shape) == shape and r[k].dtype == dtype and r[k].device.type == "cuda", k
        assert r["stats"] == dict(welded=0, degenerate=0, components=0, components_kept=0, triangles_removed=0, vertices_removed=nv)
        comp = mesh.mesh_components(t, nv)
        assert comp["labels"].tolist() == [-1] * nv and all(len(comp[k]) == 0 for k in K.COMPONENT_KEYS[1:])
        n = mesh.vertex_normals(v, t)
        assert tuple(n["normals"].shape) == (nv, 3) and not n["normals"].any() and not n["valid"].any()
    # the empty extraction through mesh_scene's path: no_sign_change
    v, c, t = on_gpu("no_sign_change")
    assert len(v) == 0 and len(mesh.clean_mesh(v, t, c)["triangles"]) == 0


@pytest.mark.parametrize("name", ["exact_zero_random", "coincident_600", "random_257x255", "sphere_views"])
def test_a_larger_table_gives_the_same_bytes(name):
    v, c, t = on_gpu(name)
    want = K.host_clean(name, 0)
    got = host_arrays(mesh.clean_mesh(v, t, c, normals=True, table_slots=4 * mesh.clean_slots(len(v)), fill=FILLS[0]))
    K.assert_clean_equal(got, want, name)


def test_sentinel_behind_the_outputs_survives():
    """The emit kernel writes Nv' and Nt' entries and nothing behind them: called on buffers two entries longer than the counts, the
    tail keeps the sentinel"""
    name = "random_257x255"
    v, c, t = on_gpu(name)
    want = K.host_clean(name, 0)
    plan = mesh._CleanPlan("test", v, t, len(v), True, 0, False, mesh.clean_slots(len(v)))
    nv, nt = plan.nv_out, plan.nt_out
    assert (nv, nt) == (len(want["vertices"]), len(want["triangles"])) and nv > 5 and nt > 5

    def buffers(nv_room, nt_room):
        return (torch.full((nv_room, 3), -7.0, device=DEV), torch.full((nv_room, 3), FILLS[0], device=DEV, dtype=torch.uint8),
                torch.full((nt_room, 3), -7, device=DEV, dtype=torch.int32), torch.full((nv_room,), -7, device=DEV, dtype=torch.int64),
                torch.full((nt_room,), -7, device=DEV, dtype=torch.int64))
    ov, oc, ot, vi, ti = buffers(nv + 2, nt + 2)
    plan.emit(c, ov, oc, ot, vi, ti)
    for got, key, n in ((ov, "vertices", nv), (oc, "colors", nv), (ot, "triangles", nt), (vi, "vertex_index", nv), (ti, "triangle_index", nt)):
        M.assert_bytes(got[:n].cpu().numpy(), want[key], key)
    assert bool((ov[nv:] == -7.0).all()) and bool((oc[nv:] == FILLS[0]).all()) and bool((ot[nt:] == -7).all())
    assert bool((vi[nv:] == -7).all()) and bool((ti[nt:] == -7).all())
    # a capacity below the counts: the entries that fit are written, nothing else
    ov, oc, ot, vi, ti = buffers(nv, nt)
    plan.emit(c, ov, oc, ot, vi, ti, nv_out=nv - 5, nt_out=nt - 3)
    M.assert_bytes(ov[:nv - 5].cpu().numpy(), want["vertices"][:nv - 5])
    M.assert_bytes(ti[:nt - 3].cpu().numpy(), want["triangle_index"][:nt - 3])
    assert bool((ov[nv - 5:] == -7.0).all()) and bool((vi[nv - 5:] == -7).all()) and bool((ot[nt - 3:] == -7).all())
    # the normals write Nv rows
    n, valid = torch.full((nv + 2, 3), -7.0, device=DEV), torch.full((nv + 2,), FILLS[0], device=DEV, dtype=torch.uint8)
    from mvster_amd import _lib
    gv, gt = torch.from_numpy(want["vertices"]).to(DEV), torch.from_numpy(want["triangles"]).to(DEV)
    blocks = _lib.load().mvster_mesh_normals_blocks(nv)
    counts, starts = torch.empty(2 * nv + blocks, device=DEV, dtype=torch.int32), torch.empty(blocks + 1, device=DEV, dtype=torch.int64)
    rows = torch.empty(3 * nt, device=DEV, dtype=torch.int32)
    _lib.check(_lib.load().mvster_mesh_vertex_normals(gv.data_ptr(), gt.data_ptr(), nv, nt, counts.data_ptr(), starts.data_ptr(),
                                                      rows.data_ptr(), n.data_ptr(), valid.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "normals")
    M.assert_bytes(n[:nv].cpu().numpy(), want["normals"])
    assert bool((n[nv:] == -7.0).all()) and bool((valid[nv:] == FILLS[0]).all())


def test_mesh_scene_with_a_clean_spec():
    c = M.map_cases()["sphere_views"]
    lo, hi = np.asarray(c["centre"]) - c["radius"], np.asarray(c["centre"]) + c["radius"]
    args = (c["depths"], c["masks"], c["images"], c["Ks"], c["Es"], c["voxel"])
    plain = mesh.mesh_scene(*args, bounds=(lo, hi), min_weight=1, device=DEV)
    got = mesh.mesh_scene(*args, bounds=(lo, hi), min_weight=1, device=DEV, mesh_clean=mesh.MeshClean(True, 15, False, True))
    want = mesh.clean_mesh(plain["vertices"], plain["triangles"], plain["colors"], True, 15, False, True)
    for k in ("vertices", "colors", "triangles", "normals", "normals_valid"):
        assert torch.equal(got[k], want[k]), k
    assert got["clean_stats"] == want["stats"] and len(got["triangles"]) < len(plain["triangles"])
    assert sorted(set(got) - set(plain)) == ["clean_stats", "normals", "normals_valid"]


def test_reconstruct_scan_with_a_cleaned_mesh(shipped_cfg, checkpoint, tmp_path):
    """One synthetic scan of 7 views at 128 x 192: with a ``MeshClean`` the mesh keys hold ``clean_mesh`` of the ``mesh=``-only
    result, the file reads back to the result's bytes with its normals, and the ``mesh=``-only result is what it was"""
    model = MVS4net(**shipped_cfg)
    model.load_state_dict(checkpoint, strict=True)
    model = model.to(DEV).eval()
    sc = SC.synthetic_scan(7, 128, 192, seed=7)
    args = (model, sc["images"], sc["Ks"], sc["Es"], sc["depth_ranges"], SC.ring_pairs(7, 4))
    kw = dict(conf=0.05, thres_view=1)
    plain = scan.reconstruct_scan(*args, **kw)
    lo, hi = plain["points"].amin(0).double().cpu().numpy(), plain["points"].amax(0).double().cpu().numpy()
    spec = fusion.TSDFMesh(float((hi - lo).max()) / 40, None, 1)
    only = scan.reconstruct_scan(*args, mesh=spec, **kw)
    assert sorted(set(only) - set(plain)) == ["mesh_colors", "mesh_triangles", "mesh_vertices", "mesh_volume"]
    ply = str(tmp_path / "mesh.ply")
    clean = fusion.MeshClean(True, 15, False, True)
    got = scan.reconstruct_scan(*args, mesh=spec, mesh_clean=clean, meshfilename=ply, **kw)
    assert sorted(set(got) - set(only)) == ["mesh_clean_stats", "mesh_normals", "mesh_normals_valid"]
    for k in plain:
        assert torch.equal(got[k], plain[k]) and torch.equal(only[k], plain[k]), k
    assert got["mesh_volume"] == only["mesh_volume"]
    want = mesh.clean_mesh(only["mesh_vertices"], only["mesh_triangles"], only["mesh_colors"], *clean)
    for k, w in (("vertices", "vertices"), ("colors", "colors"), ("triangles", "triangles"), ("normals", "normals"),
                 ("normals_valid", "normals_valid")):
        assert torch.equal(got["mesh_" + k], want[w]), k
    assert got["mesh_clean_stats"] == want["stats"]
    print("reconstruct_scan with a cleaned mesh: %d / %d -> %d / %d vertices / triangles, %r" %
          (len(only["mesh_vertices"]), len(only["mesh_triangles"]), len(got["mesh_vertices"]), len(got["mesh_triangles"]),
           got["mesh_clean_stats"]))
    assert 0 < len(got["mesh_triangles"]) <= len(only["mesh_triangles"])
    v, t, c, n = mesh.read_mesh_ply(ply, with_normals=True)
    for g, key in ((v, "mesh_vertices"), (t, "mesh_triangles"), (c, "mesh_colors"), (n, "mesh_normals")):
        M.assert_bytes(g, got[key].cpu().numpy(), key)
    # against the host build, from the mesh=-only result's bytes
    host = K.clean_host(K.load_mesh_clean_hostmath(), *(only["mesh_" + k].cpu().numpy() for k in ("vertices", "colors", "triangles")),
                        weld=True, min_triangles=15, largest_only=False, normals=True)
    K.assert_clean_equal(dict(host_arrays(want)), host, "scan")
