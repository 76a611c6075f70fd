"""TSDF integration and marching tetrahedra on the GPU: the kernels of mvster_amd/csrc/geo_mesh.hip
byte for byte against the host build of mvster_amd/csrc/tsdf_math.h on every case of tests/mesh_cases.py, a second run byte
for byte against the first, outputs pre-filled with a sentinel, and one synthetic scan through ``reconstruct_scan``."""
import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, fusion, mesh, scan
from tests import mesh_cases as M
from tests import scan_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5


def volume_on_gpu(v):
    nx, ny, nz = v["dims"]
    t = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)
    return mesh.TSDFVolume(t(v["tsdf"], np.float32).reshape(nz, ny, nx), t(v["weight"], np.int32).reshape(nz, ny, nx),
                           t(v["rgb"], np.uint8).reshape(nz, ny, nx, 3), t(v["has_color"], np.uint8).reshape(nz, ny, nx),
                           v["origin"], v["voxel"], v["dims"], v.get("trunc", 4 * v["voxel"]))


@pytest.mark.parametrize("name", sorted(M.map_cases()))
def test_integration_equals_the_host_build(name):
    c = M.map_cases()[name]
    want = M.host_volume(name)
    args = [c[k] for k in ("depths", "masks", "images", "Ks", "Es", "origin", "voxel", "dims", "trunc")]
    runs = [mesh.integrate_tsdf(*args, device=DEV, fill=FILL) for _ in range(2)]       # (an unwritten node would still hold FILL)
    for key in ("tsdf", "weight", "rgb", "has_color"):
        got = getattr(runs[0], key).cpu().numpy()
        M.assert_bytes(got, want[key], (name, key))
        M.assert_bytes(getattr(runs[1], key).cpu().numpy(), got, (name, key, "second run"))
    assert runs[0].dims == tuple(c["dims"]) and runs[0].origin == tuple(c["origin"])
    # tensors already on the GPU, masks as bytes, a list of maps: the same bytes
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    again = mesh.integrate_tsdf([dev(d) for d in c["depths"]], dev(c["masks"].astype(np.uint8) * 7), dev(c["images"]), *args[3:])
    M.assert_bytes(again.tsdf.cpu().numpy(), want["tsdf"], (name, "device inputs"))
    M.assert_bytes(again.rgb.cpu().numpy(), want["rgb"], (name, "device inputs"))


@pytest.mark.parametrize("name", sorted(M.all_volumes()))
def test_extraction_equals_the_host_build(name):
    v = M.all_volumes()[name]
    want = M.host_mesh(name)
    vol = volume_on_gpu(v)
    runs = [mesh.extract_mesh(vol, v["min_weight"], fill=FILL) for _ in range(2)]
    for got, w, key in zip(runs[0], want, ("vertices", "colors", "triangles")):
        assert got.device.type == "cuda"
        M.assert_bytes(got.cpu().numpy(), w, (name, key))                       # (an unwritten entry would still hold FILL)
    for a, b in zip(runs[0], runs[1]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), (name, "second run")
    assert runs[0].vertices.dtype == torch.float32 and runs[0].colors.dtype == torch.uint8 and runs[0].triangles.dtype == torch.int32


def test_sentinel_behind_the_outputs_survives():
    """The emit kernels write Nv and Nt entries and nothing behind them: called on buffers two entries longer than the counts, the
    tail keeps the sentinel"""
    from mvster_amd import _lib
    v = M.all_volumes()["grid_257x2x3"]
    want = M.host_mesh("grid_257x2x3")
    vol = volume_on_gpu(v)
    nx, ny, nz = v["dims"]
    lib = _lib.load()
    nodes = nx * ny * nz
    tiles = lib.mvster_mesh_blocks(nodes)
    edge_mask = torch.empty(nodes, device=DEV, dtype=torch.uint8)
    rank = torch.empty(nodes, device=DEV, dtype=torch.int16)
    counts = torch.empty(2, tiles, device=DEV, dtype=torch.int32)
    offsets = torch.empty(2, tiles + 1, device=DEV, dtype=torch.int64)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mvster_mesh_count(vol.tsdf.data_ptr(), vol.weight.data_ptr(), nx, ny, nz, 1, edge_mask.data_ptr(), rank.data_ptr(),
                                     counts[0].data_ptr(), counts[1].data_ptr(), offsets[0].data_ptr(), offsets[1].data_ptr(), stream),
               "mesh_count")
    nv, nt = (int(x) for x in offsets[:, tiles].cpu())
    assert (nv, nt) == (len(want[0]), len(want[2]))
    vertices = torch.full((nv + 2, 3), -7.0, device=DEV)
    colors = torch.full((nv + 2, 3), FILL, device=DEV, dtype=torch.uint8)
    triangles = torch.full((nt + 2, 3), -7, device=DEV, dtype=torch.int32)
    o = vol.origin
    _lib.check(lib.mvster_mesh_emit_vertices(vol.tsdf.data_ptr(), vol.rgb.data_ptr(), vol.has_color.data_ptr(), o[0], o[1], o[2],
                                             vol.voxel_size, nx, ny, nz, edge_mask.data_ptr(), rank.data_ptr(), offsets[0].data_ptr(),
                                             nv, vertices.data_ptr(), colors.data_ptr(), stream), "emit_vertices")
    _lib.check(lib.mvster_mesh_emit_triangles(vol.tsdf.data_ptr(), vol.weight.data_ptr(), nx, ny, nz, 1, edge_mask.data_ptr(),
                                              rank.data_ptr(), offsets[0].data_ptr(), offsets[1].data_ptr(), nv, nt,
                                              triangles.data_ptr(), stream), "emit_triangles")
    M.assert_bytes(vertices[:nv].cpu().numpy(), want[0])
    M.assert_bytes(triangles[:nt].cpu().numpy(), want[2])
    assert bool((vertices[nv:] == -7.0).all()) and bool((colors[nv:] == FILL).all()) and bool((triangles[nt:] == -7).all())
    # a capacity below the count: the entries that fit are written, nothing else
    short = torch.full((nv, 3), -7.0, device=DEV)
    _lib.check(lib.mvster_mesh_emit_vertices(vol.tsdf.data_ptr(), vol.rgb.data_ptr(), vol.has_color.data_ptr(), o[0], o[1], o[2],
                                             vol.voxel_size, nx, ny, nz, edge_mask.data_ptr(), rank.data_ptr(), offsets[0].data_ptr(),
                                             nv - 5, short.data_ptr(), colors.data_ptr(), stream), "emit_vertices")
    M.assert_bytes(short[:nv - 5].cpu().numpy(), want[0][:nv - 5])
    assert bool((short[nv - 5:] == -7.0).all())


def test_empty_result_is_three_empty_tensors():
    v = M.all_volumes()["no_sign_change"]
    m = mesh.extract_mesh(volume_on_gpu(v), v["min_weight"])
    assert tuple(m.vertices.shape) == (0, 3) and tuple(m.colors.shape) == (0, 3) and tuple(m.triangles.shape) == (0, 3)
    assert m.vertices.dtype == torch.float32 and m.colors.dtype == torch.uint8 and m.triangles.dtype == torch.int32
    assert m.vertices.device.type == "cuda"
    # every node unknown: the same
    m = mesh.extract_mesh(volume_on_gpu(M.all_volumes()["sphere_inside"]), 5)
    assert len(m.vertices) == 0 and len(m.triangles) == 0


def test_mesh_scene_equals_integrate_then_extract():
    c = M.map_cases()["sphere_views"]
    lo = np.asarray(c["centre"]) - c["radius"]
    hi = np.asarray(c["centre"]) + c["radius"]
    got = mesh.mesh_scene(c["depths"], c["masks"], c["images"], c["Ks"], c["Es"], c["voxel"], bounds=(lo, hi), min_weight=1, device=DEV)
    origin, dims = mesh.grid_for_bounds("t", lo, hi, c["voxel"], 4 * c["voxel"])
    assert got["volume"].origin == origin and got["volume"].dims == dims and got["volume"].trunc == 4 * c["voxel"]
    h = M.load_tsdf_hostmath()
    vol = M.integrate_host(h, c["depths"], c["masks"], c["images"], c["Ks"], c["Es"], origin, c["voxel"], dims, 4 * c["voxel"])
    want = M.extract_host(h, *vol, origin, c["voxel"], dims, 1)
    for key, w in zip(("vertices", "colors", "triangles"), want):
        M.assert_bytes(got[key].cpu().numpy(), w, key)
    assert len(want[2]) > 1000
    err = np.abs(np.linalg.norm(want[0].astype(np.float64) - c["centre"], axis=1) - c["radius"])
    assert err.max() <= (4 + np.sqrt(3)) * c["voxel"]                           # trunc + the longest edge (tests/test_mesh_cpu.py)
    # without bounds: the box of the frusta, refused by a small budget with the voxel size that fits
    with pytest.raises(RuntimeError, match="voxel_size of"):
        mesh.mesh_scene(c["depths"], c["masks"], c["images"], c["Ks"], c["Es"], c["voxel"] / 8, min_weight=1, device=DEV,
                        memory_budget=1 << 20)
    free = mesh.mesh_scene(c["depths"], c["masks"], c["images"], c["Ks"], c["Es"], c["voxel"], min_weight=1, device=DEV)
    box_lo, box_hi = np.asarray(free["volume"].origin), np.asarray(free["volume"].origin) + c["voxel"] * (np.asarray(free["volume"].dims) - 1)
    assert (box_lo <= lo).all() and (box_hi >= hi).all() and len(free["triangles"]) > 1000


def test_reconstruct_scan_with_a_mesh(shipped_cfg, checkpoint, tmp_path):
    """One synthetic scan of 7 views at 128 x 192: the mesh keys are there, equal ``mesh_scene`` on the result's own maps, the
    file reads back, and every other key is byte-equal to the run without ``mesh``"""
    model = MVS4net(**shipped_cfg)
    model.load_state_dict(checkpoint, strict=True)
    model = model.to(DEV).eval()
    sc = SC.synthetic_scan(7, 128, 192, seed=7)
    args = (model, sc["images"], sc["Ks"], sc["Es"], sc["depth_ranges"], SC.ring_pairs(7, 4))
    kw = dict(conf=0.05, thres_view=1)
    plain = scan.reconstruct_scan(*args, **kw)
    assert len(plain["points"]) > 0 and not any(k.startswith("mesh_") for k in plain)
    lo, hi = plain["points"].amin(0).double().cpu().numpy(), plain["points"].amax(0).double().cpu().numpy()
    voxel = float((hi - lo).max()) / 40
    spec = fusion.TSDFMesh(voxel, None, 1)
    ply = str(tmp_path / "mesh.ply")
    got = scan.reconstruct_scan(*args, mesh=spec, meshfilename=ply, **kw)
    assert sorted(set(got) - set(plain)) == ["mesh_colors", "mesh_triangles", "mesh_vertices", "mesh_volume"]
    for k in plain:
        assert torch.equal(got[k], plain[k]), k
    nv, nt = len(got["mesh_vertices"]), len(got["mesh_triangles"])
    print("reconstruct_scan with a mesh: %d points -> %d vertices, %d triangles in %s nodes" % (len(plain["points"]), nv, nt,
                                                                                                  got["mesh_volume"]["dims"]))
    assert nv > 0 and nt > 0 and got["mesh_volume"]["voxel_size"] == voxel and got["mesh_volume"]["trunc"] == 4 * voxel
    assert got["mesh_volume"]["bounds"] == (tuple(lo), tuple(hi)) and got["mesh_volume"]["min_weight"] == 1
    refs = np.asarray(got.scan["ref_views"])
    images = torch.from_numpy(sc["images"]).to(DEV)[torch.from_numpy(refs).to(DEV)]
    want = mesh.mesh_scene(got["depth_est_averaged"].float(), got["final_mask"], images, got.scan["Ks"][refs], got.scan["Es"][refs],
                           voxel, None, (lo, hi), 1)
    for k in ("vertices", "colors", "triangles"):
        assert torch.equal(got["mesh_" + k], want[k]), k
    v, t, c = mesh.read_mesh_ply(ply)
    M.assert_bytes(v, got["mesh_vertices"].cpu().numpy())
    M.assert_bytes(t, got["mesh_triangles"].cpu().numpy())
    M.assert_bytes(c, got["mesh_colors"].cpu().numpy())
    assert t.max() < nv and len(np.unique(t)) == nv
