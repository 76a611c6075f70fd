"""Brick-sparse TSDF volumes on the GPU: the kernels of mvster_amd/csrc/geo_mesh_sparse.hip byte for byte
against the host build of mvster_amd/csrc/tsdf_sparse_math.h -- the directory, the brick list, the brick-major volume, vertices,
colours, triangles and keys -- a second run against the first, sentinels behind every output, and the scan-level calls with
``sparse=True`` against the dense path in canonical form."""
import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, _lib, fusion, mesh, scan
from tests import mesh_cases as M
from tests import mesh_sparse_cases as S
from tests import scan_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
ALLOC_KEYS = ("depths", "masks", "Ks", "Es", "origin", "voxel", "dims", "trunc")


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def sparse_on_gpu(vol, bricks, c):
    nb = S.brick_dims(c["dims"])
    return mesh.SparseTSDFVolume(t(S.directory(bricks, c["dims"]), np.int32).view(nb[2], nb[1], nb[0]), t(bricks, np.int32),
                                 t(vol["tsdf"], np.float32), t(vol["weight"], np.int32), t(vol["rgb"], np.uint8),
                                 t(vol["has_color"], np.uint8), c["origin"], c["voxel"], c["dims"], c.get("trunc", 4 * c["voxel"]))


def assert_mesh(got, want, what):
    for g, w, key in zip(got, want, ("vertices", "colors", "triangles", "keys")):
        assert g.device.type == "cuda"
        M.assert_bytes(g.cpu().numpy(), w, (what, key))                         # (an unwritten entry would still hold FILL)


def check_against_host(c, want, what):
    """allocate, integrate and extract a map case twice on the GPU: the host build's bytes, and the same bytes again"""
    runs = []
    for _ in range(2):
        slot, bricks = mesh.allocate_bricks(*(c[k] for k in ALLOC_KEYS), device=DEV)
        vol = mesh.integrate_tsdf_sparse(*(c[k] for k in S.MAP_KEYS), device=DEV, fill=FILL)
        runs.append((slot, bricks, vol, mesh.extract_mesh_sparse(vol, 1, keys=True, fill=FILL)))
    slot, bricks, vol, m = runs[0]
    nb = S.brick_dims(c["dims"])
    assert tuple(slot.shape) == (nb[2], nb[1], nb[0]) and slot.dtype == torch.int32 and bricks.dtype == torch.int32
    M.assert_bytes(bricks.cpu().numpy(), want["bricks"], (what, "bricks"))
    M.assert_bytes(slot.cpu().numpy().ravel(), S.directory(want["bricks"], c["dims"]), (what, "brick_slot"))
    M.assert_bytes(vol.bricks.cpu().numpy(), want["bricks"], (what, "the volume's bricks"))
    M.assert_bytes(vol.brick_slot.cpu().numpy(), slot.cpu().numpy(), (what, "the volume's directory"))
    for key in ("tsdf", "weight", "rgb", "has_color"):
        M.assert_bytes(getattr(vol, key).cpu().numpy(), want["volume"][key], (what, key))
        M.assert_bytes(getattr(runs[1][2], key).cpu().numpy(), getattr(vol, key).cpu().numpy(), (what, key, "second run"))
    assert_mesh(m, want["mesh"], what)
    assert_mesh(runs[1][3], [x.cpu().numpy() for x in m], (what, "second run"))
    assert m.vertices.dtype == torch.float32 and m.colors.dtype == torch.uint8 and m.triangles.dtype == torch.int32
    assert m.vertex_key.dtype == torch.int64 and vol.dims == tuple(c["dims"]) and vol.origin == tuple(c["origin"])
    return vol


@pytest.mark.parametrize("name,s", S.REFINED)
def test_map_cases_equal_the_host_build(name, s):
    vol = check_against_host(S.refined(name, s), S.host_sparse(name, s), (name, s))
    # without keys: a Mesh of the same three tensors
    m = mesh.extract_mesh_sparse(vol, 1)
    assert isinstance(m, mesh.Mesh)
    M.assert_bytes(m.triangles.cpu().numpy(), S.host_sparse(name, s)["mesh"][2], (name, s, "no keys"))


def test_the_plane_in_a_grid_of_2_to_the_32_nodes():
    want = S.host_huge()
    check_against_host(S.plane_huge(), want, "2048 x 2048 x 1024")
    assert want["mesh"][3].min() > 1 << 34


@pytest.mark.parametrize("name", S.ANY_S_VOLUMES)
def test_any_brick_set_equals_the_host_build(name):
    v = M.volume_cases()[name]
    hs = S.load_sparse_hostmath()
    for which in ("half", "full"):
        bricks = S.brick_sets(v["dims"], 17)[which]
        cut = S.cut_into_bricks(v, bricks)
        want = S.extract_sparse_host(hs, cut, bricks, v["origin"], v["voxel"], v["dims"], v["min_weight"])
        vol = sparse_on_gpu(cut, bricks, v)
        runs = [mesh.extract_mesh_sparse(vol, v["min_weight"], keys=True, fill=FILL) for _ in range(2)]
        assert_mesh(runs[0], want, (name, which))
        assert_mesh(runs[1], [x.cpu().numpy() for x in runs[0]], (name, which, "second run"))


@pytest.mark.parametrize("name,s", [("sphere_views", 4), ("bad_depths", 3)])
def test_a_callers_own_bricks(name, s):
    """``bricks=``: a seeded random half of the grid's bricks instead of the allocation"""
    c = S.refined(name, s)
    hs = S.load_sparse_hostmath()
    bricks = S.brick_sets(c["dims"], 5)["half"]
    want_vol = S.integrate_sparse_host(hs, *(c[k] for k in S.MAP_KEYS), bricks)
    want = S.extract_sparse_host(hs, want_vol, bricks, c["origin"], c["voxel"], c["dims"], 1)
    vol = mesh.integrate_tsdf_sparse(*(c[k] for k in S.MAP_KEYS), bricks=bricks, device=DEV, fill=FILL)
    M.assert_bytes(vol.brick_slot.cpu().numpy().ravel(), S.directory(bricks, c["dims"]), (name, "brick_slot"))
    for key in ("tsdf", "weight", "rgb", "has_color"):
        M.assert_bytes(getattr(vol, key).cpu().numpy(), want_vol[key], (name, key))
    assert_mesh(mesh.extract_mesh_sparse(vol, 1, keys=True, fill=FILL), want, name)
    assert len(want[2]) > 0
    # densify: the dense volume it means, through the dense extraction
    dense = mesh.extract_mesh(mesh.densify(vol), 1)
    assert len(dense.triangles) == len(want[2]) and len(dense.vertices) == len(want[0])
    order = np.argsort(want[3], kind="stable")                                  # dense order is (owner node, d): ascending keys
    M.assert_bytes(dense.vertices.cpu().numpy(), want[0][order], (name, "densify"))
    M.assert_bytes(dense.colors.cpu().numpy(), want[1][order], (name, "densify"))


def test_sentinels_behind_the_outputs_survive():
    """Every entry point writes its counts and nothing behind them: called on buffers two entries longer, the tails keep the
    sentinel"""
    name, s = "sphere_views", 4
    c, want = S.refined(name, s), S.host_sparse(name, s)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    nx, ny, nz = c["dims"]
    o, voxel, trunc = [float(x) for x in c["origin"]], float(c["voxel"]), float(c["trunc"])
    nbricks = lib.mvster_tsdf_sparse_bricks(nx, ny, nz)
    assert nbricks == int(np.prod(S.brick_dims(c["dims"])))
    depth, mask = t(c["depths"], np.float32), t(np.asarray(c["masks"]) != 0, np.uint8)
    img, views = t(c["images"], np.uint8), t(M.views_table(c["Ks"], c["Es"]), np.float64)
    V, H, W = depth.shape
    tiles = (nbricks + 511) // 512
    full = lambda n, dtype, shape=(): torch.full((n + 2,) + shape, FILL if dtype != torch.float32 else -7.0, device=DEV, dtype=dtype)
    kept = lambda x, n: bool((x[n:] == (FILL if x.dtype != torch.float32 else -7.0)).all())
    flags, counts, offsets = full(nbricks, torch.uint8), full(tiles, torch.int32), full(tiles + 1, torch.int64)
    _lib.check(lib.mvster_tsdf_sparse_mark(depth.data_ptr(), mask.data_ptr(), views.data_ptr(), V, H, W, *o, voxel, nx, ny, nz, trunc,
                                           flags.data_ptr(), stream), "mark")
    _lib.check(lib.mvster_tsdf_sparse_compact_count(flags.data_ptr(), nbricks, counts.data_ptr(), offsets.data_ptr(), stream), "count")
    n = int(offsets[tiles].cpu())
    assert n == len(want["bricks"]) and kept(flags, nbricks) and kept(counts, tiles) and kept(offsets, tiles + 1)
    slot, bricks = full(nbricks, torch.int32), full(n, torch.int32)
    _lib.check(lib.mvster_tsdf_sparse_compact_emit(flags.data_ptr(), nbricks, offsets.data_ptr(), n, slot.data_ptr(), bricks.data_ptr(),
                                                   stream), "emit")
    M.assert_bytes(bricks[:n].cpu().numpy(), want["bricks"])
    assert kept(slot, nbricks) and kept(bricks, n)
    # a capacity below the count: the bricks that fit, and the directory names no other
    short_slot, short = full(nbricks, torch.int32), full(n, torch.int32)
    _lib.check(lib.mvster_tsdf_sparse_compact_emit(flags.data_ptr(), nbricks, offsets.data_ptr(), n - 3, short_slot.data_ptr(),
                                                   short.data_ptr(), stream), "emit")
    M.assert_bytes(short[:n - 3].cpu().numpy(), want["bricks"][:n - 3])
    assert kept(short, n - 3) and int(short_slot[:nbricks].max()) == n - 4
    vol = [full(n * 512, torch.float32), full(n * 512, torch.int32), full(n * 512 * 3, torch.uint8), full(n * 512, torch.uint8)]
    _lib.check(lib.mvster_tsdf_sparse_integrate(depth.data_ptr(), mask.data_ptr(), img.data_ptr(), views.data_ptr(), V, H, W, *o, voxel,
                                                nx, ny, nz, trunc, bricks.data_ptr(), n, *[x.data_ptr() for x in vol], stream), "integrate")
    for x, key, words in zip(vol, ("tsdf", "weight", "rgb", "has_color"), (n * 512, n * 512, n * 1536, n * 512)):
        M.assert_bytes(x[:words].cpu().numpy(), want["volume"][key].ravel(), key)
        assert kept(x, words), key
    edge_mask, rank = full(n * 512, torch.uint8), full(n * 512, torch.int16)
    vc, tc, vo, to = full(n, torch.int32), full(n, torch.int32), full(n + 1, torch.int64), full(n + 1, torch.int64)
    _lib.check(lib.mvster_mesh_sparse_count(vol[0].data_ptr(), vol[1].data_ptr(), slot.data_ptr(), bricks.data_ptr(), n, nx, ny, nz, 1,
                                            edge_mask.data_ptr(), rank.data_ptr(), vc.data_ptr(), tc.data_ptr(), vo.data_ptr(),
                                            to.data_ptr(), stream), "mesh_sparse_count")
    nv, nt = int(vo[n].cpu()), int(to[n].cpu())
    assert (nv, nt) == (len(want["mesh"][0]), len(want["mesh"][2]))
    assert kept(edge_mask, n * 512) and kept(rank, n * 512) and kept(vc, n) and kept(tc, n) and kept(vo, n + 1) and kept(to, n + 1)
    vertices, colors, keys = full(nv, torch.float32, (3,)), full(nv, torch.uint8, (3,)), full(nv, torch.int64)
    triangles = full(nt, torch.int32, (3,))
    emit_v = lambda cap, ve, co, ke: _lib.check(lib.mvster_mesh_sparse_emit_vertices(
        vol[0].data_ptr(), vol[1].data_ptr(), vol[2].data_ptr(), vol[3].data_ptr(), slot.data_ptr(), bricks.data_ptr(), n, *o, voxel, nx, ny,
        nz, edge_mask.data_ptr(), rank.data_ptr(), vo.data_ptr(), cap, ve.data_ptr(), co.data_ptr(), ke.data_ptr(), stream), "emit_vertices")
    emit_t = lambda cap, tr: _lib.check(lib.mvster_mesh_sparse_emit_triangles(
        vol[0].data_ptr(), vol[1].data_ptr(), slot.data_ptr(), bricks.data_ptr(), n, nx, ny, nz, 1, edge_mask.data_ptr(), rank.data_ptr(),
        vo.data_ptr(), to.data_ptr(), nv, cap, tr.data_ptr(), stream), "emit_triangles")
    emit_v(nv, vertices, colors, keys)
    emit_t(nt, triangles)
    for x, w, cnt in ((vertices, want["mesh"][0], nv), (colors, want["mesh"][1], nv), (triangles, want["mesh"][2], nt), (keys, want["mesh"][3], nv)):
        M.assert_bytes(x[:cnt].cpu().numpy(), w)
        assert kept(x, cnt)
    # a capacity below the counts: the entries that fit are written, nothing else
    vertices, colors, keys = full(nv, torch.float32, (3,)), full(nv, torch.uint8, (3,)), full(nv, torch.int64)
    triangles = full(nt, torch.int32, (3,))
    emit_v(nv - 5, vertices, colors, keys)
    emit_t(nt - 5, triangles)
    M.assert_bytes(vertices[:nv - 5].cpu().numpy(), want["mesh"][0][:nv - 5])
    M.assert_bytes(triangles[:nt - 5].cpu().numpy(), want["mesh"][2][:nt - 5])
    assert kept(vertices, nv - 5) and kept(colors, nv - 5) and kept(keys, nv - 5) and kept(triangles, nt - 5)


# ---- the scan-level calls ----------------------------------------------------------------------------------------------------------------

def dense_with_keys(res):
    """A dense ``mesh_scene`` result -> (vertices, colors, triangles, keys): the keys come from the host build's owners of the
    result's own volume, whose mesh must be the result's"""
    vol = res["volume"]
    ve, co, tr, owners = M.extract_host(M.load_tsdf_hostmath(), *(getattr(vol, k).cpu().numpy() for k in ("tsdf", "weight", "rgb", "has_color")),
                                        vol.origin, vol.voxel_size, vol.dims, res["min_weight"])
    M.assert_bytes(res["vertices"].cpu().numpy(), ve, "dense vertices")
    M.assert_bytes(res["triangles"].cpu().numpy(), tr, "dense triangles")
    return ve, co, tr, S.dense_keys(owners)


def scene_bounds(c):
    lo = np.asarray(c["origin"]) + c["trunc"]
    return lo, np.asarray(c["origin"]) + c["voxel"] * (np.asarray(c["dims"]) - 1) - c["trunc"]


@pytest.mark.parametrize("name,s", [("sphere_views", 4), ("bad_depths", 3)])
def test_mesh_scene_sparse_equals_dense(name, s):
    c = S.refined(name, s)
    args = [c[k] for k in ("depths", "masks", "images", "Ks", "Es", "voxel")]
    kw = dict(bounds=scene_bounds(c), min_weight=1, device=DEV)
    dense = dict(mesh.mesh_scene(*args, **kw), min_weight=1)
    sparse = mesh.mesh_scene(*args, sparse=True, fill=FILL, **kw)
    vol = sparse["volume"]
    assert isinstance(vol, mesh.SparseTSDFVolume) and vol.dims == dense["volume"].dims and vol.origin == dense["volume"].origin
    print("%s x%d: %d of %d bricks, %d vertices, %d triangles" % (name, s, vol.n_bricks, vol.brick_slot.numel(), len(sparse["vertices"]),
                                                                  len(sparse["triangles"])))
    got = tuple(sparse[k].cpu().numpy() for k in ("vertices", "colors", "triangles", "vertex_key"))
    S.assert_canonically_equal(got, dense_with_keys(dense), (name, s))
    assert len(got[2]) > 0
    if name == "sphere_views":
        # the allocated bricks against the budget, after the allocation's read-back: the directory alone (2 240 bytes) fits
        with pytest.raises(RuntimeError, match="bricks of 8 x 8 x 8 nodes .* a voxel_size of about"):
            mesh.mesh_scene(*args, sparse=True, memory_budget=100000, **kw)
        cleaned = mesh.mesh_scene(*args, sparse=True, mesh_clean=mesh.MeshClean(True, 10, True, True), **kw)
        assert cleaned["clean_stats"]["components_kept"] == 1 and 0 < len(cleaned["triangles"]) <= len(got[2])
        assert len(cleaned["normals"]) == len(cleaned["vertices"]) == len(cleaned["vertex_key"])
        pos = dict(zip(got[3].tolist(), map(bytes, got[0])))
        assert all(pos[k] == bytes(v) for k, v in zip(cleaned["vertex_key"].cpu().numpy().tolist(), cleaned["vertices"].cpu().numpy()))


def test_an_empty_allocation_gives_three_empty_tensors():
    c = S.refined("sphere_views", 4)
    nothing = np.zeros_like(np.asarray(c["masks"]))
    slot, bricks = mesh.allocate_bricks(c["depths"], nothing, *(c[k] for k in ALLOC_KEYS[2:]), device=DEV)
    assert len(bricks) == 0 and int(slot.max()) == -1
    got = mesh.mesh_scene(c["depths"], nothing, c["images"], c["Ks"], c["Es"], c["voxel"], bounds=scene_bounds(c), min_weight=1, device=DEV,
                          sparse=True)
    assert got["volume"].n_bricks == 0
    for key, dtype in (("vertices", torch.float32), ("colors", torch.uint8), ("triangles", torch.int32)):
        assert tuple(got[key].shape) == (0, 3) and got[key].dtype == dtype and got[key].device.type == "cuda"
    assert tuple(got["vertex_key"].shape) == (0,)


def test_reconstruct_scan_with_a_sparse_mesh(shipped_cfg, checkpoint):
    """One synthetic scan of 7 views at 128 x 192: ``TSDFMesh(v, sparse=True)`` gives the mesh of ``sparse=False`` in canonical
    form, and the call without ``mesh=`` returns what it returned before"""
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
    dense = scan.reconstruct_scan(*args, mesh=fusion.TSDFMesh(voxel, None, 1), **kw)
    sparse = scan.reconstruct_scan(*args, mesh=fusion.TSDFMesh(voxel, None, 1, sparse=True), **kw)
    assert sorted(set(dense) - set(plain)) == ["mesh_colors", "mesh_triangles", "mesh_vertices", "mesh_volume"]
    assert sorted(set(sparse) - set(dense)) == ["mesh_vertex_key"]
    for k in plain:
        assert torch.equal(dense[k], plain[k]) and torch.equal(sparse[k], plain[k]), k
    assert sparse["mesh_volume"]["sparse"] is True and sparse["mesh_volume"]["dims"] == dense["mesh_volume"]["dims"]
    refs = np.asarray(dense.scan["ref_views"])
    images = torch.from_numpy(sc["images"]).to(DEV)[torch.from_numpy(refs).to(DEV)]
    again = dict(mesh.mesh_scene(dense["depth_est_averaged"].float(), dense["final_mask"], images, dense.scan["Ks"][refs],
                                 dense.scan["Es"][refs], voxel, None, (lo, hi), 1), min_weight=1)
    want = dense_with_keys(again)
    M.assert_bytes(dense["mesh_vertices"].cpu().numpy(), want[0], "the dense run's mesh")
    got = tuple(sparse["mesh_" + k].cpu().numpy() for k in ("vertices", "colors", "triangles", "vertex_key"))
    print("reconstruct_scan, sparse: %d of %d bricks, %d vertices, %d triangles" % (sparse["mesh_volume"]["bricks"],
                                                                                     sparse["mesh_volume"]["grid_bricks"], len(got[0]), len(got[2])))
    S.assert_canonically_equal(got, want, "reconstruct_scan")
    assert len(got[2]) > 0
