"""Reference views with fewer than ``nviews - 1`` sources on the GPU: the counted warp entries bit for bit against today's
entries on the first n sources (every launch form, mixed counts in one launch, unused slots never read), and
``infer_scan(..., short_sources="fewer_views")`` bit for bit against the per-sample forward on the shorter samples the Tanks
and Temples / ETH3D loaders build, on the capturing and on the replaying call.  Every comparison is exact: the arbiter runs
the same kernel on the same operands in the same order."""
import numpy as np
import pytest
import torch

from mvster_amd import MVS4net, _lib, formats, fusion, ops, scan
from mvster_amd.synthetic import make_inputs
from tests import scan_cases as SC
from tests import scan_dataset_cases as DC
from tests import scan_short_cases as SS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def model(shipped_cfg, checkpoint):
    m = MVS4net(**shipped_cfg)
    m.load_state_dict(checkpoint, strict=True)
    return m.to(DEV).eval()


# ---- the kernel ------------------------------------------------------------------------------------------------------------
# (C, G, D, group_cor, variant): the four shipped stages (wave-local kernel, truly indexed), a squared-difference volume and
# D = 32 (one thread per (pixel, d), 64- and 32-pixel workgroups), the lane-split form, and C = 16 on the one-thread form,
# which has no indexed instantiation: a gather and the PLAIN counted entry
FORMS = [(64, 8, 8, True, 0), (32, 8, 8, True, 0), (16, 4, 4, True, 0), (8, 4, 4, True, 0), (8, 8, 4, False, 0),
         (8, 4, 32, True, 0), (32, 8, 8, True, 2), (16, 4, 4, True, 1)]
SIZES = [(16, 20), (13, 19)]                                                 # 13 x 19 = 247 pixels: a partial last workgroup
V, NV = 6, 4
TABLE = [3, 1, 4, 0, 2]                                                      # reference view 3; view 5 of the store is all NaN


def _operands(C, D, h, w, B=1, seed=0):
    g = torch.Generator().manual_seed(C * 100 + D + h + seed)
    store = torch.randn(V, h, w, C, generator=g)
    store[5] = float("nan")
    _, proj, dv = make_inputs(nviews=NV + 1, H=h * 8, W=w * 8, batch=B, seed=D + seed, rotate=True)
    rt = ops.relative_projection(proj["stage1"].to(DEV))
    hypo = dv[:, :1, None, None] + (dv[:, -1:, None, None] - dv[:, :1, None, None]) * torch.rand(B, D, h, w, generator=g)
    return store.to(DEV), rt, hypo.to(DEV)


def _plain(store, table, rt, hypo, n, G, gc, fuse, variant):
    """Today's plain entry on the reference map and the first n sources of a row: the arbiter."""
    ref = store[table[0]][None].contiguous()
    src = store[table[1:1 + n]][:, None].contiguous()
    return ops.warp_agg_fwd_cl(ref, src, rt[:, :n].contiguous(), hypo, G, gc, fuse, 2.0, want_wsum=True, variant=variant)


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("C,G,D,gc,variant", FORMS)
def test_counted_warp_equals_the_plain_entry_on_the_first_n_sources(C, G, D, gc, variant, fuse, h, w):
    store, rt, hypo = _operands(C, D, h, w)
    table = torch.tensor(TABLE)
    gathered_ref = store[table[0]][None].contiguous()
    gathered_src = store[table[1:]][:, None].contiguous()
    for n in range(1, NV + 1):
        want, want_ws = _plain(store, table, rt, hypo, n, G, gc, fuse, variant)
        plain_kernel = _lib.last_kernel()
        assert not torch.isnan(want).any() and not torch.isnan(want_ws).any()
        got, got_ws = ops.warp_agg_fwd_indexed_cl(store, [TABLE], rt, hypo, G, gc, fuse, 2.0, want_wsum=True, variant=variant,
                                                  nsrc=[n])
        # the same kernel (its indexed instantiation, or the plain one after the gather), not merely the same numbers
        assert _lib.last_kernel().replace(", 0, true>", ">").replace(", true>", ">") == plain_kernel
        bad = int((got != want).sum()), int((got_ws != want_ws).sum())
        print("counted indexed (%d, %d, %d) variant %d fuse %d %dx%d n=%d: differing cor_feats %d, wsum %d"
              % (C, G, D, variant, fuse, h, w, n, bad[0], bad[1]))
        assert torch.equal(got, want) and torch.equal(got_ws, want_ws)
        # the plain counted entry on the full gathered batch
        got, got_ws = ops.warp_agg_fwd_cl(gathered_ref, gathered_src, rt, hypo, G, gc, fuse, 2.0, want_wsum=True,
                                          variant=variant, nsrc=[n])
        assert _lib.last_kernel() == plain_kernel
        assert torch.equal(got, want) and torch.equal(got_ws, want_ws)
        # counts already on the device are taken as they are
        dev_n = torch.tensor([n], dtype=torch.int32, device=DEV)
        assert torch.equal(ops.warp_agg_fwd_indexed_cl(store, [TABLE], rt, hypo, G, gc, fuse, 2.0, variant=variant, nsrc=dev_n),
                           want)
        # unused slots are never read: their rt rows are NaN, their table entries name the all-NaN view, and (plain entry)
        # their maps are NaN
        rt_nan = rt.clone()
        rt_nan[:, n:] = float("nan")
        table_nan = TABLE[:1 + n] + [5] * (NV - n)
        got, got_ws = ops.warp_agg_fwd_indexed_cl(store, [table_nan], rt_nan, hypo, G, gc, fuse, 2.0, want_wsum=True,
                                                  variant=variant, nsrc=[n])
        assert not torch.isnan(got).any() and not torch.isnan(got_ws).any()
        assert torch.equal(got, want) and torch.equal(got_ws, want_ws)
        src_nan = store[torch.tensor(table_nan[1:])][:, None].contiguous()
        got, got_ws = ops.warp_agg_fwd_cl(gathered_ref, src_nan, rt_nan, hypo, G, gc, fuse, 2.0, want_wsum=True, variant=variant,
                                          nsrc=[n])
        assert torch.equal(got, want) and torch.equal(got_ws, want_ws)


@pytest.mark.parametrize("C,G,D,gc,variant", FORMS)
def test_mixed_counts_in_one_launch(C, G, D, gc, variant):
    """B = 3 with counts [1, 4, 2]: row b equals the B = 1 plain call with its own n.  (The launch form follows from C, D and
    the variant, never from B: ``_lib.last_kernel()`` is compared with the B = 1 call's.)"""
    h, w = 13, 19
    counts = [1, 4, 2]
    tables = [[3, 1, 4, 0, 2], [0, 2, 2, 4, 1], [4, 0, 3, 1, 2]]
    store, rt, hypo = _operands(C, D, h, w, B=3, seed=7)
    got, got_ws = ops.warp_agg_fwd_indexed_cl(store, tables, rt, hypo, G, gc, True, 2.0, want_wsum=True, variant=variant,
                                              nsrc=counts)
    kernel = _lib.last_kernel()
    idx = torch.tensor(tables)
    ref = store[idx[:, 0]].contiguous()
    src = store[idx[:, 1:].t().reshape(-1)].view(NV, 3, h, w, C).contiguous()
    plain, plain_ws = ops.warp_agg_fwd_cl(ref, src, rt, hypo, G, gc, True, 2.0, want_wsum=True, variant=variant,
                                          nsrc=torch.tensor(counts, dtype=torch.int32))
    for b, n in enumerate(counts):
        want, want_ws = _plain(store, torch.tensor(tables[b]), rt[b:b + 1], hypo[b:b + 1].contiguous(), n, G, gc, True, variant)
        assert _lib.last_kernel() == kernel.replace(", 0, true>", ">").replace(", true>", ">")
        assert torch.equal(got[b:b + 1], want) and torch.equal(got_ws[b:b + 1], want_ws), b
        assert torch.equal(plain[b:b + 1], want) and torch.equal(plain_ws[b:b + 1], want_ws), b


def test_counted_warp_rejects_bad_counts():
    store = torch.zeros(3, 8, 8, 8, device=DEV)
    rt, hypo = torch.zeros(1, 2, 12, device=DEV), torch.ones(1, 4, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match=r"source count 3 \(row 0\)"):
        ops.warp_agg_fwd_indexed_cl(store, [[0, 1, 2]], rt, hypo, 4, nsrc=[3])
    with pytest.raises(RuntimeError, match=r"source count 0"):
        ops.warp_agg_fwd_cl(store[:1], store[1:][:, None].contiguous(), rt, hypo, 4, nsrc=[0])
    with pytest.raises(RuntimeError, match=r"\[B\] = \[1\]"):
        ops.warp_agg_fwd_indexed_cl(store, [[0, 1, 2]], rt, hypo, 4, nsrc=[1, 1])
    with pytest.raises(RuntimeError, match="int32"):
        ops.warp_agg_fwd_indexed_cl(store, [[0, 1, 2]], rt, hypo, 4, nsrc=torch.ones(1, dtype=torch.int64, device=DEV))


# ---- scans -----------------------------------------------------------------------------------------------------------------
def _forward(model, imgs, proj, dv):
    out = model([torch.from_numpy(np.ascontiguousarray(i)).to(DEV) for i in imgs],
                {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in proj.items()},
                torch.from_numpy(np.ascontiguousarray(dv)).to(DEV))
    return out["depth"][0].clone(), out["photometric_confidence"][0].clone()


def _forward_sample(model, sample):
    return _forward(model, [i[None] for i in sample["imgs"]], {k: v[None] for k, v in sample["proj_matrices"].items()},
                    sample["depth_values"][None])


def _fresh(model):
    """Drop the model's scan runner, the way ``scan._runner`` does when the scan shape changes: the next call captures."""
    hit = scan._RUNNERS.pop(model, None)
    if hit is not None:
        hit[1].instances.clear()


def _dataset_case(model, tmp_path_factory, which):
    root = str(tmp_path_factory.mktemp(which + "_short"))
    if which == "tanks":
        name, cams, neg, kw = "Family", "cams", None, dict(crop_rows=(28, 28))
        sc = DC.dataset_scan([(184, 128)] * 6, seed=31)
        load = lambda r, srcs: formats.load_tanks_sample(root, name, r, srcs, nviews=SS.NVIEWS)
    else:
        name, cams, neg, kw = "door", "cams_1", 1, dict(img_wh=(128, 128))
        sc = DC.dataset_scan([(150, 200), (141, 211), (256, 256), (150, 200), (141, 211), (256, 256)], seed=32, negative_min_view=3)
        load = lambda r, srcs: formats.load_eth3d_sample(root, name, r, srcs, nviews=SS.NVIEWS, img_wh=(128, 128))
    DC.write_dataset_folder(root, name, sc, SS.PAIRS, cams=cams)
    samples = [load(r, srcs) for r, srcs in SS.WITH_SOURCES]
    assert [len(s["imgs"]) - 1 for s in samples] == SS.COUNTS                # the loaders return the shorter samples
    return dict(root=root, name=name, dataset=which, kw=kw, all6=SS.decode_all(root, name, cams, neg, 6), samples=samples,
                maps=[_forward_sample(model, s) for s in samples])


@pytest.fixture(scope="module")
def tanks(model, tmp_path_factory):
    """6 views of 184x128 -> 128x128 on disk, with the per-sample maps of the five reference views that have sources."""
    return _dataset_case(model, tmp_path_factory, "tanks")


@pytest.fixture(scope="module")
def eth3d(model, tmp_path_factory):
    """6 views of three native sizes -> img_wh = (128, 128); view 3's cam file has a negative depth_min."""
    return _dataset_case(model, tmp_path_factory, "eth3d")


@pytest.mark.parametrize("which", ["tanks", "eth3d"])
def test_infer_scan_with_fewer_views_is_bit_equal_to_the_forward_on_the_loaders_shorter_samples(model, request, which):
    case = request.getfixturevalue(which)
    d = case["all6"]
    _fresh(model)
    report = {}
    for in_flight in (1, 2):
        for call in ("capture", "replay"):
            res = scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, nviews=SS.NVIEWS,
                                  in_flight=in_flight, depth_range_kind="min_max", short_sources="fewer_views", **case["kw"])
            torch.cuda.synchronize()
            assert res["stats"]["captured"] == (call == "capture")
            assert res["ref_views"].tolist() == [0, 1, 2, 3, 4]              # view 5 has no sources: no depth map
            assert res["stats"]["short_views"] == 2 and res["stats"]["replays"] == 5
            # two FPN runs over the six views, one batch of 2 (views 3, 4) and one of 3 (views 0, 1, 2) for the short samples
            assert res["stats"]["fpn_runs"] == 4 and res["stats"]["store_bytes"] == scan.store_bytes(6 + 2 + 3, 128, 128)
            assert res["depth"].shape == res["photometric_confidence"].shape == (5, 128, 128)
            bad_d = [int((res["depth"][r] != case["maps"][r][0]).sum()) for r in range(5)]
            bad_c = [int((res["photometric_confidence"][r] != case["maps"][r][1]).sum()) for r in range(5)]
            report["in_flight%d_%s" % (in_flight, call)] = (bad_d, bad_c)
            print("infer_scan fewer_views %s in_flight=%d %s: differing depth %s, confidence %s per view (counts %s) of %d"
                  % (which, in_flight, call, bad_d, bad_c, SS.COUNTS, 128 * 128))
    assert all(v == ([0] * 5, [0] * 5) for v in report.values()), report
    for r, sample in enumerate(case["samples"]):
        assert res["Ks"][r].tobytes() == sample["proj_matrices"]["stage4"][0, 1, :3, :3].tobytes()
        assert res["Es"][r].tobytes() == sample["proj_matrices"]["stage4"][0, 0].tobytes()
    # without the keyword the same scan is refused, as before
    with pytest.raises(RuntimeError, match="reference view 1 has 2 source views"):
        scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, nviews=SS.NVIEWS,
                        depth_range_kind="min_max", **case["kw"])


def test_dtu_mode_scan_with_fewer_views_and_with_padding(model):
    """The DTU loader's inputs: ``short_sources="fewer_views"`` gives the forward on the UNPADDED sample (which differs from
    ``general_eval4``'s padding), and without the keyword the padded sample still rules."""
    sc = SC.synthetic_scan(6, 128, 128, seed=33)
    args = (sc["Ks"], sc["Es"], sc["depth_ranges"], SS.PAIRS)
    padded = scan.plan_scan(*args, nviews=SS.NVIEWS)
    short = scan.plan_scan(*args, nviews=SS.NVIEWS, short_sources="fewer_views")
    want_padded, want_short = [], []
    for r in range(5):
        want_padded.append(_forward(model, *SC.sample_of(sc, padded, r)))
        cut = short._replace(view_table=[row[:1 + n] for row, n in zip(short.view_table, short.source_counts)])
        want_short.append(_forward(model, *SC.sample_of(sc, cut, r)))
    _fresh(model)
    for call in ("capture", "replay"):
        got = scan.infer_scan(model, sc["images"], *args, nviews=SS.NVIEWS, short_sources="fewer_views")
        assert got["stats"]["short_views"] == 2 and got["stats"]["captured"] == (call == "capture")
        for r in range(5):
            assert torch.equal(got["depth"][r], want_short[r][0]), (call, r)
            assert torch.equal(got["photometric_confidence"][r], want_short[r][1]), (call, r)
    got = scan.infer_scan(model, sc["images"], *args, nviews=SS.NVIEWS)
    assert got["stats"]["short_views"] == 0 and got["stats"]["captured"]     # another graph: the uncounted entries
    for r in range(5):
        assert torch.equal(got["depth"][r], want_padded[r][0]) and torch.equal(got["photometric_confidence"][r], want_padded[r][1]), r


def _prepared_u8(sample_img):
    """The pixels the reference writes to images/ (test_mvs4.py:262-264) for one prepared float image [3,H,W]."""
    return np.clip(np.transpose(sample_img, (1, 2, 0)) * np.float32(255), 0, 255).astype(np.uint8)


def test_reconstruct_scan_with_fewer_views_equals_fuse_scene_on_the_per_sample_maps(model, tanks):
    d = tanks["all6"]
    conf, thres_view = 0.05, 1                                               # (random weights: keep the masks non-trivial)
    depth = torch.stack([m[0] for m in tanks["maps"]])
    confidence = torch.stack([m[1] for m in tanks["maps"]])
    images = np.stack([_prepared_u8(s["imgs"][0]) for s in tanks["samples"]])
    Ks = np.stack([s["proj_matrices"]["stage4"][0, 1, :3, :3] for s in tanks["samples"]])
    Es = np.stack([s["proj_matrices"]["stage4"][0, 0] for s in tanks["samples"]])
    want = fusion.fuse_scene(depth, confidence, images, Ks, Es, SS.WITH_SOURCES, conf, thres_view, device=DEV)
    got = scan.reconstruct_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], SS.PAIRS, conf=conf,
                                thres_view=thres_view, nviews=SS.NVIEWS, depth_range_kind="min_max", crop_rows=(28, 28),
                                short_sources="fewer_views")
    n = len(got["points"])
    print("reconstruct_scan, fewer_views, Tanks-like: %d points of %d pixels" % (n, 5 * 128 * 128))
    assert 0 < n < 5 * 128 * 128 and n == len(want["points"])
    assert torch.equal(got["points"], want["points"]) and torch.equal(got["colors"], want["colors"])
    for k in ("photo_mask", "geo_mask", "final_mask"):
        assert torch.equal(got[k], want[k])
    assert got.scan["stats"]["short_views"] == 2


def test_folder_entry_with_fewer_views_equals_infer_scan_on_the_decoded_arrays(model, eth3d):
    d = scan.read_scan_folder(eth3d["root"], eth3d["name"], dataset="eth3d")
    assert d["view_ids"] == [0, 1, 2, 3, 4]                                  # (nobody lists view 5: it is not read)
    res = scan.infer_scan_folder(model, eth3d["root"], eth3d["name"], nviews=SS.NVIEWS, dataset="eth3d", img_wh=(128, 128),
                                 short_sources="fewer_views")
    direct = scan.infer_scan(model, d["images"], d["Ks"], d["Es"], d["depth_ranges"], d["pairs"], nviews=SS.NVIEWS,
                             depth_range_kind="min_max", view_ids=d["view_ids"], img_wh=(128, 128), short_sources="fewer_views")
    for k in ("depth", "photometric_confidence", "images"):
        assert torch.equal(res[k], direct[k]), k
    assert np.array_equal(res["Ks"], direct["Ks"]) and res["stats"]["short_views"] == direct["stats"]["short_views"] == 2
    for r in range(5):
        assert torch.equal(res["depth"][r], eth3d["maps"][r][0]) and torch.equal(res["photometric_confidence"][r], eth3d["maps"][r][1]), r
    with pytest.raises(RuntimeError, match="reference view 1 has 2 source views"):
        scan.infer_scan_folder(model, eth3d["root"], eth3d["name"], nviews=SS.NVIEWS, dataset="eth3d", img_wh=(128, 128))
