"""Times cleaning an extracted mesh on an MI355X: ``mesh.clean_mesh`` as a whole and its parts, on the
meshes of scripts/mesh_bench.py (49 synthetic views of 512 x 640 fused into grids of --sides nodes per axis, default 256 and 512).

  parts        plan (weld, degenerate triangles, components, selection, the three scans and the ONE read-back), the same without
               the weld, emit (compaction), ``vertex_normals`` of the cleaned mesh, ``mesh_components`` of the raw triangle list.
               HIP events around one call, warm, inputs on the GPU; median of --runs with the lowest and the highest.  Every
               figure is that of the Python call, not of its kernels alone: the plan's includes the allocation of its scratch and
               outputs (from torch's caching allocator, warm) and its read-back (the events straddle it), the normals' the
               allocation of their rows.
  whole        ``clean_mesh`` with the defaults, with normals, and with ``min_triangles=15`` and normals.
  CPU          the same steps in NumPy (np.unique for the weld, np.add.at for the normals' sums) with
               ``scipy.sparse.csgraph.connected_components`` for the components if SciPy imports, NumPy label propagation
               otherwise; wall clock, once; the mesh read back first (not timed).  Its normals' sums have no fixed order and its
               components are vertex-connected like ours; the counts are compared, not the bytes.
  scan         ``scan.reconstruct_scan`` of the 49-view synthetic scan with ``mesh=`` alone and with
               ``mesh_clean=MeshClean(True, 15, False, True)`` beside it: wall clock to a synchronise, median of --runs, and
               the share of the wall time the step adds.

Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mesh_bench as MB  # noqa: E402


def kernel_resources():
    """VGPRs / LDS / scratch of the kernels of geo_mesh_clean.hip from the compiler's report, or None without hipcc."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "mvster_amd", "csrc", "geo_mesh_clean.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?\d+((?:clean|normals)_\w+_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, label in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def clean_cpu(v, t):
    """weld, degenerate triangles, components, compaction, area-weighted normals on the CPU -> (seconds per step, counts)"""
    s, t0 = {}, time.perf_counter()
    finite = np.isfinite(v).all(1)
    _, first, inverse = np.unique((v + np.float32(0)).view(np.uint32), axis=0, return_index=True, return_inverse=True)
    canon = np.where(finite, first[np.asarray(inverse).reshape(-1)], np.arange(len(v)))   # (np.unique's first index is the least)
    s["weld"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    c = canon[t]
    kept = (c[:, 0] != c[:, 1]) & (c[:, 0] != c[:, 2]) & (c[:, 1] != c[:, 2]) & finite[c].all(1)
    k = c[kept]
    s["degenerate"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(2 * len(k), np.int8), (np.r_[k[:, 0], k[:, 0]], np.r_[k[:, 1], k[:, 2]])), shape=(len(v), len(v)))
        _, lab = connected_components(g, directed=False)
        how = "scipy.sparse.csgraph.connected_components"
    except ImportError:
        lab = np.arange(len(v))
        while True:
            nxt = lab.copy()
            np.minimum.at(nxt, k.reshape(-1), np.repeat(lab[k].min(1), 3))
            nxt = nxt[nxt]
            if (nxt == lab).all():
                break
            lab = nxt
        how = "NumPy label propagation"
    used = np.zeros(len(v), bool)
    used[k.reshape(-1)] = True
    sizes = np.bincount(lab[k[:, 0]], minlength=lab.max() + 1)
    s["components"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    number = np.cumsum(used) - 1
    ov, ot = v[used], number[k]
    s["compaction"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    p = ov.astype(np.float64)
    n = np.cross(p[ot[:, 1]] - p[ot[:, 0]], p[ot[:, 2]] - p[ot[:, 0]])
    N = np.zeros_like(p)
    for a in range(3):
        np.add.at(N, ot[:, a], n)
    with np.errstate(all="ignore"):
        N /= np.linalg.norm(N, axis=1, keepdims=True)
    s["normals"] = time.perf_counter() - t0
    s["total"] = sum(s.values())
    return {a: round(b, 4) for a, b in s.items()}, dict(vertices=len(ov), triangles=len(ot), components=int((sizes > 0).sum()), components_by=how)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_clean.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("mesh_clean_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import fusion, mesh, scan
    dev = torch.device("cuda:0")
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "views": args.views},
              "unit": "ms between two HIP events around one call, warm, inputs on the GPU; median over the runs, lowest and highest "
                      "beside it; reconstruct_scan: wall clock to a synchronise; the CPU steps in seconds of wall clock, once",
              "launches": {"plan": 13, "plan_without_weld": 11, "emit": 1, "vertex_normals": 6,
                           "note": "plan: table, init, insert, canon, hook, flatten, count, scan, table rows, keep, two scans, number; "
                                   "one read-back (8 words); the scans run over one count per workgroup of 256"},
              "kernel_resources": kernel_resources(), "sizes": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")

    V, H, W = args.views, 512, 640
    depths, masks, images, Ks, Es = MB.sphere_scene(V, H, W, dev)
    lo, extent = -1.7, 3.4
    for side in args.sides:
        voxel = extent / (side - 1)
        vol = mesh.integrate_tsdf(depths, masks, images, Ks, Es, (lo, lo, lo), voxel, (side, side, side), 4 * voxel)
        m = mesh.extract_mesh(vol, 2)
        del vol
        torch.cuda.empty_cache()
        v, c, t = m.vertices, m.colors, m.triangles
        nv, nt = len(v), len(t)
        slots = mesh.clean_slots(nv)
        ms = {}
        times, plan = MB.event_ms(lambda: mesh._CleanPlan("bench", v, t, nv, True, 0, False, slots), args.runs, args.warmup)
        ms["plan"] = MB.spread(times)
        times, _ = MB.event_ms(lambda: mesh._CleanPlan("bench", v, t, nv, False, 0, False, slots), args.runs, args.warmup)
        ms["plan_without_weld"] = MB.spread(times)
        out = (torch.empty(plan.nv_out, 3, device=dev), torch.empty(plan.nv_out, 3, device=dev, dtype=torch.uint8),
               torch.empty(plan.nt_out, 3, device=dev, dtype=torch.int32), torch.empty(plan.nv_out, device=dev, dtype=torch.int64),
               torch.empty(plan.nt_out, device=dev, dtype=torch.int64))
        times, _ = MB.event_ms(lambda: plan.emit(c, *out), args.runs, args.warmup)
        ms["emit"] = MB.spread(times)
        times, _ = MB.event_ms(lambda: mesh.vertex_normals(out[0], out[2], _checked=True), args.runs, args.warmup)
        ms["vertex_normals_of_the_cleaned_mesh"] = MB.spread(times)
        times, _ = MB.event_ms(lambda: mesh.mesh_components(t, nv), args.runs, args.warmup)
        ms["mesh_components_with_its_range_check"] = MB.spread(times)
        times, r = MB.event_ms(lambda: mesh.clean_mesh(v, t, c), args.runs, args.warmup)
        ms["clean_mesh"] = MB.spread(times)
        times, _ = MB.event_ms(lambda: mesh.clean_mesh(v, t, c, _checked=True), args.runs, args.warmup)
        ms["clean_mesh_without_the_range_check"] = MB.spread(times)
        times, _ = MB.event_ms(lambda: mesh.clean_mesh(v, t, c, normals=True), args.runs, args.warmup)
        ms["clean_mesh_normals"] = MB.spread(times)
        times, r15 = MB.event_ms(lambda: mesh.clean_mesh(v, t, c, min_triangles=15, normals=True), args.runs, args.warmup)
        ms["clean_mesh_min_triangles_15_normals"] = MB.spread(times)
        entry = {"name": "grid_%d" % side, "vertices": nv, "triangles": nt, "ms": ms, "stats": r["stats"], "stats_min_triangles_15": r15["stats"],
                 "cleaned": {"vertices": len(r["vertices"]), "triangles": len(r["triangles"])},
                 "largest_valence": int(torch.bincount(r["triangles"].reshape(-1).long()).max()) if len(r["triangles"]) else 0}
        print(json.dumps(entry, sort_keys=True), flush=True)
        if not args.no_cpu:
            hv, ht = v.cpu().numpy(), t.cpu().numpy().astype(np.int64)
            entry["cpu_s"], entry["cpu_counts"] = clean_cpu(hv, ht)
            print(json.dumps({"cpu_s": entry["cpu_s"], "cpu_counts": entry["cpu_counts"]}, sort_keys=True), flush=True)
        report["sizes"].append(entry)
        save()
        del m, v, c, t, plan, out, r, r15
        torch.cuda.empty_cache()
    if not args.no_scan:
        from tests import scan_cases as SC
        model = MB.load_model(dev)
        sc = SC.synthetic_scan(V, 512, 640, seed=49)
        imgs = torch.from_numpy(sc["images"]).to(dev)
        call = (model, imgs, sc["Ks"], sc["Es"], sc["depth_ranges"], SC.ring_pairs(V, 10))
        kw = dict(conf=0.05, thres_view=1, nviews=5)                             # random weights: keep a cloud
        full = scan.reconstruct_scan(*call, **kw)
        p = full["points"]
        ext = float((p.amax(0) - p.amin(0)).max())
        del full
        clean = fusion.MeshClean(True, 15, False, True)
        entry = {"name": "scan", "scan": "%d views 512x640, nviews 5, 10 listed sources" % V, "ms": {}}
        for side in args.sides:
            spec = fusion.TSDFMesh(ext / (side - 1))
            t0, res0 = MB.wall_ms(lambda: scan.reconstruct_scan(*call, mesh=spec, **kw), args.runs)
            t1, res1 = MB.wall_ms(lambda: scan.reconstruct_scan(*call, mesh=spec, mesh_clean=clean, **kw), args.runs)
            a, b = statistics.median(t0), statistics.median(t1)
            entry["ms"]["reconstruct_scan_wall_mesh_extent_over_%d" % (side - 1)] = MB.spread(t0)
            entry["ms"]["reconstruct_scan_wall_mesh_clean_extent_over_%d" % (side - 1)] = MB.spread(t1)
            entry["extent_over_%d" % (side - 1)] = dict(vertices=len(res0["mesh_vertices"]), triangles=len(res0["mesh_triangles"]),
                                                       cleaned_vertices=len(res1["mesh_vertices"]),
                                                       cleaned_triangles=len(res1["mesh_triangles"]), stats=res1["mesh_clean_stats"],
                                                       added_ms=round(b - a, 4), share_of_wall_time=round((b - a) / b, 4))
            print(json.dumps(entry, sort_keys=True), flush=True)
            del res0, res1
        report["sizes"].append(entry)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
