"""Times meshing a scan on an MI355X: ``mesh.integrate_tsdf`` and ``mesh.extract_mesh`` apart, and
``scan.reconstruct_scan`` end to end with and without ``mesh=``.

  integrate / extract   49 synthetic views of 512 x 640 (analytic ray-sphere z-depths over a far plane, seeded images) into
                        grids of --sides nodes per axis (default 256 and 512) over one fixed box; trunc = 4 voxels.  HIP events
                        around one call, warm, inputs on the GPU; median of --runs.  For the integration also: node-view steps
                        per second, the depth samples it read per second (node-view pairs that reach the depth map: counted by the
                        torch restatement), and the floor of the bytes it must move at the HBM peak; the fp64-rate instructions
                        of a step are read off the compiled kernel (DESIGN.md has the tally), so that the bound can be named.
  torch restatement     the same integration in torch float64 tensor ops on the same GPU, a launch per operation, timed once per
                        side; the share of nodes whose tsdf has the kernel's bits is reported, not asserted.
  NumPy baseline        ``tests/mesh_cases.integrate_numpy`` / ``extract_numpy`` (vectorised; the triangles in a Python loop over
                        the cells the surface cuts) on the CPU at --cpu-side nodes per axis (default 64, a size that finishes),
                        wall clock, once.  The 256 / 512 figures beside it are EXTRAPOLATED by the node count and say so.
  scan                  ``scan.reconstruct_scan`` of a 49-view 512 x 640 synthetic scan (the golden checkpoint), wall clock to a
                        synchronise, median of --runs: plain, and with ``mesh=TSDFMesh(extent / 255)`` and ``extent / 511``.
  --probes              the integration again (a) with every mask byte 0: no depth or colour gather, and (b) on maps of 64 x 80
                        with K scaled by 1/8: the same arithmetic and as many gathers, all in cache -- to name what bounds it.
  --default-only        only the plain ``reconstruct_scan`` figure, importing nothing of the mesh: the same script runs on the
                        parent commit, for the record that the default path did not change.

Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12                         # bytes / s (spec)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def event_ms(fn, runs, warmup):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times, out


def sphere_scene(V, H, W, dev):
    """V cameras on a Fibonacci sphere of radius 3 around a unit sphere in front of the plane z = -1.6 as seen from above, built
    on the GPU -> depths [V,H,W] float32, masks, images uint8, Ks, Es (NumPy float64)"""
    from tests import mesh_cases as M
    K = np.array([[1.1 * W, 0, W / 2 - 0.3], [0, 1.1 * W, H / 2 + 0.2], [0, 0, 1.0]])
    Es = []
    for v in range(V):
        z = 0.15 + 0.8 * (v + 0.5) / V                                          # the upper half: every view sees the floor
        phi = v * np.pi * (3 - np.sqrt(5))
        r = np.sqrt(1 - z * z)
        Es.append(M.look_at(3.0 * np.array([r * np.cos(phi), r * np.sin(phi), z]), (0, 0, 0)))
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    pix = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W, device=dev, dtype=torch.float64)])
    depths = []
    for E in Es:
        rays = torch.linalg.solve(torch.from_numpy(K).to(dev), pix)              # z component 1
        R, t = torch.from_numpy(E[:3, :3]).to(dev), torch.from_numpy(E[:3, 3]).to(dev)
        cc = t                                                                  # the sphere's centre is the origin
        a, b = (rays * rays).sum(0), rays.T @ cc
        disc = b * b - a * (cc @ cc - 1.0)
        s = (b - disc.clamp(min=0).sqrt()) / a
        n = R[:, 2]                                                             # world z axis in camera coordinates
        floor = (-1.6 + n @ t) / (rays.T @ n)                                   # n . (s ray - t) = -1.6: world z
        d = torch.where(disc >= 0, s, torch.where(floor > 0, floor, torch.zeros_like(floor)))
        depths.append(d.reshape(H, W).float())
    g = torch.Generator(device=dev).manual_seed(49)
    images = torch.randint(0, 256, (V, H, W, 3), device=dev, generator=g, dtype=torch.uint8)
    depths = torch.stack(depths)
    return depths, depths > 0, images, [K] * V, Es


def integrate_torch(depths, masks, images, Ks, Es, origin, voxel, dims, trunc):
    """The definition in torch float64 tensor ops on the GPU, a view at a time -> (tsdf float32 [nz,ny,nx], samples read)"""
    dev = depths.device
    nx, ny, nz = dims
    ax = [origin[a] + voxel * torch.arange(n, device=dev, dtype=torch.float64) for a, n in enumerate(dims)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    sum_f = torch.zeros(nz, ny, nx, device=dev, dtype=torch.float64)
    w = torch.zeros(nz, ny, nx, device=dev, dtype=torch.int32)
    reads = 0
    V, H, W = depths.shape
    for v in range(V):
        K, E = np.asarray(Ks[v], np.float64).tolist(), np.asarray(Es[v], np.float64).tolist()      # Python floats
        c = [((E[a][0] * x + E[a][1] * y) + E[a][2] * z) + E[a][3] for a in range(3)]
        u = ((K[0][0] * c[0] + K[0][1] * c[1]) + K[0][2] * c[2]) / c[2] + 0.5
        t = ((K[1][0] * c[0] + K[1][1] * c[1]) + K[1][2] * c[2]) / c[2] + 0.5
        ok = (c[2] > 0) & (u >= 0) & (u < W) & (t >= 0) & (t < H)
        at = torch.where(ok, t.long() * W + u.long(), torch.zeros((), device=dev, dtype=torch.long))
        ok &= masks[v].reshape(-1)[at]
        reads += int(ok.sum())
        d = depths[v].reshape(-1)[at]
        ok &= torch.isfinite(d) & (d > 0)
        sdf = d.double() - c[2]
        ok &= ~(sdf < -trunc)
        f = (sdf / trunc).clamp(max=1.0)
        sum_f = torch.where(ok, sum_f + f, sum_f)
        w += ok
    return torch.where(w > 0, sum_f / w.clamp(min=1), torch.ones((), device=dev, dtype=torch.float64)).float(), reads


def kernel_resources():
    """VGPRs / LDS / scratch of the kernels of geo_mesh.hip from the compiler's report, or None without hipcc."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "mvster_amd", "csrc", "geo_mesh.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?\d+((?:tsdf|mesh)_\w+_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, label in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def load_model(dev):
    from mvster_amd import MVS4net
    cfg = dict(arch_mode="fpn", reg_net="reg2d", num_stage=4, fpn_base_channel=8, reg_channel=8, stage_splits=[8, 8, 4, 4],
               depth_interals_ratio=[0.5, 0.5, 0.5, 1], group_cor=True, group_cor_dim=[8, 8, 4, 4], inverse_depth=True,
               mono=True, attn_temp=2, attn_fuse_d=True)
    z = np.load(os.path.join(ROOT, "tests", "golden", "g7_checkpoint.npz"))
    model = MVS4net(**cfg)
    model.load_state_dict({k: torch.from_numpy(z[k]) for k in z.keys()}, strict=True)
    return model.to(dev).eval()


def wall_ms(fn, runs):
    fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--cpu-side", type=int, default=64)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--probes", action="store_true", help="also time the integration without gathers and with cache-resident maps")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("mesh_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import scan
    dev = torch.device("cuda:0")
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "views": args.views},
              "unit": "ms between two HIP events around one call, warm, inputs on the GPU; median over the runs, lowest and highest "
                      "beside it; reconstruct_scan: wall clock to a synchronise; CPU baselines in seconds of wall clock, once",
              "launches": {"integrate_tsdf": 1, "extract_mesh": 6,
                           "note": "mvster_mesh_count 4 (nodes, cells, two scans), one read-back, the two emit kernels"},
              "kernel_resources": None if args.default_only else kernel_resources(), "sizes": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")

    if not args.no_scan or args.default_only:
        from tests import scan_cases as SC
        model = load_model(dev)
        SV = args.views
        sc = SC.synthetic_scan(SV, 512, 640, seed=49)
        images = torch.from_numpy(sc["images"]).to(dev)
        call = (model, images, sc["Ks"], sc["Es"], sc["depth_ranges"], SC.ring_pairs(SV, 10))
        kw = dict(conf=0.05, thres_view=1, nviews=5)                             # random weights: keep a cloud
        times, full = wall_ms(lambda: scan.reconstruct_scan(*call, **kw), args.runs)
        entry = {"name": "scan", "scan": "%d views 512x640, nviews 5, 10 listed sources" % SV, "points": len(full["points"]),
                 "ms": {"reconstruct_scan_wall_plain": spread(times)}}
        print(json.dumps(entry, sort_keys=True), flush=True)
        if not args.default_only:
            from mvster_amd import fusion
            p = full["points"]
            extent = float((p.amax(0) - p.amin(0)).max())
            for side in args.sides:
                spec = fusion.TSDFMesh(extent / (side - 1))
                try:
                    times, res = wall_ms(lambda: scan.reconstruct_scan(*call, mesh=spec, **kw), args.runs)
                except RuntimeError as e:                                       # (a volume above the memory budget: recorded, not hidden)
                    entry["mesh_extent_over_%d" % (side - 1)] = {"refused": str(e)}
                    continue
                entry["ms"]["reconstruct_scan_wall_mesh_extent_over_%d" % (side - 1)] = spread(times)
                entry["mesh_extent_over_%d" % (side - 1)] = dict(dims=res["mesh_volume"]["dims"], vertices=len(res["mesh_vertices"]),
                                                                triangles=len(res["mesh_triangles"]))
                print(json.dumps(entry, sort_keys=True), flush=True)
                del res
        report["sizes"].append(entry)
        save()
        del full
        torch.cuda.empty_cache()
    if args.default_only:
        print("wrote", args.out)
        return

    from mvster_amd import mesh
    from tests import mesh_cases as M
    V, H, W = args.views, 512, 640
    depths, masks, images, Ks, Es = sphere_scene(V, H, W, dev)
    lo, extent = -1.7, 3.4
    for side in args.sides:
        voxel = extent / (side - 1)
        origin, dims, trunc = (lo, lo, lo), (side, side, side), 4 * voxel
        nodes = side ** 3
        run = lambda: mesh.integrate_tsdf(depths, masks, images, Ks, Es, origin, voxel, dims, trunc)
        times, vol = event_ms(run, args.runs, args.warmup)
        ms = statistics.median(times)
        entry = {"name": "grid_%d" % side, "nodes": nodes, "views": V, "map": "%dx%d" % (H, W), "voxel": voxel,
                 "ms": {"integrate_tsdf": spread(times)}, "node_view_steps_per_s": nodes * V / (ms * 1e-3),
                 "counted_node_views": int(vol.weight.sum(dtype=torch.int64))}
        must = depths.numel() * 8 + nodes * 12
        entry["floors_ms"] = {"bytes_at_hbm_peak": round(must / HBM_PEAK * 1e3, 4), "bytes": must,
                              "note": "every input byte once (depth 4, mask 1, colour 3 a pixel) and every output byte once"}
        if args.probes:
            # what bounds it: (a) every mask byte 0 -- no depth or colour gather, the arithmetic up to the mask read stays; (b) maps
            # of 64 x 80 with K scaled by 1/8 -- the same arithmetic and as many gathers, all of them in cache
            small = (depths[:, ::8, ::8].contiguous(), masks[:, ::8, ::8].contiguous(), images[:, ::8, ::8].contiguous())
            Ksmall = [np.diag([1 / 8, 1 / 8, 1.0]) @ K for K in Ks]
            for form, probe in (("masks_zero", lambda: mesh.integrate_tsdf(depths, torch.zeros_like(masks), images, Ks, Es, origin, voxel,
                                                                           dims, trunc)),
                                ("maps_64x80", lambda: mesh.integrate_tsdf(*small, Ksmall, Es, origin, voxel, dims, trunc))):
                ptimes, pvol = event_ms(probe, args.runs, args.warmup)
                entry["ms"]["integrate_tsdf_probe_" + form] = spread(ptimes)
                del pvol
        times, m = event_ms(lambda: mesh.extract_mesh(vol, 2), args.runs, args.warmup)
        entry["ms"]["extract_mesh_min_weight_2"] = spread(times)
        entry.update(vertices=len(m.vertices), triangles=len(m.triangles))
        print(json.dumps(entry, sort_keys=True), flush=True)
        if not args.no_torch:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref, reads = integrate_torch(depths, masks, images, Ks, Es, origin, voxel, dims, trunc)
            torch.cuda.synchronize()
            entry["torch_ops_s"] = round(time.perf_counter() - t0, 3)
            entry["depth_samples_read"] = reads
            entry["depth_samples_read_per_s"] = reads / (ms * 1e-3)
            entry["torch_ops_share_of_nodes_with_the_kernels_tsdf_bits"] = float((ref.view(torch.int32) == vol.tsdf.view(torch.int32)).double().mean())
            del ref
        del vol, m
        torch.cuda.empty_cache()
        report["sizes"].append(entry)
        print(json.dumps(entry, sort_keys=True), flush=True)
        save()
    if not args.no_cpu:
        side = args.cpu_side
        voxel = extent / (side - 1)
        origin, dims, trunc = (lo, lo, lo), (side, side, side), 4 * voxel
        host = [depths.cpu().numpy(), masks.cpu().numpy(), images.cpu().numpy()]
        t0 = time.perf_counter()
        vol = M.integrate_numpy(*host, Ks, Es, origin, voxel, dims, trunc)
        t1 = time.perf_counter()
        got = M.extract_numpy(*vol, origin, voxel, dims, 2)
        t2 = time.perf_counter()
        gpu = mesh.integrate_tsdf(depths, masks, images, Ks, Es, origin, voxel, dims, trunc)
        gm = mesh.extract_mesh(gpu, 2)
        entry = {"name": "numpy_cpu_%d" % side, "nodes": side ** 3, "cpu_s": {"integrate_numpy": round(t1 - t0, 3),
                                                                              "extract_numpy": round(t2 - t1, 3)},
                 "vertices": len(got[0]), "triangles": len(got[2]),
                 "equal_bytes": {"tsdf": bool(np.array_equal(vol[0].view(np.int32), gpu.tsdf.cpu().numpy().view(np.int32))),
                                 "vertices": got[0].tobytes() == gm.vertices.cpu().numpy().tobytes(),
                                 "triangles": got[2].tobytes() == gm.triangles.cpu().numpy().tobytes()},
                 "integrate_numpy_extrapolated_s": {str(s): round((t1 - t0) * (s / side) ** 3, 1) for s in args.sides},
                 "note": "integration extrapolated by the node count (the work per node does not depend on the grid); the "
                         "extraction is not extrapolated: its Python loop grows with the surface, not the volume"}
        report["sizes"].append(entry)
        print(json.dumps(entry, sort_keys=True), flush=True)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
