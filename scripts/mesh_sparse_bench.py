"""Times brick-sparse meshing on an MI355X beside the dense path of section 4.23, on the scene of
scripts/mesh_bench.py: 49 synthetic views of 512 x 640 (a unit sphere over a floor), one fixed box of 3.4 units a side.

  grids        --sides nodes per axis (default 256 and 512), trunc = 4 voxels: ``allocate_bricks``, ``integrate_tsdf_sparse`` (on
               the allocated bricks, the allocation not included) and ``extract_mesh_sparse`` apart, and beside them the dense
               ``integrate_tsdf`` / ``extract_mesh`` of the same grid in the same process.  HIP events around one call, warm,
               inputs on the GPU; median of --runs with the extremes.  Recorded: bricks allocated / bricks in the grid, the bytes
               held (``mesh.sparse_bytes``) beside the dense grid's, node-view steps per second of both integrations, mesh sizes,
               and whether the two meshes hold the same vertices (the sorted position bytes are compared).
  pixel        the grid whose voxel is one pixel of the maps at the least used depth (least depth / focal length), which the dense
               path refuses: the refusal's text is recorded, then the sparse path is timed the same way.
  --probes     the sparse integration again on the same bricks (a) with every mask byte 0: no depth or colour gather, and (b) on
               maps of 64 x 80 with K scaled by 1/8: as many gathers, all in cache -- section 4.23's probe, for the brick layout.

Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from mesh_bench import event_ms, sphere_scene, spread  # noqa: E402


def kernel_resources():
    """VGPRs / LDS / scratch of the kernels of geo_mesh_sparse.hip from the compiler's report, or None without hipcc."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(HERE, "..", "mvster_amd", "csrc", "geo_mesh_sparse.hip")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True)
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: \S*?\d+(sparse_\w+_kernel)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, label in (("vgprs", r" VGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out or None


def sorted_rows(x):
    a = x.cpu().numpy()
    return a[np.lexsort(a.T[::-1])].tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--sides", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--no-pixel", action="store_true")
    ap.add_argument("--probes", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_sparse.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 calls")
    if not torch.cuda.is_available():
        sys.exit("mesh_sparse_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import mesh
    dev = torch.device("cuda:0")
    V, H, W = args.views, 512, 640
    depths, masks, images, Ks, Es = sphere_scene(V, H, W, dev)
    lo, extent = -1.7, 3.4
    report = {"config": {"runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "views": V, "map": "%dx%d" % (H, W)},
              "unit": "ms between two HIP events around one call, warm, inputs on the GPU; median over the runs, lowest and highest beside it",
              "launches": {"allocate_bricks": 5, "integrate_tsdf_sparse": 1, "extract_mesh_sparse": 6,
                           "note": "allocation: memset, mark, flags, scan, one read-back, slots; extraction: nodes, cells, two scans, one "
                                   "read-back, the two emit kernels"},
              "kernel_resources": kernel_resources(), "sizes": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")

    def measure(name, side, dense):
        voxel = extent / (side - 1)
        origin, dims, trunc = (lo, lo, lo), (side, side, side), 4 * voxel
        entry = {"name": name, "side": side, "nodes": side ** 3, "voxel": voxel, "ms": {}}
        times, (slot, bricks) = event_ms(lambda: mesh.allocate_bricks(depths, masks, Ks, Es, origin, voxel, dims, trunc), args.runs, args.warmup)
        entry["ms"]["allocate_bricks"] = spread(times)
        n, grid = len(bricks), slot.numel()
        entry.update(bricks=n, grid_bricks=grid, brick_share=n / grid, sparse_bytes=mesh.sparse_bytes(n, grid),
                     dense_bytes=side ** 3 * mesh.NODE_BYTES)
        run = lambda: mesh.integrate_tsdf_sparse(depths, masks, images, Ks, Es, origin, voxel, dims, trunc, bricks=bricks)
        times, vol = event_ms(run, args.runs, args.warmup)
        entry["ms"]["integrate_tsdf_sparse_given_bricks"] = spread(times)
        entry["sparse_node_view_steps_per_s"] = n * 512 * V / (statistics.median(times) * 1e-3)
        entry["note_given_bricks"] = ("bricks= is checked on the host: the figure holds one copy of the brick list to the host and the "
                                      "directory's scatter in torch besides the kernel")
        if args.probes:
            small = (depths[:, ::8, ::8].contiguous(), masks[:, ::8, ::8].contiguous(), images[:, ::8, ::8].contiguous())
            Ksmall = [np.diag([1 / 8, 1 / 8, 1.0]) @ K for K in Ks]
            for form, probe in (("masks_zero", lambda: mesh.integrate_tsdf_sparse(depths, torch.zeros_like(masks), images, Ks, Es, origin,
                                                                                  voxel, dims, trunc, bricks=bricks)),
                                ("maps_64x80", lambda: mesh.integrate_tsdf_sparse(*small, Ksmall, Es, origin, voxel, dims, trunc,
                                                                                  bricks=bricks))):
                ptimes, pvol = event_ms(probe, args.runs, args.warmup)
                entry["ms"]["integrate_tsdf_sparse_probe_" + form] = spread(ptimes)
                del pvol
        times, m = event_ms(lambda: mesh.extract_mesh_sparse(vol, 2, keys=True), args.runs, args.warmup)
        entry["ms"]["extract_mesh_sparse_min_weight_2"] = spread(times)
        entry.update(vertices=len(m.vertices), triangles=len(m.triangles))
        print(json.dumps(entry, sort_keys=True), flush=True)
        if dense:
            times, dvol = event_ms(lambda: mesh.integrate_tsdf(depths, masks, images, Ks, Es, origin, voxel, dims, trunc), args.runs, args.warmup)
            entry["ms"]["dense_integrate_tsdf"] = spread(times)
            entry["dense_node_view_steps_per_s"] = side ** 3 * V / (statistics.median(times) * 1e-3)
            times, dm = event_ms(lambda: mesh.extract_mesh(dvol, 2), args.runs, args.warmup)
            entry["ms"]["dense_extract_mesh_min_weight_2"] = spread(times)
            entry.update(dense_vertices=len(dm.vertices), dense_triangles=len(dm.triangles),
                         same_vertices_as_dense=sorted_rows(dm.vertices) == sorted_rows(m.vertices))
            del dvol, dm
        else:
            try:
                mesh.grid_for_bounds("mesh_scene", (lo + trunc,) * 3, (lo + extent - trunc,) * 3, voxel, trunc)
                entry["dense_refused"] = None
            except RuntimeError as e:
                entry["dense_refused"] = str(e)
        del vol, m, slot, bricks
        torch.cuda.empty_cache()
        report["sizes"].append(entry)
        print(json.dumps(entry, sort_keys=True), flush=True)
        save()

    for side in args.sides:
        measure("grid_%d" % side, side, True)
    if not args.no_pixel:
        near = float(depths[masks].min())
        pixel = near / float(Ks[0][0][0])
        measure("voxel_is_a_pixel", int(np.ceil(extent / pixel)) + 1, False)
        report["sizes"][-1]["pixel"] = {"least_depth": near, "focal": float(Ks[0][0][0]), "pixel_size": pixel}
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
