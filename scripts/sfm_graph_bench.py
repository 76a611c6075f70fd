#!/usr/bin/env python3
"""The view graph of a structure-from-motion model (``mvster_amd.sfm``) on two synthetic models:

  small    about 300 views and 200 k points;
  large    about 2 000 views and 2 M points.

Cameras stand on three rings around the points; a point's track is a run of neighbouring views of one ring with gaps, its length
drawn log-uniformly from 2 .. --max-track (wide: most tracks are short, a few long ones carry most of the pairs).

Timed per model, the tables already on the GPU, between two HIP events around one call, warm, the median of --runs calls with the
lowest and the highest beside it: the three launches ``mvster_sfm_pair_scores`` (zero, scatter, mirror), ``mvster_sfm_depth_ranges``
and ``mvster_sfm_select_sources``; and ``sfm.view_graph`` by the wall clock (uploads, five launches, one read-back).  Against it
the same definition in NumPy on the CPU of the same box, once: all pairs of all tracks of one length at a time with ``arccos`` /
``exp`` and ``bincount``, a sort per view for the ranges, an argsort per row for the lists.  The differences between the two are
reported: |q_gpu - q_numpy| against the number of common points, ranges and counts, and the rows whose lists agree.  Writes one
JSON file (--out)."""
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

TWO32 = 4294967296.0


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "runs": len(xs)}


def event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def synthetic(V, P, max_track, seed):
    """-> the model dict ``sfm.view_graph`` takes (the fields it reads)"""
    from mvster_amd import sfm
    rng = np.random.RandomState(seed)
    rings = 3
    per = (V + rings - 1) // rings
    ring_of, slot_of = np.arange(V) % rings, np.arange(V) // rings
    ang = 2 * np.pi * slot_of / per + 0.2 * ring_of
    centres = np.stack([np.cos(ang) * (20.0 + 4.0 * ring_of), np.sin(ang) * (20.0 + 4.0 * ring_of), 2.0 + 3.0 * ring_of], 1)
    centres += 0.05 * rng.randn(V, 3)
    z = -centres / np.linalg.norm(centres, axis=1, keepdims=True)              # looking at the origin
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], 1)
    t = -np.einsum("vij,vj->vi", R, centres)
    points = (rng.rand(P, 3) - 0.5) * np.array([12.0, 12.0, 5.0])
    L = np.minimum(np.exp(rng.rand(P) * np.log(max_track / 2.0)) * 2.0, min(max_track, per)).astype(np.int64)
    ring, start = rng.randint(0, rings, P), rng.randint(0, per, P)
    k = np.arange(int(L.max() * 1.5) + 1)
    vo, po = [], []
    for lo in range(0, P, 200000):                                           # a run of 1.5 L neighbouring slots, L of them kept
        sl = slice(lo, min(P, lo + 200000))
        span = (L[sl] * 1.5).astype(np.int64)[:, None]
        keep = (k[None] < span) & (rng.rand(sl.stop - sl.start, len(k)) < 1 / 1.5)
        view = ((start[sl, None] + k[None]) % per) * rings + ring[sl, None]
        keep &= view < V
        pi, ki = np.nonzero(keep)
        vo.append(view[pi, ki])
        po.append(pi + lo)
    model = dict(image_ids=np.arange(V), point_ids=np.arange(P), centres=centres, points=points, R=R, tvecs=t)
    model.update(sfm.structure(np.concatenate(vo), np.concatenate(po), V, P))
    return model


def numpy_graph(model, num_src, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """-> (q uint64 [V,V], n, depth_min, depth_max, index [V,num_src], seconds per part)"""
    from mvster_amd import sfm
    V, P = len(model["centres"]), len(model["points"])
    secs = {}
    t0 = time.perf_counter()
    acc = np.zeros(V * V, np.float64)                                          # (sums of integers below 2^53: exact)
    lengths = np.diff(model["pt_ptr"])
    for L in np.unique(lengths[lengths >= 2]):
        pts = np.nonzero(lengths == L)[0]
        i, j = np.triu_indices(int(L), 1)
        step = max(1, 4000000 // len(i))
        for lo in range(0, len(pts), step):
            p = pts[lo:lo + step]
            views = model["pt_views"][model["pt_ptr"][p][:, None] + np.arange(L)[None]]          # [n,L]
            d = model["centres"][views] - model["points"][p][:, None]
            nn = (d * d).sum(2)
            cos = (d[:, i] * d[:, j]).sum(2) / np.sqrt(nn[:, i] * nn[:, j])
            theta = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
            sigma = np.where(theta <= theta0, sigma1, sigma2)
            term = np.floor(np.exp(-(theta - theta0) ** 2 / (2 * sigma ** 2)) * TWO32 + 0.5)
            acc += np.bincount((views[:, i].astype(np.int64) * V + views[:, j]).ravel(), weights=term.ravel(), minlength=V * V)
    q = acc.reshape(V, V).astype(np.uint64)
    q = q + q.T
    secs["pair_scores"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    rt = sfm.depth_rows(model)
    n, lo_, hi_ = np.zeros(V, np.int32), np.full(V, np.nan), np.full(V, np.nan)
    for v in range(V):
        x = model["points"][model["view_pts"][model["view_ptr"][v]:model["view_ptr"][v + 1]]]
        z = ((rt[v, 0] * x[:, 0] + rt[v, 1] * x[:, 1]) + rt[v, 2] * x[:, 2]) + rt[v, 3]
        z = np.sort(z[np.isfinite(z) & (z > 0)])
        n[v] = len(z)
        if len(z):
            lo_[v], hi_[v] = z[len(z) // 100], z[99 * len(z) // 100]
    secs["depth_ranges"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    order = np.argsort(-q.astype(np.float64), axis=1, kind="stable")[:, :num_src]
    index = np.where(np.take_along_axis(q, order, 1) > 0, order, -1).astype(np.int32)
    secs["select_sources"] = time.perf_counter() - t0
    return q, n, lo_, hi_, index, secs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfm_graph.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-track", type=int, default=40)
    ap.add_argument("--num-src", type=int, default=10)
    ap.add_argument("--models", default="small,large")
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy side")
    args = ap.parse_args()
    from mvster_amd import _lib, sfm
    lib = _lib.load()
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(0), "cpu_threads": torch.get_num_threads(), "num_src": args.num_src,
              "max_track": args.max_track, "models": {}}
    for name in args.models.split(","):
        V, P = {"small": (300, 200000), "large": (2000, 2000000)}[name]
        model = synthetic(V, P, args.max_track, seed=len(name))
        lengths = np.diff(model["pt_ptr"])
        item_ptr, total = sfm._items(model["pt_ptr"])
        entry = {"views": V, "points": P, "observations": int(len(model["view_pts"])), "terms": total,
                 "track_length": {"mean": round(float(lengths.mean()), 2), "median": int(np.median(lengths)), "max": int(lengths.max())},
                 "points_per_view": {"mean": round(float(np.diff(model["view_ptr"]).mean()), 1), "max": int(np.diff(model["view_ptr"]).max())}}
        print("%s: %d views, %d points, %d observations, %d terms" % (name, V, P, entry["observations"], total), flush=True)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        centres, points, rt = up(model["centres"], np.float64), up(model["points"], np.float64), up(sfm.depth_rows(model), np.float64)
        pt_ptr, pt_views, items = up(model["pt_ptr"], np.int64), up(model["pt_views"], np.int32), up(item_ptr, np.int64)
        view_ptr, view_pts = up(model["view_ptr"], np.int64), up(model["view_pts"], np.int32)
        q = torch.empty(V, V, device=dev, dtype=torch.int64)
        index = torch.empty(V, args.num_src, device=dev, dtype=torch.int32)
        value = torch.empty(V, args.num_src, device=dev, dtype=torch.int64)
        count, n = torch.empty(V, device=dev, dtype=torch.int32), torch.empty(V, device=dev, dtype=torch.int32)
        lo, hi = torch.empty(V, device=dev, dtype=torch.float64), torch.empty(V, device=dev, dtype=torch.float64)
        stream = torch.cuda.current_stream(dev).cuda_stream
        params = (5.0, 1.0, 10.0)
        gpu = {}
        gpu["pair_scores_ms"] = spread(event_ms(lambda: sfm._launch_pairs(lib, centres, points, pt_ptr, pt_views, items, total, params,
                                                                          q, stream), args.runs, args.warmup))
        gpu["depth_ranges_ms"] = spread(event_ms(lambda: _lib.check(lib.mvster_sfm_depth_ranges(
            rt.data_ptr(), V, points.data_ptr(), P, view_ptr.data_ptr(), view_pts.data_ptr(), view_pts.numel(), n.data_ptr(),
            lo.data_ptr(), hi.data_ptr(), stream), "depth_ranges"), args.runs, args.warmup))
        gpu["select_sources_ms"] = spread(event_ms(lambda: _lib.check(lib.mvster_sfm_select_sources(
            q.data_ptr(), V, args.num_src, index.data_ptr(), value.data_ptr(), count.data_ptr(), stream), "select"), args.runs,
            args.warmup))
        gpu["terms_per_second"] = round(total / (gpu["pair_scores_ms"]["median"] * 1e-3), 0)
        walls = []
        for _ in range(max(3, args.runs // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            graph = sfm.view_graph(model, num_src=args.num_src, device=dev)
            walls.append((time.perf_counter() - t0) * 1e3)
        gpu["view_graph_wall_ms"] = spread(walls)
        again = sfm.view_graph(model, num_src=args.num_src, device=dev)
        gpu["two_runs_same_bytes"] = all(graph[k].tobytes() == again[k].tobytes() for k in ("q", "src_index", "src_q", "depth_min", "depth_max"))
        entry["gpu"] = gpu
        print("  gpu: %s" % json.dumps(gpu), flush=True)
        if not args.no_cpu:
            qn, nn, lon, hin, idxn, secs = numpy_graph(model, args.num_src)
            diff = np.abs(graph["q"].astype(np.int64) - qn.astype(np.int64))
            entry["numpy_cpu_s"] = {k: round(v, 3) for k, v in secs.items()}
            entry["numpy_cpu_s"]["total"] = round(sum(secs.values()), 3)
            entry["against_numpy"] = {
                "max_abs_q_difference": int(diff.max()), "pairs_that_differ": int((diff > 0).sum() // 2),
                "pairs_with_a_score": int((qn > 0).sum() // 2),
                "n_equal": bool(np.array_equal(graph["n_obs"], nn)),
                "depth_ranges_equal_bytes": bool(graph["depth_min"].tobytes() == lon.tobytes() and graph["depth_max"].tobytes() == hin.tobytes()),
                "rows_with_equal_lists": int((graph["src_index"] == idxn).all(1).sum())}
            entry["speedup_launches"] = round(sum(secs.values()) * 1e3 / (gpu["pair_scores_ms"]["median"] + gpu["depth_ranges_ms"]["median"]
                                                                         + gpu["select_sources_ms"]["median"]), 1)
            entry["speedup_view_graph_wall"] = round(sum(secs.values()) * 1e3 / gpu["view_graph_wall_ms"]["median"], 1)
            print("  numpy: %s  %s" % (json.dumps(entry["numpy_cpu_s"]), json.dumps(entry["against_numpy"])), flush=True)
        report["models"][name] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
