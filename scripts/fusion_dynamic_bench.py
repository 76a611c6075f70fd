#!/usr/bin/env python3
"""Fusion of a Tanks-and-Temples-sized scan under the two rules of ``fusion.fuse_scene``: ``method="normal"`` (the fixed
thresholds; the kernel every earlier measurement of this project used, the baseline) and ``method="dynamic"`` (dynamic
consistency checking).  The scan is synthetic (``plane_depth_maps``: --views maps of --height x
--width, --sources source views each, noise and outliers) and sits on the GPU before the clock starts.

Protocol: both methods warmed up, then --runs rounds with the two methods alternating inside every round; per call the two
phases are timed with device events (``fuse_scene(events=...)``: "filter+scan" and "emit") and the whole call with the host
clock around a device synchronise; the figures are medians over the rounds.  The NumPy restatement of the dynamic rule
(tests/dynamic_fusion_cases.py) is timed on the CPU for one reference view and scaled to the scan: what a user without the
kernel runs today.  Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--conf", type=float, default=0.3)
    ap.add_argument("--thres-view", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU time of the NumPy restatement")
    ap.add_argument("--out", default=os.path.join("profiles", "dynamic_fusion.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: the median needs at least 5 runs")
    if not torch.cuda.is_available():
        sys.exit("fusion_dynamic_bench.py measures on an MI355X: no GPU here, nothing measured")
    from mvster_amd import fusion
    from mvster_amd.synthetic_scene import plane_depth_maps
    from tests import dynamic_fusion_cases as D
    from tests import fusion_scene_cases as C

    dev = torch.device("cuda:0")
    V, H, W = args.views, args.height, args.width
    depths, Ks, Es = plane_depth_maps(V, H, W, seed=9, noise=1e-3, outlier_frac=0.1)
    rng = np.random.RandomState(4)
    conf = rng.rand(V, H, W).astype(np.float32)
    images = rng.randint(0, 256, (V, H, W, 3)).astype(np.uint8)
    pairs = C.make_pairs(V, args.sources, args.sources, seed=6)
    on_gpu = [torch.from_numpy(a).to(dev) for a in (depths, conf, images)]

    def run(method, events=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fusion.fuse_scene(*on_gpu, Ks, Es, pairs, args.conf, args.thres_view, events=events, method=method)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    kept = {}
    for method in fusion.FUSION_METHODS:
        for _ in range(args.warmup):
            _, res = run(method)
        kept[method] = float(res["final_mask"].float().mean())
        del res
    phases = {m: {"filter+scan": [], "emit": [], "call_host_clock": []} for m in fusion.FUSION_METHODS}
    for _ in range(args.runs):
        for method in fusion.FUSION_METHODS:                        # alternating
            events = []
            wall, res = run(method, events)
            del res
            for name in ("filter+scan", "emit"):                    # summed over the chunks of the call (one, normally)
                phases[method][name].append(sum(e0.elapsed_time(e1) for n, e0, e1 in events if n == name))
            phases[method]["call_host_clock"].append(wall * 1e3)
    report = {"config": {"views": V, "height": H, "width": W, "sources": args.sources, "conf_thres": args.conf,
                         "thres_view": args.thres_view, "pix_base": fusion.PIX_BASE, "rel_base": fusion.REL_BASE,
                         "runs": args.runs, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
              "unit": "ms (median over the runs; filter+scan and emit from device events, call_host_clock around a "
                      "device synchronise, inputs already on the GPU)",
              "pixel_views": V * H * W * args.sources, "kept_fraction": kept, "method": {}}
    for method, p in phases.items():
        report["method"][method] = {"median_ms": {k: round(statistics.median(v), 3) for k, v in p.items()},
                                    "runs_ms": {k: [round(x, 3) for x in v] for k, v in p.items()}}
    med = {m: report["method"][m]["median_ms"]["filter+scan"] for m in phases}
    report["dynamic_over_normal_filter_scan"] = round(med["dynamic"] / med["normal"], 3)
    if not args.no_cpu:
        r, srcs = pairs[0]
        t0 = time.perf_counter()
        D.dynamic_reference_view(depths[r], Ks[r], Es[r], conf[r], depths[srcs], Ks[srcs], Es[srcs], args.conf,
                                 args.thres_view, ref_img=images[r].astype(np.float32) / np.float32(255.0))
        one = time.perf_counter() - t0
        report["numpy_restatement_cpu"] = {"one_reference_view_s": round(one, 3), "scaled_to_the_scan_s": round(one * V, 2),
                                           "note": "one reference view timed once, times the number of reference views"}
    print(json.dumps(report, sort_keys=True), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
