#!/usr/bin/env python3
"""What the training step's summary costs, at the shipped configuration (512x640, 5 views, batch 2 per GPU):
  (a) default_path   ``python bench.py --mode train`` of THIS tree against the same command in a checkout of the parent commit
                     (``--parent-dir``, built there), as alternating child processes: ms per step of every run, the medians
                     and the run-to-run spread.  The default path is unchanged code: the two must agree within the spread.
  (b) summary        ``GraphedTrainStep(summary=True)`` against ``summary=False`` in this process: launches added per step
                     (kernel nodes of the two captured graphs), time added, peak memory added (allocator peaks over construction, warm-up and
                     replays of either, each measured from an emptied cache, and what stays reserved afterwards).
  (c) today          what gives the same 17 numbers without the keyword: the step issued eagerly with the reference's
                     boolean-gather metrics and 17 ``.item()`` (``eager_gather_items``), or the captured step followed by a
                     second training-mode forward under ``no_grad`` for the loss terms and the metrics
                     (``captured_plus_second_forward``); steps per second of each against (b).
Protocol of (b) and (c): every variant its own model and optimizer from the same weights, warmed up, then WINDOWS windows of
STEPS steps per variant, the variants alternating inside every round, a window timed with the host clock around work that
ends in a device synchronise; the figure is the median window.  Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch  # noqa: E402

LOSS_KW = dict(stage_lw=[1, 1, 1, 1], l1ot_lw=[0, 1], inverse_depth=True, ot_iter=10, ot_eps=1, ot_continous=False, mono=True)


def gather_metrics(depth_est, depth_gt, mask):
    """The reference's four metrics written as it writes them: per image, boolean-mask gathers, fp32 means."""
    abs_err, thres = [], {2: [], 4: [], 8: []}
    for i in range(depth_gt.shape[0]):
        e = (depth_est[i][mask[i]] - depth_gt[i][mask[i]]).abs()
        abs_err.append(e.mean())
        for t in thres:
            thres[t].append((e > t).float().mean())
    return [torch.stack(abs_err).mean()] + [torch.stack(v).mean() for v in thres.values()]


def bench_child(tree, args):
    """One ``bench.py --mode train`` in a fresh process with ``tree`` as its working directory -> ms per step."""
    cmd = [sys.executable, "bench.py", "--mode", "train", "--gpus", "1", "--steps", str(args.bench_steps), "--warmup",
           str(args.bench_warmup), "--height", str(args.height), "--width", str(args.width), "--views", str(args.views)]
    out = subprocess.run(cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    return float(line["ms_per_step"])


def spread(xs):
    return round(max(xs) - min(xs), 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-dir", default=None, help="a built checkout of the parent commit: (a) alternates with it")
    ap.add_argument("--bench-runs", type=int, default=3, help="(a): child runs per tree")
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "train_summary.json"))
    args = ap.parse_args()
    if args.windows < 3:
        ap.error("--windows: the median needs at least 3 windows")
    if not torch.cuda.is_available():
        sys.exit("train_summary_bench.py measures on an MI355X: no GPU here, nothing measured")
    report = {"config": {"height": args.height, "width": args.width, "views": args.views, "batch": args.batch,
                         "windows": args.windows, "steps_per_window": args.steps, "warmup": args.warmup,
                         "device": torch.cuda.get_device_name(0)}}

    # ---- (a): child processes, before this process holds much of the device ----------------------------------------------
    trees = {"this_tree": ROOT}
    if args.parent_dir:
        trees["parent_commit"] = args.parent_dir
    runs = {k: [] for k in trees}
    for _ in range(args.bench_runs):
        for name, tree in trees.items():                       # alternating
            runs[name].append(bench_child(tree, args))
            print("(a) %s: %.4f ms per step" % (name, runs[name][-1]), flush=True)
    if not args.bench_runs:
        runs = {k: [float("nan")] for k in trees}
    a = {"command": "python bench.py --mode train --gpus 1 --steps %d --warmup %d" % (args.bench_steps, args.bench_warmup),
         "ms_per_step_runs": runs, "ms_per_step_median": {k: round(statistics.median(v), 4) for k, v in runs.items()},
         "run_to_run_spread_ms": {k: spread(v) for k, v in runs.items()}}
    if args.parent_dir:
        diff = a["ms_per_step_median"]["this_tree"] - a["ms_per_step_median"]["parent_commit"]
        a["median_difference_ms"] = round(diff, 4)
        a["within_spread"] = bool(abs(diff) <= max(a["run_to_run_spread_ms"].values()))
    else:
        a["note"] = "no --parent-dir: the parent commit was not measured"
    report["default_path"] = a

    # ---- (b), (c) ------------------------------------------------------------------------------------------------------
    from bench import SHIPPED, load_weights
    from mvster_amd import SCALAR_NAMES, MVS4net, MVS4net_loss
    from mvster_amd.graph import GraphedTrainStep
    from mvster_amd.optim import FusedAdam
    from mvster_amd.synthetic import make_inputs

    dev = torch.device("cuda:0")
    H, W, N, B = args.height, args.width, args.views, args.batch
    imgs, proj, dv = make_inputs(nviews=N, H=H, W=W, seed=100, device=dev, batch=B)
    g = torch.Generator().manual_seed(0)
    gt, mask = {}, {}
    for s in range(1, 5):
        hs, ws = H // 2 ** (4 - s), W // 2 ** (4 - s)
        gt["stage%d" % s] = (500 + 300 * torch.rand(B, hs, ws, generator=g)).to(dev)
        mask["stage%d" % s] = (torch.rand(B, hs, ws, generator=g) > 0.2).float().to(dev)
    weights = load_weights()

    def loss_fn(o, g_, m_):
        return MVS4net_loss(o, g_, m_, **LOSS_KW)

    def build(**kw):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base_a, base_r = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        model = MVS4net(**SHIPPED)
        model.load_state_dict(weights, strict=True)
        model.to(dev).train()
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        step = GraphedTrainStep(model, opt, loss_fn, imgs, proj, dv, gt, mask, warmup=3, **kw)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        mem = {"peak_allocated_MiB": round((torch.cuda.max_memory_allocated() - base_a) / 2 ** 20, 2),
               "peak_reserved_MiB": round((torch.cuda.max_memory_reserved() - base_r) / 2 ** 20, 2)}
        torch.cuda.empty_cache()           # what stays reserved now: the model, the optimizer state and the graph's private pool
        mem["held_reserved_MiB"] = round((torch.cuda.memory_reserved() - base_r) / 2 ** 20, 2)
        return model, step, mem

    first = build()                        # (thrown away: one-time allocations of the process stay out of the comparison)
    del first
    _, plain, mem_plain = build()
    _, summ, mem_summ = build(summary=True)
    _, eager, _ = build(capture=False)
    model2, captured2, _ = build()

    def scalars_to_host(out, res):
        metrics = gather_metrics(out["depth"].detach(), gt["stage4"], mask["stage4"] > 0.5)
        vals = [res[0]] + list(res[1]) + list(res[2]) + list(res[3]) + metrics
        return {k: v.item() for k, v in zip(SCALAR_NAMES, vals)}

    def eager_gather_items():
        """train_sample as the reference runs it: eager launches, gather metrics, 17 .item()."""
        model, opt = eager.model, eager.optimizer
        opt.zero_grad(set_to_none=True)
        out = model(imgs, proj, dv)
        res = loss_fn(out, gt, mask)
        res[0].backward()
        opt.step()
        return scalars_to_host(out, res)

    def captured_plus_second_forward():
        captured2()
        with torch.no_grad():
            out = model2(imgs, proj, dv)
            return scalars_to_host(out, loss_fn(out, gt, mask))

    variants = {"captured": plain, "captured_summary": summ, "eager_gather_items": eager_gather_items,
                "captured_plus_second_forward": captured_plus_second_forward}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.windows):
        for name, fn in variants.items():                      # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    summ.summary_reset()
    summ()
    row = summ.summary_mean()

    # launches of one step: the kernel nodes of the captured graph (graphs kept for the question, built for it alone)
    launches, note = {}, None
    try:
        from mvster_amd.graph import graph_kernel_nodes
        del plain, captured2
        kept = torch.cuda.CUDAGraph
        torch.cuda.CUDAGraph = lambda *a, **k: kept(keep_graph=True)
        try:
            for name, kw in (("summary_false", {}), ("summary_true", {"summary": True})):
                _, st, _ = build(**kw)
                launches[name] = graph_kernel_nodes(st.graph)[0]
                del st
        finally:
            torch.cuda.CUDAGraph = kept
    except Exception as e:                                       # (the figure is then missing from the file, and says why)
        note = "%s: %s" % (type(e).__name__, str(e)[:200])
    report["summary"] = {
        "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
        "ms_per_step_windows": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "window_spread_ms": {k: spread(v) for k, v in ms.items()},
        "time_added_ms": round(med["captured_summary"] - med["captured"], 4),
        "launches_per_step": launches,
        "launches_added": (launches["summary_true"] - launches["summary_false"]) if len(launches) == 2 else None,
        "memory_summary_false": mem_plain, "memory_summary_true": mem_summ,
        "peak_allocated_added_MiB": round(mem_summ["peak_allocated_MiB"] - mem_plain["peak_allocated_MiB"], 2),
        "peak_reserved_added_MiB": round(mem_summ["peak_reserved_MiB"] - mem_plain["peak_reserved_MiB"], 2),
        "held_reserved_added_MiB": round(mem_summ["held_reserved_MiB"] - mem_plain["held_reserved_MiB"], 2),
        "last_row": row}
    if note:
        report["summary"]["launches_note"] = note
    report["today"] = {
        "steps_per_s": {k: round(1e3 / v, 2) for k, v in med.items()},
        "captured_summary_over_eager_gather_items": round(med["eager_gather_items"] / med["captured_summary"], 3),
        "captured_summary_over_captured_plus_second_forward": round(med["captured_plus_second_forward"] / med["captured_summary"], 3)}
    print(json.dumps(report["summary"]), flush=True)
    print(json.dumps(report["today"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
