#!/usr/bin/env python3
"""Validation throughput at the shipped configuration (512x640, 5 views, batch 1 and 2), samples/s of
  (a) today_loop          the loop a user writes without mvster_amd.validate: eval ``model(...)`` (the forward cache's graph
                          replay), ``MVS4net_loss``, the four depth metrics as the reference's boolean-gather tensor
                          expressions (utils.py:125-159), 17 ``.item()``
  (b) validator_eager     ``Validator(capture=False)``
  (c) validator_captured  ``Validator``: one graph replay per batch, no host synchronisation
Protocol: every variant warmed up, then WINDOWS windows of STEPS batches per variant, the variants alternating inside every
round (same box, same minute), a window timed with the host clock around work that ends in a device synchronise; the figure
is the median window.  The launch count of one replay is the number of device activities (kernels and copies) the profiler
sees for the same sequence run eagerly, counted in a run of its own.  Writes one JSON file (--out)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

LOSS_KW = dict(stage_lw=[1, 1, 1, 1], l1ot_lw=[0, 1], inverse_depth=True, ot_iter=10, ot_eps=1, ot_continous=False)


def gather_metrics(depth_est, depth_gt, mask):
    """The reference's four metrics written as it writes them: per image, boolean-mask gathers, fp32 means."""
    abs_err, thres = [], {2: [], 4: [], 8: []}
    for i in range(depth_gt.shape[0]):
        e = (depth_est[i][mask[i]] - depth_gt[i][mask[i]]).abs()
        abs_err.append(e.mean())
        for t in thres:
            thres[t].append((e > t).float().mean())
    return [torch.stack(abs_err).mean()] + [torch.stack(v).mean() for v in thres.values()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "validation_step.json"))
    args = ap.parse_args()
    if args.windows < 3:
        ap.error("--windows: the median needs at least 3 windows")
    if not torch.cuda.is_available():
        sys.exit("val_bench.py measures on an MI355X: no GPU here, nothing measured")
    from bench import SHIPPED, load_weights
    from mvster_amd import SCALAR_NAMES, MVS4net, MVS4net_loss, Validator
    from mvster_amd.synthetic import make_inputs

    dev = torch.device("cuda:0")
    H, W, N = args.height, args.width, args.views
    model = MVS4net(**SHIPPED)
    model.load_state_dict(load_weights(), strict=True)
    model.to(dev).eval()
    report = {"config": {"height": H, "width": W, "views": N, "windows": args.windows, "steps_per_window": args.steps,
                         "warmup": args.warmup, "device": torch.cuda.get_device_name(0)},
              "unit": "samples/s (median window; a sample is one reference view with its source views)", "batch": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        imgs, proj, dv = make_inputs(nviews=N, H=H, W=W, seed=0, device=dev, batch=B)
        g = torch.Generator().manual_seed(0)
        gt, mask = {}, {}
        for s in range(1, 5):
            hs, ws = H // 2 ** (4 - s), W // 2 ** (4 - s)
            gt["stage%d" % s] = (500 + 300 * torch.rand(B, hs, ws, generator=g)).to(dev)
            mask["stage%d" % s] = (torch.rand(B, hs, ws, generator=g) > 0.2).float().to(dev)

        def today_loop():
            with torch.no_grad():
                out = model(imgs, proj, dv)
                loss, d_loss, c_loss, range_err = MVS4net_loss(out, gt, mask, mono=False, **LOSS_KW)
                metrics = gather_metrics(out["depth"], gt["stage4"], mask["stage4"] > 0.5)
                scalars = dict(zip(SCALAR_NAMES, [loss] + list(d_loss) + list(c_loss) + list(range_err) + metrics))
                return {k: v.item() for k, v in scalars.items()}

        eager = Validator(model, imgs, proj, dv, gt, mask, capture=False, **LOSS_KW)
        captured = Validator(model, imgs, proj, dv, gt, mask, **LOSS_KW)
        variants = {"today_loop": today_loop,
                    "validator_eager": lambda: eager(imgs, proj, dv, gt, mask),
                    "validator_captured": lambda: captured(imgs, proj, dv, gt, mask)}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the three agree on what they compute (the gathers' fp32 means against fp64 sums: last bits)
        ref = today_loop()
        row = dict(zip(SCALAR_NAMES, captured(imgs, proj, dv, gt, mask).tolist()))
        worst = max(abs(row[k] - ref[k]) / max(abs(ref[k]), 1e-30) for k in SCALAR_NAMES if ref[k] != 0.0 or row[k] != 0.0)
        rates = {k: [] for k in variants}
        for _ in range(args.windows):
            for name, fn in variants.items():                   # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    fn()
                torch.cuda.synchronize()
                rates[name].append(args.steps * B / (time.perf_counter() - t0))
        # launches of one batch: the eager sequence under the profiler, in a run of its own
        launches, note = None, None
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                eager()
                torch.cuda.synchronize()
            launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception as e:                                   # (the figure is then missing from the file, and says why)
            note = "%s: %s" % (type(e).__name__, str(e)[:200])
        med = {k: statistics.median(v) for k, v in rates.items()}
        entry = {"samples_per_s": {k: round(v, 2) for k, v in med.items()},
                 "windows": {k: [round(x, 2) for x in v] for k, v in rates.items()},
                 "captured_over_today_loop": round(med["validator_captured"] / med["today_loop"], 3),
                 "captured_over_eager": round(med["validator_captured"] / med["validator_eager"], 3),
                 "launches_per_batch": launches,
                 "scalars_worst_relative_difference_to_today_loop": worst}
        if note:
            entry["launches_note"] = note
        report["batch"][str(B)] = entry
        print("batch %d: %s" % (B, json.dumps(entry)), flush=True)
        del eager, captured
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
