"""Time the pseudo-labeler's step (csrc/pseudo_gt.hip) with device events around the Python call, after warm-up, median of >= 30:

    python tools/bench_pseudo.py [--iters 30] [--out profiles/pseudo_step.txt]

  (a) one step at 1 / 16 / 64 / 128 crops, keep-all and with a threshold at the median of var[:, 0];
  (b) the host path it replaces on the same tensors: D2H of the five outputs + tests/pseudo_np.py in float32 (wall clock, numpy on
      the CPUs the process is given);
  (c) resnet50-cliff and hrnet_w48_cls-cliff: forward + step at 64 crops against the forward alone, same process, interleaved
      A/B rounds.
Prints one line per measurement; --out also writes them to a file."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import pseudo, synth  # noqa: E402
from tests import pseudo_np, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

KEYS = {"pred_pose": "pred_pose", "pred_shape": "pred_shape", "var_pose": "var_pose", "smpl_joints2d": "joints2d", "smpl_joints3d": "joints3d"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_pseudo.py on {torch.cuda.get_device_name(0)}, median of {iters} (min .. max), ms"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for B in (1, 16, 64, 128):
        x = pseudo_np.step_inputs(B, 1, seed=B)
        pred = {k: t(x[v]) for k, v in KEYS.items()}
        boxes, sid = t(x["boxes"]), t(x["source_id"])
        med_thr = float(np.median(x["var_pose"][:, 0]))
        for name, thr in (("keep all", None), ("median threshold", med_thr)):
            pl = pseudo.PseudoLabeler(B, thr, "hrnet_w48_cls-cliff", device=dev)

            def step():
                pl.reset()
                pl.step(pred, boxes, sid)

            med, lo, hi = event_ms(step, iters)
            lines.append(f"(a) step B={B} {name}: {med:.4f} ({lo:.4f} .. {hi:.4f})  [reset + step: two memsets, two launches]")
            pl.close()

        def host():
            h = {v: pred[k].cpu().numpy() for k, v in KEYS.items()}
            pseudo_np.step(**h, boxes=x["boxes"], source_id=x["source_id"], threshold=med_thr, dtype=np.float32)

        host()
        ts = []
        for _ in range(max(iters // 3, 10)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            ts.append(1e3 * (time.perf_counter() - t0))
        lines.append(f"(b) host path B={B} (D2H of the five outputs + pseudo_np float32): {statistics.median(ts):.3f} "
                     f"({min(ts):.3f} .. {max(ts):.3f})")
    for variant in ("resnet50-cliff", "hrnet_w48_cls-cliff"):
        B = 64
        model = util.make_engine(variant, max_batch=B)
        batch = util.cuda_batch(synth.synth_batch(B, 1234), dev)
        x = pseudo_np.step_inputs(B, 1, seed=B)
        boxes, sid = t(x["boxes"]), t(x["source_id"])
        out = model._alloc_outputs(B, False)
        pl = pseudo.PseudoLabeler(B, None, variant, device=dev)

        def fwd():
            model(batch, out=out, want_segm=False)

        def fwd_step():
            model(batch, out=out, want_segm=False)
            pl.reset()
            pl.step(out, boxes, sid)

        a, b = [], []
        for rnd in range(4):                                   # interleaved A/B rounds
            a.append(event_ms(fwd, iters // 2)[0])
            b.append(event_ms(fwd_step, iters // 2)[0])
        model.check_status(sync=True)
        lines.append(f"(c) {variant} B=64 forward: {statistics.median(a):.4f}  forward + step: {statistics.median(b):.4f}  "
                     f"difference: {statistics.median(b) - statistics.median(a):+.4f}  (rounds fwd {['%.4f' % v for v in a]}, "
                     f"fwd+step {['%.4f' % v for v in b]})")
        pl.close()
        del model
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
