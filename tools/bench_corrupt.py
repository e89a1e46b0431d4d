"""Time the image degradation operator (poco_amd/corrupt.py, csrc/corrupt.hip), after warm-up:

    python tools/bench_corrupt.py [--iters 30] [--out profiles/corrupt_step.txt]

  (a) the operator per kind (one launch + the wrapper's checks and the upload of the records; jpeg: one encode, one read-back of the
      bytes and one decode per crop) at 16 / 64 / 128 crops of 224 x 224, normalised output, and for the two kinds that have a plain
      torch form the same on the device in float32: depthwise conv2d on a mirror-padded crop for gaussian_blur, avg_pool2d
      (ceil_mode) + repeat_interleave for pixelate;
  (b) CorruptModel's step (repeat the raw crops K times, the operator, the engine's forward of K * b rows) against the engine's
      forward of the same K * b rows alone, resnet50-cliff, K * b = 64, K = 4 and 8 levels without jpeg, and K = 4 with one jpeg level.
Device events around the Python call, the median (min .. max) of the iterations.  Prints one line per measurement; --out also
writes them to a file.  No pass / fail ratio.  Not measured here: eval.py's whole loop against the loop without the flag."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import corrupt, ops, synth  # noqa: E402
from tests import util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

KINDS = ["gaussian_blur:1", "gaussian_blur:5", "motion_blur:15:30", "pixelate:4", "pixelate:32", "contrast:0.5", "gamma:2.2", "gaussian_noise:8", "jpeg:30"]
LEVELS4 = "gaussian_blur:2,gaussian_noise:8,pixelate:4"
LEVELS8 = "gaussian_blur:1,gaussian_blur:2,gaussian_blur:4,gaussian_noise:8,gaussian_noise:16,pixelate:4,contrast:0.5+gamma:1.5"
LEVELS4J = "gaussian_blur:2,gaussian_noise:8,jpeg:30"


def torch_blur(x, sigma):
    r = int(3.0 * sigma + 0.5)
    k = torch.arange(-r, r + 1, device=x.device, dtype=torch.float32)
    w = torch.exp(-k * k / (2.0 * sigma * sigma))
    w = (w / w.sum())
    xp = torch.nn.functional.pad(x, (r, r, r, r), mode="reflect")
    h = torch.nn.functional.conv2d(xp, w.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    return torch.nn.functional.conv2d(h, w.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)


def torch_pixelate(x, f):
    p = torch.nn.functional.avg_pool2d(x, f, ceil_mode=True, count_include_pad=False)
    return p.repeat_interleave(f, 2).repeat_interleave(f, 3)[..., :x.shape[2], :x.shape[3]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_corrupt.py on {torch.cuda.get_device_name(0)}: ms, median (min .. max) of {a.iters} iterations between device events"]
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"   # noqa: E731
    for N in (16, 64, 128):
        x = (torch.rand(N, 3, 224, 224, device=dev) * 255.0).contiguous()
        out, tmp = torch.empty_like(x), torch.empty_like(x)
        for text in KINDS:
            if text.startswith("jpeg") and N > 16:
                continue                                              # one host round trip per crop: linear in N
            recs = corrupt.records([corrupt.parse_levels(text)[1]] * N, list(range(N)))
            t = event_ms(lambda: ops.corrupt(x, recs, True, out=out, tmp=tmp), a.iters if not text.startswith("jpeg") else 3)
            line = f"(a) {text:18s} N={N:3d}: operator {fmt(t)}"
            if text.startswith("gaussian_blur"):
                line += f" | torch conv2d {fmt(event_ms(lambda: torch_blur(x, float(text.split(':')[1])), a.iters))}"
            if text.startswith("pixelate"):
                line += f" | torch avg_pool2d + repeat {fmt(event_ms(lambda: torch_pixelate(x, int(text.split(':')[1])), a.iters))}"
            lines.append(line)
            print(line, flush=True)
    model = util.make_engine("resnet50-cliff", max_batch=64)
    for text in (LEVELS4, LEVELS8, LEVELS4J):
        cm = corrupt.CorruptModel(model, corrupt.parse_levels(text), 0)
        b = 64 // cm.K
        raw = util.cuda_batch(synth.synth_batch(b, 1), dev)
        raw["img"] = (torch.rand(b, 3, 224, 224, device=dev) * 255.0).contiguous()
        lb = cm.level_batch(raw, range(b))
        iters = a.iters if "jpeg" not in text else 3
        t_fwd = event_ms(lambda: model(lb, want_segm=False), iters)
        t_all = event_ms(lambda: cm.forward_levels(raw, range(b)), iters)
        t_op = event_ms(lambda: cm.level_batch(raw, range(b)), iters)
        line = (f"(b) K={cm.K} x b={b} ({text}): forward alone {fmt(t_fwd)} | repeat + operator + forward {fmt(t_all)} | repeat + operator {fmt(t_op)}"
                f" = {100.0 * t_op[0] / t_all[0]:.1f} % of the step")
        lines.append(line)
        print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
