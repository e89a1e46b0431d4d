"""Time the segmentation step of eval.py --segm on the GPU.

    python tools/bench_segm.py --out profiles/segm_step.txt [--forward]

Per batch size (1, 16, 64, 128 crops): the device step (body-part labels of SMPL-sized meshes + the score of a [B,25,56,56] mask)
against the same scoring arithmetic written with torch on the device (F.interpolate + F.cross_entropy + argmax + bincount; torch
has no rasteriser, so the labels are the device's in both).  --forward adds the HRNet-W32-PARE forward (synthetic weights) alone and
followed by the step.  CUDA events around `iters` back-to-back repetitions after a warm-up, median of `reps` such measurements."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops, segm, synth  # noqa: E402
from tests import render_np  # noqa: E402


def timed(fn, iters, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def torch_score(logits, labels):
    up = F.interpolate(logits, size=labels.shape[1:], mode="bilinear", align_corners=True)
    lab = labels.long()
    ce = F.cross_entropy(up, lab, reduction="none").double().sum((1, 2))
    arg = up.argmax(1)
    B, C = logits.shape[:2]
    base = torch.arange(B, device=logits.device).view(B, 1, 1) * C
    pred = torch.bincount((arg + base).view(-1), minlength=B * C)
    gt = torch.bincount((lab + base).view(-1), minlength=B * C)
    inter = torch.bincount((arg + base)[arg == lab], minlength=B * C)
    return ce, pred, gt, inter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,16,64,128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--forward", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    v2, f2 = render_np.icosphere(5)                                   # 10242 vertices, 20480 faces; the first 13776 are drawn (SMPL: 6890 / 13776)
    faces = f2[:13776]
    mesh = segm.PartMesh(faces, (np.arange(len(faces)) % 24).astype(np.uint8), dev)
    r = np.random.default_rng(0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; mesh: {len(v2)} vertices, {len(faces)} faces (SMPL: 6890 / 13776), about 150 px tall",
             f"iters {a.iters} back to back per measurement, median (min .. max) of {a.reps} measurements, ms per step",
             "B | labels | score | labels + score | torch score (interpolate + cross_entropy + argmax + bincount) | torch / device score"]
    model = None
    if a.forward:
        from tests import util
        model = util.make_engine("hrnet_w32-pare", 128)
    for B in (int(x) for x in a.batches.split(",")):
        verts = torch.from_numpy(np.stack([v2 * 0.5 * (1 + 0.05 * r.standard_normal()) for _ in range(B)]).astype(np.float32)).to(dev)
        cam_t = torch.from_numpy(np.stack([[0.02 * r.standard_normal(), 0.02 * r.standard_normal(), 33.0 + r.uniform(-2, 2)] for _ in range(B)])
                                 .astype(np.float32)).to(dev)
        logits = torch.randn(B, 25, 56, 56, device=dev)
        labels = segm.part_labels(verts, cam_t, mesh)
        rec = torch.empty(B, ops.segm_record_words(25), dtype=torch.int64, device=dev)
        t_lab = timed(lambda: segm.part_labels(verts, cam_t, mesh, out=labels), a.iters, a.reps)
        t_sc = timed(lambda: ops.segm_score(logits, labels, out=rec), a.iters, a.reps)
        t_both = timed(lambda: ops.segm_score(logits, segm.part_labels(verts, cam_t, mesh, out=labels), out=rec), a.iters, a.reps)
        t_torch = timed(lambda: torch_score(logits, labels), a.iters, a.reps)
        fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f} .. {t[2]:.4f})"   # noqa: E731
        lines.append(f"{B} | {fmt(t_lab)} | {fmt(t_sc)} | {fmt(t_both)} | {fmt(t_torch)} | {t_torch[0] / t_sc[0]:.2f}")
        if model is not None:
            batch = {k: torch.from_numpy(x).to(dev) for k, x in synth.synth_batch(B, 0).items()}
            t_f = timed(lambda: model(batch, want_segm=True), 5, a.reps)

            def both():
                o = model(batch, want_segm=True)
                ops.segm_score(o["pred_segm_mask"], segm.part_labels(verts, cam_t, mesh, out=labels), out=rec)
            t_fs = timed(both, 5, a.reps)
            lines.append(f"    forward alone {fmt(t_f)} | forward + step {fmt(t_fs)} | step share {100 * (t_fs[0] - t_f[0]) / t_fs[0]:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
