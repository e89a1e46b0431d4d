"""Time the visibility step of eval.py --visibility on the GPU.

    python tools/bench_visibility.py --out profiles/visibility_step.txt [--forward]

Per batch size (1, 16, 64, 128 crops) on the 13776-face stand-in mesh of tools/bench_segm.py: poco_op_part_visibility at margin 0 and
at the default margin res / 2, with and without an occluder mask, beside poco_op_part_labels alone - the difference is the price of
the part-bit pass, the counting pass and the margin.  --forward adds the HRNet-W32-PARE forward (synthetic weights) alone and followed
by the step.  CUDA events around `iters` back-to-back repetitions after a warm-up, median of `reps` such measurements; every figure is
one run's, on one machine."""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops, segm, synth  # noqa: E402
from tests import render_np  # noqa: E402
from tools.bench_segm import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,16,64,128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--forward", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    res, margin = 224, 112
    v2, f2 = render_np.icosphere(5)                                   # 10242 vertices, 20480 faces; the first 13776 are drawn (SMPL: 6890 / 13776)
    faces = f2[:13776]
    mesh = segm.PartMesh(faces, (np.arange(len(faces)) % 24).astype(np.uint8), dev)
    r = np.random.default_rng(0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; mesh: {len(v2)} vertices, {len(faces)} faces (SMPL: 6890 / 13776), about 150 px tall",
             f"res {res}; iters {a.iters} back to back per measurement, median (min .. max) of {a.reps} measurements, ms per call; single-run figures",
             f"B | part_labels | visibility margin 0 | visibility margin {margin} | visibility margin {margin} + mask | margin {margin} / part_labels"]
    model = None
    if a.forward:
        from tests import util
        model = util.make_engine("hrnet_w32-pare", 128)
    fmt = lambda t: f"{t[0]:.4f} ({t[1]:.4f} .. {t[2]:.4f})"   # noqa: E731
    for B in (int(x) for x in a.batches.split(",")):
        verts = torch.from_numpy(np.stack([v2 * 0.5 * (1 + 0.05 * r.standard_normal()) for _ in range(B)]).astype(np.float32)).to(dev)
        cam_t = torch.from_numpy(np.stack([[0.02 * r.standard_normal(), 0.02 * r.standard_normal(), 33.0 + r.uniform(-2, 2)] for _ in range(B)])
                                 .astype(np.float32)).to(dev)
        mask = (torch.rand(B, res, res, device=dev) < 0.2).to(torch.uint8)
        labels = segm.part_labels(verts, cam_t, mesh)
        out = torch.empty(B, 24, 4, dtype=torch.int32, device=dev)
        scratch = torch.empty(ops.part_visibility_scratch_bytes(B, res, margin), dtype=torch.uint8, device=dev)

        def vis(m, msk=None):
            return ops.part_visibility(verts, cam_t, mesh.faces, mesh.face_part, 5000.0, res, m, msk, out=out, scratch=scratch)
        t_lab = timed(lambda: segm.part_labels(verts, cam_t, mesh, out=labels), a.iters, a.reps)
        t_v0 = timed(lambda: vis(0), a.iters, a.reps)
        t_vm = timed(lambda: vis(margin), a.iters, a.reps)
        t_vk = timed(lambda: vis(margin, mask), a.iters, a.reps)
        lines.append(f"{B} | {fmt(t_lab)} | {fmt(t_v0)} | {fmt(t_vm)} | {fmt(t_vk)} | {t_vm[0] / t_lab[0]:.2f}")
        if model is not None:
            batch = {k: torch.from_numpy(x).to(dev) for k, x in synth.synth_batch(B, 0).items()}
            t_f = timed(lambda: model(batch, want_segm=False), 5, a.reps)

            def both():
                model(batch, want_segm=False)
                vis(margin, mask)
            t_fs = timed(both, 5, a.reps)
            lines.append(f"    forward alone {fmt(t_f)} | forward + step {fmt(t_fs)} | step share {100 * (t_fs[0] - t_f[0]) / t_fs[0]:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
