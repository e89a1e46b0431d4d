"""Time the choice between two regressors (poco_amd/select.py, csrc/select_regressor.hip), after warm-up:

    python tools/bench_select.py [--iters 30] [--out profiles/select_step.txt]

  (a) the operator (two launches + the wrapper's checks and allocations) at 1 / 16 / 64 / 128 rows in both modes with the demo's
      five payloads (vertices, 3-D joints, 2-D joints, betas, pred_cam), against the same selection written with torch.where and
      indexing; device events around the Python call, interleaved rounds, the median of the rounds' medians;
  (b) the pair's forward (two resnet50-cliff engines + the operator; joint mode adds the read-back of the mixed count and the LBS
      of the mixed rows) against the two engines' forwards run one after the other, at 64 crops, the same way.
  (c) eval.py's loop over 128 ready-made crops in batches of 64 with SMPL ground truth: evaluate.run_eval with model 1 alone
      against evaluate.run_eval_pair (two forwards, the operator, three evaluators, three finish() calls), the same way; the
      call includes the uploads of the batches and ends with the read-back of the records.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import evaluate, ops, select, synth  # noqa: E402
from poco_amd.synth import SMPL_PARENTS  # noqa: E402
from tests import util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

WIDTHS = (20670, 147, 98, 10, 3)
ROUNDS = 5


def torch_select(pose0, var0, pose1, var1, pay, scale, mode, thr=0.40):
    """The same selection (root rule for both models, kinematic on) with torch.where and indexing: the baseline of (a)."""
    u0, u1 = var0.clone(), var1.clone()
    for c in range(1, 24):
        u0[:, c] += u0[:, int(SMPL_PARENTS[c])]
        u1[:, c] += u1[:, int(SMPL_PARENTS[c])]
    if mode == "crop":
        g0 = torch.where(u0[:, 0] > 2 * thr, torch.ones_like(u0[:, 0]), u0[:, 0]).double()
        g1 = torch.where(u1[:, 0] > 2 * thr, torch.ones_like(u1[:, 0]), u1[:, 0]).double()
        choice = ((scale * g1) < g0)[:, None].expand(-1, 24)
    else:
        choice = (scale * u1.double()) < u0.double()
    pose = torch.where(choice[:, :, None, None], pose1, pose0)
    var = torch.where(choice, var1, var0)
    root = choice[:, 0]
    out = [torch.where(root[:, None], b, a) for a, b in pay]
    mixed = choice.any(1) & ~choice.all(1)
    return pose, var, out, torch.nonzero(mixed)[:, 0]


def rounds(fns, iters):
    """Interleaved rounds of the given callables; per callable the median of its rounds' medians and the spread of those."""
    meds = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            meds[i].append(event_ms(fn, iters)[0])
    return [(statistics.median(m), min(m), max(m)) for m in meds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 10)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_select.py on {torch.cuda.get_device_name(0)}: ms, median of {ROUNDS} interleaved rounds' medians of {iters} "
             "calls (lowest .. highest round), device events around the Python call"]
    r = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    for B in (1, 16, 64, 128):
        pose0, pose1 = t(r.standard_normal((B, 24, 3, 3))), t(r.standard_normal((B, 24, 3, 3)))
        var0, var1 = t(r.uniform(0.01, 0.05, (B, 24))), t(r.uniform(0.01, 0.05, (B, 24)))
        pay = [(t(r.standard_normal((B, w))), t(r.standard_normal((B, w)))) for w in WIDTHS]
        for mode in select.MODES:
            op = lambda: ops.select_regressor(pose0, var0, 1, pose1, var1, 1, pay, scale=1.0, mode=mode, rows=True)   # noqa: E731
            ref = lambda: torch_select(pose0, var0, pose1, var1, pay, 1.0, mode)                                      # noqa: E731
            (a, alo, ahi), (b, blo, bhi) = rounds([op, ref], iters)
            lines.append(f"(a) operator {B:3d} rows, {mode:5s}: {a:.4f} ({alo:.4f} .. {ahi:.4f})   torch.where + indexing: {b:.4f} "
                         f"({blo:.4f} .. {bhi:.4f})")
    B = 64
    m0 = util.make_engine("resnet50-cliff", max_batch=B, seed=0)
    m1 = util.make_engine("resnet50-cliff", max_batch=B, seed=1)
    batch = {"img": t(r.standard_normal((B, 3, 224, 224))), "bbox_info": t(r.standard_normal((B, 3)) * 0.1),
             "focal_length": t(np.full(B, 1500.0)), "scale": t(np.full(B, 1.2)), "center": t(np.tile([[640.0, 360.0]], (B, 1))),
             "orig_shape": t(np.tile([[720.0, 1280.0]], (B, 1)))}

    def both():
        m0(batch, want_segm=False)
        m1(batch, want_segm=False)

    fns, names = [both], ["the two forwards one after the other"]
    for mode in select.MODES:
        pair = select.RegressorPair(m0, m1, mode=mode)
        fns.append(lambda pair=pair: pair(batch))
        names.append(f"the pair's forward, --select {mode}")
    for name, (a, lo, hi) in zip(names, rounds(fns, max(iters // 3, 5))):
        lines.append(f"(b) {B} crops, resnet50-cliff x 2, {name}: {a:.3f} ({lo:.3f} .. {hi:.3f})")
    N = 128
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(Path(tmp) / "ds.npz", imgname=np.array([f"{i}.png" for i in range(N)]), center=np.tile([[640.0, 360.0]], (N, 1)),
                 scale=np.full(N, 1.2), pose=(r.standard_normal((N, 72)) * 0.2).astype(np.float32),
                 shape=r.standard_normal((N, 10)).astype(np.float32), img=r.standard_normal((N, 3, 224, 224)).astype(np.float32),
                 orig_shape=np.tile([[720.0, 1280.0]], (N, 1)))
        ds = evaluate.EvalDataset(str(Path(tmp) / "ds.npz"))
        J = synth.synth_j_regressor_h36m(11)
        fns, names = [lambda: evaluate.run_eval(m0, ds, J, batch_size=B)], ["model 1 alone (run_eval)"]
        for mode in select.MODES:
            pair = select.RegressorPair(m0, m1, mode=mode)
            fns.append(lambda pair=pair: evaluate.run_eval_pair(pair, ds, J, batch_size=B))
            names.append(f"with the second model (run_eval_pair), --select {mode}")
        for name, (a, lo, hi) in zip(names, rounds(fns, max(iters // 3, 5))):
            lines.append(f"(c) eval.py's loop, {N} crops in batches of {B}, {name}: {a:.3f} ({lo:.3f} .. {hi:.3f})")
    m0.check_status(sync=True)
    m1.check_status(sync=True)
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
