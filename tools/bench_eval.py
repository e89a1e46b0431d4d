"""Time the evaluator step (csrc/eval_metrics.hip) with device events, after warm-up, median of >= 20:

    python tools/bench_eval.py [--iters 30] [--out profiles/eval_step.txt]

  (a) one step at 1 / 16 / 64 / 128 crops with ground-truth vertices;
  (b) the host path it replaces on the same tensors: D2H of both vertex arrays + tests/eval_np.py in float32 (wall clock);
  (c) resnet50-cliff and hrnet_w48_cls-cliff: forward + step at 64 crops against the forward alone, same process, interleaved
      A/B rounds.
--likelihood measures the flow likelihood instead (csrc/eval_likelihood.hip; --out profiles/eval_likelihood.txt):
  (d) one POCO.flow_nll step (context layer, residual rows, RealNVP log_prob, epilogue) at 1 / 16 / 64 / 128 crops for both flow
      depths (resnet50-cliff: 1 layer pair, 2048-d features; hrnet_w32-pare: 3 pairs, 3072-d);
  (e) the host path it replaces on the same tensors: D2H of pred_pose, var_pose and uncert_feat + tests/likelihood_np.py in float32
      (wall clock, torch on the CPUs the process is given);
  (f) forward + evaluator step against forward + evaluator step + likelihood step at 64 crops, interleaved A/B rounds.
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

from poco_amd import evaluate, synth  # noqa: E402
from tests import eval_np, util  # noqa: E402


def event_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def likelihood_legs(iters, dev):
    from tests import likelihood_np as lnp
    lines = [f"# tools/bench_eval.py --likelihood on {torch.cuda.get_device_name(0)}, median of {iters} (min .. max), ms"]
    einp = eval_np.fixture_inputs()
    J, jm = einp["J_regressor"], eval_np.joint_map("3dpw")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for variant, L, in_ctx in lnp.FIXTURE_CASES:
        model = util.make_engine(variant, max_batch=128)
        w = lnp.flow_weights(variant)
        inp = lnp.fixture_inputs(variant)
        for B in (1, 16, 64, 128):
            idx = np.arange(B) % lnp.FIXTURE_CROPS
            pred = {k: t(inp[k][idx]) for k in ("pred_pose", "var_pose", "uncert_feat")}
            gp, valid = t(inp["gt_pose"][idx]), t(inp["has_smpl"][idx])
            rec = torch.empty(B, 80, device=dev)
            med, lo, hi = event_ms(lambda: model.flow_nll(pred, gp, valid, out=rec), iters)
            lines.append(f"(d) {variant} ({L} layer pair{'s' if L > 1 else ''}) flow_nll B={B}: {med:.4f} ({lo:.4f} .. {hi:.4f})")

            def host():
                pp, var, uf = (pred[k].cpu().numpy() for k in ("pred_pose", "var_pose", "uncert_feat"))
                ctx = lnp.context(w, uf, np.float32)
                lnp.summary(lnp.records(lnp.flow_nll(w, pp, inp["gt_pose"][idx], var, ctx, inp["has_smpl"][idx], np.float32)))

            host()
            ts = []
            for _ in range(max(iters // 3, 7)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                ts.append(1e3 * (time.perf_counter() - t0))
            lines.append(f"(e) {variant} host path B={B} (D2H of pose, sigma, features + likelihood_np float32, {torch.get_num_threads()} threads): "
                         f"{statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})")
        del model
        # (f) behind the forward and the evaluator step
        B = 64
        model = util.make_engine(variant, max_batch=B)
        batch = util.cuda_batch(synth.synth_batch(B, 1234), dev)
        idx = np.arange(B) % eval_np.FIXTURE_CROPS
        gp, gv = t(einp["gt_pose"][idx]), t(einp["gt_vertices"][idx])
        out = model._alloc_outputs(B, False)
        ev = evaluate.Evaluator(J, jm, capacity=B, device=dev)
        lk = evaluate.LikelihoodAccumulator(model, capacity=B)

        def fwd_step():
            model(batch, out=out, want_segm=False)
            ev.reset()
            ev.step(out, gp, gt_vertices=gv)

        def fwd_step_lk():
            fwd_step()
            lk.reset()
            lk.step(out, gp)

        a, b = [], []
        for rnd in range(4):                                   # interleaved A/B rounds
            a.append(event_ms(fwd_step, iters // 2)[0])
            b.append(event_ms(fwd_step_lk, iters // 2)[0])
        model.check_status(sync=True)
        lines.append(f"(f) {variant} B=64 forward + step: {statistics.median(a):.4f}  + likelihood step: {statistics.median(b):.4f}  "
                     f"difference: {statistics.median(b) - statistics.median(a):+.4f}  (rounds {['%.4f' % x for x in a]}, "
                     f"with likelihood {['%.4f' % x for x in b]})")
        ev.close()
        del model, lk
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--likelihood", action="store_true", help="measure the flow likelihood legs (d) - (f) instead of (a) - (c)")
    args = ap.parse_args()
    iters = max(args.iters, 20)
    dev = torch.device("cuda:0")
    if args.likelihood:
        lines = likelihood_legs(iters, dev)
        print("\n".join(lines))
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")
        return
    lines = [f"# tools/bench_eval.py on {torch.cuda.get_device_name(0)}, median of {iters} (min .. max), ms"]
    inp = eval_np.fixture_inputs()
    J, jm = inp["J_regressor"], eval_np.joint_map("3dpw")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for B in (1, 16, 64, 128):
        idx = np.arange(B) % eval_np.FIXTURE_CROPS
        pred = {"smpl_vertices": t(inp["pred_vertices"][idx]), "pred_pose": t(inp["pred_pose"][idx]), "var_pose": t(inp["var_pose"][idx])}
        gp, gv = t(inp["gt_pose"][idx]), t(inp["gt_vertices"][idx])
        ev = evaluate.Evaluator(J, jm, capacity=B, device=dev)

        def step():
            ev.reset()
            ev.step(pred, gp, gt_vertices=gv)

        med, lo, hi = event_ms(step, iters)
        lines.append(f"(a) step B={B}: {med:.4f} ({lo:.4f} .. {hi:.4f})")

        def host():
            pv, g = pred["smpl_vertices"].cpu().numpy(), gv.cpu().numpy()
            eval_np.evaluate(pv, inp["pred_pose"][idx], inp["var_pose"][idx], inp["gt_pose"][idx], J, jm, gt_vertices=g, dtype=np.float32)

        host()
        ts = []
        for _ in range(max(iters // 3, 7)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            ts.append(1e3 * (time.perf_counter() - t0))
        lines.append(f"(b) host path B={B} (D2H of both meshes + eval_np float32): {statistics.median(ts):.3f} ({min(ts):.3f} .. {max(ts):.3f})")
        ev.close()
    for variant in ("resnet50-cliff", "hrnet_w48_cls-cliff"):
        B = 64
        model = util.make_engine(variant, max_batch=B)
        batch = util.cuda_batch(synth.synth_batch(B, 1234), dev)
        idx = np.arange(B) % eval_np.FIXTURE_CROPS
        gp, gv = t(inp["gt_pose"][idx]), t(inp["gt_vertices"][idx])
        out = model._alloc_outputs(B, False)
        ev = evaluate.Evaluator(J, jm, capacity=B, device=dev)

        def fwd():
            model(batch, out=out, want_segm=False)

        def fwd_step():
            model(batch, out=out, want_segm=False)
            ev.reset()
            ev.step(out, gp, gt_vertices=gv)

        a, b = [], []
        for rnd in range(4):                                   # interleaved A/B rounds
            a.append(event_ms(fwd, iters // 2)[0])
            b.append(event_ms(fwd_step, iters // 2)[0])
        model.check_status(sync=True)
        lines.append(f"(c) {variant} B=64 forward: {statistics.median(a):.4f}  forward + step: {statistics.median(b):.4f}  "
                     f"difference: {statistics.median(b) - statistics.median(a):+.4f}  (rounds fwd {['%.4f' % x for x in a]}, "
                     f"fwd+step {['%.4f' % x for x in b]})")
        ev.close()
        del model
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
