"""Time the temporal metric of eval.py --sequences (poco_amd/sequences.py, csrc/track_accel.hip), after warm-up:

    python tools/bench_accel.py [--iters 30] [--out profiles/accel_step.txt]

  (a) the operator (three launches), device events around the Python call, at 1 / 8 tracks x 300 / 3000 frames, M = 14, on rows of
      stride 416 (the evaluator's records) - and the bytes it moves over that time for the largest case;
  (b) the torch form on the same device rows: slicing, norm, mean and a mask, with the sums per track left out;
  (c) the numpy host path, wall clock: the rows copied to the host, then the same slicing in float64;
  (d) evaluate.run_eval against evaluate.run_eval_sequences (no pipeline) on 256 synthetic crops in 4 tracks, resnet50-cliff, batch
      64, interleaved rounds.
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

from poco_amd import evaluate, ops, synth  # noqa: E402
from tests import util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402
from tools.bench_infill import wall_ms  # noqa: E402

M, REC, R_PRED, R_GT = 14, 416, 116, 212
HBM_TBS = 6.29                                   # measured float4 copy rate of an MI355X (8.0 TB/s spec)


def torch_form(p, g, frames, same):
    """accel / accel_err of rows 1 .. N-2 where the neighbours are of the same track and at consecutive frames, NaN elsewhere."""
    ap = p[:-2] - 2.0 * p[1:-1] + p[2:]
    ag = g[:-2] - 2.0 * g[1:-1] + g[2:]
    ok = same & (frames[:-2] + 1 == frames[1:-1]) & (frames[1:-1] + 1 == frames[2:])
    nan = torch.full_like(ap[:, 0, 0], float("nan"))
    return torch.where(ok, ap.double().norm(dim=-1).mean(-1).float(), nan), torch.where(ok, (ap - ag).double().norm(dim=-1).mean(-1).float(), nan)


def numpy_form(rec_d, frames, track):
    rec = rec_d.cpu().numpy()
    p = rec[:, R_PRED:R_PRED + 3 * M].reshape(-1, M, 3).astype(np.float64)
    g = rec[:, R_GT:R_GT + 3 * M].reshape(-1, M, 3).astype(np.float64)
    ap, ag = p[:-2] - 2.0 * p[1:-1] + p[2:], g[:-2] - 2.0 * g[1:-1] + g[2:]
    ok = (track[:-2] == track[2:]) & (frames[:-2] + 1 == frames[1:-1]) & (frames[1:-1] + 1 == frames[2:])
    acc, err = np.linalg.norm(ap, axis=-1).mean(-1), np.linalg.norm(ap - ag, axis=-1).mean(-1)
    return np.where(ok, acc, np.nan), np.where(ok, err, np.nan), np.bincount(track[1:-1], weights=np.where(ok, err, 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_accel.py on {torch.cuda.get_device_name(0)}, median (min .. max), ms; M = {M}, rows of stride {REC} floats"]
    for P, T in ((1, 300), (8, 300), (1, 3000), (8, 3000)):
        r = np.random.default_rng(100 * P + T)
        N = P * T
        rec = torch.from_numpy(r.standard_normal((N, REC)).astype(np.float32)).to(dev)
        frames_h, track_h = np.tile(np.arange(T, dtype=np.int32), P), np.repeat(np.arange(P), T)
        frames, offsets = torch.from_numpy(frames_h).to(dev), torch.from_numpy(np.arange(P + 1, dtype=np.int32) * T)
        pv, gv = rec[:, R_PRED:R_PRED + 3 * M], rec[:, R_GT:R_GT + 3 * M]
        med, lo, hi = event_ms(lambda: ops.track_accel(pv, gv, frames, offsets), iters)
        lines.append(f"(a) operator {P} x {T}: {med:.4f} ({lo:.4f} .. {hi:.4f})  [three launches + the wrapper's checks and allocations]")
        if (P, T) == (8, 3000):
            # read: 2 buffers x 3M floats (66 rows per 64), frames; written: accel, accel_err, the 3 fp64 terms; read again: the terms
            nbytes = N * (2 * 3 * M * 4 * 66 / 64 + 4 + 8 + 24 + 24)
            lines.append(f"    bytes moved {nbytes / 1e6:.2f} MB over {med:.4f} ms = {nbytes / med / 1e9:.4f} TB/s beside the {HBM_TBS} TB/s an MI355X "
                         f"copies at: at this size the call is bound by its three launches and the wrapper, not by memory")
        p3, g3 = pv.reshape(N, M, 3).contiguous(), gv.reshape(N, M, 3).contiguous()
        same = torch.from_numpy(track_h[:-2] == track_h[2:]).to(dev)
        med_t, lo, hi = event_ms(lambda: torch_form(p3, g3, frames, same), iters)
        lines.append(f"(b) torch form {P} x {T} (dense rows, no sums): {med_t:.4f} ({lo:.4f} .. {hi:.4f})  operator / torch = {med / med_t:.2f}")
        med, lo, hi = wall_ms(lambda: numpy_form(rec, frames_h, track_h), 10)
        lines.append(f"(c) numpy host path {P} x {T} (rows to the host, float64): {med:.3f} ({lo:.3f} .. {hi:.3f})")
    # (d) the evaluation loop with and without --sequences
    with tempfile.TemporaryDirectory() as tmp:
        n, tracks = 256, 4
        r = np.random.default_rng(3)
        names = [f"seq{i % tracks}/image_{i // tracks:05d}.jpg" for i in range(n)]
        np.savez(f"{tmp}/ds.npz", imgname=np.array(names), center=r.uniform(80, 200, (n, 2)).astype(np.float32),
                 scale=r.uniform(0.5, 1.0, n).astype(np.float32), pose=(0.4 * r.standard_normal((n, 72))).astype(np.float32),
                 shape=(0.5 * r.standard_normal((n, 10))).astype(np.float32), img=r.standard_normal((n, 3, 224, 224)).astype(np.float32),
                 orig_shape=np.tile([[240.0, 320.0]], (n, 1)).astype(np.float32))
        model = util.make_engine("resnet50-cliff", max_batch=64)
        J = synth.synth_j_regressor_h36m(11)
        ds = evaluate.EvalDataset(f"{tmp}/ds.npz")
        rounds = {False: [], True: []}
        for _ in range(4):
            for seq in (False, True):
                fn = (lambda: evaluate.run_eval_sequences(model, ds, J, batch_size=64)) if seq else (lambda: evaluate.run_eval(model, ds, J, batch_size=64))
                rounds[seq].append(wall_ms(fn, 3)[0])
        p_, s_ = statistics.median(rounds[False]), statistics.median(rounds[True])
        lines.append(f"(d) evaluation loop, {n} crops in {tracks} tracks: run_eval {p_:.1f}  run_eval_sequences {s_:.1f}  difference: {s_ - p_:+.1f} "
                     f"= {100 * (s_ - p_) / p_:.1f} % of the plain loop  "
                     f"(rounds plain {['%.1f' % v for v in rounds[False]]}, sequences {['%.1f' % v for v in rounds[True]]})")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
