"""The conv configurations the engine runs BETWEEN the tuned batch sizes.

poco_amd/tuned/gfx950.json holds entries for a few batch sizes only; at every other batch tune.apply_table hands each conv op the
entry of the nearest tuned batch (log space, ties to the larger one), poco_set_conv_cfg accepts it after looking at LDS bytes and
weight layout, and a refusal leaves the built-in heuristic in place.  test_tuned_table_entries (test_conv_gpu.py) launches the
table's (shape, cfg) pairs at the batch sizes they were measured at; the pairs (shape at B', cfg measured at B) of a forward of 23,
46 or 91 crops - ragged last items of the flat / mosaic Winograd kernels, another stream-K split, persistent grids with a partial
last round - met a reference only through whole-model outputs of damped weights.

(1) test_transferred_pairs: the work list is read from finalized engines (model.conv_cfg applies the table as the forward does, so
    heuristic fall-backs are in it too), reduced to distinct (B', shape, cfg), and every pair goes through ops.conv2d_nhwc with
    residual and ReLU against the fp64 conv of test_conv_gpu.py, all crops and all pixels, with the per-ALG tolerances of the
    project (test_conv_views_gpu.TOL, 2e-5 otherwise; relative to max(1, max|ref|)).
    Batch sizes: the first and the last batch every entry is ever transferred to (raggedness is extreme at the ends of a transfer
    range), derived from the table's own batch sizes.
(2) test_transferred_forward: whole forwards at 23 / 46 / 91 crops (workspace planned for an odd max_batch, lanes, fused, grouped and
    chained launches that have no stand-alone cfg) against the same crops run in batches of 32 - a tuned size, itself held against
    the oracle - on a second engine.  Crops are independent, so the two must agree to the whole-model gate.
"""
import math
import re
import time
import zlib
from collections import Counter

import numpy as np
import pytest
import torch

from poco_amd import synth, tune
from tests import util
from tests.test_conv_gpu import _conv_fp64_gpu
from tests.test_conv_views_gpu import TOL as WINO_TOL

pytestmark = pytest.mark.gpu

VARIANTS = ["hrnet_w32-pare", "hrnet_w48_cls-cliff", "resnet50-cliff"]
DEFAULT_TOL = 2e-5          # exact fp32 fma chains, only the summation order differs (test_conv_gpu.py)
EXPECTED_BATCHES = [2, 3, 7, 8, 9, 22, 23, 45, 46, 90, 91, 127, 130]


def _parse_key(key):
    return tuple(map(int, re.fullmatch(r"(\d+)x(\d+)x(\d+)x(\d+)x(\d+)k(\d+)s(\d+)", key).groups()))


def _tuned_batches():
    return sorted({_parse_key(k)[0] for k, cfg in tune.load_table().items() if cfg and cfg[0] > 0})


def _transfer_batches():
    """Both sides of the log-space midpoint of every two consecutive tuned batches a < b: m = floor(sqrt(a b)) is the last batch
    that takes a's entry and m + 1 the first that takes b's; where a b is a square, m itself is the tie (it goes to b) and m - 1
    the last on a's side, so both are kept.  Then the other end of the outermost ranges (a + 1 of the smallest pair, b - 1 of the
    largest) and a batch two above the largest tuned one (above every entry, and no multiple of 4: a partly empty 2 x 2 mosaic)."""
    tuned = _tuned_batches()
    out = set()
    for a, b in zip(tuned, tuned[1:]):
        m = math.isqrt(a * b)
        out |= {m, m + 1}
        if m * m == a * b:
            out.add(m - 1)
    out |= {tuned[0] + 1, tuned[-1] - 1, tuned[-1] + 2}
    return sorted(out - set(tuned))


BATCHES = _transfer_batches()

_ENGINES = {}
_STRESS = {}            # variant -> (synthetic "stress" weights, engine for batches of CHUNK): made once, shared by the three B'
_CHECKED = set()        # (B', H, W, Cin, Cout, ks, stride, cfg7) already launched: a pair shared by two variants runs once


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    """The engines of this module (three at max(BATCHES) crops, three at CHUNK) go when its last test is done."""
    yield
    _ENGINES.clear()
    _STRESS.clear()


def _engine(variant):
    """One finalized engine per variant: the per-batch cfgs are kept in a map per op, so it serves every B'."""
    if variant not in _ENGINES:
        _ENGINES[variant] = util.make_engine(variant, max_batch=max(BATCHES))
    return _ENGINES[variant]


def _work_list(variant, B):
    """Distinct (B, H, W, Cin, Cout, ks, stride, cfg7) of the variant's conv ops at batch size B, and for each the tuned batch its
    cfg came from (0 = the heuristic) with the number of ops that run it.  Pairs that are verbatim in the table are dropped
    (test_tuned_table_entries has them)."""
    m = _engine(variant)
    table = tune.load_table()
    by_shape = {}
    for k, cfg in table.items():
        b, rest = k.split("x", 1)
        by_shape.setdefault(rest, []).append((int(b), cfg))
    pairs, origin = {}, Counter()
    for i, _ in enumerate(m.ops()):
        d = m.conv_desc(i)
        if d is None:
            continue
        cfg = tuple(m.conv_cfg(i, B))
        key = tune.shape_key(B, *d[:6])
        if tuple(table.get(key, ())) == cfg:
            continue
        src = next((b for b, c in tune.transfer_candidates(by_shape.get(key.split("x", 1)[1], []), B, d[4]) if tuple(c) == cfg), 0)
        origin[src] += 1
        pairs[(B,) + tuple(d[:6]) + (cfg,)] = src
    return pairs, origin


def _table_algs(variant):
    """ALGs of the table's entries for the conv shapes of this variant."""
    m = _engine(variant)
    shapes = {tuple(m.conv_desc(i)[:6]) for i, _ in enumerate(m.ops()) if m.conv_desc(i) is not None}
    return {cfg[6] for k, cfg in tune.load_table().items() if cfg and cfg[0] > 0 and _parse_key(k)[1:] in shapes}


def test_transfer_batches_follow_the_table():
    """A table with other batch sizes has other transfer ranges: whoever changes it revisits this list."""
    assert _tuned_batches() == [1, 4, 16, 32, 64, 128]
    assert BATCHES == EXPECTED_BATCHES


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_transferred_pairs(variant, B, cuda):
    """Every distinct (shape at B, cfg) the engine of `variant` launches at the off-table batch size B against the fp64 conv.
    A pair the library refuses at launch although poco_set_conv_cfg accepted it fails (the forward would fail there too)."""
    from poco_amd import ops
    from poco_amd._lib import PocoHipError
    pairs, origin = _work_list(variant, B)
    assert pairs, "no off-table pairs"
    gen = torch.Generator(device=cuda)
    bad, refused, by_alg, ran = {}, [], {}, 0
    t0 = time.perf_counter()
    for pair in sorted(pairs):
        if pair in _CHECKED:
            continue
        _CHECKED.add(pair)
        _, H, W, Cin, Cout, ks, stride, cfg = pair
        key = tune.shape_key(*pair[:7])
        seed = zlib.crc32(key.encode())
        gen.manual_seed(seed % (2 ** 31))
        x = torch.randn((B, H, W, Cin), device=cuda, generator=gen)
        rng = np.random.default_rng(seed)
        w = (rng.standard_normal((Cout, Cin, ks, ks)) / np.sqrt(Cin * ks * ks)).astype(np.float32)
        shift = rng.uniform(-0.5, 0.5, Cout).astype(np.float32)
        pad = (ks - 1) // 2
        Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
        res = torch.randn((B, Ho, Wo, Cout), device=cuda, generator=gen)
        try:
            out = ops.conv2d_nhwc(x, w, None, shift, stride, res, True, cfg=cfg)
        except (PocoHipError, RuntimeError) as e:
            refused.append((key, cfg, str(e)[:80]))
            del x, res
            continue
        ref = _conv_fp64_gpu(x, w, shift, stride, res, True)
        assert out.shape == ref.shape
        scale = max(1.0, float(ref.abs().max()))
        err = float((out.double() - ref).abs().max()) / scale       # NaN (an element the kernel left unwritten) fails below
        ran += 1
        by_alg[cfg[6]] = max(by_alg.get(cfg[6], 0.0), err) if err == err else err
        if not err <= WINO_TOL.get(cfg[6], DEFAULT_TOL):
            bad[key] = (cfg, "from B=%d" % pairs[pair] if pairs[pair] else "heuristic", err, WINO_TOL.get(cfg[6], DEFAULT_TOL))
        del x, res, out, ref
    torch.cuda.synchronize()
    print(f"transfer {variant} B={B}: {len(pairs)} distinct pairs, {ran} launched here ({len(pairs) - ran - len(refused)} shared with "
          f"an earlier case), {time.perf_counter() - t0:.2f} s; ops by origin (tuned batch: ops, 0 = heuristic):",
          dict(sorted(origin.items())), "; worst relative deviation per ALG:", {a: "%.1e" % v for a, v in sorted(by_alg.items())})
    for r in refused:
        print("  refused:", r)
    assert not bad, bad
    assert refused == [], refused


def test_transfer_work_list_not_vacuous(cuda):
    """The work list is read from the engine; this holds it to what it is there for: something at every (variant, B'), every
    ALG of the table for the variant's shapes also off the table, and the batch-dependent forms - flat and mosaic items of ALG 13,
    the stream-K split of ALG 14 - among the transferred pairs."""
    every = set()
    for variant in VARIANTS:
        algs = set()
        for B in BATCHES:
            pairs, origin = _work_list(variant, B)
            assert pairs, (variant, B)
            algs |= {p[7][6] for p in pairs}
            every |= set(pairs)
            print(f"work list {variant} B={B}: {len(pairs)} distinct pairs; ops by origin (tuned batch: ops, 0 = heuristic):",
                  dict(sorted(origin.items())))
        assert _table_algs(variant) <= algs, (variant, sorted(_table_algs(variant) - algs))
    cfgs = [p[7] for p in every]
    assert any(c[6] == 13 and c[5] == 0 and c[4] == 4 for c in cfgs), "no ALG 13 pair with flat items"
    assert any(c[6] == 13 and c[5] == 0 and c[4] > 4 for c in cfgs), "no ALG 13 pair with mosaic items"
    assert any(c[6] == 14 for c in cfgs), "no ALG 14 pair"
    print(f"work list: {len(every)} distinct transferred pairs over all variants; per ALG:", dict(sorted(Counter(c[6] for c in cfgs).items())))


# ------------------------------------------------------------------------------------------------------------
# Whole forwards at transferred batch sizes
# ------------------------------------------------------------------------------------------------------------
GATE = 1e-3                  # test_model_gpu.py TOL (BASELINE.json north_star)
CHUNK = 32                   # a tuned batch size
KEYS = ("pred_pose", "pred_shape", "pred_cam", "var_pose", "smpl_vertices", "smpl_joints3d", "pred_cam_t")


def _stress(variant):
    if variant not in _STRESS:
        w = util.synth_weights(variant, 0, "stress")
        _STRESS[variant] = (w, util.make_engine(variant, max_batch=CHUNK, profile="stress", weights=w))
    return _STRESS[variant]


@pytest.mark.parametrize("B", [23, 46, 91])       # one of each large transfer range: the entries of 32, 64 and 128 crops
@pytest.mark.parametrize("variant", VARIANTS)
def test_transferred_forward(variant, B, cuda):
    """Crop k of a forward of B crops (engine planned for max_batch = B, undamped "stress" weights) equals crop k run inside batches
    of 32 on a second engine; the last chunk is padded by repeating its crops.  Gate and keys of test_oracle_other_batches."""
    assert B in BATCHES
    batch = util.cuda_batch(synth.synth_batch(B, 4321 + B, profile="stress"), cuda)
    weights, small = _stress(variant)
    m = util.make_engine(variant, max_batch=B, profile="stress", weights=weights)
    out = m(batch)
    m.check_status(sync=True)
    out = {k: out[k].clone() for k in KEYS + ("smpl_joints2d",)}
    parts = {k: [] for k in out}
    for s in range(0, B, CHUNK):
        n = min(CHUNK, B - s)
        idx = torch.arange(CHUNK, device=cuda) % n + s
        o = small({k: v[idx].contiguous() for k, v in batch.items()})
        small.check_status(sync=True)
        for k in parts:
            parts[k].append(o[k][:n].clone())
    ref = {k: torch.cat(v) for k, v in parts.items()}
    j2_scale = max(1.0, float(ref["smpl_joints2d"].abs().max()))
    scale = {k: 1.0 for k in KEYS}
    scale["smpl_joints2d"] = j2_scale        # full-image pixels (values ~1e3) for cliff: relative gate
    # a forward that ignores its input must not pass: the first and the last crop differ by far more than the gate
    differ = {k: float((ref[k][0] - ref[k][B - 1]).abs().max()) / scale[k] for k in ref}
    errs = {k: float((out[k] - ref[k]).abs().max()) / scale[k] for k in ref}
    print(f"forward {variant} B={B}: deviation from the chunked run", {k: "%.1e" % v for k, v in errs.items()},
          "; crop 0 against crop B-1:", {k: "%.1e" % v for k, v in differ.items()})
    for k, v in differ.items():
        assert v > 10 * GATE, (k, v)
    for k in ref:
        assert out[k].shape == ref[k].shape and bool(torch.isfinite(out[k]).all()), k
        assert errs[k] < GATE, (k, errs[k])
