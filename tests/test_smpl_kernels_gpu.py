"""poco_smpl_lbs (poco_amd/csrc/kernels_smpl.hip) on the body models and inputs of tests/smpl_cases.py against the float64
restatement oracle/smpl_np.smpl_lbs_np: vertices and all 49 joints.

Three engines (resnet50-cliff, max_batch 130), one per body model:
  dense  standard tree, dense and one-hot skinning rows, regressors on the last vertex, 5 x posedirs, joint map A
  chain  parents[i] = i - 1, joint map B (A and B together read all 54 joint sources)
  tree   random tree with the uint32 -1 root marker, the standard map reversed

The bound is not a constant.  Per case d32 = max |float32 restatement - float64| is measured on the CPU (smpl_lbs_np with
dtype=float32: the same arithmetic in the kernels' number format, numpy's summation order); the GPU may be 8 x d32 away from
float64 - the margin tests/test_eval_gpu.py tol() gives another summation order of the same float32 arithmetic - and never more
than 1e-3 max(1, max |ref|).  Identity pose with zero betas must give the template to 1e-6.  tests/test_smpl_cases_cpu.py shows
that each fault these cases are built for moves the result by at least ten times this bound.

Measured on an MI355X over every input kind and batch size of test_parity (all within the bound, which is 8):
           worst GPU error   worst d32   worst ratio error / d32 of one case
  dense    1.62e-06          2.28e-06    1.42  (noise, B = 15: 1.62e-06 / 1.14e-06)
  chain    8.24e-07          7.35e-07    1.45  (blend, B = 1:  1.92e-07 / 1.32e-07)
  tree     1.06e-06          1.03e-06    1.06  (noise, B = 48: 1.01e-06 / 9.51e-07)
Column probe, worst ratio of a single crop: 1.09 / 1.46 / 1.30.  Identity pose: the vertices are 2.4e-07 / 1.2e-07 / 1.2e-07 from
the template.  Crop independence and the forward path are bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import smpl_cases as sc
from tests import util

pytestmark = pytest.mark.gpu
VARIANT = "resnet50-cliff"


@pytest.fixture(scope="module")
def engines(cuda):
    """name -> (body model, engine); at most three engines are built for this file, each on first use"""
    from poco_amd.model import POCO
    weights = util.synth_weights(VARIANT)
    built = {}

    def get(name):
        if name not in built:
            smpl = sc.build_model(name)
            m = POCO(backbone=VARIANT, num_flow_layers=util.FLOW_LAYERS[VARIANT], max_batch=sc.N_CROPS, smpl=smpl,
                     keep_state_dict=False)
            m.load_state_dict(weights, strict=True)
            built[name] = (smpl, m.finalize())
        return built[name]
    return get


_refs = {}


def reference(smpl, name, kind):
    """(betas, R, float64 result, float32 restatement) of the 130 crops of an input set: computed once, never changed"""
    if (name, kind) not in _refs:
        betas, R = sc.column_probe() if kind == "probe" else sc.inputs(name, kind)
        ref64, ref32 = sc.lbs_pair(smpl, betas, R)
        for a in (betas, R, ref64, ref32):
            a.setflags(write=False)
        _refs[name, kind] = (betas, R, ref64, ref32)
    return _refs[name, kind]


def run(m, cuda, betas, R):
    """poco_smpl_lbs -> [B, V + 49, 3] float32 on the host, vertices then joints"""
    v, j = m.smpl_lbs(torch.from_numpy(np.array(betas)).to(cuda), torch.from_numpy(np.array(R)).to(cuda))
    torch.cuda.synchronize()
    return torch.cat([v, j], 1).cpu().numpy()


@pytest.mark.parametrize("name,kind", [(n, k) for n in sc.MODELS for k in sc.KINDS[n]])
def test_parity(engines, cuda, name, kind):
    """every batch size of smpl_cases.BATCHES: the first B crops of the input set"""
    smpl, m = engines(name)
    betas, R, ref64, ref32 = reference(smpl, name, kind)
    bad = []
    for B in sc.BATCHES:
        got = run(m, cuda, betas[:B], R[:B])
        assert got.shape == (B, sc.V + 49, 3)
        bound, d32 = sc.tolerance(ref64[:B], ref32[:B])
        err = np.abs(got - ref64[:B])
        ev, ej = float(err[:, :sc.V].max()), float(err[:, sc.V:].max())
        print(f"smpl parity {name} {kind} B={B}: gpu error {max(ev, ej):.3e} (vertices {ev:.3e}, joints {ej:.3e}) d32 {d32:.3e} "
              f"ratio {max(ev, ej) / d32:.2f} bound {bound:.3e}")
        if not max(ev, ej) <= bound:
            crop, row, _ = np.unravel_index(int(np.nanargmax(err)), err.shape)
            what = f"vertex {row}" if row < sc.V else f"joint slot {row - sc.V} (source {int(smpl['joint_map'][row - sc.V])})"
            bad.append(f"B={B}: {max(ev, ej):.3e} > {bound:.3e} at crop {crop}, {what}")
    assert not bad, bad


@pytest.mark.parametrize("name", sc.MODELS)
def test_identity_gives_the_template(engines, cuda, name):
    smpl, m = engines(name)
    betas, R = sc.inputs(name, "identity", 65)
    ref64, ref32 = sc.lbs_pair(smpl, betas[:1], R[:1])
    bound, d32 = sc.tolerance(ref64, ref32)
    assert np.abs(ref64[0, :sc.V] - smpl["v_template"]).max() < 1e-7      # the float32 skinning weights sum to one within 6e-8
    for B in (1, 2, 65):
        got = run(m, cuda, betas[:B], R[:B])
        ev = float(np.abs(got[:, :sc.V] - smpl["v_template"][None]).max())
        ej = float(np.abs(got[:, sc.V:] - ref64[:, sc.V:]).max())
        print(f"smpl identity {name} B={B}: vertices - template {ev:.3e}, joints {ej:.3e} (d32 {d32:.3e}, bound {bound:.3e})")
        assert ev < 1e-6 and ej <= bound, (B, ev, ej, bound)


@pytest.mark.parametrize("name", sc.MODELS)
def test_column_probe(engines, cuda, name):
    """One crop per K row of the blend GEMM (207 pose rows, 10 shape rows), each compared on its own: a misplaced row is named."""
    smpl, m = engines(name)
    betas, R, ref64, ref32 = reference(smpl, name, "probe")
    got = np.concatenate([run(m, cuda, betas[:sc.N_CROPS], R[:sc.N_CROPS]), run(m, cuda, betas[sc.N_CROPS:], R[sc.N_CROPS:])])
    assert got.shape == ref64.shape
    bad, worst = [], (0.0, 0, 0.0, 0.0)
    for k in range(sc.N_PROBE):
        bound, d32 = sc.tolerance(ref64[k], ref32[k])
        err = float(np.abs(got[k] - ref64[k]).max())
        if err / d32 > worst[0]:
            worst = (err / d32, k, err, d32)
        if not err <= bound:
            bad.append(f"{sc.probe_name(k)}: {err:.3e} > {bound:.3e}")
    print(f"smpl probe {name}: worst ratio {worst[0]:.2f} at {sc.probe_name(worst[1])}: gpu error {worst[2]:.3e} d32 {worst[3]:.3e}")
    assert not bad, bad


@pytest.mark.parametrize("name,kind", [("dense", "noise"), ("chain", "euro"), ("tree", "ortho")])
def test_crop_independence(engines, cuda, name, kind):
    """A crop's result does not depend on its neighbours or on where it stands: bit for bit the same alone, in a batch of 130, and
    at a position in another wave (16 crops) of another block (64 crops)."""
    smpl, m = engines(name)
    betas, R = sc.inputs(name, kind)
    full = run(m, cuda, betas, R)
    for i in (0, 15, 16, 47, 48, 63, 64, 79, 80, 128, 129):
        alone = run(m, cuda, betas[i:i + 1], R[i:i + 1])
        assert np.array_equal(alone[0].view(np.uint32), full[i].view(np.uint32)), f"crop {i} alone"
    # position p of the second batch holds crop src[p]: the two full blocks change places with their waves moved on by one, and the
    # two crops of the third block (its wave 0) change places with one crop of wave 1 of either full block
    p = np.arange(sc.N_CROPS)
    src = np.where(p < 64, 64 + (p - 16) % 64, (p - 80) % 64)
    src[128], src[40] = src[40], 128
    src[129], src[104] = src[104], 129
    assert sorted(src.tolist()) == p.tolist() and (src // 64 != p // 64).all() and (src % 64 // 16 != p % 64 // 16).all()
    moved = run(m, cuda, betas[src], R[src])
    same = (moved.view(np.uint32) == full[src].view(np.uint32)).all(axis=(1, 2))
    assert same.all(), f"crops {src[~same].tolist()} differ at positions {p[~same].tolist()}"


@pytest.mark.parametrize("name", ["dense", "chain"])
def test_forward_path(engines, cuda, name):
    """forward() runs the same three kernels on strided betas / rotations inside the engine and writes joints49_out: bit for bit
    poco_smpl_lbs on the pose and shape it returns."""
    from poco_amd import synth
    smpl, m = engines(name)
    out = m(util.cuda_batch(synth.synth_batch(5, 4321), cuda))
    torch.cuda.synchronize()
    m.check_status()
    shape, pose = out["pred_shape"].clone(), out["pred_pose"].clone()
    fv, fj = out["smpl_vertices"].clone(), out["smpl_joints3d"].clone()
    v, j = m.smpl_lbs(shape, pose)
    torch.cuda.synchronize()
    assert torch.isfinite(fv).all() and float((fv[0] - fv[1]).abs().max()) > 1e-3        # five different bodies
    assert torch.equal(fv.view(torch.int32), v.view(torch.int32)), float((fv - v).abs().max())
    assert torch.equal(fj.view(torch.int32), j.view(torch.int32)), float((fj - j).abs().max())
    # and the forward's bodies are this model's, not the standard one's
    ref64, ref32 = sc.lbs_pair(smpl, shape.cpu().numpy(), pose.cpu().numpy())
    bound, d32 = sc.tolerance(ref64, ref32)
    err = float(np.abs(torch.cat([fv, fj], 1).cpu().numpy() - ref64).max())
    print(f"smpl forward {name}: gpu error {err:.3e} d32 {d32:.3e} ratio {err / d32:.2f} bound {bound:.3e}")
    assert err <= bound
