"""The material of tests/smpl_cases.py holds every case it claims, and each kernel fault it is built for moves the float64 result
(oracle/smpl_np.smpl_lbs_np, the reference of tests/test_smpl_kernels_gpu.py) by at least ten times that file's tolerance - while
the first two faults leave the material of test_model_gpu.py::test_smpl_lbs_op (synth.synth_smpl(7), the standard map) untouched:
the gap these models close was real.  No GPU."""
import numpy as np
import pytest

from oracle.smpl_np import smpl_lbs_np
from poco_amd import synth
from tests import smpl_cases as sc

N = 6                                    # crops per check: the faults are per-crop properties


@pytest.fixture(scope="module")
def models():
    return {name: sc.build_model(name) for name in sc.MODELS}


def _cat(smpl, betas, R):
    v, j = smpl_lbs_np(smpl, betas, R)
    return np.concatenate([v, j], 1)


_cache = {}


def _reference(models, name, kind):
    """(betas, R, float64 result, tolerance) of the first N crops of an input set - computed once"""
    if (name, kind) not in _cache:
        betas, R = sc.column_probe() if kind == "probe" else sc.inputs(name, kind, N)
        ref64, ref32 = sc.lbs_pair(models[name], betas, R)
        _cache[name, kind] = (betas, R, ref64, sc.tolerance(ref64, ref32)[0], ref32)
    return _cache[name, kind][:4]


def test_maps_cover_all_sources(models):
    a, b = models["dense"]["joint_map"], models["chain"]["joint_map"]
    assert a.shape == b.shape == (49,)
    assert set(a.tolist()) | set(b.tolist()) == set(range(54))
    for m in (a, b):                                                  # both keep repeats, as the standard map does
        assert len(set(m.tolist())) < 49
    assert set(sc.UNREAD_CHAIN) | set(sc.UNREAD_PICKS) == set(range(45)) - set(synth.JOINT_MAP_49.tolist())
    assert np.array_equal(models["tree"]["joint_map"], synth.JOINT_MAP_49[::-1])
    # the reading order is not the source order: a map applied as its own inverse, or sorted, differs
    assert not np.array_equal(a, np.sort(a)) and not np.array_equal(b, np.sort(b))


def test_dense_model_material(models):
    m = models["dense"]
    je, jr, w = m["J_regressor_extra"], m["J_regressor"], m["lbs_weights"]
    assert (je[:, sc.V - 1] > 0).all()
    assert (je[:, list(sc.JRE_FIXED)] > 0).all()
    assert (je[:, 6144:].sum(1) >= 0.5 * je.sum(1)).all()
    assert (jr[:, sc.V - 1] > 0).sum() >= 4
    nnz = (w != 0).sum(1)
    one_hot = np.flatnonzero(nnz == 1)
    assert len(one_hot) == 64 and set(sc.ONE_HOT_FIXED) <= set(one_hot.tolist())
    assert (w[one_hot].max(1) == 1.0).all()
    assert len(set(w[one_hot].argmax(1).tolist())) == 24             # every joint, so every lane of the float4 loads, is the 1 once
    assert (nnz[np.setdiff1d(np.arange(sc.V), one_hot)] == 24).all()   # every other row is dense
    np.testing.assert_allclose(w.sum(1), 1.0, atol=1e-6)
    ids = m["extra_vertex_ids"]
    assert {0, 6889, 6880, 6879, 31, 32} <= set(ids.tolist()) and len(set(ids.tolist())) == 20 and ids.max() < sc.V
    assert float(np.abs(m["posedirs"]).std()) > 4.9 * float(np.abs(synth.synth_smpl(7)["posedirs"]).std())
    for name in sc.MODELS:
        assert set(models[name]) == set(synth.synth_smpl(7)) and models[name]["v_template"].shape == (sc.V, 3)


def test_trees(models):
    for name in sc.MODELS:
        p = [int(x) for x in models[name]["parents"]]
        assert all(0 <= p[i] < i for i in range(1, 24)), name
    assert np.array_equal(models["dense"]["parents"], synth.SMPL_PARENTS)
    assert [int(x) for x in models["chain"]["parents"][1:]] == list(range(23))
    assert int(models["tree"]["parents"][0]) == 4294967295
    tree = [int(x) for x in models["tree"]["parents"][1:]]
    assert tree != list(range(23)) and tree != synth.SMPL_PARENTS[1:].tolist()
    differs = sum(a != b for a, b in zip(tree, synth.SMPL_PARENTS[1:].tolist()))
    assert differs >= 12                                              # most joints hang elsewhere than in the standard tree


def test_inputs(models):
    for kind in ("ortho", "bigbeta"):
        betas, R = sc.inputs("dense", kind, N)
        assert np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max() < 1e-5 and np.allclose(np.linalg.det(R), 1.0, atol=1e-5)
    assert np.abs(betas).max() == 5.0
    for kind in ("euro", "blend", "noise"):
        _, R = sc.inputs("dense", kind, N)
        assert np.abs(np.swapaxes(R[1:], -1, -2) @ R[1:] - np.eye(3)).max() > 0.05, kind
    betas, R = sc.column_probe()
    assert betas.shape == (217, 10) and R.shape == (217, 24, 3, 3)
    coef = np.concatenate([(R[:, 1:] - np.eye(3, dtype=np.float32)).reshape(217, 207), betas], 1)
    assert np.array_equal(coef, np.eye(217, dtype=np.float32))        # crop k raises the coefficient of K row k alone
    assert "noise" not in sc.KINDS["chain"] and set(sc.KINDS) == set(sc.MODELS)


@pytest.mark.parametrize("kind", sc.KINDS["dense"])
def test_fault_keep_dropped(models, kind):
    betas, R, ref, tol = _reference(models, "dense", kind)
    moved = np.abs(_cat(sc.fault_keep(models["dense"]), betas, R) - ref).max(axis=(1, 2))
    assert moved.min() >= 10 * tol, (moved.min(), tol)


@pytest.mark.parametrize("kind", sc.KINDS["dense"])
def test_fault_extra_ids_rotated(models, kind):
    betas, R, ref, tol = _reference(models, "dense", kind)
    moved = np.abs(_cat(sc.fault_extra_ids(models["dense"]), betas, R) - ref).max(axis=(1, 2))
    assert moved.min() >= 10 * tol, (moved.min(), tol)


def test_first_two_faults_are_invisible_on_the_old_material():
    """synth.synth_smpl(7) with orthonormal rotations and N(0, 1) betas, as test_smpl_lbs_op runs it"""
    old = synth.synth_smpl(7)
    r = np.random.default_rng(5)
    betas = r.standard_normal((N, 10)).astype(np.float32)
    R = sc.random_rotations(r, (N, 24)).astype(np.float32)
    ref64, ref32 = sc.lbs_pair(old, betas, R)
    tol = sc.tolerance(ref64, ref32)[0]
    assert 0 < tol <= 2e-5
    for fault in (sc.fault_keep, sc.fault_extra_ids):
        assert np.abs(_cat(fault(old), betas, R) - ref64).max() < tol, fault.__name__
    assert (old["J_regressor_extra"][:, sc.V - 1] == 0).all()


@pytest.mark.parametrize("name,kind", [(n, k) for n in ("chain", "tree") for k in sc.KINDS[n]])
def test_fault_standard_tree(models, name, kind):
    betas, R, ref, tol = _reference(models, name, kind)
    moved = np.abs(_cat(sc.fault_tree(models[name]), betas, R) - ref).max(axis=(1, 2))
    assert moved.min() >= 10 * tol, (moved.min(), tol)


@pytest.mark.parametrize("k1,k2", [(17, 18), (100, 163), (0, 206)])
@pytest.mark.parametrize("kind", sc.KINDS["dense"])
def test_fault_k_rows_swapped(models, kind, k1, k2):
    betas, R, ref, tol = _reference(models, "dense", kind)
    moved = np.abs(_cat(sc.fault_swap_k(models["dense"], k1, k2), betas, R) - ref).max(axis=(1, 2))
    assert moved.min() >= 10 * tol, (moved.min(), tol)


def test_column_probe_names_the_swapped_rows(models):
    """In the probe a swap of two K rows shows in exactly the two crops that carry them."""
    betas, R, ref, _ = _reference(models, "dense", "probe")
    ref32 = _cache["dense", "probe"][4]
    k1, k2 = 100, 163
    moved = np.abs(_cat(sc.fault_swap_k(models["dense"], k1, k2), betas, R) - ref).max(axis=(1, 2))
    for k in range(sc.N_PROBE):
        tol = sc.tolerance(ref[k], ref32[k])[0]
        assert tol > 0
        assert (moved[k] >= 10 * tol) if k in (k1, k2) else (moved[k] == 0.0), sc.probe_name(k)


@pytest.mark.parametrize("joint", [0, 7, 23])
@pytest.mark.parametrize("name,kind", [(n, k) for n in sc.MODELS for k in sc.KINDS[n]])
def test_fault_rotation_transposed(models, name, kind, joint):
    betas, R, ref, tol = _reference(models, name, kind)
    moved = np.abs(_cat(models[name], betas, sc.fault_transpose(R, joint)) - ref).max(axis=(1, 2))
    assert moved.min() >= 10 * tol, (moved.min(), tol)
