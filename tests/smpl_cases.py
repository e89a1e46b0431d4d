"""Adversarial body models and inputs for the SMPL kernels (poco_amd/csrc/kernels_smpl.hip), numpy only.

tests/test_model_gpu.py::test_smpl_lbs_op runs one body model, synth.synth_smpl(7): the standard joint tree, four skinning weights
per vertex, a 49-joint map that reads 25 of the 54 joint sources, an extra-joint regressor that does not touch the last vertex, and
orthonormal rotations only.  The models here hold what that one leaves out; tests/test_smpl_cases_cpu.py proves in float64 that a
kernel fault of each kind moves their results by far more than the tolerance, tests/test_smpl_kernels_gpu.py runs them on the GPU.

The engine fixes V = 6890, so every model has the full mesh.
"""
import numpy as np

from poco_amd import synth
from poco_amd.smooth import one_euro_rotmats

V = synth.NUM_VERTS
MODELS = ("dense", "chain", "tree")
N_CROPS = 130                                           # crops per input set = the engines' max_batch
BATCHES = (1, 15, 16, 17, 48, 49, 63, 64, 65, 129, 130)  # wave boundaries (16 crops) and block boundaries (64 crops) of the skin kernel
ONE_HOT_FIXED = (0, 31, 32, 6879, 6880, 6889)           # first / last vertex, both sides of a 32-vertex block edge
JRE_FIXED = (1023, 1024, 6143, 6144, 6889)              # both sides of a 1024-vertex round edge of the joints kernel, the last vertex
TAIL_LANES = 7 * 1024 - V                               # lanes of the joints kernel's seventh round that lie past the last vertex
KINDS = {"dense": ("ortho", "bigbeta", "euro", "blend", "noise"),
         "chain": ("ortho", "bigbeta", "euro", "blend"),    # no I + noise on a depth-23 chain: 23 non-contractive factors only blow up
         "tree": ("ortho", "bigbeta", "euro", "blend", "noise")}

# Joint sources: 0..23 chain joints, 24..44 vertex picks (extra_vertex_ids[0..20]), 45..53 regressed joints.
# The standard map (synth.JOINT_MAP_49) never reads these:
UNREAD_CHAIN = (3, 6, 9, 10, 11, 13, 14, 15, 22, 23)
UNREAD_PICKS = tuple(range(35, 45))


def _shuffled(items, seed):
    a = np.array(items, np.int32)
    assert a.shape == (49,)
    return a[np.random.default_rng(seed).permutation(49)]


# map A: everything the standard map skips, all nine regressed joints, the picks it does read, and six repeats
JOINT_MAP_A = _shuffled(UNREAD_CHAIN + UNREAD_PICKS + tuple(range(45, 54)) + tuple(range(24, 35)) + (0, 1, 2)
                        + (23, 44, 53, 3, 35, 45), 101)
# map B: every chain joint, every pick, and four repeats
JOINT_MAP_B = _shuffled(tuple(range(24)) + tuple(range(44, 23, -1)) + (53, 45, 0, 44), 102)
# map C: the standard map read backwards
JOINT_MAP_C = synth.JOINT_MAP_49[::-1].copy()


def model_dense(seed=21):
    """M1: standard tree; dense skinning weights with 64 rigid (one-hot) vertices; both regressors touch the last vertex; five times
    the pose blend shapes; vertex picks at the mesh's and the blocks' edges with one id twice; map A."""
    r = np.random.default_rng(seed)
    m = synth.synth_smpl(seed)
    m["posedirs"] = (0.01 * r.standard_normal((207, V * 3))).astype(np.float32)
    w = r.dirichlet(np.ones(24), V)
    rigid = list(ONE_HOT_FIXED) + list(r.choice(np.setdiff1d(np.arange(V), ONE_HOT_FIXED), 64 - len(ONE_HOT_FIXED), replace=False))
    for n, v in enumerate(rigid):
        w[v] = 0.0
        w[v, (5 * n + 3) % 24] = 1.0                     # walks over all 24 joints, i.e. every slot of the six float4 loads
    m["lbs_weights"] = w.astype(np.float32)
    je = np.zeros((9, V))
    for j in range(9):
        lo = np.concatenate([JRE_FIXED[:3], r.choice(np.setdiff1d(np.arange(6143), JRE_FIXED), 4, replace=False)])
        hi = np.concatenate([JRE_FIXED[3:], 6145 + r.choice(V - 1 - 6145, 7, replace=False)])
        je[j, lo] = 0.4 * r.dirichlet(np.full(len(lo), 4.0))
        je[j, hi] = 0.6 * r.dirichlet(np.full(len(hi), 4.0))     # 60 % of the row on vertices >= 6144: the seventh round
    m["J_regressor_extra"] = je.astype(np.float32)
    jr = m["J_regressor"].astype(np.float64)
    for j in (0, 5, 11, 23):
        jr[j] *= 0.75
        jr[j, V - 1] += 0.25
    m["J_regressor"] = jr.astype(np.float32)
    ids = np.concatenate([[0, 6889, 6880, 6879, 31, 32, 6880], r.choice(V, 14, replace=False)])   # 6880 twice
    m["extra_vertex_ids"] = ids.astype(np.int32)
    m["joint_map"] = JOINT_MAP_A.copy()
    return m


def model_chain(seed=22):
    """M2: one chain of depth 23, parents[i] = i - 1; sparse weights as synth.synth_smpl; map B."""
    m = synth.synth_smpl(seed)
    m["parents"] = np.arange(-1, 23, dtype=np.int32)
    m["joint_map"] = JOINT_MAP_B.copy()
    return m


def model_tree(seed=23):
    """M3: a random tree, parents[i] drawn from [0, i); the root entry is the uint32 -1 of an SMPL pickle; map C."""
    r = np.random.default_rng(seed)
    m = synth.synth_smpl(seed)
    p = np.zeros(24, np.int64)
    p[0] = 4294967295
    for i in range(1, 24):
        p[i] = r.integers(0, i)
    m["parents"] = p
    m["joint_map"] = JOINT_MAP_C.copy()
    return m


BUILDERS = {"dense": model_dense, "chain": model_chain, "tree": model_tree}


def build_model(name):
    return BUILDERS[name]()


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def random_rotations(r, shape):
    """Haar-distributed rotation matrices [*shape, 3, 3], float64."""
    q, t = np.linalg.qr(r.standard_normal(tuple(shape) + (3, 3)))
    q = q * np.sign(np.diagonal(t, axis1=-2, axis2=-1))[..., None, :]
    q[..., :, 2] *= np.linalg.det(q)[..., None]
    return q


def _rodrigues(aa):
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    k = aa / np.maximum(np.linalg.norm(aa, axis=-1, keepdims=True), 1e-12)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def rotation_track(r, T, step=0.25):
    """A random walk over rotations: [T, 24, 3, 3], each frame the previous one times a rotation by up to ~`step` rad per axis."""
    out = np.empty((T, 24, 3, 3))
    out[0] = random_rotations(r, (24,))
    for t in range(1, T):
        out[t] = out[t - 1] @ _rodrigues(step * r.standard_normal((24, 3)))
    return out


def _seed(model, kind):
    return [MODELS.index(model), sum(map(ord, kind)), 77]


def inputs(model, kind, n=N_CROPS):
    """(betas [n, 10], rotmat [n, 24, 3, 3]) float32 for one input kind:
      ortho    orthonormal rotations, betas ~ N(0, 1)
      bigbeta  orthonormal rotations, betas uniform in [-5, 5] with every tenth entry exactly +-5
      euro     the One-Euro filter's output (poco_amd.smooth.one_euro_rotmats) on a random rotation track: what --smooth feeds
      blend    t R1 + (1 - t) R2 per joint, t ~ U(0, 1)
      noise    I + 0.3 N(0, 1)
      identity identity pose, zero betas"""
    r = np.random.default_rng(_seed(model, kind))
    betas = r.standard_normal((n, 10))
    if kind == "ortho":
        R = random_rotations(r, (n, 24))
    elif kind == "bigbeta":
        R = random_rotations(r, (n, 24))
        betas = r.uniform(-5.0, 5.0, (n, 10))
        flat = betas.reshape(-1)
        flat[::10] = np.where(flat[::10] < 0, -5.0, 5.0)
    elif kind == "euro":
        R = one_euro_rotmats(rotation_track(r, n).astype(np.float32))
    elif kind == "blend":
        t = r.uniform(0.0, 1.0, (n, 24, 1, 1))
        R = t * random_rotations(r, (n, 24)) + (1.0 - t) * random_rotations(r, (n, 24))
    elif kind == "noise":
        R = np.eye(3) + 0.3 * r.standard_normal((n, 24, 3, 3))
    elif kind == "identity":
        R = np.broadcast_to(np.eye(3), (n, 24, 3, 3))
        betas = np.zeros((n, 10))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(betas, np.float32), np.ascontiguousarray(R, np.float32)


N_PROBE = 217


def probe_name(k):
    """What crop k of the column probe isolates, in the blend GEMM's K order (207 pose rows | 10 shape rows)."""
    return f"K row {k} (joint {1 + k // 9}, rotation entry {k % 9})" if k < 207 else f"K row {k} (beta {k - 207})"


def column_probe():
    """217 crops, each with one coefficient of the blend GEMM raised by one: crop k < 207 has rotmat = I except that entry k % 9 of
    joint 1 + k // 9 gets +1; crops 207..216 have one-hot betas."""
    betas = np.zeros((N_PROBE, 10), np.float32)
    R = np.tile(np.eye(3, dtype=np.float32), (N_PROBE, 24, 1, 1))
    for k in range(207):
        R[k, 1 + k // 9, (k % 9) // 3, (k % 9) % 3] += 1.0
    betas[np.arange(207, 217), np.arange(10)] = 1.0
    return betas, R


# ---- the comparison rule ------------------------------------------------------------------------------------------------------
def lbs_pair(smpl, betas, R):
    """(float64 result, float32 restatement), each verts [B, V, 3] and joints [B, 49, 3] laid side by side as [B, V + 49, 3]."""
    from oracle.smpl_np import smpl_lbs_np
    v64, j64 = smpl_lbs_np(smpl, betas, R)
    v32, j32 = smpl_lbs_np(smpl, betas, R, dtype=np.float32)
    assert v32.dtype == np.float32 and j32.dtype == np.float32
    return np.concatenate([v64, j64], 1), np.concatenate([v32, j32], 1).astype(np.float64)


def tolerance(ref64, ref32):
    """(bound, d32) for a set of crops.  d32 = max |float32 restatement - float64| is what float32 rounding does to these sums in
    one summation order; another order of the same float32 arithmetic gets 8 x that (the margin of tests/test_eval_gpu.py tol()),
    capped at 1e-3 of the values' size so that a degenerate d32 cannot hide a failure."""
    d32 = float(np.abs(ref32 - ref64).max())
    return min(8.0 * d32, 1e-3 * max(1.0, float(np.abs(ref64).max()))), d32


# ---- kernel faults, stated on the reference's operands --------------------------------------------------------------------------
def fault_keep(smpl):
    """smpl_joints_kernel without `keep`: the 278 tail lanes of the seventh round add the last vertex again."""
    m = dict(smpl)
    je = m["J_regressor_extra"].astype(np.float64)
    je[:, V - 1] *= 1 + TAIL_LANES
    m["J_regressor_extra"] = je
    return m


def fault_extra_ids(smpl):
    """extra_vertex_ids[11..20] rotated by one: an offset error behind the picks the standard map reads."""
    m = dict(smpl)
    ids = np.array(m["extra_vertex_ids"])
    ids[11:21] = np.roll(ids[11:21], 1)
    m["extra_vertex_ids"] = ids
    return m


def fault_tree(smpl):
    """the standard tree hard-coded in place of the loaded one"""
    m = dict(smpl)
    m["parents"] = synth.SMPL_PARENTS.copy()
    return m


def fault_swap_k(smpl, k1, k2):
    """two pose rows of the blend GEMM's packed operand swapped"""
    m = dict(smpl)
    pd = np.array(m["posedirs"])
    pd[[k1, k2]] = pd[[k2, k1]]
    m["posedirs"] = pd
    return m


def fault_transpose(R, joint):
    """R^T in place of R for one joint: the shortcut R^-1 = R^T, or a row / column mix-up"""
    R = np.array(R)
    R[:, joint] = np.swapaxes(R[:, joint], -1, -2)
    return R
