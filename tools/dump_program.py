"""Print the engine's op program as text (no GPU needed): for every variant and every A/B option string, the declared
tensors, every op with its schedule, geometry and default conv configurations, and which configurations of the tuned
table poco_set_conv_cfg accepts for every conv op.

    python tools/dump_program.py > program.txt

A change that must leave the program as it is (a refactor of the builder) produces a byte-identical listing before and
after.  Uses only the declare-mode C ABI, so it runs against any build of the library (POCO_HIP_LIB selects another).
"""
from __future__ import annotations

import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from poco_amd import tune  # noqa: E402
from poco_amd.model import POCO  # noqa: E402

VARIANTS = {"hrnet_w32-pare": 3, "hrnet_w48_cls-cliff": 1, "resnet50-cliff": 1}
OPTIONS = ("", "kcat=0", "kmerge=0", "chain=0", "dual=0", "xdep=0", "tail_lanes=0", "up_lanes=0", "mlp_fuse=0", "wg_fuse=0",
           "seq_phases=255", "w4_min_plane=14", "wg_max_plane=1", "branch_lanes=0000")
MATRIX_OPTIONS = ("", "w4_min_plane=14", "wg_max_plane=1")
BATCHES = (1, 16, 64, 128)
MATRIX_BATCHES = (1, 64)
ALG7_CFG = (4, 2, 2, 4, 4, 1, 7)          # the table holds no ALG 7 entry: one by hand (conv_wino4.hip w4geo)


def engine(variant: str, options: str) -> POCO:
    return POCO(backbone=variant, num_flow_layers=VARIANTS[variant], max_batch=128, engine_options=options)


def table_cfgs() -> list:
    cfgs = sorted({tuple(v["cfg"]) for v in json.loads(tune.TABLE.read_text()).values()})
    return cfgs + [ALG7_CFG]


def default_cfg(m: POCO, i: int, B: int) -> tuple:
    c = (C.c_int * 7)()
    rc = m._L.poco_get_conv_cfg(m._h, i, B, c)       # the C function itself: model.conv_cfg would apply the tuned table first
    return tuple(c) if rc == 0 else ("rc", rc)


def dump_listing(variant: str, options: str, out) -> None:
    m = engine(variant, options)
    tensors, ops = m.expected_tensors(), m.ops()
    out.write(f"== {variant} [{options}]: {len(tensors)} tensors, {len(ops)} ops\n")
    for name, shape, req in tensors:
        out.write(f"T {name} {list(shape)} {int(req)}\n")
    for i, (name, flops, ty) in enumerate(ops):
        desc = m.conv_desc(i)
        out.write(f"O {i} {name} type={ty} flops={flops!r} sched={m.op_sched(i)} desc={desc}")
        if desc is not None:
            out.write(" cfg=" + " ".join(f"{B}:{default_cfg(m, i, B)}" for B in BATCHES))
        out.write("\n")


def dump_matrix(variant: str, options: str, cfgs: list, out) -> None:
    m = engine(variant, options)
    conv = [i for i in range(len(m.ops())) if m.conv_desc(i) is not None]
    out.write(f"== accept {variant} [{options}]: {len(conv)} conv ops x {len(cfgs)} configurations\n")
    arrs = [(C.c_int * 7)(*c) for c in cfgs]
    accepted = 0
    for i in conv:
        for B in MATRIX_BATCHES:
            rcs = "".join(str(m._L.poco_set_conv_cfg(m._h, i, B, a)) for a in arrs)
            accepted += rcs.count("0")
            out.write(f"A {i} B={B} {rcs}\n")
    out.write(f"accepted {accepted} of {len(conv) * len(MATRIX_BATCHES) * len(cfgs)}\n")


def main() -> None:
    out = sys.stdout
    cfgs = table_cfgs()
    out.write(f"configurations: {len(cfgs)}\n")
    for k, c in enumerate(cfgs):
        out.write(f"C {k} {list(c)}\n")
    for variant in VARIANTS:
        for options in OPTIONS:
            dump_listing(variant, options, out)
        for options in MATRIX_OPTIONS:
            dump_matrix(variant, options, cfgs, out)


if __name__ == "__main__":
    main()
