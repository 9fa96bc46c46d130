r"""Scenarios of the tree launch loop (run_insert_multi, bblean_amd/csrc/bb_tree.hip), as data: the smallest inputs that reach
each of its branches - which engine takes a launch, how many elements it is given, why it stopped, what the host grew.  One
scenario runs in one fresh process (`python launch_trace_cases.py NAME`: the switches are read once per process) with
BBHIP_LAUNCH_LOG=1; `trace()` does that and parses the `[bbhip launch]` lines.  tests/golden/make_launch_trace.py records them
from the library of an earlier commit, tests/test_hip_launch_trace.py holds the present library against the recording."""
from __future__ import annotations

import ctypes as C
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
F = 2048
CONCURRENT_SIZES, CONCURRENT_KINDS = [30_000, 12_000, 40_000, 9_000, 45_000], [0, 4, 4, 2, 1]  # test_pipe_concurrent_trees_vs_oracle, tiny
SYS_ROWS = ("workload", "zipf", 20_000, 31)

# name -> (environment, trees as (branching factor, criterion, features), rows, how they are passed)
#   rows: ("workload", name of bench.WORKLOADS, n, seed) | ("segment", kind, n, seed) | ("near", n) | ("table", ...) | ("shards", bf)
SCENARIOS: dict[str, tuple[dict, tuple, tuple, str]] = {
    "first_stretch_then_pipeline": ({}, (50, "diameter", F), ("workload", "fake", 20_000, 11), "device"),
    "tiny_pools": ({"BBHIP_TINY_POOLS": "1"}, (50, "diameter", F), ("workload", "fake", 12_000, 11), "device"),
    "pipe_unsupported_stretches": ({}, (254, "tolerance-diameter", F), ("segment", 4, 30_000, 254), "device"),
    "single_and_multi_level": ({}, (50, "diameter", F), ("workload", "fake", 0, 5001), "device"),  # (n: ML_ROWS)
    "complete_engine": ({}, (7, "diameter", 64), ("near", 3_000), "device"),
    "more_trees_than_cus": ({}, (10, "diameter", 128), ("near", 200), "trees300"),
    "misaligned_rows": ({}, (50, "diameter", F), ("misaligned",), "offset1"),
    "buffers_singleton_runs": ({}, (6, "diameter", 64), ("table", "mixed"), "buffers"),
    "buffers_no_singleton_path": ({"BBHIP_NO_SINGLETON_PATH": "1"}, (6, "diameter", 64), ("table", "mixed"), "buffers"),
    "buffers_uint16": ({}, (5, "diameter", 64), ("table", 2), "buffers"),
    "concurrent_254": ({}, (254, "diameter", F), ("shards", 254), "trees"),
    "concurrent_254_no_pipe_multi": ({"BBHIP_NO_PIPE_MULTI": "1"}, (254, "diameter", F), ("shards", 254), "trees"),
    "concurrent_50": ({}, (50, "diameter", F), ("shards", 50), "trees"),
    "sys_forced_50": ({"BBHIP_SYS": "1"}, (50, "diameter", F), SYS_ROWS, "device"),
    "sys_forced_254": ({"BBHIP_SYS": "1"}, (254, "diameter", F), SYS_ROWS, "device"),
    "sys_auto_50": ({"BBHIP_SYS": "auto"}, (50, "diameter", F), SYS_ROWS, "device"),
    "sys_auto_254": ({"BBHIP_SYS": "auto"}, (254, "diameter", F), SYS_ROWS, "device"),
}
SWITCHES = ("BBHIP_NO_PIPE", "BBHIP_NO_FAST", "BBHIP_NO_FIXED_SHAPE", "BBHIP_PHASES", "BBHIP_PIPE_PHASES", "BBHIP_PIPE_AUDIT")
for _sw in SWITCHES:
    SCENARIOS["first_stretch_" + _sw[6:].lower()] = ({_sw: "1"},) + SCENARIOS["first_stretch_then_pipeline"][1:]
# the rows of "single_and_multi_level": the smallest multiple of 20 000 (up to 400 000, the size of
# test_pipe_moves_between_single_and_multi_level_instances) at which the recorded trace shows both stop=11 and stop=12
ML_STEP, ML_CAP = 20_000, 400_000
# lines bbh_tree_stats prints under these switches: their beginnings are compared, their numbers (cycle counts) are not
REPORT_PREFIX = re.compile(r"^(\[bbhip [a-z0-9 ,/+-]+\])")
LAUNCH = re.compile(r"^\[bbhip launch\] (\S+) trees=(\d+) (\S+) crit=(\d+) elems=(\d+) \S+ ms \(\S+ us/elem\) calls=(\d+) rows=(\d+) merges=(\d+) "
                    r"appends=(\d+) leaf_splits=(\d+) node_splits=(\d+) stop=(\d+)$")
FIELDS = ("engine", "trees", "kind", "crit", "elems", "calls", "rows", "merges", "appends", "leaf_splits", "node_splits", "stop")
CRIT = {"diameter": 0, "tolerance-diameter": 2}


def _rows(spec, n_override=0):
    import torch

    if spec[0] == "workload":
        from bench import WORKLOADS

        gen, thr, _ = WORKLOADS[spec[1]]
        return gen(n_override or spec[2], spec[3], torch.device("cuda")).cpu().numpy(), thr
    if spec[0] == "segment":
        from test_hip_pipe_fuzz import _segment

        return np.ascontiguousarray(_segment(np.random.default_rng(spec[3]), spec[2], spec[1])), 0.45
    raise ValueError(spec)


def run_scenario(name: str, ml_rows: int = 0) -> dict:
    r"""Runs in the child process -> the final counters of the (first) tree."""
    import torch

    import tree_abi_cases as T
    from test_hip_tree_abi_edges import SENT8, Raw, at, dev, ok
    from bblean_amd import _lib

    lib = _lib.load()
    _, (bf, crit, feats), spec, how = SCENARIOS[name]
    if how in ("trees", "trees300"):
        if how == "trees":
            from test_hip_pipe_fuzz import _segment

            rng = np.random.default_rng(4242 + spec[1])
            shards = [np.ascontiguousarray(_segment(rng, m, k)) for m, k in zip(CONCURRENT_SIZES, CONCURRENT_KINDS)]
            thr = 0.45
        else:
            shards, thr = [T.rows_near(900 + i, spec[1], feats) for i in range(300)], 0.5
        engines = [Raw(lib, torch, T.cfg(bf, thr, feats, CRIT[crit])) for _ in shards]
        src = [dev(torch, s) for s in shards]
        outs = [torch.zeros(s.shape[0], dtype=torch.int32, device="cuda") for s in shards]
        n = len(shards)
        handles = (C.c_void_p * n)(*[e.h.value for e in engines])
        a_in, a_out = (C.c_void_p * n)(*[at(s) for s in src]), (C.c_void_p * n)(*[at(o) for o in outs])
        a_n, a_stride = (C.c_int64 * n)(*[s.shape[0] for s in shards]), (C.c_int64 * n)(*[feats // 8] * n)
        ok(lib, lib.bbh_trees_fit_packed(C.addressof(handles), n, C.addressof(a_in), C.addressof(a_n), C.addressof(a_stride), C.addressof(a_out), None))
        res = dict(kernel_counts=[e.kernel_counts() for e in engines[:5]], stats=[[int(v) for v in e.stats()] for e in engines[:5]])
        for e in engines:
            e.close()
        return res
    if how == "buffers":
        c = T.RUN_CFG if spec[1] == "mixed" else T.TIER_CFG
        eng = Raw(lib, torch, c, where="device", out="device")
        eng.fit_buffers(T.run_table("mixed") if spec[1] == "mixed" else T.tier_table(spec[1])[0])
    elif how == "offset1":
        rows, (off, stride) = T.misaligned_rows(), T.MISALIGNED[0]
        flat = torch.full((off + rows.shape[0] * stride,), SENT8, dtype=torch.uint8, device="cuda")
        view = flat[off:].as_strided(rows.shape, (stride, 1))
        view.copy_(dev(torch, rows))
        eng = Raw(lib, torch, T.MISALIGNED_CFG, out="device")
        eng._fit(lambda o: lib.bbh_tree_fit_packed(eng.h, view.data_ptr(), rows.shape[0], stride, o, None), rows.shape[0])
    else:
        rows, thr = (T.rows_near(77, spec[1], feats), 0.5) if spec[0] == "near" else _rows(spec, ml_rows)
        eng = Raw(lib, torch, T.cfg(bf, thr, feats, CRIT[crit]), where="device", out="device")
        eng.fit_packed(rows)
    res = dict(kernel_counts=eng.kernel_counts(), stats=[int(v) for v in eng.stats()])
    if name.startswith("sys_"):
        sc = np.zeros(8, np.uint64)
        ok(lib, lib.bbh_tree_sys_counts(eng.h, at(sc)))
        res["sys_counts"] = [int(sc[i]) for i in (0, 1, 2, 3, 7)]
    eng.close()
    return res


def no_out_leaf() -> dict:
    r"""Runs in the child process, under BBHIP_SYS=1: the rows of "sys_forced_50" into a tree without an out_leaf and into one
    with it -> launches of the systolic kernel on either; both trees' exports must be the oracle's."""
    import torch

    import tree_abi_cases as T
    from test_hip_tree_abi_edges import Raw, at, ok
    from bblean_amd import _lib

    lib = _lib.load()
    rows, thr = _rows(SYS_ROWS)
    c = T.cfg(50, thr, F)
    want = dict(T.replay(c, [("packed", rows)]), out_leaf=[])
    launches = []
    for out in (None, "device"):
        eng = Raw(lib, torch, c, where="device", out=out)
        eng.fit_packed(rows)
        T.same(dict(T.snapshot(eng), out_leaf=[]), want)
        sc = np.zeros(8, np.uint64)
        ok(lib, lib.bbh_tree_sys_counts(eng.h, at(sc)))
        launches.append(int(sc[1]))
        eng.close()
    return dict(sys_launches_without_out=launches[0], sys_launches_with_out=launches[1])


def child(args: list[str], extra_env: dict, timeout=300):
    env = {k: v for k, v in os.environ.items() if not (k.startswith("BBHIP_") and k != "BBHIP_LIBRARY")}
    env.update(extra_env, BBHIP_LAUNCH_LOG="1", PYTHONPATH=os.pathsep.join([str(REPO), str(REPO / "tests")]))
    return subprocess.run([sys.executable, str(Path(__file__).resolve())] + args, env=env, capture_output=True, text=True, timeout=timeout)


def trace(name: str, ml_rows: int = 0) -> dict:
    r"""The scenario in a fresh process -> {"launches": [one dict of FIELDS per launch], "reports": [...], "final": {...}}, or
    {"error": last lines of its stderr} if it failed."""
    done = child([name, str(ml_rows)], SCENARIOS[name][0])
    if done.returncode != 0:
        return {"error": done.stderr[-2000:], "returncode": done.returncode}
    launches, reports = [], []
    for line in done.stderr.splitlines():
        m = LAUNCH.match(line)
        if m:
            launches.append({k: (v if k in ("engine", "kind") else int(v)) for k, v in zip(FIELDS, m.groups())})
        elif line.startswith("[bbhip ") and not line.startswith("[bbhip launch]"):
            reports.append(REPORT_PREFIX.match(line).group(1) if REPORT_PREFIX.match(line) else line[:20])
    final = json.loads(done.stdout.strip().splitlines()[-1])
    return dict(launches=launches, reports=reports, final=final)


if __name__ == "__main__":
    print(json.dumps(no_out_leaf() if sys.argv[1] == "no_out_leaf" else run_scenario(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 0)))
