r"""Records tests/golden/launch_trace.json: the launch traces of tests/launch_trace_cases.py from the library of an EARLIER commit
(never from the code under test).  Build that commit's library in a checkout of its own and run, on the GPU,

    BBHIP_LIBRARY=/path/to/that/libbbhip.so python tests/golden/make_launch_trace.py <that commit's hash>

Every scenario is recorded three times.  The engine names, the tree counts, the stop codes and the final counts must agree
across the three: a scenario where they do not is reported and not written (replace it).  Any other field that differs between
the three recordings is left out of that scenario's launches and named under "varies"."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import launch_trace_cases as L  # noqa: E402

HARD = ("engine", "trees", "stop")


def both_instances(tr) -> bool:
    stops = {la["stop"] for la in tr.get("launches", [])}
    return 11 in stops and 12 in stops


def main() -> int:
    assert os.environ.get("BBHIP_LIBRARY"), "BBHIP_LIBRARY must name the library of the commit that is recorded"
    out = dict(parent=sys.argv[1], fields=list(L.FIELDS), ml_rows=L.ML_CAP, scenarios={})
    first_ml = None
    for n in range(L.ML_STEP, L.ML_CAP + 1, L.ML_STEP):
        first_ml = L.trace("single_and_multi_level", n)
        if "error" in first_ml or both_instances(first_ml):
            out["ml_rows"] = n
            break
    if first_ml.get("returncode", 1) != 1:
        print(f"single_and_multi_level: ended with {first_ml['returncode']}: {first_ml['error'][-600:]}", flush=True)
        return 1
    print(f"single_and_multi_level: {out['ml_rows']} rows, both instances: {both_instances(first_ml)}", flush=True)
    bad = []
    for name in L.SCENARIOS:
        runs = []
        while len(runs) < 3 and not (runs and runs[-1].get("returncode", 1) != 1):
            runs.append(L.trace(name, out["ml_rows"]))
        errors = [r["error"] for r in runs if "error" in r]
        if any(r.get("returncode", 1) != 1 for r in runs):  # (not a Python exception: a crash - nothing more is started)
            print(f"{name}: a recording ended with {[r.get('returncode') for r in runs]}: {errors[0][-600:]}", flush=True)
            return 1
        if errors:
            print(f"{name}: FAILED in {len(errors)} of 3 recordings: {errors[0][-600:]}", flush=True)
            bad.append(name)
            continue
        a = runs[0]
        hard_ok = all(len(r["launches"]) == len(a["launches"]) and r["final"] == a["final"] and r["reports"] == a["reports"] and
                      all(x[k] == y[k] for x, y in zip(r["launches"], a["launches"]) for k in HARD) for r in runs[1:])
        if not hard_ok:
            print(f"{name}: engines / tree counts / stop codes / final counts differ between the recordings: NOT written", flush=True)
            for r in runs:
                print("   ", len(r["launches"]), [(la["engine"], la["elems"], la["stop"]) for la in r["launches"]][:40], r["final"], flush=True)
            bad.append(name)
            continue
        varies = sorted({k for r in runs[1:] for x, y in zip(r["launches"], a["launches"]) for k in L.FIELDS if x[k] != y[k]})
        out["scenarios"][name] = dict(varies=varies, launches=[[la[k] for k in L.FIELDS if k not in varies] for la in a["launches"]],
                                      reports=a["reports"], final=a["final"])
        print(f"{name}: {len(a['launches'])} launches, varies: {varies}", flush=True)
    path = Path(sys.argv[2]) if len(sys.argv) > 2 else Path(__file__).with_name("launch_trace.json")
    path.write_text(json.dumps(out, separators=(",", ":")) + "\n")
    print("not written:", bad, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
