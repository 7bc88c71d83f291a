#!/usr/bin/env python3
"""Device time per tick of supervised workers with and without restartWithBackoff at 2^20 actors,
from agx_run_timed: a warm-up engine first, then on a fresh engine one settling window and five measured windows of
`--ticks` ticks each; the median window and the windows, as JSON.

  python tools/backoff_cost.py flaky              # flaky_workers, jobs that keep circulating (any library: AKKA_AMD_LIB)
  python tools/backoff_cost.py flaky_unused       # ... with agx_set_backoff made, every row plain: the backoff instantiation, unused
  python tools/backoff_cost.py backoff_workers    # backoff_workers in steady churn: every client fails on every 13th job
"""
import argparse
import json
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

N = 1 << 20


def workload(case: str, ticks: int):
    from akka_amd import typed
    from akka_amd import workloads as wl
    total = ticks * 6 + 16
    if case == "backoff_workers":
        return wl.backoff_workers(N, jobs=2, hops=total, churn=12, bucket_actors=256)
    w = wl.flaky_workers(N, hops=total, max_poison=3)  # (within the limit of 3 restarts: nobody stops, no job dies)
    if case == "flaky_unused":
        w.supervision = dict(w.supervision, backoff=[[typed.AgxBackoff() for _ in r] for r in w.supervision["rows"]])
    return w


def windows(w, ticks: int, n_windows: int):
    from akka_amd.engine import EngineConfig, GpuEngine
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    out = []
    for _ in range(n_windows):
        st, ms = eng.run_timed(ticks)[:2]
        out.append(ms / ticks)
    info = dict(supervision=eng.supervision_info())
    if w.supervision.get("backoff"):
        info["backoff"] = eng.backoff_info()
    eng.close()
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["flaky", "flaky_unused", "backoff_workers"])
    ap.add_argument("--ticks", type=int, default=32)
    a = ap.parse_args()
    w = workload(a.case, a.ticks)
    windows(w, 4, 1)  # the warm-up engine
    ms, info = windows(w, a.ticks, 6)
    meas = ms[1:]  # (the first window settles: the poison, the first backoffs)
    print(json.dumps(dict(case=a.case, ticks=a.ticks, ms_per_tick_median=statistics.median(meas), windows=meas, settling=ms[0],
                          info=info)))


if __name__ == "__main__":
    main()
