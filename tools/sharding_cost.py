#!/usr/bin/env python3
"""Device time per tick of sharded entities at 2^20 ids, from agx_run_timed: a warm-up engine first,
then on a fresh engine one settling window and five measured windows of `--ticks` ticks each, the tick's host tells
staged before its run(1); the median window and the windows' range, as JSON.

  python tools/sharding_cost.py passivating             # passivating_entities, the receive-timeout engine (any library: AKKA_AMD_LIB)
  python tools/sharding_cost.py passivating_sharding    # ... with agx_set_sharding made over 256 further ids that never get mail
  python tools/sharding_cost.py sharded_entities        # sharded_entities in steady churn: starts, passivations, restarts
"""
import argparse
import json
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

N = 1 << 20


def workload(case: str, ticks: int):
    from akka_amd import workloads as wl
    total = ticks * 6 + 8
    if case == "sharded_entities":
        return wl.sharded_entities(N, idle=4, ticks=total)
    w = wl.passivating_entities(N, spread=total)
    if case == "passivating_sharding":  # an entity range behind the registered actors: no bucket but its own meets it
        first = w.n_actors
        w.n_actors += 256
        w.timers["receive_timeout"]["sharding"] = [(first, 256, w.ranges[0][2], 0, None, wl.PE_STOP << 24, 0, 0)]
    return w


def windows(w, ticks: int, n_windows: int):
    from akka_amd.engine import EngineConfig, GpuEngine
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    out, t = [], 0
    for _ in range(n_windows):
        ms = 0.0
        for _ in range(ticks):
            dst, src, pay = w.schedule[t]
            eng.tell(dst, pay, src)
            ms += eng.run_timed(1)[1]
            t += 1
        out.append(ms / ticks)
    sharded = bool(w.timers["receive_timeout"].get("sharding"))
    info = dict(receive_timeout=eng.receive_timeout_info(), sharding=eng.sharding_info() if sharded else None)
    eng.close()
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["passivating", "passivating_sharding", "sharded_entities"])
    ap.add_argument("--ticks", type=int, default=32)
    a = ap.parse_args()
    w = workload(a.case, a.ticks)
    windows(w, 4, 1)  # the warm-up engine
    ms, info = windows(w, a.ticks, 6)
    meas = ms[1:]  # (the first window settles)
    print(json.dumps(dict(case=a.case, ticks=a.ticks, ms_per_tick_median=statistics.median(meas), windows=meas, settling=ms[0],
                          info=info)))


if __name__ == "__main__":
    main()
